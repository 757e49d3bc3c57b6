#!/usr/bin/env python3
"""Record tests/golden/edge_vectors.npz: what the REFERENCE'S OWN object code (oracle/_ref) answers for the edge-case
battery of tests/edge_cases.py, so that tests/test_edge_vectors.py and tests/test_gpu_edge_rays.py run where oracle/_ref
cannot be built.

Run where oracle/_ref is built (needs the reference tree):  python tests/golden/make_edge_vectors.py
Every vector comes from tests/test_edge_vectors.py::live_edge_vectors.  Results only: the inputs are stored as one sha256
over the pairs, the rays and the scene file (edge_cases.digest), which the tests recompute from edge_cases.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import test_edge_vectors as T  # noqa: E402
from oracle import ref_py as R  # noqa: E402


def main():
    for depth in T.DEPTHS + (4,):
        if not R.available(depth):
            raise SystemExit("oracle/_ref has no depth-%d build: run build() where the reference tree is present" % depth)
    out = T.live_edge_vectors()
    for k, v in sorted(out.items()):
        print(k, v.shape, v.dtype)
    np.savez_compressed(T.EDGE_VECTORS, **out)
    size = os.path.getsize(T.EDGE_VECTORS)
    print("wrote %s: %d entries, %d bytes" % (T.EDGE_VECTORS, len(out), size))
    assert size < 300 << 10, "the fixture must stay under 300 KB"


if __name__ == "__main__":
    main()
