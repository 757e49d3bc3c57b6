#!/usr/bin/env python3
"""Record tests/golden/ref_vectors.npz: what the REFERENCE'S OWN object code (oracle/_ref) returns for every
comparison of tests/test_oracle_vs_ref.py, so that those tests run where oracle/_ref cannot be built.

Run where oracle/_ref is built (needs the reference tree):  python tests/golden/make_ref_vectors.py
Every vector comes from the live functions of the test module.  Entries are "<key>/<name>"; an array larger than
DIGEST_ABOVE_BYTES is stored as "<key>/<name>#sha256" (digest of shape, dtype and bytes).  The golden frames
themselves are in frames.npz already: for those keys only the ray count is recorded.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import test_oracle_vs_ref as T  # noqa: E402
from oracle import ref_py as R  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key, depth, live in T.live_vectors(tmp):
            if not R.available(depth):
                raise SystemExit("oracle/_ref has no depth-%d build: run build() where the reference tree is present" % depth)
            got = live()
            if key.startswith("golden/"):
                got = {"rays": got["rays"]}
            for name, v in got.items():
                v = T.canon(v)
                if v.nbytes > T.DIGEST_ABOVE_BYTES:
                    out["%s/%s#sha256" % (key, name)] = T.digest(v)
                else:
                    out["%s/%s" % (key, name)] = v
            print(key, sorted(got))
    np.savez_compressed(T.REF_VECTORS, **out)
    print("wrote %s: %d entries, %d bytes" % (T.REF_VECTORS, len(out), os.path.getsize(T.REF_VECTORS)))


if __name__ == "__main__":
    main()
