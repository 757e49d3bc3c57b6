#!/usr/bin/env python3
"""Generate tests/golden/accumulate_refusals.json: what the probes p3d_debug_accumulate, p3d_debug_accumulate_moving and
p3d_debug_accumulate_variance answer to every request of their tests' refusal_cases() (and of accepted_cases(), where the
test file has them), on a machine without a device.

Run with the library of the commit whose answers are to be kept (needs no GPU and no oracle/_ref):
    python tests/golden/make_accumulate_refusals.py
The file in the repository was recorded at the last commit at which each of the three entries had an argument check of its
own (accumulate.hip, accumulate_motion.hip, accumulate_variance.hip); the one check that replaced them has to give the same
status and the same text for every request, the requests with two defects included: their text says which check came first.

accumulate_refusals.json   a list of {"entry", "case" (the name in refusal_cases()), "status", "text" (p3d_last_error())}.
                           An accepted request is recorded as the machine without a device answers it: -3, "no HIP device
                           visible" -- the probes look for a device only after every check has passed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import test_accumulate_host as TA  # noqa: E402
import test_accumulate_moving_host as TM  # noqa: E402
import test_accumulate_variance_host as TV  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P  # noqa: E402

OUT = os.path.join(HERE, "accumulate_refusals.json")


def main():
    L = P.lib()
    assert P.device_count() == 0, "record on a machine without a device: an accepted request would run"
    rows = []
    for entry, T in (("p3d_debug_accumulate", TA), ("p3d_debug_accumulate_moving", TM), ("p3d_debug_accumulate_variance", TV)):
        probe = getattr(L, entry)
        call = T.make_call(lambda *a: probe(0, *a))
        cases = [(name, change) for name, _, change in T.refusal_cases()] + list(getattr(T, "accepted_cases", lambda: [])())
        assert len({name for name, _ in cases}) == len(cases), "two cases of %s have one name" % entry
        for name, change in cases:
            rc = call(**change)
            rc = rc[0] if isinstance(rc, tuple) else rc        # the moving test's call() also says whether anything was written
            rows.append(dict(entry=entry, case=name, status=int(rc), text=L.p3d_last_error().decode()))
        print(entry, len(cases), "cases")
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
