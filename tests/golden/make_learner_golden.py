#!/usr/bin/env python3
"""Generate tests/golden/learner_*.npz by RUNNING THE REFERENCE's own ``update()`` of each learner in the build container.

    python tests/golden/make_learner_golden.py [case ...]

The reference is imported through oracle/ref_harness.py; nothing of it is copied, nothing is written into its tree, and the fixtures
are data only.  The machinery, the cases and the layout of a fixture are oracle/learner_golden.py's; what a case's data must exercise
is asserted by ``tests/learner_golden.py: conditions`` before the file is written (the first data seed that meets it is taken).
The same arrays give the same bytes.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import learner_golden as rec  # noqa: E402


def main(cases):
    total = 0
    for case in cases or rec.CASES:
        arrays = rec.generate(case)
        rec.write_npz(rec.path(case), arrays)
        size = os.path.getsize(rec.path(case))
        total += size
        print("%-14s data seed %d, %d arrays, %d bytes" % (case, int(arrays["meta/data_seed"]), len(arrays), size))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main(sys.argv[1:])
