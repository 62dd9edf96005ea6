"""Regenerate tests/golden/*.npz from the UNMODIFIED reference, or check that they still come out as committed.

    python -m oracle.gen_golden                 # (re)writes every fixture into tests/golden/
    python -m oracle.gen_golden g10 t4          # only the fixtures whose names start with g10 or t4
    python -m oracle.gen_golden --check [NAME]  # regenerates into a temporary directory and compares with tests/golden/:
                                                # one line ``<fixture>: <key>: <what>`` per difference, exit status 1 if any

Test infrastructure, run by hand where the reference checkout is present (oracle/ref_harness.py locates it); no test
reads the reference.  A fixture's generator is the module named after its prefix: oracle/golden_g1_g8.py (numpy
backend), golden_t1_t5.py (torch forward), golden_s1.py (shadows), golden_g9_g11.py (image + depth gradients),
golden_n1.py (all four outputs' gradients), golden_c1_c2.py (camera gradients, descent), golden_v1.py (batched views),
golden_p1.py (splats).  Each holds its scenes, its kwargs, its extra keys and the record of what its fixtures pin.
"""
import argparse
import contextlib
import glob
import io
import os
import sys
import tempfile
import time

import numpy as np

from oracle import (golden_c1_c2, golden_g1_g8, golden_g9_g11, golden_n1, golden_p1, golden_s1, golden_t1_t5, golden_v1,
                    ref_harness as R)
from oracle.golden_io import diff_npz

FAMILIES = (golden_g1_g8, golden_t1_t5, golden_s1, golden_g9_g11, golden_n1, golden_c1_c2, golden_v1, golden_p1)


def check(tmp):
    """Difference lines between the fixtures just written into ``tmp`` and the committed ones they stand for."""
    committed = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(R.REPO, "tests", "golden", "*.npz")))
    lines = [f"{n}: (file): committed, but no generator writes it" for n in committed if R.wanted(n) and n not in R.WRITTEN]
    for n in R.WRITTEN:
        path = os.path.join(R.REPO, "tests", "golden", n + ".npz")
        if not os.path.exists(path):
            lines.append(f"{n}: (file): generated, but not committed")
            continue
        new, old = (np.load(p, allow_pickle=False) for p in (os.path.join(tmp, n + ".npz"), path))
        lines += [f"{n}: {key}: {what}" for key, what in diff_npz(old, new)]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("names", nargs="*", metavar="NAME", help="fixture name prefixes (default: all)")
    ap.add_argument("--check", action="store_true", help="compare with tests/golden/ instead of writing there")
    args = ap.parse_args()
    R.ONLY = args.names
    t0 = time.time()
    with tempfile.TemporaryDirectory() if args.check else contextlib.nullcontext() as tmp:
        if args.check:
            R.OUT = tmp
        with contextlib.redirect_stdout(io.StringIO() if args.check else sys.stdout):
            for fam in FAMILIES:
                fam.main()
        lines = check(tmp) if args.check else []
    print("\n".join(lines + [f"{len(R.WRITTEN)} fixtures {'checked' if args.check else 'generated'}, "
                             f"{len(lines)} differences, {time.time() - t0:.0f} s"]))
    return 1 if lines or not R.WRITTEN else 0


if __name__ == "__main__":
    sys.exit(main())
