#!/usr/bin/env python3
"""Wall time of the spherical-harmonic synthesis (qf_shr2fun / qf_shc2fun) at a few bandwidths.

Each call is synchronous (the library synchronises its stream before it returns), so the time between two host clock
reads brackets one whole call: coefficient upload, the three kernels, the grid's copy back.  The per-kernel split comes
from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python3 tools/sht_time.py [L ...]          (default 1024 2048 8192)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import quflow_amd as qfa  # noqa: E402


def timed(fn, reps):
    fn()                                   # first call: context, scratch allocation
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    Ls = [int(a) for a in sys.argv[1:]] or [1024, 2048, 8192]
    for L in Ls:
        rng = np.random.default_rng(L)
        omr = rng.standard_normal(L * L)
        omc = qfa.shr2shc(omr)
        reps = 5 if L <= 2048 else 2
        row = {"L": L,
               "shr2fun_ms": timed(lambda: qfa.shr2fun(omr), reps),
               "shc2fun_complex_ms": timed(lambda: qfa.shc2fun(omc, isreal=False), reps),
               "grid_MB_real": L * (2 * L - 1) * 8 / 1e6,
               "fourier_gflop_real": 8.0 * L ** 3 / 1e9}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
