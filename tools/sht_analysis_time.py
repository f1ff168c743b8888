#!/usr/bin/env python3
"""Wall time of the spherical-harmonic analysis (qf_fun2shr / qf_fun2shc) at a few bandwidths.

Each call is synchronous (the library synchronises its stream before it returns), so the time between two host clock
reads brackets one whole call: the grid's upload, the four kernels, the coefficients' copy back.  The first call at a
bandwidth also builds the two theta operators (and allocates): it is timed on its own, and the difference to a later call
is the one-off build.  Timed calls repeat until at least 0.5 s has been measured.  The per-kernel split comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script.

    python3 tools/sht_analysis_time.py [L ...]          (default 1024 2048 8192)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from quflow_amd import sht  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    fn()                                   # warm
    t, total = [], 0.0
    while total < 0.5 or len(t) < 3:
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
        total += t[-1]
    return 1e3 * first, 1e3 * float(np.median(t))


def main():
    Ls = [int(a) for a in sys.argv[1:]] or [1024, 2048, 8192]
    for L in Ls:
        rng = np.random.default_rng(L)
        f = rng.standard_normal((L, 2 * L - 1))
        first_r, real_ms = timed(lambda: sht.fun2shr(f))
        fc = f + 1j * rng.standard_normal((L, 2 * L - 1))
        _, cplx_ms = timed(lambda: sht.fun2shc(fc))
        row = {"L": L, "fun2shr_first_call_ms": first_r, "fun2shr_ms": real_ms, "fun2shc_complex_ms": cplx_ms,
               "grid_MB_real": L * (2 * L - 1) * 8 / 1e6, "dft_gflop_real": 8.0 * L ** 3 / 1e9,
               "theta_gflop_real": 4.0 * L ** 3 / 1e9, "legendre_lane_steps": 0.5 * L ** 3}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
