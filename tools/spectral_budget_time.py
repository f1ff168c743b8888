#!/usr/bin/env python3
"""Wall time of the spectral budget of a resident forced trajectory against the composition that gave the same numbers
before qf_spectral_budget existed.

    python3 tools/spectral_budget_time.py [N ...]          (default 512 1024 2048)

Per N, a DeviceTrajectory with an AffineForcing (all four terms) and a ViscDampStep, resident basis, three timings (median
of `reps` host clock reads around synchronous calls; the first call of each kind is warm-up):

  budget_ms       tr.spectral_budget(): solve, product, forcing, ONE sweep carrying three vectors, degree sums on the device;
                  3 N doubles come back
  composed_ms     tr.shr(), tr.download(), solve_poisson, commutator, the forcing as a callable, two more mat2shr (on the
                  trajectory's own context, so no second basis is built), numpy sums per degree: three sweeps, and the state,
                  P, A, F and 3 N^2 coefficients cross PCIe
  spectrum_ms     tr.enstrophy_spectrum(): the sweep with one vector and the degree sums, nothing else -- the sweep's time
  mat2shr_ms      qf_mat2shr(ctx, NULL, NULL, N^2): the existing one-vector sweep, coefficients kept on the device

and the sweep's traffic: `basis_GB` = 8 sum_m (N - m)^2 bytes read once, over spectrum_ms (`sweep_GBps`, a lower bound of
the sweep kernel's own rate: pack, unpack and the sums are inside the clock) and over the HBM peak of 8 TB/s
(`sweep_share_of_peak`).  `budget_GBps_floor` divides the same bytes by the whole budget call.  The two routes' numbers are
compared (`max_rel_diff`: Z, T, I of the composition against the call's, relative to the largest entry of each row)."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import quflow_amd as qfa  # noqa: E402
from quflow_amd import _lib  # noqa: E402
from quflow_amd.context import ptr  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    out = fn()                             # warm-up: allocations, code objects
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), out


def ctx_mat2shr(ctx, M, n):
    om = np.zeros(n, dtype=np.float64)
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, ptr(M), ptr(om), ctypes.c_longlong(n)))
    return om


def degree_sums(u, v, N):
    prod = u * v
    return np.array([prod[l * l:(l + 1) * (l + 1)].sum() for l in range(1, N)])


def composed(tr, forcing):
    """Z, T, I for l = 1..N-1 the way a user of the parent commit gets them."""
    N = tr.N
    om = tr.shr()
    W = tr.download()
    P = qfa.solve_poisson(W)
    A = np.ascontiguousarray(-qfa.integrators.commutator(W, P) / qfa.hbar(N))      # [P, W] / hbar
    F = forcing(P, W)
    a = ctx_mat2shr(tr.ctx, A, N * N)
    f = ctx_mat2shr(tr.ctx, F, N * N)
    return degree_sums(om, om, N), 2 * degree_sums(om, a, N), 2 * degree_sums(om, f, N)


def main():
    Ns = [int(a) for a in sys.argv[1:]] or [512, 1024, 2048]
    if qfa.device_count() < 1:
        raise SystemExit("no HIP device visible: the timings need the GPU")
    for N in Ns:
        rng = np.random.default_rng(N)
        om0 = rng.standard_normal(N * N)
        om0[0] = 0.0
        l = np.floor(np.sqrt(np.arange(1, N * N)))
        om0[1:] /= (l * (l + 1)) ** 0.75
        W = qfa.shr2mat(om0, N, streamed=True)
        B = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        F0 = B - B.conj().T
        F0 *= 2 * np.abs(W).max() / np.abs(F0).max()
        forcing = qfa.AffineForcing(F0, a_W=-0.5, a_P=0.3, a_lap=2e-5)
        tr = qfa.DeviceTrajectory(W, forcing=forcing, strang_splitting=qfa.ViscDampStep(nu=2e-5, alpha=0.5))
        reps = 3 if N >= 2048 else 5
        budget_ms, b = timed(tr.spectral_budget, reps)
        composed_ms, (Z, T, I) = timed(lambda: composed(tr, forcing), reps)
        spectrum_ms, _ = timed(tr.enstrophy_spectrum, reps)
        mat2shr_ms, _ = timed(lambda: _lib.check(tr._lib.qf_mat2shr(tr.ctx.handle, None, None, ctypes.c_longlong(N * N))), reps)
        diff = max(np.abs(x - y).max() / np.abs(y).max() for x, y in
                   ((Z, b["enstrophy"]), (T, b["enstrophy_transfer"]), (I, b["enstrophy_input"])))
        basis_bytes = 8 * sum((N - m) ** 2 for m in range(N))
        row = {"N": N, "budget_ms": budget_ms, "composed_ms": composed_ms, "speedup": composed_ms / budget_ms,
               "spectrum_ms": spectrum_ms, "mat2shr_ms": mat2shr_ms, "basis_GB": basis_bytes / 1e9,
               "sweep_GBps": basis_bytes / (spectrum_ms * 1e-3) / 1e9,
               "sweep_share_of_peak": basis_bytes / (spectrum_ms * 1e-3) / HBM_PEAK,
               "budget_GBps_floor": basis_bytes / (budget_ms * 1e-3) / 1e9, "max_rel_diff": float(diff), "reps": reps}
        print(json.dumps(row), flush=True)
        tr.ctx.close()


if __name__ == "__main__":
    main()
