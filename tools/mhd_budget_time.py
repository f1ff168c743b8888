#!/usr/bin/env python3
"""Wall time of the MHD budget of a resident pair (W, Theta) against the composition that gave the same numbers before
qf_mhd_spectral_budget existed, and against the hydrodynamic budget of one forced state at the same N.

    python3 tools/mhd_budget_time.py [N ...]          (default 512 1024 2048; appends to profiles/mhd_budget_time.jsonl)

Per N, a DeviceMHDTrajectory with the resident basis; medians of `reps` host clock reads around synchronous calls (the
first call of each kind is warm-up):

  call_ms         tr.mhd_budget(): solve, stencil, three products, ONE sweep carrying five vectors, nine degree-sum rows on
                  the device; 9 N doubles come back
  composed_ms     two tr.shr(j), tr.download(), solve_poisson, laplace, three commutator, three more mat2shr (on the
                  trajectory's own context, so no second basis is built), numpy sums per degree: five sweeps, and the pair,
                  P, B, three tendencies and 5 N^2 coefficients cross PCIe
  hydro_ms        DeviceTrajectory.spectral_budget() of W with an AffineForcing: the three-vector sweep, the yardstick for
                  "five vectors cost what three cost"
  mat2shr_ms      qf_mat2shr(ctx, NULL, NULL, N^2): the one-vector sweep, coefficients kept on the device

`basis_GB` = 8 sum_m (N - m)^2 bytes is what one sweep reads.  The sweep kernels' own times (k_block_vecmat_five against
k_block_vecmat<0, false>, mat2shr's) come from a separate `rocprofv3 --kernel-trace --stats` run of this script; the share
of mat2shr's sweep rate the five-vector sweep reaches is the ratio of those two kernel times.  The two routes' numbers are
compared (`max_rel_diff`: the nine rows of the composition against the call's, relative to the largest entry of each)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import quflow_amd as qfa  # noqa: E402
from quflow_amd import _lib  # noqa: E402
from quflow_amd.context import ptr  # noqa: E402

ROWS = [(0, 0, 1), (1, 1, 1), (0, 1, 1), (0, 2, 2), (0, 3, 2), (1, 4, 2), (1, 2, 1), (1, 3, 1), (0, 4, 1)]


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
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, ptr(np.ascontiguousarray(M)), ptr(om), ctypes.c_longlong(n)))
    return om


def degree_sums(u, v, N):
    prod = u * v
    return np.array([prod[l * l:(l + 1) * (l + 1)].sum() for l in range(N)])


def composed(tr):
    """The nine rows, l = 0..N-1, the way a user of the parent commit gets them."""
    N = tr.N
    hb = qfa.hbar(N)
    om, th = tr.shr(0), tr.shr(1)
    W, Theta = tr.download()
    P = qfa.solve_poisson(W).copy()
    B = np.array(qfa.laplace(Theta))
    commutator = qfa.integrators.commutator
    c = [om, th] + [ctx_mat2shr(tr.ctx, -commutator(Y, X) / hb, N * N) for X, Y in ((P, W), (B, Theta), (P, Theta))]
    return np.array([s * degree_sums(c[u], c[v], N) for u, v, s in ROWS])


def coefficients(N, rng, power):
    om = rng.standard_normal(N * N)
    om[0] = 0.0
    l = np.floor(np.sqrt(np.arange(1, N * N)))
    om[1:] /= (l * (l + 1)) ** power
    return om


def main():
    Ns = [int(a) for a in sys.argv[1:]] or [512, 1024, 2048]
    if qfa.device_count() < 1:
        raise SystemExit("no HIP device visible: the timings need the GPU")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mhd_budget_time.jsonl"), "a") as log:
        for N in Ns:
            rng = np.random.default_rng(N)
            W = qfa.shr2mat(coefficients(N, rng, 0.75), N, streamed=True)
            Theta = qfa.shr2mat(coefficients(N, rng, 1.25), N, streamed=True)
            reps = 3 if N >= 2048 else 5
            tr = qfa.DeviceMHDTrajectory(np.stack([W, Theta]))
            call_ms, _ = timed(tr.mhd_budget, reps)
            rows = np.zeros((9, N))
            _lib.check(tr._lib.qf_mhd_spectral_budget(tr.ctx.handle, N, ptr(rows), None))
            composed_ms, ref = timed(lambda: composed(tr), reps)
            mat2shr_ms, _ = timed(lambda: _lib.check(tr._lib.qf_mat2shr(tr.ctx.handle, None, None, ctypes.c_longlong(N * N))),
                                  reps)
            tr.ctx.close()
            B = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
            F0 = B - B.conj().T
            F0 *= 2 * np.abs(W).max() / np.abs(F0).max()
            hydro = qfa.DeviceTrajectory(W, forcing=qfa.AffineForcing(F0, a_W=-0.5, a_P=0.3, a_lap=2e-5))
            hydro_ms, _ = timed(hydro.spectral_budget, reps)
            hydro.ctx.close()
            diff = max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(ref, rows))
            basis_bytes = 8 * sum((N - m) ** 2 for m in range(N))
            row = {"N": N, "call_ms": call_ms, "composed_ms": composed_ms, "speedup": composed_ms / call_ms,
                   "hydro_ms": hydro_ms, "call_over_hydro": call_ms / hydro_ms, "mat2shr_ms": mat2shr_ms,
                   "basis_GB": basis_bytes / 1e9, "call_GBps_floor": basis_bytes / (call_ms * 1e-3) / 1e9,
                   "max_rel_diff": float(diff), "reps": reps}
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")


if __name__ == "__main__":
    main()
