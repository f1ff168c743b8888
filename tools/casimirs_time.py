#!/usr/bin/env python3
"""What the device Casimirs cost, what they resolve, and the per-chunk drift they make loggable.

    python3 tools/casimirs_time.py [N ...]          (default 512 1024 2048; appends to profiles/casimirs.jsonl)

Per N, a DeviceTrajectory on IC-A (quflow_amd.ensemble.make_W0); medians of `reps` calls after a warm-up call:

  kind "time"        casimirs4 / casimirs8: one tr.casimirs(4) / tr.casimirs(8) -- wall_ms (host clock around the synchronous
                     call), event_ms (HIP events on the context's stream around it), products_ms and traces_ms (the call's own
                     events: the products that store the powers; k_power_traces with its fold), hbm_bound_ms = 16 p N^2 bytes
                     over 8 TB/s and traces_hbm_frac = hbm_bound_ms / traces_ms;
                     download_numpy_ms: the route without the entry point, tr.download() and numpy traces for k = 2, 3, 4 as
                     tools/longrun.py forms them; spectrum_ms: tr.spectrum(), the other conserved quantity of a resident run;
                     first_product_ms: one plain N x N product alone (products_ms of casimirs(3), which stores A_2 only)
  kind "resolution"  |device - reference| per k <= 8 in units of u |C_k| (u = 2^-53; entries with |C_k| < 1e-12 reported
                     absolutely, as null units): reference = the same powers in long double for N <= 257, numpy complex128
                     above
  kind "drift"       N = 512 and 1024: C_k - C_k(0) for k = 2, 3, 4 after every chunk of 100 steps of a 1,000-step run at
                     dt = 0.25 hbar, from tr.casimirs(4), with the time the ten instrument calls took next to the run's"""
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

U = 2.0 ** -53


def host_casimirs_k234(W):
    H = 1j * W
    N = W.shape[-1]
    H2 = H @ H
    return [float(np.trace(H2).real / N), float(np.trace(H2 @ H).real / N), float(np.trace(H2 @ H2).real / N)]


def reference(W, kmax=8):
    """The library's recipe for the powers on the host: long double up to N = 257, numpy complex128 above."""
    N = W.shape[-1]
    H = (1j * W).astype(np.clongdouble if N <= 257 else np.complex128)
    A = [H, H @ H]
    A.append(A[1] @ H)
    A.append(A[1] @ A[1])
    out = [np.trace(H).real / N]
    for k in range(2, kmax + 1):
        out.append((A[k // 2 - 1] * A[k - k // 2 - 1].T).sum().real / N)
    return np.array(out, dtype=np.longdouble)


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def casimir_times(tr, kmax, reps):
    lib, h = tr._lib, tr.ctx.handle
    tr.casimirs(kmax)
    wall, event, products, traces = [], [], [], []
    ms, a, b = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for _ in range(reps):
        _lib.check(lib.qf_timer_start(h))
        t0 = time.perf_counter()
        tr.casimirs(kmax)
        wall.append(1e3 * (time.perf_counter() - t0))
        _lib.check(lib.qf_timer_stop(h, ctypes.byref(ms)))
        _lib.check(lib.qf_casimirs_times(h, ctypes.byref(a), ctypes.byref(b)))
        event.append(ms.value)
        products.append(a.value)
        traces.append(b.value)
    p = (kmax + 1) // 2
    bound = 1e3 * 16.0 * p * tr.N * tr.N / 8e12
    med = lambda v: float(np.median(v))      # noqa: E731
    return {"wall_ms": med(wall), "event_ms": med(event), "products_ms": med(products), "traces_ms": med(traces),
            "hbm_bound_ms": bound, "traces_hbm_frac": bound / med(traces)}


def main():
    Ns = [int(a) for a in sys.argv[1:]] or [512, 1024, 2048]
    if qfa.device_count() < 1:
        raise SystemExit("no HIP device visible: the timings need the GPU")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "casimirs.jsonl"), "a") as log:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")

        for N in Ns:
            W0 = qfa.ensemble.make_W0(N, 0)
            tr = qfa.DeviceTrajectory(W0)
            reps = 20
            row = {"kind": "time", "N": N, "reps": reps}
            row["casimirs4"] = casimir_times(tr, 4, reps)
            row["casimirs8"] = casimir_times(tr, 8, reps)
            row["download_numpy_ms"] = median_ms(lambda: host_casimirs_k234(tr.download()), 3 if N >= 2048 else 5)
            row["spectrum_ms"] = median_ms(tr.spectrum, 1 if N >= 2048 else 3)
            # (the A_2 launch alone: casimirs(3) stores A_2 only; its products_ms is that one product)
            row["first_product_ms"] = casimir_times(tr, 3, reps)["products_ms"]
            emit(row)
            tr.ctx.close()

        for N in sorted(set([100, 257] + Ns)):
            W0 = qfa.ensemble.make_W0(N, 0)
            dev = qfa.casimirs(W0, 8).astype(np.longdouble)
            ref = reference(W0)
            diff = np.abs(dev - ref)
            units = [float(d / (U * abs(r))) if abs(r) >= 1e-12 else None for d, r in zip(diff, ref)]
            emit({"kind": "resolution", "N": N, "reference": "long double" if N <= 257 else "numpy complex128",
                  "casimirs": [float(v) for v in dev], "abs_diff": [float(d) for d in diff], "diff_in_u_C": units})

        for N in [n for n in (512, 1024) if n in Ns]:
            tr = qfa.DeviceTrajectory(qfa.ensemble.make_W0(N, 0))
            dt = 0.25 * qfa.hbar(N)
            c0 = tr.casimirs(4)
            rows, t_run, t_cas = [], 0.0, 0.0
            for k in range(10):
                t0 = time.perf_counter()
                tr.advance(dt, 100)
                t1 = time.perf_counter()
                c = tr.casimirs(4)
                t2 = time.perf_counter()
                t_run += t1 - t0
                t_cas += t2 - t1
                rows.append({"step": 100 * (k + 1), "casimir_drift_k234": [float(a - b) for a, b in zip(c[1:], c0[1:])]})
            emit({"kind": "drift", "N": N, "steps": 1000, "chunk": 100, "stepsize": 0.25, "casimirs0_k234": [float(v) for v in c0[1:]],
                  "run_ms": 1e3 * t_run, "casimir_calls_ms": 1e3 * t_cas, "chunks": rows})
            tr.ctx.close()


if __name__ == "__main__":
    main()
