#!/usr/bin/env python3
"""Times and error ratios of the device rotation and gradient (quflow_amd.geometry, csrc/geometry.hip).

    python3 tools/rotate_time.py [N ...] [--out profiles/rotate_times.jsonl]          (default 512 1024 2048 4096)

Per size, on a resident trajectory (no PCIe traffic inside the timed calls), for xi = (0.3, -1.1, 0.7):
  * `rotation_matrix`: qf_so3_exp with the matrix left on the device, split by the library's own HIP events
    (qf_so3_exp_times) into the one Taylor launch and the sigma squarings; the host clock around the whole call next to them;
  * `rotate` on the resident state (the finiteness check with its read-back, the exponential, two products, one adjoint);
  * `grad` of the resident state with the result left on the device: the host clock around the call, and the HIP-event time
    of the stream between its first and last command (qf_timer_start / qf_timer_stop).
Each call is synchronous.  One warm-up call, then the median of REPS = 5 repetitions.
  * the error of the pure z rotation exp(2.5 S3) against diag(exp(2.5 i (a - s))) and the unitarity defect |R R^H - I|
    (product on the device) for the vector above, both in units of N max(1, |xi|) eps: the tests' bar is 8.
One JSON line per size, appended to --out.
"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import quflow_amd as qfa  # noqa: E402
from quflow_amd import _lib, geometry  # noqa: E402

REPS = 5
XI = np.array([0.3, -1.1, 0.7])
EPS = np.finfo(np.float64).eps


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def wall(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return stats(t)


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    Ns = [int(a) for a in args] or [512, 1024, 2048, 4096]
    for N in Ns:
        rng = np.random.default_rng(N)
        A = (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) / N
        traj = qfa.DeviceTrajectory(A - A.conj().T)
        lib, h = traj._lib, traj.ctx.handle
        xi_p = XI.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        sigma, degree = geometry.exp_plan(XI, N)

        taylor, squarings, total = [], [], []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            _lib.check_eigh(lib.qf_so3_exp(h, xi_p, None))
            t1 = time.perf_counter()
            a, b = ctypes.c_double(), ctypes.c_double()
            _lib.check_eigh(lib.qf_so3_exp_times(h, ctypes.byref(a), ctypes.byref(b)))
            if rep:
                taylor.append(a.value)
                squarings.append(b.value)
                total.append(1e3 * (t1 - t0))
        rotate_ms = wall(lambda: traj.rotate(XI))
        grad_ms = wall(lambda: _lib.check_eigh(lib.qf_grad(h, None, None)))
        grad_dev = []
        for rep in range(REPS):
            _lib.check(lib.qf_timer_start(h))
            _lib.check_eigh(lib.qf_grad(h, None, None))
            ms = ctypes.c_double()
            _lib.check(lib.qf_timer_stop(h, ctypes.byref(ms)))
            grad_dev.append(ms.value)

        z = np.array([0.0, 0.0, 2.5])
        a_s = np.arange(N) - (N - 1) / 2
        z_err = float(np.abs(qfa.rotation_matrix(z, N) - np.diag(np.exp(2.5j * a_s))).max())
        R = qfa.rotation_matrix(XI, N)
        unit_err = float(np.abs(geometry._device_matmul(R, np.ascontiguousarray(R.conj().T)) - np.eye(N)).max())
        rec = {"N": N, "reps": REPS, "xi": XI.tolist(), "squarings": sigma, "degree": degree,
               "so3_exp_taylor_ms": stats(taylor), "so3_exp_squarings_ms": stats(squarings),
               "so3_exp_ms_per_squaring": float(np.median(squarings)) / max(sigma, 1),
               "so3_exp_call_ms": stats(total),
               "rotate_resident_ms": rotate_ms,
               "grad_resident_ms": grad_ms, "grad_resident_stream_ms": stats(grad_dev),
               "z_rotation_err_over_N_xi_eps": z_err / (N * 2.5 * EPS),
               "unitarity_err_over_N_xi_eps": unit_err / (N * max(1.0, float(np.linalg.norm(XI))) * EPS),
               "device": qfa.device_info(0).get("name")}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")
        del traj
        qfa.release_contexts()


if __name__ == "__main__":
    main()
