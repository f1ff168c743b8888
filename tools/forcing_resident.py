#!/usr/bin/env python3
"""Time of a forced, viscous run by its four routes, and of k_forcing_affine alone.

The run: `--steps` isomp steps in chunks of `--chunk` from make_W0(N, 1) with dt = 0.25 hbar(N), the forcing
F(P, W) = F0 + a_W W + a_lap Delta W (F0 = 0.1 make_W0(N, 2), a_W = -0.02, a_lap = 0.1 / N^2) and the half step
ViscDampStep(nu=1e-4, alpha=0.01).  Every route is warmed up by one untimed run; a run is timed by a host clock around work that
ends in a device synchronisation, `--repeats` times from the same initial state, and reported as steps/s: median and min-max.

  a  callable    qfa.isomp chunk by chunk with the forcing as a numpy callable: the host-hook route, P and Whalf down and F up
                 over PCIe in every fixed-point iteration.  The only route before AffineForcing: the baseline.
  b  installed   qfa.isomp chunk by chunk with the AffineForcing installed for the call: the state still goes up and down per
                 chunk, nothing per iteration.
  c  resident    DeviceTrajectory(forcing=, strang_splitting=).advance chunk by chunk: nothing crosses PCIe.
  d  unforced    DeviceTrajectory.advance without forcing or half step: the fused stepper, the ceiling.

a, b and c run the same loop and must end in the same state bit for bit (the SHA-256 is reported).  The kernel alone:
`--launches` back-to-back launches on the resident state between two HIP events (qf_timer_start / qf_timer_stop), its time per
launch, the bytes it must move (F0, W and the result: 3 N^2 complex128; the Laplacian's two neighbours are re-reads of W that
the caches serve) over that time, and that rate as a fraction of the HBM peak (8 TB/s).

One JSON line per (route, N) on stdout."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

HBM_PEAK_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--routes", default="abcdk", help="which of a, b, c, d and k (the kernel alone) to run")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("at least 3 repeats: the report is a median with its spread")
    sys.path.insert(0, args.root)
    import numpy as np
    import quflow_amd as qfa
    from quflow_amd import _lib

    if qfa.device_count() < 1:
        raise SystemExit("no HIP device visible: this measures on the GPU only")
    chunks = [min(args.chunk, args.steps - k0) for k0 in range(0, args.steps, args.chunk)]

    def report(N, route, seconds, state, **more):
        rates = sorted(args.steps / t for t in seconds)
        row = {"route": route, "N": N, "steps": args.steps, "chunk": args.chunk, "repeats": len(seconds),
               "steps_per_s_median": statistics.median(rates), "steps_per_s_min": rates[0], "steps_per_s_max": rates[-1],
               "seconds": seconds}
        if state is not None:
            row["state_sha256"] = hashlib.sha256(np.ascontiguousarray(state).tobytes()).hexdigest()
        row.update(more)
        print(json.dumps(row), flush=True)

    for N in args.sizes:
        W0 = qfa.ensemble.make_W0(N, 1)
        F0 = 0.1 * qfa.ensemble.make_W0(N, 2)
        a_W, a_lap = -0.02, 0.1 / (N * N)
        dt = 0.25 * qfa.hbar(N)
        visc = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
        aff = qfa.AffineForcing(F0, a_W=a_W, a_lap=a_lap)

        def callable_forcing(P, W):          # the order of operations of AffineForcing, in numpy
            L = qfa.laplace(np.ascontiguousarray(W))
            out = np.empty(W.shape, dtype=np.complex128)
            out.real = (F0.real + a_W * W.real) + a_lap * L.real
            out.imag = (F0.imag + a_W * W.imag) + a_lap * L.imag
            return out

        def host_route(forcing):
            def run():
                W = W0.copy()
                its = 0.0
                t0 = time.perf_counter()
                for n in chunks:
                    stats = {"iterations": 0.0}
                    qfa.isomp(W, dt, n, forcing=forcing, strang_splitting=visc, stats=stats)     # (returns after its download)
                    its += stats["iterations"] * n
                return time.perf_counter() - t0, W, its / args.steps
            return run

        def resident_route(tr):
            def run():
                tr.upload(W0)
                tr.sync()
                its = 0
                t0 = time.perf_counter()
                for n in chunks:
                    its += tr.advance(dt, n)["total_iterations"]
                tr.sync()
                return time.perf_counter() - t0, None, its / args.steps
            return run

        for route, name, forcing in (("a", "callable", callable_forcing), ("b", "installed", aff)):
            if route not in args.routes:
                continue
            run = host_route(forcing)
            run()
            res = [run() for _ in range(args.repeats)]
            report(N, name, [r[0] for r in res], res[-1][1], iterations_per_step=res[-1][2])

        if "c" in args.routes or "k" in args.routes:
            tr = qfa.DeviceTrajectory(W0, forcing=aff, strang_splitting=visc)
            try:
                if "c" in args.routes:
                    run = resident_route(tr)
                    run()
                    res = [run() for _ in range(args.repeats)]
                    report(N, "resident", [r[0] for r in res], tr.download(), iterations_per_step=res[-1][2])
                if "k" in args.routes:
                    lib, h = tr._lib, tr.ctx.handle
                    tr.upload(W0)
                    tr.advance(dt, 1)            # (the stream-matrix buffer holds a stream matrix)

                    def launches():
                        ms = ctypes.c_double()
                        _lib.check(lib.qf_timer_start(h))
                        for _ in range(args.launches):
                            _lib.check(lib.qf_forcing(h, None, None, None))
                        _lib.check(lib.qf_timer_stop(h, ctypes.byref(ms)))
                        return ms.value * 1e-3 / args.launches
                    launches()
                    per = sorted(launches() for _ in range(args.repeats))
                    nbytes = 3 * N * N * 16
                    med = statistics.median(per)
                    print(json.dumps({"route": "k_forcing_affine", "N": N, "launches": args.launches, "repeats": len(per),
                                      "terms": "F0 + a_W W + a_lap Delta W", "bytes_moved": nbytes,
                                      "us_per_launch_median": med * 1e6, "us_per_launch_min": per[0] * 1e6,
                                      "us_per_launch_max": per[-1] * 1e6, "bytes_per_s_median": nbytes / med,
                                      "fraction_of_hbm_peak": nbytes / med / HBM_PEAK_BYTES_PER_S,
                                      "note": "back-to-back launches between two events: launch gaps are inside the time; "
                                              "at these sizes the operands fit the 256 MiB Infinity Cache"}), flush=True)
            finally:
                tr.ctx.close()

        if "d" in args.routes:
            tr = qfa.DeviceTrajectory(W0)
            try:
                run = resident_route(tr)
                run()
                res = [run() for _ in range(args.repeats)]
                report(N, "unforced", [r[0] for r in res], None, iterations_per_step=res[-1][2])
            finally:
                tr.ctx.close()


if __name__ == "__main__":
    main()
