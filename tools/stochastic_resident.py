#!/usr/bin/env python3
"""Time of a stochastically forced, viscous run by its three routes, and of the per-step pattern launches alone.

The run: `--steps` isomp steps in chunks of `--chunk` from make_W0(N, 1) with dt = 0.25 hbar(N), white-in-time noise in the band
l in [20, 24] (sigma = 0.1, one pattern per step), friction a_W = -0.02, viscosity a_lap = 0.1 / N^2 and the half step
ViscDampStep(nu=1e-4, alpha=0.01).  Every route is warmed up by one untimed run; a run is timed by a host clock around work that
ends in a device synchronisation, `--repeats` times from the same initial state and counter 0, and reported as steps/s: median
and min-max.

  a  redraw      what there was before StochasticForcing, at its best: a resident DeviceTrajectory, and per step a pattern made
                 on the host (draw_host, then the band-limited streamed shr2mat), wrapped in an AffineForcing, installed with
                 set_forcing (an N^2 upload) and one advance(dt, 1).
  b  callable    qfa.isomp chunk by chunk with as_callable: the host-hook route, P and Whalf down and F up over PCIe in every
                 fixed-point iteration.
  c  resident    DeviceTrajectory(forcing=StochasticForcing, strang_splitting=).advance chunk by chunk: nothing crosses PCIe.

b and c run the same loop on the same numbers and must end in the same state bit for bit (the SHA-256 is reported); a restarts
the iteration vector every step and draws with numpy's log / cos / sin, so its state differs in the last digits.  The pattern
launches alone (k_stoch_draw, k_pack_coeffs, k_block_matvec on the band basis): `--launches` back-to-back patterns between two
HIP events (qf_timer_start / qf_timer_stop), the time per pattern, and the bytes of the band basis it reads.

One JSON line per (route, N) on stdout."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--band", type=int, nargs=2, default=[20, 24])
    ap.add_argument("--routes", default="abck", help="which of a, b, c and k (the pattern launches alone) to run")
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
    l_min, l_max = args.band

    def report(N, route, seconds, state, **more):
        rates = sorted(args.steps / t for t in seconds)
        row = {"route": route, "N": N, "band": [l_min, l_max], "steps": args.steps, "chunk": args.chunk, "repeats": len(seconds),
               "steps_per_s_median": statistics.median(rates), "steps_per_s_min": rates[0], "steps_per_s_max": rates[-1],
               "seconds": seconds}
        if state is not None:
            row["state_sha256"] = hashlib.sha256(np.ascontiguousarray(state).tobytes()).hexdigest()
        row.update(more)
        print(json.dumps(row), flush=True)

    for N in args.sizes:
        W0 = qfa.ensemble.make_W0(N, 1)
        a_W, a_lap = -0.02, 0.1 / (N * N)
        dt = 0.25 * qfa.hbar(N)
        visc = qfa.ViscDampStep(nu=1e-4, alpha=0.01)

        def make():
            return qfa.StochasticForcing(l_min, l_max, 0.1, seed=2026, a_W=a_W, a_lap=a_lap)

        if "a" in args.routes:
            tr = qfa.DeviceTrajectory(W0, strang_splitting=visc)
            try:
                def run():
                    sf = make()
                    tr.upload(W0)
                    tr.sync()
                    its = 0
                    t0 = time.perf_counter()
                    for n in range(args.steps):
                        F0 = qfa.shr2mat(sf.draw_host(n, dt), N, streamed=True)
                        tr.set_forcing(qfa.AffineForcing(F0, a_W=a_W, a_lap=a_lap))
                        its += tr.advance(dt, 1)["total_iterations"]
                    tr.sync()
                    return time.perf_counter() - t0, None, its / args.steps
                run()
                res = [run() for _ in range(args.repeats)]
                report(N, "redraw", [r[0] for r in res], tr.download(), iterations_per_step=res[-1][2])
            finally:
                tr.ctx.close()

        if "b" in args.routes:
            def run():
                sf = make()
                W = W0.copy()
                its, t = 0.0, 0.0
                t0 = time.perf_counter()
                for n in chunks:
                    stats = {"iterations": 0.0}
                    qfa.isomp(W, dt, n, forcing=sf.as_callable(dt, N, time0=t), time=t, strang_splitting=visc, stats=stats)
                    sf.step += n
                    t += n * dt
                    its += stats["iterations"] * n
                return time.perf_counter() - t0, W, its / args.steps
            run()
            res = [run() for _ in range(args.repeats)]
            report(N, "callable", [r[0] for r in res], res[-1][1], iterations_per_step=res[-1][2])

        if "c" in args.routes or "k" in args.routes:
            sf = make()
            tr = qfa.DeviceTrajectory(W0, forcing=sf, strang_splitting=visc)
            try:
                if "c" in args.routes:
                    def run():
                        tr.upload(W0)
                        tr.stochastic_seek(0)
                        tr.sync()
                        its = 0
                        t0 = time.perf_counter()
                        for n in chunks:
                            its += tr.advance(dt, n)["total_iterations"]
                        tr.sync()
                        return time.perf_counter() - t0, None, its / args.steps
                    run()
                    res = [run() for _ in range(args.repeats)]
                    report(N, "resident", [r[0] for r in res], tr.download(), iterations_per_step=res[-1][2])
                if "k" in args.routes:
                    lib, h = tr._lib, tr.ctx.handle

                    def launches():
                        ms = ctypes.c_double()
                        _lib.check(lib.qf_timer_start(h))
                        for n in range(args.launches):
                            _lib.check(lib.qf_stochastic_pattern(h, ctypes.c_ulonglong(n), dt, None, None))
                        _lib.check(lib.qf_timer_stop(h, ctypes.byref(ms)))
                        return ms.value * 1e-3 / args.launches
                    launches()
                    per = sorted(launches() for _ in range(args.repeats))
                    nmax = l_max + 1
                    band_bytes = 8 * sum((N - m) * (nmax - m) for m in range(nmax))
                    med = statistics.median(per)
                    print(json.dumps({"route": "pattern_launches", "N": N, "band": [l_min, l_max], "launches": args.launches,
                                      "repeats": len(per), "kernels": "k_stoch_draw, k_pack_coeffs, k_block_matvec",
                                      "band_basis_bytes": band_bytes, "us_per_pattern_median": med * 1e6,
                                      "us_per_pattern_min": per[0] * 1e6, "us_per_pattern_max": per[-1] * 1e6,
                                      "note": "three back-to-back launches per pattern between two events: launch gaps are "
                                              "inside the time; the band basis fits the 256 MiB Infinity Cache"}), flush=True)
            finally:
                tr.ctx.close()


if __name__ == "__main__":
    main()
