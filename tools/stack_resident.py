#!/usr/bin/env python3
"""Time of an MHD run with the state resident on the device against the host-in / host-out stepper (DESIGN.md 6.1,
profiles/stack_resident.json).

The run: `--steps` MHD steps in chunks of `--chunk`, the state of tests/test_hip_stack_resident.py -- (make_W0(N, 1),
solve_poisson(make_W0(N, 2))) -- with dt = 0.25 hbar(N).  Every shape is warmed up by one untimed run; a run is timed by a
host clock around work that ends in a device synchronisation, `--repeats` times from the same initial state, and reported
as median and min-max.

  --mode host      qfa.magmp chunk by chunk on a host array (every chunk uploads and downloads the pair).  Touches nothing
                   newer than magmp, so the same file runs against a checkout of an older commit (`--root DIR` imports
                   quflow_amd from there): that is the baseline.
  --mode resident  DeviceMHDTrajectory.advance chunk by chunk, without and with diagnostics=True, and for comparison the
                   diagnostics composed on the host side of the library (download, solve_poisson, laplace, inner_L2).

One JSON line per (mode, variant, N) on stdout, with the SHA-256 of the final state (the paths agree bit for bit).
`--collect FILE...` merges such lines into one JSON document on stdout."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time


def collect(files):
    rows = []
    for name in files:
        with open(name) as f:
            rows += [json.loads(line) for line in f if line.startswith("{")]
    print(json.dumps({"tool": "tools/stack_resident.py", "rows": rows}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["host", "resident"], default="resident")
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--collect", nargs="+")
    args = ap.parse_args()
    if args.collect:
        return collect(args.collect)
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats: the report is a median with its spread")
    sys.path.insert(0, args.root)
    import numpy as np
    import quflow_amd as qfa

    if qfa.device_count() < 1:
        raise SystemExit("no HIP device visible: this measures on the GPU only")
    chunks = [min(args.chunk, args.steps - k0) for k0 in range(0, args.steps, args.chunk)]

    def report(N, variant, seconds, state, **more):
        row = {"mode": args.mode, "variant": variant, "N": N, "label": args.label, "steps": args.steps, "chunk": args.chunk,
               "repeats": len(seconds), "median_s": statistics.median(seconds), "min_s": min(seconds), "max_s": max(seconds),
               "seconds": seconds}
        if state is not None:
            row["state_sha256"] = hashlib.sha256(np.ascontiguousarray(state).tobytes()).hexdigest()
        row.update(more)
        print(json.dumps(row), flush=True)

    for N in args.sizes:
        state0 = np.stack([qfa.ensemble.make_W0(N, 1), qfa.solve_poisson(qfa.ensemble.make_W0(N, 2)).copy()])
        dt = 0.25 * qfa.hbar(N)

        if args.mode == "host":
            def run():
                W = state0.copy()
                t0 = time.perf_counter()
                for n in chunks:
                    qfa.magmp(W, dt, n)          # (returns after its download: synchronised)
                return time.perf_counter() - t0, W
            run()
            res = [run() for _ in range(args.repeats)]
            report(N, "magmp", [t for t, _ in res], res[-1][1])
            continue

        from quflow_amd.geometry import inner_L2

        def host_composed(state):
            W, T = state[0], state[1]
            P, LT = qfa.solve_poisson(W), qfa.laplace(T)
            return (-inner_L2(W, P) / 2, -inner_L2(T, LT) / 2, inner_L2(W, T), inner_L2(T, T) / 2, inner_L2(W, W) / 2)

        tr = qfa.DeviceMHDTrajectory(state0)
        try:
            for variant, diag in (("advance", False), ("advance+diagnostics", True)):
                def run():
                    tr.upload(state0)
                    tr.sync()
                    t0 = time.perf_counter()
                    for n in chunks:
                        tr.advance(dt, n, diagnostics=diag)
                    tr.sync()
                    return time.perf_counter() - t0
                run()
                secs = [run() for _ in range(args.repeats)]
                report(N, variant, secs, tr.download())
            # one diagnostics call on the resident state against the same five numbers composed from the library's host-in
            # functions (what a chunk's log cost before): per call
            tr.diagnostics()
            host_composed(tr.download())
            for variant, fn in (("diagnostics", tr.diagnostics), ("diagnostics host-composed", lambda: host_composed(tr.download()))):
                secs = []
                for _ in range(args.repeats):
                    tr.sync()
                    t0 = time.perf_counter()
                    fn()
                    secs.append(time.perf_counter() - t0)
                report(N, variant, secs, None, per="call")
        finally:
            tr.ctx.close()


if __name__ == "__main__":
    main()
