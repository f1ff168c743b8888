#!/usr/bin/env python3
"""Step rate of the resident stepper under an installed Hamiltonian (profiles/hamiltonian_resident.jsonl).

Variants, each on DeviceTrajectory.advance, `--steps` steps after `--warmup` warm-up steps, white data (make_W0, seed 0),
dt = 0.25 hbar(N):
  a  the built-in Hamiltonian
  b  TridiagonalHamiltonian.poisson(N) installed, no offset          (the same factors, the same kernels as a)
  c  A = poisson,      F = coriolis(N, 0.1) + 0.1 smooth             (k_solve_off)
  d  B = globalqg(50), F = coriolis(N, 0.5) + 0.5 smooth             (installed factors + k_solve_off)
  hc, hd  the same Hamiltonians as c and d handed over as a plain callable: the hooked route (qf_isomp_hooked, the state
          crosses PCIe twice per iteration), `--hooked-steps` steps -- the only route there was before qf_set_hamiltonian.

One JSON line per (variant, N, repeat) on stdout; `--root DIR` imports quflow_amd from another tree (the parent commit's,
for variant a).  Times are host clocks around calls that end in a device synchronisation."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--variants", nargs="+", default=["a", "b", "c", "d", "hc", "hd"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hooked-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import numpy as np
    import quflow_amd as qfa

    if qfa.device_count() < 1:
        raise SystemExit("no HIP device visible: this measures on the GPU only")

    def smooth(N, seed):
        W = qfa.solve_poisson(qfa.ensemble.make_W0(N, seed)).copy()
        return W / (np.linalg.norm(W, "fro") / np.sqrt(N))

    def hamiltonian(v, N):
        if v == "a":
            return None
        if v == "b":
            return qfa.TridiagonalHamiltonian.poisson(N)
        if v in ("c", "hc"):
            return qfa.TridiagonalHamiltonian.poisson(N, offset=qfa.coriolis(N, 0.1) + 0.1 * smooth(N, 7))
        return qfa.TridiagonalHamiltonian.globalqg(N, 50.0, offset=qfa.coriolis(N, 0.5) + 0.5 * smooth(N, 7))

    for N in args.sizes:
        W0 = qfa.ensemble.make_W0(N, 0)
        dt = 0.25 * qfa.hbar(N)
        for rep in range(args.repeats):           # repeats alternate the variants: same-box pairs
            for v in args.variants:
                H = hamiltonian(v, N)
                row = {"variant": v, "N": N, "repeat": rep, "label": args.label}
                if v.startswith("h"):
                    f = (lambda W, H=H: H(W))     # a plain callable: the foreign-Hamiltonian route
                    W = W0.copy()
                    qfa.isomp(W, dt, steps=2, hamiltonian=f)
                    st = {"iterations": 0.0}
                    t0 = time.perf_counter()
                    qfa.isomp(W, dt, steps=args.hooked_steps, hamiltonian=f, stats=st)
                    t = time.perf_counter() - t0
                    row.update(route="qf_isomp_hooked", steps=args.hooked_steps, seconds=t, steps_per_s=args.hooked_steps / t,
                               iterations=st["iterations"])
                else:
                    tr = qfa.DeviceTrajectory(W0) if H is None else qfa.DeviceTrajectory(W0, hamiltonian=H)
                    try:
                        tr.advance(dt, args.warmup)
                        tr.sync()
                        t0 = time.perf_counter()
                        st = tr.advance(dt, args.steps)
                        tr.sync()
                        t = time.perf_counter() - t0
                        plan = tr.ctx.plan()
                    finally:
                        tr.ctx.close()
                    row.update(route="DeviceTrajectory.advance", steps=args.steps, seconds=t, steps_per_s=args.steps / t,
                               iterations=st["iterations"], solve_kernel=plan["laplacian_inverse"]["kernel"])
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
