#!/usr/bin/env python3
"""Wall time of the device eigensolver and of scale_decomposition, next to numpy.linalg.eigh on the same host.

    python3 tools/eigh_time.py [N ...] [--out profiles/eigh_times.jsonl]          (default 512 1024 2048)

Per size: a white Hermitian matrix for `linalg.eigh` (eigenvalues and vectors, host in / host out: the PCIe copies of H and V
are part of the call), a smooth state W = shr2mat(random_shr) for `scale_decomposition(W)` (P solved on the device).  Each
call is synchronous -- the library synchronises its stream before it returns -- so two host clock reads bracket all of its
launches.  One warm-up call (context, work matrices), then the median of REPS = 5 repetitions; the sweeps and rotations the
solver took come from its own statistics.  numpy.linalg.eigh runs with the thread count of the environment (recorded).
One JSON line per size.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import quflow_amd as qfa  # noqa: E402
from quflow_amd import linalg  # noqa: E402

REPS = 5


def timed(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(min(t)), 1e3 * float(max(t))


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    Ns = [int(a) for a in args] or [512, 1024, 2048]
    lines = []
    for N in Ns:
        rng = np.random.default_rng(N)
        A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        H = (A + A.conj().T) / 2
        W = qfa.shr2mat(qfa.analysis.random_shr(lmax=N - 1, seed=N))
        eigh_ms = timed(lambda: linalg.eigh(H))
        st = linalg.last_stats()
        vals_ms = timed(lambda: linalg.eigvalsh(H))
        sd_ms = timed(lambda: qfa.scale_decomposition(W))
        np_ms = timed(lambda: np.linalg.eigh(H))
        rec = {"N": N, "reps": REPS,
               "eigh_ms": {"median": eigh_ms[0], "min": eigh_ms[1], "max": eigh_ms[2]},
               "eigh_sweeps": st["sweeps"], "eigh_rotations": st["rotations"],
               "eigh_ms_per_sweep": eigh_ms[0] / max(st["sweeps"], 1),
               "eigvalsh_ms": {"median": vals_ms[0], "min": vals_ms[1], "max": vals_ms[2]},
               "scale_decomposition_ms": {"median": sd_ms[0], "min": sd_ms[1], "max": sd_ms[2]},
               "numpy_eigh_ms": {"median": np_ms[0], "min": np_ms[1], "max": np_ms[2]},
               "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
               "device": qfa.device_info(0).get("name")}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
