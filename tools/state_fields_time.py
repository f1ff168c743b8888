#!/usr/bin/env python3
"""What one output row of function-space qutypes costs on a resident trajectory, composed and in one call.

For N = 512, 1024, 2048 (one process) and the qutype sets {'fun': f32, 'funL2': f32} (the reference's defaults) and
{'funhalf': f32}:
  (a) composed on the one-field API: tr.fun(n, berezin).astype(float32) per qutype -- one mat2shr sweep, one synthesis, one
      float64 grid over PCIe and one host cast each;
  (b) one tr.fields(qutypes) call -- one sweep, one stacked synthesis per bandwidth, float32 grids over PCIe;
  (c) the kernels of (a) and (b), from `rocprofv3 --kernel-trace --stats` runs of their own (one fresh child process per
      N and set, this script with --child): average time per launch by kernel name.  The one-field kernels (k_sht_pack<..>,
      k_sht_legendre<false>, k_sht_fourier) are (a)'s, the k_sht_*_fields ones (b)'s; mat2shr's kernels are launched by both.
Every call synchronises its stream before it returns, so the host clock around a call brackets the whole call.  After a
warm-up (context, basis, scratch, code objects) (a) and (b) alternate, and the median of REPS calls of each is reported; the
two results are compared bit for bit while warming up.  One JSON line per (N, set); --out appends them to a file.

    python3 tools/state_fields_time.py [--reps 20] [--no-kernels] [--out profiles/state_fields.jsonl] [N ...]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# (quflow_amd is imported by the two modes that use the GPU: the orchestrating process never opens the device, it only starts
# fresh child processes)
SETS = {"default_pair": {'fun': np.float32, 'funL2': np.float32}, "funhalf": {'funhalf': np.float32}}
KERNELS = ("k_pack_diags", "k_block_vecmat", "k_unpack_coeffs", "k_sht_twiddle", "k_sht_pack", "k_sht_legendre", "k_sht_fourier")


def state(N):
    rng = np.random.default_rng(N)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    W = A - A.conj().T
    return W / np.linalg.norm(W)


def composed(tr, qutypes):
    from quflow_amd.transforms import field_spec
    out = {}
    for q, dt in qutypes.items():
        n, berezin, _ = field_spec(q, tr.N)
        out[q] = tr.fun(n, berezin).astype(dt)
    return out


def measure(tr, qutypes, reps):
    a, b = composed(tr, qutypes), tr.fields(qutypes)          # warm-up of both, and the comparison
    same = all(np.array_equal(a[q], b[q]) for q in qutypes)
    ta, tb = [], []
    for _ in range(reps):                                     # alternating: both see the same neighbours
        t0 = time.perf_counter()
        composed(tr, qutypes)
        t1 = time.perf_counter()
        tr.fields(qutypes)
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    ms = lambda t: 1e3 * float(np.median(t))                  # noqa: E731
    return {"composed_ms": ms(ta), "fields_ms": ms(tb), "composed_min_ms": 1e3 * min(ta), "fields_min_ms": 1e3 * min(tb),
            "bit_identical": bool(same), "reps": reps}


def child(N, name, reps):
    import quflow_amd as qfa
    tr = qfa.DeviceTrajectory(state(N))
    try:
        measure(tr, SETS[name], reps)
    finally:
        tr.ctx.close()


def kernel_times(N, name, reps):
    """{kernel name: average microseconds per launch} from a rocprofv3 run of `--child N name` in a fresh process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", str(N), name, "--reps", str(reps)]
        done = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
        if done.returncode != 0:          # what the child or the profiler said goes with the failure
            sys.stderr.write(done.stderr.decode(errors="replace")[-4000:])
            raise RuntimeError("the profiled run of N=%d %s ended with status %d" % (N, name, done.returncode))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        out = {}
        for r in csv.DictReader(open(files[0])):
            short = r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            if short.startswith(KERNELS):
                out[short] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
        return out


def measure_all(sizes, reps):
    """(a) and (b) for every size and set in THIS process; one JSON line each."""
    import quflow_amd as qfa
    if qfa.device_count() < 1:
        sys.exit("no HIP device visible: nothing is measured")
    for N in sizes:
        tr = qfa.DeviceTrajectory(state(N))
        try:
            for name, qutypes in SETS.items():
                row = {"N": N, "qutypes": name}
                row.update(measure(tr, qutypes, reps))
                print(json.dumps(row), flush=True)
        finally:
            tr.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--measure", action="store_true", help="(internal) the wall times, in this process")
    ap.add_argument("--child", nargs=2, metavar=("N", "SET"), help="(internal) the profiled workload")
    args = ap.parse_args()
    sizes = args.sizes or [512, 1024, 2048]
    if args.child:
        child(int(args.child[0]), args.child[1], args.reps)
        return
    if args.measure:
        measure_all(sizes, args.reps)
        return
    me = [sys.executable, os.path.abspath(__file__)]
    done = subprocess.run(me + ["--measure", "--reps", str(args.reps)] + [str(n) for n in sizes], check=True,
                          stdout=subprocess.PIPE, timeout=900)
    for text in done.stdout.decode().splitlines():
        row = json.loads(text)
        if not args.no_kernels:
            row["kernels_us"] = kernel_times(row["N"], row["qutypes"], max(args.reps // 2, 5))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
