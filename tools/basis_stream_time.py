#!/usr/bin/env python3
"""Wall time of the quantization transforms on the streamed basis (qf_basis_stream), and on the resident one where it fits.

Every call is the device-only NULL form -- qf_shr2mat(ctx, NULL, n, NULL): coefficients left on the device -> the state W;
qf_mat2shr(ctx, NULL, NULL, n): W -> coefficients kept on the device -- so no PCIe copy is timed, and each call is
synchronous (the library synchronises its stream before it returns): two host clock reads bracket pack, every slab's
generate -> apply and unpack.  The split between generating columns (k_basis_slab) and applying them (k_block_matvec /
k_block_vecmat) comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python3 tools/basis_stream_time.py [N ...]          (default 1024 2048 4096 8192)

Band limits: full (Nmax = N) and Nmax = 128 (lmax = 127, n_omega = 128^2); the resident path at N <= 2048.  The slab
budget is QUFLOW_HIP_BASIS_SLAB_MB (4096 MiB by default).
"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from quflow_amd import _lib  # noqa: E402
from quflow_amd import quantization as q  # noqa: E402
from quflow_amd.context import Context, ptr  # noqa: E402


def timed(fn, reps):
    fn()                                   # first call: slab allocation
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    Ns = [int(a) for a in sys.argv[1:]] or [1024, 2048, 4096, 8192]
    slab = q.slab_bytes()
    for N in Ns:
        ctx = Context(N)
        lib = ctx._lib
        try:
            paths = [("streamed", slab)]
            if N <= 2048:
                _lib.check(lib.qf_basis_compute(ctx.handle))
                paths.append(("resident", 0))
            for Nmax in sorted({N, min(N, 128)}, reverse=True):
                n = Nmax * Nmax
                omega = np.random.default_rng(N).standard_normal(n)
                entries = sum((N - m) * (Nmax - m) for m in range(Nmax))
                for path, b in paths:
                    _lib.check(lib.qf_basis_stream(ctx.handle, ctypes.c_longlong(b)))
                    _lib.check(lib.qf_shr2mat(ctx.handle, ptr(omega), ctypes.c_longlong(n), None))
                    nslabs = lib.qf_basis_slab_plan(N, Nmax, ctypes.c_longlong(slab), None, 0) if b else 0
                    reps = 1 if entries > 2e10 else 3
                    fwd = timed(lambda: _lib.check(lib.qf_shr2mat(ctx.handle, None, ctypes.c_longlong(n), None)), reps)
                    bwd = timed(lambda: _lib.check(lib.qf_mat2shr(ctx.handle, None, None, ctypes.c_longlong(n))), reps)
                    row = {"N": N, "Nmax": Nmax, "path": path, "slab_MiB": b / 2 ** 20, "slabs": nslabs,
                           "basis_entries": entries, "shr2mat_ms": fwd, "mat2shr_ms": bwd,
                           "basis_GB": 8 * entries / 1e9}
                    print(json.dumps(row), flush=True)
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
