#!/usr/bin/env python3
"""Generate tests/golden/transforms.npz by running the reference's host-side transforms (quflow/transforms.py:271-401:
shr2shc, shc2shr, fun2img, img2fun; quflow/utils.py:179-203: sphgrid).  They are pure numpy there.

The inputs are rebuilt from integer hashes (det_values), so only the outputs are stored: as SHA-256 digests of their
bytes, with the arrays themselves where they are small.

Runs where the reference is importable (QUFLOW_REFERENCE, default /root/reference), with oracle/refshim on sys.path as
oracle/gen_golden.py does; only the input/output vectors are committed.

Run:   python3 tools/gen_transforms_golden.py
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("QUFLOW_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.path.join(REPO, "oracle", "refshim"))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import quflow as qf  # noqa: E402  (the reference)
from quflow import transforms as rt  # noqa: E402
from quflow import utils as ru  # noqa: E402


def det_values(n, salt):
    """Inputs that any machine rebuilds bit for bit (integer hashing, one correctly rounded division): the fixture stores
    the reference's outputs only.  The same function is in tests/test_transforms_host.py."""
    k = np.arange(n, dtype=np.int64)
    v = (k * 2654435761 + (salt + 1) * 40503) % 2147483647
    return (v / 2147483647.0 - 0.5) * 4.0


def det_image(shape, salt):
    k = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((k * 2654435761 + (salt + 1) * 40503) % 2147483647 % 256).astype(np.uint8).reshape(shape)


def record(out, key, arr):
    """A reference output: its SHA-256 digest, dtype and shape always; the array itself when it is small."""
    arr = np.ascontiguousarray(arr)
    out[key + "__sha256"] = np.array(hashlib.sha256(arr.tobytes()).hexdigest())
    out[key + "__dtype"] = np.array(str(arr.dtype))
    out[key + "__shape"] = np.array(arr.shape, dtype=np.int64)
    if arr.size <= 4096:
        out[key] = arr


def main():
    out = {}
    for N in (17, 128):
        omr = det_values(N * N, 1)
        omc = det_values(N * N, 2) + 1j * det_values(N * N, 3)
        record(out, "shr2shc_%d" % N, rt.shr2shc(omr))
        record(out, "shc2shr_%d" % N, rt.shc2shr(omc))
        # the reference tests' round trips (quflow/tests/test_transforms.py): real -> complex -> real, and complex -> real
        # -> complex for a complex array that is the expansion of a real function
        record(out, "shc2shr_shr2shc_%d" % N, rt.shc2shr(rt.shr2shc(omr)))
        record(out, "shr2shc_shc2shr_%d" % N, rt.shr2shc(rt.shc2shr(rt.shr2shc(omr))))
        theta, phi = ru.sphgrid(N)
        record(out, "sphgrid_theta_%d" % N, theta)
        record(out, "sphgrid_phi_%d" % N, phi)
        f = det_values(N * (2 * N - 1), 4).reshape(N, 2 * N - 1)
        record(out, "fun2img_%d" % N, rt.fun2img(f))
        record(out, "fun2img_lim_%d" % N, rt.fun2img(f, lim=(-0.5, 1.5)))
        record(out, "fun2img_sym_%d" % N, rt.fun2img(f, lim=0.75))
        img = det_image((N, 2 * N - 1), 5)
        record(out, "img2fun_%d" % N, rt.img2fun(img))
        record(out, "img2fun_lim_%d" % N, rt.img2fun(img, lim=(-2.0, 3.0)))
    # lengths that are not squares: degrees cut short where the reference still completes
    for n in (5, 12, 30):
        record(out, "shr2shc_n%d" % n, rt.shr2shc(det_values(n, 6)))
    path = os.path.join(REPO, "tests", "golden", "transforms.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "(%d arrays)" % len(out), "reference", qf.__file__)


if __name__ == "__main__":
    main()
