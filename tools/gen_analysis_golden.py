#!/usr/bin/env python3
"""Generate tests/golden/analysis.npz by running the reference's quflow/analysis.py:37-148 (energy_spectrum,
enstrophy_spectrum, gamma_ratio, random_shr) on `shr`, `shc` and `mat` input at N = 16 and 64.

The coefficient inputs are rebuilt from integer hashes (det_values, as in tools/gen_transforms_golden.py), so only the
reference's outputs are stored; the matrices W = shr2mat(omega), made by the reference, are stored with them (the tests
that read them need the device transform mat2shr).  The `fun` branch is not reachable here (no pyssht / ducc0).

Runs where the reference is importable (QUFLOW_REFERENCE, default /root/reference), with oracle/refshim on sys.path as
oracle/gen_golden.py does; only the input/output vectors are committed.

Run:   python3 tools/gen_analysis_golden.py
"""
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
from quflow import analysis as ra  # noqa: E402

RANDOM_SETS = ((15, 1.0, 0.0, 11), (31, 2.0, 0.3, 12), (20, 0.0, None, 13))     # (lmax, s, gamma, seed)


def det_values(n, salt):
    k = np.arange(n, dtype=np.int64)
    v = (k * 2654435761 + (salt + 1) * 40503) % 2147483647
    return (v / 2147483647.0 - 0.5) * 4.0


def main():
    out = {}
    for N in (16, 64):
        omr = det_values(N * N, 21)
        omc = det_values(N * N, 22) + 1j * det_values(N * N, 23)
        W = qf.shr2mat(omr, N)
        out["mat_%d" % N] = W
        for kind, data in (("shr", omr), ("shc", omc), ("mat", W)):
            for beta in (0, 1):
                el, e = ra.energy_spectrum(data, beta=beta)
                out["energy_%s_b%d_%d" % (kind, beta, N)] = e
            el, s = ra.enstrophy_spectrum(data)
            out["enstrophy_%s_%d" % (kind, N)] = s
            out["el_%d" % N] = el
        out["gamma_shr_%d" % N] = np.array(ra.gamma_ratio(omr))
        out["gamma_mat_%d" % N] = np.array(ra.gamma_ratio(W))
    for i, (lmax, s, gamma, seed) in enumerate(RANDOM_SETS):
        out["random_shr_%d" % i] = ra.random_shr(lmax=lmax, s=s, gamma=gamma, seed=seed)
    path = os.path.join(REPO, "tests", "golden", "analysis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "(%d arrays)" % len(out), "reference", qf.__file__)


if __name__ == "__main__":
    main()
