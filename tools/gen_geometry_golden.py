#!/usr/bin/env python3
"""Generate tests/golden/geometry.npz by running the reference's geometry / dynamics / physics / quantization helpers at
N = 16 and N = 33: so3_generators, cartesian_generators, rotate and the matrices expm(xi . S) behind it, grad,
north_blob, blob, project_el, sectional_curvature, elmr2mat, elmc2mat.

The matrix inputs are rebuilt from integer hashes (det_values, as in tools/gen_analysis_golden.py; `inputs` below is what
the tests call too), so only the reference's OUTPUTS are stored.

blob(N, (0, 0, -1), 0.1): the reference's QR frame for the south pole is a half turn, where scipy's as_rotvec is still
well defined, so the reference returns a finite matrix and the case is stored; were it not finite, the script would
leave it out and say so.

Runs where the reference is importable (QUFLOW_REFERENCE, default /root/reference), with oracle/refshim on sys.path as
oracle/gen_golden.py does; only the output vectors are committed.

Run:   python3 tools/gen_geometry_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("QUFLOW_REFERENCE", "/root/reference")

import numpy as np  # noqa: E402

SIZES = (16, 33)
XIS = ((0.3, -1.1, 0.7), (2.0, 1.5, -1.4), (0.0, 0.0, 2.5))
BLOB_POS = ((0.3, 0.5, -0.81), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0))
PROJECT_ELS = (1, 3, -1, [1, 2])


def det_values(n, salt):
    k = np.arange(n, dtype=np.int64)
    v = (k * 2654435761 + (salt + 1) * 40503) % 2147483647
    return (v / 2147483647.0 - 0.5) * 4.0


def generic(N, salt):
    return (det_values(N * N, salt) + 1j * det_values(N * N, salt + 1)).reshape(N, N)


def skewherm(N, salt):
    A = generic(N, salt)
    return (A - A.conj().T) / 2


def curvature_pairs(N):
    """Two pairs (F, G) of skew-Hermitian matrices that are linearly independent of each other.

    A salt only shifts det_values' sequence by a constant of order 1e-4, so matrices built from neighbouring salts are
    equal to four digits.  The curvature expression vanishes to second order where F and G are parallel: for such a pair
    its two Poisson terms are 1e8 times the result and cancel, the reference's own value moves by 5e-8 of itself when an
    input moves by one ulp, and no comparison to 1e-10 means anything.  So the eight real and imaginary parts are cut as
    disjoint segments from ONE sequence instead; a segment starts N^2 multiplier steps after the last, anywhere in the
    range.  For these pairs the largest of the four terms is 4 to 11 times the result, and an input noise of one ulp
    moves the reference's value by 6e-15 of itself at the most (measured at N = 16 and 33, 20 draws each)."""
    v = det_values(8 * N * N, 37).reshape(8, N, N)
    mats = [v[2 * i] + 1j * v[2 * i + 1] for i in range(4)]
    F0, G0, F1, G1 = [(A - A.conj().T) / 2 for A in mats]
    return ((F0, G0), (F1, G1))


def inputs(N):
    """The matrices the fixture's outputs belong to: W generic / skew-Hermitian (rotate, project_el), P (grad), and the two
    skew-Hermitian pairs of sectional_curvature."""
    return {"W_generic": generic(N, 31), "W_skew": skewherm(N, 33), "P": generic(N, 35), "pairs": curvature_pairs(N)}


def elm_cases(N):
    return ((0, 0), (3, -2), (3, 2), (5, 0), (N - 1, N - 1))


def el_tag(el):
    return "_".join(str(e) for e in el) if isinstance(el, list) else str(el)


def main():
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, os.path.join(REPO, "oracle", "refshim"))
    sys.path.insert(0, REF)
    from scipy.linalg import expm
    import quflow as qf  # the reference
    from quflow import dynamics as rd
    from quflow import geometry as rg
    from quflow import physics as rp
    from quflow import quantization as rq

    out = {}
    for N in SIZES:
        data = inputs(N)
        S = rg.so3_generators(N)
        X = rg.cartesian_generators(N)
        out["so3_%d" % N] = np.stack(S)
        out["cartesian_%d" % N] = np.stack(X)
        for i, xi in enumerate(XIS):
            out["expm_%d_%d" % (i, N)] = expm(xi[0] * S[0] + xi[1] * S[1] + xi[2] * S[2])
            out["rotate_generic_%d_%d" % (i, N)] = rg.rotate(np.array(xi), data["W_generic"])
            out["rotate_skew_%d_%d" % (i, N)] = rg.rotate(np.array(xi), data["W_skew"])
        out["grad_%d" % N] = rg.grad(data["P"])
        out["north_blob_s0_%d" % N] = rd.north_blob(N, 0)
        out["north_blob_s01_%d" % N] = rd.north_blob(N, 0.1)
        for i, pos in enumerate(BLOB_POS):
            B = rd.blob(N, np.array(pos), 0.1)
            if np.all(np.isfinite(B)):
                out["blob_%d_%d" % (i, N)] = B
            else:
                print("blob at", pos, "N =", N, ": the reference's result is not finite -- left out")
        for kind in ("generic", "skew"):
            for el in PROJECT_ELS:
                for comp in (False, True):
                    out["project_%s_el%s_c%d_%d" % (kind, el_tag(el), comp, N)] = \
                        rd.project_el(data["W_" + kind].copy(), el, complement=comp)
        out["curvature_%d" % N] = np.array([rp.sectional_curvature(F, G) for F, G in data["pairs"]])
        for el, m in elm_cases(N):
            out["elmr_%d_%d_%d" % (el, m, N)] = rq.elmr2mat(el, m, N).toarray()
            out["elmc_%d_%d_%d" % (el, m, N)] = rq.elmc2mat(el, m, N).toarray()
    path = os.path.join(REPO, "tests", "golden", "geometry.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "(%d arrays, %d bytes)" % (len(out), os.path.getsize(path)), "reference", qf.__file__)


if __name__ == "__main__":
    main()
