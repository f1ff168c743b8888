"""The quantization basis and the four spherical-harmonics <-> matrix transforms (quantization.hip)
at the sizes runs use: N = 1000, 1024, 1025 and 2048.

Above N = 512 the transform kernels run launch geometry that the smaller tests never reach:
J = Nmax - m past the 32-row tiles and 256-column LDS chunks of k_block_matvec, past the 64-column
tiles and 256-row chunks of k_block_vecmat, and band limits Nmax < N on both sides of those edges.
The basis kernel k_basis picks each column's sign by adjust_basis_orientation_; at these sizes most
of LAPACK's eigenvectors end in an exact 0.0 where the twisted factorisation's end in a tiny value,
so the two sides take different branches of that rule.

Everything is compared with values computed independently on the host:
  * the basis with the tridiagonal blocks T_m of the direct Laplacian (residual, orthogonality) and
    with the oracle's LAPACK blocks (orientation, entries);
  * the transforms with an extended-precision restatement of the reference's shr2mat_ / mat2shr_ /
    shc2mat_ / mat2shc_ (below), held to a rounding-error bound per entry.

At N = 2048 the basis has 2.9e9 entries (23 GB): it stays on the device, and sampled columns are
read out through single-mode transforms instead.
"""
import contextlib
import ctypes
import gc
import math
import time

import numpy as np
import pytest
from scipy.linalg import eigh_tridiagonal

from conftest import load_golden
from oracle import quantization_oracle as qo

EPS = np.finfo(np.float64).eps
LD = np.longdouble
C1DSQ2 = 1.0 / np.sqrt(2.0)      # the reference's constants, as float64 (quantization.py:223, :303)
SQRT2 = np.sqrt(2.0)


# ----------------------------------------------------------------------------- host reference
# Extended-precision restatement of the reference's transforms (oracle/quantization_oracle.py:
# shr2mat_, mat2shr_, shc2mat_, mat2shc_) on a caller-supplied basis.  Each function returns the
# value (long double) and a bound per real component on how far a float64 evaluation may lie from it:
#     (terms + 2) * eps64 * (|B_m| @ |x_m|) * factor   +   k * eps64 * |value|
# i.e. the worst case of a sum of `terms` rounded products in any order (gamma_n <= n eps / 2, taken
# twice over) plus the rounding of the convention factors and of the final entry.

def band_limit(N, n_omega):
    """Nmax of a coefficient array with n_omega entries (quantization.py:204-208, 294-298)."""
    return N if n_omega >= N * N else math.isqrt(n_omega)


def basis_blocks(basis, N):
    """block(m) -> the (N-m) x (N-m) view of block m of a flat basis."""
    def block(m):
        o = qo.basis_break_index(m, N)
        n = N - m
        return basis[o:o + n * n].reshape(n, n)
    return block


def _matvec(B, X):
    """(B @ X in long double, |B| @ |X| in float64) for a float64 B and long double X (columns)."""
    return B.astype(LD) @ X, np.abs(B) @ np.abs(X).astype(np.float64)


def _vecmat(D, B):
    """(D^T @ B in long double, |D|^T @ |B|) for long double D (columns of diagonals)."""
    return (D.T @ B.astype(LD)).T, (np.abs(D).astype(np.float64).T @ np.abs(B)).T


def _idx(els, m):
    return els * els + els + m


def _sgn(m):
    return 1.0 if m % 2 == 0 else -1.0


def ref_shr2mat(omega, N, block, ms=None):
    """diag_m = sgn B_m[:, :J] @ x_m, x_m = (omega[el,m] - 1j omega[el,-m]) / sqrt2 (m > 0), W *= 1j.
    Returns (W_re, W_im, bound_re, bound_im) as (N, N) arrays; entries outside the band are exact
    zeros.  `ms` restricts to some blocks (the others stay zero)."""
    om = np.asarray(omega, dtype=np.float64)
    Nmax = band_limit(N, om.shape[0])
    Wr = np.zeros((N, N), dtype=LD)
    Wi = np.zeros((N, N), dtype=LD)
    br = np.zeros((N, N))
    bi = np.zeros((N, N))
    for m in (range(Nmax) if ms is None else [m for m in ms if m < Nmax]):
        els = np.arange(m, Nmax)
        B = block(m)[:, :Nmax - m]
        if m == 0:
            X = np.stack([om[_idx(els, 0)].astype(LD), np.zeros(els.shape[0], dtype=LD)], 1)
        else:
            X = np.stack([LD(C1DSQ2) * om[_idx(els, m)].astype(LD), -LD(C1DSQ2) * om[_idx(els, -m)].astype(LD)], 1)
        Y, A = _matvec(B, X)
        bnd = (X.shape[0] + 2) * EPS * A + EPS * np.abs(Y).astype(np.float64)
        s = _sgn(m)
        i = np.arange(N - m)
        # upper W[i, i+m] = 1j * s * y ; lower W[i+m, i] = 1j * conj(s * y)
        Wr[i, i + m], Wi[i, i + m] = -s * Y[:, 1], s * Y[:, 0]
        br[i, i + m], bi[i, i + m] = bnd[:, 1], bnd[:, 0]
        if m:
            Wr[i + m, i], Wi[i + m, i] = s * Y[:, 1], s * Y[:, 0]
            br[i + m, i], bi[i + m, i] = bnd[:, 1], bnd[:, 0]
    return Wr, Wi, br, bi


def ref_mat2shr(W, n_omega, block, ms=None):
    """z_m = diag(W, -m) @ B_m[:, :J]; omega[el,0] = Im z / N, omega[el,m] = sqrt2 sgn Im z / N,
    omega[el,-m] = -sqrt2 sgn Re z / N.  Returns (omega, bound) of length n_omega."""
    N = W.shape[-1]
    Nmax = band_limit(N, n_omega)
    out = np.zeros(n_omega, dtype=LD)
    bnd = np.zeros(n_omega)
    for m in (range(Nmax) if ms is None else [m for m in ms if m < Nmax]):
        els = np.arange(m, Nmax)
        d = np.diagonal(W, -m)
        D = np.stack([d.real.astype(LD), d.imag.astype(LD)], 1)
        Z, A = _vecmat(D, block(m)[:, :Nmax - m])
        s = _sgn(m)
        if m == 0:
            v = Z[:, 1] / N
            out[_idx(els, 0)] = v
            bnd[_idx(els, 0)] = (d.shape[0] + 2) * EPS * A[:, 1] / N + 2 * EPS * np.abs(v).astype(np.float64)
        else:
            vp = LD(SQRT2) * s * Z[:, 1] / N
            vm = -LD(SQRT2) * s * Z[:, 0] / N
            out[_idx(els, m)], out[_idx(els, -m)] = vp, vm
            bnd[_idx(els, m)] = (d.shape[0] + 2) * EPS * SQRT2 * A[:, 1] / N + 3 * EPS * np.abs(vp).astype(np.float64)
            bnd[_idx(els, -m)] = (d.shape[0] + 2) * EPS * SQRT2 * A[:, 0] / N + 3 * EPS * np.abs(vm).astype(np.float64)
    return out, bnd


def ref_shc2mat(omega, N, block, ms=None):
    """W[i+m, i] = 1j B_m @ omega[el,m], W[i, i+m] = 1j sgn B_m @ omega[el,-m] (m != 0)."""
    om = np.asarray(omega, dtype=np.complex128)
    Wr = np.zeros((N, N), dtype=LD)
    Wi = np.zeros((N, N), dtype=LD)
    br = np.zeros((N, N))
    bi = np.zeros((N, N))
    for m in (range(N) if ms is None else ms):
        els = np.arange(m, N)
        lo, up = om[_idx(els, m)], om[_idx(els, -m)]
        X = np.stack([lo.real, lo.imag, up.real, up.imag], 1).astype(LD)
        Y, A = _matvec(block(m), X)
        bnd = (X.shape[0] + 2) * EPS * A + EPS * np.abs(Y).astype(np.float64)
        i = np.arange(N - m)
        Wr[i + m, i], Wi[i + m, i] = -Y[:, 1], Y[:, 0]
        br[i + m, i], bi[i + m, i] = bnd[:, 1], bnd[:, 0]
        if m:
            s = _sgn(m)
            Wr[i, i + m], Wi[i, i + m] = -s * Y[:, 3], s * Y[:, 2]
            br[i, i + m], bi[i, i + m] = bnd[:, 3], bnd[:, 2]
    return Wr, Wi, br, bi


def ref_mat2shc(G, block, ms=None):
    """omega[el,m] = (diag(G, -m) @ B_m) / (1j N), omega[el,-m] = sgn (diag(G, m) @ B_m) / (1j N).
    Returns (omega_re, omega_im, bound_re, bound_im)."""
    N = G.shape[0]
    orr = np.zeros(N * N, dtype=LD)
    oi = np.zeros(N * N, dtype=LD)
    br = np.zeros(N * N)
    bi = np.zeros(N * N)
    for m in (range(N) if ms is None else ms):
        els = np.arange(m, N)
        lo, up = np.diagonal(G, -m), np.diagonal(G, m)
        D = np.stack([lo.real, lo.imag, up.real, up.imag], 1).astype(LD)
        Z, A = _vecmat(D, block(m))
        n = N - m
        # z / (1j N) = (Im z, -Re z) / N
        for (c_re, c_im, sign, key) in ((0, 1, 1.0, m), (2, 3, _sgn(m), -m))[:2 if m else 1]:
            vr, vi = sign * Z[:, c_im] / N, -sign * Z[:, c_re] / N
            orr[_idx(els, key)], oi[_idx(els, key)] = vr, vi
            br[_idx(els, key)] = (n + 2) * EPS * A[:, c_im] / N + 3 * EPS * np.abs(vr).astype(np.float64)
            bi[_idx(els, key)] = (n + 2) * EPS * A[:, c_re] / N + 3 * EPS * np.abs(vi).astype(np.float64)
    return orr, oi, br, bi


def excess(got, ref, bound):
    """max over entries of |got - ref| - bound, the entry where it is largest, and |got - ref| there."""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).astype(np.float64)
    over = err - bound
    k = int(np.argmax(over))
    return float(over.flat[k]), np.unravel_index(k, np.shape(over)), float(err.flat[k])


def assert_within(got, ref, bound, what):
    over, where, err = excess(got, ref, bound)
    assert over <= 0.0, "%s: |got - ref| = %.3e exceeds the rounding bound %.3e at %s" % (
        what, err, err - over, where)


def assert_W_within(W, ref, what):
    Wr, Wi, br, bi = ref
    assert_within(W.real, Wr, br, what + " (real part)")
    assert_within(W.imag, Wi, bi, what + " (imaginary part)")


def assert_shc_within(om, ref, what):
    orr, oi, br, bi = ref
    assert_within(om.real, orr, br, what + " (real part)")
    assert_within(om.imag, oi, bi, what + " (imaginary part)")


# ----------------------------------------------------------------------------- CPU: pin the helper
@pytest.mark.parametrize("N", [5, 16, 33, 64])
def test_reference_helper_vs_golden(N):
    """The extended-precision helper reproduces the reference's own outputs (tests/golden/quantization.npz,
    written by quflow.quantization), on the reference's basis (the golden one; at N = 64, which has no
    golden basis, the oracle's LAPACK basis restated from quantization.py:68-113)."""
    g = load_golden("quantization")
    basis = g["basis_N%d" % N] if "basis_N%d" % N in g.files else qo.compute_basis(N)
    block = basis_blocks(basis, N)
    pre = "N%d_" % N
    tol = 1e-13 * N
    Wr, Wi, _, _ = ref_shr2mat(g[pre + "omega"], N, block)
    assert np.abs(Wr - g[pre + "shr2mat"].real).max() <= tol
    assert np.abs(Wi - g[pre + "shr2mat"].imag).max() <= tol
    for W, key in ((g[pre + "W"], "mat2shr"), (g[pre + "G"], "mat2shr_G")):
        om, _ = ref_mat2shr(W, N * N, block)
        assert np.abs(om - g[pre + key]).max() <= tol
    Wr, Wi, _, _ = ref_shc2mat(g[pre + "omega_c"], N, block)
    assert np.abs(Wr - g[pre + "shc2mat"].real).max() <= tol
    assert np.abs(Wi - g[pre + "shc2mat"].imag).max() <= tol
    orr, oi, _, _ = ref_mat2shc(g[pre + "G"], block)
    assert np.abs(orr - g[pre + "mat2shc_G"].real).max() <= tol
    assert np.abs(oi - g[pre + "mat2shc_G"].imag).max() <= tol
    if N in (33, 64):      # the band-limited fixtures: 10 coefficients, and elmax = 2 (81 entries)
        Wr, Wi, _, _ = ref_shr2mat(g["short_omega"], N, block)
        ref = g["short_N%d_shr2mat" % N]
        assert np.abs(Wr - ref.real).max() <= tol and np.abs(Wi - ref.imag).max() <= tol
        for n, key in ((10, "short_N%d_mat2shr10"), (81, "short_N%d_mat2shr_elmax2")):
            om, _ = ref_mat2shr(ref, n, block)
            assert np.abs(om - g[key % N]).max() <= tol


def test_reference_helper_bound_holds_for_float64():
    """The helper's bound is a real rounding bound: plain float64 evaluations of the same sums, in
    two different orders (the oracle's BLAS products, and sequential sums), lie inside it; an error
    of one part in 1e12 in a single basis entry does not."""
    N = 64
    rng = np.random.default_rng(11)
    basis = qo.compute_basis(N)
    block = basis_blocks(basis, N)
    omega = rng.standard_normal(N * N)
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    W = np.zeros((N, N), dtype=complex)
    qo.shr2mat_(omega, basis, W)
    assert_W_within(W, ref_shr2mat(omega, N, block), "oracle shr2mat_")
    om = np.zeros(N * N)
    qo.mat2shr_(G, basis, om)
    assert_within(om, *ref_mat2shr(G, N * N, block), "oracle mat2shr_")
    omc = rng.standard_normal(N * N) + 1j * rng.standard_normal(N * N)
    W = np.zeros((N, N), dtype=complex)
    qo.shc2mat_(omc, basis, W)
    assert_W_within(W, ref_shc2mat(omc, N, block), "oracle shc2mat_")
    omc = np.zeros(N * N, dtype=complex)
    qo.mat2shc_(G, basis, omc)
    assert_shc_within(omc, ref_mat2shc(G, block), "oracle mat2shc_")
    # a sequential float64 sum of block 0 (another order than BLAS)
    B = block(0)
    x = omega[_idx(np.arange(N), 0)]
    seq = np.zeros(N)
    for j in range(N):
        seq = seq + B[:, j] * x[j]
    Wr, Wi, br, bi = ref_shr2mat(omega, N, block)
    assert_within(seq, Wi[np.arange(N), np.arange(N)], bi[np.arange(N), np.arange(N)], "sequential sum")
    # teeth: one basis entry off by 1e-12 relative is far outside the bound
    bad = basis.copy()
    o = qo.basis_break_index(3, N)
    bad[o + 5 * (N - 3) + 7] *= 1 + 1e-12
    Wb = np.zeros((N, N), dtype=complex)
    qo.shr2mat_(omega, bad, Wb)
    over_r = excess(Wb.real, ref_shr2mat(omega, N, block)[0], ref_shr2mat(omega, N, block)[2])[0]
    over_i = excess(Wb.imag, ref_shr2mat(omega, N, block)[1], ref_shr2mat(omega, N, block)[3])[0]
    assert max(over_r, over_i) > 0.0


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


_lap_tables = {}


def tridiagonal(N, m):
    """(diagonal, off-diagonal) of block m of the direct Laplacian (oracle compute_direct_laplacian),
    exactly as the oracle's compute_basis hands them to LAPACK."""
    if N not in _lap_tables:
        _lap_tables.clear()
        _lap_tables[N] = qo.compute_direct_laplacian(N, bc=False)
    lap = _lap_tables[N]
    n = N - m
    s = N * (N + 1) // 2 - n * (n + 1) // 2
    return lap[1, s:s + n], lap[0, s + 1:s + n]


def oracle_block(N, m):
    """The oracle's LAPACK block m (compute_basis) and the raw last entries LAPACK returned, before
    adjust_basis_orientation_ chose the signs."""
    d, e = tridiagonal(N, m)
    _, w2 = eigh_tridiagonal(d, e)
    w2 *= np.sqrt(N)
    w2 = w2[:, ::-1].copy()
    raw_last = w2[-1].copy()
    qo.adjust_basis_orientation_(w2, m)
    return w2, raw_last


def residual_ratio(N, m, B, cols):
    """||T_m b_j - lambda_j b_j||_inf / (eps ||T_m||_inf ||b_j||_2) for the columns `cols` of B
    (B holds those columns in order), lambda_j = -el (el + 1), el = m + j."""
    d, e = tridiagonal(N, m)
    TB = d[:, None] * B
    TB[:-1] += e[:, None] * B[1:]
    TB[1:] += e[:, None] * B[:-1]
    el = m + np.asarray(cols, dtype=np.float64)
    R = np.abs(TB + (el * (el + 1))[None, :] * B).max(axis=0)
    normT = np.abs(d).copy()
    normT[:-1] += np.abs(e)
    normT[1:] += np.abs(e)
    return R / (EPS * normT.max() * np.linalg.norm(B, axis=0))


RESIDUAL_C = 8.0        # observed <= 1 for the twisted factorisations (LAPACK's own vectors: up to ~20)


def _branch(raw_last):
    if raw_last == 0.0:
        return "last entry exactly 0: sign pattern of the trailing entries"
    return "last entry %+.1e: its sign" % raw_last


def check_columns(N, m, Bdev, cols, failures):
    """Residual, norm and orientation of the device's columns `cols` of block m (Bdev holds them in
    order) against T_m and the oracle's LAPACK block.  Returns how many of them LAPACK ended in an
    exact 0.0 while the device did not."""
    r = residual_ratio(N, m, Bdev, cols)
    for k in np.nonzero(r > RESIDUAL_C)[0]:
        failures.append("residual of column j=%d (el=%d, m=%d): %.1f eps |T| |b| > %g"
                        % (cols[k], m + cols[k], m, r[k], RESIDUAL_C))
    L, raw = oracle_block(N, m)
    L, raw = L[:, cols], raw[cols]
    dots = np.einsum("ij,ij->j", Bdev, L)
    diff = np.abs(Bdev - L).max(axis=0)
    for k in np.nonzero((dots <= 0) | (diff > 1e-12 * N))[0]:
        failures.append("column j=%d (el=%d, m=%d): b_dev . b_lapack = %.3e, max|b_dev - b_lapack| = %.3e; "
                        "orientation by LAPACK: %s, by the device: %s"
                        % (cols[k], m + cols[k], m, dots[k], diff[k], _branch(raw[k]),
                           _branch(0.0 if Bdev[-1, k] == 0.0 else Bdev[-1, k])))
    return int(np.count_nonzero((raw == 0.0) & (Bdev[-1] != 0.0)))


def _report(failures):
    return "\n".join(failures[:20]) + ("\n... %d failures in all" % len(failures) if len(failures) > 20 else "")


@contextlib.contextmanager
def downloaded_basis(N):
    """The device basis for N, downloaded once (quantization.get_basis) and dropped from the host
    cache afterwards, so that the 2.7-2.9 GB copies do not pile up across the session."""
    from quflow_amd import quantization as q
    try:
        yield q.get_basis(N)
    finally:
        q._basis_cache.pop((N, np.dtype(np.float64)), None)
        gc.collect()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 1025])
def test_device_basis_every_block(qfa, N):
    """Every block of the device basis: eigenpair residual at the exact eigenvalue -el(el+1),
    B_m^T B_m = N I (the gaps are >= 2, so together they bound each vector's error), and the signs
    and entries of every column against the oracle's LAPACK block."""
    failures = []
    zero_branch = 0
    t0 = time.time()
    with downloaded_basis(N) as basis:
        block = basis_blocks(basis, N)
        for m in range(N):
            B = block(m)
            n = N - m
            orth = np.abs(B.T @ B - N * np.eye(n)).max()
            if orth > 1e-11 * N * N:
                failures.append("block m=%d: max|B^T B - N I| = %.3e" % (m, orth))
            zero_branch += check_columns(N, m, B, np.arange(n), failures)
    assert not failures, _report(failures)
    print("N=%d: %d columns end in an exact 0.0 from LAPACK and not on the device; all %d columns have the "
          "same orientation on both sides (%.0f s)" % (N, zero_branch, N * (N + 1) // 2, time.time() - t0))


def _inputs(N, rng):
    """Real coefficients that decay with el (smooth) and that stay flat."""
    el = np.floor(np.sqrt(np.arange(N * N))).astype(np.float64)
    return {"smooth": rng.standard_normal(N * N) / (1.0 + el) ** 2, "flat": rng.standard_normal(N * N)}


def _n_omegas(N):
    """Coefficient counts whose band limit Nmax = J + m lands on both sides of the 32-, 64- and
    256-wide tile and chunk edges, with Nmax = 1, 2 and non-square lengths."""
    return [N * N, N * N - 1, (N // 2) ** 2, 257 ** 2, 256 ** 2, 255 ** 2 + 7, 33 ** 2, 32 ** 2, 4, 1]


ELMAX = [1, 4, 5, 15, 16, 31]      # mat2shr(W, elmax): band limits (elmax+1)^2 = 4, 25, 36, 256, 289, 1024


def _mat2shr_n(N, W, n):
    """The host-array mat2shr with an n-entry output (qf_mat2shr)."""
    from quflow_amd import _lib
    from quflow_amd import quantization as q
    from quflow_amd.context import ptr
    ctx = q._resident_context(N)
    om = np.zeros(n)
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, ptr(Wc), ptr(om), ctypes.c_longlong(n)))
    return om


EDGE_J = (0, 1, 31, 32, 63, 64, 255, 256, 257)


def _edge_ms(N):
    return sorted({m for m in (0, 1, 2, 31, 32, 33, 255, 256, 257, N // 2, N - 2, N - 1) if m < N})


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1000, 1024, 1025])
def test_transforms_vs_extended_precision(qfa, N):
    """shr2mat, mat2shr, shc2mat and mat2shc on the downloaded device basis, against the helper at
    every band limit of _n_omegas, on smooth and flat data; single modes at the tile and chunk
    edges bit for bit; the round trips."""
    from quflow_amd import quantization as q
    rng = np.random.default_rng(N)
    with downloaded_basis(N) as basis:
        block = basis_blocks(basis, N)
        inputs = _inputs(N, rng)
        G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        both = N == 1024        # elsewhere the kinds alternate along the list (host time)
        for c, n in enumerate(_n_omegas(N)):
            for kind, omega in list(inputs.items())[(0 if both else c % 2):(2 if both else c % 2 + 1)]:
                W = q.shr2mat(omega[:n], N=N)
                assert_W_within(W, ref_shr2mat(omega[:n], N, block), "shr2mat N=%d n_omega=%d %s" % (N, n, kind))
        Ws = q.shr2mat(inputs["smooth"], N=N)
        for c, n in enumerate(_n_omegas(N)):
            for kind, W in (("smooth", Ws), ("flat", G))[(0 if both else (c + 1) % 2):(2 if both else (c + 1) % 2 + 1)]:
                om = _mat2shr_n(N, W, n)
                assert_within(om, *ref_mat2shr(W, n, block), "mat2shr N=%d n_omega=%d %s" % (N, n, kind))
        for elmax in ELMAX:
            nout = (elmax + 1) ** 4
            om = q.mat2shr(G, elmax=elmax)
            assert om.shape == (nout,)
            assert_within(om, *ref_mat2shr(G, nout, block), "mat2shr N=%d elmax=%d" % (N, elmax))
        # round trip on the full band (the existing bar of the smaller sizes)
        omega = inputs["flat"]
        assert np.abs(q.mat2shr(q.shr2mat(omega, N=N)) - omega).max() <= 1e-11 * np.abs(omega).max()
        # complex coefficients: a general complex matrix, and back
        omc = q.mat2shc(G)
        assert_shc_within(omc, ref_mat2shc(G, block), "mat2shc N=%d" % N)
        omc_s = inputs["smooth"] + 1j * rng.standard_normal(N * N) / (1.0 + np.floor(np.sqrt(np.arange(N * N)))) ** 2
        for kind, oc in (("round trip", omc), ("smooth", omc_s)):
            Wc = q.shc2mat(oc, N=N)
            assert_W_within(Wc, ref_shc2mat(oc, N, block), "shc2mat N=%d %s" % (N, kind))
        assert np.abs(q.shc2mat(omc, N=N) - G).max() <= 1e-11 * np.abs(G).max()

        # single modes: omega = e_(el,m) reads out column j = el - m of B_m, times 1/sqrt2 (m > 0);
        # a single entry W[k+m, k] = 1j reads out row k of B_m
        for m in _edge_ms(N):
            n = N - m
            B = block(m)
            s = _sgn(m)
            i = np.arange(n)
            for j in sorted({jj for jj in EDGE_J + (n - 1,) if jj < n}):
                el = m + j
                for neg in ((False, True) if m else (False,)):
                    omega = np.zeros(N * N)
                    omega[_idx(el, -m if neg else m)] = 1.0
                    W = q.shr2mat(omega, N=N)
                    x = complex(1.0, 0.0) if m == 0 else (complex(0.0, -C1DSQ2) if neg else complex(C1DSQ2, 0.0))
                    diag = s * (B[:, j] * x)
                    want = np.zeros((N, N), dtype=complex)
                    want[i, i + m] = 1j * diag
                    if m:
                        want[i + m, i] = 1j * diag.conj()
                    np.testing.assert_array_equal(W, want, err_msg="shr2mat single mode el=%d m=%d" % (el, -m if neg else m))
            for k in sorted({kk for kk in (0, 1, 255, 256, 257, n - 1) if kk < n}):
                W = np.zeros((N, N), dtype=complex)
                W[k + m, k] = 1j
                om = q.mat2shr(W)
                want = np.zeros(N * N)
                els = np.arange(m, N)
                want[_idx(els, m)] = (B[k, :] / N) if m == 0 else (SQRT2 * s * B[k, :]) / N
                np.testing.assert_array_equal(om, want, err_msg="mat2shr single entry W[%d, %d]" % (k + m, k))


@pytest.mark.gpu
def test_resident_forms_vs_extended_precision(qfa):
    """DeviceTrajectory.from_shr and tr.shr(n) at N = 1024 (the forms behind a run's initial data and
    its 'shr' / 'funhalf' outputs) against the helper, and tr.shr(n) against the host-array form."""
    from quflow_amd import quantization as q
    N = 1024
    rng = np.random.default_rng(7)
    with downloaded_basis(N) as basis:
        block = basis_blocks(basis, N)
        for kind, omega in _inputs(N, rng).items():
            tr = qfa.DeviceTrajectory.from_shr(omega, N=N)
            try:
                W = tr.download()
                assert_W_within(W, ref_shr2mat(omega, N, block), "from_shr N=%d %s" % (N, kind))
                np.testing.assert_array_equal(W, q.shr2mat(omega, N=N))
                for n in ((N // 2) ** 2, N * N):
                    om = tr.shr(n)
                    assert_within(om, *ref_mat2shr(W, n, block), "tr.shr(%d) %s" % (n, kind))
                    np.testing.assert_array_equal(om, _mat2shr_n(N, W, n))
            finally:
                tr.ctx.close()


# ----------------------------------------------------------------------------- N = 2048, basis on the device only
N_BIG = 2048


def _sampled_ms(N):
    return sorted({m for m in (0, 1, 2, 3, 31, 32, 33, 255, 256, 257, N // 2, N - 2, N - 1) if m < N})


def _sampled_js(n):
    return sorted({j for j in (0, 1, 31, 32, 63, 64, 255, 256, 257, n - 1) if j < n})


@pytest.fixture(scope="module")
def ctx_big(qfa):
    """A context for N = 2048 with the basis computed on the device (qf_basis_compute) and never
    downloaded; closed, with its 23 GB, when the module ends."""
    from quflow_amd import _lib
    from quflow_amd.context import Context
    ctx = Context(N_BIG)
    try:
        _lib.check(ctx._lib.qf_basis_compute(ctx.handle))
        yield ctx
    finally:
        ctx.close()


def _big_shr2mat(ctx, omega):
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    om = np.ascontiguousarray(omega, dtype=np.float64)
    W = np.zeros((N_BIG, N_BIG), dtype=np.complex128)
    _lib.check(ctx._lib.qf_shr2mat(ctx.handle, ptr(om), ctypes.c_longlong(om.shape[0]), ptr(W)))
    return W


def _big_mat2shr(ctx, W, n):
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    om = np.zeros(n)
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, ptr(Wc), ptr(om), ctypes.c_longlong(n)))
    return om


def _big_mat2shc(ctx, G):
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    Gc = np.ascontiguousarray(G, dtype=np.complex128)
    om = np.zeros(N_BIG * N_BIG, dtype=np.complex128)
    _lib.check(ctx._lib.qf_mat2shc(ctx.handle, ptr(Gc), ptr(om)))
    return om


def _big_shc2mat(ctx, omega):
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    om = np.ascontiguousarray(omega, dtype=np.complex128)
    W = np.zeros((N_BIG, N_BIG), dtype=np.complex128)
    _lib.check(ctx._lib.qf_shc2mat(ctx.handle, ptr(om), ptr(W)))
    return W


@pytest.mark.gpu
def test_device_basis_2048_sampled_columns(qfa, ctx_big):
    """Sampled blocks of the N = 2048 basis.  A single entry W[N-1, n-1] = 1j reads out the last row of
    B_m through mat2shr (times sqrt2 sgn / N): every column's last entry, which decides its orientation,
    is held to the oracle's LAPACK block.  Single-mode shr2mat reads out columns (exact for m = 0, one
    rounding of 1/sqrt2 for m > 0): the sampled columns, and some whose last entry is an exact 0.0 on
    the device, are checked for residual, norm sqrt(N) and orientation.  Nothing else of W is touched."""
    N = N_BIG
    failures = []
    zero_branch = ncols = nlast = 0
    t0 = time.time()
    for m in _sampled_ms(N):
        n = N - m
        i = np.arange(n)
        s = _sgn(m)
        W = np.zeros((N, N), dtype=np.complex128)
        W[N - 1, n - 1] = 1j
        om = _big_mat2shr(ctx_big, W, N * N)
        els = np.arange(m, N)
        last = om[_idx(els, m)] * N / (1.0 if m == 0 else SQRT2 * s)
        L, raw = oracle_block(N, m)
        bad = np.nonzero(np.abs(last - L[-1]) > 1e-12 * N)[0]
        for j in bad[:5]:
            failures.append("last entry of column j=%d (el=%d, m=%d): device %.6e, LAPACK %.6e"
                            % (j, m + j, m, last[j], L[-1, j]))
        zero_branch += int(np.count_nonzero((raw == 0.0) & (last != 0.0)))
        nlast += n
        dev_zero = np.nonzero(last == 0.0)[0]
        js = sorted(set(_sampled_js(n)) | set(dev_zero[np.linspace(0, len(dev_zero) - 1, 6).astype(int)] if len(dev_zero) else []))
        cols = np.empty((n, len(js)))
        for c, j in enumerate(js):
            omega = np.zeros(N * N)
            omega[_idx(m + j, m)] = 1.0
            W = _big_shr2mat(ctx_big, omega)
            up = W[i, i + m].copy()
            assert np.all(up.real == 0.0)
            cols[:, c] = s * up.imag * (1.0 if m == 0 else SQRT2)
            if m:
                np.testing.assert_array_equal(W[i + m, i], up)       # 1j conj(d) = 1j d for a real d
            W[i, i + m] = 0.0
            W[i + m, i] = 0.0
            assert np.count_nonzero(W) == 0, "single mode (el=%d, m=%d) wrote outside diagonals +-m" % (m + j, m)
        norm2 = (cols * cols).sum(axis=0)
        for c in np.nonzero(np.abs(norm2 - N) > 1e-11 * N * N)[0]:
            failures.append("column j=%d (el=%d, m=%d): |b|^2 = %.15g, not N" % (js[c], m + js[c], m, norm2[c]))
        check_columns(N, m, cols, np.asarray(js), failures)
        ncols += len(js)
    assert not failures, _report(failures)
    print("N=%d: in the %d columns of the sampled blocks, %d end in an exact 0.0 from LAPACK and not on the "
          "device; the %d columns read out have the same orientation on both sides (%.0f s)"
          % (N, nlast, zero_branch, ncols, time.time() - t0))


@pytest.mark.gpu
def test_transforms_2048_sampled_blocks(qfa, ctx_big):
    """The four transforms at N = 2048 on the sampled blocks, against the helper on the oracle's LAPACK
    blocks: the bar is the helper's bound plus the basis bar 1e-12 N per entry times |x|."""
    N = N_BIG
    rng = np.random.default_rng(N)
    ms = _sampled_ms(N)
    blocks = {m: oracle_block(N, m)[0] for m in ms}
    block = blocks.__getitem__
    dB = 1e-12 * N

    def widen(ref, extra):
        Wr, Wi, br, bi = ref
        return Wr, Wi, br + extra, bi + extra

    inputs = _inputs(N, rng)
    for n in _n_omegas(N):
        Nmax = band_limit(N, n)
        for kind, omega in inputs.items():
            om = omega[:n]
            W = _big_shr2mat(ctx_big, om)
            ref = ref_shr2mat(om, N, block, ms)
            # basis error: |dB| @ |x| per entry of diagonal m, |x| <= |omega[el,m]| + |omega[el,-m]|
            extra = np.zeros((N, N))
            for m in ms:
                if m < Nmax:
                    els = np.arange(m, Nmax)
                    xs = np.abs(om[_idx(els, m)]).sum() + (np.abs(om[_idx(els, -m)]).sum() if m else 0.0)
                    i = np.arange(N - m)
                    extra[i, i + m] = extra[i + m, i] = dB * xs
            sel = np.zeros((N, N), dtype=bool)
            for m in ms:
                i = np.arange(N - m)
                sel[i, i + m] = sel[i + m, i] = True
            Wr, Wi, br, bi = widen(ref, extra)
            assert_within(W.real[sel], Wr[sel], br[sel], "shr2mat N=%d n_omega=%d %s (real)" % (N, n, kind))
            assert_within(W.imag[sel], Wi[sel], bi[sel], "shr2mat N=%d n_omega=%d %s (imag)" % (N, n, kind))
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    Ws = _big_shr2mat(ctx_big, inputs["smooth"])
    for n in _n_omegas(N):
        Nmax = band_limit(N, n)
        for kind, W in (("smooth", Ws), ("flat", G)):
            om = _big_mat2shr(ctx_big, W, n)
            ref, bnd = ref_mat2shr(W, n, block, ms)
            idx = []
            for m in ms:
                if m < Nmax:
                    els = np.arange(m, Nmax)
                    extra = dB * SQRT2 * np.abs(np.diagonal(W, -m)).sum() * 2 / N
                    bnd[_idx(els, m)] += extra
                    bnd[_idx(els, -m)] += extra
                    idx += [_idx(els, m), _idx(els, -m)]
            idx = np.concatenate(idx)
            assert_within(om[idx], ref[idx], bnd[idx], "mat2shr N=%d n_omega=%d %s" % (N, n, kind))
            assert np.count_nonzero(om[Nmax * Nmax:]) == 0
    omega = inputs["flat"]
    assert np.abs(_big_mat2shr(ctx_big, _big_shr2mat(ctx_big, omega), N * N) - omega).max() <= 1e-11 * np.abs(omega).max()
    # complex coefficients
    omc = _big_mat2shc(ctx_big, G)
    orr, oi, br, bi = ref_mat2shc(G, block, ms)
    Wc = _big_shc2mat(ctx_big, omc)
    assert np.abs(Wc - G).max() <= 1e-11 * np.abs(G).max()
    sel_o = []
    for m in ms:
        els = np.arange(m, N)
        extra = 2 * dB * max(np.abs(np.diagonal(G, -m)).sum(), np.abs(np.diagonal(G, m)).sum()) / N
        for key in ((m, -m) if m else (0,)):
            br[_idx(els, key)] += extra
            bi[_idx(els, key)] += extra
            sel_o.append(_idx(els, key))
    sel_o = np.concatenate(sel_o)
    assert_within(omc.real[sel_o], orr[sel_o], br[sel_o], "mat2shc N=%d (real)" % N)
    assert_within(omc.imag[sel_o], oi[sel_o], bi[sel_o], "mat2shc N=%d (imag)" % N)
    Wr, Wi, br, bi = ref_shc2mat(omc, N, block, ms)
    for m in ms:
        els = np.arange(m, N)
        i = np.arange(N - m)
        lo = np.abs(omc[_idx(els, m)]).sum() * 2 * dB
        br[i + m, i] += lo
        bi[i + m, i] += lo
        if m:
            hi = np.abs(omc[_idx(els, -m)]).sum() * 2 * dB
            br[i, i + m] += hi
            bi[i, i + m] += hi
        for (a, b) in ((i + m, i), (i, i + m)):
            assert_within(Wc.real[a, b], Wr[a, b], br[a, b], "shc2mat N=%d m=%d (real)" % (N, m))
            assert_within(Wc.imag[a, b], Wi[a, b], bi[a, b], "shc2mat N=%d m=%d (imag)" % (N, m))
