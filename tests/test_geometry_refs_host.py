"""Closed-form host references for the rotations and gradients at ANY size (no GPU, no fixture beyond the committed
N = 16 / 33 arrays that pin them here), shared with tests/test_hip_geometry_large.py.

R = exp(xi . S) is the spin-(N-1)/2 representation of the 2 x 2 matrix g = exp(xi . S^(2)).  From that, in np.longdouble:

  su2(xi)                     g = cos(theta/2) I + 2 sin(theta/2) (n . S^(2)): (n . S^(2))^2 = -I/4 for a unit vector n
  extreme_columns(xi, N)      R[r,0] = sqrt(C(N-1,r)) g00^(N-1-r) g10^r,  R[r,N-1] = sqrt(C(N-1,r)) g01^(N-1-r) g11^r, in
                              log space (modulus and phase apart, 0^0 = 1), O(N)
  taylor_reference(xi, N)     exp(B), B = xi . S with |B|_inf <= 0.5 (the device's sigma = 0 path): the Horner form of the
                              Taylor polynomial to a degree at which the next term is below 1e-22, on the band, O(40 N D)
  gen_tri / tri_dense /       a1 S1 + a2 S2 + a3 S3 as (lower, diagonal, upper) vectors; its products with a dense matrix
  tri_left / tri_right        are O(N^2)
  rotated_generators(xi, N)   rotate(xi, S_j) = sum_i Q_ij S_i (Q the Rodrigues matrix), as three such triples
  equivariance_error(R, xi)   max_j max|R S_j - S'_j R| in row blocks: with unitarity it fixes R up to a phase, the extreme
                              columns fix the phase
  closed_form_case(xi, N)     (W, want): W = (2/N)(a S1 + b S2 + e S3) + (2-1j) E_{0,N-1} + 1j E_{N-1,N-1} + E_{0,0} and
                              R W R^H by linearity: generators rotate by Q, E_{N-1,N-1} -> c c^H, E_{0,N-1} -> c0 c^H,
                              E_{0,0} -> c0 c0^H with c0, c the extreme columns
  grad_reference(P)           [S_k, P] as shifted, scaled copies of P with c_a = sqrt((a+1)(N-1-a)) in long double
"""
import functools
import math

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import geometry
from test_geometry_host import EPS, XIS, FIXTURE_SIZES, golden, plan_model, rot_tol, rodrigues   # noqa: F401  (golden: fixture)

LD = np.longdouble
CLD = np.clongdouble
EPS_LD = float(np.finfo(LD).eps)

CASE_COEF = (0.7, -1.3, 0.9)          # (a, b, e) of closed_form_case's W


# ---- the helpers ---------------------------------------------------------------------------------------------------------

def su2(xi):
    """g = exp(xi . S^(2)), 2 x 2 clongdouble."""
    x = np.array(xi, dtype=LD)
    theta = np.sqrt((x * x).sum())
    g = np.eye(2, dtype=CLD)
    if theta == 0:
        return g
    n = x / theta
    S = qfa.so3_generators(2)            # entries 0, +-1/2, +-i/2: exact
    nS = sum(n[k] * S[k].astype(CLD) for k in range(3))
    return np.cos(theta / 2) * g + 2 * np.sin(theta / 2) * nS


def _spin_column(u, v, N):
    """sqrt(C(N-1, r)) u^(N-1-r) v^r, r = 0..N-1, for complex long doubles u, v with |u|^2 + |v|^2 = 1."""
    r = np.arange(N, dtype=LD)
    k = np.arange(1, N, dtype=LD)
    logC = np.concatenate((np.zeros(1, dtype=LD), np.cumsum(np.log((LD(N) - k) / k))))
    log_mod = 0.5 * logC
    phase = np.zeros(N, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        for z, e in ((u, LD(N - 1) - r), (v, r)):
            log_mod = log_mod + np.where(e > 0, e * np.log(np.abs(z)), LD(0))        # 0^0 = 1, 0^e = 0
            phase = phase + e * np.arctan2(z.imag, z.real)
    return (np.exp(log_mod) * (np.cos(phase) + 1j * np.sin(phase))).astype(CLD)


def extreme_columns(xi, N):
    """(R[:, 0], R[:, N-1]) of R = exp(xi . S), clongdouble."""
    g = su2(xi)
    return _spin_column(g[0, 0], g[1, 0], N), _spin_column(g[0, 1], g[1, 1], N)


def so3_c(N):
    """c_a = sqrt((a+1)(N-1-a)), a = 0..N-2, long double."""
    a = np.arange(N - 1, dtype=LD)
    return np.sqrt((a + 1) * (LD(N - 1) - a))


def gen_tri(coef, N, dtype=np.complex128):
    """(lo, dg, up) of M = coef[0] S1 + coef[1] S2 + coef[2] S3: lo[a] = M[a+1,a], up[a] = M[a,a+1], a = 0..N-2."""
    a1, a2, a3 = (LD(c) for c in coef)
    half_c = so3_c(N) / 2
    dg = 1j * (a3 * (np.arange(N, dtype=LD) - LD(N - 1) / 2))
    up = (a2 + 1j * a1) * half_c
    lo = (-a2 + 1j * a1) * half_c
    return lo.astype(dtype), dg.astype(dtype), up.astype(dtype)


def tri_dense(tri):
    lo, dg, up = tri
    return np.diag(dg) + np.diag(up, 1) + np.diag(lo, -1)


def tri_left(tri, R, i0=0, i1=None):
    """Rows i0..i1-1 of M @ R."""
    lo, dg, up = tri
    N = R.shape[0]
    i1 = N if i1 is None else i1
    out = dg[i0:i1, None] * R[i0:i1]
    a0 = max(i0, 1)
    out[a0 - i0:] += lo[a0 - 1:i1 - 1, None] * R[a0 - 1:i1 - 1]
    a1 = min(i1, N - 1)
    out[:a1 - i0] += up[i0:a1, None] * R[i0 + 1:a1 + 1]
    return out


def tri_right(R, tri, i0=0, i1=None):
    """Rows i0..i1-1 of R @ M."""
    lo, dg, up = tri
    X = R[i0:i1]
    out = X * dg[None, :]
    out[:, 1:] += X[:, :-1] * up[None, :]
    out[:, :-1] += X[:, 1:] * lo[None, :]
    return out


def rotated_generators(xi, N):
    """The three matrices rotate(xi, S_j) = sum_i Q_ij S_i, each as a (lo, dg, up) triple."""
    Q = rodrigues(xi)
    return [gen_tri(Q[:, j], N) for j in range(3)]


def block_max(fn, N, block, threads=8):
    """Entrywise maximum over the row blocks [i0, i1) of the float arrays fn(i0, i1), the blocks spread over a few threads
    (numpy releases the interpreter lock inside its loops)."""
    from concurrent.futures import ThreadPoolExecutor
    spans = [(i0, min(N, i0 + block)) for i0 in range(0, N, block)]
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(spans)))) as pool:
        return functools.reduce(np.maximum, pool.map(lambda span: fn(*span), spans))


def equivariance_error(R, xi, block=256):
    """max over j and entries of |R S_j - S'_j R| (scale: |S_j| <= N/2), O(N^2), in row blocks."""
    N = R.shape[0]
    pairs = [(gen_tri(np.eye(3)[j], N), rotated) for j, rotated in enumerate(rotated_generators(xi, N))]

    def worst(i0, i1):
        out = 0.0
        for plain, rotated in pairs:
            d = tri_right(R, plain, i0, i1)
            d -= tri_left(rotated, R, i0, i1)
            out = max(out, float(np.abs(d).max()))
        return np.float64(out)
    return float(block_max(worst, N, block))


def taylor_degree(b0):
    D = 1
    while b0 ** D / math.factorial(D) >= 1e-22:
        D += 1
    return D


def taylor_reference(xi, N):
    """exp(xi . S) for |xi . S|_inf <= 0.5 as a dense clongdouble matrix: T <- I + B T / k, k = D..1, on the band
    |r - j| <= D (the degree-D polynomial of a tridiagonal matrix has no entry outside it)."""
    b0 = plan_model(N, xi)[2]
    assert b0 <= 0.5, "taylor_reference is the reference of the unscaled path only"
    D = taylor_degree(b0)
    lo, dg, up = gen_tri(xi, N, dtype=CLD)
    w = np.arange(2 * D + 1)[:, None]
    j = np.arange(N)[None, :]
    r = j - D + w                                        # Tb[w, j] = T[r, j]
    ok = (r >= 0) & (r < N)
    rc = np.clip(r, 0, N - 1)
    pad = np.zeros(1, dtype=CLD)
    Bd = np.where(ok, dg[rc], 0)
    Bl = np.where(ok, np.concatenate((pad, lo))[rc], 0)          # B[r, r-1] = lo[r-1], 0 at r = 0
    Bu = np.where(ok, np.concatenate((up, pad))[rc], 0)          # B[r, r+1] = up[r],   0 at r = N-1
    eye = ((r == j) & ok).astype(CLD)
    Tb = eye.copy()
    zrow = np.zeros((1, N), dtype=CLD)
    for k in range(D, 0, -1):
        BT = Bd * Tb + Bl * np.concatenate((zrow, Tb[:-1])) + Bu * np.concatenate((Tb[1:], zrow))
        Tb = eye + BT / LD(k)
    out = np.zeros((N, N), dtype=CLD)
    jj = np.broadcast_to(j, r.shape)
    out[r[ok], jj[ok]] = Tb[ok]
    return out


def closed_form_case(xi, N, coef=CASE_COEF):
    """(W, want = R W R^H), complex128, O(N^2).  W is neither Hermitian nor skew-Hermitian, with entries of order 1 on the
    band and in three corners."""
    W = (2.0 / N) * tri_dense(gen_tri(coef, N))
    W[0, N - 1] += 2 - 1j
    W[N - 1, N - 1] += 1j
    W[0, 0] += 1
    c0, c = (col.astype(np.complex128) for col in extreme_columns(xi, N))
    want = (2.0 / N) * tri_dense(gen_tri(rodrigues(xi) @ np.array(coef), N))
    want += np.outer((2 - 1j) * c0 + 1j * c, c.conj())
    want += np.outer(c0, c0.conj())
    return W, want


def grad_reference(P, i0=0, i1=None):
    """Rows i0..i1-1 of the three commutators [S_k, P], (3, i1 - i0, N) clongdouble:
    [S1,P] = (i/2) u, [S2,P] = v/2, u, v = c_a P[a+1,b] +- c_{a-1} P[a-1,b] - c_{b-1} P[a,b-1] -+ c_b P[a,b+1],
    [S3,P]_ab = i (a - b) P_ab."""
    P = np.asarray(P)
    N = P.shape[0]
    i1 = N if i1 is None else i1
    half_c = np.concatenate((np.zeros(1, dtype=LD), so3_c(N) / 2, np.zeros(1, dtype=LD)))     # [a + 1] = c_a / 2; c_{-1} = c_{N-1} = 0
    rows = np.arange(i0, i1)

    def parts(A):                                        # (rows, N, 2) long double: real weights meet real arrays only
        return np.stack((A.real, A.imag), axis=-1).astype(LD)
    X = parts(P[i0:i1])
    lo, hi = max(i0 - 1, 0), min(i1 + 1, N)
    halo = np.zeros((i1 - i0 + 2, N + 2, 2), dtype=LD)   # P[i0-1 .. i1, -1 .. N], zero outside the matrix
    halo[lo - i0 + 1:hi - i0 + 1, 1:N + 1] = parts(P[lo:hi])
    p1 = half_c[rows + 1][:, None, None] * halo[2:, 1:N + 1]         # c_a P[a+1,b] / 2
    p2 = half_c[rows][:, None, None] * halo[:-2, 1:N + 1]            # c_{a-1} P[a-1,b] / 2
    p3 = half_c[0:N][None, :, None] * halo[1:-1, 0:N]                # c_{b-1} P[a,b-1] / 2
    p4 = half_c[1:N + 1][None, :, None] * halo[1:-1, 2:]             # c_b P[a,b+1] / 2
    m = (rows.astype(LD)[:, None] - np.arange(N, dtype=LD)[None, :])[:, :, None] * X
    s13, s24 = p1 - p3, p2 - p4
    u, v = s13 + s24, s13 - s24
    out = np.empty((3, i1 - i0, N), dtype=CLD)
    for k, (re, im) in enumerate(((-u[..., 1], u[..., 0]), (v[..., 0], v[..., 1]), (-m[..., 1], m[..., 0]))):
        out[k].real = re
        out[k].imag = im
    return out


# ---- the pins ------------------------------------------------------------------------------------------------------------

def test_long_double_is_extended():
    """The phases of the extreme columns at N = 8192 are 8191 arguments added up: they need the 64-bit mantissa."""
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_extreme_columns_against_reference(golden, N):
    for i, xi in enumerate(XIS):
        R = golden["expm_%d_%d" % (i, N)]
        c0, c = extreme_columns(xi, N)
        err = max(np.abs(c0 - R[:, 0]).max(), np.abs(c - R[:, -1]).max())
        print("extreme columns vs expm  N=%d xi=%s  max err = %.3e = %.2f eps" % (N, xi, err, err / EPS))
        assert err <= 16 * EPS


@pytest.mark.parametrize("N", (1025, 4096, 8192))
def test_extreme_columns_have_unit_norm(N):
    for xi in XIS + (np.array((25.0, -20.0, 24.0)),):
        for col in extreme_columns(xi, N):
            assert col.dtype == CLD
            defect = abs(float((np.abs(col) ** 2).sum() - 1))
            assert defect <= 64 * EPS, (N, xi, defect)


@pytest.mark.parametrize("N", (2, 5, 33, 4096))
def test_extreme_columns_of_a_z_rotation(N):
    """S3 = i diag(a - s): R = diag(exp(i xi3 (a - s))), so column 0 is exp(-i xi3 s) e_0 and column N-1 exp(+i xi3 s) e_{N-1}."""
    s = LD(N - 1) / 2
    for xi3 in (2.5, -0.4):
        c0, c = extreme_columns([0.0, 0.0, xi3], N)
        want0 = np.zeros(N, dtype=CLD)
        want0[0] = np.cos(xi3 * s) - 1j * np.sin(xi3 * s)
        want = np.zeros(N, dtype=CLD)
        want[-1] = np.cos(xi3 * s) + 1j * np.sin(xi3 * s)
        assert np.abs(c0 - want0).max() <= 4 * N * EPS_LD and np.abs(c - want).max() <= 4 * N * EPS_LD
        assert np.all(c0[1:] == 0) and np.all(c[:-1] == 0)


def small_xi(N, target, xi=XIS[0]):
    """xi scaled so that |xi . S|_inf = target."""
    return np.asarray(xi) * (target / plan_model(N, xi)[2])


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_taylor_reference_against_expm(N):
    """Against scipy's expm of the dense xi . S where scipy imports, against an eigh reconstruction of the skew-Hermitian
    B otherwise.  Either reference sums N products per entry of a matrix with entries <= 1: N eps."""
    for target in (0.48, 1e-3):
        xi = small_xi(N, target)
        assert geometry.exp_plan(xi, N)[0] == 0
        S = qfa.so3_generators(N)
        B = xi[0] * S[0] + xi[1] * S[1] + xi[2] * S[2]
        try:
            from scipy.linalg import expm
            want = expm(B)
        except ImportError:
            lam, V = np.linalg.eigh(-1j * B)
            want = (V * np.exp(1j * lam)) @ V.conj().T
        T = taylor_reference(xi, N)
        assert T.dtype == CLD
        err = float(np.abs(T - want).max())
        print("taylor_reference vs dense exponential  N=%d |B|=%.3g  max err = %.2f eps" % (N, target, err / EPS))
        assert err <= N * EPS
        assert float(np.abs(T @ T.conj().T - np.eye(N)).max()) <= 64 * EPS_LD      # unitary to ITS precision


@pytest.mark.parametrize("N", (33, 257))
def test_grad_reference_against_dense_generators(N):
    rng = np.random.default_rng(N)
    P = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    S = qfa.so3_generators(N)
    ref = grad_reference(P)
    assert ref.shape == (3, N, N) and ref.dtype == CLD
    for k in range(3):
        want = S[k] @ P - P @ S[k]
        # the dense double side: four nonzero terms per entry, each |S| |P| <= N/2 max|P|
        assert float(np.abs(ref[k] - want).max()) <= 4 * EPS * N / 2 * np.abs(P).max(), k
    blocks = np.concatenate([grad_reference(P, i0, min(N, i0 + 16)) for i0 in range(0, N, 16)], axis=1)
    assert np.array_equal(blocks, ref)


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_tridiagonal_helpers(N):
    S = qfa.so3_generators(N)
    rng = np.random.default_rng(N)
    R = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    coef = np.array(CASE_COEF)
    tri = gen_tri(coef, N)
    M = sum(coef[k] * S[k] for k in range(3))
    assert np.abs(tri_dense(tri) - M).max() <= 4 * EPS * N / 2
    assert np.abs(tri_left(tri, R) - M @ R).max() <= 8 * EPS * N / 2 * np.abs(R).max()
    assert np.abs(tri_right(R, tri) - R @ M).max() <= 8 * EPS * N / 2 * np.abs(R).max()
    assert np.array_equal(np.concatenate([tri_left(tri, R, i, min(N, i + 5)) for i in range(0, N, 5)]), tri_left(tri, R))
    assert np.array_equal(np.concatenate([tri_right(R, tri, i, min(N, i + 5)) for i in range(0, N, 5)]), tri_right(R, tri))


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_equivariance_error_on_the_reference(golden, N):
    for i, xi in enumerate(XIS):
        R = golden["expm_%d_%d" % (i, N)]
        err = equivariance_error(R, xi, block=7)
        assert err <= rot_tol(N, xi, N / 2)
        # and it sees a wrong matrix: one interior entry off by 1e-9
        bad = R.copy()
        bad[N // 2, N // 3] += 1e-9
        assert equivariance_error(bad, xi, block=7) > rot_tol(N, xi, N / 2)


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_closed_form_case_against_reference(golden, N):
    for i, xi in enumerate(XIS):
        R = golden["expm_%d_%d" % (i, N)]
        W, want = closed_form_case(xi, N)
        assert np.abs(W - W.conj().T).max() > 0.5 and np.abs(W + W.conj().T).max() > 0.5
        direct = R @ W @ R.conj().T
        assert np.abs(want - direct).max() <= rot_tol(N, xi, np.abs(want).max())
