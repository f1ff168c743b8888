"""Host side of quflow_amd.transforms (no GPU needed), and the independent evaluator of the synthesis that the device tests
(tests/test_hip_sht.py) compare against.

* shr2shc, shc2shr, sphgrid, fun2img, img2fun against tests/golden/transforms.npz, made by the reference itself
  (tools/gen_transforms_golden.py) on inputs rebuilt here from integer hashes; the outputs must match bit for bit (SHA-256
  of their bytes), and the argument rules of the reference.
* The evaluator: f = sqrt(4 pi) sum w_l a_lm Y_lm on the MW grid in np.longdouble.  lambda_lm(theta) comes from the
  normalised three-term recurrence in l, vectorised over rings, with an explicit binary exponent per ring (np.frexp /
  np.ldexp) so that sin^m theta at m = 8191 (~1e-30000, below even the long double range) is carried exactly; the ring
  transform is an explicit DFT.  It is pinned here to scipy.special.sph_harm_y for every (l, m) at L <= 24 and to the three
  l = 1 closed forms.  Its own error is that of long double arithmetic (~1e-19 relative per operation), far below fp64.
* Rings: theta_t = pi q_t with q_t = (2t+1)/(2L-1) ROUNDED TO FLOAT64, the argument the device hands to sincospi; the
  evaluator then sees the same sample points as the device and differs from it only by arithmetic.
"""
import hashlib
import os

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import transforms as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transforms.npz")
LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
FOURPI = 4 * PI


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------------

def ring_q(L):
    """q_t = (2t+1)/(2L-1) as float64: theta_t = pi q_t."""
    return (2.0 * np.arange(L) + 1.0) / (2.0 * L - 1.0)


def cospi_sinpi(q):
    """cos(pi q), sin(pi q) in long double with sincospi's exact reduction: sin(pi q) = sin(pi (1 - q)) with 1 - q exact,
    so that the south pole q = 1 has sin = 0 exactly (long double pi is not pi: sin(PI) is ~5e-20)."""
    q = np.asarray(q, dtype=np.float64).astype(LD)
    upper = q > 0.5
    r = np.where(upper, 1 - q, q)
    return np.where(upper, -np.cos(PI * r), np.cos(PI * r)), np.sin(PI * r)


def berezin_ld(L):
    """w_l = sqrt(prod_{j=1..l} (L-j)/(L+j)) in long double: what berezin_multipliers(L) (utils.py:108-135) computes
    through log-gamma."""
    w2 = np.ones(L, dtype=LD)
    for el in range(1, L):
        w2[el] = w2[el - 1] * (LD(L - el) / LD(L + el))
    return np.sqrt(w2)


def lambda_iter(m, q):
    """Yields (l, mantissa, exponent) for l = m, m+1, ...: lambda_lm(pi q_t) = mantissa * 2**exponent at every ring
    (arrays over q), long double mantissa renormalised at every degree."""
    x, s = cospi_sinpi(q)
    sm, se = np.frexp(s)
    prod = LD(1)
    for k in range(1, m + 1):
        prod *= LD(2 * k - 1) / LD(2 * k)
    c = np.sqrt(LD(2 * m + 1) / FOURPI * prod) * (-1 if m % 2 else 1)
    p1, d = np.frexp(sm ** m)            # sin^m = sm^m 2^(m se); sm^m >= 2^-m stays in range
    E = se.astype(np.int64) * m + d
    p1 = p1 * c
    p2 = np.zeros_like(p1)
    el = m
    yield el, p1, E
    while True:
        el += 1
        a = np.sqrt(LD(4 * el * el - 1) / LD((el - m) * (el + m)))
        b = np.sqrt(LD((el - 1 - m) * (el - 1 + m)) / LD(4 * (el - 1) * (el - 1) - 1))
        p = a * (x * p1 - b * p2)
        mant, d = np.frexp(p)
        p2 = np.ldexp(p1, -d)
        p1 = mant
        E = E + d
        yield el, p1, E


def lambda_rows(m, lmax, q):
    """lambda_lm(theta_t) for l = m..lmax (rows) at the rings q (columns), long double (values below its range are 0)."""
    out = np.empty((lmax - m + 1, len(q)), dtype=LD)
    for el, mant, E in lambda_iter(m, q):
        if el > lmax:
            break
        out[el - m] = np.ldexp(mant, E)
    return out


def lambda_at(el, m, q):
    """lambda_lm at the rings q as (mantissa, exponent): exact far below every floating-point range."""
    for ell, mant, E in lambda_iter(m, q):
        if ell == el:
            return mant, E


def padded(omega, L):
    om = np.zeros(L * L, dtype=np.clongdouble)
    n = min(len(omega), L * L)
    om[:n] = np.asarray(omega)[:n]
    return om


def synth_ref(omega, L, isreal, berezin):
    """shc2fun(omega, isreal, N=L, berezin) in long double: (L, 2L-1) real (isreal) or complex."""
    a = padded(omega, L)
    w = berezin_ld(L) if berezin else np.ones(L, dtype=LD)
    el = np.floor(np.sqrt(np.arange(L * L))).astype(np.int64)
    a = a * (np.sqrt(FOURPI) * w[el])
    q = ring_q(L)
    P = 2 * L - 1
    Gp = np.zeros((L, L), dtype=np.clongdouble)     # [m, t]: sum_l a_lm lambda_lm
    Gm = np.zeros((L, L), dtype=np.clongdouble)     # [m, t]: sum_l a_l,-m lambda_l,-m,  lambda_l,-m = (-1)^m lambda_lm
    for m in range(L):
        lam = lambda_rows(m, L - 1, q)
        ls = np.arange(m, L)
        Gp[m] = a[ls * ls + ls + m] @ lam
        if m > 0:
            Gm[m] = ((-1) ** m * a[ls * ls + ls - m]) @ lam
    k = (np.arange(L)[:, None] * np.arange(P)[None, :]) % P          # exact reduction of m p mod (2L-1)
    ang = 2 * PI * k.astype(LD) / P
    cs, sn = np.cos(ang), np.sin(ang)
    if isreal:
        # f = sum_l Re(a_l0) lambda_l0 + 2 sum_{m>0} Re(G_m e^{i m phi})
        wm = np.full(L, 2, dtype=LD)
        wm[0] = 1
        return (wm[:, None] * Gp.real).T @ cs - (wm[:, None] * Gp.imag).T @ sn
    e = cs + 1j * sn
    return Gp.T @ e + Gm.T @ np.conj(e)


def real_term(el, m, a, L, rows=None, cols=None):
    """The contribution w_m Re(a lambda_lm(theta_t) e^{i m phi_p}) (w_0 = 1, w_m = 2) of ONE complex coefficient a_lm,
    m >= 0, to a real synthesis (berezin=False), at the rings `rows` x the columns `cols`; also its scale per ring,
    w_m |a| (lambda_lm^2 + lambda_l-1,m^2)^(1/2): the size of the pair a recurrence in l carries, which its rounding errors
    are relative to (lambda_lm alone passes through zero between rings in the oscillatory region).  Long double."""
    P = 2 * L - 1
    rows = np.arange(L) if rows is None else np.asarray(rows)
    cols = np.arange(P) if cols is None else np.asarray(cols)
    prev = np.zeros(len(rows), dtype=LD)
    for ell, mant, E in lambda_iter(m, ring_q(L)[rows]):
        lam = np.ldexp(mant, E)
        if ell == el:
            break
        prev = lam
    ang = 2 * PI * ((m * cols) % P).astype(LD) / P
    w = LD(1 if m == 0 else 2)
    av = np.clongdouble(a) * np.sqrt(FOURPI)
    val = w * (av.real * np.outer(lam, np.cos(ang)) - av.imag * np.outer(lam, np.sin(ang)))
    return val, w * abs(av) * np.sqrt(lam * lam + prev * prev)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator against independent references
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 2, 7, 24])
def test_evaluator_legendre_vs_scipy(L):
    from scipy.special import sph_harm_y
    q = ring_q(L)
    theta = np.pi * q
    for m in range(L):
        lam = lambda_rows(m, L - 1, q).astype(np.float64)
        for el in range(m, L):
            Y = sph_harm_y(el, m, theta, 0.0)
            np.testing.assert_allclose(lam[el - m], Y.real, rtol=0, atol=1e-13, err_msg="(l, m) = (%d, %d)" % (el, m))


@pytest.mark.parametrize("L", [3, 24])
def test_evaluator_synthesis_vs_scipy(L):
    """Every unit coefficient (l, m), -l <= m <= l, synthesised by the evaluator equals sqrt(4 pi) Y_lm on the grid."""
    from scipy.special import sph_harm_y
    theta, phi = T.sphgrid(L)
    for ind in range(L * L):
        el = int(np.floor(np.sqrt(ind)))
        m = ind - el * el - el
        om = np.zeros(L * L, dtype=complex)
        om[ind] = 1.0
        f = synth_ref(om, L, isreal=False, berezin=False)
        Y = np.sqrt(4 * np.pi) * sph_harm_y(el, m, theta, phi)
        np.testing.assert_allclose(f.astype(np.complex128), Y, rtol=0, atol=1e-12, err_msg="(l, m) = (%d, %d)" % (el, m))


def test_evaluator_l1_closed_forms():
    """Unit shr coefficients at l = 1 (berezin=False): sqrt(3) cos(theta), sqrt(3) sin(theta) cos(phi),
    -sqrt(3) sin(theta) sin(phi) for m = 0, 1, -1."""
    L = 5
    theta = PI * ring_q(L).astype(LD)
    phi = 2 * PI * np.arange(2 * L - 1).astype(LD) / (2 * L - 1)
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    r3 = np.sqrt(LD(3))
    want = {0: r3 * np.cos(th), 1: r3 * np.sin(th) * np.cos(ph), -1: -r3 * np.sin(th) * np.sin(ph)}
    for m, w in want.items():
        om = np.zeros(L * L)
        om[qfa.elm2ind(1, m)] = 1.0
        # (bar: shr2shc's float64 factor 1/sqrt(2) carries one rounding, 1.1e-16 relative)
        f = synth_ref(T.shr2shc(om), L, isreal=True, berezin=False)
        assert np.abs(f - w).max() < 1e-15, (m, float(np.abs(f - w).max()))
        # the complex synthesis of the same (real) function agrees and is real
        fc = synth_ref(T.shr2shc(om), L, isreal=False, berezin=False)
        assert np.abs(fc.real - w).max() < 1e-15 and np.abs(fc.imag).max() < 1e-15, m


def test_evaluator_tracks_exponents_below_every_range():
    """lambda_{L-1,L-1} at the first ring for L = 8192 is ~1e-30000: the mantissa / exponent pair holds it exactly (its
    log10 matches the closed form log10|c_m| + m log10 sin(theta)), where the value itself would be 0."""
    L = 8192
    m = L - 1
    q = ring_q(L)[:1]
    mant, E = lambda_at(m, m, q)
    log10 = np.log10(np.abs(mant.astype(np.float64))) + E * np.log10(2.0)
    prod = np.exp(np.sum(np.log(np.arange(1, 2 * m, 2, dtype=np.float64)) - np.log(np.arange(2, 2 * m + 1, 2, dtype=np.float64))))
    want = 0.5 * np.log10((2 * m + 1) / (4 * np.pi) * prod) + m * np.log10(np.sin(np.pi * q))
    assert abs(log10[0] - want[0]) < 1e-9 and log10[0] < -29000, (log10, want)
    assert np.ldexp(mant, E)[0] == 0


@pytest.mark.parametrize("L", [16, 300, 512])
def test_berezin_product_is_the_reference_multiplier(L):
    """The long double product the device uses for w_l equals berezin_multipliers(L) (the reference's log-gamma form) to
    that form's own rounding: ~|lgamma| eps relative."""
    w_ref = qfa.berezin_multipliers(L)
    el = np.floor(np.sqrt(np.arange(L * L))).astype(int)
    w = berezin_ld(L)[el].astype(np.float64)
    big = w_ref > 1e-200
    rel = np.abs(w[big] - w_ref[big]) / w_ref[big]
    assert rel.max() < 1e-12, rel.max()


# ---------------------------------------------------------------------------------------------------------------------
# host transforms against the reference
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def det_values(n, salt):
    """The fixture's inputs, rebuilt bit for bit from integer hashes (as tools/gen_transforms_golden.py makes them)."""
    k = np.arange(n, dtype=np.int64)
    v = (k * 2654435761 + (salt + 1) * 40503) % 2147483647
    return (v / 2147483647.0 - 0.5) * 4.0


def det_image(shape, salt):
    k = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((k * 2654435761 + (salt + 1) * 40503) % 2147483647 % 256).astype(np.uint8).reshape(shape)


def expect(gold, key, got):
    """`got` is the reference's output `key` bit for bit: dtype, shape and the SHA-256 digest of its bytes (and the stored
    array itself where the fixture keeps it, for a readable difference)."""
    got = np.ascontiguousarray(got)
    if key in gold.files:
        np.testing.assert_array_equal(got, gold[key])
    assert str(got.dtype) == str(gold[key + "__dtype"]), key
    assert got.shape == tuple(gold[key + "__shape"]), key
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(gold[key + "__sha256"]), key


@pytest.mark.parametrize("N", [17, 128])
def test_shr2shc_shc2shr_vs_reference(gold, N):
    omr = det_values(N * N, 1)
    omc = det_values(N * N, 2) + 1j * det_values(N * N, 3)
    expect(gold, "shr2shc_%d" % N, T.shr2shc(omr))
    expect(gold, "shc2shr_%d" % N, T.shc2shr(omc))
    expect(gold, "shc2shr_shr2shc_%d" % N, T.shc2shr(T.shr2shc(omr)))
    expect(gold, "shr2shc_shc2shr_%d" % N, T.shr2shc(T.shc2shr(T.shr2shc(omr))))
    # the reference tests' round trips (quflow/tests/test_transforms.py:29-43)
    np.testing.assert_allclose(T.shc2shr(T.shr2shc(omr)), omr)
    c = T.shr2shc(omr)
    np.testing.assert_allclose(T.shr2shc(T.shc2shr(c)), c)


@pytest.mark.parametrize("n", [5, 12, 30])
def test_shr2shc_cut_short_lengths(gold, n):
    expect(gold, "shr2shc_n%d" % n, T.shr2shc(det_values(n, 6)))


@pytest.mark.parametrize("n", [0, 3, 7, 8, 13, 14, 31])
def test_shr2shc_lengths_the_reference_refuses(n):
    """The reference's loops index past a last degree cut short (IndexError) at exactly these lengths."""
    with pytest.raises(IndexError):
        T.shr2shc(np.ones(n))
    with pytest.raises(IndexError):
        T.shc2shr(np.ones(n, dtype=complex))


@pytest.mark.parametrize("N", [17, 128])
def test_sphgrid_fun2img_img2fun_vs_reference(gold, N):
    theta, phi = T.sphgrid(N)
    expect(gold, "sphgrid_theta_%d" % N, theta)
    expect(gold, "sphgrid_phi_%d" % N, phi)
    f = det_values(N * (2 * N - 1), 4).reshape(N, 2 * N - 1)
    expect(gold, "fun2img_%d" % N, T.fun2img(f))
    expect(gold, "fun2img_lim_%d" % N, T.fun2img(f, lim=(-0.5, 1.5)))
    expect(gold, "fun2img_sym_%d" % N, T.fun2img(f, lim=0.75))
    img = det_image((N, 2 * N - 1), 5)
    expect(gold, "img2fun_%d" % N, T.img2fun(img))
    expect(gold, "img2fun_lim_%d" % N, T.img2fun(img, lim=(-2.0, 3.0)))


def test_package_exports_transforms():
    for name in ("shr2fun", "shc2fun", "shr2shc", "shc2shr", "as_fun", "as_shr", "sphgrid", "fun2img", "img2fun",
                 "fun2shr", "fun2shc"):
        assert getattr(qfa, name) is getattr(T, name), name
    assert qfa.transforms is T


def test_analysis_is_refused_by_name():
    f = np.zeros((4, 7))
    with pytest.raises(NotImplementedError, match="fun2shr"):
        T.fun2shr(f)
    with pytest.raises(NotImplementedError, match="fun2shc"):
        T.fun2shc(f)
    with pytest.raises(NotImplementedError, match="fun2shr"):
        T.as_shr(f)
    with pytest.raises(NotImplementedError, match="fun2shr"):
        T.as_shr(np.zeros((4, 7), dtype=np.uint8))


def test_host_dispatch_branches():
    f = np.random.default_rng(0).standard_normal((4, 7))
    assert T.as_fun(f) is not None and np.array_equal(T.as_fun(f), f)
    img = np.arange(28, dtype=np.uint8).reshape(4, 7)
    np.testing.assert_array_equal(T.as_fun(img), T.img2fun(img))
    omr = np.random.default_rng(1).standard_normal(16)
    assert T.as_shr(omr) is omr or np.array_equal(T.as_shr(omr), omr)
    omc = T.shr2shc(omr)
    np.testing.assert_array_equal(T.as_shr(omc), T.shc2shr(omc))


def test_synthesis_argument_rules_on_the_host():
    """What is refused before any device work: a non-square length with N = -1 (the reference's assert), a bandwidth
    outside 1..8192, complex input to shr2fun."""
    with pytest.raises(AssertionError, match="right length"):
        T.shc2fun(np.ones(5, dtype=complex))
    with pytest.raises(AssertionError, match="right length"):
        T.shr2fun(np.ones(12))
    with pytest.raises(ValueError, match="outside 1..8192"):
        T.shc2fun(np.ones(4, dtype=complex), N=8193)
    with pytest.raises(ValueError, match="outside 1..8192"):
        T.shr2fun(np.ones(4), N=0)
    with pytest.raises(AssertionError, match="real"):
        T.shr2fun(np.ones(4, dtype=complex))
    with pytest.raises(IndexError):
        T.shr2fun(np.ones(7), N=3)
