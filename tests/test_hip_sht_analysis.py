"""Spherical-harmonic ANALYSIS on the device (quflow_amd.sht: fun2shc, fun2shr, as_shr; DeviceTrajectory.from_fun;
quflow_amd.analysis on `fun` data; kernels in quflow_amd/csrc/sht.hip) against the evaluators of
tests/test_sht_analysis_host.py and tests/test_transforms_host.py.

Bar, per coefficient, from the input and the arithmetic and never from the device output:
    |omega_dev - omega_ref| <= C_DEVICE L eps ||f||_2,
||f||_2 the L2(S^2) norm of the input over sqrt(4 pi): ||omega||_2 for band-limited input, so 1 in the dense cases and
sqrt(n) for n superposed unit harmonics.  C_DEVICE = 8 x the worst ratio of the fp64 numpy reference analysis_fp64
(test_sht_analysis_host.py: RATIO_FP64, measured there), the same at every L.  For the grids that are not band-limited
that norm is not defined; there the scale is S_lm = (2 pi/P)/sqrt(4 pi) sum_t |lambda_lm| sum_t' |Q[t,t']| |F_m(t')|,
formed by the evaluator from the input.  Each case prints max err and max err / bar.

Small L is checked against analysis_ref (long double, dense).  At large L the input is independent of the device: a dozen
single harmonics per L, made by the long double recurrence at every ring and superposed in one grid, must come back as
unit coefficients with zeros everywhere else -- every 256-ring block, both halves of every Legendre workgroup, every tile
and edge tile of the two GEMMs, the seeds that underflow (m ~ 8000) and the leak into every other coefficient; and dense
coefficient sets go through the device synthesis with berezin=False (held to the evaluator by test_hip_sht_large.py;
Berezin data would be blind from l ~ 3300 at L = 8192, see there) and must come back.
"""
import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import sht
from quflow_amd import transforms as T

from test_transforms_host import FOURPI, LD, lambda_iter, ring_q, det_values
from test_sht_analysis_host import C_DEVICE, SMALL_LS, analysis_ref, white, GOLD

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LARGE_LS = (511, 512, 513, 1024, 2047, 2048, 4096, 8192)


def report(label, err, bar):
    ratio = float(np.max(err / bar))
    print("%-46s max err %.2e   err/bar %.3f" % (label, float(np.max(err)), ratio))
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# small L: every coefficient against the long double evaluator
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("L", SMALL_LS)
def test_small_band_limited(L, isreal):
    om = white(L, 300 + L, cplx=not isreal)
    f = np.ascontiguousarray(T.shc2fun(om, isreal=isreal, N=L, berezin=False))
    ref = analysis_ref(f, L)
    norm = float(np.sqrt((np.abs(ref) ** 2).sum()))
    got = sht.fun2shc(f)
    assert got.dtype == np.complex128 and got.shape == (L * L,)
    err = np.abs(got - ref).astype(np.float64)
    assert report("band-limited L=%d %s" % (L, "real" if isreal else "complex"), err, C_DEVICE * L * EPS * norm) <= 1.0
    # fun2shr is shc2shr of it bit for bit; two calls give the same bits
    assert sht.fun2shr(f).tobytes() == T.shc2shr(got).tobytes()
    assert sht.fun2shc(f).tobytes() == got.tobytes()


@pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("L", SMALL_LS)
def test_small_arbitrary_grid(L, isreal):
    """A random grid is not band-limited: the part of the map that a round trip never sees."""
    rng = np.random.default_rng(500 + L)
    f = rng.standard_normal((L, 2 * L - 1))
    if not isreal:
        f = f + 1j * rng.standard_normal((L, 2 * L - 1))
    ref, S = analysis_ref(f, L, scales=True)
    got = sht.fun2shc(f)
    err = np.abs(got - ref).astype(np.float64)
    assert report("arbitrary grid L=%d %s" % (L, "real" if isreal else "complex"), err, C_DEVICE * L * EPS * S + 1e-300) <= 1.0
    if isreal:
        el = np.floor(np.sqrt(np.arange(L * L))).astype(np.int64)
        m = np.arange(L * L) - el * el - el
        mirror = np.where(m % 2 == 0, 1, -1) * np.conj(got[el * el + el - m])
        assert np.array_equal(got, mirror)
    assert sht.fun2shr(f).tobytes() == T.shc2shr(got).tobytes()
    assert sht.fun2shc(f).tobytes() == got.tobytes()


@pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])
def test_operator_cache_across_bandwidths(isreal):
    """Other bandwidths on ONE context and back, through the C ABI: growing (16 -> 65 -> 130: the padded order of the theta
    operators goes 64 -> 128 -> 192 and their buffer is replaced), shrinking (-> 5, -> 16: a larger allocation is reused at
    a smaller order) and a repeat without a change.  Every result is held to the long double evaluator, and every later
    call at a bandwidth returns the bits of the first one there, for fun2shc and fun2shr."""
    import ctypes
    from quflow_amd import _lib
    from quflow_amd.context import Context, ptr
    ctx = Context(65)

    def run(f, L, shr):
        out = np.empty(L * L, dtype=np.float64 if shr else np.complex128)
        fn = ctx._lib.qf_fun2shr if shr else ctx._lib.qf_fun2shc
        _lib.check(fn(ctx.handle, ptr(f), L, int(isreal), ptr(out)))
        return out

    grids = {}
    for L in (16, 65, 130, 5):
        rng = np.random.default_rng(40 + L)
        f = rng.standard_normal((L, 2 * L - 1))
        grids[L] = f if isreal else f + 1j * rng.standard_normal((L, 2 * L - 1))
    first = {}
    for L in (16, 65, 130, 5, 16, 16, 65, 5, 130):
        got = run(grids[L], L, False)
        if L not in first:
            ref, S = analysis_ref(grids[L], L, scales=True)
            assert report("one context, now at L=%d %s" % (L, "real" if isreal else "complex"),
                          np.abs(got - ref).astype(np.float64), C_DEVICE * L * EPS * S + 1e-300) <= 1.0
            first[L] = got
        assert got.tobytes() == first[L].tobytes(), L
        assert run(grids[L], L, True).tobytes() == T.shc2shr(first[L]).tobytes(), L


def test_python_entry_points_share_one_context():
    """sht.fun2shc at several bandwidths runs on one context (the analysis does not depend on N) and returns what a
    context of its own returns."""
    from quflow_amd.context import Context, ptr
    from quflow_amd import _lib
    grids = {L: np.random.default_rng(L).standard_normal((L, 2 * L - 1)) for L in (16, 65, 5)}
    first = {L: sht.fun2shc(f) for L, f in grids.items()}
    assert sht._context(None) is sht._context(None)
    for L in (5, 16, 65, 16):
        assert sht.fun2shc(grids[L]).tobytes() == first[L].tobytes(), L
        own = Context(max(L, 2))
        out = np.empty(L * L, dtype=np.complex128)
        _lib.check(own._lib.qf_fun2shc(own.handle, ptr(grids[L]), L, 1, ptr(out)))
        assert out.tobytes() == first[L].tobytes(), L


def test_dtype_rules_and_as_shr():
    L = 8
    rng = np.random.default_rng(3)
    f = rng.standard_normal((L, 2 * L - 1))
    want = sht.fun2shr(f)
    assert sht.fun2shr(f.astype(np.float32).astype(np.float64)).shape == want.shape
    assert sht.as_shr(f).tobytes() == want.tobytes()
    assert sht.fun2shr(np.asfortranarray(f)).tobytes() == want.tobytes()
    ints = rng.integers(-5, 5, (L, 2 * L - 1))
    assert sht.fun2shr(ints).tobytes() == sht.fun2shr(ints.astype(float)).tobytes()
    img = rng.integers(0, 256, (L, 2 * L - 1)).astype(np.uint8)
    assert sht.as_shr(img).tobytes() == sht.fun2shr(T.img2fun(img)).tobytes()
    assert sht.fun2shc(f.astype(np.complex64)).dtype == np.complex128


# ---------------------------------------------------------------------------------------------------------------------
# large L: single harmonics made by the long double evaluator
# ---------------------------------------------------------------------------------------------------------------------

def _harmonics(L):
    """A dozen (l, m): the orders of the issue's list, the degree cycling through m, m+1, (m+L)/2, L-1."""
    orders = []
    for m in (0, 1, 2, 63, 64, 255, 256, 100, L - 1 - 100, L // 2, L - 2, L - 1):
        if 0 <= m < L and m not in orders:
            orders.append(m)
    out = []
    for i, m in enumerate(orders):
        el = (m, m + 1, (m + L) // 2, L - 1)[i % 4]
        out.append((min(el, L - 1), m))
    return out


def _lambda_fp64(el, m, L):
    """lambda_lm at every ring, long double recurrence (explicit exponents), rounded to float64."""
    for ell, mant, E in lambda_iter(m, ring_q(L)):
        if ell == el:
            return np.ldexp(mant, E).astype(np.float64)


def _phase(m, L):
    P = 2 * L - 1
    k = (m * np.arange(P, dtype=np.int64)) % P
    ang = (2 * np.pi * k) / P
    return np.cos(ang), np.sin(ang)


@pytest.mark.parametrize("L", LARGE_LS)
def test_large_single_harmonics_real(L):
    """Real harmonics: the real coefficient (l, +m) or (l, -m) is 1 -- f = sqrt(4 pi) sqrt(2) (-1)^m lambda_lm cos(m phi) or
    -sin(m phi) (shr2shc's convention; lambda_l0 at m = 0) -- all in one grid; fun2shr must return those ones and zeros."""
    hs = _harmonics(L)
    f = np.zeros((L, 2 * L - 1))
    want = np.zeros(L * L)
    r4pi = float(np.sqrt(FOURPI))
    for i, (el, m) in enumerate(hs):
        lam = _lambda_fp64(el, m, L) * r4pi
        cs, sn = _phase(m, L)
        if m == 0:
            f += np.outer(lam, cs)
            want[el * el + el] = 1.0
        else:
            lam = lam * (np.sqrt(2.0) * (-1.0 if m % 2 else 1.0))
            neg = i % 2 == 1
            f += np.outer(lam, -sn if neg else cs)
            want[el * el + el + (-m if neg else m)] = 1.0
    got = sht.fun2shr(f)
    err = np.abs(got - want)
    assert report("single harmonics real L=%d (n=%d)" % (L, len(hs)), err, C_DEVICE * L * EPS * np.sqrt(len(hs))) <= 1.0


@pytest.mark.parametrize("L", LARGE_LS)
def test_large_single_harmonics_complex(L):
    """Complex harmonics Y_lm and Y_l,-m (lambda_l,-m = (-1)^m lambda_lm), alternating, all in one grid; fun2shc must
    return those unit coefficients and zeros."""
    hs = _harmonics(L)
    f = np.zeros((L, 2 * L - 1), dtype=np.complex128)
    want = np.zeros(L * L, dtype=np.complex128)
    r4pi = float(np.sqrt(FOURPI))
    for i, (el, m) in enumerate(hs):
        lam = _lambda_fp64(el, m, L) * r4pi
        cs, sn = _phase(m, L)
        neg = i % 2 == 1 and m > 0
        if neg:
            f += np.outer(lam * (-1.0 if m % 2 else 1.0), cs - 1j * sn)
        else:
            f += np.outer(lam, cs + 1j * sn)
        want[el * el + el + (-m if neg else m)] = 1.0
    got = sht.fun2shc(f)
    err = np.abs(got - want)
    assert report("single harmonics complex L=%d (n=%d)" % (L, len(hs)), err, C_DEVICE * L * EPS * np.sqrt(len(hs))) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# large L: dense coefficients through the device synthesis and back
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["shr", "shc"])
@pytest.mark.parametrize("spec", ["white", "decay"])
@pytest.mark.parametrize("L", LARGE_LS)
def test_large_dense_round_trip(L, spec, kind):
    rng = np.random.default_rng(1000 + L)
    el = np.floor(np.sqrt(np.arange(L * L))).astype(np.int64)
    damp = 1.0 if spec == "white" else 1.0 / (1.0 + el)
    if kind == "shr":
        om = rng.standard_normal(L * L) * damp
        om /= np.linalg.norm(om)
        got = sht.fun2shr(T.shr2fun(om, berezin=False))
    else:
        om = (rng.standard_normal(L * L) + 1j * rng.standard_normal(L * L)) * damp
        om /= np.linalg.norm(om)
        got = sht.fun2shc(T.shc2fun(om, berezin=False))
    err = np.abs(got - om)
    assert report("dense %s %s L=%d" % (kind, spec, L), err, C_DEVICE * L * EPS) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# DeviceTrajectory.from_fun, quflow_amd.analysis on fun data, argument errors
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,L", [(256, 256), (256, 64), (2304, 512)])
def test_from_fun_is_from_shr_of_fun2shr(N, L):
    om = np.random.default_rng(N + L).standard_normal(L * L)
    om[0] = 0.0
    om /= np.linalg.norm(om)
    f = T.shr2fun(om, berezin=False)
    a = qfa.DeviceTrajectory.from_fun(f, N)
    Wa = a.download()
    b = qfa.DeviceTrajectory.from_shr(sht.fun2shr(f), N)
    Wb = b.download()
    assert Wa.shape == (N, N) and Wa.tobytes() == Wb.tobytes()
    assert np.array_equal(Wa, -Wa.conj().T)
    assert np.abs(Wa).max() > 0
    dt = 0.1 * qfa.hbar(N)
    a.advance(dt, 5)
    b.advance(dt, 5)
    assert a.download().tobytes() == b.download().tobytes()
    if N == L:
        assert qfa.DeviceTrajectory.from_fun(f).download().tobytes() == Wa.tobytes()      # N = -1: N = L


def test_from_fun_refuses_a_grid_above_the_matrix_size():
    f = np.zeros((65, 129))
    with pytest.raises(ValueError, match="L=65.*N=64"):
        qfa.DeviceTrajectory.from_fun(f, 64)
    with pytest.raises(AssertionError):
        qfa.DeviceTrajectory.from_fun(f.astype(complex), 128)


def test_spectra_of_fun_and_mat_data():
    """energy_spectrum / enstrophy_spectrum of a `fun` array are those of its known coefficients (the branch the reference
    fixtures cannot reach), and of `mat` data those the reference computed (tests/golden/analysis.npz)."""
    from quflow_amd import analysis as A
    L = 48
    om = A.random_shr(lmax=L - 1, s=1.0, seed=5)
    f = T.shr2fun(om, berezin=False)
    # coefficients within d = C L eps ||f||_2 (||f||_2 = 1): a degree's sum of 2l+1 squares moves by at most
    # 2 sqrt(2l+1) sqrt(sum) d + (2l+1) d^2, and the energy divides that by l (l+1) >= 2
    d = C_DEVICE * L * EPS
    tol = 2 * np.sqrt(2 * L * A.enstrophy_spectrum(om)[1].max()) * d + 2 * L * d * d
    for fn in (A.energy_spectrum, A.enstrophy_spectrum):
        el, want = fn(om)
        el2, got = fn(f)
        assert np.array_equal(el, el2)
        print("%s of fun data: max err %.2e  tol %.2e" % (fn.__name__, np.abs(got - want).max(), tol))
        assert np.abs(got - want).max() <= tol
    # mat data against the reference's own outputs, to the 1e-14 relative of the host fixtures
    gold = np.load(GOLD)

    def rel(got, want, label):
        r = float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))
        print("%-28s relative difference to the reference %.2e" % (label, r))
        return r

    for N in (16, 64):
        W = gold["mat_%d" % N]
        for beta in (0, 1):
            assert rel(A.energy_spectrum(W, beta=beta)[1], gold["energy_mat_b%d_%d" % (beta, N)],
                       "energy mat beta=%d N=%d" % (beta, N)) <= 1e-14
        assert rel(A.enstrophy_spectrum(W)[1], gold["enstrophy_mat_%d" % N], "enstrophy mat N=%d" % N) <= 1e-14
        assert rel(A.gamma_ratio(W), gold["gamma_mat_%d" % N], "gamma_ratio mat N=%d" % N) <= 1e-14


def test_argument_errors_are_error_returns():
    import ctypes
    from quflow_amd import _lib
    from quflow_amd.context import get_context, ptr
    ctx = get_context(64)
    f = np.zeros((8, 15))
    out = np.zeros(8193 * 2)
    for L in (0, -3, 8193):
        for fn in (ctx._lib.qf_fun2shc, ctx._lib.qf_fun2shr):
            with pytest.raises(qfa.QuflowHipError, match="INVALID.*L=%d" % L):
                _lib.check(fn(ctx.handle, ptr(f), L, 1, ptr(out)))
    with pytest.raises(qfa.QuflowHipError, match="INVALID"):
        _lib.check(ctx._lib.qf_fun2shc(ctx.handle, None, 8, 1, ptr(out)))
    with pytest.raises(qfa.QuflowHipError, match="INVALID"):
        _lib.check(ctx._lib.qf_fun2shc(ctx.handle, ptr(f), 8, 1, None))
    with pytest.raises(qfa.QuflowHipError, match="INVALID.*L=65.*N=64"):                 # the NULL form keeps L^2 <= N^2 on ctx
        _lib.check(ctx._lib.qf_fun2shr(ctx.handle, ptr(np.zeros((65, 129))), 65, 1, None))
    with pytest.raises(AssertionError, match="Shape of input"):
        sht.fun2shc(np.zeros((8, 16)))
    # the context is still usable
    g = np.random.default_rng(0).standard_normal((8, 15))
    ref, S = analysis_ref(g, 8, scales=True)
    assert np.max(np.abs(sht.fun2shc(g) - ref).astype(np.float64) / (C_DEVICE * 8 * EPS * S + 1e-300)) <= 1.0
