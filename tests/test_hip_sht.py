"""Spherical-harmonic synthesis on the device (shr2fun / shc2fun, quflow_amd/csrc/sht.hip) against the long double
evaluator of tests/test_transforms_host.py.

Bars, from the error of the evaluator (long double, ~1e-19) and of an fp64 pipeline, not from the device output:
  * dense random coefficients with ||omega||_2 = 1 at L <= 300: max |df| <= 16 L eps max(1, max |f|).  The fp64 errors (the
    l-recurrence, ~l eps relative; a sum over 2L terms per grid point) grow like L eps |f|: the bar is 1e-12 at L ~ 70 and
    ~4e-12 at L = 300 (|f| is ~4 there);
  * the underflow regime (L = 1024, 2048, 8192, berezin=False so that w_l does not vanish at l ~ L): per grid point
    |df| <= 32 L eps sum_terms w_m |a| (lambda_lm^2 + lambda_l-1,m^2)^(1/2) + 1e-300 at ring theta_t -- the fp64 recurrence
    and the seed sin^m theta carry ~(l + m) eps error relative to the pair of values the recurrence carries -- and a lone
    term that the evaluator finds above 1e-300 at a ring must be there, to the same bar.
"""
import ctypes

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import _lib
from quflow_amd import transforms as T
from quflow_amd.context import get_context, ptr

from test_transforms_host import real_term, synth_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DENSE_L = [1, 2, 3, 16, 33, 64, 255, 256, 300]
# (entry point, isreal, berezin, length relative to L^2)
MODES = [("shr", True, True, "exact"), ("shr", True, False, "trim"), ("shr", True, True, "pad"),
         ("shc", False, True, "pad"), ("shc", False, False, "exact"), ("shc", False, True, "trim"),
         ("shc", True, True, "trim"), ("shc", True, False, "pad")]


def _length(L, kind):
    return {"exact": L * L, "trim": L * L + 2 * L + 3, "pad": max(1, L * L - L)}[kind]


@pytest.mark.parametrize("mode", MODES, ids=["-".join(map(str, m)) for m in MODES])
@pytest.mark.parametrize("L", DENSE_L)
def test_dense_vs_evaluator(L, mode):
    entry, isreal, berezin, kind = mode
    rng = np.random.default_rng(1000 * L + MODES.index(mode))
    n = _length(L, kind)
    if entry == "shr":
        if kind == "trim":
            n = (L + 1) ** 2        # (a degree cut short past L^2 is refused by shr2shc, as by the reference)
        om = rng.standard_normal(n)
        om /= np.linalg.norm(om[:L * L])
        f = T.shr2fun(om, N=L, berezin=berezin)
        ref = synth_ref(T.shr2shc(om), L, isreal=True, berezin=berezin)
    else:
        om = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        om /= np.linalg.norm(om[:L * L])
        f = T.shc2fun(om, isreal=isreal, N=L, berezin=berezin)
        ref = synth_ref(om, L, isreal=isreal, berezin=berezin)
    assert f.shape == (L, 2 * L - 1)
    assert f.dtype == (np.float64 if isreal else np.complex128)
    err = float(np.abs(f - ref).max())
    bar = 16 * L * EPS * max(1.0, float(np.abs(ref).max()))
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("L", [16, 255, 300])
@pytest.mark.parametrize("berezin", [True, False])
def test_shr_and_shc_routes_agree(L, berezin):
    """shc2fun(shr2shc(omega), isreal=True) == shr2fun(omega) bit for bit; the complex synthesis of the same (real)
    function is real to 1e-13 and equals it to 1e-13."""
    om = np.random.default_rng(L).standard_normal(L * L)
    om /= np.linalg.norm(om)
    fr = T.shr2fun(om, berezin=berezin)
    fc_real = T.shc2fun(T.shr2shc(om), isreal=True, berezin=berezin)
    assert np.array_equal(fr, fc_real)
    fc = T.shc2fun(T.shr2shc(om), isreal=False, berezin=berezin)
    assert np.abs(fc.imag).max() <= 1e-13
    assert np.abs(fc.real - fr).max() <= 1e-13


def _sparse_terms(L):
    """(l, m) with the real coefficient set to 1: three deep in the underflow regime and one of low order."""
    return [(L - 1, L - 1), (L - 1, L // 2), (L // 2, L // 2 - 1), (5, 2)]


def _checked_points(L, terms):
    """~257 columns at every ring; every column at the pole rings and at the rings around each term's turning point."""
    P = 2 * L - 1
    cols = np.unique(np.linspace(0, P - 1, 257).round().astype(int))
    rows = {0, 1, 2, L - 3, L - 2, L - 1}
    for el, m in terms:
        th = np.arcsin(min(1.0, abs(m) / (el + 0.5)))
        for c in (th, np.pi - th):
            t = int(round(c * (2 * L - 1) / (2 * np.pi) - 0.5))
            rows.update(range(t - 2, t + 3))
    rows = np.array(sorted(r for r in rows if 0 <= r < L))
    return cols, rows


def _terms_of(om, L):
    """The m >= 0 complex coefficients a real synthesis of omega uses (shr2shc), as (l, m, a)."""
    omc = T.shr2shc(om)
    out = []
    for ind in np.nonzero(omc)[0]:
        el = int(np.floor(np.sqrt(ind)))
        m = int(ind - el * el - el)
        if m >= 0:
            out.append((el, m, omc[ind]))
    return out


def _check_sparse(f, om, L):
    terms = _terms_of(om, L)
    cols, rows = _checked_points(L, [(el, m) for el, m, _ in terms])
    P = 2 * L - 1
    for sel_rows, sel_cols in ((np.arange(L), cols), (rows, np.arange(P))):
        ref = 0
        mag = 0
        for el, m, a in terms:
            val, mg = real_term(el, m, a, L, sel_rows, sel_cols)
            ref = ref + val
            mag = mag + mg
        dev = f[np.ix_(sel_rows, sel_cols)]
        bar = 32 * L * EPS * mag[:, None] + 1e-300
        bad = np.abs(dev - ref) > bar
        assert not bad.any(), (L, int(bad.sum()), float(np.abs(dev - ref).max()))
        # nothing the evaluator finds above 1e-300 is lost: those rings are nonzero on the device
        live = mag > 1e-290
        assert np.all(np.abs(dev[live]).max(axis=1) > 0)
    return terms


@pytest.mark.parametrize("L", [1024, 2048, 8192])
def test_underflow_regime(L):
    om = np.zeros(L * L)
    for el, m in _sparse_terms(L):
        om[qfa.elm2ind(el, m)] = 1.0
    f = T.shr2fun(om, berezin=False)
    _check_sparse(f, om, L)
    del f
    # every deep term alone: at the rings where it is tiny it is the whole signal
    for el, m in _sparse_terms(L)[:3]:
        one = np.zeros(L * L)
        one[qfa.elm2ind(el, m)] = 1.0
        f = T.shr2fun(one, berezin=False)
        _check_sparse(f, one, L)
        del f
    # (the check reaches the scaled range: lambda_{L-1,L-1} lies between 1e-300 and 1e-200 at some rings)
    mag = real_term(L - 1, L - 1, 1.0, L, None, np.array([0]))[1]
    assert ((mag > 1e-300) & (mag < 1e-200)).any()


@pytest.mark.parametrize("L", [1024, 2048])
def test_underflow_regime_complex(L):
    """The same deep terms through the complex synthesis (second accumulator): real input, so the output is the real
    synthesis up to rounding."""
    om = np.zeros(L * L)
    for el, m in _sparse_terms(L):
        om[qfa.elm2ind(el, m)] = 1.0
    fr = T.shr2fun(om, berezin=False)
    fc = T.shc2fun(T.shr2shc(om), isreal=False, berezin=False)
    _check_sparse(fc.real.copy(), om, L)
    assert np.abs(fc.imag).max() <= 1e-13
    assert np.abs(fc.real - fr).max() <= 1e-13


@pytest.mark.parametrize("N", [256, 1024])
def test_trajectory_fun_is_shr2fun_of_shr(N):
    from oracle import isomp_oracle
    traj = qfa.DeviceTrajectory(isomp_oracle.make_W0(N, 3))
    for n in (None, (N // 2) ** 2):
        for berezin in (True, False):
            f = traj.fun(n, berezin=berezin)
            g = T.shr2fun(traj.shr(n), berezin=berezin)
            L = N if n is None else N // 2
            assert f.shape == (L, 2 * L - 1)
            assert np.array_equal(f, g), (n, berezin)


def test_as_fun_dispatch():
    from oracle import isomp_oracle
    N = 16
    W = isomp_oracle.make_W0(N, 1)                  # skew-Hermitian: mat2shr, shr2fun
    f = T.as_fun(W)
    assert f.dtype == np.float64 and np.array_equal(f, T.shr2fun(qfa.mat2shr(W), N))
    A = W + 0.3 * np.eye(N) * 1j + 0.2 * np.eye(N)  # not skew-Hermitian: mat2shc, shc2fun, complex output
    g = T.as_fun(A)
    assert g.dtype == np.complex128 and g.shape == (N, 2 * N - 1)
    assert np.array_equal(g, T.shc2fun(qfa.mat2shc(A), N=N))
    omr = qfa.mat2shr(W)
    assert np.array_equal(T.as_fun(omr), T.shr2fun(omr))
    assert np.array_equal(T.as_fun(omr, N=8, berezin=False), T.shr2fun(omr, 8, berezin=False))
    omc = qfa.mat2shc(A)
    h = T.as_fun(omc)
    assert h.dtype == np.complex128 and np.array_equal(h, T.shc2fun(omc))
    assert np.array_equal(T.as_fun(f), f)
    img = T.fun2img(f)
    assert np.array_equal(T.as_fun(img), T.img2fun(img))
    assert np.array_equal(T.as_shr(W), qfa.mat2shr(W))


def test_c_abi_argument_errors():
    ctx = get_context(4)
    lib = ctx._lib
    om = np.ones(16)
    f = np.zeros((4, 7))
    n = ctypes.c_longlong(16)
    for L in (0, -1, 8193):
        assert lib.qf_shr2fun(ctx.handle, ptr(om), n, L, 1, ptr(f)) == 1
        assert lib.qf_shc2fun(ctx.handle, ptr(om), n, L, 1, 1, ptr(f)) == 1
    assert lib.qf_shr2fun(ctx.handle, ptr(om), ctypes.c_longlong(0), 4, 1, ptr(f)) == 1
    assert lib.qf_shr2fun(ctx.handle, ptr(om), n, 4, 1, None) == 1
    assert lib.qf_shc2fun(ctx.handle, None, n, 4, 1, 1, ptr(f)) == 1
    with pytest.raises(qfa.QuflowHipError, match="outside 1..8192"):
        _lib.check(lib.qf_shr2fun(ctx.handle, ptr(om), n, 9000, 1, ptr(f)))
    with pytest.raises(qfa.QuflowHipError, match="empty coefficient array"):
        _lib.check(lib.qf_shc2fun(ctx.handle, ptr(om), ctypes.c_longlong(0), 4, 1, 1, ptr(f)))
    with pytest.raises(qfa.QuflowHipError, match="null output grid"):
        _lib.check(lib.qf_shr2fun(ctx.handle, ptr(om), n, 4, 1, None))
    # omega == NULL reads what qf_mat2shr left; a context where none ran refuses
    fresh = qfa.context.Context(5)
    try:
        with pytest.raises(qfa.QuflowHipError, match="no qf_mat2shr"):
            _lib.check(lib.qf_shr2fun(fresh.handle, None, ctypes.c_longlong(25), 5, 1, ptr(np.zeros((5, 9)))))
    finally:
        fresh.close()


def test_bandwidth_independent_of_context_and_growing_scratch():
    """L is independent of the context's N, and a context's scratch grows with L: on one context (N = 16) the bandwidths
    33, 40, 33 give the bits of shr2fun at 33 on its own context."""
    om = np.random.default_rng(7).standard_normal(40 * 40)
    a = T.shr2fun(om[:33 * 33])
    ctx = get_context(16)
    for L in (33, 40, 33):
        f = np.zeros((L, 2 * L - 1))
        _lib.check(ctx._lib.qf_shr2fun(ctx.handle, ptr(om), ctypes.c_longlong(L * L), L, 1, ptr(f)))
        if L == 33:
            assert np.array_equal(f, a)
