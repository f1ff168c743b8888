"""Host side of the spherical-harmonic ANALYSIS (quflow_amd.sht, quflow_amd.analysis; no GPU needed), and the independent
evaluators that the device tests (tests/test_hip_sht_analysis.py) compare against.

The transform is fixed by its definition (McEwen-Wiaux analysis as pyssht states it), for f (L, P), P = 2L-1:
  1. F_m(t) = (1/P) sum_p f[t, p] e^{-2 pi i m p/P};
  2. F_m(theta_{P-1-t}) = (-1)^m F_m(theta_t), t < L-1 (theta = pi kept);  3. the trigonometric interpolant of those P values;
  4. a_lm = 2 pi int_0^pi F_m(theta) lambda_lm(theta) sin(theta) d theta, exactly;   5. omega[l^2+l+m] = a_lm / sqrt(4 pi).
Steps 2-4 are a_lm = (2 pi/P) sum_{t<L} lambda_lm(theta_t) (Q_{m mod 2} F_m)(t) with two L x L matrices formed here from
their complex factors: extend -> DFT in theta -> Toeplitz matrix w(m' - k), w(n) = int_0^pi e^{i n x} sin x dx -> evaluate at
the P nodes -> fold.  (The device builds them from a different, real factorisation: csrc/sht.hip.)

* analysis_ref : all of it in np.longdouble, dense, O(L^3): the reference of the device tests at small L.  lambda_lm comes
  from test_transforms_host.lambda_rows at the rings theta_t = pi q_t, q_t rounded to float64 -- the sample points the
  device hands to sincospi, the convention of the synthesis tests.
* analysis_fp64: the same three stages in plain float64 (numpy.fft for the rings, complex128 BLAS for Q, lambda_lm
  rounded once): the fp64 reference whose own error against analysis_ref sizes the device's accuracy bar,
      |omega_dev - omega_ref| <= C L eps ||f||_2,   C = 8 x (worst ratio err / (L eps ||f||_2) of analysis_fp64),
  ||f||_2 the L2(S^2) norm over sqrt(4 pi): ||omega||_2 for band-limited input.  test_fp64_reference_ratio measures the
  ratio, prints it, and holds it below RATIO_FP64, the figure recorded from that measurement; the device tests import
  C_DEVICE = 8 RATIO_FP64.  Measured (this file, white coefficients of norm 1, real and complex grids): see RATIO_FP64.
"""
import functools
import os

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import transforms as T
from test_transforms_host import LD, PI, FOURPI, ring_q, lambda_rows, synth_ref, det_values

EPS = np.finfo(np.float64).eps
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis.npz")
CLD = np.clongdouble

# Worst err / (L eps ||f||_2) of analysis_fp64 against analysis_ref over SMALL_LS and, by round trip through synth_ref, up
# to L = 255, real and complex white data: measured 0.798 (L = 2, complex; 0.69 at L = 2 real, 0.50 at L = 1, 0.27 at
# L = 4, 0.05 at L = 9, 0.02 at L = 16, 0.007 at L = 32 and 128, 0.004 at L = 255: at the smallest L one rounding of a
# coefficient of size 1 is already half of L eps).  The device's bar is 8 times this, the same C at every L.
RATIO_FP64 = 0.80
C_DEVICE = 8 * RATIO_FP64
SMALL_LS = (1, 2, 3, 4, 5, 16, 63, 64, 65)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluators
# ---------------------------------------------------------------------------------------------------------------------

def _w(n, ctype):
    """w(n) = int_0^pi e^{i n x} sin x dx: 2/(1-n^2) for even n, +-i pi/2 for n = +-1, else 0."""
    n = np.asarray(n)
    rtype = LD if ctype is CLD else np.float64
    out = np.zeros(n.shape, dtype=ctype)
    ev = n % 2 == 0
    out[ev] = rtype(2) / (rtype(1) - n[ev].astype(rtype) ** 2)
    half_pi = (PI / 2) if ctype is CLD else np.pi / 2
    out[n == 1] = 1j * half_pi
    out[n == -1] = -1j * half_pi
    return out


def theta_operators(L, ctype=CLD):
    """(Q_even, Q_odd) as complex arrays (their imaginary parts are rounding) from the factors of steps 2-4."""
    P = 2 * L - 1
    rtype = LD if ctype is CLD else np.float64
    pi = PI if ctype is CLD else np.pi
    ks = np.arange(-(L - 1), L)
    # k theta_s = pi k (2s+1)/P with the integer reduced mod 2P
    n = (ks[:, None] * (2 * np.arange(P)[None, :] + 1)) % (2 * P)
    ang = pi * n.astype(rtype) / P
    E = (np.cos(ang) + 1j * np.sin(ang)).astype(ctype)          # e^{i k theta_s}, [k, s]
    W = _w(ks[None, :] - ks[:, None], ctype)                      # [k, m'] = w(m' - k)
    out = []
    for sgn in (1, -1):
        X = np.zeros((P, L), dtype=rtype)
        X[:L] = np.eye(L)
        for t in range(L - 1):
            X[P - 1 - t, t] = sgn
        C = (np.conj(E) / P) @ X.astype(ctype)                    # F_mm'  [m', ring]
        G = W @ C
        H = E.T @ G                                               # on the full circle, [node, ring]
        Hf = H[:L].copy()
        if L > 1:
            Hf[:L - 1] += sgn * H[P - 1:L - 1:-1]
        out.append(Hf)
    return out


@functools.lru_cache(maxsize=4)
def _q_ld(L):
    return [q.real.copy() for q in theta_operators(L, CLD)]


@functools.lru_cache(maxsize=4)
def _q_64(L):
    return [q.real.copy() for q in theta_operators(L, np.complex128)]


def ring_dft_ref(f, L):
    """F[m + L-1, t] for |m| < L in long double (dense DFT at the exact reduction of m p mod P)."""
    P = 2 * L - 1
    ms = np.arange(-(L - 1), L)
    k = (ms[:, None] * np.arange(P)[None, :]) % P
    ang = 2 * PI * k.astype(LD) / P
    E = np.cos(ang) - 1j * np.sin(ang)
    return (E @ np.asarray(f).astype(CLD).T) / P


def analysis_ref(f, L, scales=False):
    """fun2shc(f) by the definition, long double: L^2 complex coefficients.  With scales=True also S[l^2+l+m] =
    (2 pi/P)/sqrt(4 pi) sum_t |lambda_lm(theta_t)| sum_t' |Q[t, t']| |F_m(t')|: the size rounding errors of a sum in this
    form are relative to, for grids that are not band-limited."""
    P = 2 * L - 1
    F = ring_dft_ref(f, L)
    Q = _q_ld(L)
    q = ring_q(L)
    c = 2 * PI / P / np.sqrt(FOURPI)
    om = np.zeros(L * L, dtype=CLD)
    S = np.zeros(L * L)
    for m in range(L):
        lam = lambda_rows(m, L - 1, q)
        ls = np.arange(m, L)
        for sign in ((1, -1) if m else (1,)):
            Fm = F[sign * m + L - 1]
            a = c * (lam.astype(CLD) @ (Q[m % 2].astype(CLD) @ Fm))
            if sign < 0 and m % 2:
                a = -a
            om[ls * ls + ls + sign * m] = a
            if scales:
                S[ls * ls + ls + sign * m] = (c * (np.abs(lam) @ (np.abs(Q[m % 2]) @ np.abs(Fm)))).astype(np.float64)
    return (om, S) if scales else om


def analysis_fp64(f, L):
    """The same map in plain float64: numpy.fft on the rings, Q from complex128 factors, lambda_lm rounded to float64, BLAS
    sums."""
    P = 2 * L - 1
    F = np.fft.fft(np.asarray(f, dtype=np.complex128), axis=1) / P          # [t, m mod P]
    Q = _q_64(L)
    q = ring_q(L)
    c = 2 * np.pi / P
    om = np.zeros(L * L, dtype=np.complex128)
    for m in range(L):
        lam = lambda_rows(m, L - 1, q).astype(np.float64)
        ls = np.arange(m, L)
        for sign in ((1, -1) if m else (1,)):
            a = c * (lam @ (Q[m % 2] @ F[:, (sign * m) % P])) / np.sqrt(4 * np.pi)
            if sign < 0 and m % 2:
                a = -a
            om[ls * ls + ls + sign * m] = a
    return om


def white(L, seed, cplx, decay=False):
    """Coefficients of norm 1: white or ~ 1/(1+l); complex (any) or those of a real function."""
    rng = np.random.default_rng(seed)
    if cplx:
        om = rng.standard_normal(L * L) + 1j * rng.standard_normal(L * L)
    else:
        om = T.shr2shc(rng.standard_normal(L * L))
    if decay:
        om = om / (1.0 + np.floor(np.sqrt(np.arange(L * L))))
    return om / np.linalg.norm(om)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator against scipy and quad: independent of this repository's synthesis
# ---------------------------------------------------------------------------------------------------------------------

def scipy_grid(coeffs, L):
    """sum a_lm Y_lm on the MW grid by scipy.special.sph_harm_y (coeffs: {(l, m): a})."""
    from scipy.special import sph_harm_y
    P = 2 * L - 1
    th = np.pi * (2 * np.arange(L) + 1) / P
    ph = 2 * np.pi * np.arange(P) / P
    f = np.zeros((L, P), dtype=complex)
    for (el, m), a in coeffs.items():
        f += a * sph_harm_y(el, m, th[:, None], ph[None, :])
    return f


@pytest.mark.parametrize("L", [1, 2, 3, 9, 16, 33])
def test_evaluator_recovers_scipy_harmonics(L):
    """Grids of single harmonics and of random band-limited sums made by scipy: the coefficients come back (times
    1/sqrt(4 pi), step 5) to 1e-13 ||a||_2."""
    rng = np.random.default_rng(L)
    singles = {(0, 0), (L - 1, 0), (L - 1, L - 1), (L - 1, -(L - 1)), (L // 2, -(L // 3)), (L - 1, (L - 1) // 2)}
    for el, m in sorted(singles):
        want = np.zeros(L * L, dtype=complex)
        want[el * el + el + m] = 1.0
        got = analysis_ref(scipy_grid({(el, m): 1.0}, L), L) * np.sqrt(FOURPI)
        assert np.abs(got - want).max() <= 1e-13, (L, el, m)
    a = rng.standard_normal(L * L) + 1j * rng.standard_normal(L * L)
    coeffs = {(el, m): a[el * el + el + m] for el in range(L) for m in range(-el, el + 1)}
    got = analysis_ref(scipy_grid(coeffs, L), L) * np.sqrt(FOURPI)
    assert np.abs(got - a).max() <= 1e-13 * np.linalg.norm(a), L
    got64 = analysis_fp64(scipy_grid(coeffs, L), L) * np.sqrt(4 * np.pi)
    assert np.abs(got64 - a).max() <= 1e-12 * np.linalg.norm(a), L


def test_evaluator_is_the_integral_of_the_interpolant():
    """An arbitrary (not band-limited) complex grid at L = 9: every coefficient equals step 4 evaluated by
    scipy.integrate.quad on the interpolant of steps 1-3, to 1e-12."""
    from scipy.integrate import quad
    from scipy.special import sph_harm_y
    L = 9
    P = 2 * L - 1
    rng = np.random.default_rng(1)
    g = rng.standard_normal((L, P)) + 1j * rng.standard_normal((L, P))
    got = analysis_ref(g, L) * np.sqrt(FOURPI)
    ph = 2 * np.pi * np.arange(P) / P
    thf = np.pi * (2 * np.arange(P) + 1) / P
    ks = np.arange(-(L - 1), L)
    worst = 0.0
    for m in range(-(L - 1), L):
        Fm = (g * np.exp(-1j * m * ph)[None, :]).sum(axis=1) / P
        Fe = np.concatenate([Fm, (-1.0) ** abs(m) * Fm[:L - 1][::-1]])
        c = (np.exp(-1j * np.outer(ks, thf)) / P) @ Fe
        for el in range(abs(m), L):
            def integrand(t, part):
                v = (c @ np.exp(1j * ks * t)) * sph_harm_y(el, m, t, 0.0).real * np.sin(t)
                return v.real if part == 0 else v.imag
            val = 2 * np.pi * (quad(integrand, 0, np.pi, args=(0,), epsabs=1e-13, epsrel=1e-13)[0]
                               + 1j * quad(integrand, 0, np.pi, args=(1,), epsabs=1e-13, epsrel=1e-13)[0])
            worst = max(worst, abs(complex(got[el * el + el + m]) - val))
    print("L=9 arbitrary grid: max |evaluator - quad| = %.2e" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("L", [1, 2, 3, 9, 16, 33])
def test_theta_operators_are_real(L):
    for q in theta_operators(L, CLD):
        assert np.abs(q.imag).max() <= 1e-16 * L
    for q in theta_operators(L, np.complex128):
        assert np.abs(q.imag).max() <= 64 * EPS * L
    assert max(np.abs(q).sum(axis=1).max() for q in _q_ld(L)) <= 7.8        # ||Q||_inf, the figure the bar's form rests on


@pytest.mark.parametrize("L", [1, 2, 5, 16, 33])
@pytest.mark.parametrize("isreal", [True, False])
def test_evaluator_inverts_the_long_double_synthesis(L, isreal):
    om = white(L, 7 * L + isreal, cplx=not isreal)
    f = synth_ref(om, L, isreal, berezin=False)
    got = analysis_ref(f, L)
    assert np.abs(got - om).max() <= 1e-16 * L * 4, np.abs(got - om).max()


@pytest.mark.parametrize("L", [2, 9, 16])
def test_real_input_symmetry_and_real_packing(L):
    """A real grid gives a_l,-m = (-1)^m conj(a_lm); fun2shr's packing, restated on the host with shc2shr's operations, is
    shc2shr of the complex result bit for bit."""
    rng = np.random.default_rng(L)
    f = rng.standard_normal((L, 2 * L - 1))
    om = analysis_fp64(f, L)
    ref = analysis_ref(f, L)
    for el in range(L):
        for m in range(1, el + 1):
            assert abs(ref[el * el + el - m] - (-1) ** m * np.conj(ref[el * el + el + m])) <= 1e-17 * L * np.abs(f).max()
    packed = np.zeros(L * L)
    for el in range(L):
        packed[el * el + el] = om[el * el + el].real
        for m in range(1, el + 1):
            c = np.sqrt(2.0) * (-1.0 if m % 2 else 1.0)
            packed[el * el + el + m] = c * om[el * el + el + m].real
            packed[el * el + el - m] = c * om[el * el + el + m].imag
    assert packed.tobytes() == T.shc2shr(om).tobytes()


def fp64_ratio(L, isreal, f=None, om=None):
    """err / (L eps ||f||_2) of analysis_fp64, against analysis_ref (a grid f) or against the coefficients om whose long
    double synthesis is analysed (||f||_2 = ||om||_2 = 1)."""
    if f is None:
        f = synth_ref(om, L, isreal, berezin=False)
        f = f.astype(np.float64 if isreal else np.complex128)
        ref = om
    else:
        ref = analysis_ref(f, L)
    got = analysis_fp64(f, L)
    return float(np.abs(got - ref).max()) / (L * EPS)


def test_fp64_reference_ratio():
    """The worst ratio of the fp64 reference: what C_DEVICE is 8 times.  Small L against analysis_ref, larger L by round trip
    through synth_ref (there the rounding of f to fp64 is part of the figure: it is part of any fp64 input)."""
    worst = 0.0
    for L in SMALL_LS + (9, 32, 33):
        for isreal in (True, False):
            om = white(L, 100 + L, cplx=not isreal)
            f = synth_ref(om, L, isreal, berezin=False).astype(np.float64 if isreal else np.complex128)
            r = fp64_ratio(L, isreal, f=f)
            print("analysis_fp64 vs analysis_ref   L=%4d %s  err/(L eps ||f||) = %.3f" % (L, "real" if isreal else "cplx", r))
            worst = max(worst, r)
    for L, isreal in ((128, True), (128, False), (255, True)):
        r = fp64_ratio(L, isreal, om=white(L, 100 + L, cplx=not isreal))
        print("analysis_fp64 round trip        L=%4d %s  err/(L eps ||f||) = %.3f" % (L, "real" if isreal else "cplx", r))
        worst = max(worst, r)
    print("worst ratio %.3f (recorded RATIO_FP64 = %.2f, C_DEVICE = %.2f)" % (worst, RATIO_FP64, C_DEVICE))
    assert worst <= RATIO_FP64


# ---------------------------------------------------------------------------------------------------------------------
# host rules of quflow_amd.sht
# ---------------------------------------------------------------------------------------------------------------------

def have_gpu():
    return qfa.device_count() > 0


def test_sht_module_is_exported_and_transforms_still_refuse():
    from quflow_amd import sht
    assert qfa.sht is sht and callable(sht.fun2shc) and callable(sht.fun2shr) and callable(sht.as_shr)
    assert qfa.fun2shr is T.fun2shr and qfa.fun2shr is not sht.fun2shr


@pytest.mark.parametrize("shape", [(4, 6), (4, 8), (5, 5), (7,)])
def test_wrong_shapes_raise_the_reference_assertion(shape):
    from quflow_amd import sht
    for fn in (sht.fun2shc, sht.fun2shr):
        with pytest.raises(AssertionError, match=r"Shape of input must be \(N, 2\*N-1\)"):
            fn(np.zeros(shape))


def test_as_shr_dispatch_without_a_device():
    from quflow_amd import sht
    omr = det_values(25, 1)
    assert sht.as_shr(omr) is not None and np.array_equal(sht.as_shr(omr), omr)
    omc = det_values(25, 2) + 1j * det_values(25, 3)
    assert sht.as_shr(omc).tobytes() == T.shc2shr(omc).tobytes()
    if not have_gpu():
        W = np.zeros((8, 8), dtype=complex)
        with pytest.raises(qfa.QuflowHipError, match="NO_DEVICE"):       # a square complex matrix goes to mat2shr
            sht.as_shr(W)


def test_no_silent_cpu_fallback():
    """Without a HIP device the analysis raises and never returns a host result."""
    if have_gpu():
        pytest.skip("a GPU is present")
    from quflow_amd import sht
    f = np.zeros((4, 7))
    for call in (lambda: sht.fun2shc(f), lambda: sht.fun2shr(f), lambda: sht.fun2shc(f.astype(complex)),
                 lambda: sht.as_shr(f), lambda: sht.as_shr(np.zeros((4, 7), dtype=np.uint8)),
                 lambda: qfa.DeviceTrajectory.from_fun(f), lambda: qfa.analysis.energy_spectrum(f)):
        with pytest.raises(qfa.QuflowHipError, match="NO_DEVICE"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# quflow_amd.analysis against the reference's own outputs (tools/gen_analysis_golden.py)
# ---------------------------------------------------------------------------------------------------------------------

RANDOM_SETS = ((15, 1.0, 0.0, 11), (31, 2.0, 0.3, 12), (20, 0.0, None, 13))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def close(got, want):
    return np.abs(np.asarray(got) - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("N", [16, 64])
def test_spectra_vs_reference(gold, N):
    from quflow_amd import analysis as A
    omr = det_values(N * N, 21)
    omc = det_values(N * N, 22) + 1j * det_values(N * N, 23)
    for kind, data in (("shr", omr), ("shc", omc)):
        for beta in (0, 1):
            el, e = A.energy_spectrum(data, beta=beta)
            assert np.array_equal(el, gold["el_%d" % N]) and e.shape == (N - 1,)
            assert close(e, gold["energy_%s_b%d_%d" % (kind, beta, N)]), (kind, beta)
        el, s = A.enstrophy_spectrum(data)
        assert np.array_equal(el, gold["el_%d" % N])
        assert close(s, gold["enstrophy_%s_%d" % (kind, N)]), kind
    assert abs(A.gamma_ratio(omr) - float(gold["gamma_shr_%d" % N])) <= 1e-14 * float(gold["gamma_shr_%d" % N])


@pytest.mark.parametrize("i", range(len(RANDOM_SETS)))
def test_random_shr_is_the_reference_bit_for_bit(gold, i):
    from quflow_amd import analysis as A
    lmax, s, gamma, seed = RANDOM_SETS[i]
    got = A.random_shr(lmax=lmax, s=s, gamma=gamma, seed=seed)
    assert got.tobytes() == gold["random_shr_%d" % i].tobytes()
    assert abs(np.linalg.norm(got) - 1.0) <= 4 * EPS
