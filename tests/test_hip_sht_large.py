"""Spherical-harmonic synthesis on the device (quflow_amd/csrc/sht.hip) with full sets of coefficients at the bandwidths
runs use, L = 511 to 8192, against the long double evaluator of tests/test_transforms_host.py (legendre_sums: the
Legendre stage in O(L^2) per ring; synth_rings: the ring transform in fp64 with its own rounding bound).

What only does work at large L and is covered here: the Legendre stage's blocks of 256 rings (up to 32), the pairing of m
with L-1-m in one workgroup for both parities of L, the 256-degree LDS chunks, the Fourier GEMM at K = 2L with zeroed
K padding (L mod 8 != 0), the 64-wide column tiles over 2L-1 and the 64-row tiles of the L- or 2L-row operand, the
twiddle gather (m p) mod (2L-1), the Berezin multipliers that reach zero near l ~ L, the trimmed or padded coefficient
array, and DeviceTrajectory.fun().

Bar, per grid point and per real component, from the arithmetic and never from the device output (_check_sparse's
convention in tests/test_hip_sht.py):
    |f_dev - f_ref| <= 32 L eps scale(t) + err_ref(t) + 1e-300,
scale(t) = sum_{m,l} w_m |a~_lm| (lambda_lm^2 + lambda_l-1,m^2)^(1/2) at ring t (both accumulators for the complex
synthesis): the fp64 recurrence and the seed carry ~(l + m) eps relative to the pair the recurrence holds, and the device
GEMM's ~2L eps sum |At| lies below it.  err_ref(t) is synth_rings' bound on the evaluator's own fp64 ring transform.
Each case prints max err / bar and max err / (L eps max|f|).
"""
import functools

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import transforms as T

from test_transforms_host import FOURPI, LD, berezin_ld, legendre_sums, synth_rings

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# (entry point, isreal, berezin): shr2fun with and without Berezin, the complex synthesis, and a real synthesis of
# complex input (Im a_l0 must be ignored)
MODES = [("shr", True, True), ("shr", True, False), ("shc", False, False), ("shc", True, True)]
DENSE = [(L, spec, mode) for L in (511, 512, 513, 1024, 1025, 2047, 2048) for spec in ("white", "decay")
         for mode in MODES]
# (the evaluator's cost grows as L^2 per ring and coefficient set: two modes per spectrum at 4096, one at 8192.  Both
# 8192 cases go without Berezin: w_l ~ exp(-l^2/L) is 3e-27 at l = 1000 and below 1e-300 from l = 3316 on, so a Berezin
# case cannot see the high orders -- the Fourier stage's second half or the seeds of m >= 4096 could be wrong unnoticed.)
DENSE += [(4096, "white", MODES[0]), (4096, "white", MODES[2]), (4096, "decay", MODES[1]), (4096, "decay", MODES[3])]
DENSE += [(8192, "white", ("shr", True, False)), (8192, "decay", ("shc", False, False))]


def _mode_id(mode):
    entry, isreal, berezin = mode
    return "%s-%s-%s" % (entry, "real" if isreal else "complex", "berezin" if berezin else "plain")


def _scale_l(L, berezin):
    return np.sqrt(FOURPI) * (berezin_ld(L) if berezin else np.ones(L, dtype=LD))


def _rings(L):
    """Both poles' three rings, L/2 +- 1, both sides of every 256-ring block boundary of the Legendre stage, both sides of
    a few 64-row tile boundaries of the Fourier stage (rows t, and rows L + t of the complex stack), 4 seeded rings."""
    r = {0, 1, 2, L - 3, L - 2, L - 1, L // 2 - 1, L // 2 + 1}
    for k in range(256, L, 256):
        r.update((k - 1, k))
    for t in (64, 64 * (L // 128), 64 * (L // 64)):
        r.update((t - 1, t))
    t = -L % 64                                     # row L + t opens a tile of the complex stack
    r.update((t, t + 63, t + 64 * (L // 128)))
    r.update(int(v) for v in np.random.default_rng(L).integers(0, L, 4))
    return np.array(sorted(v for v in r if 0 <= v < L))


def _coefficients(L, spec, seed):
    """Real omega (L^2) and complex omega (L^2): ||omega||_2 = 1, white or decaying like 1/(1 + l) as trajectory data."""
    rng = np.random.default_rng(seed)
    el = np.floor(np.sqrt(np.arange(L * L))).astype(np.int64)
    damp = 1.0 if spec == "white" else 1.0 / (1.0 + el)
    omr = rng.standard_normal(L * L) * damp
    omc = (rng.standard_normal(L * L) + 1j * rng.standard_normal(L * L)) * damp
    return omr / np.linalg.norm(omr), omc / np.linalg.norm(omc)


def _check(f, Gp, Gm, scale, L, isreal, label, ms=None):
    """f (the device's rows at the rings of G) against synth_rings of G, every column, to the bar; returns the ratios."""
    ref, err_ref = synth_rings(Gp, Gm, L, isreal, ms=ms)
    bar = (32 * L * EPS * scale + err_ref)[:, None] + 1e-300
    if isreal:
        err = np.abs(f - ref)
    else:
        err = np.maximum(np.abs(f.real - ref.real), np.abs(f.imag - ref.imag))
    ratio = float((err / bar).max())
    rel = float(err.max() / (L * EPS * np.abs(ref).max()))
    print("%-44s max err %.3e  err/bar %.3e  err/(L eps max|f|) %.3e" % (label, float(err.max()), ratio, rel))
    bad = err > bar
    assert not bad.any(), (label, int(bad.sum()), ratio)
    return ratio, rel


@functools.lru_cache(maxsize=1)
def _dense_reference(L, spec):
    """The evaluator's sums at _rings(L) for every mode of DENSE at (L, spec), in one shared walk."""
    omr, omc = _coefficients(L, spec, 7 * L + (spec == "decay"))
    modes = [mode for LL, sp, mode in DENSE if (LL, sp) == (L, spec)]
    coeffs = [T.shr2shc(omr) if entry == "shr" else omc for entry, _, _ in modes]
    sums = legendre_sums(coeffs, L, _rings(L), neg=[not isreal for _, isreal, _ in modes],
                         scale_l=[_scale_l(L, berezin) for _, _, berezin in modes])
    return omr, omc, dict(zip(modes, sums))


@pytest.mark.parametrize("L, spec, mode", DENSE, ids=["%d-%s-%s" % (L, s, _mode_id(m)) for L, s, m in DENSE])
def test_dense_sampled_rings(L, spec, mode):
    entry, isreal, berezin = mode
    omr, omc, sums = _dense_reference(L, spec)
    if entry == "shr":
        f = T.shr2fun(omr, N=L, berezin=berezin)
    else:
        f = T.shc2fun(omc, isreal=isreal, N=L, berezin=berezin)
    assert f.shape == (L, 2 * L - 1) and f.dtype == (np.float64 if isreal else np.complex128)
    Gp, Gm, scale = sums[mode]
    _check(f[_rings(L)], Gp, Gm, scale, L, isreal, "dense L=%d %s %s" % (L, spec, _mode_id(mode)))


def _few_orders(L):
    y = 100                                         # with L-1-y: the two halves of one Legendre workgroup
    return np.unique([m for m in (0, 1, 2, 63, 64, 255, 256, y, L - 1 - y, L // 2, L - 2, L - 1) if 0 <= m < L])


@pytest.mark.parametrize("L", [513, 2048, 8191])
@pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])
def test_few_orders_every_degree_every_point(L, isreal):
    """Coefficients nonzero for every l >= m at a dozen orders m only (both signs), zero elsewhere; every ring and every
    column checked: every Legendre workgroup that holds one of these orders, every Fourier tile and every edge tile.  The
    real case runs shr2fun with Berezin (multipliers down to ~0 at l ~ L), the complex one without."""
    ms = _few_orders(L)
    rng = np.random.default_rng(L + isreal)
    idx = np.concatenate([el * el + el + s * m for m in ms for el in [np.arange(m, L)] for s in ((1, -1) if m else (1,))])
    if isreal:
        om = np.zeros(L * L)
        om[idx] = rng.standard_normal(len(idx))
        f = T.shr2fun(om, N=L, berezin=True)
        coeffs, berezin = T.shr2shc(om), True
    else:
        om = np.zeros(L * L, dtype=complex)
        om[idx] = rng.standard_normal(len(idx)) + 1j * rng.standard_normal(len(idx))
        f = T.shc2fun(om, isreal=False, N=L, berezin=False)
        coeffs, berezin = om, False
    Gp, Gm, scale = legendre_sums(coeffs, L, np.arange(L), neg=not isreal, scale_l=_scale_l(L, berezin), ms=ms)
    worst = (0.0, 0.0)
    for r0 in range(0, L, 1024):
        rows = slice(r0, min(L, r0 + 1024))
        got = _check(f[rows], Gp[:, rows], None if Gm is None else Gm[:, rows], scale[rows], L, isreal,
                     "few orders L=%d %s rings %d.." % (L, "real" if isreal else "complex", r0), ms=ms)
        worst = tuple(max(a, b) for a, b in zip(worst, got))
    print("few orders L=%d %s: worst err/bar %.3e, err/(L eps max|f|) %.3e" % ((L, "real" if isreal else "complex") + worst))


def test_trimmed_and_padded_arrays_at_1025():
    """k_sht_pack's n_valid at L = 1025: coefficients past L^2 are ignored (trimmed), entries past the array are zero
    (padded; shr2fun converts whole degrees only, as shr2shc does), for both entry points."""
    L = 1025
    rng = np.random.default_rng(1025)
    n_trim, n_pad = (L + 1) ** 2, L * L - L
    cases = [("shr", n_trim), ("shr", n_pad), ("shc", n_trim), ("shc", n_pad)]
    arrays, coeffs = [], []
    for entry, n in cases:
        if entry == "shr":
            om = rng.standard_normal(n)
            coeffs.append(T.shr2shc(om))          # zero past the last whole degree
        else:
            om = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            coeffs.append(om)
        arrays.append(om)
    rings = _rings(L)
    sums = legendre_sums([c[:L * L] for c in coeffs], L, rings, neg=[e == "shc" for e, _ in cases],
                         scale_l=_scale_l(L, True))
    for (entry, n), om, (Gp, Gm, scale) in zip(cases, arrays, sums):
        if entry == "shr":
            f = T.shr2fun(om, N=L)
        else:
            f = T.shc2fun(om, N=L)
        _check(f[rings], Gp, Gm, scale, L, entry == "shr", "n_valid L=%d %s n=%d" % (L, entry, n))


def test_trajectory_fun_at_2048_vs_evaluator():
    """DeviceTrajectory.fun() at N = 2048, with and without Berezin and for the half bandwidth ('funhalf'), against the
    evaluator on the coefficients tr.shr() gives: the user-facing path checked independently of shr2fun."""
    from oracle import isomp_oracle
    N = 2048
    tr = qfa.DeviceTrajectory(isomp_oracle.make_W0(N, 3))
    try:
        om = tr.shr()
        half = (N // 2) ** 2
        om_half = tr.shr(half)
        runs = [(N, om, True, tr.fun()), (N, om, False, tr.fun(berezin=False)), (N // 2, om_half, True, tr.fun(half))]
    finally:
        tr.ctx.close()
    for L, omega, berezin, f in runs:
        assert f.shape == (L, 2 * L - 1)
        rings = _rings(L)
        Gp, Gm, scale = legendre_sums(T.shr2shc(omega), L, rings, scale_l=_scale_l(L, berezin))
        _check(f[rings], Gp, Gm, scale, L, True, "trajectory fun L=%d berezin=%s" % (L, berezin))
