"""GPU tests of the stochastic band-limited forcing (qf_set_stochastic_forcing, k_stoch_draw, quflow_amd.StochasticForcing):
the device draw against the numpy mirror, the pattern against the existing shr2mat, runs with the forcing installed against
the same numbers as a host callable, the resident trajectory, solve, and the refusals.

Only the draw has a tolerance (the device's log / sincos against numpy's): see test_draw_equals_the_mirror.  Everything else
is an EQUALITY: the reference of a run is a host callable g(P, W, time), written below from `coefficients(n)`, the existing
`shr2mat` and the mirror lines of tests/test_hip_forcing.py, given as `forcing=g, time=0.0`; it takes the host-hook route
(qf_isomp_hooked with a forcing hook), which tests/test_hip_parity.py pins to the reference's fixtures.  States must be
np.array_equal, `iterations` / `number_of_maxit` / `tol_auto` ==.

Data: a random skew-Hermitian state from a seeded default_rng, scaled to |W|_F = sqrt(N); dt = 0.25 hbar(N)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

QF_ERR_INVALID, QF_ERR_STATE, QF_ERR_UNSUPPORTED = 1, 4, 6          # include/quflow_hip.h


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


# ----------------------------------------------------------------------------- data (made once, read only)
_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        a = make()
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def skew(N, seed, scale=1.0):
    """A random, exactly skew-Hermitian (N,N) matrix with Frobenius norm scale * sqrt(N)."""
    def make():
        rng = np.random.default_rng(seed)
        A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        W = A - A.conj().T
        W = W / (np.linalg.norm(W, "fro") / np.sqrt(N))
        W = W * scale
        assert np.array_equal(W, -W.conj().T)
        return W
    return _cached(("skew", N, seed, scale), make)


SEED = 0x5EED00012345678         # (both key words in use)
BAND = (2, 5)


def band_sigma(l_min, l_max):
    """One amplitude per l, none a power of two: s = sigma_l * inv is a rounded product."""
    return 0.3 + 0.001 * np.arange(l_min, l_max + 1)


def run_params(N):
    """All three affine terms at sizes of a forced-dissipative run, and a band whose kick per step is a few percent of the
    state: friction, a drag on the stream function, a viscosity whose largest eigenvalue (~ N^2) stays 0.1."""
    return dict(l_min=BAND[0], l_max=BAND[1], sigma=0.1 * band_sigma(*BAND) / 0.3, seed=SEED, a_W=-0.02, a_P=0.05,
                a_lap=0.1 / (N * N))


def no_host_class(qfa):
    """A StochasticForcing whose host methods raise: a run with it succeeds only if the device never came back to the host."""
    class NoHost(qfa.StochasticForcing):
        def _host(self, *a, **k):
            raise AssertionError("the installed stochastic forcing came back to the host")
        draw_host = coefficients = pattern = as_callable = _device_pattern = _host
    return NoHost


def host_callable(qfa, sf, dt, N, step0=0, time0=0.0):
    """g(P, W, time): the step index from the time the loop evaluates the forcing at (t + dt/2), the pattern from
    coefficients(n) and the existing shr2mat, then the mirror lines of tests/test_hip_forcing.py."""
    a_W, a_P, a_lap = sf.a_W, sf.a_P, sf.a_lap
    seen = {}

    def g(P, W, time):
        n = max(step0 + int(round((time - time0 - dt / 2) / dt)), 0)
        if n not in seen:
            seen[n] = qfa.shr2mat(sf.coefficients(n, dt, N), N, streamed=True)
        F0 = seen[n]
        fr, fi = F0.real.copy(), F0.imag.copy()
        if a_W != 0.0:
            fr = fr + a_W * W.real
            fi = fi + a_W * W.imag
        if a_P != 0.0:
            fr = fr + a_P * P.real
            fi = fi + a_P * P.imag
        if a_lap != 0.0:
            L = qfa.laplace(np.ascontiguousarray(W))
            fr = fr + a_lap * L.real
            fi = fi + a_lap * L.imag
        out = np.empty(W.shape, dtype=np.complex128)
        out.real = fr
        out.imag = fi
        return out
    g.seen = seen
    return g


# ----------------------------------------------------------------------------- 1. the draw against the mirror
DRAW_CASES = [(3, (1, 2)), (33, (2, 5)), (65, (1, 64)), (300, (1, 299))]
DRAW_STEPS = [0, 1, 2 ** 32 + 5]
DRAW_D = 3.4652          # max |device - mirror| / (eps * s) measured on the MI355X over DRAW_CASES x DRAW_STEPS
DRAW_BAR = 4 * DRAW_D


@pytest.mark.parametrize("N,band", DRAW_CASES)
def test_draw_equals_the_mirror(qfa, N, band):
    """coefficients(n, dt, N) (k_stoch_draw on the device) against draw_host(n, dt) (numpy) for n = 0, 1 and 2^32 + 5 (the
    counter's high word).  (65, [1,64]) is a full band; (300, [1,299]) gives 90,000 entries, odd and even l_min^2 between the
    cases, and J = 300 columns cross the matvec's 256-column chunk.  Zeros outside the band are exact.  Inside it the two
    differ only by the device's log / sincos against libm's: with s = sigma_l / sqrt(dt) the scale of an entry,

        d = max |device - mirror| / (eps * s)      measured on the MI355X over all these cases:  d = 3.4652

    (the largest of a bounded few-ulp rounding error of r cos t, r sin t over a finite sample, |xi| up to ~4.5), and the
    bar is 4 d = 13.86; by the rule it may never exceed 64 -- above that the formulas differ, which is no rounding."""
    assert DRAW_BAR <= 64
    dt = 0.25 * qfa.hbar(N)
    l_min, l_max = band
    sf = qfa.StochasticForcing(l_min, l_max, band_sigma(l_min, l_max), seed=SEED)
    el = np.floor(np.sqrt(np.arange((l_max + 1) ** 2))).astype(int)
    s = np.zeros((l_max + 1) ** 2)
    s[l_min ** 2:] = sf.sigma[el[l_min ** 2:] - l_min] * (1.0 / np.sqrt(dt))
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for n in DRAW_STEPS:
        dev, host = sf.coefficients(n, dt, N), sf.draw_host(n, dt)
        assert dev.shape == host.shape == ((l_max + 1) ** 2,) and dev.dtype == np.float64
        assert not np.any(dev[:l_min ** 2]) and not np.any(host[:l_min ** 2])
        assert np.all(np.isfinite(dev)) and np.count_nonzero(dev[l_min ** 2:]) >= dev.size - l_min ** 2 - 1
        d = float((np.abs(dev - host)[l_min ** 2:] / (eps * s[l_min ** 2:])).max())
        worst = max(worst, d)
        print("draw N=%d band=%s n=%d: d = %.3f, max |xi| = %.2f" % (N, band, n, d, float(np.abs(host[l_min ** 2:] / s[l_min ** 2:]).max())))
        assert d <= DRAW_BAR, (N, band, n, d)
    assert sf.step == 0
    # other steps are other numbers
    assert not np.array_equal(sf.coefficients(0, dt, N), sf.coefficients(1, dt, N))


# ----------------------------------------------------------------------------- 2. the pattern
@pytest.mark.parametrize("N,band", DRAW_CASES + [(1024, (20, 24))])
def test_pattern_equals_shr2mat_of_the_coefficients(qfa, N, band):
    dt = 0.25 * qfa.hbar(N)
    l_min, l_max = band
    sf = qfa.StochasticForcing(l_min, l_max, band_sigma(l_min, l_max), seed=SEED, step=3)
    for n in (0, 2 ** 32 + 5):
        om = sf.coefficients(n, dt, N)
        F0 = sf.pattern(n, dt, N)
        want = qfa.shr2mat(om, N, streamed=True)
        assert F0.dtype == np.complex128 and F0.shape == (N, N)
        assert np.array_equal(F0, want), (N, band, n, float(np.abs(F0 - want).max()))
        if N <= 65:
            assert np.array_equal(F0, qfa.shr2mat(om, N, streamed=False))
        assert np.array_equal(F0, -F0.conj().T)
        i, j = np.indices((N, N))
        assert not np.any(F0[np.abs(i - j) > l_max])
        assert np.any(F0[np.abs(i - j) == l_max]) and np.any(np.diag(F0))
    assert sf.step == 3               # asking for a pattern consumes nothing
    # a narrower band after a wider one on the same context: the wider band's outer diagonals are gone
    if l_max - l_min >= 2:
        g = qfa.StochasticForcing(l_min, l_max - 1, band_sigma(l_min, l_max - 1), seed=SEED)
        F1 = g.pattern(0, dt, N)
        assert np.array_equal(F1, qfa.shr2mat(g.coefficients(0, dt, N), N, streamed=True))
        assert not np.any(F1[np.abs(i - j) > l_max - 1])


# ----------------------------------------------------------------------------- 3. runs: installed == host callable
def variant_kwargs(qfa, N, variant):
    if variant == "plain":
        return {}
    if variant == "strang":
        return {"strang_splitting": qfa.ViscDampStep(nu=1e-4, alpha=0.01)}
    if variant == "coriolis":
        return {"hamiltonian": qfa.TridiagonalHamiltonian.poisson(N, offset=qfa.coriolis(N, 0.5))}
    if variant == "reinitialize":
        return {"reinitialize": True}
    if variant == "minit":
        return {"minit": 2}
    raise KeyError(variant)


def run_isomp(qfa, W0, dt, steps, forcing, **kw):
    stats = {"iterations": 0.0}
    W = qfa.isomp(np.array(W0), dt, steps=steps, forcing=forcing, stats=stats, **kw)
    return W, stats


def isomp_reference(qfa, N, variant):
    """The 5-step host-callable run of a variant, made once: (state, stats)."""
    def make():
        dt = 0.25 * qfa.hbar(N)
        g = host_callable(qfa, qfa.StochasticForcing(**run_params(N)), dt, N)
        W, stats = run_isomp(qfa, skew(N, 0), dt, 5, g, time=0.0, **variant_kwargs(qfa, N, variant))
        assert sorted(g.seen) == [0, 1, 2, 3, 4]          # one pattern per step, whatever the iterations
        return (W, dict(stats))
    return _cached(("isomp_ref", N, variant), make)


def same_run(W, stats, Wr, sr):
    assert np.array_equal(W, Wr), float(np.abs(W - Wr).max())
    assert stats["iterations"] == sr["iterations"] and stats["number_of_maxit"] == sr["number_of_maxit"]
    assert stats["tol_auto"] == sr["tol_auto"]
    assert stats["iterations"] >= 2.0                 # the fixed-point loop really iterated


VARIANTS = ["plain", "strang", "coriolis", "reinitialize", "minit"]


@pytest.mark.parametrize("N", [33, 64])
@pytest.mark.parametrize("variant", VARIANTS)
def test_isomp_installed_equals_host_callable(qfa, N, variant):
    dt = 0.25 * qfa.hbar(N)
    Wr, sr = isomp_reference(qfa, N, variant)
    sf = no_host_class(qfa)(**run_params(N))
    W, stats = run_isomp(qfa, skew(N, 0), dt, 5, sf, **variant_kwargs(qfa, N, variant))
    print("isomp N=%d %s: iterations %r / %r, max|diff| %.3e" % (N, variant, stats["iterations"], sr["iterations"],
                                                                   float(np.abs(W - Wr).max())))
    same_run(W, stats, Wr, sr)
    assert sf.step == 5
    assert not np.array_equal(W, skew(N, 0))
    # the context is left without a forcing: the next default call on it is the unforced one
    from quflow_amd.context import get_stepper_context
    ctx = get_stepper_context(N)
    out = np.empty((N, N), dtype=np.complex128)
    assert ctx._lib.qf_forcing(ctx.handle, out.ctypes.data, out.ctypes.data, out.ctypes.data) == QF_ERR_STATE
    n = ctypes.c_ulonglong()
    assert ctx._lib.qf_stochastic_tell(ctx.handle, ctypes.byref(n)) == QF_ERR_STATE


@pytest.mark.parametrize("N", [33, 64])
@pytest.mark.parametrize("variant", VARIANTS)
def test_as_callable_equals_host_callable(qfa, N, variant):
    dt = 0.25 * qfa.hbar(N)
    Wr, sr = isomp_reference(qfa, N, variant)
    sf = qfa.StochasticForcing(**run_params(N))
    W, stats = run_isomp(qfa, skew(N, 0), dt, 5, sf.as_callable(dt, N), time=0.0, **variant_kwargs(qfa, N, variant))
    same_run(W, stats, Wr, sr)
    assert sf.step == 0               # the callable is a pure function of the time: it consumes nothing


def test_as_callable_resumes_from_the_counter_and_time(qfa):
    """Two chunks through as_callable -- the second from the counter and the time the first left -- are the 5-step run with
    reinitialize (the iteration vector restarts per call)."""
    N = 33
    dt = 0.25 * qfa.hbar(N)
    Wr, _ = isomp_reference(qfa, N, "reinitialize")
    sf = qfa.StochasticForcing(**run_params(N))
    W = qfa.isomp(np.array(skew(N, 0)), dt, steps=2, forcing=sf.as_callable(dt, N), time=0.0, reinitialize=True)
    sf.step = 2
    W = qfa.isomp(W, dt, steps=3, forcing=sf.as_callable(dt, N, time0=2 * dt), time=2 * dt, reinitialize=True)
    assert np.array_equal(W, Wr)


def test_another_seed_is_another_run_and_the_force_moves_the_state(qfa):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    Wr, _ = isomp_reference(qfa, N, "plain")
    W, _ = run_isomp(qfa, skew(N, 0), dt, 5, qfa.StochasticForcing(**dict(run_params(N), seed=SEED + 1)))
    assert float(np.abs(W - Wr).max()) > 1e-6
    U, _ = run_isomp(qfa, skew(N, 0), dt, 5, None)
    assert float(np.abs(Wr - U).max()) > 1e-6
    # zero amplitudes: the affine forcing alone
    Z, _ = run_isomp(qfa, skew(N, 0), dt, 5, qfa.StochasticForcing(**dict(run_params(N), sigma=0.0)))
    p = run_params(N)
    A, _ = run_isomp(qfa, skew(N, 0), dt, 5, qfa.AffineForcing(a_W=p["a_W"], a_P=p["a_P"], a_lap=p["a_lap"]))
    assert float(np.abs(Z - A).max()) <= 1e-13 and float(np.abs(Z - Wr).max()) > 1e-6


# ----------------------------------------------------------------------------- 4. the resident trajectory
@pytest.mark.parametrize("N", [33, 64])
@pytest.mark.parametrize("variant", ["plain", "strang", "coriolis"])
def test_resident_trajectory_equals_the_run(qfa, N, variant):
    dt = 0.25 * qfa.hbar(N)
    Wr, sr = isomp_reference(qfa, N, variant)
    kw = variant_kwargs(qfa, N, variant)
    sf = no_host_class(qfa)(**run_params(N))
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=sf, **kw)
    try:
        assert tr.stochastic_tell() == 0
        st = tr.advance(dt, 5)
        W = tr.download()
        assert np.array_equal(W, Wr), float(np.abs(W - Wr).max())
        assert st["iterations"] == sr["iterations"] and st["number_of_maxit"] == sr["number_of_maxit"]
        assert st["tol"] == sr["tol_auto"]
        assert sf.step == 5 and tr.stochastic_tell() == 5
    finally:
        tr.ctx.close()


def test_resident_chunks_consume_consecutive_counters(qfa):
    """advance(2) then advance(3) with reinitialize: the single 5-step reinitialize run; the counter goes 0, 2, 5.  A pattern
    asked for between the advances (on the trajectory's own context) and tr.shr() change nothing, and tr.shr() is mat2shr of
    the downloaded state: the forcing's staging buffers are its own."""
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    N = 33
    dt = 0.25 * qfa.hbar(N)
    Wr, _ = isomp_reference(qfa, N, "reinitialize")
    sf = no_host_class(qfa)(**run_params(N))
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=sf)
    try:
        tr.advance(dt, 2, reinitialize=True)
        assert tr.stochastic_tell() == 2 and sf.step == 2
        W2 = tr.download()
        om = tr.shr()
        assert np.array_equal(om, qfa.mat2shr(W2))
        F0 = np.empty((N, N), dtype=np.complex128)
        coef = np.empty((BAND[1] + 1) ** 2)
        _lib.check(tr._lib.qf_stochastic_pattern(tr.ctx.handle, ctypes.c_ulonglong(99), dt, ptr(coef), ptr(F0)))
        assert np.array_equal(F0, qfa.shr2mat(coef, N, streamed=True)) and np.any(F0)
        assert tr.stochastic_tell() == 2
        assert np.array_equal(tr.shr(), om)                      # (what the transforms left on the device is still theirs)
        assert np.array_equal(tr.download(), W2)
        tr.advance(dt, 3, reinitialize=True)
        assert tr.stochastic_tell() == 5 and sf.step == 5
        assert np.array_equal(tr.download(), Wr)
        assert np.array_equal(tr.shr(), qfa.mat2shr(Wr))
        # seek: back to counter 2 on the state after two steps reproduces steps 2..4
        tr.upload(W2)
        tr.stochastic_seek(2)
        assert sf.step == 2
        tr.advance(dt, 3, reinitialize=True)
        assert np.array_equal(tr.download(), Wr) and sf.step == 5
    finally:
        tr.ctx.close()
    # step=: a fresh trajectory from the state after two steps
    resumed = qfa.StochasticForcing(**dict(run_params(N), step=2))
    tr = qfa.DeviceTrajectory(W2, forcing=resumed)
    try:
        tr.advance(dt, 3, reinitialize=True)
        assert np.array_equal(tr.download(), Wr) and resumed.step == 5
    finally:
        tr.ctx.close()


def test_set_forcing_switches_between_none_affine_and_stochastic(qfa):
    """Chunks of two steps: stochastic, none, affine, stochastic again (its counter carries on at 2).  Reference: the same
    chunks as host-in isomp calls (installed for a call each: equal to the host callable by the tests above)."""
    N = 33
    dt = 0.25 * qfa.hbar(N)
    p = run_params(N)
    aff = qfa.AffineForcing(F0=skew(N, 100, 0.1), a_W=p["a_W"], a_lap=p["a_lap"])
    ref_sf, sf = qfa.StochasticForcing(**p), no_host_class(qfa)(**p)
    W = np.array(skew(N, 0))
    want = []
    for f in (ref_sf, None, aff, ref_sf):
        W = qfa.isomp(W, dt, steps=2, forcing=f)
        want.append(W.copy())
    assert ref_sf.step == 4
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=sf)
    try:
        for chunk, f in enumerate((sf, None, aff, sf)):
            if chunk:
                tr.set_forcing(f)
            tr.advance(dt, 2)
            assert np.array_equal(tr.download(), want[chunk]), chunk
            if f is None or f is aff:
                with pytest.raises(ValueError, match="no StochasticForcing"):
                    tr.stochastic_tell()
        assert sf.step == 4 and tr.stochastic_tell() == 4
        assert not np.array_equal(want[0], want[1])
    finally:
        tr.ctx.close()


def test_resident_trajectory_refusals(qfa):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    sf = qfa.StochasticForcing(**run_params(N))
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=sf)
    try:
        with pytest.raises(NotImplementedError, match="Compensated sum with forcing is not yet implemented."):
            tr.advance(dt, 2, compsum=True)
        with pytest.raises(NotImplementedError, match="forcing"):
            tr.advance_erk("rk4", dt, 1)
        with pytest.raises(NotImplementedError, match="forcing"):
            tr.advance_lu("isomp_simple", dt, 1)
        from quflow_amd import _lib
        with pytest.raises(_lib.QuflowHipError, match="QF_ERR_INVALID.*step size"):
            tr.advance(0.0, 1)
        assert np.array_equal(tr.download(), skew(N, 0)) and sf.step == 0
    finally:
        tr.ctx.close()
    ens = qfa.DeviceEnsemble([skew(N, 0), skew(N, 1)])
    try:
        ens.members[1].set_forcing(sf)
        with pytest.raises(NotImplementedError, match="DeviceEnsemble"):
            ens.advance(dt, 1)
    finally:
        ens.close()
    if qfa.laplacian.single_precision_on_device():
        with pytest.raises(NotImplementedError, match="complex128"):
            qfa.DeviceTrajectory(skew(N, 0).astype(np.complex64), forcing=sf)
    W = np.array(skew(N, 0))
    with pytest.raises(NotImplementedError, match="Compensated sum with forcing is not yet implemented."):
        qfa.isomp(W, dt, steps=2, forcing=sf, compsum=True)
    assert np.array_equal(W, skew(N, 0)) and sf.step == 0


# ----------------------------------------------------------------------------- 5. solve
def test_solve_resident_equals_host_in(qfa):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    v = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
    seen = {}
    for resident in (True, False):
        sf = no_host_class(qfa)(**run_params(N))
        states = []
        W = qfa.solve(np.array(skew(N, 0)), dt, steps=6, steps_out=3, integrator=qfa.isomp, forcing=sf, strang_splitting=v,
                      resident=resident, progress_bar=False,
                      callback=lambda W, **kw: states.append((np.array(W), kw.get("iterations"), kw.get("number_of_maxit"))))
        assert len(states) == 2 and np.array_equal(states[-1][0], W)
        assert sf.step == 6
        seen[resident] = states
    for (Wa, ia, ma), (Wb, ib, mb) in zip(seen[True], seen[False]):
        assert np.array_equal(Wa, Wb)
        assert ia == ib and ma == mb
    # ... and the chunked host-in calls written out
    sf = qfa.StochasticForcing(**run_params(N))
    W = np.array(skew(N, 0))
    for chunk in range(2):
        W = qfa.isomp(W, dt, steps=3, forcing=sf, strang_splitting=v)
        assert np.array_equal(W, seen[True][chunk][0])
    from quflow_amd import simulation
    assert simulation._resident_kind(qfa.isomp, {"forcing": sf, "strang_splitting": v}, skew(N, 0)) == 'single'


RESUME_CHILD = """
import sys
sys.path.insert(0, %r)
import quflow_amd as qfa
from quflow_amd.simulation import Simulation, solve
sim = Simulation(sys.argv[1])
assert sim['forcing'].step == 3, sim['forcing'].step
solve(sim, progress_bar=False)
print("child ok", sim['forcing'].step)
"""


def test_a_stored_simulation_resumed_in_a_fresh_process_continues_the_sequence(qfa, tmp_path):
    from quflow_amd.simulation import Simulation, solve
    N = 33
    dt = 0.25 * qfa.hbar(N)
    path = str(tmp_path / "stochastic_run")
    sim = Simulation(path, state=np.array(skew(N, 0)))
    sim['dt'] = dt
    sim['steps'] = 3
    sim['steps_out'] = 3
    sim['integrator'] = qfa.isomp
    sim['forcing'] = qfa.StochasticForcing(**run_params(N))
    solve(sim, progress_bar=False)
    assert sim['forcing'].step == 3               # the record follows the counter
    r = subprocess.run([sys.executable, "-c", RESUME_CHILD % REPO, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok 6" in r.stdout, (r.stdout, r.stderr)
    sim = Simulation(path)
    assert sim['forcing'].step == 6
    sf = qfa.StochasticForcing(**run_params(N))
    W = np.array(skew(N, 0))
    for row in (1, 2):
        W = qfa.isomp(W, dt, steps=3, forcing=sf)
        assert np.array_equal(sim['mat', row], W), row


# ----------------------------------------------------------------------------- 6. refusals
def test_entry_points_that_cannot_apply_the_noise_refuse(qfa):
    from quflow_amd.context import Context, ptr
    from quflow_amd import _lib
    N = 33
    dt = 0.25 * qfa.hbar(N)
    W0 = np.array(skew(N, 0))
    ctx, fresh = Context(N), Context(N)
    try:
        lib = ctx._lib
        st = _lib.IsompStats()
        e, s = ctypes.c_double(), ctypes.c_double()
        five = (ctypes.c_double * 5)()
        qfa.StochasticForcing(**run_params(N)).install(ctx)
        _lib.check(lib.qf_upload_W(ctx.handle, ptr(W0)))
        stack = np.stack([W0, np.array(skew(N, 5))])
        _lib.check(lib.qf_states_upload(ctx.handle, ptr(stack), 2))
        hooks = _lib.IsompHooks()
        hooks.skewh = hooks.solve_skewh = 1
        handles = (ctypes.c_void_p * 1)(ctx.handle)
        host = np.array(W0)
        hstack = stack.copy()
        rk4 = _lib.ERK_METHODS["rk4"]
        calls = {
            "qf_isomp": lambda: lib.qf_isomp(ctx.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st)),
            "qf_isomp_continue": lambda: lib.qf_isomp_continue(ctx.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st)),
            "qf_isomp_diag": lambda: lib.qf_isomp_diag(ctx.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st), ctypes.byref(e),
                                                       ctypes.byref(s)),
            "qf_isomp_multi": lambda: lib.qf_isomp_multi(handles, 1, dt, 2, -1.0, 1, 10, ctypes.byref(st)),
            "qf_isomp_states": lambda: lib.qf_isomp_states(ctx.handle, ptr(hstack), 2, dt, 1, -1.0, 1, 10, 0, 0, ctypes.byref(st)),
            "qf_states_advance": lambda: lib.qf_states_advance(ctx.handle, dt, 1, -1.0, 1, 10, 0, 0, ctypes.byref(st)),
            "qf_states_advance_diag": lambda: lib.qf_states_advance_diag(ctx.handle, dt, 1, -1.0, 1, 10, 0, 1, ctypes.byref(st), five),
            "qf_erk": lambda: lib.qf_erk(ctx.handle, rk4, dt, 1, 1),
            "qf_erk_states": lambda: lib.qf_erk_states(ctx.handle, ptr(hstack), 2, rk4, dt, 1, 1),
            "qf_erk_states_hooked": lambda: lib.qf_erk_states_hooked(ctx.handle, ptr(hstack), 2, rk4, dt, 1, ctypes.byref(hooks)),
            "qf_isomp_simple": lambda: lib.qf_isomp_simple(ctx.handle, dt, 1),
            "qf_isomp_quasinewton": lambda: lib.qf_isomp_quasinewton(ctx.handle, dt, 1, -1.0, 10, ctypes.byref(st)),
            "qf_isomp_simple_hooked": lambda: lib.qf_isomp_simple_hooked(ctx.handle, dt, 1, ctypes.byref(hooks)),
            "qf_isomp_quasinewton_hooked": lambda: lib.qf_isomp_quasinewton_hooked(ctx.handle, dt, 1, -1.0, 10, ctypes.byref(st),
                                                                                   ctypes.byref(hooks)),
            "qf_isomp_hooked on a stack": lambda: lib.qf_isomp_hooked(ctx.handle, ptr(hstack), 2, dt, 1, -1.0, 1, 10, 0, 0,
                                                                      ctypes.byref(hooks), ctypes.byref(st)),
            # the two that follow an affine forcing and refuse a stochastic one
            "qf_erk_hooked": lambda: lib.qf_erk_hooked(ctx.handle, ptr(host), rk4, dt, 1, ctypes.byref(hooks)),
            "qf_forcing": lambda: lib.qf_forcing(ctx.handle, ptr(host), ptr(host), ptr(host)),
        }
        if qfa.laplacian.single_precision_on_device():
            w32 = W0.astype(np.complex64)
            _lib.check(lib.qf_c64_upload_W(ctx.handle, ptr(w32)))
            calls["qf_c64_isomp"] = lambda: lib.qf_c64_isomp(ctx.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st))
            calls["qf_c64_isomp_continue"] = lambda: lib.qf_c64_isomp_continue(ctx.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st))
            calls["qf_c64_isomp_multi"] = lambda: lib.qf_c64_isomp_multi(handles, 1, dt, 2, -1.0, 1, 10, ctypes.byref(st))
        for name, call in calls.items():
            rc = call()
            msg = lib.qf_last_error().decode("utf-8", "replace")
            assert rc == QF_ERR_UNSUPPORTED, (name, rc, msg)
            assert "forcing" in msg, (name, msg)
        # nothing was advanced, nothing was consumed
        got = np.empty_like(W0)
        _lib.check(lib.qf_download_W(ctx.handle, ptr(got)))
        assert np.array_equal(got, W0) and np.array_equal(host, W0) and np.array_equal(hstack, stack)
        n = ctypes.c_ulonglong(7)
        _lib.check(lib.qf_stochastic_tell(ctx.handle, ctypes.byref(n)))
        assert n.value == 0
        # cleared: the same call is a fresh context's
        _lib.check(lib.qf_clear_forcing(ctx.handle))
        assert lib.qf_stochastic_tell(ctx.handle, ctypes.byref(n)) == QF_ERR_STATE
        assert lib.qf_stochastic_seek(ctx.handle, 1) == QF_ERR_STATE
        assert lib.qf_stochastic_pattern(ctx.handle, 0, dt, None, None) == QF_ERR_STATE
        _lib.check(calls["qf_isomp"]())
        _lib.check(lib.qf_download_W(ctx.handle, ptr(got)))
        st2 = _lib.IsompStats()
        _lib.check(lib.qf_upload_W(fresh.handle, ptr(W0)))
        _lib.check(lib.qf_isomp(fresh.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st2)))
        want = np.empty_like(W0)
        _lib.check(lib.qf_download_W(fresh.handle, ptr(want)))
        assert np.array_equal(got, want) and not np.array_equal(got, W0)
        assert (st.total_iterations, st.number_of_maxit) == (st2.total_iterations, st2.number_of_maxit)
    finally:
        ctx.close()
        fresh.close()


def test_bad_arguments_are_invalid_and_leave_the_context_usable(qfa):
    from quflow_amd.context import Context, ptr
    from quflow_amd import _lib
    from quflow_amd.quantization import slab_bytes
    N = 33
    dt = 0.25 * qfa.hbar(N)
    ctx = Context(N)
    try:
        lib = ctx._lib
        cap = slab_bytes()
        sig = np.full(40, 0.1)

        def install(l_min, l_max, sigma=sig, a=(0.0, 0.0, 0.0), cap=cap):
            return lib.qf_set_stochastic_forcing(ctx.handle, l_min, l_max, None if sigma is None else ptr(sigma),
                                                 ctypes.c_ulonglong(1), ctypes.c_ulonglong(0), a[0], a[1], a[2],
                                                 ctypes.c_longlong(cap))
        neg, nan, inf = sig.copy(), sig.copy(), sig.copy()
        neg[2], nan[1], inf[0] = -0.1, np.nan, np.inf
        band_bytes = 8 * sum((N - m) * (6 - m) for m in range(6))        # 8 qf_slab_prefix(N, 6, 6)
        bad = {
            "l_min = 0": lambda: install(0, 3), "l_min < 0": lambda: install(-2, 3), "l_max < l_min": lambda: install(4, 3),
            "l_max = N": lambda: install(1, N), "null sigma": lambda: install(2, 5, sigma=None),
            "negative sigma": lambda: install(2, 5, sigma=neg), "nan sigma": lambda: install(2, 5, sigma=nan),
            "inf sigma": lambda: install(2, 5, sigma=inf), "nan coefficient": lambda: install(2, 5, a=(0.0, np.nan, 0.0)),
            "inf coefficient": lambda: install(2, 5, a=(np.inf, 0.0, 0.0)),
            "band basis over the cap": lambda: install(2, 5, cap=band_bytes - 1), "no cap": lambda: install(2, 5, cap=0),
        }
        for name, call in bad.items():
            assert call() == QF_ERR_INVALID, name
            assert lib.qf_last_error(), name
            n = ctypes.c_ulonglong()
            assert lib.qf_stochastic_tell(ctx.handle, ctypes.byref(n)) == QF_ERR_STATE, name       # nothing was installed
        # the cap itself is enough, the full band is a band, and the context works
        assert install(2, 5, cap=band_bytes) == 0
        assert install(1, N - 1) == 0
        assert install(2, 5) == 0
        for bad_dt in (0.0, -dt, np.inf, np.nan):
            assert lib.qf_stochastic_pattern(ctx.handle, 0, bad_dt, None, None) == QF_ERR_INVALID
        sf = qfa.StochasticForcing(2, 5, 0.1, seed=1)
        om = np.empty(36)
        _lib.check(lib.qf_stochastic_pattern(ctx.handle, 4, dt, ptr(om), None))
        assert np.array_equal(om, sf.coefficients(4, dt, N))
        # an affine forcing replaces the stochastic one; its pattern is uploaded whatever key the buffer carried before
        F0 = np.array(skew(N, 100, 0.1))
        for trial in range(2):
            assert install(2, 5) == 0
            _lib.check(lib.qf_stochastic_pattern(ctx.handle, 0, dt, None, None))
            _lib.check(lib.qf_set_forcing(ctx.handle, ptr(F0), ctypes.c_ulonglong(77), 0.0, 0.0, 0.0))
            n = ctypes.c_ulonglong()
            assert lib.qf_stochastic_tell(ctx.handle, ctypes.byref(n)) == QF_ERR_STATE
            out = np.empty((N, N), dtype=np.complex128)
            P = np.array(skew(N, 1))
            _lib.check(lib.qf_forcing(ctx.handle, ptr(P), ptr(P), ptr(out)))
            assert np.array_equal(out, F0), trial
    finally:
        ctx.close()


# ----------------------------------------------------------------------------- 7. the size class of the 64 x 64 kernels
def test_resident_equals_host_callable_n1024(qfa):
    N, band = 1024, (20, 24)
    dt = 0.25 * qfa.hbar(N)
    p = dict(l_min=band[0], l_max=band[1], sigma=0.1, seed=SEED, a_W=-0.02, a_P=0.05, a_lap=0.1 / (N * N))
    g = host_callable(qfa, qfa.StochasticForcing(**p), dt, N)
    Wr, sr = run_isomp(qfa, skew(N, 0), dt, 3, g, time=0.0)
    sf = no_host_class(qfa)(**p)
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=sf)
    try:
        st = tr.advance(dt, 3)
        W = tr.download()
    finally:
        tr.ctx.close()
    print("N=1024: iterations %r / %r, max|diff| %.3e" % (st["iterations"], sr["iterations"], float(np.abs(W - Wr).max())))
    assert np.array_equal(W, Wr)
    assert st["iterations"] == sr["iterations"] and st["number_of_maxit"] == sr["number_of_maxit"] and st["tol"] == sr["tol_auto"]
    assert st["iterations"] >= 2.0 and sf.step == 3 and sorted(g.seen) == [0, 1, 2]
