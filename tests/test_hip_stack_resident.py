"""The resident (k,N,N) stack: DeviceStackTrajectory / DeviceMHDTrajectory, qf_states_*, qf_mhd_diagnostics and the
resident branch of `solve` for magmp and for isomp on a stack.

Data: the MHD state of test_states_vs_oracle_large, (make_W0(N,1), solve_poisson(make_W0(N,2))), dt = 0.25 hbar(N), 3 steps.
On these inputs the oracle ends no step by maxit and takes at least 2 iterations per step (asserted on its stats in every
test that uses it), so the exit logic is exercised.  Sizes: 33 (guarded edge tiles), 64, 257 (odd, next solver chunk class),
1024 (stream-K upper-triangle second product).  The oracle runs once per size and is shared."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 3
_cache = {}


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def mhd_state(oracle, N):
    key = ("state", N)
    if key not in _cache:
        s = np.stack([oracle.make_W0(N, 1), oracle.solve_poisson(oracle.make_W0(N, 2)).copy()])
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def tracer_stack(oracle, N):
    key = ("stack", N)
    if key not in _cache:
        s = np.stack([oracle.make_W0(N, 1), oracle.solve_poisson(oracle.make_W0(N, 2)).copy(), oracle.make_W0_smooth(N, 3)])
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def check_oracle_stats(st, maxit_key):
    """What makes the case a test of the exit logic: no step ended by maxit, at least 2 iterations per step."""
    assert st[maxit_key] == 0
    assert st["iterations"] >= 2.0


def mhd_oracle(oracle, qfa, N):
    key = ("mhd_oracle", N)
    if key not in _cache:
        st = {"iterations": 0.0}
        W = oracle.magmp_fixedpoint(mhd_state(oracle, N).copy(), 0.25 * qfa.hbar(N), STEPS, stats=st)
        W.setflags(write=False)
        _cache[key] = (W, st)
    W, st = _cache[key]
    check_oracle_stats(st, "maxit")
    return W, st


def mhd_host(oracle, qfa, N):
    """qfa.magmp, the host-in / host-out path, on the same data (computed once per size)."""
    key = ("mhd_host", N)
    if key not in _cache:
        st = {"iterations": 0.0}
        W = qfa.magmp(mhd_state(oracle, N).copy(), 0.25 * qfa.hbar(N), STEPS, stats=st)
        W.setflags(write=False)
        _cache[key] = (W, st)
    return _cache[key]


def close(tr):
    tr.ctx.close()


# ----------------------------------------------------------------------------- 1. MHD against the oracle
@pytest.mark.parametrize("N", [33, 64, 257, 1024])
def test_mhd_vs_oracle(qfa, oracle, N):
    Wo, so = mhd_oracle(oracle, qfa, N)
    tr = qfa.DeviceMHDTrajectory(mhd_state(oracle, N))
    try:
        st = tr.advance(0.25 * qfa.hbar(N), STEPS)
        W = tr.download()
    finally:
        close(tr)
    err = maxabs(W, Wo)
    print("N=%d max error %.3e iterations %s / %s" % (N, err, st["iterations"], so["iterations"]))
    assert err <= 1e-12 * max(1.0, np.abs(Wo).max())
    assert st["iterations"] == so["iterations"]
    assert st["number_of_maxit"] == 0
    np.testing.assert_allclose(st["tol"], so["tol"], rtol=1e-12)
    assert np.array_equal(W[0], -W[0].conj().T) and np.array_equal(W[1], -W[1].conj().T)


# ----------------------------------------------------------------------------- 2. bit identity with the host path
@pytest.mark.parametrize("N", [33, 64, 257, 1024])
def test_mhd_bits_of_host_path(qfa, oracle, N):
    mhd_oracle(oracle, qfa, N)
    dt = 0.25 * qfa.hbar(N)
    Wh, sh = mhd_host(oracle, qfa, N)
    tr = qfa.DeviceMHDTrajectory(mhd_state(oracle, N))
    try:
        st = tr.advance(dt, STEPS)
        assert np.array_equal(tr.download(), Wh)
        assert st["iterations"] == sh["iterations"] and st["number_of_maxit"] == sh["maxit"] and st["tol"] == sh["tol"]
        # two calls are two calls of the host path: dX restarts from zero in each
        tr.upload(mhd_state(oracle, N))
        s2, s1 = tr.advance(dt, 2), tr.advance(dt, 1)
        h2, h1 = {"iterations": 0.0}, {"iterations": 0.0}
        Wh2 = qfa.magmp(qfa.magmp(mhd_state(oracle, N).copy(), dt, 2, stats=h2), dt, 1, stats=h1)
        assert np.array_equal(tr.download(), Wh2)
        assert (s2["iterations"], s1["iterations"]) == (h2["iterations"], h1["iterations"])
        assert (s2["tol"], s1["tol"]) == (h2["tol"], h1["tol"])
    finally:
        close(tr)


def test_mhd_bits_of_host_path_options(qfa, oracle):
    """A given tolerance, minit = 2 and reinitialize, once."""
    N = 64
    dt = 0.25 * qfa.hbar(N)
    kw = dict(tol=1e-11, minit=2, reinitialize=True)
    sh = {"iterations": 0.0}
    Wh = qfa.magmp(mhd_state(oracle, N).copy(), dt, STEPS, stats=sh, **kw)
    tr = qfa.DeviceMHDTrajectory(mhd_state(oracle, N))
    try:
        st = tr.advance(dt, STEPS, **kw)
        assert np.array_equal(tr.download(), Wh)
        assert st["iterations"] == sh["iterations"] and st["number_of_maxit"] == sh["maxit"]
    finally:
        close(tr)


# ----------------------------------------------------------------------------- 3. a stack of tracers, k = 3
@pytest.mark.parametrize("N", [33, 257, 1024])
def test_tracer_stack(qfa, oracle, N):
    dt = 0.25 * qfa.hbar(N)
    stack = tracer_stack(oracle, N)
    sh = {"iterations": 0.0}
    Wh = qfa.isomp(stack.copy(), dt, STEPS, stats=sh)
    tr = qfa.DeviceStackTrajectory(stack, magnetic=False)
    try:
        st = tr.advance(dt, STEPS)
        W = tr.download()
    finally:
        close(tr)
    assert np.array_equal(W, Wh)
    assert st["iterations"] == sh["iterations"] and st["number_of_maxit"] == sh["number_of_maxit"] and st["tol"] == sh["tol_auto"]
    if N <= 257:
        so = {"iterations": 0.0}
        Wo = oracle.isomp(stack.copy(), dt, STEPS, stats=so)
        check_oracle_stats(so, "number_of_maxit")
        err = maxabs(W, Wo)
        print("N=%d max error %.3e" % (N, err))
        assert err <= 1e-12
        assert st["iterations"] == so["iterations"]


# ----------------------------------------------------------------------------- 4. diagnostics
def numpy_mhd(oracle, state):
    W, T = state[0], state[1]
    P = oracle.solve_poisson(W.copy()).copy()
    LT = oracle.laplace(T.copy()).copy()
    return {"energy_kinetic": -oracle.inner_L2(W, P) / 2, "energy_magnetic": -oracle.inner_L2(T, LT) / 2,
            "cross_helicity": oracle.inner_L2(W, T), "magnetic_casimir": oracle.inner_L2(T, T) / 2,
            "enstrophy": oracle.inner_L2(W, W) / 2}


@pytest.mark.parametrize("which", ["advanced", "white"])
@pytest.mark.parametrize("N", [33, 257, 1024])
def test_mhd_diagnostics(qfa, oracle, N, which):
    dt = 0.25 * qfa.hbar(N)
    if which == "advanced":
        mhd_oracle(oracle, qfa, N)
        tr = qfa.DeviceMHDTrajectory(mhd_state(oracle, N))
    else:
        # white Theta: a wrong stencil edge shows at full weight
        tr = qfa.DeviceMHDTrajectory(np.stack([oracle.make_W0(N, 1), oracle.make_W0(N, 2)]))
    try:
        if which == "advanced":
            out = tr.advance(dt, STEPS, diagnostics=True)
        d = tr.diagnostics()
        if which == "advanced":
            # queued behind the last step or asked for afterwards: the same launches, the same bits
            assert {k: out[k] for k in d} == d
        state = tr.download()
    finally:
        close(tr)
    ref = numpy_mhd(oracle, state)
    for k in sorted(ref):
        print("N=%d %s %-16s device %.17g numpy %.17g" % (N, which, k, d[k], ref[k]))
    np.testing.assert_allclose(d["energy_kinetic"], ref["energy_kinetic"], rtol=1e-10)
    np.testing.assert_allclose(d["energy_magnetic"], ref["energy_magnetic"], rtol=1e-10)
    np.testing.assert_allclose(d["enstrophy"], ref["enstrophy"], rtol=1e-12)
    np.testing.assert_allclose(d["magnetic_casimir"], ref["magnetic_casimir"], rtol=1e-12)
    # X is a cancelling sum: an absolute bar from the sizes of its two factors
    bar = 1e-12 * np.sqrt(2 * ref["enstrophy"] * 2 * ref["magnetic_casimir"])
    assert abs(d["cross_helicity"] - ref["cross_helicity"]) <= bar
    assert d["energy"] == d["energy_kinetic"] + d["energy_magnetic"]
    # the sums are arranged as qf_diagnostics arranges them
    for j, keys in ((0, ("energy_kinetic", "enstrophy")), (1, (None, "magnetic_casimir"))):
        t1 = qfa.DeviceTrajectory(state[j])
        try:
            e, s = t1.diagnostics()
        finally:
            close(t1)
        if keys[0]:
            assert d[keys[0]] == e
        assert d[keys[1]] == s
    # host in, through the shared context
    assert qfa.physics.mhd_diagnostics(state) == d
    assert qfa.energy_mhd(state) == d["energy"]
    assert qfa.cross_helicity(state) == d["cross_helicity"]
    assert qfa.magnetic_energy(state[1]) == d["energy_magnetic"]


def test_tracer_diagnostics(qfa, oracle):
    N = 33
    stack = tracer_stack(oracle, N)
    tr = qfa.DeviceStackTrajectory(stack)
    try:
        d = tr.diagnostics()
    finally:
        close(tr)
    np.testing.assert_allclose(d["energy"], oracle.energy_euler(stack[0].copy()), rtol=1e-10)
    np.testing.assert_allclose(d["enstrophy"], oracle.enstrophy(stack[0].copy()), rtol=1e-12)
    assert len(d["members"]) == 3
    for j, (x0, half) in enumerate(d["members"]):
        np.testing.assert_allclose(half, oracle.inner_L2(stack[j], stack[j]) / 2, rtol=1e-12)
        assert abs(x0 - oracle.inner_L2(stack[j], stack[0])) <= 1e-12 * np.sqrt(
            oracle.inner_L2(stack[j], stack[j]) * oracle.inner_L2(stack[0], stack[0]))
    assert d["members"][0][1] == d["enstrophy"]


# ----------------------------------------------------------------------------- 5. member access
def test_member_access(qfa, oracle):
    N = 64
    dt = 0.25 * qfa.hbar(N)
    state = mhd_state(oracle, N)
    tr = qfa.DeviceMHDTrajectory(state)
    try:
        for j in range(2):
            t1 = qfa.DeviceTrajectory(tr.download()[j])
            try:
                assert np.array_equal(tr.shr(j), t1.shr())
                assert np.array_equal(tr.shr(j, 100), t1.shr(100))
                assert np.array_equal(tr.fun(j), t1.fun())
                assert np.array_equal(tr.spectrum(j), t1.spectrum())
            finally:
                close(t1)
        assert np.array_equal(tr.download(), state)           # looking at a member changes nothing
        xi = np.array([0.3, -0.2, 0.5])
        rotated = np.stack([qfa.rotate(xi, state[j].copy()) for j in range(2)])
        assert tr.rotate(xi) is tr
        assert np.array_equal(tr.download(), rotated)
        tr.advance(dt, 2)
        assert np.array_equal(tr.download(), qfa.magmp(rotated.copy(), dt, 2))
    finally:
        close(tr)


def test_member_spectrum_odd(qfa, oracle):
    N = 257
    state = mhd_state(oracle, N)
    tr = qfa.DeviceMHDTrajectory(state)
    try:
        lam = tr.spectrum(1)
    finally:
        close(tr)
    t1 = qfa.DeviceTrajectory(state[1])
    try:
        assert np.array_equal(lam, t1.spectrum())
    finally:
        close(t1)


# ----------------------------------------------------------------------------- 6. solve
def _run_solve(qfa, W, dt, resident, **kw):
    chunks, stats = [], []

    def cb(W, delta_time=None, delta_steps=None, **st):
        chunks.append(W.copy())
        stats.append(dict(st))

    out = qfa.solve(W, dt=dt, steps=6, steps_out=2, callback=cb, progress_bar=False, resident=resident, **kw)
    return out, chunks, stats


@pytest.mark.parametrize("kind", ["mhd", "stack"])
def test_solve_keeps_the_stack_resident(qfa, oracle, monkeypatch, kind):
    N = 64
    dt = 0.25 * qfa.hbar(N)
    if kind == "mhd":
        W0, kw = mhd_state(oracle, N), dict(integrator=qfa.magmp, hamiltonian=qfa.solve_mhd)
    else:
        W0, kw = tracer_stack(oracle, N), dict(integrator=qfa.isomp)
    ref, ref_chunks, ref_stats = _run_solve(qfa, W0.copy(), dt, False, **kw)

    def boom(*a, **k):
        raise AssertionError("the host-in / host-out stack stepper was called")

    monkeypatch.setattr(qfa.integrators, "_isomp_states", boom)
    mine = W0.copy()
    out, chunks, stats = _run_solve(qfa, mine, dt, None, **kw)
    assert len(chunks) == len(ref_chunks) == 3
    for a, b in zip(chunks, ref_chunks):
        assert np.array_equal(a, b)
    assert np.array_equal(out, ref) and np.array_equal(mine, ref)      # the caller's array is advanced in place
    assert stats == ref_stats
    assert set(stats[-1]) == ({"tol", "iterations", "maxit"} if kind == "mhd" else {"tol_auto", "iterations", "number_of_maxit"})


# ----------------------------------------------------------------------------- 7. errors
def test_errors(qfa, oracle):
    from quflow_amd import _lib
    from quflow_amd.context import Context, get_context, ptr
    N = 16
    dt = 0.25 * qfa.hbar(N)
    state = mhd_state(oracle, N)
    lib = _lib.load()
    st = _lib.IsompStats()
    d = (ctypes.c_double * 5)()
    ctx = Context(N, 0)
    try:
        adv = lambda magnetic: lib.qf_states_advance(ctx.handle, dt, 1, -1.0, 1, 10, 0, magnetic, ctypes.byref(st))
        assert adv(1) == 4                                               # QF_ERR_STATE: nothing resident yet
        assert lib.qf_mhd_diagnostics(ctx.handle, d) == 4
        assert lib.qf_states_select(ctx.handle, 0) == 4
        three = np.ascontiguousarray(tracer_stack(oracle, N))
        assert lib.qf_states_upload(ctx.handle, ptr(three), 3) == 0
        assert adv(1) == 1                                               # QF_ERR_INVALID: magnetic with k = 3
        assert lib.qf_mhd_diagnostics(ctx.handle, d) == 1
        assert lib.qf_states_select(ctx.handle, 5) == 1
        assert lib.qf_states_store(ctx.handle, -1) == 1
        back = np.zeros((2, N, N), dtype=complex)
        assert lib.qf_states_download(ctx.handle, ptr(back), 2) == 1     # k mismatch
        assert adv(0) == 0
    finally:
        ctx.close()
    # a host-in / host-out call on the same context discards the resident stack
    shared = get_context(N)
    qfa.physics.mhd_diagnostics(state)
    assert lib.qf_mhd_diagnostics(shared.handle, d) == 0
    qfa.magmp(state.copy(), dt, 1)
    assert lib.qf_mhd_diagnostics(shared.handle, d) == 4
    # a NaN in Theta's data is reported as the host path reports it, and an upload recovers the trajectory
    bad = state.copy()
    bad[1, 3, 4] = np.nan
    bad[1, 4, 3] = np.nan
    with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
        qfa.magmp(bad.copy(), dt, 1)
    tr = qfa.DeviceMHDTrajectory(bad)
    try:
        with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
            tr.advance(dt, 1)
        tr.upload(state)
        tr.advance(dt, STEPS)
        assert np.array_equal(tr.download(), qfa.magmp(state.copy(), dt, STEPS))
    finally:
        tr.ctx.close()
