"""GPU tests of the device-resident affine forcing F(P, W) = F0 + a_W W + a_P P + a_lap Delta W: k_forcing_affine alone
(qf_forcing / AffineForcing.__call__), the steppers that install an AffineForcing for a call (isomp, euler / heun / rk4), the
forced resident DeviceTrajectory (qf_isomp_forced), solve, and the entry points that refuse an installed forcing.

Everything here is an EQUALITY: the reference is a numpy callable, defined below, that repeats the order of operations the
AffineForcing docstring fixes, on `.real` / `.imag` float64 arrays with Delta W from quflow_amd.laplace; given as `forcing=`
it takes the host-hook route (qf_isomp_hooked / qf_erk_hooked with a forcing hook), which tests/test_hip_parity.py pins to
the reference's fixtures (tests/golden/hooks.npz).  States must be np.array_equal, `iterations` / `number_of_maxit` ==.

Data: random skew-Hermitian matrices from a seeded default_rng, states scaled to |W|_F = sqrt(N); dt = 0.25 hbar(N)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def coefficients(N):
    """All four terms at sizes of a forced-dissipative run: a pattern a tenth of the state, friction, a drag on the stream
    function, and a viscosity whose largest eigenvalue (~ N^2) stays 0.1."""
    return dict(F0=skew(N, 100, 0.1), a_W=-0.02, a_P=0.05, a_lap=0.1 / (N * N))


# ----------------------------------------------------------------------------- the numpy mirror
def mirror(qfa, F0=None, a_W=0.0, a_P=0.0, a_lap=0.0):
    """The forcing as a host callable, operation by operation in the order the AffineForcing docstring fixes (the loop has
    scaled P before the call and scales F behind it: pscale and s are the host route's own)."""
    def forcing(P, W):
        if W.ndim == 3:
            return np.stack([forcing(P, w) for w in W])
        if F0 is None:
            fr, fi = np.zeros(W.shape), np.zeros(W.shape)
        else:
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
    return forcing


def no_host_class(qfa):
    """An AffineForcing whose host protocol raises: a run with it succeeds only if the device never came back for the force."""
    class NoHost(qfa.AffineForcing):
        def __call__(self, P, W):
            raise AssertionError("the installed forcing was evaluated on the host")
    return NoHost


def forcing_class(qfa, which):
    return qfa.AffineForcing if which == "plain" else no_host_class(qfa)


# ----------------------------------------------------------------------------- 1. the kernel alone
TERMS = {
    "F0": lambda N: dict(F0=skew(N, 100, 0.1)),
    "a_W": lambda N: dict(a_W=-0.02),
    "a_P": lambda N: dict(a_P=0.05),
    "a_lap": lambda N: dict(a_lap=0.1 / (N * N)),
    "all": coefficients,
    "no_F0": lambda N: dict(a_W=-0.02, a_P=0.05, a_lap=0.1 / (N * N)),
}


@pytest.mark.parametrize("N", [2, 3, 31, 32, 33, 65, 257])
def test_kernel_alone_equals_the_mirror(qfa, N):
    """N = 2, 3: the degenerate sizes; 31 .. 33, 65: both sides of a 32-wide tile and of a 64-lane row; 257: a partial last
    block of 256 lanes.  Every term alone, all four, and the three linear ones without a pattern."""
    P, W = skew(N, 1), skew(N, 2)
    for name, make in TERMS.items():
        kw = make(N)
        got = qfa.AffineForcing(**kw)(P, W)
        want = mirror(qfa, **kw)(P, W)
        assert got.dtype == np.complex128 and got.shape == (N, N)
        assert np.array_equal(got, want), (N, name, float(np.abs(got - want).max()))
        assert np.any(got != 0), (N, name)
    # nothing but zero coefficients: the zero matrix
    assert not np.any(qfa.AffineForcing()(P, W))
    # a stack: member by member with the shared P
    kw = coefficients(N)
    S = np.stack([W, skew(N, 3)])
    assert np.array_equal(qfa.AffineForcing(**kw)(P, S), mirror(qfa, **kw)(P, S))


def test_forcing_key_and_fingerprint(qfa):
    """A repeated key with another pattern (same shape, one entry pair changed) is uploaded again: the result follows."""
    from quflow_amd.context import Context, ptr
    from quflow_amd import _lib
    N = 33
    P, W = np.array(skew(N, 1)), np.array(skew(N, 2))        # (held here: the library reads them through bare pointers)
    F0 = np.array(skew(N, 100, 0.1))
    ctx = Context(N)
    try:
        out = np.empty((N, N), dtype=np.complex128)
        for trial in range(3):
            if trial == 2:
                F0 = F0.copy()
                F0[0, 1] += 1.0
                F0[1, 0] -= 1.0
            _lib.check(ctx._lib.qf_set_forcing(ctx.handle, ptr(F0), ctypes.c_ulonglong(77), 0.0, 0.0, 0.0))
            _lib.check(ctx._lib.qf_forcing(ctx.handle, ptr(P), ptr(W), ptr(out)))
            assert np.array_equal(out, F0), trial
        _lib.check(ctx._lib.qf_clear_forcing(ctx.handle))
        with pytest.raises(_lib.QuflowHipError, match="no forcing is installed"):
            _lib.check(ctx._lib.qf_forcing(ctx.handle, ptr(P), ptr(W), ptr(out)))
    finally:
        ctx.close()


# ----------------------------------------------------------------------------- 2. isomp: installed == host hook
def run_isomp(qfa, W0, dt, steps, forcing, **kw):
    stats = {"iterations": 0.0}
    W = qfa.isomp(np.array(W0), dt, steps=steps, forcing=forcing, stats=stats, **kw)
    return W, stats


def isomp_reference(qfa, N, steps, variant):
    """The host-hook run of a variant, made once: (state, stats)."""
    def make():
        kw = coefficients(N)
        W, stats = run_isomp(qfa, skew(N, 0), 0.25 * qfa.hbar(N), steps, mirror(qfa, **kw), **variant_kwargs(qfa, N, variant))
        return (W, dict(stats))
    return _cached(("isomp_ref", N, steps, variant), make)


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


def check_isomp(qfa, N, steps, variant, which):
    f = forcing_class(qfa, which)(**coefficients(N))
    W, stats = run_isomp(qfa, skew(N, 0), 0.25 * qfa.hbar(N), steps, f, **variant_kwargs(qfa, N, variant))
    Wr, sr = isomp_reference(qfa, N, steps, variant)
    print("isomp N=%d %s: iterations %r / %r, max|diff| %.3e" % (N, variant, stats["iterations"], sr["iterations"],
                                                                   float(np.abs(W - Wr).max())))
    assert np.array_equal(W, Wr)
    assert stats["iterations"] == sr["iterations"] and stats["number_of_maxit"] == sr["number_of_maxit"]
    assert stats["tol_auto"] == sr["tol_auto"]
    assert stats["iterations"] >= 2.0                 # the fixed-point loop really iterated
    assert not np.array_equal(W, skew(N, 0))
    # the context is left without a forcing: the next default call on it is the unforced one
    from quflow_amd.context import get_stepper_context
    from quflow_amd import _lib
    ctx = get_stepper_context(N)
    out = np.empty((N, N), dtype=np.complex128)
    assert ctx._lib.qf_forcing(ctx.handle, out.ctypes.data, out.ctypes.data, out.ctypes.data) == 4       # QF_ERR_STATE


@pytest.mark.parametrize("N,variant", [(33, "plain"), (64, "plain"), (33, "strang"), (33, "coriolis"), (33, "reinitialize"),
                                       (33, "minit")])
def test_isomp_installed_equals_host_hook(qfa, N, variant):
    check_isomp(qfa, N, 5, variant, "plain")


def test_forced_run_differs_from_the_unforced_one(qfa):
    """(the equality above is not vacuous: the force moves the state)"""
    N = 33
    W, _ = run_isomp(qfa, skew(N, 0), 0.25 * qfa.hbar(N), 5, qfa.AffineForcing(**coefficients(N)))
    U, _ = run_isomp(qfa, skew(N, 0), 0.25 * qfa.hbar(N), 5, None)
    assert float(np.abs(W - U).max()) > 1e-6


# ----------------------------------------------------------------------------- 3. the explicit steppers
@pytest.mark.parametrize("method", ["euler", "heun", "rk4"])
@pytest.mark.parametrize("which", ["plain", "no_host"])
def test_erk_installed_equals_host_hook(qfa, method, which):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    kw = coefficients(N)
    stepper = getattr(qfa, method)
    Wr = _cached(("erk_ref", method), lambda: stepper(np.array(skew(N, 0)), dt, steps=3, forcing=mirror(qfa, **kw)))
    W = stepper(np.array(skew(N, 0)), dt, steps=3, forcing=forcing_class(qfa, which)(**kw))
    print("%s N=%d: max|diff| %.3e" % (method, N, float(np.abs(W - Wr).max())))
    assert np.array_equal(W, Wr)
    U = stepper(np.array(skew(N, 0)), dt, steps=3)
    assert float(np.abs(W - U).max()) > 1e-6


# ----------------------------------------------------------------------------- 4. the pipelined 64 x 64 product class
def test_isomp_installed_equals_host_hook_n1024(qfa):
    check_isomp(qfa, 1024, 2, "plain", "no_host")


# ----------------------------------------------------------------------------- 5. the resident trajectory
def trajectory_reference(qfa, N, case):
    """Two successive host-in isomp calls of 3 steps: [(state, stats), (state, stats)]."""
    def make():
        dt = 0.25 * qfa.hbar(N)
        kw = coefficients(N)
        kw2 = dict(kw, F0=skew(N, 101, 0.1))
        v = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
        fs = {"forced": (mirror(qfa, **kw), mirror(qfa, **kw)), "switch": (mirror(qfa, **kw), mirror(qfa, **kw2)),
              "strang_only": (None, None)}[case]
        W = np.array(skew(N, 0))
        out = []
        for f in fs:
            W, stats = run_isomp(qfa, W, dt, 3, f, strang_splitting=v)
            out.append((W.copy(), dict(stats)))
        return out
    return _cached(("traj_ref", N, case), make)


def check_trajectory(qfa, N, case, which):
    dt = 0.25 * qfa.hbar(N)
    cls = forcing_class(qfa, which)
    kw = coefficients(N)
    f1 = None if case == "strang_only" else cls(**kw)
    f2 = cls(**dict(kw, F0=skew(N, 101, 0.1))) if case == "switch" else f1
    v = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
    ref = trajectory_reference(qfa, N, case)
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=f1, strang_splitting=v)
    try:
        for chunk, f in enumerate((f1, f2)):
            if chunk == 1 and case == "switch":
                tr.set_forcing(f)
            st = tr.advance(dt, 3)
            W = tr.download()
            Wr, sr = ref[chunk]
            print("trajectory N=%d %s chunk %d: iterations %r / %r, max|diff| %.3e"
                  % (N, case, chunk, st["iterations"], sr["iterations"], float(np.abs(W - Wr).max())))
            assert st["iterations"] == sr["iterations"] and st["number_of_maxit"] == sr["number_of_maxit"], (chunk, st, sr)
            if case != "strang_only":      # (isomp with a Strang step alone forms its tolerance on the host)
                assert st["tol"] == sr["tol_auto"]
            assert np.array_equal(W, Wr), chunk
        # diagnostics=True: a diagnostics() call behind the advance
        st = tr.advance(dt, 1, diagnostics=True)
        assert (st["energy"], st["enstrophy"]) == tr.diagnostics()
    finally:
        tr.ctx.close()


@pytest.mark.parametrize("N", [33, 64])
@pytest.mark.parametrize("case", ["forced", "switch", "strang_only"])
def test_resident_trajectory_equals_host_in_calls(qfa, N, case):
    check_trajectory(qfa, N, case, "plain")


# ----------------------------------------------------------------------------- 6. solve
def test_solve_resident_equals_host_in(qfa):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    f = no_host_class(qfa)(**coefficients(N))
    v = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
    seen = {}
    for resident in (True, False):
        states = []
        W = qfa.solve(np.array(skew(N, 0)), dt, steps=6, steps_out=3, integrator=qfa.isomp, forcing=f, strang_splitting=v,
                      resident=resident, progress_bar=False,
                      callback=lambda W, **kw: states.append((np.array(W), kw.get("iterations"), kw.get("number_of_maxit"))))
        assert len(states) == 2 and np.array_equal(states[-1][0], W)
        seen[resident] = states
    for (Wa, ia, ma), (Wb, ib, mb) in zip(seen[True], seen[False]):
        assert np.array_equal(Wa, Wb)
        assert ia == ib and ma == mb
    assert np.array_equal(seen[True][0][0], trajectory_reference(qfa, N, "forced")[0][0])
    # the default is the resident route
    from quflow_amd import simulation
    assert simulation._resident_kind(qfa.isomp, {"forcing": f, "strang_splitting": v}, skew(N, 0)) == 'single'


# ----------------------------------------------------------------------------- 7. the installed route never calls the host
@pytest.mark.parametrize("N,variant", [(33, "plain"), (64, "plain"), (33, "strang"), (33, "coriolis"), (33, "reinitialize"),
                                       (33, "minit")])
def test_isomp_installed_never_calls_the_host(qfa, N, variant):
    check_isomp(qfa, N, 5, variant, "no_host")


@pytest.mark.parametrize("N", [33, 64])
@pytest.mark.parametrize("case", ["forced", "switch"])
def test_resident_trajectory_never_calls_the_host(qfa, N, case):
    check_trajectory(qfa, N, case, "no_host")


# ----------------------------------------------------------------------------- 8. refusals
def test_entry_points_that_cannot_apply_the_force_refuse(qfa):
    from quflow_amd.context import Context, ptr
    from quflow_amd import _lib
    N = 33
    dt = 0.25 * qfa.hbar(N)
    W0 = np.array(skew(N, 0))
    ctx, fresh = Context(N), Context(N)
    try:
        lib = ctx._lib
        st = _lib.IsompStats()
        qfa.AffineForcing(**coefficients(N)).install(ctx)
        _lib.check(lib.qf_upload_W(ctx.handle, ptr(W0)))
        stack = np.stack([W0, np.array(skew(N, 5))])
        _lib.check(lib.qf_states_upload(ctx.handle, ptr(stack), 2))
        calls = {
            "qf_isomp": lambda: lib.qf_isomp(ctx.handle, dt, 2, -1.0, 1, 10, 0, 0, ctypes.byref(st)),
            "qf_erk": lambda: lib.qf_erk(ctx.handle, _lib.ERK_METHODS["rk4"], dt, 1, 1),
            "qf_isomp_simple": lambda: lib.qf_isomp_simple(ctx.handle, dt, 1),
            "qf_states_advance": lambda: lib.qf_states_advance(ctx.handle, dt, 1, -1.0, 1, 10, 0, 0, ctypes.byref(st)),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.QuflowHipError, match="QF_ERR_UNSUPPORTED.*%s.*forcing" % name):
                _lib.check(call())
        # nothing was advanced
        got = np.empty_like(W0)
        _lib.check(lib.qf_download_W(ctx.handle, ptr(got)))
        assert np.array_equal(got, W0)
        # cleared: the same call is a fresh context's
        _lib.check(lib.qf_clear_forcing(ctx.handle))
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


def test_compsum_and_complex64_are_not_implemented(qfa):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    f = qfa.AffineForcing(**coefficients(N))
    W = np.array(skew(N, 0))
    with pytest.raises(NotImplementedError, match="Compensated sum with forcing is not yet implemented."):
        qfa.isomp(W, dt, steps=2, forcing=f, compsum=True)
    assert np.array_equal(W, skew(N, 0))
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=f)
    try:
        with pytest.raises(NotImplementedError, match="Compensated sum with forcing is not yet implemented."):
            tr.advance(dt, 2, compsum=True)
        with pytest.raises(NotImplementedError, match="forcing"):
            tr.advance_erk("rk4", dt, 1)
        with pytest.raises(NotImplementedError, match="forcing"):
            tr.advance_lu("isomp_simple", dt, 1)
        assert np.array_equal(tr.download(), skew(N, 0))
    finally:
        tr.ctx.close()
    if qfa.laplacian.single_precision_on_device():
        with pytest.raises(NotImplementedError):
            qfa.DeviceTrajectory(skew(N, 0).astype(np.complex64), forcing=f)
        with pytest.raises(NotImplementedError):
            qfa.DeviceTrajectory(skew(N, 0).astype(np.complex64), strang_splitting=qfa.ViscDampStep())


# ----------------------------------------------------------------------------- 9. a stack keeps the host route
def test_stack_keeps_the_host_route(qfa):
    N = 33
    dt = 0.25 * qfa.hbar(N)
    kw = coefficients(N)
    S0 = np.stack([skew(N, 0), skew(N, 5)])
    calls = []

    class Counting(qfa.AffineForcing):
        def __call__(self, P, W):
            calls.append(np.shape(W))
            return super().__call__(P, W)

    sa, sb = {"iterations": 0.0}, {"iterations": 0.0}
    A = qfa.isomp(S0.copy(), dt, steps=2, forcing=Counting(**kw), stats=sa)
    B = qfa.isomp(S0.copy(), dt, steps=2, forcing=mirror(qfa, **kw), stats=sb)
    assert np.array_equal(A, B)
    assert sa["iterations"] == sb["iterations"] and sa["number_of_maxit"] == sb["number_of_maxit"]
    assert (2, N, N) in calls            # called as any callable is: with the whole stack (which it takes member by member)
