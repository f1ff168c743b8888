"""Host-side parts of the resident stack that need no GPU: the exported symbols, the constructors' validation (before any
context exists) and the pure helper by which `solve` decides what stays on the device."""
import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import _lib, integrators, simulation

NEW_SYMBOLS = ("qf_states_upload", "qf_states_download", "qf_states_advance", "qf_states_advance_diag", "qf_states_select",
               "qf_states_store", "qf_states_inner", "qf_mhd_diagnostics")


def skew(N, k, seed=0, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((k, N, N)) + 1j * rng.standard_normal((k, N, N))
    return (A - A.conj().transpose(0, 2, 1)).astype(dtype)


def test_new_symbols_resolve():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), "libquflow_hip.so does not export %s" % name


def test_top_level_names():
    for name in ("DeviceStackTrajectory", "DeviceMHDTrajectory", "mhd_diagnostics", "energy_mhd", "cross_helicity",
                 "magnetic_energy"):
        assert hasattr(qfa, name)
    assert issubclass(qfa.DeviceMHDTrajectory, qfa.DeviceStackTrajectory)


def test_constructors_validate_before_any_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was created before the arguments were validated")

    monkeypatch.setattr(integrators, "Context", no_context)
    with pytest.raises(ValueError):
        qfa.DeviceStackTrajectory(skew(8, 1)[0])                          # a 2-D array
    with pytest.raises(ValueError):
        qfa.DeviceMHDTrajectory(skew(8, 1)[0])
    with pytest.raises(ValueError):
        qfa.DeviceStackTrajectory(skew(8, 3), magnetic=True)              # magnetic wants the pair
    with pytest.raises(ValueError):
        qfa.DeviceMHDTrajectory(skew(8, 3))
    with pytest.raises(ValueError):
        qfa.DeviceStackTrajectory(np.zeros((2, 8, 6), dtype=complex))     # members not square
    with pytest.raises(ValueError):
        qfa.DeviceStackTrajectory(np.zeros((2, 8, 8)))                    # not complex128
    with pytest.raises(ValueError):
        qfa.DeviceStackTrajectory(skew(8, 2, dtype=np.complex64))
    # valid arguments get as far as the context
    with pytest.raises(AssertionError, match="a context was created"):
        qfa.DeviceMHDTrajectory(skew(8, 2))


def test_physics_validate_shapes():
    with pytest.raises(ValueError):
        qfa.mhd_diagnostics(skew(8, 3))
    with pytest.raises(ValueError):
        qfa.energy_mhd(skew(8, 1)[0])
    with pytest.raises(ValueError):
        qfa.magnetic_energy(skew(8, 2))


def test_resident_kind():
    kind = simulation._resident_kind
    W2, W3, M = skew(8, 1)[0], skew(8, 3), skew(8, 2)
    base = {"time": 0.0, "stats": {"iterations": 0.0}}
    poisson = dict(base, hamiltonian=qfa.solve_poisson)
    mhd = dict(base, hamiltonian=qfa.solve_mhd)

    assert kind(qfa.isomp, poisson, W2) == 'single'
    assert kind(qfa.isomp, poisson, W2.astype(np.complex64)) == 'single'
    assert kind(qfa.isomp, poisson, W3) == 'stack'
    assert kind(qfa.isomp_fixedpoint, dict(poisson, tol=1e-10, maxit=5, minit=2, reinitialize=True, verbatim=False), W3) == 'stack'
    assert kind(qfa.isomp, poisson, M) == 'stack'                          # a pair under isomp is a stack of two
    for integ in (qfa.magmp, qfa.magmp_fixedpoint):
        assert kind(integ, mhd, M) == 'mhd'
        assert kind(integ, dict(mhd, tol=1e-10, maxit=5, minit=2, reinitialize=True, verbatim=False), M) == 'mhd'

    # what keeps a run on the host path
    assert kind(qfa.magmp, mhd, W3) is None                                # not a pair
    assert kind(qfa.magmp, poisson, M) is None                             # solve's default Hamiltonian is not solve_mhd
    assert kind(qfa.magmp, dict(mhd, hamiltonian=lambda s: qfa.solve_mhd(s)), M) is None
    assert kind(qfa.magmp, dict(mhd, forcing=lambda P, W: W), M) is None
    assert kind(qfa.magmp, dict(mhd, callback=lambda W, dW: None), M) is None
    assert kind(qfa.magmp, dict(mhd, compsum=False), M) is None            # not an argument of magmp
    assert kind(qfa.magmp, mhd, M.astype(np.complex64)) is None
    assert kind(qfa.isomp, dict(poisson, forcing=lambda P, W: W), W3) is None
    assert kind(qfa.isomp, dict(poisson, callback=lambda W, dW: None), W3) is None
    assert kind(qfa.isomp, dict(poisson, strang_splitting=lambda h, W: W), W3) is None
    assert kind(qfa.isomp, dict(poisson, hamiltonian=lambda W: W), W3) is None
    assert kind(qfa.isomp, dict(poisson, compsum=True), W3) is None
    assert kind(qfa.isomp, poisson, W3.astype(np.complex64)) is None
    assert kind(qfa.isomp, dict(poisson, forcing=lambda P, W: W), W2) is None
    assert kind(qfa.rk4, poisson, W3) is None
    assert kind(qfa.isomp, poisson, np.zeros((2, 8, 6), dtype=complex)) is None

    integrators.select_skewherm(False)
    try:
        assert kind(qfa.magmp, mhd, M) is None
        assert kind(qfa.isomp, poisson, W3) is None
        assert kind(qfa.isomp, poisson, W2) is None
    finally:
        integrators.select_skewherm(True)
    assert kind(qfa.magmp, mhd, M) == 'mhd'

    # _device_resident_ok keeps its meaning
    assert simulation._device_resident_ok(qfa.isomp, poisson) is True
    assert simulation._device_resident_ok(qfa.magmp, mhd) is False


class _Resident(Exception):
    """solve built a resident trajectory."""


class _HostPath(Exception):
    """solve called the integrator, which asked for its device context."""


def test_solve_resident_is_one_decision(monkeypatch):
    """`resident=True` means what the default means: a run the trajectory cannot carry takes the host path with the stepper,
    the Hamiltonian and the hooks the caller named; `resident=False` always does.  Only the decision is under test: the
    trajectories and the integrators' contexts are stubs that say which way `solve` went."""
    def resident(*a, **k):
        raise _Resident()

    def host(*a, **k):
        raise _HostPath()

    monkeypatch.setattr(integrators, "DeviceTrajectory", resident)
    monkeypatch.setattr(integrators, "DeviceStackTrajectory", resident)
    monkeypatch.setattr(integrators, "get_context", host)
    monkeypatch.setattr(integrators, "get_stepper_context", host)
    N = 8
    W2, W3, M = skew(N, 1)[0], skew(N, 3), skew(N, 2)

    def rk4_stub(W, dt, steps=100, **kw):      # (rk4 takes no `time`, which solve passes to every stepper: stubbed, as the
        raise _HostPath()                      # test is about the decision and not about that signature)

    monkeypatch.setattr(integrators, "rk4", rk4_stub)
    monkeypatch.setattr(qfa, "rk4", rk4_stub)

    def went(W, **kw):
        with pytest.raises((_Resident, _HostPath)) as info:
            qfa.solve(W.copy(), dt=1e-3, steps=1, progress_bar=False, **kw)
        return info.type

    not_carried = (dict(integrator=qfa.rk4),
                   dict(integrator=qfa.isomp_quasinewton),
                   dict(hamiltonian=lambda W: W),
                   dict(integrator_callback=lambda W, dW: None),
                   dict(forcing=lambda P, W: 0.0 * W))
    for kw in not_carried:
        assert went(W2, resident=True, **kw) is _HostPath, kw
        assert went(W2, **kw) is _HostPath, kw
        assert went(W2, resident=False, **kw) is _HostPath, kw

    carried = ((W2, {}), (W2.astype(np.complex64), {}), (W3, {}),
               (M, dict(integrator=qfa.magmp, hamiltonian=qfa.solve_mhd)))
    for W, kw in carried:
        assert went(W, resident=True, **kw) is _Resident, (W.shape, W.dtype)
        assert went(W, **kw) is _Resident, (W.shape, W.dtype)
        assert went(W, resident=False, **kw) is _HostPath, (W.shape, W.dtype)
