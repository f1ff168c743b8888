"""Host-side checks of the device-resident affine forcing (qf_set_forcing, k_forcing_affine, quflow_amd.AffineForcing, the forced
DeviceTrajectory): what can be said without a GPU -- the constructor's argument rules, check_size, what simulation._resident_kind
makes of a forced run, what the code generator made of the new kernel, and the ctypes prototypes of the new entry points."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("qf_set_forcing", "qf_clear_forcing", "qf_forcing", "qf_isomp_forced")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from quflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    return quflow_amd


def skew(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return A - A.conj().T


# ----------------------------------------------------------------------------- the constructor
def test_constructor_keeps_what_it_is_given(qfa):
    F0 = skew(8, 0)
    f = qfa.AffineForcing(F0, a_W=-0.01, a_P=0.5, a_lap=1e-4)
    assert f.N == 8 and (f.a_W, f.a_P, f.a_lap) == (-0.01, 0.5, 1e-4)
    np.testing.assert_array_equal(f.F0, F0)
    assert f.F0 is not F0 and not f.F0.flags.writeable          # a copy of its own: the caller's array may change
    assert f.F0.dtype == np.complex128 and f.F0.flags.c_contiguous and f.F0_key != 0
    g = qfa.AffineForcing()
    assert g.F0 is None and g.N is None and (g.a_W, g.a_P, g.a_lap) == (0.0, 0.0, 0.0) and g.F0_key == 0
    assert all(isinstance(a, float) for a in (qfa.AffineForcing(a_W=1, a_P=np.float32(2), a_lap=np.int64(3)).a_W,))
    assert callable(f)


def test_constructor_rejects_a_pattern_that_is_not_skew_hermitian(qfa):
    F0 = skew(6, 1)
    # one entry off by the smallest amount that changes a bit pattern
    F0[1, 2] = np.nextafter(F0[1, 2].real, np.inf) + 1j * F0[1, 2].imag
    with pytest.raises(ValueError, match="skew-Hermitian"):
        qfa.AffineForcing(F0)
    H = skew(6, 2)
    with pytest.raises(ValueError, match="skew-Hermitian"):
        qfa.AffineForcing(1j * H)          # Hermitian
    with pytest.raises(ValueError, match="skew-Hermitian"):
        qfa.AffineForcing(np.ones((4, 4)))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_constructor_rejects_a_pattern_that_is_not_finite(qfa, bad):
    F0 = skew(5, 3)
    F0[0, 3] = bad * 1j
    F0[3, 0] = bad * 1j           # (skew-Hermitian as far as inf goes: the finite check must speak first)
    with pytest.raises(ValueError, match="finite"):
        qfa.AffineForcing(F0)
    F0 = skew(5, 3)
    F0[2, 2] = complex(0.0, bad)
    with pytest.raises(ValueError, match="finite"):
        qfa.AffineForcing(F0)


@pytest.mark.parametrize("shape", [(4,), (4, 5), (2, 4, 4), (1, 1), ()])
def test_constructor_rejects_a_wrong_shape(qfa, shape):
    with pytest.raises(ValueError, match="shape"):
        qfa.AffineForcing(np.zeros(shape, dtype=np.complex128))


@pytest.mark.parametrize("name", ["a_W", "a_P", "a_lap"])
def test_constructor_rejects_complex_and_non_finite_coefficients(qfa, name):
    for bad in (1j, np.complex128(2.0), complex(1.0, 0.0)):
        with pytest.raises(TypeError, match=name):
            qfa.AffineForcing(**{name: bad})
    for bad in ("1.0", None, [1.0], np.ones(2)):
        with pytest.raises(TypeError, match=name):
            qfa.AffineForcing(**{name: bad})
    for bad in (np.nan, np.inf, -np.inf, float("nan")):
        with pytest.raises(ValueError, match=name):
            qfa.AffineForcing(**{name: bad})


def test_check_size(qfa):
    f = qfa.AffineForcing(skew(8, 4), a_W=-1.0)
    f.check_size(8)
    f.check_size(np.int64(8))
    with pytest.raises(ValueError, match="N=8"):
        f.check_size(9)
    # without a pattern the forcing has no size of its own: it goes with any state
    g = qfa.AffineForcing(a_W=-1.0, a_lap=1e-3)
    for N in (2, 33, 1024):
        g.check_size(N)


# ----------------------------------------------------------------------------- what solve keeps on the device
def test_resident_kind_of_forced_runs(qfa):
    from quflow_amd import simulation
    kind = simulation._resident_kind
    N = 8
    W = skew(N, 5)
    f = qfa.AffineForcing(skew(N, 6), a_W=-0.01, a_lap=1e-4)
    v = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
    H = qfa.TridiagonalHamiltonian(np.ones((N, N, 2)), offset=qfa.coriolis(N, 1.0))      # (any table: nothing is solved here)
    base = {"hamiltonian": qfa.solve_poisson, "time": 0.0, "stats": {}}
    for isomp in (qfa.isomp, qfa.isomp_fixedpoint):
        assert kind(isomp, dict(base, forcing=f), W) == 'single'
        assert kind(isomp, dict(base, strang_splitting=v), W) == 'single'
        assert kind(isomp, dict(base, forcing=f, strang_splitting=v), W) == 'single'
        assert kind(isomp, dict(base, forcing=f, strang_splitting=v, hamiltonian=H), W) == 'single'
        assert kind(isomp, dict(base, forcing=None, strang_splitting=None), W) == 'single'
        # host hooks, and what the resident forced loop does not have
        assert kind(isomp, dict(base, forcing=lambda P, W: 0 * W), W) is None
        assert kind(isomp, dict(base, forcing=f, strang_splitting=lambda h, W: W), W) is None
        assert kind(isomp, dict(base, forcing=f, compsum=True), W) is None
        assert kind(isomp, dict(base, strang_splitting=v, compsum=True), W) is None
        assert kind(isomp, dict(base, forcing=f, callback=lambda W, dW: None), W) is None
        assert kind(isomp, dict(base, forcing=f, hamiltonian=lambda W: W), W) is None
        # a stack and complex64 data keep the host route: the instance is then a plain callable
        assert kind(isomp, dict(base, forcing=f), np.stack([W, W])) is None
        assert kind(isomp, dict(base, strang_splitting=v), np.stack([W, W])) is None
        assert kind(isomp, dict(base, forcing=f), W.astype(np.complex64)) is None
        assert kind(isomp, dict(base, strang_splitting=v), W.astype(np.complex64)) is None
    assert kind(qfa.rk4, dict(base, forcing=f), W) is None
    # unforced runs are what they were
    assert kind(qfa.isomp, dict(base), W) == 'single'
    assert kind(qfa.isomp, dict(base), W.astype(np.complex64)) == 'single'
    assert kind(qfa.isomp, dict(base, compsum=True), W) == 'single'


def test_resident_kind_follows_select_skewherm(qfa):
    from quflow_amd import simulation
    N = 8
    W = skew(N, 7)
    f = qfa.AffineForcing(a_W=-0.01)
    ikw = {"hamiltonian": qfa.solve_poisson, "forcing": f}
    try:
        qfa.integrators.select_skewherm(False)
        assert simulation._resident_kind(qfa.isomp, ikw, W) is None
    finally:
        qfa.integrators.select_skewherm(True)
    assert simulation._resident_kind(qfa.isomp, ikw, W) == 'single'


def test_device_trajectory_refuses_what_it_cannot_carry_before_it_touches_a_device(qfa):
    W = skew(8, 8)
    with pytest.raises(TypeError, match="AffineForcing"):
        qfa.DeviceTrajectory(W, forcing=lambda P, W: W)
    with pytest.raises(TypeError, match="ViscDampStep"):
        qfa.DeviceTrajectory(W, strang_splitting=lambda h, W: W)
    with pytest.raises(ValueError, match="N=6"):
        qfa.DeviceTrajectory(W, forcing=qfa.AffineForcing(skew(6, 9)))
    if qfa.laplacian.single_precision_on_device():
        with pytest.raises(NotImplementedError, match="complex128"):
            qfa.DeviceTrajectory(W.astype(np.complex64), forcing=qfa.AffineForcing(a_W=-1.0))
        with pytest.raises(NotImplementedError, match="complex128"):
            qfa.DeviceTrajectory(W.astype(np.complex64), strang_splitting=qfa.ViscDampStep())


# ----------------------------------------------------------------------------- the build's records and the ABI
def test_forcing_kernel_in_the_build_records(built):
    """One instantiation per set of terms (F0, a_W, a_P, a_lap present or not: decided per launch), none with scratch or a
    dynamic stack, all in hooks.res."""
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    names = sorted(k for k in res if k.startswith("k_forcing_affine"))
    assert names == sorted("k_forcing_affine<%d>" % t for t in range(16)), names
    for name in names:
        assert res[name]["unit"] == "hooks.res", (name, res[name])
        assert res[name]["scratch"] == 0 and not res[name]["dynamic_stack"] and res[name]["lds"] == 0, (name, res[name])
        assert res[name]["occupancy"] >= 8, (name, res[name])          # a streaming pass: nothing may cap the waves in flight


def test_new_symbols_resolve_with_their_signatures(built):
    import ctypes
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in built.SIGNATURES, name
        fn = getattr(lib, name)
        res, args = built.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert re.search(r"\bint %s\(qf_ctx \*ctx" % name, header), name
    assert built.SIGNATURES["qf_set_forcing"][1][2:] == [ctypes.c_ulonglong, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    assert len(built.SIGNATURES["qf_forcing"][1]) == 4
    assert len(built.SIGNATURES["qf_isomp_forced"][1]) == 10
    # a null context is refused, not dereferenced
    assert lib.qf_clear_forcing(None) == 1
    assert lib.qf_set_forcing(None, None, 0, 0.0, 0.0, 0.0) == 1
    assert lib.qf_forcing(None, None, None, None) == 1
    assert lib.qf_isomp_forced(None, 0.1, 1, -1.0, 1, 10, 0, None, 0, None) == 1


def test_header_lists_who_follows_and_who_refuses():
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    block = header[header.index("the forcing of the flow"):header.index("int qf_set_forcing(")]
    for name in ("qf_isomp_forced", "qf_isomp_hooked", "qf_erk_hooked", "qf_isomp_states", "qf_states_advance", "qf_erk_states",
                 "qf_isomp_simple", "qf_c64_isomp", "Compensated sum with forcing is not yet implemented."):
        assert name in block, name
