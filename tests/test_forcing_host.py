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


# ----------------------------------------------------------------------------- the key identifies the content
# The library reuses the pattern a context holds when F0_key and its own fingerprint both repeat, and the fingerprint reads
# 4096 strided doubles (stride 2 N^2 / 4096: even from N = 64, so real parts only) plus the last one.  The key alone tells two
# patterns apart.  N = 256, 257: the smallest sizes at which a key made of 65536 strided doubles skips entries as well (one a
# multiple of 64, one ragged); 1024: strides 32 and 512.  Each perturbation keeps the matrix exactly skew-Hermitian.
IDENTITY_SIZES = (256, 257, 1024)


def perturb_imag_pair(X):
    X[1, 2] += 0.5j
    X[2, 1] += 0.5j


def perturb_zonal(X):
    X[5, 5] += 0.5j          # (an odd flat index of the interleaved doubles: no even stride visits it)


def perturb_real_pair(X):
    X[1, 2] += 0.5
    X[2, 1] -= 0.5


PERTURBATIONS = {"imag_pair": perturb_imag_pair, "zonal": perturb_zonal, "real_pair": perturb_real_pair}
_BASE = {}


def base_and_perturbed(N, name):
    """(X, X perturbed): seeded, exactly skew-Hermitian, different in one entry or one mirrored pair."""
    if N not in _BASE:
        _BASE[N] = skew(N, 40)
        _BASE[N].setflags(write=False)
    X = _BASE[N]
    G = X.copy()
    PERTURBATIONS[name](G)
    assert np.array_equal(G, -G.conj().T) and int(np.count_nonzero(G != X)) in (1, 2)
    return X, G


@pytest.mark.parametrize("name", sorted(PERTURBATIONS))
@pytest.mark.parametrize("N", IDENTITY_SIZES)
def test_f0_key_tells_patterns_apart(qfa, N, name):
    X, G = base_and_perturbed(N, name)
    fx, fg = qfa.AffineForcing(X), qfa.AffineForcing(G)
    assert fx.F0_key != fg.F0_key, (N, name)
    assert fx.F0_key != 0 and fg.F0_key != 0
    # equal content, built twice (from another array object, and with other coefficients): the same key
    assert qfa.AffineForcing(X.copy(), a_W=-0.5).F0_key == fx.F0_key
    assert qfa.AffineForcing(np.asfortranarray(G)).F0_key == fg.F0_key


def test_f0_key_covers_shape_and_tag(qfa):
    from quflow_amd import laplacian as lap
    a = np.zeros((4, 4), dtype=np.complex128)
    assert lap._content_key("forcing_f0", a) != lap._content_key("ham_offset", a)
    assert lap._content_key("forcing_f0", a) != lap._content_key("forcing_f0", a.reshape(2, 8))
    assert lap._content_key("forcing_f0", a) != lap._content_key("forcing_f0", a.view(np.float64))
    assert all(0 < lap._content_key("t", np.full(3, v)) < 2 ** 64 for v in range(64))


class StubContext:
    """What install() needs of a context, without a device: the size, a handle, and a library whose entry points record
    their arguments and succeed."""

    def __init__(self, N):
        import ctypes
        self.N, self.handle, self.calls = N, ctypes.c_void_p(1), []
        self._lib = self

    def __getattr__(self, name):
        if not name.startswith("qf_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def counted_digest(monkeypatch):
    """quflow_amd.laplacian._content_key with a counter in front: [(tag, shape), ...] of every call."""
    from quflow_amd import laplacian as lap
    seen = []
    real = lap._content_key

    def counting(tag, a):
        seen.append((tag, np.shape(a)))
        return real(tag, a)
    monkeypatch.setattr(lap, "_content_key", counting)
    return seen


def test_key_is_computed_once_and_install_does_not_hash(qfa, monkeypatch):
    N = 256
    X, _ = base_and_perturbed(N, "zonal")
    seen = counted_digest(monkeypatch)
    f = qfa.AffineForcing(X, a_W=-0.01)
    assert seen == [("forcing_f0", (N, N))]
    qfa.AffineForcing(a_W=-0.01)                       # no pattern: nothing to key
    assert len(seen) == 1
    ctx = StubContext(N)
    for _ in range(3):
        f.install(ctx)
        f.uninstall(ctx)
    assert len(seen) == 1, seen
    sets = [args for name, args in ctx.calls if name == "qf_set_forcing"]
    assert len(sets) == 3 and all(a[1].value == f.F0.ctypes.data and a[2].value == f.F0_key for a in sets)
    assert [name for name, _ in ctx.calls].count("qf_clear_forcing") == 3


def test_pattern_stays_write_protected_through_pickle(qfa):
    import pickle
    f = qfa.AffineForcing(skew(8, 0), a_W=-0.01)
    g = pickle.loads(pickle.dumps(f))
    assert np.array_equal(g.F0, f.F0) and g.F0_key == f.F0_key and not g.F0.flags.writeable
    assert pickle.loads(pickle.dumps(qfa.AffineForcing(a_P=1.0))).F0 is None
    # a stored instance is keyed again from its content: one written with a key of sampled entries does not bring it back
    old = qfa.AffineForcing(skew(8, 0))
    old.F0_key = 12345
    assert pickle.loads(pickle.dumps(old)).F0_key == f.F0_key


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
