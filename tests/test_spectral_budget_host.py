"""Host-side checks of the spectral budget (qf_spectral_budget, qf_degree_spectrum, quflow_amd.analysis.spectral_budget,
DeviceTrajectory.spectral_budget): what can be said without a GPU -- the argument rules, which reach no device; the keys of
the returned dict for every combination of forcing and Strang arguments; the host formulas for the energy forms, the fluxes
and the dissipation on synthetic rows; what the code generator made of the new kernels; the prototypes of the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("qf_spectral_budget", "qf_degree_spectrum")
BASE_KEYS = {"el", "enstrophy", "energy", "enstrophy_transfer", "energy_transfer", "enstrophy_flux", "energy_flux"}
INPUT_KEYS = {"enstrophy_input", "energy_input"}
DISSIPATION_KEYS = {"enstrophy_dissipation", "energy_dissipation"}


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


def synthetic_rows(nmax, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((3, nmax))
    rows[0] = rows[0] ** 2
    return rows


class FakeLib:
    """Stands where libquflow_hip.so would: records the calls, fills the budget's rows (and coefficients) with known numbers."""

    def __init__(self, rows):
        self.rows, self.calls = rows, []

    def qf_set_forcing(self, *a):
        self.calls.append("set_forcing")
        return 0

    def qf_clear_forcing(self, *a):
        self.calls.append("clear_forcing")
        return 0

    def qf_set_hamiltonian(self, *a):
        self.calls.append("set_hamiltonian")
        return 0

    def qf_clear_hamiltonian(self, *a):
        self.calls.append("clear_hamiltonian")
        return 0

    def qf_spectral_budget(self, handle, W, nmax, out, coeffs):
        self.calls.append("budget")
        assert W is not None and nmax == self.rows.shape[1]
        np.ctypeslib.as_array((ctypes.c_double * (3 * nmax)).from_address(out.value))[:] = self.rows.ravel()
        if coeffs is not None:
            np.ctypeslib.as_array((ctypes.c_double * (3 * nmax * nmax)).from_address(coeffs.value))[:] = \
                np.arange(3 * nmax * nmax, dtype=np.float64)
        return 0


class FakeContext:
    def __init__(self, N, rows):
        self.N, self.handle, self._lib = N, object(), FakeLib(rows)


def no_device(monkeypatch):
    """Any attempt to reach a device context from here on fails the test."""
    from quflow_amd import context, quantization

    def refuse(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(context, "Context", refuse)
    monkeypatch.setattr(context, "get_context", refuse)
    monkeypatch.setattr(quantization, "get_context", refuse)
    monkeypatch.setattr(quantization, "_transform_context", refuse)


# ----------------------------------------------------------------------------- argument rules
def test_argument_checks_reach_no_device(qfa, monkeypatch):
    from quflow_amd import integrators
    no_device(monkeypatch)
    N = 8
    W = skew(N, 1)
    budget = qfa.analysis.spectral_budget
    for bad in (1, 0, -2, N + 1, 2.5, True):
        with pytest.raises(ValueError, match="lmax"):
            budget(W, lmax=bad)
    with pytest.raises(NotImplementedError, match="complex64"):
        budget(W.astype(np.complex64))
    with pytest.raises(ValueError, match="square"):
        budget(W[:, :4])
    with pytest.raises(TypeError, match="Hamiltonian"):
        budget(W, hamiltonian=lambda X: X)
    with pytest.raises(TypeError, match="AffineForcing"):
        budget(W, forcing=lambda P, X: X)
    with pytest.raises(TypeError, match="AffineForcing"):
        budget(W, forcing=qfa.StochasticForcing(1, 3, 0.1, seed=1))
    with pytest.raises(TypeError, match="ViscDampStep"):
        budget(W, strang_splitting=lambda h, X: X)
    with pytest.raises(ValueError, match="N=4"):
        budget(W, forcing=qfa.AffineForcing(skew(4, 2)))
    with pytest.raises(ValueError, match="N=4"):
        budget(W, hamiltonian=qfa.TridiagonalHamiltonian(np.ones((4, 4, 2))))
    integrators.select_skewherm(False)
    try:
        with pytest.raises(NotImplementedError, match="skew-Hermitian"):
            budget(W)
    finally:
        integrators.select_skewherm(True)


def test_band_limit_rule(qfa):
    band = qfa.analysis._band_limit
    assert band(8, None) == 8 and band(8, 8) == 8 and band(8, 2) == 2 and band(8, np.int64(5)) == 5
    for bad in (1, 9, 0, -1):
        with pytest.raises(ValueError):
            band(8, bad)


# ----------------------------------------------------------------------------- the dict
@pytest.mark.parametrize("with_strang", [False, True])
@pytest.mark.parametrize("with_forcing", [False, True])
@pytest.mark.parametrize("coefficients", [False, True])
def test_keys_for_every_combination(qfa, monkeypatch, with_forcing, with_strang, coefficients):
    from quflow_amd import quantization
    N, nmax = 8, 6
    rows = synthetic_rows(nmax)
    ctx = FakeContext(N, rows)
    monkeypatch.setattr(quantization, "_transform_context", lambda n, device, streamed: ctx)
    f = qfa.AffineForcing(skew(N, 3), a_W=-0.5) if with_forcing else None
    visc = qfa.ViscDampStep(nu=1e-3, alpha=0.25) if with_strang else None
    b = qfa.analysis.spectral_budget(skew(N, 4), forcing=f, strang_splitting=visc, lmax=nmax, coefficients=coefficients)
    want = set(BASE_KEYS)
    if with_forcing:
        want |= INPUT_KEYS
    if with_strang:
        want |= DISSIPATION_KEYS
    if coefficients:
        want.add("coefficients")
        assert set(b["coefficients"]) == ({"omega", "tendency", "forcing"} if with_forcing else {"omega", "tendency"})
        assert np.array_equal(b["coefficients"]["tendency"], np.arange(nmax * nmax, 2 * nmax * nmax))
    assert set(b) == want
    # the forcing is installed for the call alone, and taken off again
    assert ctx._lib.calls == (["set_forcing", "budget", "clear_forcing"] if with_forcing else ["budget"])
    assert all(b[k].shape == (nmax - 1,) for k in want - {"coefficients"})
    assert np.array_equal(b["enstrophy"], rows[0, 1:])


def test_installed_hamiltonian_is_taken_off_after_an_error(qfa, monkeypatch):
    from quflow_amd import quantization
    N = 8
    ctx = FakeContext(N, synthetic_rows(N))
    ctx._lib.qf_spectral_budget = lambda *a: 3            # QF_ERR_HIP
    ctx._lib.qf_last_error = lambda: b"synthetic"
    monkeypatch.setattr(quantization, "_transform_context", lambda n, device, streamed: ctx)
    monkeypatch.setattr("quflow_amd._lib.load", lambda: ctx._lib)
    ham = qfa.TridiagonalHamiltonian(np.ones((N, N, 2)))
    with pytest.raises(qfa._lib.QuflowHipError, match="synthetic"):
        qfa.analysis.spectral_budget(skew(N, 5), hamiltonian=ham, forcing=qfa.AffineForcing(a_W=-1.0))
    assert ctx._lib.calls == ["set_hamiltonian", "set_forcing", "clear_forcing", "clear_hamiltonian"]


# ----------------------------------------------------------------------------- the host formulas
def test_host_formulas_on_synthetic_rows(qfa):
    nmax = 12
    rows = synthetic_rows(nmax, 7)
    nu, alpha = 3e-4, 0.125
    b = qfa.analysis._budget_dict(rows, True, qfa.ViscDampStep(nu=nu, alpha=alpha))
    el = np.arange(1, nmax)
    assert np.array_equal(b["el"], el) and b["el"].dtype.kind == "i"
    Z, T, I = rows[0, 1:], rows[1, 1:], rows[2, 1:]
    for l in el:
        w = float(l * (l + 1))
        assert b["enstrophy"][l - 1] == Z[l - 1] and b["energy"][l - 1] == Z[l - 1] / w
        assert b["enstrophy_transfer"][l - 1] == T[l - 1] and b["energy_transfer"][l - 1] == T[l - 1] / w
        assert b["enstrophy_input"][l - 1] == I[l - 1] and b["energy_input"][l - 1] == I[l - 1] / w
        assert b["enstrophy_dissipation"][l - 1] == -2 * (nu * w + alpha) * Z[l - 1]
        assert b["energy_dissipation"][l - 1] == (-2 * (nu * w + alpha) * Z[l - 1]) / w
    # the fluxes: minus the running sums, in numpy's cumsum order
    acc_z = acc_e = 0.0
    for l in el:
        acc_z += T[l - 1]
        acc_e += T[l - 1] / float(l * (l + 1))
        assert b["enstrophy_flux"][l - 1] == -acc_z and b["energy_flux"][l - 1] == -acc_e
    # degree 0 is not reported, and the rows are not aliased
    assert all(v.shape == (nmax - 1,) for v in b.values())
    b["enstrophy"][0] = -1.0
    assert rows[0, 1] != -1.0
    assert set(qfa.analysis._budget_dict(rows, False)) == BASE_KEYS


# ----------------------------------------------------------------------------- the build's records and the ABI
def test_budget_kernels_in_the_build_records(built):
    """The multi-vector sweep for two and three vectors over the resident basis and over slabs, and the degree reduction: no
    scratch, no dynamic stack, all in quantization.res; mat2shr's and mat2shc's own kernels keep their names."""
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    multi = sorted(k for k in res if k.startswith("k_block_vecmat_multi"))
    assert multi == sorted("k_block_vecmat_multi<%d, %s>" % (nv, slab) for nv in (2, 3) for slab in ("false", "true")), multi
    old = sorted(k for k in res if k.startswith("k_block_vecmat<") or k.startswith("k_block_matvec<"))
    assert old == sorted("%s<%d, %s>" % (k, mode, slab) for k in ("k_block_vecmat", "k_block_matvec") for mode in (0, 1)
                         for slab in ("false", "true")), old
    for name in multi + ["k_degree_sums"] + [k for k in old if "vecmat" in k]:
        assert res[name]["unit"] == "quantization.res", (name, res[name])
        assert res[name]["scratch"] == 0 and not res[name]["dynamic_stack"], (name, res[name])
    # LDS of the sweep: NV x (256 staged complex + 4 x 2 x 64 partial sums)
    for nv in (2, 3):
        assert res["k_block_vecmat_multi<%d, false>" % nv]["lds"] == nv * (256 * 16 + 4 * 2 * 64 * 8)
    assert res["k_block_vecmat<0, false>"]["lds"] == 256 * 16 + 4 * 2 * 64 * 8
    assert res["k_degree_sums"]["lds"] == 0 and res["k_degree_sums"]["occupancy"] >= 8


def test_new_symbols_resolve_with_their_signatures(built):
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in built.SIGNATURES, name
        fn = getattr(lib, name)
        res, args = built.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert re.search(r"\bint %s\(qf_ctx \*ctx, const void \*W_host, int Nmax" % name, header), name
    assert len(built.SIGNATURES["qf_spectral_budget"][1]) == 5 and len(built.SIGNATURES["qf_degree_spectrum"][1]) == 4
    # a null context is refused, not dereferenced
    assert lib.qf_spectral_budget(None, None, 4, None, None) == 1
    assert lib.qf_degree_spectrum(None, None, 4, None) == 1


def test_trajectories_have_the_budget(qfa):
    for name in ("spectral_budget", "enstrophy_spectrum", "energy_spectrum"):
        assert callable(getattr(qfa.DeviceTrajectory, name))
    assert callable(qfa.DeviceStackTrajectory.spectral_budget)
