"""Host-side checks of the MHD budget (qf_mhd_spectral_budget, quflow_amd.analysis.mhd_spectral_budget,
DeviceStackTrajectory.mhd_budget): what can be said without a GPU -- the dictionary's arithmetic on made-up rows, the
argument rules, which reach no device, what the code generator made of the new kernels, and the prototype of the new entry."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

KEYS = {"el", "enstrophy", "kinetic_energy", "magnetic_potential", "magnetic_energy", "energy", "cross_helicity",
        "kinetic_transfer_advection", "kinetic_transfer_lorentz", "magnetic_transfer", "energy_transfer",
        "enstrophy_transfer_advection", "enstrophy_source_lorentz", "potential_transfer", "cross_helicity_transfer",
        "kinetic_flux_advection", "energy_flux", "potential_flux", "cross_helicity_flux", "enstrophy_flux_advection"}
FLUXES = {"kinetic_flux_advection": "kinetic_transfer_advection", "energy_flux": "energy_transfer",
          "potential_flux": "potential_transfer", "cross_helicity_flux": "cross_helicity_transfer",
          "enstrophy_flux_advection": "enstrophy_transfer_advection"}
COEFFICIENTS = ("omega", "theta", "advection", "lorentz", "induction")


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
    rows = rng.standard_normal((9, nmax))
    rows[:2] = rows[:2] ** 2
    return rows


def no_device(monkeypatch):
    """Any attempt to reach a device context from here on fails the test."""
    from quflow_amd import context, quantization

    def refuse(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(context, "Context", refuse)
    monkeypatch.setattr(context, "get_context", refuse)
    monkeypatch.setattr(quantization, "get_context", refuse)
    monkeypatch.setattr(quantization, "_transform_context", refuse)


class FakeLib:
    """Stands where libquflow_hip.so would: records the calls, fills the rows (and coefficients) with known numbers."""

    def __init__(self, rows):
        self.rows, self.calls = rows, []

    def qf_states_upload(self, handle, states, k):
        self.calls.append(("upload", k))
        return 0

    def qf_mhd_spectral_budget(self, handle, nmax, out, coeffs):
        self.calls.append(("budget", nmax))
        assert nmax == self.rows.shape[1]
        np.ctypeslib.as_array((ctypes.c_double * (9 * nmax)).from_address(out.value))[:] = self.rows.ravel()
        if coeffs is not None:
            np.ctypeslib.as_array((ctypes.c_double * (5 * nmax * nmax)).from_address(coeffs.value))[:] = \
                np.arange(5 * nmax * nmax, dtype=np.float64)
        return 0


class FakeContext:
    def __init__(self, N, rows):
        self.N, self.handle, self._lib = N, object(), FakeLib(rows)


# ----------------------------------------------------------------------------- the dictionary
def test_dictionary_arithmetic_on_synthetic_rows(qfa):
    nmax = 12
    rows = synthetic_rows(nmax, 7)
    b = qfa.analysis._mhd_budget_dict(rows)
    assert set(b) == KEYS
    el = np.arange(1, nmax)
    assert np.array_equal(b["el"], el) and b["el"].dtype.kind == "i"
    r = rows[:, 1:]
    for l in el:
        w, i = float(l * (l + 1)), l - 1
        assert b["enstrophy"][i] == r[0, i] and b["kinetic_energy"][i] == r[0, i] / w
        assert b["magnetic_potential"][i] == r[1, i] and b["magnetic_energy"][i] == w * r[1, i]
        assert b["energy"][i] == r[0, i] / w + w * r[1, i]
        assert b["cross_helicity"][i] == r[2, i]
        assert b["kinetic_transfer_advection"][i] == r[3, i] / w and b["enstrophy_transfer_advection"][i] == r[3, i]
        assert b["kinetic_transfer_lorentz"][i] == r[4, i] / w and b["enstrophy_source_lorentz"][i] == r[4, i]
        assert b["magnetic_transfer"][i] == w * r[5, i] and b["potential_transfer"][i] == r[5, i]
        assert b["energy_transfer"][i] == r[3, i] / w + r[4, i] / w + w * r[5, i]
        assert b["cross_helicity_transfer"][i] == r[6, i] + r[7, i] + r[8, i]
    # the fluxes: minus the running sums, in numpy's cumsum order
    for flux, transfer in FLUXES.items():
        acc = 0.0
        for l in el:
            acc += b[transfer][l - 1]
            assert b[flux][l - 1] == -acc, (flux, l)
    # degree 0 is not reported, and the rows are not aliased
    assert all(v.shape == (nmax - 1,) for v in b.values())
    b["enstrophy"][0] = -1.0
    assert rows[0, 1] != -1.0


@pytest.mark.parametrize("coefficients", [False, True])
def test_host_call_band_limited(qfa, monkeypatch, coefficients):
    from quflow_amd import quantization
    N, nmax = 8, 6
    rows = synthetic_rows(nmax)
    ctx = FakeContext(N, rows)
    monkeypatch.setattr(quantization, "_transform_context", lambda n, device, streamed: ctx)
    state = np.stack([skew(N, 1), skew(N, 2)])
    b = qfa.analysis.mhd_spectral_budget(state, lmax=nmax, coefficients=coefficients)
    assert ctx._lib.calls == [("upload", 2), ("budget", nmax)]
    assert set(b) == (KEYS | {"coefficients"} if coefficients else KEYS)
    assert all(b[k].shape == (nmax - 1,) for k in KEYS)
    assert np.array_equal(b["magnetic_potential"], rows[1, 1:])
    if coefficients:
        assert tuple(b["coefficients"]) == COEFFICIENTS
        for v, name in enumerate(COEFFICIENTS):
            assert np.array_equal(b["coefficients"][name], np.arange(v * nmax * nmax, (v + 1) * nmax * nmax))


# ----------------------------------------------------------------------------- argument rules
def test_argument_checks_reach_no_device(qfa, monkeypatch):
    from quflow_amd import integrators
    no_device(monkeypatch)
    N = 8
    state = np.stack([skew(N, 1), skew(N, 2)])
    budget = qfa.analysis.mhd_spectral_budget
    for bad in (1, 0, -2, N + 1, 2.5, True):
        with pytest.raises(ValueError, match="lmax"):
            budget(state, lmax=bad)
    with pytest.raises(NotImplementedError, match="complex64"):
        budget(state.astype(np.complex64))
    for wrong in (state[0], state[:1], np.stack([state[0]] * 3), state[:, :, :4]):
        with pytest.raises(ValueError, match=r"\(2,N,N\)"):
            budget(wrong)
    integrators.select_skewherm(False)
    try:
        with pytest.raises(NotImplementedError, match="skew-Hermitian"):
            budget(state)
    finally:
        integrators.select_skewherm(True)


def test_trajectory_refusals_before_any_library_call(qfa):
    """mhd_budget on a stack that is not the MHD pair, a bad lmax, the non-skew mode: decided from the object alone."""
    from quflow_amd import integrators

    class Lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)

    def bare(k, magnetic):
        st = object.__new__(qfa.DeviceStackTrajectory)
        st.k, st.N, st.magnetic, st._lib = k, 8, magnetic, Lib()
        st.ctx = st._member = None
        return st
    for k, magnetic in ((3, False), (2, False), (1, False)):
        with pytest.raises(ValueError, match="not magnetic"):
            bare(k, magnetic).mhd_budget()
    for bad in (1, 9, 0, 2.5):
        with pytest.raises(ValueError, match="lmax"):
            bare(2, True).mhd_budget(lmax=bad)
    integrators.select_skewherm(False)
    try:
        with pytest.raises(NotImplementedError, match="skew-Hermitian"):
            bare(2, True).mhd_budget()
    finally:
        integrators.select_skewherm(True)
    assert callable(qfa.DeviceMHDTrajectory.mhd_budget) and callable(qfa.DeviceStackTrajectory.spectral_budget)


# ----------------------------------------------------------------------------- the build's records and the ABI
def test_mhd_budget_kernels_in_the_build_records(built):
    """The five-vector sweep over the resident basis and over slabs and the pair form of the degree reduction: no scratch,
    no dynamic stack, all in quantization.res; the sweeps for one, two and three vectors keep their LDS."""
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    five = sorted(k for k in res if k.startswith("k_block_vecmat_five"))
    assert five and all(re.fullmatch(r"k_block_vecmat_five<(true|false)>|k_block_vecmat_five<(true|false), (true|false)>", k)
                        for k in five), five
    slab_flags = {k[:-1].split(", ")[-1].split("<")[-1] for k in five}
    assert slab_flags == {"true", "false"}, five          # resident and slab form
    for name in five + ["k_degree_pair_sums", "k_degree_sums"]:
        assert res[name]["unit"] == "quantization.res", (name, res[name])
        assert res[name]["scratch"] == 0 and not res[name]["dynamic_stack"], (name, res[name])
    # LDS of a five-vector sweep: at most 5 x (256 staged complex + 4 x 2 x 64 partial sums)
    assert all(0 < res[k]["lds"] <= 5 * (256 * 16 + 4 * 2 * 64 * 8) for k in five)
    for nv in (2, 3):
        assert res["k_block_vecmat_multi<%d, false>" % nv]["lds"] == nv * (256 * 16 + 4 * 2 * 64 * 8)
    assert res["k_block_vecmat<0, false>"]["lds"] == 256 * 16 + 4 * 2 * 64 * 8
    assert res["k_degree_pair_sums"]["lds"] == 0 and res["k_degree_pair_sums"]["occupancy"] >= 8


def test_new_symbol_resolves_with_its_signature(built):
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    name = "qf_mhd_spectral_budget"
    assert name in built.SIGNATURES
    fn = getattr(lib, name)
    res, args = built.SIGNATURES[name]
    assert fn.restype is res and list(fn.argtypes) == list(args)
    m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
    assert m, "no prototype in the header"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params == ["qf_ctx *ctx", "int Nmax", "double *out", "double *coeffs"], params
    # a pointer for a pointer, an int for the int
    assert res is ctypes.c_int and args[1] is ctypes.c_int
    assert all(a is ctypes.c_void_p for a in (args[0], args[2], args[3])) and len(args) == 4
    # the buffers the call leaves behind have ids in the header and in the binding, and they agree
    for key, macro in (("P", "QF_BUF_MHD_P"), ("B", "QF_BUF_MHD_B"), ("advection", "QF_BUF_MHD_ADVECTION"),
                       ("lorentz", "QF_BUF_MHD_LORENTZ"), ("induction", "QF_BUF_MHD_INDUCTION")):
        d = re.search(r"#define %s (\d+)" % macro, header)
        assert d and int(d.group(1)) == built.MHD_BUFFER_IDS[key], macro
    assert not set(built.MHD_BUFFER_IDS.values()) & set(built.BUFFER_IDS.values())
    # a null context is refused, not dereferenced
    assert lib.qf_mhd_spectral_budget(None, 4, None, None) == 1
