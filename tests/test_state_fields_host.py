"""Host-side checks of the function-space output (qf_state_fields, transforms.state_fields, DeviceTrajectory.fields,
Simulation(..., function_space=True)): what can be said without a GPU -- the mapping from a qutype to its coefficients,
multipliers and variable; the reference's two ValueErrors and the refusal of complex rows; the opt-in keyword; a record
that creates and appends rows through the one seam that fetches fields (replaced by numpy here); the new symbol's
prototype; what the code generator made of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from quflow_amd import _lib
    return _lib


def skew(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return A - A.conj().T


# ----------------------------------------------------------------------------- the mapping
@pytest.mark.parametrize("N", [3, 8, 33, 130, 257])
def test_qutype_to_coefficients_multipliers_and_variable(N):
    from quflow_amd.transforms import FUNCTION_VARNAMES, field_spec
    half = (N // 2) ** 2
    assert field_spec('fun', N) == (N * N, True, 'fun')
    assert field_spec('funL2', N) == (N * N, False, 'funL2')
    assert field_spec('funhalf', N) == (half, True, 'fun')
    assert field_spec('funL2half', N) == (half, False, 'funL2')
    assert FUNCTION_VARNAMES == {'fun': 'fun', 'funhalf': 'fun', 'funL2': 'funL2', 'funL2half': 'funL2'}
    with pytest.raises(KeyError):
        field_spec('shr', N)


def test_the_two_conflicts_and_the_dtype_rules():
    from quflow_amd.transforms import check_function_qutypes
    with pytest.raises(ValueError, match="Cannot have both fun and funhalf outputs."):
        check_function_qutypes({'fun': np.float32, 'funhalf': np.float32})
    with pytest.raises(ValueError, match="Cannot have both funL2 and funL2half outputs."):
        check_function_qutypes({'mat': None, 'funL2': np.float32, 'funL2half': np.float64})
    for bad in (np.complex64, np.complex128, complex):
        with pytest.raises(NotImplementedError, match="complex"):
            check_function_qutypes({'fun': bad})
    with pytest.raises(NotImplementedError):
        check_function_qutypes({'funL2': np.float16})
    got = check_function_qutypes({'mat': None, 'shr': np.float32, 'funhalf': np.float32, 'funL2': None, })
    assert got == {'funhalf': np.dtype(np.float32), 'funL2': np.dtype(np.float64)} and list(got) == ['funhalf', 'funL2']


# ----------------------------------------------------------------------------- the keyword
def test_the_keyword_is_opt_in_and_the_refusal_names_it(tmp_path):
    import inspect
    from quflow_amd.simulation import Simulation
    assert inspect.signature(Simulation.__init__).parameters["function_space"].default is False
    W = skew(8, 0)
    for q in ('fun', 'funL2', 'funhalf', 'funL2half'):
        with pytest.raises(NotImplementedError, match="function_space=True"):
            Simulation(str(tmp_path / "a"), state=W, qutypes={'mat': None, q: np.float32})
    assert not os.path.exists(str(tmp_path / "a"))
    # with the keyword: the reference's ValueErrors and the refusal of complex rows, before anything is written
    with pytest.raises(ValueError, match="fun and funhalf"):
        Simulation(str(tmp_path / "b"), state=W, qutypes={'fun': np.float32, 'funhalf': np.float32}, function_space=True)
    with pytest.raises(ValueError, match="funL2 and funL2half"):
        Simulation(str(tmp_path / "b"), state=W, qutypes={'funL2': np.float32, 'funL2half': np.float32}, function_space=True)
    with pytest.raises(NotImplementedError, match="complex"):
        Simulation(str(tmp_path / "b"), state=W, qutypes={'fun': np.complex128}, function_space=True)
    assert not os.path.exists(str(tmp_path / "b"))
    # an unknown qutype stays refused either way
    with pytest.raises(NotImplementedError):
        Simulation(str(tmp_path / "b"), state=W, qutypes={'img': np.uint8}, function_space=True)


# ----------------------------------------------------------------------------- a record through the seam
class Seam:
    """Stands where transforms.state_fields would: grids of the right shapes filled with a number that names the call."""

    def __init__(self):
        self.calls = []
        self.fail = False

    def __call__(self, W, qutypes):
        from quflow_amd.transforms import _bandwidth, field_spec
        if self.fail:
            raise RuntimeError("no device")
        self.calls.append(dict(qutypes))
        W = np.asarray(W)
        N, lead = W.shape[-1], W.shape[:-2]
        out = {}
        for q, dt in qutypes.items():
            L = _bandwidth(field_spec(q, N)[0], -1)
            out[q] = np.full(lead + (L, 2 * L - 1), len(self.calls) + (0.5 if 'L2' in q else 0.0), dtype=dt)
        return out


@pytest.mark.parametrize("stack", [False, True], ids=["state", "stack"])
def test_a_record_creates_and_appends_rows_through_the_seam(tmp_path, monkeypatch, stack):
    from quflow_amd import simulation
    from quflow_amd.simulation import Simulation
    seam = Seam()
    monkeypatch.setattr(simulation, "_state_fields", seam)
    N, L = 9, 4
    W = np.stack([skew(N, 1), skew(N, 2)]) if stack else skew(N, 1)
    lead = (2,) if stack else ()
    qutypes = {'mat': None, 'funhalf': np.float32, 'funL2': np.float64}
    path = str(tmp_path / "rec")
    sim = Simulation(path, state=W, qutypes=qutypes, function_space=True)
    assert seam.calls == [{'funhalf': np.dtype(np.float32), 'funL2': np.dtype(np.float64)}]      # one call for both rows
    f = sim.fieldnames
    assert 'funhalf' not in f and 'funL2half' not in f
    assert f['fun'] == ((1,) + lead + (L, 2 * L - 1), np.dtype(np.float32))
    assert f['funL2'] == ((1,) + lead + (N, 2 * N - 1), np.dtype(np.float64))
    sim(W, delta_time=0.5, delta_steps=2)
    assert len(seam.calls) == 2
    assert np.all(sim['fun', 0] == 1.0) and np.all(sim['fun', 1] == 2.0) and np.all(sim['funL2', 1] == 2.5)
    # rows handed in from a resident trajectory take the seam's place
    given = {'funhalf': np.full(lead + (L, 2 * L - 1), 7, dtype=np.float32), 'funL2': np.full(lead + (N, 2 * N - 1), 8.0)}
    sim(W, delta_time=0.5, delta_steps=2, device_fields=given)
    assert len(seam.calls) == 2 and np.all(sim['fun', 2] == 7.0) and np.all(sim['funL2', 2] == 8.0)
    # the seam raises: nothing is appended, to any dataset
    seam.fail = True
    before = {name: info[0][0] for name, info in sim.fieldnames.items()}
    with pytest.raises(RuntimeError, match="no device"):
        sim(W, delta_time=0.5, delta_steps=2)
    assert {name: info[0][0] for name, info in sim.fieldnames.items()} == before
    assert all(before[name] == 3 for name in ('mat', 'fun', 'funL2', 'time', 'step'))
    seam.fail = False
    # re-opened: with the keyword it appends, without it it refuses and appends nothing
    again = Simulation(path, function_space=True)
    again(W, delta_time=0.5, delta_steps=2)
    assert again.fieldnames['fun'][0][0] == 4 and again['step', -1] == 6
    closed = Simulation(path)
    assert closed.function_space is False
    with pytest.raises(NotImplementedError, match="function_space=True"):
        closed(W, delta_time=0.5, delta_steps=2)
    assert all(closed.fieldnames[name][0][0] == 4 for name in ('mat', 'fun', 'funL2', 'time', 'step'))


def test_without_function_qutypes_the_seam_is_never_asked(tmp_path, monkeypatch):
    from quflow_amd import simulation
    from quflow_amd.simulation import Simulation
    seam = Seam()
    monkeypatch.setattr(simulation, "_state_fields", seam)
    W = skew(6, 3)
    sim = Simulation(str(tmp_path / "rec"), state=W, function_space=True)
    sim(W, delta_time=0.1)
    assert seam.calls == [] and set(sim.fieldnames) == {'mat', 'time', 'step', 'tol_auto', 'iterations', 'number_of_maxit'}


# ----------------------------------------------------------------------------- the ABI and the build's records
def test_the_new_symbol_is_declared_and_resolves(built):
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    assert re.search(r"typedef struct \{ long long n_omega; int berezin; int dtype; \} qf_field;", header)
    assert re.search(r"\bint qf_state_fields\(qf_ctx \*ctx, const void \*W_host, int nfields, const qf_field \*fields, "
                     r"void \*const \*f_host\);", header)
    res, args = built.SIGNATURES["qf_state_fields"]
    fn = lib.qf_state_fields
    assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) == 5
    assert [(n, t) for n, t in built.Field._fields_] == [("n_omega", ctypes.c_longlong), ("berezin", ctypes.c_int),
                                                         ("dtype", ctypes.c_int)]
    assert ctypes.sizeof(built.Field) == 16
    # a null context is refused, not dereferenced
    assert lib.qf_state_fields(None, None, 1, None, None) == 1
    assert re.search(r"\bint qf_shr_held\(qf_ctx \*ctx, double \*omega_host, long long n_omega\);", header)
    assert list(lib.qf_shr_held.argtypes) == list(built.SIGNATURES["qf_shr_held"][1]) and lib.qf_shr_held(None, None, 1) == 1
    import quflow_amd as qfa
    assert callable(qfa.DeviceTrajectory.fields) and callable(qfa.DeviceTrajectory.fields_and_shr) and callable(qfa.DeviceStackTrajectory.fields) and callable(qfa.state_fields)


def test_the_new_kernels_in_the_build_records(built):
    """The stacked pack and Legendre kernels for 1..4 fields and the stacked Fourier stage: no scratch, no dynamic stack, all
    in sht.res; the one-field kernels keep their names."""
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    new = ["k_sht_pack_fields<%d>" % f for f in (1, 2, 3, 4)] + ["k_sht_legendre_fields<%d>" % f for f in (1, 2, 3, 4)]
    new.append("k_sht_fourier_fields")
    assert sorted(k for k in res if "_fields" in k and k.startswith("k_sht_")) == sorted(new)
    for name in new + ["k_sht_pack<true, false>", "k_sht_legendre<false>", "k_sht_fourier"]:
        assert res[name]["unit"] == "sht.res", (name, res[name])
        assert res[name]["scratch"] == 0 and not res[name]["dynamic_stack"], (name, res[name])
    # LDS of the Legendre stage: the recurrence's 256 (A, B) pairs and 256 complex coefficients per field
    for f in (1, 2, 3, 4):
        assert res["k_sht_legendre_fields<%d>" % f]["lds"] == 256 * 16 * (1 + f)
    assert res["k_sht_legendre_fields<1>"]["lds"] == res["k_sht_legendre<false>"]["lds"]
    assert res["k_sht_fourier_fields"]["lds"] == res["k_sht_fourier"]["lds"] == 2 * 16 * 64 * 8
