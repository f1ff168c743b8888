"""Host-side checks of the Casimirs (qf_casimirs, qf_c64_casimirs, qf_states_casimirs, qf_mhd_casimirs; quflow_amd.casimirs
and the trajectories' methods): what can be said without a GPU -- the prototypes and their symbols, the kmax rule, which
reaches no device, and what the code generator made of the new unit's kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

PROTOTYPES = {
    "qf_casimirs": ["qf_ctx *ctx", "const void *W_host", "int kmax", "double *out"],
    "qf_c64_casimirs": ["qf_ctx *ctx", "int kmax", "double *out"],
    "qf_states_casimirs": ["qf_ctx *ctx", "int j", "int kmax", "double *out"],
    "qf_mhd_casimirs": ["qf_ctx *ctx", "int kmax", "double *magnetic", "double *cross"],
}


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


def test_prototypes_and_symbols(built):
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    dp = ctypes.POINTER(ctypes.c_double)
    for name, params in PROTOTYPES.items():
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m, "no prototype of %s in the header" % name
        assert [p.strip() for p in m.group(1).split(",")] == params, (name, m.group(1))
        res, args = built.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
        # a pointer for a pointer, an int for an int
        want = [ctypes.c_int if p.startswith("int ") else dp if p.startswith("double *") else ctypes.c_void_p for p in params]
        assert list(args) == want, (name, args)
    # a null context is refused, not dereferenced
    out = (ctypes.c_double * 8)()
    assert lib.qf_casimirs(None, None, 4, out) == 1
    assert lib.qf_c64_casimirs(None, 4, out) == 1
    assert lib.qf_states_casimirs(None, 0, 4, out) == 1
    assert lib.qf_mhd_casimirs(None, 4, out, out) == 1


class Lib:
    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def bare(cls, **attrs):
    obj = object.__new__(cls)
    obj._lib, obj.ctx = Lib(), None
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


@pytest.mark.parametrize("kmax", [0, 9, -1])
def test_bad_kmax_is_a_value_error_before_any_device(qfa, monkeypatch, kmax):
    from quflow_amd import context, physics

    def refuse(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(context, "Context", refuse)
    monkeypatch.setattr(context, "get_context", refuse)
    monkeypatch.setattr(physics, "get_context", refuse)
    W = np.zeros((4, 4), dtype=np.complex128)
    forms = [
        lambda: qfa.casimirs(W, kmax),
        lambda: qfa.physics.casimirs(W.astype(np.complex64), kmax=kmax),
        lambda: bare(qfa.DeviceTrajectory, c64=False, N=4).casimirs(kmax),
        lambda: bare(qfa.DeviceTrajectory, c64=True, N=4).casimirs(kmax=kmax),
        lambda: bare(qfa.DeviceStackTrajectory, k=3, N=4, magnetic=False).casimirs(0, kmax),
        lambda: bare(qfa.DeviceMHDTrajectory, k=2, N=4, magnetic=True).mhd_casimirs(kmax),
        lambda: bare(qfa.DeviceMHDTrajectory, k=2, N=4, magnetic=True).casimirs(1, kmax=kmax),
        lambda: bare(qfa.DeviceEnsemble, members=[bare(qfa.DeviceTrajectory, c64=False, N=4)]).casimirs(kmax),
    ]
    for form in forms:
        with pytest.raises(ValueError, match="kmax"):
            form()


def test_kmax_must_be_an_integer(qfa):
    for bad in (2.5, "4", None, True):
        with pytest.raises(ValueError, match="kmax"):
            qfa.physics.check_kmax(bad)
    assert [qfa.physics.check_kmax(k) for k in (1, np.int64(8))] == [1, 8]
    assert qfa.casimirs is qfa.physics.casimirs
    # the MHD form on a stack that is not the pair: decided from the object alone
    with pytest.raises(ValueError, match="not magnetic"):
        bare(qfa.DeviceStackTrajectory, k=3, N=4, magnetic=False).mhd_casimirs(4)


def test_casimir_kernels_in_the_build_records(built):
    """The new unit's kernels: the traces kernel for 1..4 stored powers with and without the cross sums, its fold and the
    widening copy -- no scratch, no dynamic stack; the traces kernel's LDS is its two padded 32 x 32 complex tiles and the
    four waves' (sum, compensation) pairs, under the 64 KiB a workgroup gets without asking."""
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    mine = {k: v for k, v in res.items() if v["unit"] == "casimir.res"}
    want = {"k_power_traces<%d, %s>" % (p, m) for p in (1, 2, 3, 4) for m in ("false", "true")}
    want |= {"k_power_traces_fold", "k_widen_c64"}
    assert set(mine) == want, sorted(mine)
    for name, v in mine.items():
        assert v["scratch"] == 0 and not v["dynamic_stack"], (name, v)
        assert v["occupancy"] >= 1, (name, v)
    for p in (1, 2, 3, 4):
        for m, sums in (("false", 2 * p), ("true", 3 * p)):
            lds = res["k_power_traces<%d, %s>" % (p, m)]["lds"]
            assert lds == 2 * 32 * 33 * 16 + 4 * sums * 2 * 8, (p, m, lds)
