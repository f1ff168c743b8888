"""CPU checks of the streamed quantization basis (qf_basis_stream): the C ABI exports it and its slab planner, the planner
cuts the blocks m < Nmax into whole-block slabs in order and within the budget, and the Python layer's automatic choice
between the resident and the streamed path follows its thresholds, its environment overrides and a cached basis."""
import ctypes
import inspect

import numpy as np
import pytest

from test_abi_and_host import header_symbols

MIB = 1 << 20


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from quflow_amd import _lib
    return _lib


def test_stream_symbols_exported(built):
    lib = built.load()
    for name in ("qf_basis_stream", "qf_basis_slab_plan"):
        assert name in header_symbols()
        assert name in built.SIGNATURES
        assert hasattr(lib, name)


def plan(lib, N, Nmax, budget):
    """(number of slabs, first block of each) from qf_basis_slab_plan, or (-rc, None)."""
    count = lib.qf_basis_slab_plan(N, Nmax, ctypes.c_longlong(budget), None, 0)
    if count < 0:
        return count, None
    first = (ctypes.c_int * count)()
    assert lib.qf_basis_slab_plan(N, Nmax, ctypes.c_longlong(budget), first, count) == count
    return count, list(first)


def block_bytes(N, Nmax, m):
    return 8 * (N - m) * (Nmax - m)


@pytest.mark.parametrize("N, Nmax", [(2, 2), (3, 1), (31, 31), (64, 17), (257, 257), (1025, 1025), (1024, 128),
                                     (4096, 4096), (8192, 8192), (8192, 128)])
def test_slab_plan_covers_every_block_once_in_order_within_budget(built, N, Nmax):
    lib = built.load()
    b0 = block_bytes(N, Nmax, 0)
    total = sum(block_bytes(N, Nmax, m) for m in range(Nmax))
    for budget in (b0, 3 * b0 + 8, total // 7 + b0, total, 4096 * MIB):
        count, first = plan(lib, N, Nmax, budget)
        assert count >= 1, (N, Nmax, budget)
        assert first[0] == 0 and first == sorted(set(first))
        ends = first[1:] + [Nmax]
        for s, (m0, m1) in enumerate(zip(first, ends)):
            assert m1 > m0
            size = sum(block_bytes(N, Nmax, m) for m in range(m0, m1))
            assert size <= budget, (N, Nmax, budget, s)
            if m1 < Nmax:       # as many whole blocks as fit: the next one would not
                assert size + block_bytes(N, Nmax, m1) > budget
        if budget >= total:
            assert count == 1


def test_slab_plan_one_block_per_slab_at_the_smallest_budget(built):
    lib = built.load()
    N = 64
    count, first = plan(lib, N, N, block_bytes(N, N, 0))
    # block 0 alone fills the budget; blocks 1 and 2 together (63 + 62 rows of 63 and 62) do not fit 64 x 64 either
    assert first[:3] == [0, 1, 2]
    assert count < N        # the small late blocks share slabs


def test_slab_plan_refuses_an_oversized_block(built):
    lib = built.load()
    N, Nmax = 8192, 8192
    b0 = block_bytes(N, Nmax, 0)
    assert b0 == 536870912
    rc = lib.qf_basis_slab_plan(N, Nmax, ctypes.c_longlong(b0 - 8), None, 0)
    assert rc == -1                                          # -QF_ERR_INVALID
    msg = lib.qf_last_error().decode()
    assert str(b0) in msg and str(b0 - 8) in msg, msg
    assert lib.qf_basis_slab_plan(N, Nmax, ctypes.c_longlong(b0), None, 0) > 0
    for bad in ((N, 0), (N, N + 1), (0, 1)):
        assert lib.qf_basis_slab_plan(bad[0], bad[1], ctypes.c_longlong(1 << 40), None, 0) == -1


def test_stream_mode_needs_a_context(built):
    lib = built.load()
    assert lib.qf_basis_stream(None, ctypes.c_longlong(1 << 30)) != 0


# ----------------------------------------------------------------------------- the automatic choice
@pytest.fixture
def q(monkeypatch):
    from quflow_amd import quantization
    monkeypatch.delenv("QUFLOW_HIP_BASIS_RESIDENT_MB", raising=False)
    monkeypatch.delenv("QUFLOW_HIP_BASIS_SLAB_MB", raising=False)
    return quantization


def test_auto_rule_defaults(q):
    for N in (2, 3, 64, 1000, 1024, 1025, 2048):
        assert not q.use_streamed(N), N
    for N in (2600, 4096, 8192):
        assert q.use_streamed(N), N
    # the largest resident N under the default 32768 MiB
    last = max(N for N in range(2000, 3000) if q.basis_size(N) * 8 <= 32768 * MIB)
    assert not q.use_streamed(last) and q.use_streamed(last + 1)
    for N in (64, 8192):
        assert q.use_streamed(N, True) and not q.use_streamed(N, False)
    assert q.slab_bytes() == 4096 * MIB


def test_auto_rule_environment(q, monkeypatch):
    N = 1024
    exact_mb = q.basis_size(N) * 8 / MIB
    monkeypatch.setenv("QUFLOW_HIP_BASIS_RESIDENT_MB", repr(exact_mb))
    assert not q.use_streamed(N)
    monkeypatch.setenv("QUFLOW_HIP_BASIS_RESIDENT_MB", repr(exact_mb - 1e-3))
    assert q.use_streamed(N)
    monkeypatch.setenv("QUFLOW_HIP_BASIS_RESIDENT_MB", "0")
    assert q.use_streamed(2) and not q.use_streamed(2, False)
    monkeypatch.setenv("QUFLOW_HIP_BASIS_RESIDENT_MB", "1e9")
    assert not q.use_streamed(8192) and q.use_streamed(8192, True)
    monkeypatch.setenv("QUFLOW_HIP_BASIS_SLAB_MB", "64")
    assert q.slab_bytes() == 64 * MIB
    monkeypatch.setenv("QUFLOW_HIP_BASIS_SLAB_MB", "0.5")
    assert q.slab_bytes() == MIB // 2


def test_a_cached_basis_wins(q, monkeypatch):
    """A basis in the cache (set_basis, an earlier get_basis) is what the transforms use, whatever its size."""
    N = 4096
    assert q.use_streamed(N)
    monkeypatch.setitem(q._basis_cache, (N, np.dtype(np.float64)), np.zeros(1))
    assert not q.use_streamed(N)
    assert q.use_streamed(N, True)
    monkeypatch.setenv("QUFLOW_HIP_BASIS_RESIDENT_MB", "0")
    assert not q.use_streamed(N)


def test_streamed_is_keyword_only_and_the_reference_signature_stays(q):
    expect = {"shr2mat": ["omega", "N", "berezin", "device"], "mat2shr": ["W", "elmax", "berezin", "device"],
              "shc2mat": ["omega", "N", "berezin", "device"], "mat2shc": ["W", "berezin", "device"]}
    for name, positional in expect.items():
        params = inspect.signature(getattr(q, name)).parameters
        assert [p for p, v in params.items() if v.kind == v.POSITIONAL_OR_KEYWORD] == positional, name
        assert params["streamed"].kind == inspect.Parameter.KEYWORD_ONLY and params["streamed"].default is None
