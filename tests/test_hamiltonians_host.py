"""Host-side checks of the device-resident tridiagonal Hamiltonians (qf_set_hamiltonian, k_solve_off,
quflow_amd.TridiagonalHamiltonian, quflow_amd.coriolis): what can be said without a GPU -- the ABI, what the code generator made
of the offset kernels and of the plain ones next to them, the tables the constructors hand to the library, argument errors,
pickling, and the Coriolis matrix against the CPU oracle's Poisson solve."""
import os
import pickle
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("qf_set_hamiltonian", "qf_clear_hamiltonian", "qf_hamiltonian", "qf_hamiltonian_energy")

# (chunk length L, FOLD) of every class pick_cfg can choose for the skew-Hermitian double-precision solve, with the occupancy
# floor tests/test_abi_and_host.py::test_kernel_resources holds for the plain kernel of that class.  L = 16 has no floor there:
# the offset kernel must not fall below what the plain one has.
OFFSET_CLASSES = {(4, 0): 5, (8, 0): 3, (16, 0): None, (9, 1): 3, (17, 1): 2, (32, 0): 1}

# (vgpr, agpr, occupancy) of the plain instantiations as the parent commit's build recorded them (hipcc of ROCm 7, gfx950): the
# offset form is a second kernel over the same text, and the plain kernels must come out of the code generator as before.  A
# toolchain change that moves these numbers re-records them; a source change must not.
PLAIN_RECORDS = {
    "k_solve<double, 4, 0, 0>": (88, 0, 5), "k_solve<double, 4, 1, 0>": (93, 0, 5),
    "k_solve<double, 8, 0, 0>": (124, 0, 4), "k_solve<double, 8, 1, 0>": (132, 0, 3),
    "k_solve<double, 9, 1, 1>": (146, 0, 3),
    "k_solve<double, 16, 0, 0>": (190, 0, 2), "k_solve<double, 16, 1, 0>": (206, 0, 2),
    "k_solve<double, 17, 1, 1>": (214, 0, 2),
    "k_solve<double, 32, 0, 0>": (256, 72, 1), "k_solve<double, 32, 1, 0>": (256, 104, 1),
    "k_solve<float, 4, 0, 0>": (73, 0, 6), "k_solve<float, 4, 1, 0>": (74, 0, 6),
    "k_solve<float, 8, 0, 0>": (88, 0, 5), "k_solve<float, 8, 1, 0>": (98, 0, 4),
    "k_solve<float, 9, 1, 1>": (108, 0, 4),
    "k_solve<float, 16, 0, 0>": (160, 0, 3), "k_solve<float, 16, 1, 0>": (178, 0, 2),
    "k_solve<float, 17, 1, 1>": (187, 0, 2),
    "k_solve<float, 32, 0, 0>": (255, 50, 1), "k_solve<float, 32, 1, 0>": (256, 68, 1),
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from quflow_amd import _lib
    return _lib


def test_new_symbols_resolve_with_their_signatures(built):
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in built.SIGNATURES, name
        fn = getattr(lib, name)
        res, args = built.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert re.search(r"\bint %s\(qf_ctx \*ctx" % name, header), name
    assert len(built.SIGNATURES["qf_set_hamiltonian"][1]) == 5
    # a null context is refused, not dereferenced
    assert lib.qf_clear_hamiltonian(None) == 1
    assert lib.qf_set_hamiltonian(None, None, 0, None, 0) == 1


def test_offset_kernels_hold_the_plain_kernels_occupancy(built):
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    for (L, fold), floor in OFFSET_CLASSES.items():
        name = "k_solve_off<%d, %d>" % (L, fold)
        plain = "k_solve<double, %d, 1, %d>" % (L, fold)
        assert name in res, (name, sorted(k for k in res if k.startswith("k_solve_off")))
        assert res[name]["unit"] == "poisson.res"
        assert res[name]["scratch"] == 0 and not res[name]["dynamic_stack"], (name, res[name])
        want = floor if floor is not None else res[plain]["occupancy"]
        assert res[name]["occupancy"] >= want, (name, res[name], want)
    assert len([k for k in res if k.startswith("k_solve_off")]) == len(OFFSET_CLASSES)


def test_plain_solve_kernels_are_unchanged(built):
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    got = {k: (res[k]["vgpr"], res[k]["agpr"], res[k]["occupancy"]) for k in res if k.startswith("k_solve<")}
    assert got == PLAIN_RECORDS, {k: (got.get(k), PLAIN_RECORDS.get(k)) for k in set(got) | set(PLAIN_RECORDS)
                                  if got.get(k) != PLAIN_RECORDS.get(k)}


@pytest.fixture()
def host_tables(oracle, monkeypatch):
    """quflow_amd.laplacian with its Laplacian table taken from the CPU oracle and empty table caches: the constructors run
    without a device."""
    from quflow_amd import laplacian as lap
    monkeypatch.setattr(lap, "laplacian", lambda N, bc=False, dtype=np.float64: oracle.laplacian(N, bc, dtype))
    for name, size in (("_table_cache", 8), ("_plain_table_cache", 4), ("_globalqg_cache", 4)):
        monkeypatch.setattr(lap, name, lap._LRU(size))
    return lap


def test_constructors_build_the_tables_of_the_solvers(host_tables, oracle):
    lap = host_tables
    N = 24
    H = lap.TridiagonalHamiltonian.poisson(N)
    assert H.builtin and H.offset is None and H.N == N
    assert np.array_equal(H.table, oracle.laplacian(N, bc=True))
    # globalqg: the table solve_globalqg solves with (oracle.solve_globalqg builds the same one)
    gamma = 50.0
    s = (N - 1) / 2
    z = oracle.hbar(N) * np.arange(-s, s + 1)
    want = oracle.laplacian(N, bc=False).copy()
    want[:, :, 0] -= (gamma / 2.0) * z ** 2
    want[:, :, 0] -= (gamma / 2.0) * z[:, np.newaxis] ** 2
    G = lap.TridiagonalHamiltonian.globalqg(N, gamma)
    assert not G.builtin and np.array_equal(G.table, want)
    assert np.array_equal(lap._globalqg_table(N, gamma), want)
    # shifted: _shifted_table, the operator of solve_helmholtz / solve_heat / solve_viscdamp
    S = lap.TridiagonalHamiltonian.shifted(N, -0.5, -1.0)
    assert np.array_equal(S.table, lap._shifted_table(N, -0.5, -1.0))
    base = oracle.laplacian(N, bc=False)
    assert np.array_equal(S.table[:, :, 0], -0.5 + base[:, :, 0]) and np.array_equal(S.table[:, :, 1], base[:, :, 1])
    # distinct tables, distinct keys; the same table, the same key
    assert len({H.table_key, G.table_key, S.table_key}) == 3
    assert lap.TridiagonalHamiltonian.globalqg(N, gamma).table_key == G.table_key


def test_instances_pickle(host_tables):
    lap = host_tables
    N = 16
    F = lap.coriolis(N, 0.3)
    for H in (lap.TridiagonalHamiltonian.poisson(N, offset=F), lap.TridiagonalHamiltonian.globalqg(N, 2.0)):
        H2 = pickle.loads(pickle.dumps(H))
        assert type(H2) is type(H) and H2.N == H.N and H2.builtin == H.builtin
        assert np.array_equal(H2.table, H.table)
        assert (H.offset is None and H2.offset is None) or np.array_equal(H2.offset, H.offset)
        assert (H2.table_key, H2.offset_key) == (H.table_key, H.offset_key)


def test_argument_errors(host_tables):
    lap = host_tables
    N = 12
    tab = lap._shifted_table(N, 1.0, 0.5)
    with pytest.raises(ValueError, match="table"):
        lap.TridiagonalHamiltonian(np.zeros((N, N)))
    with pytest.raises(ValueError, match="table"):
        lap.TridiagonalHamiltonian(np.zeros((N, N + 1, 2)))
    with pytest.raises(ValueError, match="offset"):
        lap.TridiagonalHamiltonian(tab, offset=np.zeros((N + 1, N + 1), dtype=complex))
    F = lap.coriolis(N, 0.2).copy()
    F[0, 1] = 1e-300                                  # not mirrored: the kernel would read it, the reference both
    with pytest.raises(ValueError, match="skew-Hermitian"):
        lap.TridiagonalHamiltonian(tab, offset=F)
    with pytest.raises(ValueError, match="skew-Hermitian"):
        lap.TridiagonalHamiltonian(tab, offset=np.eye(N))
    H = lap.TridiagonalHamiltonian(tab, offset=lap.coriolis(N, 0.2))
    # a state of another size: refused by every stepper before a context exists (this box has no device to make one on)
    import quflow_amd as qfa
    W = np.zeros((N + 1, N + 1), dtype=np.complex128)
    for stepper in (qfa.isomp, qfa.rk4, qfa.isomp_simple, qfa.isomp_quasinewton):
        with pytest.raises(ValueError, match="built for N=%d" % N):
            stepper(W.copy(), 0.1, 2, hamiltonian=H)
    with pytest.raises(ValueError, match="built for N=%d" % N):
        H(W)


def test_coriolis_matrix(oracle):
    import quflow_amd as qfa
    for N in (5, 64):
        Om = 0.37
        F = qfa.coriolis(N, Om)
        assert F.dtype == np.complex128 and F.shape == (N, N)
        assert np.count_nonzero(F - np.diag(np.diag(F))) == 0
        assert np.array_equal(F, -F.conj().T)
        assert abs(np.trace(F)) <= 1e-13 * np.abs(F).max()
        # 2 Omega cos(theta) = 2 Omega x3, and x3 is quantized to X3 = hbar S3 (cartesian_generators)
        X3 = qfa.cartesian_generators(N)[2]
        # |T_10|_L2 = 1 and T_10 = sqrt(3) X3:  (2 Omega / sqrt(3)) T_10 = 2 Omega X3
        assert np.abs(F - 2.0 * Om * X3).max() <= 1e-13 * np.abs(F).max()
        np.testing.assert_allclose(qfa.norm_L2(F), 2.0 * Om / np.sqrt(3.0), rtol=1e-13)
        # cos(theta) is an l = 1 eigenfunction: Delta^-1 F = -F / 2
        P = oracle.solve_poisson(F).copy()
        assert np.abs(P + F / 2.0).max() <= 1e-12
