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


# ----------------------------------------------------------------------------- the keys identify the content
# The library reuses the factors and the offset a context holds when the key and its own fingerprint both repeat, and the
# fingerprint reads 4096 strided doubles -- from N = 64 an even stride: real parts of an offset, the diagonal column of a
# table -- plus the last one.  The keys alone tell two contents apart (sizes and offset perturbations: test_forcing_host.py).
def coupling_perturbed(table, factor=1.5):
    """A copy of an (N,N,2) table with ONE coupling coefficient changed: entry (2, 3) of the second column -- it ties P[2,3] to
    P[1,2] on the first superdiagonal -- and its partner (3, 2), which the layout of laplacian(N) keeps equal to it."""
    T = np.array(table)
    assert T[2, 3, 1] != 0.0 and T[2, 3, 1] == T[3, 2, 1]
    T[2, 3, 1] *= factor
    T[3, 2, 1] *= factor
    return T


_ONES = {}


def ones_table(N):
    if N not in _ONES:
        _ONES[N] = np.ones((N, N, 2))
        _ONES[N].setflags(write=False)
    return _ONES[N]


@pytest.mark.parametrize("name", ["imag_pair", "real_pair", "zonal"])
@pytest.mark.parametrize("N", [256, 257, 1024])
def test_offset_key_tells_offsets_apart(N, name):
    from quflow_amd import laplacian as lap
    from test_forcing_host import base_and_perturbed
    X, G = base_and_perturbed(N, name)
    tab = ones_table(N)                                  # (any table: nothing is solved here)
    hx, hg = lap.TridiagonalHamiltonian(tab, offset=X), lap.TridiagonalHamiltonian(tab, offset=G)
    assert hx.offset_key != hg.offset_key, (N, name)
    assert hx.offset_key != 0 and hg.offset_key != 0 and hx.table_key == hg.table_key
    # equal content, built twice: the same keys
    h2 = lap.TridiagonalHamiltonian(tab.copy(), offset=X.copy())
    assert (h2.table_key, h2.offset_key) == (hx.table_key, hx.offset_key)
    # the same matrix as a forcing pattern is another cache's content
    assert lap.AffineForcing(X).F0_key != hx.offset_key


@pytest.mark.parametrize("N", [256, 257, 1024])
def test_table_key_tells_tables_apart(host_tables, N):
    lap = host_tables
    S = lap.TridiagonalHamiltonian.shifted(N, -0.5, -1.0)
    T = coupling_perturbed(S.table)
    assert int(np.count_nonzero(T != S.table)) == 2 and np.array_equal(T[:, :, 0], S.table[:, :, 0])
    P = lap.TridiagonalHamiltonian(T)
    assert P.table_key != S.table_key, N
    assert lap.TridiagonalHamiltonian(T.copy()).table_key == P.table_key
    assert lap.TridiagonalHamiltonian.shifted(N, -0.5, -1.0).table_key == S.table_key
    assert P.offset_key == 0 and S.offset_key == 0


def test_keys_are_computed_once_and_install_does_not_hash(host_tables, monkeypatch):
    from test_forcing_host import StubContext, base_and_perturbed, counted_digest
    lap = host_tables
    N = 256
    X, _ = base_and_perturbed(N, "zonal")
    seen = counted_digest(monkeypatch)
    H = lap.TridiagonalHamiltonian(ones_table(N), offset=X)
    assert seen == [("ham_table", (N, N, 2)), ("ham_offset", (N, N))]
    made = [H, lap.TridiagonalHamiltonian.poisson(N), lap.TridiagonalHamiltonian.globalqg(N, 2.0),
            lap.TridiagonalHamiltonian.shifted(N, -0.5, -1.0), lap.TridiagonalHamiltonian.poisson(N, offset=X)]
    assert [tag for tag, _ in seen[2:]] == ["ham_table", "ham_table", "ham_table", "ham_table", "ham_offset"]
    ctx = StubContext(N)
    for h in made:
        for _ in range(2):
            h.install(ctx)
            h.uninstall(ctx)
    assert len(seen) == 7, seen
    sets = [args for name, args in ctx.calls if name == "qf_set_hamiltonian"]
    assert len(sets) == 10 and [name for name, _ in ctx.calls].count("qf_clear_hamiltonian") == 10
    for h, a in zip([h for h in made for _ in range(2)], sets):
        assert (a[1] is None) == h.builtin and (a[3] is None) == (h.offset is None)
        assert h.builtin or a[1].value == h.table.ctypes.data
        assert a[2].value == h.table_key and a[4].value == h.offset_key
        assert h.offset is None or a[3].value == h.offset.ctypes.data


def test_instance_owns_its_arrays(host_tables):
    from test_forcing_host import base_and_perturbed
    lap = host_tables
    N = 256
    X, _ = base_and_perturbed(N, "zonal")
    for tab, off in ((np.array(lap._shifted_table(N, -0.5, -1.0)), X.copy()),                   # contiguous, right dtype
                     (np.asfortranarray(lap._shifted_table(N, -0.5, -1.0)), np.asfortranarray(X))):
        tab0, off0 = tab.copy(), off.copy()
        H = lap.TridiagonalHamiltonian(tab, offset=off)
        keys = (H.table_key, H.offset_key)
        assert not np.shares_memory(H.table, tab) and not np.shares_memory(H.offset, off)
        assert H.table.flags.c_contiguous and H.offset.flags.c_contiguous
        assert not H.table.flags.writeable and not H.offset.flags.writeable
        # the caller goes on with its arrays: a topography edit, another coupling
        tab[2, 3, 1] *= 1.5
        tab[3, 2, 1] *= 1.5
        off[5, 5] += 0.5j
        assert np.array_equal(H.table, tab0) and np.array_equal(H.offset, off0)
        assert (H.table_key, H.offset_key) == keys
        fresh = lap.TridiagonalHamiltonian(tab0, offset=off0)
        assert (fresh.table_key, fresh.offset_key) == keys
        edited = lap.TridiagonalHamiltonian(tab, offset=off)
        assert edited.table_key != keys[0] and edited.offset_key != keys[1]
        with pytest.raises(ValueError):
            H.table[2, 3, 1] = 0.0
        with pytest.raises(ValueError):
            H.offset[5, 5] = 0.0
    # the classmethods go through the constructor: an instance never holds the module's cached table
    S = lap.TridiagonalHamiltonian.shifted(N, -0.5, -1.0)
    G = lap.TridiagonalHamiltonian.globalqg(N, 2.0)
    assert not np.shares_memory(S.table, lap._shifted_table(N, -0.5, -1.0)) and not S.table.flags.writeable
    assert not np.shares_memory(G.table, lap._globalqg_table(N, 2.0)) and not G.table.flags.writeable
    assert lap._shifted_table(N, -0.5, -1.0).flags.writeable          # (the cache's own array is left as it was)
    # ... and a pickled instance comes back write-protected, with its keys
    H1 = lap.TridiagonalHamiltonian.poisson(N, offset=X)
    keys = (H1.table_key, H1.offset_key)
    H2 = pickle.loads(pickle.dumps(H1))
    assert H2.builtin and not H2.table.flags.writeable and not H2.offset.flags.writeable
    # ... keyed again from its content: one stored with keys of sampled entries does not bring them back
    H1.table_key, H1.offset_key = 12345, 6789
    H3 = pickle.loads(pickle.dumps(H1))
    assert (H2.table_key, H2.offset_key) == keys and (H3.table_key, H3.offset_key) == keys


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
