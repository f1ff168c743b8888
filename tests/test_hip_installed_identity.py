"""GPU tests of the IDENTITY of installed content: that the device works on the forcing pattern, the Hamiltonian offset and the
Hamiltonian table the caller handed over, not on a neighbour that an earlier call left on the context.

A context keeps what qf_set_forcing / qf_set_hamiltonian uploaded and reuses it when the caller's 64-bit key and the library's
own fingerprint both repeat.  The fingerprint reads 4096 strided doubles of the 2 N^2 (from N = 64 an even stride: only real
parts of a matrix, only the diagonal column of a table) plus the last one, so the KEY is what identifies the content:
quflow_amd computes it from every byte (laplacian._content_key).  Every case here runs the sequence F, G, F -- base content,
a neighbour that differs in one entry or one mirrored pair, the base again -- on ONE context, checks each result against a
reference made from that step's own content, and first asserts that the two references differ by at least 1000 times the case's
tolerance (for an equality: that they differ), so a stale hit cannot pass.

Sizes: N = 256 and 257, the smallest at which a key of 65536 strided doubles would skip entries (the fingerprint's stride is 32
there; one size a multiple of 64, one ragged), and N = 1024 once or twice per group (strides 32 and 512).  Perturbations
(tests/test_forcing_host.py, each keeps the matrix exactly skew-Hermitian): the imaginary parts of (1,2)/(2,1); the zonal,
purely imaginary diagonal entry (5,5) -- a Coriolis-like offset changed away from its last entry; the real parts of (1,2)/(2,1),
which no sample reads at N = 1024.  Tables: one coupling coefficient and its partner times 1.5 (tests/test_hamiltonians_host.py).

References, none from the device path under test: the pattern itself and the numpy `mirror` of tests/test_hip_forcing.py through
the host-hook route (equalities, that file's convention); the CPU oracle's solves and its isomp with the matching host callable
(bars of tests/test_hip_hamiltonians.py, imported).  The oracle's solve with the perturbed table is itself checked by its
residual: the operator applied to its P reproduces W within the bar.

test_hip_stochastic.py::test_set_forcing_switches_between_none_affine_and_stochastic runs at N = 33, where key and fingerprint
read every entry, and never returns to the SAME AffineForcing after a stochastic one: that case is here."""
import ctypes

import numpy as np
import pytest

from test_forcing_host import PERTURBATIONS
from test_hamiltonians_host import coupling_perturbed
from test_hip_forcing import coefficients, mirror, run_isomp, skew
from test_hip_hamiltonians import STEP_TOL, evaluation_bar, maxabs, report, resident_class, white

pytestmark = pytest.mark.gpu

CASES = [(256, "imag_pair"), (256, "zonal"), (257, "imag_pair"), (257, "zonal"), (1024, "imag_pair"), (1024, "real_pair")]
SEQUENCE = "FGF"
GAMMA = 50.0


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


# ----------------------------------------------------------------------------- data and references (made once, read only)
_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        a = make()
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def contents(N, name):
    """{"F": base, "G": neighbour}: skew(N, 100, 0.1) of tests/test_hip_forcing.py and its perturbed copy."""
    def make():
        F = skew(N, 100, 0.1)
        G = F.copy()
        PERTURBATIONS[name](G)
        assert np.array_equal(G, -G.conj().T) and int(np.count_nonzero(G != F)) in (1, 2)
        G.setflags(write=False)
        return {"F": F, "G": G}
    return _cached(("contents", N, name), make)


def forced(N, X):
    """All four terms of tests/test_hip_forcing.py with the pattern X."""
    return dict(coefficients(N), F0=X)


def differ(a, b):
    d = maxabs(a, b)
    assert d > 0.0
    return d


# ----------------------------------------------------------------------------- 1. the forcing pattern, kernel alone
@pytest.mark.parametrize("N,name", CASES)
def test_forcing_pattern_kernel_alone(qfa, N, name):
    """AffineForcing.__call__ on the shared per-N context.  All coefficients zero: the pattern comes back bit for bit; with
    every term: the mirror built from the same pattern."""
    c = contents(N, name)
    P, W = skew(N, 1), skew(N, 2)
    want = {k: mirror(qfa, **forced(N, X))(P, W) for k, X in c.items()}
    print("N=%d %s: patterns differ by %.3e, mirrors by %.3e" % (N, name, differ(c["F"], c["G"]), differ(want["F"], want["G"])))
    for step, k in enumerate(SEQUENCE):
        got = qfa.AffineForcing(F0=c[k])(P, W)
        assert np.array_equal(got, c[k]), (step, k, maxabs(got, c[k]))
    for step, k in enumerate(SEQUENCE):
        got = qfa.AffineForcing(**forced(N, c[k]))(P, W)
        assert np.array_equal(got, want[k]), (step, k, maxabs(got, want[k]))


# ----------------------------------------------------------------------------- 2. the forcing in a run
def run_reference(qfa, N, name, k, method):
    """The host-hook run with the mirror of content k: (state, stats)."""
    def make():
        f = mirror(qfa, **forced(N, contents(N, name)[k]))
        dt = 0.25 * qfa.hbar(N)
        if method == "isomp":
            W, stats = run_isomp(qfa, skew(N, 0), dt, 3, f)
            return (W, dict(stats))
        return (qfa.rk4(np.array(skew(N, 0)), dt, steps=2, forcing=f), None)
    return _cached(("run_ref", N, name, k, method), make)


@pytest.mark.parametrize("N,name", CASES)
def test_forcing_in_an_isomp_run(qfa, N, name):
    c = contents(N, name)
    ref = {k: run_reference(qfa, N, name, k, "isomp") for k in c}
    print("isomp N=%d %s: references differ by %.3e" % (N, name, differ(ref["F"][0], ref["G"][0])))
    for step, k in enumerate(SEQUENCE):
        W, stats = run_isomp(qfa, skew(N, 0), 0.25 * qfa.hbar(N), 3, qfa.AffineForcing(**forced(N, c[k])))
        Wr, sr = ref[k]
        assert np.array_equal(W, Wr), (step, k, maxabs(W, Wr))
        assert stats["iterations"] == sr["iterations"] and stats["number_of_maxit"] == sr["number_of_maxit"], (step, stats, sr)
        assert stats["iterations"] >= 2.0


@pytest.mark.parametrize("N,name", CASES)
def test_forcing_in_an_rk4_run(qfa, N, name):
    c = contents(N, name)
    ref = {k: run_reference(qfa, N, name, k, "rk4")[0] for k in c}
    print("rk4 N=%d %s: references differ by %.3e" % (N, name, differ(ref["F"], ref["G"])))
    for step, k in enumerate(SEQUENCE):
        W = qfa.rk4(np.array(skew(N, 0)), 0.25 * qfa.hbar(N), steps=2, forcing=qfa.AffineForcing(**forced(N, c[k])))
        assert np.array_equal(W, ref[k]), (step, k, maxabs(W, ref[k]))


# ----------------------------------------------------------------------------- 3. the resident trajectory
def trajectory_reference(qfa, N, name):
    """Successive host-in isomp calls of 2 steps with the mirrors of F, G, F: [(state, stats, stale)], `stale` the state the
    chunk would have reached with the OTHER pattern."""
    def make():
        c = contents(N, name)
        dt = 0.25 * qfa.hbar(N)
        W = np.array(skew(N, 0))
        out = []
        for k in SEQUENCE:
            other = "G" if k == "F" else "F"
            Wn, stats = run_isomp(qfa, W, dt, 2, mirror(qfa, **forced(N, c[k])))
            stale = run_isomp(qfa, W, dt, 2, mirror(qfa, **forced(N, c[other])))[0] if out else None
            out.append((Wn, dict(stats), stale))
            W = Wn
        return out
    return _cached(("traj_ref", N, name), make)


@pytest.mark.parametrize("N,name", CASES)
def test_resident_trajectory_follows_set_forcing(qfa, N, name):
    c = contents(N, name)
    ref = trajectory_reference(qfa, N, name)
    dt = 0.25 * qfa.hbar(N)
    tr = qfa.DeviceTrajectory(skew(N, 0))
    try:
        for chunk, k in enumerate(SEQUENCE):
            Wr, sr, stale = ref[chunk]
            if stale is not None:
                print("trajectory N=%d %s chunk %d: the other pattern would move the state by %.3e" % (N, name, chunk, differ(Wr, stale)))
            tr.set_forcing(qfa.AffineForcing(**forced(N, c[k])))
            st = tr.advance(dt, 2)
            W = tr.download()
            assert np.array_equal(W, Wr), (chunk, k, maxabs(W, Wr))
            assert st["iterations"] == sr["iterations"] and st["number_of_maxit"] == sr["number_of_maxit"], (chunk, st, sr)
    finally:
        tr.ctx.close()


# ----------------------------------------------------------------------------- 4. the same AffineForcing after a stochastic one
@pytest.mark.parametrize("N", [256, 257, 1024])
def test_affine_pattern_returns_after_a_stochastic_forcing(qfa, N):
    """A stochastic forcing draws its patterns into the buffer the affine pattern lives in (and resets the key the context
    holds): the SAME AffineForcing object installed again must bring F back.  One step each; the stale result -- the
    last drawn pattern taken for F -- is the third chunk with the mirror of that pattern."""
    from test_hip_stochastic import run_params
    dt = 0.25 * qfa.hbar(N)
    F = contents(N, "imag_pair")["F"]
    aff = qfa.AffineForcing(**forced(N, F))
    sf, sf_ref = qfa.StochasticForcing(**run_params(N)), qfa.StochasticForcing(**run_params(N))
    drawn = sf_ref.pattern(0, dt, N)
    W = np.array(skew(N, 0))
    want = []
    for f in (mirror(qfa, **forced(N, F)), sf_ref, mirror(qfa, **forced(N, F))):
        W = qfa.isomp(W, dt, steps=1, forcing=f)
        want.append(W.copy())
    assert sf_ref.step == 1
    stale = qfa.isomp(want[1].copy(), dt, steps=1, forcing=mirror(qfa, **forced(N, drawn)))
    print("N=%d: drawn pattern differs from F by %.3e, the stale third chunk from the true one by %.3e"
          % (N, differ(drawn, F), differ(stale, want[2])))
    tr = qfa.DeviceTrajectory(skew(N, 0), forcing=aff)
    try:
        for chunk, f in enumerate((aff, sf, aff)):
            if chunk:
                tr.set_forcing(f)
            tr.advance(dt, 1)
            got = tr.download()
            assert np.array_equal(got, want[chunk]), (chunk, maxabs(got, want[chunk]))
        assert sf.step == 1
    finally:
        tr.ctx.close()


# ----------------------------------------------------------------------------- 5. the Hamiltonian's offset
HAM_CASES = ([(kind, N, name) for kind in ("poisson", "globalqg") for N, name in CASES if N != 1024]
             + [("poisson", 1024, "imag_pair"), ("globalqg", 1024, "real_pair")])      # (an oracle step at N = 1024 takes 0.4 s)


def hamiltonian(qfa, kind, N, X, cls=None):
    cls = resident_class(qfa) if cls is None else cls
    return cls.poisson(N, offset=X) if kind == "poisson" else cls.globalqg(N, GAMMA, offset=X)


def oracle_hamiltonian(oracle, kind, X):
    """The same Hamiltonian as a host function for the oracle: its solve of W - X (a fresh array: solve_poisson hands back a
    persistent buffer)."""
    if kind == "poisson":
        return lambda W: oracle.solve_poisson(W - X).copy()
    return lambda W: oracle.solve_globalqg(W - X, gamma=GAMMA)


def offset_run_reference(qfa, oracle, kind, N, name, k):
    """The oracle's isomp of 2 steps with content k as offset: (state, stats)."""
    def make():
        sc = {"iterations": 0.0}
        f = oracle_hamiltonian(oracle, kind, contents(N, name)[k])
        Wc = oracle.isomp_fixedpoint(white(oracle, N).copy(), 0.25 * qfa.hbar(N), steps=2, hamiltonian=f, stats=sc)
        assert sc["number_of_maxit"] == 0.0 and sc["iterations"] >= 2.0, sc
        return (Wc, dict(sc))
    return _cached(("offset_run", kind, N, name, k), make)


def offset_run_references(qfa, oracle, kind, N, name):
    ref = {k: offset_run_reference(qfa, oracle, kind, N, name, k) for k in "FG"}
    d = maxabs(ref["F"][0], ref["G"][0])
    print("%s N=%d %s: oracle runs differ by %.3e = %.1e bars" % (kind, N, name, d, d / STEP_TOL))
    assert d >= 1000.0 * STEP_TOL
    return ref


@pytest.mark.parametrize("kind,N,name", HAM_CASES)
def test_offset_in_the_evaluation(qfa, oracle, kind, N, name):
    c = contents(N, name)
    W = white(oracle, N)
    Pc = {k: oracle_hamiltonian(oracle, kind, X)(W) for k, X in c.items()}
    bar = max(evaluation_bar(N, Pc["F"]), evaluation_bar(N, Pc["G"]))
    d = maxabs(Pc["F"], Pc["G"])
    print("H(W) %s N=%d %s: oracle solves differ by %.3e = %.1e bars" % (kind, N, name, d, d / bar))
    assert d >= 1000.0 * bar
    for step, k in enumerate(SEQUENCE):
        Pg = hamiltonian(qfa, kind, N, c[k], cls=qfa.TridiagonalHamiltonian)(W)
        err = report("H(W) %s N=%d %s step %d (%s)" % (kind, N, name, step, k), maxabs(Pg, Pc[k]), evaluation_bar(N, Pc[k]))
        assert err <= evaluation_bar(N, Pc[k]), (step, k, err)


def check_run(tag, Wg, sg, ref):
    Wc, sc = ref
    err = report(tag, maxabs(Wg, Wc), STEP_TOL)
    assert sg["iterations"] == sc["iterations"] and sg["number_of_maxit"] == sc["number_of_maxit"], (tag, sg, sc)
    assert err <= STEP_TOL, (tag, err)


@pytest.mark.parametrize("kind,N,name", HAM_CASES)
def test_offset_in_an_isomp_run(qfa, oracle, kind, N, name):
    c = contents(N, name)
    ref = offset_run_references(qfa, oracle, kind, N, name)
    for step, k in enumerate(SEQUENCE):
        sg = {"iterations": 0.0}
        Wg = qfa.isomp(white(oracle, N).copy(), 0.25 * qfa.hbar(N), steps=2, hamiltonian=hamiltonian(qfa, kind, N, c[k]), stats=sg)
        check_run("isomp %s N=%d %s step %d (%s)" % (kind, N, name, step, k), Wg, sg, ref[k])
        np.testing.assert_allclose(sg["tol_auto"], ref[k][1]["tol_auto"], rtol=1e-12)


@pytest.mark.parametrize("kind,N,name", HAM_CASES)
def test_offset_on_one_device_trajectory(qfa, oracle, kind, N, name):
    """One private context for the whole sequence: each Hamiltonian installed on it in turn, the state uploaded again."""
    c = contents(N, name)
    ref = offset_run_references(qfa, oracle, kind, N, name)
    W0 = white(oracle, N)
    tr = qfa.DeviceTrajectory(W0, hamiltonian=hamiltonian(qfa, kind, N, c["F"]))
    try:
        for step, k in enumerate(SEQUENCE):
            if step:
                H = hamiltonian(qfa, kind, N, c[k])
                H.install(tr.ctx)
                tr.hamiltonian = H
                tr.upload(W0)
            st = tr.advance(0.25 * qfa.hbar(N), 2)
            check_run("DeviceTrajectory %s N=%d %s step %d (%s)" % (kind, N, name, step, k), tr.download(), st, ref[k])
    finally:
        tr.ctx.close()


# ----------------------------------------------------------------------------- 6. the Hamiltonian's table
def apply_table(tab, P):
    """W = T P for an (N,N,2) table in the layout of laplacian(N): entry (i, j) takes tab[i,j,0] P[i,j], tab[i+1,j+1,1] P[i+1,j+1]
    and tab[i,j,1] P[i-1,j-1] (its neighbours on its own diagonal)."""
    W = tab[:, :, 0] * P
    W[:-1, :-1] += tab[1:, 1:, 1] * P[1:, 1:]
    W[1:, 1:] += tab[1:, 1:, 1] * P[:-1, :-1]
    return W


@pytest.mark.parametrize("N", [256, 257, 1024])
def test_table_in_the_evaluation(qfa, oracle, N):
    """T = -1/2 + Delta (shifted), T' = T with one coupling coefficient and its partner times 1.5, T again."""
    S = qfa.TridiagonalHamiltonian.shifted(N, -0.5, -1.0)
    H = {"F": S, "G": qfa.TridiagonalHamiltonian(coupling_perturbed(S.table))}
    assert H["F"].table_key != H["G"].table_key
    W = white(oracle, N)
    Pc = {k: oracle.solve_with_table(H[k].table, W) for k in H}
    for k in H:
        res = report("oracle residual |T P - W| N=%d (%s)" % (N, k), maxabs(apply_table(H[k].table, Pc[k]), W), STEP_TOL)
        assert res <= STEP_TOL, (k, res)
    d = maxabs(Pc["F"], Pc["G"])
    print("table N=%d: oracle solves differ by %.3e = %.1e bars" % (N, d, d / STEP_TOL))
    assert d >= 1000.0 * STEP_TOL
    for step, k in enumerate(SEQUENCE):
        err = report("H(W) table N=%d step %d (%s)" % (N, step, k), maxabs(H[k](W), Pc[k]), STEP_TOL)
        assert err <= STEP_TOL, (step, k, err)


# ----------------------------------------------------------------------------- 7. the C ABI: key 0 always uploads
@pytest.mark.parametrize("name", ["imag_pair", "zonal"])
def test_forcing_key_zero_always_uploads(qfa, name):
    """The N = 256 counterpart of test_hip_forcing.py::test_forcing_key_and_fingerprint: the two patterns have the same
    fingerprint (stride 32: real parts only), and with F0_key = 0 the library must not consult it."""
    from quflow_amd.context import Context, ptr
    from quflow_amd import _lib
    N = 256
    c = contents(N, name)
    P, W = np.array(skew(N, 1)), np.array(skew(N, 2))        # (held here: the library reads them through bare pointers)
    ctx = Context(N)
    try:
        out = np.empty((N, N), dtype=np.complex128)
        for step, k in enumerate(SEQUENCE):
            _lib.check(ctx._lib.qf_set_forcing(ctx.handle, ptr(c[k]), ctypes.c_ulonglong(0), 0.0, 0.0, 0.0))
            _lib.check(ctx._lib.qf_forcing(ctx.handle, ptr(P), ptr(W), ptr(out)))
            assert np.array_equal(out, c[k]), (step, k)
            _lib.check(ctx._lib.qf_clear_forcing(ctx.handle))
    finally:
        ctx.close()
