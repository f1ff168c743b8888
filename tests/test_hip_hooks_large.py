"""GPU tests of the steppers that run through csrc/hooks.hip -- qf_isomp_hooked (forcing, foreign Hamiltonian, Strang half
steps, callback, compsum and hooks on (k,N,N) stacks, the general commutator, the magnetic mode of magmp with hooks),
qf_erk_hooked, qf_erk_states_hooked -- and of the plain stack stepper qf_isomp_states, ABOVE N = 1024, against the CPU oracle.

Sizes, each the smallest that reaches its code:
  * 1024  the 64x64 pipelined product (pick_gemm); the last size at which k_hook_update / k_erk_stage_forced make ONE
          grid-stride trip (4096 blocks of 256 threads = N^2 entries exactly) and k_max_rows ONE pass over its 1024 threads:
          the control of the two sizes below.
  * 1025  the bounds-checked generic 32x32 product; 33 row-sum slots whose last tile is one row by one column
          (k_hook_assemble, k_hook_add_forcing, k_magnetic_fix, k_magnetic_update); the second grid-stride trip; row 1024
          in the second pass of k_max_rows.
  * 1056  the exact 32x32 product, 33 full slots, second trips.

Every host hook is the SAME pure-CPU function in the device run and in the oracle run (built from oracle.solve_poisson,
oracle.laplace, oracle.solve_viscdamp), so that only the device's own work enters the comparison.

Bars (all held elsewhere in the suite): isomp state 1e-11 (STEP_TOL), magmp 1e-12 max(1, max|W|), explicit steppers 1e-12;
iteration and maxit counts identical; automatic tolerance to rtol 1e-12; callback records to rtol 1e-9.  Each case also asserts,
on the oracle alone, that no step ended by maxit and that a step took at least 2 iterations (5 on smooth data): the reference
side converges and iterates, a case cannot pass by doing nothing.  compsum cases pass tol=1e-12 (with tol='auto' the exit sits at
rounding level and the counts may differ by one, tests/fuzz_stepper_vs_oracle.py).  Every case prints its error and error / bar.

Two kinds of initial data exist only to make a wrong exit norm visible.  (1) `last_row`: smooth data whose last row and column
are four times heavier, so that the largest row sum -- all that an infinity norm keeps -- sits in row N-1, beyond the first 1024
rows; on seeded white or smooth data the largest row is practically never among the last 1 (N = 1025) or 32 (N = 1056), and a
k_max_rows that skipped them would return the same norm.  (2) a smooth vorticity for magmp with a forcing: on white data both
steps leave the loop after 3 and 2 iterations whether or not the force term enters the residual, on smooth data (6 per step)
the count depends on it.  Both were checked by making the ORACLE wrong in the same way (norm over the first 1024 rows only;
magmp's residual without the force term) at N = 1025 and 1056: `last_row` then changes `tol_auto` by a factor of 3 to 8 and the
iteration counts, the smooth magmp cases change count and state (4.6e-12) in three of four.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-11
ERK_TOL = 1e-12
SAME_TOL = 1e-13          # two device runs of the same arithmetic through different entry points


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def report(tag, err, bar):
    print("%-44s err = %.3e   err/bar = %.3e" % (tag, err, err / bar))
    return err


# ----------------------------------------------------------------------------- initial data (made once, never written to)
_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        a = make()
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def white(oracle, N, seed):
    return _cached(("white", N, seed), lambda: oracle.make_W0(N, seed))


def smooth(oracle, N, seed):
    return _cached(("smooth", N, seed), lambda: oracle.make_W0_smooth(N, seed))


def last_row(oracle, N, seed):
    """Smooth data with the last row and column four times heavier (still skew-Hermitian and trace-free)."""
    def make():
        W = smooth(oracle, N, seed).copy()
        W[N - 1, :] *= 4.0
        W[:, N - 1] *= 4.0
        W -= np.eye(N) * (np.trace(W) / N)
        return W
    return _cached(("last_row", N, seed), make)


def stack2(oracle, N):
    return _cached(("stack2", N), lambda: np.stack([white(oracle, N, 1), white(oracle, N, 2)]))


def mhd_state(oracle, N, vorticity="white"):
    """(W, Theta) with a smooth Theta, as test_states_vs_oracle_large makes it (white Theta: B = Delta Theta is huge)."""
    w = {"white": white, "smooth": smooth, "last_row": last_row}[vorticity]
    return _cached(("mhd", N, vorticity), lambda: np.stack([w(oracle, N, 1), oracle.solve_poisson(white(oracle, N, 2)).copy()]))


def general(oracle, N, seed):
    """A general (not skew-Hermitian) matrix with its trace removed, normalised like make_W0."""
    def make():
        rng = np.random.default_rng(seed)
        G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        G -= np.eye(N) * (np.trace(G) / N)
        G /= np.linalg.norm(G, "fro") / np.sqrt(N)
        return G
    return _cached(("general", N, seed), make)


# ----------------------------------------------------------------------------- hooks: pure CPU, the same in both runs
def forcing(P, W):
    return -0.05 * W + 0.02 * P


def forcing_t(P, W, time=0.0):
    return (-0.05 * np.cos(time)) * W + 0.02 * P


def forcing_state(P, st):
    return -0.05 * st


def forcing_state_t(P, st, time=0.0):
    return (-0.05 * np.cos(time)) * st


def make_hooks(oracle):
    """(solve_poisson hands back one cached buffer: every hook returns an arithmetic result or a copy)"""
    h = {}

    def foreign(W):
        N = W.shape[-1]
        return 0.5 * oracle.solve_poisson(W) + 0.1j * np.eye(N)

    def foreign_per_state(st):
        return np.stack([(0.5 + 0.25 * j) * oracle.solve_poisson(st[j]) for j in range(st.shape[0])])

    def strang_stack(hh, W):
        return np.stack([oracle.solve_viscdamp(hh, W[j], nu=1e-3, alpha=0.05) for j in range(W.shape[0])])

    def mhd_foreign(st):
        return 0.8 * oracle.solve_poisson(st[0]), 0.9 * oracle.laplace(st[1])

    def mhd_foreign_t(st, time=0.0):
        return (0.8 + 0.1 * np.sin(time)) * oracle.solve_poisson(st[0]), 0.9 * oracle.laplace(st[1])
    h.update(foreign=foreign, foreign_per_state=foreign_per_state, strang_stack=strang_stack, mhd_foreign=mhd_foreign,
             mhd_foreign_t=mhd_foreign_t)
    return h


@pytest.fixture(scope="module")
def hooks(oracle):
    return make_hooks(oracle)


class Recorder:
    """callback(W, dW) recording (|W|, |dW|)."""

    def __init__(self):
        self.rows = []

    def __call__(self, W, dW):
        self.rows.append([np.linalg.norm(W), np.linalg.norm(dW)])


def check_isomp(qfa, oracle, tag, W0, dt, kw_dev, kw_cpu=None, min_its=2.0, steps=2):
    """One isomp case: device against oracle at STEP_TOL, counts identical, automatic tolerance to rtol 1e-12; the oracle run
    converged (no maxit) and iterated (>= min_its per step).  Returns (device result, oracle result)."""
    kw_cpu = kw_dev if kw_cpu is None else kw_cpu
    sg, sc = {"iterations": 0.0}, {"iterations": 0.0}
    Wc = oracle.isomp(W0.copy(), dt, steps=steps, stats=sc, **kw_cpu)
    Wg = qfa.isomp(W0.copy(), dt, steps=steps, stats=sg, **kw_dev)
    err = report(tag, maxabs(Wg, Wc), STEP_TOL)
    assert sc["number_of_maxit"] == 0.0 and sc["iterations"] >= min_its, (tag, sc)
    assert sg["iterations"] == sc["iterations"] and sg["number_of_maxit"] == sc["number_of_maxit"], (tag, sg, sc)
    if "tol_auto" in sc or "tol_auto" in sg:
        np.testing.assert_allclose(sg["tol_auto"], sc["tol_auto"], rtol=1e-12)
    assert err <= STEP_TOL, (tag, err)
    return Wg, Wc


def check_magmp(qfa, oracle, tag, S0, dt, kw_dev, kw_cpu=None, min_its=2.0, steps=2):
    """One magmp case: the same against the bar of test_states_golden, relative to the size of the state."""
    kw_cpu = kw_dev if kw_cpu is None else kw_cpu
    sg, sc = {"iterations": 0.0}, {"iterations": 0.0}
    Wc = oracle.magmp_fixedpoint(S0.copy(), dt, steps, stats=sc, **kw_cpu)
    Wg = qfa.magmp(S0.copy(), dt, steps, stats=sg, **kw_dev)
    bar = 1e-12 * max(1.0, float(np.abs(Wc).max()))
    err = report(tag, maxabs(Wg, Wc), bar)
    assert sc["maxit"] == 0.0 and sc["iterations"] >= min_its, (tag, sc)
    assert sg["iterations"] == sc["iterations"] and sg["maxit"] == sc["maxit"], (tag, sg, sc)
    np.testing.assert_allclose(sg["tol"], sc["tol"], rtol=1e-12)
    assert err <= bar, (tag, err, bar)
    return Wg, Wc


# ----------------------------------------------------------------------------- a, b: qf_isomp_hooked, one state
@pytest.mark.parametrize("data", ["white", "smooth", "last_row"])
@pytest.mark.parametrize("N", [1024, 1025, 1056])
def test_isomp_forcing_one_state(qfa, oracle, N, data):
    """forcing = -0.05 W + 0.02 P on white and on smooth initial data (long iteration sequences) at the three sizes, and on
    smooth data whose largest row is the last one (the automatic tolerance is an infinity norm: k_max_rows' second pass)."""
    W0 = {"white": white, "smooth": smooth, "last_row": last_row}[data](oracle, N, 0)
    check_isomp(qfa, oracle, "isomp forcing %s N=%d" % (data, N), W0, 0.25 * qfa.hbar(N), {"forcing": forcing},
                min_its=2.0 if data == "white" else 5.0)


@pytest.mark.parametrize("case", ["forcing_t", "foreign", "reinit"])
def test_isomp_hooks_one_state(qfa, oracle, hooks, case):
    """N = 1025: a time-dependent forcing (time = 0.3), the foreign Hamiltonian 0.5 Delta^-1 W + 0.1i I, `reinitialize`
    with a forcing."""
    N = 1025
    kw = {"forcing_t": {"forcing": forcing_t, "time": 0.3}, "foreign": {"hamiltonian": hooks["foreign"]},
          "reinit": {"reinitialize": True, "forcing": forcing}}[case]
    check_isomp(qfa, oracle, "isomp %s N=%d" % (case, N), white(oracle, N, 0), 0.25 * qfa.hbar(N), kw)


# ----------------------------------------------------------------------------- c, d: qf_isomp_hooked, 2-stack
@pytest.mark.parametrize("case", ["compsum", "callback", "strang", "viscdamp"])
@pytest.mark.parametrize("N", [1025, 1056])
def test_isomp_hooks_on_a_stack(qfa, oracle, hooks, N, case):
    """A (2,N,N) stack: compsum (tol = 1e-12), a callback recording (|W|, |dW|), a host Strang function on the stack, and the
    resident ViscDampStep(nu=1e-3, alpha=0.05) against oracle.solve_viscdamp per state."""
    S0 = stack2(oracle, N)
    dt = 0.25 * qfa.hbar(N)
    tag = "isomp stack %s N=%d" % (case, N)
    if case == "compsum":
        Wg, _ = check_isomp(qfa, oracle, tag, S0, dt, {"compsum": True, "tol": 1e-12})
        assert np.array_equal(Wg[0], -Wg[0].conj().T) and np.array_equal(Wg[1], -Wg[1].conj().T)
    elif case == "callback":
        rg, rc = Recorder(), Recorder()
        check_isomp(qfa, oracle, tag, S0, dt, {"callback": rg}, {"callback": rc})
        assert len(rg.rows) == len(rc.rows) == 2
        np.testing.assert_allclose(np.array(rg.rows), np.array(rc.rows), rtol=1e-9)
    elif case == "strang":
        check_isomp(qfa, oracle, tag, S0, dt, {"strang_splitting": hooks["strang_stack"]})
    else:
        check_isomp(qfa, oracle, tag, S0, dt, {"strang_splitting": qfa.ViscDampStep(nu=1e-3, alpha=0.05)},
                    {"strang_splitting": hooks["strang_stack"]})


def test_isomp_stream_matrix_per_state(qfa, oracle, hooks):
    """N = 1025: a foreign Hamiltonian that returns one stream matrix per state, (2,N,N): the Pj(j) buffers and the exit
    test on `resnormvec.max()` (isospectral.py:527-532)."""
    N = 1025
    check_isomp(qfa, oracle, "isomp stack per-state P N=%d" % N, stack2(oracle, N), 0.25 * qfa.hbar(N),
                {"hamiltonian": hooks["foreign_per_state"]})


# ----------------------------------------------------------------------------- e: the general commutator
@pytest.mark.parametrize("case", ["plain", "forcing", "compsum", "stack"])
def test_isomp_general_branch(qfa, oracle, case):
    """select_skewherm(False) on both sides (the general Poisson solve and `PWcomm -= Whalf @ Phalf`, three products per
    iteration, k_hook_assemble<false>) on a general matrix at N = 1025: plain, forcing, compsum (tol = 1e-12), a 2-stack."""
    N = 1025
    dt = 0.25 * qfa.hbar(N)
    G0 = general(oracle, N, 5)
    W0 = np.stack([G0, general(oracle, N, 6)]) if case == "stack" else G0
    kw = {"plain": {}, "forcing": {"forcing": forcing}, "compsum": {"compsum": True, "tol": 1e-12}, "stack": {}}[case]
    old = oracle.select_skewherm(False)
    qfa.integrators.select_skewherm(False)
    try:
        check_isomp(qfa, oracle, "isomp general %s N=%d" % (case, N), W0, dt, kw)
    finally:
        qfa.integrators.select_skewherm(True)
        oracle.select_skewherm(old)
    assert old is True and qfa.laplacian._SKEW_HERM_ is True


# ----------------------------------------------------------------------------- f: magmp with hooks
@pytest.mark.parametrize("N,case", [(N_, c_) for N_ in (1025, 1056) for c_ in ("forcing", "foreign", "callback", "timed",
                                                                                 "forcing_smooth", "timed_smooth")]
                         + [(1024, "forcing"), (1024, "forcing_smooth")])
def test_magmp_hooks(qfa, oracle, hooks, N, case):
    """qf_isomp_hooked in its magnetic mode: forcing = -0.05 state (k_hook_add_forcing), the foreign pair
    (0.8 Delta^-1 W, 0.9 Delta Theta), a callback, a timed forcing with a timed Hamiltonian at time = 0.5; the two with a
    forcing also on a smooth vorticity, where the iteration count depends on the force term's share of the residual."""
    case, _, vorticity = case.partition("_")
    S0 = mhd_state(oracle, N, vorticity or "white")
    dt = 0.1 * qfa.hbar(N)
    tag = "magmp %s %s N=%d" % (case, vorticity or "white", N)
    if case == "callback":
        rg, rc = Recorder(), Recorder()
        check_magmp(qfa, oracle, tag, S0, dt, {"callback": rg}, {"callback": rc})
        assert len(rg.rows) == len(rc.rows) == 2
        np.testing.assert_allclose(np.array(rg.rows), np.array(rc.rows), rtol=1e-9)
        return
    kw = {"forcing": {"forcing": forcing_state}, "foreign": {"hamiltonian": hooks["mhd_foreign"]},
          "timed": {"time": 0.5, "forcing": forcing_state_t, "hamiltonian": hooks["mhd_foreign_t"]}}[case]
    check_magmp(qfa, oracle, tag, S0, dt, kw, min_its=5.0 if vorticity else 2.0)


# ----------------------------------------------------------------------------- g, h: the explicit steppers with hooks
@pytest.mark.parametrize("N,method,hook", [(1025, m_, h_) for m_ in ("euler", "heun", "rk4") for h_ in ("forcing", "foreign")]
                         + [(1024, "rk4", "forcing"), (1056, "rk4", "forcing")])
def test_erk_hooks_one_state(qfa, oracle, hooks, N, method, hook):
    """qf_erk_hooked: euler and heun (2 steps), rk4 (1 step) with the forcing and with the foreign Hamiltonian."""
    W0 = white(oracle, N, 2)
    dt = 0.05 * qfa.hbar(N)
    steps = 1 if method == "rk4" else 2
    kw = {"forcing": forcing} if hook == "forcing" else {"hamiltonian": hooks["foreign"]}
    Wc = getattr(oracle, method)(W0.copy(), dt, steps, **kw)
    Wg = getattr(qfa, method)(W0.copy(), dt, steps, **kw)
    err = report("%s %s N=%d" % (method, hook, N), maxabs(Wg, Wc), ERK_TOL)
    assert maxabs(Wc, W0) > 1e-6          # (the reference side moved)
    assert err <= ERK_TOL


@pytest.mark.parametrize("method,hook", [("rk4", "forcing"), ("heun", "forcing"), ("rk4", "per_state")])
def test_erk_hooks_on_a_stack(qfa, oracle, hooks, method, hook):
    """qf_erk_states_hooked at N = 1025 on a 2-stack: rk4 and heun with a forcing that returns a stack, rk4 with a foreign
    Hamiltonian that returns one stream matrix per state."""
    N = 1025
    S0 = stack2(oracle, N)
    dt = 0.05 * qfa.hbar(N)
    steps = 1 if method == "rk4" else 2
    kw = {"forcing": forcing} if hook == "forcing" else {"hamiltonian": hooks["foreign_per_state"]}
    Wc = getattr(oracle, method)(S0.copy(), dt, steps, **kw)
    Wg = getattr(qfa, method)(S0.copy(), dt, steps, **kw)
    err = report("%s stack %s N=%d" % (method, hook, N), maxabs(Wg, Wc), ERK_TOL)
    assert maxabs(Wc[1], S0[1]) > 1e-6
    assert err <= ERK_TOL


# ----------------------------------------------------------------------------- i: qf_isomp_states, no hooks
@pytest.mark.parametrize("data", ["white", "last_row"])
@pytest.mark.parametrize("N", [1025, 1056])
def test_states_without_hooks(qfa, oracle, N, data):
    """magmp and a 2-stack isomp through qf_isomp_states, as test_states_vs_oracle_large runs them at 1024; also with a state 0
    whose largest row is the last one (the stepper's own automatic tolerance)."""
    S0 = mhd_state(oracle, N, data)
    Wg, _ = check_magmp(qfa, oracle, "magmp plain %s N=%d" % (data, N), S0, 0.1 * qfa.hbar(N), {}, min_its=2.0 if data == "white" else 5.0)
    assert np.array_equal(Wg[0], -Wg[0].conj().T) and np.array_equal(Wg[1], -Wg[1].conj().T)
    S0 = stack2(oracle, N) if data == "white" else np.stack([last_row(oracle, N, 1), white(oracle, N, 2)])
    check_isomp(qfa, oracle, "isomp stack plain %s N=%d" % (data, N), S0, 0.25 * qfa.hbar(N), {}, min_its=2.0 if data == "white" else 5.0)


# ----------------------------------------------------------------------------- oracle-free identities at N = 1025
def test_hooks_that_change_nothing_change_nothing(qfa, oracle):
    """The hooked loop with a forcing that returns zeros, or a callback that does nothing, against the plain entry points the
    oracle already verifies (qf_isomp, qf_isomp_states): 1e-13, the bar of the small-N tests."""
    N = 1025
    W0 = white(oracle, N, 0)
    dt = 0.25 * qfa.hbar(N)
    sp, sh = {"iterations": 0.0}, {"iterations": 0.0}
    plain = qfa.isomp(W0.copy(), dt, steps=2, stats=sp)
    hooked = qfa.isomp(W0.copy(), dt, steps=2, stats=sh, forcing=lambda P, W: np.zeros_like(W))
    err = report("isomp zero forcing vs plain N=%d" % N, maxabs(hooked, plain), SAME_TOL)
    assert err <= SAME_TOL and sh["iterations"] == sp["iterations"] >= 2.0
    S0 = stack2(oracle, N)
    plain = qfa.isomp(S0.copy(), dt, steps=2, stats=sp)
    hooked = qfa.isomp(S0.copy(), dt, steps=2, stats=sh, callback=lambda W, dW: None)
    err = report("isomp stack idle callback vs plain N=%d" % N, maxabs(hooked, plain), SAME_TOL)
    assert err <= SAME_TOL and sh["iterations"] == sp["iterations"] >= 2.0
    M0 = mhd_state(oracle, N)
    dtm = 0.1 * qfa.hbar(N)
    plain = qfa.magmp(M0.copy(), dtm, 2, stats=sp)
    for name, kw in (("idle callback", {"callback": lambda W, dW: None}), ("zero forcing", {"forcing": lambda P, st: np.zeros_like(st)})):
        hooked = qfa.magmp(M0.copy(), dtm, 2, stats=sh, **kw)
        err = report("magmp %s vs plain N=%d" % (name, N), maxabs(hooked, plain), SAME_TOL)
        assert err <= SAME_TOL and sh["iterations"] == sp["iterations"] >= 2.0


def test_state_0_of_a_hooked_stack_is_the_single_state_run(qfa, oracle):
    """With a shared stream matrix, state 0 of a hooked 2-stack evolves exactly like the single-state hooked run."""
    N = 1025
    dt = 0.25 * qfa.hbar(N)
    S0 = stack2(oracle, N)
    ss, s1 = {"iterations": 0.0}, {"iterations": 0.0}
    Ws = qfa.isomp(S0.copy(), dt, steps=2, stats=ss, forcing=forcing)
    W1 = qfa.isomp(S0[0].copy(), dt, steps=2, stats=s1, forcing=forcing)
    err = report("isomp hooked stack state 0 vs single N=%d" % N, maxabs(Ws[0], W1), SAME_TOL)
    assert err <= SAME_TOL and ss["iterations"] == s1["iterations"] >= 2.0
    assert maxabs(Ws[1], S0[1]) > 1e-6      # (the passive state moved too)
