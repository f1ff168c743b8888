"""Shared by tests/test_lu_steppers_host.py (CPU) and tests/test_hip_lu_steppers.py (GPU): the cases of isomp_simple /
isomp_quasinewton in which the device's Newton-Schulz inverse (ns_invert, quflow_amd/csrc/api_steppers.hip) has work to do,
their data, and a numpy restatement of ns_invert and of the two steppers around it.  Not a test module.

The REFERENCE of every case is the CPU oracle (oracle/isomp_oracle.py: LAPACK LU, as quflow does it).  The restatement is
not a reference: it runs the device's control flow (cold start, warm continuation, kept inverse, give-up rule, refusal) in
numpy so that (1) the spread of two CPU evaluations of the same step -- LU and Newton-Schulz -- is known per case, which is
what says that the 1e-12 bar has margin in these regimes, and (2) the path the device should take (which inversions start
cold, which are kept, how many iterations) is known and can be compared with qf_ns_stats.

Path notation of `NewtonSchulz.path()`: c = cold start, w = warm continuation, s = inverse kept; the digit is the number of
Newton-Schulz iterations of that inversion; " / " separates steps.
"""
import collections
import contextlib

import numpy as np
import scipy.linalg

SEED = 6                 # skew-Hermitian data: oracle.make_W0_smooth(N, 6) / make_W0(N, 6)
GENERAL_SEED = 3
GENERAL_E_INF = 0.45     # first-pass |E|_inf of the general data (fixes its dt)
STATE_BAR = 1e-12        # the project's bar for these steppers (tests/test_hip_parity.py::test_lu_steppers_vs_oracle_large)
SPREAD_BAR = 1e-13       # LU vs Newton-Schulz, both in numpy: what the two CPU evaluations of a case may differ by
NO_TOL = 1e-300          # an exit tolerance no residual reaches: the pass count is maxit

Case = collections.namedtuple("Case", "id stepper data N dt_hbar e_inf steps tol maxit ham skewherm regime")


def _case(id, stepper, data, N, dt_hbar=None, e_inf=None, steps=2, tol=None, maxit=10, ham="native", skewherm=True, regime=None):
    return Case(id, stepper, data, N, dt_hbar, e_inf, steps, tol, maxit, ham, skewherm, regime)


def _table():
    t = []
    # 1. isomp_simple on smooth data
    for N in (257, 768, 1025):
        t.append(_case("simple-S%d-dt0.25" % N, "simple", "S", N, dt_hbar=0.25))
        t.append(_case("simple-S%d-dt4" % N, "simple", "S", N, dt_hbar=4.0, regime="near1"))
    t.append(_case("simple-S1024-dt4", "simple", "S", 1024, dt_hbar=4.0, regime="near1"))
    # 2. isomp_quasinewton, fixed pass count
    t.append(_case("qn10-S257-dt0.25", "qn", "S", 257, dt_hbar=0.25, tol=NO_TOL, maxit=10))
    for N in (257, 768, 1025):
        t.append(_case("qn4-S%d-dt4" % N, "qn", "S", N, dt_hbar=4.0, tol=NO_TOL, maxit=4, regime="near1"))
    # 3. isomp_quasinewton with an exit test that can be held exactly (tol: exit_tolerance)
    for N in (257, 768, 1025):
        t.append(_case("qnexit-S%d-dt0.25" % N, "qn", "S", N, dt_hbar=0.25, tol="gap", maxit=10))
    # 4. foreign Hamiltonian: skew-Hermitian, which the device cannot know -- general start, explicit A^H
    for N in (257, 1025):
        t.append(_case("simple-foreign%d-dt4" % N, "simple", "S", N, dt_hbar=4.0, ham="foreign"))
        t.append(_case("qn4-foreign%d-dt4" % N, "qn", "S", N, dt_hbar=4.0, steps=1, tol=NO_TOL, maxit=4, ham="foreign"))
    # 5. the general branch, select_skewherm(False) on a general matrix
    for N in (257, 1025):
        t.append(_case("simple-general%d" % N, "simple", "G", N, e_inf=GENERAL_E_INF, skewherm=False, regime="general"))
        t.append(_case("qn4-general%d" % N, "qn", "G", N, e_inf=GENERAL_E_INF, steps=1, tol=NO_TOL, maxit=4, skewherm=False,
                       regime="general"))
    # 6. stiff steps
    for e in (10, 100, 1000):
        t.append(_case("stiff-S257-E%d" % e, "simple", "S", 257, e_inf=float(e), regime="near1"))
    # the regression on white data, where the inverse has nothing to do
    t.append(_case("simple-white257-dt0.25", "simple", "white", 257, dt_hbar=0.25, regime="white"))
    t.append(_case("qnauto-white257-dt0.25", "qn", "white", 257, dt_hbar=0.25, tol=-1.0, maxit=10, regime="white"))
    return collections.OrderedDict((c.id, c) for c in t)


CASES = _table()


def ids(prefixes):
    """The case ids that start with one of `prefixes`, in table order."""
    prefixes = (prefixes,) if isinstance(prefixes, str) else tuple(prefixes)
    return [k for k in CASES if k.startswith(prefixes)]


# ----------------------------------------------------------------------------- data (made once, never written to)
_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        a = make()
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


@contextlib.contextmanager
def general_mode(oracle, qfa=None):
    """select_skewherm(False) on the oracle (and on the device package), restored on the way out."""
    old = oracle.select_skewherm(False)
    if qfa is not None:
        qfa.integrators.select_skewherm(False)
    try:
        yield
    finally:
        oracle.select_skewherm(old)
        if qfa is not None:
            qfa.integrators.select_skewherm(True)


def smooth(oracle, N):
    return _cached(("S", N), lambda: oracle.make_W0_smooth(N, SEED))


def white(oracle, N):
    return _cached(("white", N), lambda: oracle.make_W0(N, SEED))


def general(oracle, N):
    """A random general matrix (seed 3, trace removed) through the oracle's general Poisson solve, trace removed again,
    Frobenius norm sqrt(N): smooth, and not skew-Hermitian."""
    def make():
        rng = np.random.default_rng(GENERAL_SEED)
        G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        G -= np.eye(N) * (np.trace(G) / N)
        with general_mode(oracle):
            G = oracle.solve_poisson(G).copy()
        G -= np.eye(N) * (np.trace(G) / N)
        G /= np.linalg.norm(G, "fro") / np.sqrt(N)
        return G
    return _cached(("G", N), make)


def singular(oracle, N):
    """White data whose stream function has a null vector (its eigenvalue of smallest modulus set to zero, the trace kept):
    A = I - E then has the singular value 1 next to |E|_2, cond(A) = |E|_2 -- the data on which the size of E limits the
    Newton-Schulz inverse (and LAPACK's LU).  Frobenius norm sqrt(N)."""
    def make():
        P = oracle.solve_poisson(oracle.make_W0(N, SEED)).copy()
        lam, V = np.linalg.eigh(1j * P)
        k, j = np.argmin(np.abs(lam)), np.argmax(np.abs(lam))
        lam[j] += lam[k]
        lam[k] = 0.0
        P0 = -1j * (V * lam) @ V.conj().T
        W = oracle.laplace(0.5 * (P0 - P0.conj().T))
        W /= np.linalg.norm(W, "fro") / np.sqrt(N)
        return W
    return _cached(("singular", N), make)


def scaled_to_e_inf(oracle, W0, dt, e_inf):
    """W0 times the factor that makes the first-pass |E|_inf = |(dt / 2 hbar) Delta^-1 W|_inf equal to e_inf."""
    e1 = norm_inf(oracle.solve_poisson(W0)) * dt / (2.0 * oracle.hbar(W0.shape[-1]))
    return W0 * (e_inf / e1)


SMALL = _case("small-16", "simple", "white", 16, dt_hbar=0.25, steps=1)       # the stepper of the refusal and band cases


def data(oracle, case):
    return {"S": smooth, "G": general, "white": white}[case.data](oracle, case.N)


def make_foreign(oracle):
    """0.5 Delta^-1 W + 0.1i I: the same pure-CPU function in the device run and in the oracle run."""
    def foreign(W):
        return 0.5 * oracle.solve_poisson(W) + 0.1j * np.eye(W.shape[-1])
    return foreign


def hamiltonian(oracle, case):
    return make_foreign(oracle) if case.ham == "foreign" else oracle.solve_poisson


def norm_inf(A):
    return float(np.abs(A).sum(axis=1).max())


@contextlib.contextmanager
def mode_of(oracle, case, qfa=None):
    if case.skewherm:
        yield
    else:
        with general_mode(oracle, qfa):
            yield


def dt_of(oracle, case):
    """The case's dt: a multiple of hbar, or what makes the first-pass |E|_inf = |(dt / 2 hbar) hamiltonian(W0)|_inf the
    case's e_inf."""
    def make():
        hb = oracle.hbar(case.N)
        if case.dt_hbar is not None:
            return case.dt_hbar * hb
        with mode_of(oracle, case):
            return 2.0 * hb * case.e_inf / norm_inf(hamiltonian(oracle, case)(data(oracle, case)))
    return _cached(("dt", case.id), make)


def first_e_inf(oracle, case):
    """|E|_inf of the first pass, E = (dt / 2 hbar) hamiltonian(W0)."""
    def make():
        with mode_of(oracle, case):
            P = hamiltonian(oracle, case)(data(oracle, case))
            return norm_inf(P) * dt_of(oracle, case) / (2.0 * oracle.hbar(case.N))
    return _cached(("e", case.id), make)


def check_regime(oracle, case):
    """On CPU values alone: the case is in the regime it is there for, so that it cannot quietly become trivial."""
    e = first_e_inf(oracle, case)
    if case.regime == "near1":
        assert e >= 1.0, (case.id, e)
    elif case.regime == "general":
        assert 0.3 <= e <= 0.6, (case.id, e)
        G = data(oracle, case)
        assert np.abs(G + G.conj().T).max() > 0.1, case.id          # not skew-Hermitian
    elif case.regime == "white":
        assert e <= 0.01, (case.id, e)
    if case.e_inf is not None:
        assert abs(e - case.e_inf) <= 1e-12 * case.e_inf, (case.id, e)
    return e


# ----------------------------------------------------------------------------- ns_invert, restated
class NSRefused(RuntimeError):
    """|E|_inf > 1e150: 'too large for the Newton-Schulz inverse'."""


class NSNoConvergence(RuntimeError):
    """'Newton-Schulz did not converge'."""


class NewtonSchulz:
    """ns_invert of api_steppers.hip on one `ns_work`: Y ~ (I - E)^-1 by Y <- Y + Y (I - A Y), with its control flow.
    `rule`: "below_one" -- a rise of the infinity-norm residual ends the loop once the residual has been below 1;
    "parent" -- the rule before that: any rise after iteration 8."""

    def __init__(self, general=False, rule="below_one", Y=None):
        self.general = general
        self.rule = rule
        self.Y = Y
        self.warm = False
        self.floor = 0.0
        self.counts = dict(inversions=0, cold_starts=0, kept=0, iterations=0)
        self.log = [[]]                  # per step: (kind, iterations) of every inversion
        self.warm_residuals = []         # what a warm inversion measured before it chose its path
        self.sequences = []              # the residuals of every inversion that iterated
        self.cold_iterations = []

    def next_step(self):
        self.log.append([])

    def path(self):
        return " / ".join(" ".join("%s%d" % e for e in step) for step in self.log if step)

    def _residual(self, E):
        R = E @ self.Y
        R -= self.Y
        R[np.diag_indices_from(R)] += 1.0
        return R, norm_inf(R)

    def invert(self, E):
        self.counts["inversions"] += 1
        N = E.shape[0]
        r, R, kind = 2.0, None, "w"
        if self.warm:
            R, r = self._residual(E)
            self.warm_residuals.append(r)
            if self.floor > 0.0 and r <= 2.0 * self.floor:
                self.counts["kept"] += 1
                self.log[-1].append(("s", 0))
                return self.Y
        if not (r < 0.5):
            kind = "c"
            self.counts["cold_starts"] += 1
            en = norm_inf(E)
            if not np.isfinite(en):
                raise ValueError("array must not contain infs or NaNs")
            if en > 1e150:
                raise NSRefused("|dt/(2 hbar) P|_inf = %.3g is too large for the Newton-Schulz inverse" % en)
            if self.general:
                s = 1.0 / ((1.0 + en) * (1.0 + en))
                self.Y = s * (-E.conj().T)
            else:
                s = 1.0 / (1.0 + en * en)
                self.Y = s * E
            self.Y[np.diag_indices(N)] += s
            R, r = self._residual(E)
        seq = [r]
        self.sequences.append(seq)
        below_one = r < 1.0
        its = 0
        for it in range(200):
            self.Y = self.Y + self.Y @ R
            its += 1
            self.counts["iterations"] += 1
            if r < 1e-8:
                self.warm = True
                R, self.floor = self._residual(E)
                self.log[-1].append((kind, its))
                if kind == "c":
                    self.cold_iterations.append(its)
                return self.Y
            r_prev = r
            R, r = self._residual(E)
            seq.append(r)
            if self.rule == "parent":
                if not (r == r) or (it > 8 and r > r_prev):
                    break
            else:
                if not (r == r) or (below_one and r > r_prev):
                    break
                below_one = below_one or r < 1.0
        raise NSNoConvergence("Newton-Schulz did not converge (residual %.3e after %d iterations)" % (r, its))


Run = collections.namedtuple("Run", "W iterations number_of_maxit residuals ns ns2")


def run_ns(oracle, case, tol=None, rule="below_one", W0=None, dt=None):
    """The device's isomp_simple_impl / isomp_quasinewton_impl in numpy, Newton-Schulz inverse included."""
    W = (data(oracle, case) if W0 is None else W0).copy()
    dt = dt_of(oracle, case) if dt is None else dt
    ham = hamiltonian(oracle, case)
    tol = case.tol if tol is None else tol
    N = W.shape[0]
    Id = np.eye(N)
    stepsize = dt / oracle.hbar(N)
    general_branch = not case.skewherm
    foreign = case.ham == "foreign"
    with mode_of(oracle, case), np.errstate(over="ignore", invalid="ignore"):
        if case.stepper == "simple":
            ns = NewtonSchulz(general=foreign or general_branch, rule=rule)
            ns2 = NewtonSchulz(general=True, rule=rule) if general_branch else None
            Wt = W.copy()
            for k in range(case.steps):
                E = (stepsize / 2.0) * ham(Wt)
                Y = ns.invert(E)
                if general_branch:
                    Y2 = ns2.invert(-E)
                    Wt = (Y @ W) @ Y2
                    V = Wt + E @ Wt
                    W = V - V @ E
                    ns2.next_step()
                else:
                    X = Y @ W
                    Wt = Y @ (-X.conj().T)
                    V = (Wt - E.conj().T @ Wt) if foreign else (Wt + E @ Wt)
                    W = V - V @ E
                ns.next_step()
            return Run(W, float(case.steps), 0, [], ns, ns2)
        if tol < 0:
            tol = np.finfo(float).eps * stepsize * norm_inf(W)
        ns = NewtonSchulz(general=foreign or general_branch, rule=rule)
        explicit = foreign or general_branch
        Wt = W.copy()
        total, nmax, residuals = 0, 0, []
        for k in range(case.steps):
            residuals.append([])
            converged = False
            for i in range(case.maxit):
                total += 1
                E = (stepsize / 2.0) * ham(Wt)
                Y = ns.invert(E)
                X = Y @ W
                Wt_new = Y @ (-X.conj().T)
                res = norm_inf(Wt - Wt_new)
                residuals[-1].append(res)
                Wt = Wt_new
                if res < tol:
                    converged = True
                    break
            nmax += 0 if converged else 1
            V = (Wt - E.conj().T @ Wt) if explicit else (Wt + E @ Wt)
            W = V - V @ E
            ns.next_step()
        return Run(W, total / case.steps, nmax / case.steps, residuals, ns, None)


def run_lu(oracle, case, tol=None, W0=None, dt=None):
    """The reference: oracle.isomp_simple as it is; isomp_quasinewton as the oracle's loop (isospectral.py:155-251, LAPACK
    LU) that also lists the residual of every pass and the steps that ran out -- the host tests hold it to the oracle's own
    function bit for bit."""
    W = (data(oracle, case) if W0 is None else W0).copy()
    dt = dt_of(oracle, case) if dt is None else dt
    ham = hamiltonian(oracle, case)
    tol = case.tol if tol is None else tol
    with mode_of(oracle, case):
        if case.stepper == "simple":
            W = oracle.isomp_simple(W, dt, case.steps, hamiltonian=ham, skewherm=case.skewherm)
            return Run(W, float(case.steps), 0, [], None, None)
        stepsize = dt / oracle.hbar(W.shape[-1])
        if tol < 0:
            tol = np.finfo(W.dtype).eps * stepsize * np.linalg.norm(W, np.inf)
        Id = np.eye(W.shape[0])
        Wtilde = W.copy()
        total, nmax, residuals = 0, 0, []
        for k in range(case.steps):
            residuals.append([])
            converged = False
            for i in range(case.maxit):
                total += 1
                Ptilde = ham(Wtilde)
                A = Id - (stepsize / 2.0) * Ptilde
                luA, piv = scipy.linalg.lu_factor(A)
                B = scipy.linalg.lu_solve((luA, piv), W)
                Wtilde_new = scipy.linalg.lu_solve((luA, piv), -B.conj().T)
                resnorm = scipy.linalg.norm(Wtilde - Wtilde_new, np.inf)
                residuals[-1].append(float(resnorm))
                Wtilde = Wtilde_new
                if resnorm < tol:
                    converged = True
                    break
            nmax += 0 if converged else 1
            W_new = A.conj().T @ Wtilde @ A
            np.copyto(W, W_new)
        return Run(W, total / case.steps, nmax / case.steps, residuals, None, None)


# ----------------------------------------------------------------------------- case 3: a tolerance with a gap around it
GAP = 3.0
TOL_CANDIDATES = [10.0 ** (-9.0 - 0.1 * k) for k in range(31)]        # 1e-9 ... 1e-12 in steps of 10^0.1
LISTING_TOL = TOL_CANDIDATES[-1] / 4.0      # a residual below this is more than GAP away from every candidate


def has_gap(tol, residuals):
    return all(not (tol / GAP <= r <= tol * GAP) for step in residuals for r in step)


def exit_tolerance(oracle, case):
    """The first tolerance of 1e-9 ... 1e-12 from which no residual of the oracle's passes is within a factor 3: with it the
    exit pass of every step is decided by the method, not by the last bits of the solve, and the device's pass count must EQUAL
    the oracle's.  Returns (tol, the oracle's Run with that tolerance) -- the gap is asserted on that run's own residuals --
    or (None, the listing run) when there is none."""
    def make():
        listing = run_lu(oracle, case, tol=LISTING_TOL)
        for tol in TOL_CANDIDATES:
            if has_gap(tol, listing.residuals):
                run = run_lu(oracle, case, tol=tol)
                if has_gap(tol, run.residuals):
                    return tol, run
        return None, listing
    return _cached(("gap", case.id), make)


def tolerance(oracle, case):
    return exit_tolerance(oracle, case)[0] if case.tol == "gap" else case.tol


def reference(oracle, case):
    """The oracle's run of the case (cached, read-only)."""
    def make():
        if case.tol == "gap":
            tol, run = exit_tolerance(oracle, case)
            assert tol is not None, case.id
        else:
            run = run_lu(oracle, case)
        run.W.setflags(write=False)
        return run
    return _cached(("lu", case.id), make)


def restated(oracle, case):
    """The restatement's run of the case (cached, read-only)."""
    def make():
        run = run_ns(oracle, case, tol=tolerance(oracle, case))
        run.W.setflags(write=False)
        return run
    return _cached(("ns", case.id), make)


def spread(oracle, case):
    return float(np.abs(reference(oracle, case).W - restated(oracle, case).W).max())


def spread_bar(oracle, case):
    """SPREAD_BAR; a stiff case: a backward-stable solve with A carries a relative error of eps cond(A), and
    cond(A) = sqrt(1 + |E|_2^2) <= 1 + |E|_inf, so two such evaluations may differ by eps |E|_inf on a state of size 1."""
    if case.id.startswith("stiff"):
        return max(SPREAD_BAR, np.finfo(float).eps * case.e_inf)
    return SPREAD_BAR


PROVISO_FACTOR = 1.05


def cold_start_proviso(ns):
    """No warm residual the restatement saw lies within 5 % of the 0.5 threshold, so the device takes the same branch: its
    residual is the same sum of N products per entry in another order, N eps ~ 1e-13 away in relative terms, from a state
    that the bar holds to 1e-12.  (A factor of 2 instead of 1.05 would exclude the very cases that restart cold: at
    dt = 4 hbar the warm residuals of S(257) are 0.573, 0.553, then 0.296 -- 10 % off at the closest.)"""
    return all(not (0.5 / PROVISO_FACTOR <= r <= 0.5 * PROVISO_FACTOR) for r in ns.warm_residuals)
