"""CPU-only conditions of the LU-stepper cases of tests/lu_cases.py (the GPU side is tests/test_hip_lu_steppers.py): what has
to hold of the REFERENCE and of the numpy restatement of the device's Newton-Schulz inverse for the GPU assertions to mean
something, checked where no GPU is needed.

  * every case is in the regime it is there for (first-pass |E|_inf, E = (dt / 2 hbar) P);
  * two CPU evaluations of a case -- the oracle's LAPACK LU and Newton-Schulz in numpy -- agree to 1e-13 (eps |E|_inf for the
    stiff cases), two orders inside the 1e-12 bar the device is held to;
  * the quasi-Newton loop that lists its residuals IS the oracle's isomp_quasinewton, bit for bit;
  * a tolerance with a factor-3 gap to every residual exists at N = 257, 768 and 1025 (case 3);
  * the restatement's paths: an inverse is kept in the 10-pass case, the dt = 4 hbar case restarts cold more than once;
  * the give-up rule: the infinity-norm residual starts above 1 and rises before it falls; the parent's rule (any rise after
    iteration 8) ends an iteration that converges, the rule that waits for a residual below 1 does not;
  * how far the size of E can go: data whose stream function is regular converges at every scale up to the 1e150 refusal
    (the iteration count does not depend on the scale), data whose stream function has a null vector up to |E|_inf ~ 1e8,
    where LU has lost the state as well.
"""
import numpy as np
import pytest

import lu_cases as lc


def show(tag, value, bar):
    print("%-30s %.3e   /bar = %.3e" % (tag, value, value / bar))


@pytest.mark.parametrize("cid", list(lc.CASES))
def test_case_is_in_its_regime_and_the_two_cpu_evaluations_agree(oracle, cid):
    case = lc.CASES[cid]
    e = lc.check_regime(oracle, case)
    ref, ns = lc.reference(oracle, case), lc.restated(oracle, case)
    s, bar = lc.spread(oracle, case), lc.spread_bar(oracle, case)
    print("%-26s |E|inf = %.3g   path %s%s" % (cid, e, ns.ns.path(), (" | " + ns.ns2.path()) if ns.ns2 else ""))
    show("LU vs Newton-Schulz (numpy)", s, bar)
    if case.regime != "white":
        assert 0.5 <= np.abs(ref.W).max() <= 4.0      # entries of O(1): the absolute 1e-12 is a relative one
    assert s <= bar
    if case.stepper == "qn" and case.tol == lc.NO_TOL:
        assert ref.iterations == case.maxit and ref.number_of_maxit == 1.0
    if case.regime == "near1":
        assert ns.ns.cold_iterations[0] >= 6


@pytest.mark.parametrize("cid", ["qn10-S257-dt0.25", "qn4-S257-dt4", "qn4-foreign257-dt4", "qn4-general257",
                                 "qnauto-white257-dt0.25"])
def test_listing_loop_is_the_oracles(oracle, cid):
    case = lc.CASES[cid]
    run = lc.reference(oracle, case)
    st = {}
    with lc.mode_of(oracle, case):
        W = oracle.isomp_quasinewton(lc.data(oracle, case).copy(), lc.dt_of(oracle, case), case.steps,
                                     hamiltonian=lc.hamiltonian(oracle, case), tol=case.tol, maxit=case.maxit, stats=st)
    np.testing.assert_array_equal(run.W, W)
    assert run.iterations == st["iterations"]
    assert [len(r) for r in run.residuals] == [case.maxit] * case.steps or case.tol < 0


@pytest.mark.parametrize("N", [257, 768, 1025])
def test_exit_tolerance_with_a_gap_exists(oracle, N):
    case = lc.CASES["qnexit-S%d-dt0.25" % N]
    tol, run = lc.exit_tolerance(oracle, case)
    print("N = %d: tol = %.3e, passes per step %s" % (N, tol or 0.0, [len(r) for r in run.residuals]))
    for r in run.residuals:
        print("   " + " ".join("%.1e" % x for x in r))
    assert tol is not None and 1e-12 * (1 - 1e-12) <= tol <= 1e-9
    assert lc.has_gap(tol, run.residuals)
    assert run.number_of_maxit == 0 and all(2 <= len(r) < case.maxit for r in run.residuals)
    # the exit pass of a step is the first below the tolerance, by more than the gap; the one before is above, by more than it
    for r in run.residuals:
        assert r[-1] < tol / lc.GAP and r[-2] > tol * lc.GAP
    if N == 257:
        listing = lc.run_lu(oracle, case, tol=lc.LISTING_TOL)
        assert lc.has_gap(3e-12, listing.residuals)
        # about 80 x per pass
        assert 40 < listing.residuals[0][1] / listing.residuals[0][2] < 160


def test_restated_paths(oracle):
    kept = lc.restated(oracle, lc.CASES["qn10-S257-dt0.25"]).ns
    print("qn10, dt = 0.25 hbar:", kept.path())
    assert kept.counts["kept"] >= 1 and kept.counts["cold_starts"] == 1
    cold = lc.restated(oracle, lc.CASES["qn4-S257-dt4"]).ns
    print("qn4, dt = 4 hbar:   ", cold.path())
    assert cold.counts["cold_starts"] >= 2 and cold.counts["kept"] == 0
    assert max(cold.warm_residuals) >= 0.5 > min(cold.warm_residuals)
    white = lc.restated(oracle, lc.CASES["simple-white257-dt0.25"]).ns
    print("white, dt = 0.25 hbar:", white.path())
    assert white.counts == dict(inversions=2, cold_starts=1, kept=0, iterations=4)
    for cid in lc.ids(("simple-S257", "qn", "simple-foreign257", "simple-general257", "stiff")):
        if lc.CASES[cid].N == 257:
            assert lc.cold_start_proviso(lc.restated(oracle, lc.CASES[cid]).ns), cid


def test_a_kept_inverse_ends_the_step(oracle):
    """Wtilde_new = Y (-(Y W)^H) depends on Wtilde through Y alone: a pass whose inverse is kept, other than a step's first,
    repeats the previous pass bit for bit, its residual is exactly 0, and `resnorm < tol` holds for every positive tol -- the
    step ends there, counted as converged.  With the reference's LU the passes go on to maxit on residuals of 1e-15."""
    case = lc.CASES["qn10-S257-dt0.25"]
    ref, ns = lc.reference(oracle, case), lc.restated(oracle, case)
    assert ref.iterations == case.maxit
    for res, log in zip(ns.residuals, ns.ns.log):
        later_kept = [i for i, (kind, _) in enumerate(log) if kind == "s" and i > 0]
        if later_kept:
            assert later_kept == [len(log) - 1] and res[-1] == 0.0
        else:
            assert len(log) == case.maxit and min(res) > 0.0


def test_give_up_rule(oracle):
    case = lc.CASES["stiff-S257-E1000"]
    ok = lc.restated(oracle, case).ns
    first = ok.sequences[0]
    print("|E|inf = 1000:", " ".join("%.3g" % r for r in first))
    rises = [k for k in range(1, len(first)) if first[k] > first[k - 1]]
    assert first[0] > 1.0 and rises and max(rises) >= 9          # the infinity norm rises before it falls, past iteration 8
    below = next(k for k, r in enumerate(first) if r < 1.0)
    assert max(rises) < below and all(first[k + 1] <= first[k] ** 2 * (1 + 1e-6) + 1e-11 for k in range(below, len(first) - 1))
    assert ok.log[0] == [("c", len(first))] and 20 <= len(first) <= 26
    with pytest.raises(lc.NSNoConvergence):
        lc.run_ns(oracle, case, rule="parent")
    # |E|inf = 100 gets through the parent's rule by one iteration; both rules then do the same
    mild = lc.CASES["stiff-S257-E100"]
    np.testing.assert_array_equal(lc.run_ns(oracle, mild, rule="parent").W, lc.restated(oracle, mild).W)


def test_how_large_E_may_be(oracle):
    case, N = lc.SMALL, lc.SMALL.N
    dt = lc.dt_of(oracle, case)
    eps = np.finfo(float).eps

    def both(W0, e):
        W = lc.scaled_to_e_inf(oracle, W0, dt, e)
        with np.errstate(all="ignore"):
            ref = lc.run_lu(oracle, case, W0=W, dt=dt).W
        run = lc.run_ns(oracle, case, W0=W, dt=dt)
        return float(np.abs(run.W - ref).max() / np.abs(ref).max()), run.ns

    # a regular stream function: cond(A) is the ratio of E's extreme singular values once they are large -- the scale drops out
    counts = set()
    for e in (1e3, 1e12, 1e100, 1e149):
        rel, ns = both(lc.white(oracle, N), e)
        print("regular  |E|inf = %.0e: %s, relative spread %.2e" % (e, ns.path(), rel))
        assert rel <= 1e-13
        counts.add(ns.counts["iterations"])
    assert len(counts) == 1
    with pytest.raises(lc.NSRefused, match="too large for the Newton-Schulz inverse"):
        both(lc.white(oracle, N), 1e160)
    # a null vector: cond(A) = |E|_2; the residual's rounding noise, eps cond(A), must get below the exit level 1e-8
    P = oracle.solve_poisson(lc.singular(oracle, N))
    sv = np.linalg.svd(P, compute_uv=False)
    assert sv[-1] <= 1e-14 * sv[0] < 1e-3 * sv[0] <= sv[-2]
    for e in (1e2, 1e4, 1e6):
        rel, ns = both(lc.singular(oracle, N), e)
        print("singular |E|inf = %.0e: %s, relative spread %.2e" % (e, ns.path(), rel))
        assert rel <= max(1e-13, eps * e * e)           # eps cond(A)^2: what LU itself loses of the state
        assert ns.counts["iterations"] >= np.log2(e * e)
    for e in (1e10, 1e12, 1e100):
        with pytest.raises(lc.NSNoConvergence):
            both(lc.singular(oracle, N), e)
