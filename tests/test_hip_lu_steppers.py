"""GPU tests of isomp_simple / isomp_quasinewton (csrc/api_steppers.hip) where the Newton-Schulz inverse that replaces the
reference's LAPACK LU has work to do: smooth data (|E|_inf = 0.1 at dt = 0.25 hbar, 1.7 at 4 hbar, E = (dt / 2 hbar) P), a
foreign Hamiltonian (general start, explicit A^H), the general branch of select_skewherm(False) (two inverses per step), stiff
steps (|E|_inf = 10, 100, 1000), the refusals, and the resident route DeviceTrajectory.advance_lu.  Cases, data and the numpy
restatement of ns_invert: tests/lu_cases.py; what must hold of the reference alone: tests/test_lu_steppers_host.py.

Sizes, each the smallest that reaches its code: 257 (guarded 32x32 product tiles, odd N, a partial last block in k_lincomb,
k_neg_conj_transpose and the norm), 768 (exact 32x32 tiling, folded solve), 1024 (64x64 tiles), 1025 (guarded tiles above the
64x64 class).

Bars: states 1e-12 absolute against the CPU oracle on data with entries of O(1) -- the bar of
test_hip_parity.py::test_lu_steppers_vs_oracle_large; two CPU evaluations (LU, Newton-Schulz in numpy) differ by at most 6e-15
in these regimes.  The stiff cases: max(1e-12, 8 x the spread of those two CPU evaluations, computed here), 8 for the device's
3M products and its summation order.  Pass counts are equalities: maxit where the tolerance is out of reach, the oracle's where
the tolerance has a factor-3 gap to every residual (lu_cases.exit_tolerance); only the regression on white data at the
automatic, rounding-level tolerance keeps the +-2 of the existing test.  qf_ns_stats (Context.ns_stats) says which path the
device took: at N = 257 it is compared with the restatement's path, above with what |E|_inf implies.  Every case prints its
error and error / bar.

One exception to "maxit passes where the tolerance is out of reach", and why: Wtilde_new = Y (-(Y W)^H) depends on Wtilde
through the inverse Y alone, so a pass whose inverse was KEPT (E moved by less than the inverse's rounding noise) repeats the
pass before it bit for bit and its residual is exactly 0 -- below every positive tolerance, 1e-300 included.  In the 10-pass
case the device therefore ends a step on the first kept inverse after the step's first pass, counted as converged, where the
reference's LU goes on to maxit on residuals of 1e-15 (test_lu_steppers_host.py::test_a_kept_inverse_ends_the_step).  That
case asserts: the state against the oracle's 10 passes, at least one inverse kept, no more than maxit passes per step, and
every step that ended early ended on a kept inverse (inversions = passes, so kept >= steps that did not run out).
"""
import numpy as np
import pytest

import lu_cases as lc

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-11          # isomp_fixedpoint states (tests/test_hip_hooks_large.py)


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


def context_of(qfa, case):
    """The cached context a host-in call of the case ran on (integrators._lu_needs_hook_table)."""
    from quflow_amd.context import get_context, get_stepper_context
    return (get_context if case.ham == "native" and case.skewherm else get_stepper_context)(case.N)


def device_run(qfa, oracle, case, W0=None, dt=None):
    """The case through the host-in entry points: (state, stats, qf_ns_stats)."""
    W = (lc.data(oracle, case) if W0 is None else W0).copy()
    dt = lc.dt_of(oracle, case) if dt is None else dt
    kw = {} if case.ham == "native" else {"hamiltonian": lc.make_foreign(oracle)}
    stats = {}
    with lc.mode_of(oracle, case, qfa):
        if case.stepper == "simple":
            qfa.isomp_simple(W, dt, case.steps, **kw)
        else:
            qfa.isomp_quasinewton(W, dt, case.steps, tol=lc.tolerance(oracle, case), maxit=case.maxit, stats=stats, **kw)
    return W, stats, context_of(qfa, case).ns_stats()


def check_case(qfa, oracle, cid):
    case = lc.CASES[cid]
    e = lc.check_regime(oracle, case)
    ref = lc.reference(oracle, case)
    bar = lc.STATE_BAR
    if cid.startswith("stiff"):
        spread = lc.spread(oracle, case)
        assert spread <= lc.spread_bar(oracle, case)
        bar = max(lc.STATE_BAR, 8.0 * spread)
    W, stats, ns = device_run(qfa, oracle, case)
    print("%s: |E|inf = %.3g, device %s %s" % (cid, e, ns, stats))
    err = report(cid, maxabs(W, ref.W), bar)
    assert np.all(np.isfinite(W)) and err <= bar
    passes = None
    if case.stepper == "qn":
        passes = stats["iterations"] * case.steps
        ran_out = stats["number_of_maxit"] * case.steps
        if cid == "qn10-S257-dt0.25":
            # (module docstring) a kept inverse ends its step on a residual of exactly zero
            assert ns["kept"] >= 1
            assert case.steps <= passes <= case.maxit * case.steps
            assert ns["kept"] >= case.steps - ran_out
        elif case.tol == lc.NO_TOL:
            assert stats["iterations"] == case.maxit and ran_out == case.steps
        elif case.tol == "gap":
            assert stats["iterations"] == ref.iterations and ran_out == 0
            assert stats["tol"] == lc.tolerance(oracle, case)
        else:
            # the automatic, rounding-level tolerance (test_lu_steppers_vs_oracle_large): the state, and convergence
            assert abs(stats["iterations"] - ref.iterations) <= 2.0 and ran_out == 0 and ref.iterations < case.maxit
        assert ns["inversions"] == passes
    else:
        assert ns["inversions"] == case.steps * (1 if case.skewherm else 2)
    if case.N == 257:
        run = lc.restated(oracle, case)
        want = dict(run.ns.counts)
        proviso = lc.cold_start_proviso(run.ns)
        if run.ns2 is not None:
            want = {k: want[k] + run.ns2.counts[k] for k in want}
            proviso = proviso and lc.cold_start_proviso(run.ns2)
        print("   restated %s  %s%s" % (want, run.ns.path(), (" | " + run.ns2.path()) if run.ns2 else ""))
        assert proviso
        assert ns["cold_starts"] == want["cold_starts"]
        # (where the passes end at the rounding level -- the kept inverse of the 10-pass case, the automatic tolerance -- the
        # two sides may make a different number of passes; their inversions are then not the same ones)
        if not (cid == "qn10-S257-dt0.25" or case.regime == "white") or ns["inversions"] == want["inversions"]:
            assert ns["inversions"] == want["inversions"]
            assert abs(ns["iterations"] - want["iterations"]) <= want["inversions"]
    if case.regime == "near1":
        assert ns["cold_starts"] >= 1 and ns["iterations"] >= 6
    if case.regime == "white":
        assert ns["cold_starts"] == 1 and ns["kept"] + ns["iterations"] >= ns["inversions"]
    return W, stats, ns


@pytest.mark.parametrize("cid", lc.ids("simple-S"))
def test_simple_on_smooth_data(qfa, oracle, cid):
    check_case(qfa, oracle, cid)


@pytest.mark.parametrize("cid", lc.ids(("qn10-", "qn4-S")))
def test_quasinewton_fixed_pass_count(qfa, oracle, cid):
    W, stats, ns = check_case(qfa, oracle, cid)
    if cid == "qn10-S257-dt0.25" and stats["number_of_maxit"] < 1.0:
        # a step that did not run out ended on a residual of exactly zero (the resident route, whose statistics keep the last
        # residual, is the same call bit for bit)
        case = lc.CASES[cid]
        tr = qfa.DeviceTrajectory(lc.data(oracle, case))
        try:
            first = tr.advance_lu("isomp_quasinewton", lc.dt_of(oracle, case), 1, tol=case.tol, maxit=case.maxit)
            W1 = tr.download()
            tr.upload(lc.data(oracle, case))
            both = tr.advance_lu("isomp_quasinewton", lc.dt_of(oracle, case), case.steps, tol=case.tol, maxit=case.maxit)
            np.testing.assert_array_equal(tr.download(), W)
        finally:
            tr.ctx.close()
        print("   resident: first step %s, both steps %s" % (first, both))
        assert both["total_iterations"] == stats["iterations"] * case.steps
        for st in (first, both):
            assert st["number_of_maxit"] == 1.0 or st["last_resnorm"] == 0.0
        # the first step alone against the oracle's ten passes: ending on the kept inverse costs the state nothing
        one = lc.run_lu(oracle, case._replace(steps=1))
        assert report(cid + " (first step)", maxabs(W1, one.W), lc.STATE_BAR) <= lc.STATE_BAR


@pytest.mark.parametrize("cid", lc.ids("qnexit-"))
def test_quasinewton_exit_pass_equals_the_oracles(qfa, oracle, cid):
    case = lc.CASES[cid]
    tol, run = lc.exit_tolerance(oracle, case)
    assert tol is not None and lc.has_gap(tol, run.residuals)
    print("%s: tol = %.3e, oracle's passes %s" % (cid, tol, [len(r) for r in run.residuals]))
    check_case(qfa, oracle, cid)


@pytest.mark.parametrize("cid", lc.ids(("simple-foreign", "qn4-foreign")))
def test_foreign_hamiltonian(qfa, oracle, cid):
    check_case(qfa, oracle, cid)


@pytest.mark.parametrize("cid", lc.ids(("simple-general", "qn4-general")))
def test_general_branch(qfa, oracle, cid):
    try:
        check_case(qfa, oracle, cid)
    finally:
        qfa.integrators.select_skewherm(True)
        oracle.select_skewherm(True)


@pytest.mark.parametrize("cid", lc.ids("stiff-"))
def test_stiff_steps(qfa, oracle, cid):
    W, stats, ns = check_case(qfa, oracle, cid)
    assert ns["cold_starts"] == 2                 # a warm residual of 2 to 4: both steps start cold


@pytest.mark.parametrize("cid", lc.ids(("simple-white", "qnauto-white")))
def test_white_data_regression(qfa, oracle, cid):
    W, stats, ns = check_case(qfa, oracle, cid)
    if cid.startswith("simple"):
        assert ns == dict(inversions=2, cold_starts=1, kept=0, iterations=4)


# ----------------------------------------------------------------------------- 7. refusals (error returns, not faults)
def _normal_call_still_right(qfa, oracle, stepper):
    case = lc.SMALL._replace(stepper=stepper, tol=-1.0)
    W, stats, ns = device_run(qfa, oracle, case)
    err = report("normal call after the refusal (%s)" % stepper, maxabs(W, lc.run_lu(oracle, case).W), lc.STATE_BAR)
    assert err <= lc.STATE_BAR


@pytest.mark.parametrize("stepper", ["simple", "qn"])
def test_refusal_above_1e150(qfa, oracle, stepper):
    case = lc.SMALL._replace(stepper=stepper, tol=-1.0)
    dt = lc.dt_of(oracle, case)
    W = lc.scaled_to_e_inf(oracle, lc.white(oracle, case.N), dt, 1e160)
    with pytest.raises(qfa.QuflowHipError, match="too large for the Newton-Schulz inverse"):
        device_run(qfa, oracle, case, W0=W, dt=dt)
    _normal_call_still_right(qfa, oracle, stepper)


def test_regular_data_converges_at_any_scale(qfa, oracle):
    """cond(A) of a regular stream function is the ratio of E's extreme singular values once they are large: |E|_inf = 1e12
    is no harder than 1e3 (19 iterations either way in the restatement).  Relative bar, the state being of size 1e12."""
    case = lc.SMALL
    dt = lc.dt_of(oracle, case)
    W0 = lc.scaled_to_e_inf(oracle, lc.white(oracle, case.N), dt, 1e12)
    ref = lc.run_lu(oracle, case, W0=W0, dt=dt).W
    want = lc.run_ns(oracle, case, W0=W0, dt=dt).ns.counts
    W, stats, ns = device_run(qfa, oracle, case, W0=W0, dt=dt)
    scale = float(np.abs(ref).max())
    print("device %s, restated %s" % (ns, want))
    assert report("regular data at |E|inf = 1e12 (relative)", maxabs(W, ref) / scale, lc.STATE_BAR) <= lc.STATE_BAR
    assert ns["cold_starts"] == 1 and abs(ns["iterations"] - want["iterations"]) <= 1


@pytest.mark.parametrize("stepper", ["simple", "qn"])
def test_unusable_band_is_an_error_not_a_state(qfa, oracle, stepper):
    """A stream function with a null vector at |E|_inf = 1e12: cond(A) = 1e12, the residual's rounding noise (1e-4) never gets
    below the exit level 1e-8 -- the restatement ends with 'did not converge' after 85 iterations, and so must the device."""
    case = lc.SMALL._replace(stepper=stepper, tol=-1.0)
    dt = lc.dt_of(oracle, case)
    W0 = lc.scaled_to_e_inf(oracle, lc.singular(oracle, case.N), dt, 1e12)
    with pytest.raises(lc.NSNoConvergence):
        lc.run_ns(oracle, case, W0=W0, dt=dt)
    with pytest.raises(qfa.QuflowHipError, match="Newton-Schulz did not converge"):
        device_run(qfa, oracle, case, W0=W0, dt=dt)
    ns = context_of(qfa, case).ns_stats()
    print("device", ns)
    assert ns["cold_starts"] == 1 and 20 <= ns["iterations"] <= 200
    _normal_call_still_right(qfa, oracle, stepper)


# ----------------------------------------------------------------------------- 8. the resident route
@pytest.mark.parametrize("cid", ["simple-S257-dt4", "qn4-S257-dt4", "qnexit-S257-dt0.25", "simple-S1025-dt4"])
def test_advance_lu_is_the_host_in_call(qfa, oracle, cid):
    case = lc.CASES[cid]
    W, stats, ns = device_run(qfa, oracle, case)
    tr = qfa.DeviceTrajectory(lc.data(oracle, case))
    try:
        method = "isomp_simple" if case.stepper == "simple" else "isomp_quasinewton"
        if case.stepper == "simple":
            st = tr.advance_lu(method, lc.dt_of(oracle, case), case.steps)
        else:
            st = tr.advance_lu(method, lc.dt_of(oracle, case), case.steps, tol=lc.tolerance(oracle, case), maxit=case.maxit)
        Wr = tr.download()
        nsr = tr.ctx.ns_stats()
    finally:
        tr.ctx.close()
    print("%s: resident %s %s" % (cid, st, nsr))
    np.testing.assert_array_equal(Wr, W)
    assert nsr == ns
    if case.stepper == "simple":
        assert st["iterations"] == 1.0 and st["number_of_maxit"] == 0.0 and st["total_iterations"] == case.steps
    else:
        assert {k: st[k] for k in ("iterations", "number_of_maxit", "tol")} == stats
    report(cid + " (resident)", maxabs(Wr, lc.reference(oracle, case).W), lc.STATE_BAR)
    assert maxabs(Wr, lc.reference(oracle, case).W) <= lc.STATE_BAR


def test_mixed_sequence_on_one_trajectory(qfa, oracle):
    """advance, advance_lu (simple), advance_lu (quasi-Newton), advance on one resident state: the bits of the same sequence of
    host-in calls -- an LU call leaves nothing behind in Whalf, dW, stage, PW and Phalf that the stepper would pick up, and
    clears w_skew_known -- and the oracle's sequence."""
    N = 257
    dt = 0.25 * oracle.hbar(N)
    tol = lc.tolerance(oracle, lc.CASES["qnexit-S257-dt0.25"])
    W0 = lc.smooth(oracle, N)
    tr = qfa.DeviceTrajectory(W0)
    try:
        r = [tr.advance(dt, 2), tr.advance_lu("isomp_simple", dt, 1),
             tr.advance_lu("isomp_quasinewton", dt, 1, tol=tol, maxit=10), tr.advance(dt, 2)]
        Wr = tr.download()
    finally:
        tr.ctx.close()
    h = [{"iterations": 0.0}, None, {}, {"iterations": 0.0}]
    Wh = W0.copy()
    qfa.isomp(Wh, dt, steps=2, stats=h[0])
    qfa.isomp_simple(Wh, dt, 1)
    qfa.isomp_quasinewton(Wh, dt, 1, tol=tol, maxit=10, stats=h[2])
    qfa.isomp(Wh, dt, steps=2, stats=h[3])
    np.testing.assert_array_equal(Wr, Wh)
    o = [{"iterations": 0.0}, None, {}, {"iterations": 0.0}]
    Wo = W0.copy()
    oracle.isomp(Wo, dt, steps=2, stats=o[0])
    oracle.isomp_simple(Wo, dt, 1)
    oracle.isomp_quasinewton(Wo, dt, 1, tol=tol, maxit=10, stats=o[2])
    oracle.isomp(Wo, dt, steps=2, stats=o[3])
    print("iterations per step: resident %s, host-in %s, oracle %s" % (
        [s["iterations"] for s in r], [s and s["iterations"] for s in h], [s and s["iterations"] for s in o]))
    assert report("mixed sequence", maxabs(Wr, Wo), STEP_TOL) <= STEP_TOL
    for k in (0, 3):
        assert r[k]["iterations"] == h[k]["iterations"] == o[k]["iterations"] and r[k]["number_of_maxit"] == 0.0
        assert o[k]["iterations"] >= 2.0
    assert r[2]["iterations"] == h[2]["iterations"] and r[2]["number_of_maxit"] == 0.0
