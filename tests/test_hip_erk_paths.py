"""GPU tests of the explicit steppers' driver (csrc/api_erk.hip): what the four entry points qf_erk, qf_erk_states,
qf_erk_hooked and qf_erk_states_hooked share, and the one path on which the plain entries leave the tiled stage kernel.

1. The general branch from the PLAIN entries: select_skewherm(False) on a general matrix, so both products are formed and
   the stage runs in the flat grid-stride kernel (k_erk_stage_forced without a force term).  N = 1025: its grid of 4096 blocks
   of 256 lanes (1024^2 entries) makes a second trip, and the products' 32-tiles are ragged.  Against the CPU oracle at
   ERK_TOL = 1e-12, the bar of the explicit steppers at this size (tests/test_hip_hooks_large.py).

2. Identities between the entry points, bit for bit: the same table, the same per-state loop and the same kernels run whichever
   entry is taken, so a (1,N,N) stack is the single state, state 0 of a stack of skew-Hermitian states is the single-state run,
   a resident advance_erk is the host-in / host-out call, and a hooked (1,N,N) stack is the hooked single state.  N = 33 (one
   ragged tile beyond the first) and N = 1025.
"""
import numpy as np
import pytest

from test_hip_hooks_large import ERK_TOL, forcing, general, maxabs, report, white

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


@pytest.mark.parametrize("method,stack", [("euler", False), ("heun", False), ("rk4", False), ("rk4", True)])
def test_erk_general_branch_plain_entries(qfa, oracle, method, stack):
    """qf_erk / qf_erk_states under select_skewherm(False) on general data at N = 1025: euler and heun 2 steps, rk4 1 step; rk4
    also on a 2-stack (every state advected by state 0's flow)."""
    N = 1025
    dt = 0.05 * qfa.hbar(N)
    steps = 1 if method == "rk4" else 2
    G0 = general(oracle, N, 5)
    W0 = np.stack([G0, general(oracle, N, 6)]) if stack else G0
    old = oracle.select_skewherm(False)
    qfa.integrators.select_skewherm(False)
    try:
        Wc = getattr(oracle, method)(W0.copy(), dt, steps)
        Wg = getattr(qfa, method)(W0.copy(), dt, steps)
    finally:
        qfa.integrators.select_skewherm(True)
        oracle.select_skewherm(old)
    assert old is True and qfa.laplacian._SKEW_HERM_ is True
    err = report("%s general plain%s N=%d" % (method, " stack" if stack else "", N), maxabs(Wg, Wc), ERK_TOL)
    assert maxabs(Wc, W0) > 1e-6          # (the reference side moved)
    if stack:
        assert maxabs(Wc[1], W0[1]) > 1e-6
    assert err <= ERK_TOL


@pytest.mark.parametrize("method,steps", [("rk4", 1), ("heun", 2)])
@pytest.mark.parametrize("N", [33, 1025])
def test_erk_entry_points_agree_bit_for_bit(qfa, oracle, N, method, steps):
    dt = 0.05 * qfa.hbar(N)
    W0, W1 = white(oracle, N, 1), white(oracle, N, 2)
    run = getattr(qfa, method)
    single = run(W0.copy(), dt, steps)
    assert maxabs(single, W0) > 1e-6
    # a (1,N,N) stack; state 0 of a 2-stack of skew-Hermitian states (one product per stage in both entries)
    assert np.array_equal(run(W0.copy()[None], dt, steps)[0], single)
    pair = run(np.stack([W0, W1]), dt, steps)
    assert np.array_equal(pair[0], single) and maxabs(pair[1], W1) > 1e-6
    # the resident state
    tr = qfa.DeviceTrajectory(W0)
    try:
        tr.advance_erk(method, dt, steps)
        assert np.array_equal(tr.download(), single)
    finally:
        tr.ctx.close()
    # the hooked entries with the same forcing
    hooked = run(W0.copy(), dt, steps, forcing=forcing)
    assert maxabs(hooked, single) > 1e-9      # (the force term entered)
    assert np.array_equal(run(W0.copy()[None], dt, steps, forcing=forcing)[0], hooked)
