"""Rotations, gradients and initial data on the MI355X at the sizes runs use (N = 1025 .. 8192), and the Taylor kernel
at every strip layout, against the closed forms of tests/test_geometry_refs_host.py -- no fixture, no dense host
exponential.  tests/test_hip_geometry.py keeps the fixture sizes 16 and 33.

Every case prints its worst error in the unit of that file, N max(1, |xi|) eps scale; the bar is 8 (24 where two device
rotations and two products enter: the dense-data cases say why).  Every case also asserts the plan it means to test
(`geometry.exp_plan`), so a change of the scaling rule cannot silently move it to another path.

  a  k_so3_taylor alone (sigma = 0) against the long double Horner form, dense, at N around the multiples of the
     32-column strip: windows clipped at one or both matrix edges, the first sizes with an interior strip (95, 96, 97),
     last strips of 1, 31 and 32 columns; |B|_inf = 0.48 (degree 16, the full 64-row window) and 1e-3 (degree 6)
  b  rotation_matrix end to end: the guarded 32 x 32 product (1025, 2049), the exact one (1056), a multiple of 64 that
     the tile rule still sends to 32 x 32 (1536), the pipelined 64 x 64 product (2048, 4096, 8192); extreme columns,
     equivariance, unitarity on a row sample; the pure z rotation against the exact diagonal
  c  rotate of a matrix whose rotation is known in closed form, entrywise over the whole matrix
  d  rotate of dense Gaussian data on a row/column sample, and complex64 input
  e  the resident state: rotate, grad and rotate-then-advance, bit for bit
  f  grad against the long double stencil around its 256-column workgroup boundaries and at 1025, 2049, 4096
  g  north_blob and blob at N = 512, 1025, 2048
"""
import functools

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import dynamics, geometry
from test_geometry_host import EPS, XIS, gen, rot_tol
from test_geometry_refs_host import (LD, block_max, closed_form_case, equivariance_error, extreme_columns, grad_reference,
                                     small_xi, taylor_reference)

pytestmark = pytest.mark.gpu

XI_TURNS = np.array((25.0, -20.0, 24.0))           # |xi| ~ 40: more than six turns, not reduced modulo 2 pi
VECTORS = {"xi0": XIS[0], "xi1": XIS[1], "z": XIS[2], "turns": XI_TURNS, "neg0": -XIS[0]}

TAYLOR_SIZES = (31, 32, 33, 63, 64, 65, 95, 96, 97, 129, 257, 1025)
EXP_SIZES = (1025, 1056, 1536, 2048, 2049, 4096)
EXP_CASES = ([(N, key) for N in EXP_SIZES for key in (("xi1", "z") if N not in (1025, 2048) else tuple(VECTORS))]
             + [(8192, "xi1")])
ROTATE_CASES = [(N, "xi1") for N in EXP_SIZES] + [(2048, "turns")]


def report(what, N, xi, err, scale=1.0, bar=8.0):
    unit = N * max(1.0, float(np.linalg.norm(xi))) * EPS * scale
    print("%-44s N=%5d |xi|=%7.3f  max err = %.3e   err/(N max(1,|xi|) eps scale) = %.3f  (bar %g)"
          % (what, N, np.linalg.norm(xi), err, err / unit, bar))
    assert err <= bar * unit, (what, N, err, bar * unit)


def maxabs(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def assert_squared_plan(xi, N):
    sigma, d = geometry.exp_plan(xi, N)
    assert sigma >= 1 and 14 <= d <= 16, (sigma, d)
    return sigma, d


@functools.lru_cache(maxsize=None)
def row_sample(N):
    """64 rows: the first and last two rows of the first, one interior and the last 32-row and 64-row tile, and seeded
    random rows."""
    rows = set()
    for tile in (32, 64):
        last = (N - 1) // tile
        for t in (0, last // 2, last):
            lo, hi = t * tile, min(N, (t + 1) * tile)
            rows.update((lo, min(lo + 1, hi - 1), max(hi - 2, lo), hi - 1))
    rng = np.random.default_rng(N)
    for r in rng.permutation(N):
        if len(rows) >= min(64, N):
            break
        rows.add(int(r))
    return np.array(sorted(rows))


@functools.lru_cache(maxsize=4)
def device_R(N, key):
    return qfa.rotation_matrix(VECTORS[key], N)


@functools.lru_cache(maxsize=None)
def columns(N, xi):
    return tuple(c.astype(np.complex128) for c in extreme_columns(np.array(xi), N))


def skew_state(N, salt=51):
    return gen.skewherm(N, salt) / N


# ---- a: the Taylor kernel alone ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", (0.48, 1e-3))
@pytest.mark.parametrize("N", TAYLOR_SIZES)
def test_taylor_kernel_dense(N, target):
    xi = small_xi(N, target)
    sigma, d = geometry.exp_plan(xi, N)
    assert sigma == 0 and (d == 16 if target > 0.25 else 2 <= d <= 7), (sigma, d)
    R = qfa.rotation_matrix(xi, N)
    ref = taylor_reference(xi, N)
    err = float(np.abs(R - ref).max())
    where = np.unravel_index(np.argmax(np.abs(R - ref)), R.shape)
    print("worst entry %s, strip %d of %d" % (where, where[1] // 32, (N + 31) // 32), end="   ")
    report("Taylor start vs Horner, degree %d" % d, N, xi, err)
    r = np.arange(N)
    assert not np.any(R[np.abs(r[:, None] - r[None, :]) > d]), "an entry outside the band |r - j| <= %d is not zero" % d


# ---- b: rotation_matrix end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,key", EXP_CASES)
def test_rotation_matrix_large(N, key):
    xi = VECTORS[key]
    sigma, d = assert_squared_plan(xi, N)
    R = device_R(N, key) if (N in (1025, 2048) and key == "xi1") else qfa.rotation_matrix(xi, N)
    assert R.shape == (N, N) and R.dtype == np.complex128
    tag = "%s, %d squarings: " % (key, sigma)
    c0, c = columns(N, tuple(xi))
    report(tag + "column 0 vs closed form", N, xi, maxabs(R[:, 0], c0))
    report(tag + "column N-1 vs closed form", N, xi, maxabs(R[:, -1], c))
    report(tag + "R S_j - S'_j R", N, xi, equivariance_error(R, xi), N / 2)
    rows = row_sample(N)
    G = (R[rows].conj() @ R.T).conj()                  # R[I,:] R^H without a conjugated copy of R
    G[np.arange(len(rows)), rows] -= 1
    report(tag + "R[I,:] R^H - I[I,:]", N, xi, float(np.abs(G).max()))
    if key == "z":
        a = np.arange(N, dtype=LD) - LD(N - 1) / 2
        want = (np.cos(LD(xi[2]) * a) + 1j * np.sin(LD(xi[2]) * a)).astype(np.complex128)
        diag = R.diagonal().copy()
        R[np.arange(N), np.arange(N)] = 0                 # (R is this test's own copy)
        report(tag + "vs diag(exp(i xi3 (a-s)))", N, xi, max(maxabs(diag, want), float(np.abs(R).max())))


# ---- c: rotate, closed form ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,key", ROTATE_CASES)
def test_rotate_closed_form(N, key):
    xi = VECTORS[key]
    assert_squared_plan(xi, N)
    W, want = closed_form_case(xi, N)
    out = qfa.rotate(xi, W)
    assert out.dtype == np.complex128 and out is not W
    diff = np.abs(out - want)
    print("worst entry %s" % (np.unravel_index(np.argmax(diff), diff.shape),), end="   ")
    report("rotate(%s, closed-form W)" % key, N, xi, float(diff.max()), float(np.abs(want).max()))


# ---- d: rotate, dense data -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (1025, 2048))
def test_rotate_dense(N):
    """rotate(xi, W)[I, J] against R[I,:] W R[J,:]^H with the DEVICE's R, which test_rotation_matrix_large holds to the
    bar at this size and vector.  3 x the bar: R's own error enters twice (left and right factor), and the device's two
    products add theirs, which the bar's constant was made to cover once."""
    xi = VECTORS["xi1"]
    assert_squared_plan(xi, N)
    rng = np.random.default_rng(1000 + N)
    W = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    R = device_R(N, "xi1")
    out = qfa.rotate(xi, W)
    I = row_sample(N)
    ref = (R[I] @ W) @ R[I].conj().T
    report("rotate(xi1, Gaussian W)[I, I]", N, xi, maxabs(out[np.ix_(I, I)], ref), float(np.abs(out).max()), bar=24.0)
    if N == 1025:
        W32 = W.astype(np.complex64)
        out32 = qfa.rotate(xi, W32)
        assert out32.dtype == np.complex64
        err = maxabs(out32, out)
        bar32 = 2 * np.finfo(np.float32).eps * N * float(np.abs(W32).max())
        print("complex64 in and out vs complex128: max diff = %.3e  (bar %.3e)" % (err, bar32))
        assert err <= bar32


# ---- e: the resident state -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (1025, 2048))
def test_trajectory_rotate_bits(N):
    W0 = skew_state(N)
    xi = XIS[0]
    traj = qfa.DeviceTrajectory(W0)
    assert traj.rotate(xi) is traj
    Wr = traj.download()
    assert np.array_equal(Wr, qfa.rotate(xi, W0))
    if N == 1025:
        assert np.array_equal(traj.grad(), qfa.grad(Wr))


@pytest.mark.parametrize("N,after", ((1056, 2), (2048, 1)))
def test_trajectory_rotate_then_advance(N, after):
    """The carried-increment rule of tests/test_hip_geometry.py where the second product and the step end take other
    kernels: the 32 x 32 triangle path (1056) and the stream-K path (2048)."""
    dt = 0.25 * qfa.hbar(N)
    traj = qfa.DeviceTrajectory(skew_state(N))
    traj.advance(dt, 2)
    W1 = traj.download()
    traj.rotate(XIS[0])
    W1r = traj.download()
    assert np.array_equal(W1r, qfa.rotate(XIS[0], W1))
    s1 = traj.advance(dt, after)
    fresh = qfa.DeviceTrajectory(W1r)
    s2 = fresh.advance(dt, after)
    assert s1["total_iterations"] == s2["total_iterations"]
    assert np.array_equal(traj.download(), fresh.download())


# ---- f: grad against the host stencil ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (255, 256, 257, 511, 512, 513, 1025, 2049, 4096))
def test_grad_against_host_stencil(N):
    """Bar 8 eps N max|P| (tests/test_hip_geometry.py's test_grad_edges): four terms, each weighted by c <= N/2."""
    rng = np.random.default_rng(2000 + N)
    P = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    for (a, b), v in (((0, 0), 9 - 7j), ((N - 1, N - 1), -8 + 6j), ((7, 255), 7 + 9j), ((7, 256), -9 + 5j), ((8, 256), 6 - 8j)):
        if a < N and b < N:
            P[a, b] = v                     # outsized: a halo taken from the wrong row or side shows
    dP = qfa.grad(P)
    assert dP.shape == (3, N, N) and dP.dtype == np.complex128
    unit = EPS * N * float(np.abs(P).max())
    names = ["all", "first row", "last row", "first column", "last column"] + ["column %d" % b for b in (255, 256, 257) if b < N]

    def worst(i0, i1):
        diff = np.abs(dP[:, i0:i1] - grad_reference(P, i0, i1)).max(axis=0).astype(np.float64)
        found = {"all": diff.max(), "first row": diff[0].max() if i0 == 0 else 0.0, "last row": diff[-1].max() if i1 == N else 0.0,
                 "first column": diff[:, 0].max(), "last column": diff[:, -1].max()}
        found.update({"column %d" % b: diff[:, b].max() for b in (255, 256, 257) if b < N})
        return np.array([found[name] for name in names])
    regions = dict(zip(names, block_max(worst, N, 128)))
    print("grad vs host stencil N=%5d  err/(eps N max|P|), bar 8:  " % N
          + "  ".join("%s %.3f" % (k, v / unit) for k, v in regions.items()))
    for name, err in regions.items():
        assert err <= 8 * unit, (name, N, err / unit)


# ---- g: initial data at run sizes ----------------------------------------------------------------------------------------

BLOB_SIZES = (512, 1025, 2048)
NEAR_SOUTH = tuple(np.array((1e-9, 0.0, -1.0)) / np.linalg.norm((1e-9, 0.0, -1.0)))
BLOB_POSITIONS = tuple(gen.BLOB_POS) + (NEAR_SOUTH,)


def heat_diagonal(oracle, N):
    W = np.zeros((N, N), dtype=np.complex128)
    W[-1, -1] = 1.0j
    return np.array(oracle.solve_heat(0.1 / 4.0, W))


@pytest.mark.parametrize("N", BLOB_SIZES)
def test_north_blob_large(oracle, N):
    nb = qfa.north_blob(N, 0.1)
    assert nb.shape == (N, N) and nb.dtype == np.complex128
    assert np.count_nonzero(nb) == np.count_nonzero(nb.diagonal()), "north_blob has an entry off the diagonal"
    heat_tol = 16 * N * EPS * float(np.abs(nb).max())
    err = maxabs(nb, heat_diagonal(oracle, N))
    print("north_blob(%d, 0.1) vs oracle heat solve: max err = %.3e  (bar %.3e, max entry %.3e)" % (N, err, heat_tol, np.abs(nb).max()))
    assert err <= heat_tol


@pytest.mark.parametrize("N", BLOB_SIZES)
def test_point_blob_closed_form(N):
    """blob(N, pos, 0) = 1j c c^H with c the last column of exp(xi . S), xi = rotation_vector(pos)."""
    assert tuple(gen.BLOB_POS[2]) == (0.0, 0.0, -1.0)         # the half-turn branch of rotvec_from_matrix is among them
    for pos in BLOB_POSITIONS:
        xi = dynamics.rotation_vector(pos)
        if np.any(xi):
            assert_squared_plan(xi, N)
        c = columns(N, tuple(xi))[1]
        want = 1j * np.outer(c, c.conj())
        err = maxabs(qfa.blob(N, np.array(pos), 0), want)
        unit = N * max(1.0, float(np.linalg.norm(xi))) * EPS
        bar = rot_tol(N, xi) + 2 * N * EPS * np.linalg.norm(xi)
        print("blob(%d, %s, 0) vs 1j c c^H  |xi|=%.3f  max err = %.3e  err/(N max(1,|xi|) eps) = %.3f  (bar %.2f)"
              % (N, pos, np.linalg.norm(xi), err, err / unit, bar / unit))
        assert err <= bar


def test_smoothed_blob_sampled(oracle):
    """blob(1025, pos, 0.1)[I, I] against R[I,:] D R[I,:]^H with the device's R and the oracle's diagonal D: the bar of
    tests/test_hip_geometry.py's blob test, times 3 as for the dense rotate above."""
    N, pos = 1025, gen.BLOB_POS[0]
    xi = dynamics.rotation_vector(pos)
    assert_squared_plan(xi, N)
    D = heat_diagonal(oracle, N).diagonal()
    R = qfa.rotation_matrix(xi, N)
    # the blob sits on the rows where the last column of R does: the row sample, and 16 rows around that column's peak
    peak = int(np.argmax(np.abs(columns(N, tuple(xi))[1])))
    I = np.unique(np.concatenate((row_sample(N), np.clip(np.arange(peak - 8, peak + 8), 0, N - 1))))
    ref = (R[I] * D[None, :]) @ R[I].conj().T
    got = qfa.blob(N, np.array(pos), 0.1)[np.ix_(I, I)]
    heat_tol = 16 * N * EPS * float(np.abs(D).max())
    bar = 3 * ((rot_tol(N, xi) + 2 * N * EPS * np.linalg.norm(xi)) * float(np.abs(D).max()) + heat_tol)
    err = maxabs(got, ref)
    print("blob(%d, %s, 0.1)[I, I]: max err = %.3e  (bar %.3e, max entry %.3e, largest sampled %.3e)"
          % (N, pos, err, bar, np.abs(D).max(), np.abs(ref).max()))
    assert np.abs(ref).max() >= 1e6 * bar                     # the sample holds the blob, not only its far field
    assert err <= bar
