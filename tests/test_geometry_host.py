"""Host side of quflow_amd.geometry / dynamics (no GPU): the so(3) generators against the reference's, their commutation
relations, the scaling rule of the device matrix exponential (qf_so3_exp_plan is host code) and the rotation vector that
`blob` derives from a position.

Shared with tests/test_hip_geometry.py: the fixture, its inputs (tools/gen_geometry_golden.py rebuilds them from integer
hashes), the Rodrigues matrix and the tolerance of the rotation
    entrywise error <= 8 N max(1, |xi|) eps max|entry|
-- squaring amplifies the rounding of the Taylor start by 2^sigma ~ N |xi|; a numpy model of the algorithm stays below 0.9
in units of N |xi| eps, 8 leaves the device's product kernels their own summation order.
"""
import importlib.util
import math
import os

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import dynamics, geometry
from conftest import REPO, load_golden

EPS = np.finfo(np.float64).eps

_spec = importlib.util.spec_from_file_location("gen_geometry_golden", os.path.join(REPO, "tools", "gen_geometry_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)          # (imports the reference only inside main())

XIS = tuple(np.array(xi) for xi in gen.XIS)
FIXTURE_SIZES = gen.SIZES


@pytest.fixture(scope="module")
def golden():
    return load_golden("geometry")


def rot_tol(N, xi, scale=1.0):
    return 8.0 * N * max(1.0, float(np.linalg.norm(xi))) * EPS * scale


def rodrigues(xi):
    """The 3 x 3 rotation matrix exp([xi]_x)."""
    xi = np.asarray(xi, dtype=np.float64)
    theta = np.linalg.norm(xi)
    if theta == 0:
        return np.eye(3)
    n = xi / theta
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def plan_model(N, xi):
    """(sigma, d, b0) by the rule of include/quflow_hip.h, from the closed forms -- not from the library."""
    a = np.arange(N, dtype=np.float64)
    s = (N - 1) / 2
    off = 0.5 * np.sqrt(xi[0] * xi[0] + xi[1] * xi[1])
    lo = off * np.sqrt(a * (N - a))                      # |B[a,a-1]| = off c_{a-1}; 0 at a = 0
    up = off * np.sqrt((a + 1) * (N - 1 - a))            # |B[a,a+1]| = off c_a;     0 at a = N-1
    b0 = float((lo + abs(xi[2]) * np.abs(a - s) + up).max())
    sigma = max(0, math.ceil(math.log2(b0 / 0.5))) if b0 > 0 else 0
    b = b0 / 2.0 ** sigma
    d = 1
    while b ** d / math.factorial(d) >= 1e-18:
        d += 1
    return sigma, d, b0


# ---- generators ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_generators_against_reference(golden, N):
    for name, mine in (("so3", qfa.so3_generators(N)), ("cartesian", qfa.cartesian_generators(N))):
        ref = golden["%s_%d" % (name, N)]
        assert len(mine) == 3
        for k in range(3):
            assert mine[k].dtype == np.complex128 and mine[k].shape == (N, N)
            # to 1 ulp of each part (the reference takes sqrt(s(s+1) - m(m+1)), here sqrt((a+1)(N-1-a)): the same number)
            for part in (np.real, np.imag):
                assert np.all(np.abs(part(mine[k]) - part(ref[k])) <= np.spacing(np.abs(part(ref[k])))), (name, k)


def test_generators_dtype():
    S = qfa.so3_generators(8, dtype=np.complex64)
    assert all(s.dtype == np.complex64 for s in S)


@pytest.mark.parametrize("N", [15, 16, 64, 128])
def test_so3_commutation_relations(N):
    S1, S2, S3 = qfa.so3_generators(N)
    np.testing.assert_allclose(S1 @ S2 - S2 @ S1, S3, atol=1e-14)
    np.testing.assert_allclose(S2 @ S3 - S3 @ S2, S1, atol=1e-14)
    np.testing.assert_allclose(S3 @ S1 - S1 @ S3, S2, atol=1e-14)
    for S in (S1, S2, S3):
        assert np.array_equal(S, -S.conj().T)


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_equivariance_convention_on_the_reference(golden, N):
    """R S_j R^H = sum_i Q_ij S_i with Q the Rodrigues matrix of xi, for the REFERENCE's expm(xi . S): the identity the GPU
    tests use needs no device to be pinned."""
    S = qfa.so3_generators(N)
    for i, xi in enumerate(XIS):
        R = golden["expm_%d_%d" % (i, N)]
        Q = rodrigues(xi)
        for j in range(3):
            want = sum(Q[k, j] * S[k] for k in range(3))
            assert np.abs(R @ S[j] @ R.conj().T - want).max() <= rot_tol(N, xi, np.abs(S[j]).max())


# ---- the scaling rule ------------------------------------------------------------------------------------------------

def test_plan_zero_vector():
    for N in (2, 5, 33, 1024):
        assert geometry.exp_plan(np.zeros(3), N) == (0, 1)


@pytest.mark.parametrize("N", [5, 33, 1024])
def test_plan_follows_the_rule(N):
    for xi in XIS:
        sigma, d, b0 = plan_model(N, xi)
        assert geometry.exp_plan(xi, N) == (sigma, d), (N, xi)
        assert b0 / 2.0 ** sigma <= 0.5
        assert 1 <= d <= 16


def test_plan_scaled_norm_is_at_most_half():
    rng = np.random.default_rng(5)
    for N in (2, 3, 5, 16, 33, 64, 257, 1024, 4096, 8192):
        for scale in (1e-9, 1e-3, 0.5, 1.0, 3.0, 40.0):
            xi = scale * rng.standard_normal(3)
            sigma, d = geometry.exp_plan(xi, N)
            b = plan_model(N, xi)[2] / 2.0 ** sigma
            assert b <= 0.5 and (sigma == 0 or b > 0.25 * (1 - 4 * EPS)), (N, xi, sigma, b)
            assert b ** d / math.factorial(d) < 1e-18 * (1 + 64 * EPS)
            assert d == 1 or b ** (d - 1) / math.factorial(d - 1) >= 1e-18 * (1 - 64 * EPS)
    # powers of two on the diagonal: b0 / 0.5 is an exact power of two, the ceiling must not step over it
    assert geometry.exp_plan([0.0, 0.0, 1.0], 3) == (1, plan_model(3, [0.0, 0.0, 1.0])[1])
    assert geometry.exp_plan([0.0, 0.0, 0.5], 3)[0] == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_plan_rejects_nonfinite(bad):
    for k in range(3):
        xi = np.array([0.1, 0.2, 0.3])
        xi[k] = bad
        with pytest.raises(qfa.QuflowHipError, match="INVALID"):
            geometry.exp_plan(xi, 16)
    with pytest.raises(ValueError):
        geometry.exp_plan([0.1, 0.2], 16)


# ---- blob's rotation vector ------------------------------------------------------------------------------------------

def test_rotation_vector_against_scipy():
    R = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(11)
    for _ in range(10):
        pos = rng.standard_normal(3)
        pos /= np.linalg.norm(pos)
        q = dynamics._frame(pos)
        assert abs(np.linalg.det(q) - 1) <= 8 * EPS and np.abs(q[:, 2] - pos).max() <= 8 * EPS
        want = R.from_matrix(q).as_rotvec()
        got = dynamics.rotation_vector(pos)
        assert np.abs(got - want).max() <= 16 * EPS * max(1.0, np.linalg.norm(want)), (pos, got, want)
        assert np.abs(rodrigues(got) - q).max() <= 16 * EPS


def test_rotation_vector_special_positions():
    assert np.abs(rodrigues(dynamics.rotation_vector([0.0, 0.0, 1.0]))[:, 2] - [0, 0, 1]).max() <= 8 * EPS
    south = dynamics.rotation_vector([0.0, 0.0, -1.0])          # a half turn: the symmetric-part branch
    assert abs(np.linalg.norm(south) - np.pi) <= 8 * EPS
    assert np.abs(rodrigues(south)[:, 2] - [0, 0, -1]).max() <= 8 * EPS
    near = np.array([1e-9, 0.0, -1.0])
    near /= np.linalg.norm(near)
    assert np.abs(rodrigues(dynamics.rotation_vector(near))[:, 2] - near).max() <= 16 * EPS
    assert np.array_equal(dynamics.rotvec_from_matrix(np.eye(3)), np.zeros(3))


def test_argument_checks_need_no_device():
    with pytest.raises(ValueError):
        qfa.rotate([0.1, 0.2], np.zeros((4, 4), dtype=complex))
    with pytest.raises(ValueError):
        qfa.rotate([0.1, 0.2, 0.3], np.zeros((4, 5), dtype=complex))
    with pytest.raises(ValueError):
        qfa.grad(np.zeros((3, 4, 4), dtype=complex))
    with pytest.raises(ValueError):
        dynamics.rotation_vector([1.0, 0.0])
