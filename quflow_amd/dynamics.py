"""Helpers that make initial data and move it around the sphere (quflow/dynamics.py:87-124, 244-304): `north_blob`,
`blob`, `project_el`.  The time loop of that module (`dynamics.solve`) is `quflow_amd.solve` here.

`project_el` DEVIATES from the reference on purpose.  The reference's routine scales its basis columns to squared norm N,
not 1, so it returns N times the orthogonal projection onto the degree-el eigenspace -- it is not idempotent, and with
`complement=True` it returns W - N P_el W.  Here `project_el` IS the projection P_el W = shc2mat(mask * mat2shc(W)), built on
the device transforms, so that `complement=True` gives W - P_el W; N * project_el(W, el) reproduces the reference's output.
"""
import numpy as np

from .geometry import rotate
from .laplacian import solve_heat
from .quantization import mat2shc, shc2mat


def north_blob(N, sigma=0):
    """Vorticity matrix of a blob at the north pole (quflow/dynamics.py:282-304): the point-vortex approximation
    i E_{N-1,N-1}, smoothed by one heat solve with h nu = sigma / 4 when sigma != 0."""
    W = np.zeros((N, N), dtype=np.complex128)
    W[-1, -1] = 1.0j
    if sigma != 0:
        W = solve_heat(sigma / 4.0, W)
    return W


def _frame(pos):
    """The proper rotation q whose LAST column points along `pos` (it takes the north pole there), by a QR factorisation
    of [pos, 0, 0] as the reference makes it (quflow/dynamics.py:259-267)."""
    pos = np.asarray(pos, dtype=np.float64)
    if pos.shape != (3,):
        raise ValueError("pos must have shape (3,), got %s" % (pos.shape,))
    a = np.zeros((3, 3))
    a[:, 0] = pos
    q, _ = np.linalg.qr(a)
    if np.dot(q[:, 0], pos) < 0:
        q[:, 0] = -q[:, 0]
    if np.linalg.det(q) < 0:
        q[:, -1] = -q[:, -1]
    return np.roll(q, 2, axis=-1)


def rotvec_from_matrix(q):
    """The rotation vector theta * n of a 3 x 3 rotation matrix (its matrix logarithm, written out; what
    scipy.spatial.transform.Rotation.from_matrix(q).as_rotvec() returns).  Away from a half turn n comes from the
    skew part q - q^T = 2 sin(theta) [n]_x; near one (cos(theta) < -0.9), where that part vanishes, from the symmetric
    part (q + q^T) / 2 = cos(theta) I + (1 - cos(theta)) n n^T, with the sign the skew part still shows."""
    q = np.asarray(q, dtype=np.float64)
    v = np.array([q[2, 1] - q[1, 2], q[0, 2] - q[2, 0], q[1, 0] - q[0, 1]])
    sin_t = 0.5 * np.linalg.norm(v)
    cos_t = 0.5 * (np.trace(q) - 1.0)
    theta = np.arctan2(sin_t, cos_t)
    if cos_t >= -0.9:
        if sin_t == 0.0:
            return np.zeros(3)
        return v * (0.5 * theta / sin_t)
    M = 0.5 * (q + q.T) - cos_t * np.eye(3)
    n = M[:, np.argmax(np.diag(M))]
    n = n / np.linalg.norm(n)
    if np.dot(n, v) < 0:
        n = -n
    return theta * n


def rotation_vector(pos):
    """The axis-angle vector xi of the rotation that `blob` applies to the north blob to put it at `pos`."""
    return rotvec_from_matrix(_frame(pos))


def blob(N, pos=np.array([0.0, 0.0, 1.0]), sigma=0, device=None):
    """Vorticity matrix of a blob at `pos` (quflow/dynamics.py:244-279): the north blob, rotated on the device.  numpy
    only: no scipy is needed for the rotation vector."""
    return rotate(rotation_vector(pos), north_blob(N, sigma), device=device)


def project_el(W, el=1, complement=False):
    """Orthogonal projection of W onto the eigenspace of the Laplacian for degree `el` -- an int or a list of ints, a
    negative one counting from N -- or, with `complement=True`, onto its orthogonal complement: W - P_el W.

    Unlike quflow/dynamics.py:87-124, which returns N TIMES this projection (module docstring): multiply by N for the
    reference's numbers.  Runs on the device transforms at every N they accept."""
    W = np.asarray(W)
    N = W.shape[-1]
    ells = [el] if np.isscalar(el) else list(el)
    keep = np.zeros(N * N, dtype=np.float64)
    for e in ells:
        e = int(e)
        if e < 0:
            e += N
        if not 0 <= e < N:
            raise ValueError("el = %d is outside 0..%d" % (e, N - 1))
        keep[e * e:(e + 1) * (e + 1)] = 1.0
    if complement:
        keep = 1.0 - keep
    out = shc2mat(keep * mat2shc(W), N)
    return out.astype(W.dtype, copy=False) if W.dtype == np.complex64 else out
