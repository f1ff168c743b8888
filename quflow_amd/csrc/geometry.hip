// Rotations and gradients on the sphere (quflow/geometry.py:132-207): the so(3) representation in u(N) is tridiagonal
// with closed-form entries, so no generator matrix is ever stored.  With s = (N-1)/2 and c_a = sqrt((a+1)(N-1-a)):
//     S3 = i diag(a - s),   S1[a,a+1] = S1[a+1,a] = i c_a / 2,   S2[a,a+1] = c_a / 2,  S2[a+1,a] = -c_a / 2
// (c_{-1} = c_{N-1} = 0: the matrix edge needs no special case in the stencils below).
//
// k_so3_taylor   T = p_d(B), B = (xi . S) / 2^sigma, p_d the degree-d Taylor polynomial of exp, as a dense N x N matrix in
//                ONE launch.  Column j of p_d(B) lives on the rows j-d .. j+d, so a workgroup that owns a strip of
//                QF_SO3_STRIP columns keeps only the (strip + 2d)-row window in LDS, runs the d Horner steps
//                T <- I + (B T) / k there and writes its columns once, zeros outside the window.  The host squares T
//                sigma times with the ordinary product (api_geometry.hip).
// k_so3_grad     the three commutators [S_k, P] in one pass over P: [S3,P]_ab = i (a-b) P_ab, [S1,.] and [S2,.] are
//                five-point stencils.  Replaces the reference's six dense products (geometry.py:197-207).
#include "qf_internal.h"

#include <cmath>

namespace {

#define QF_SO3_WINDOW (QF_SO3_STRIP + 2 * QF_SO3_MAX_DEGREE)
#define QF_SO3_ROWS_PER_THREAD ((QF_SO3_WINDOW + 7) / 8)

// c_a for 0 <= a <= N-2, zero elsewhere (also for rows of a window that hangs over the matrix edge)
__device__ __forceinline__ double so3_c(int a, int N)
{
    return (a >= 0 && a < N - 1) ? sqrt((double)(a + 1) * (double)(N - 1 - a)) : 0.0;
}

// alpha = xi1 / 2^(sigma+1), beta = xi2 / 2^(sigma+1), gamma = xi3 / 2^sigma:
//     B[r,r+1] = (beta + i alpha) c_r,   B[r,r-1] = (-beta + i alpha) c_{r-1},   B[r,r] = i gamma (r - s)
__global__ __launch_bounds__(256) void k_so3_taylor(int N, int d, double alpha, double beta, double gamma,
                                                    cplx *__restrict__ T)
{
    __shared__ cplx win[QF_SO3_WINDOW][QF_SO3_STRIP];
    __shared__ double cdn[QF_SO3_WINDOW], cup[QF_SO3_WINDOW], dg[QF_SO3_WINDOW];
    const int tx = threadIdx.x & (QF_SO3_STRIP - 1), ty = threadIdx.x / QF_SO3_STRIP;     // 32 columns x 8 row lanes
    const int j0 = blockIdx.x * QF_SO3_STRIP, j = j0 + tx;
    const int rows = QF_SO3_STRIP + 2 * d;      // window rows in use: matrix rows r0 .. r0 + rows - 1
    const int r0 = j0 - d;
    for (int w = threadIdx.x; w < rows; w += 256) {
        const int r = r0 + w;
        cdn[w] = so3_c(r - 1, N);
        cup[w] = so3_c(r, N);
        dg[w] = gamma * (0.5 * (double)(2 * r - N + 1));
    }
    // T = I restricted to the window (rows and columns past the matrix edge stay zero for ever: their c vanish)
    for (int w = ty; w < rows; w += 8) win[w][tx] = make_double2((r0 + w == j && j < N) ? 1.0 : 0.0, 0.0);
    __syncthreads();
    cplx next[QF_SO3_ROWS_PER_THREAD];
    for (int k = d; k >= 1; --k) {
        const double kk = (double)k;
#pragma unroll
        for (int i = 0; i < QF_SO3_ROWS_PER_THREAD; ++i) {
            const int w = ty + 8 * i;
            next[i] = make_double2(0.0, 0.0);
            if (w < rows) {
                const int r = r0 + w;
                const cplx zero = make_double2(0.0, 0.0);
                const cplx tm = w > 0 ? win[w - 1][tx] : zero, t0 = win[w][tx], tp = w + 1 < rows ? win[w + 1][tx] : zero;
                const double cm = cdn[w], cp = cup[w], g = dg[w];
                const double re = cm * (-beta * tm.x - alpha * tm.y) - g * t0.y + cp * (beta * tp.x - alpha * tp.y);
                const double im = cm * (alpha * tm.x - beta * tm.y) + g * t0.x + cp * (alpha * tp.x + beta * tp.y);
                const bool inside = r >= 0 && r < N && j < N;
                next[i] = make_double2(inside ? (r == j ? 1.0 : 0.0) + re / kk : 0.0, inside ? im / kk : 0.0);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < QF_SO3_ROWS_PER_THREAD; ++i) {
            const int w = ty + 8 * i;
            if (w < rows) win[w][tx] = next[i];
        }
        __syncthreads();
    }
    if (j >= N) return;
    for (int r = ty; r < N; r += 8) {
        const int w = r - r0;
        T[(size_t)r * N + j] = (w >= 0 && w < rows) ? win[w][tx] : make_double2(0.0, 0.0);
    }
}

// P[e] where `ok`, zero elsewhere (a value, not a choice between two addresses: that would put the zero into scratch)
__device__ __forceinline__ cplx so3_load(const cplx *__restrict__ P, size_t e, bool ok)
{
    cplx v = make_double2(0.0, 0.0);
    if (ok) v = P[e];
    return v;
}

// One workgroup: QF_GRAD_ROWS rows x 256 columns of P.  A thread walks down its column with the rows a-1, a, a+1 in
// registers; the row a goes through LDS (double-buffered, one barrier per row) with a one-entry halo on either side for
// the column neighbours.  out = (3, N, N).
#define QF_GRAD_ROWS 8
__global__ __launch_bounds__(256) void k_so3_grad(int N, const cplx *__restrict__ P, cplx *__restrict__ out)
{
    __shared__ cplx seg[2][258];
    const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid, a0 = blockIdx.y * QF_GRAD_ROWS;
    const bool col = b < N;
    const size_t NN = (size_t)N * N;
    const double cbm = so3_c(b - 1, N), cb = so3_c(b, N);
    cplx prev = so3_load(P, (size_t)(a0 - 1) * N + b, col && a0 > 0);
    cplx cur = so3_load(P, (size_t)a0 * N + b, col);          // (a0 < N by the launch geometry)
#pragma unroll
    for (int i = 0; i < QF_GRAD_ROWS; ++i) {
        const int a = a0 + i;
        if (a >= N) break;                                    // uniform over the workgroup
        const cplx next = so3_load(P, (size_t)(a + 1) * N + b, col && a + 1 < N);
        cplx *s = seg[i & 1];
        s[tid + 1] = cur;
        if (tid == 0) s[0] = so3_load(P, (size_t)a * N + b0 - 1, b0 > 0);
        if (tid == 255) s[257] = so3_load(P, (size_t)a * N + b0 + 256, b0 + 256 < N);
        __syncthreads();
        if (col) {
            const cplx left = s[tid], right = s[tid + 2];
            const double cam = so3_c(a - 1, N), ca = so3_c(a, N);
            // u = c_a P[a+1,b] + c_{a-1} P[a-1,b] - c_{b-1} P[a,b-1] - c_b P[a,b+1]:   [S1,P] = (i/2) u
            const double ux = ca * next.x + cam * prev.x - cbm * left.x - cb * right.x;
            const double uy = ca * next.y + cam * prev.y - cbm * left.y - cb * right.y;
            // v = c_a P[a+1,b] - c_{a-1} P[a-1,b] - c_{b-1} P[a,b-1] + c_b P[a,b+1]:   [S2,P] = v / 2
            const double vx = ca * next.x - cam * prev.x - cbm * left.x + cb * right.x;
            const double vy = ca * next.y - cam * prev.y - cbm * left.y + cb * right.y;
            const double m = (double)(a - b);
            const size_t e = (size_t)a * N + b;
            out[e] = make_double2(-0.5 * uy, 0.5 * ux);
            out[NN + e] = make_double2(0.5 * vx, 0.5 * vy);
            out[2 * NN + e] = make_double2(-m * cur.y, m * cur.x);
        }
        prev = cur;
        cur = next;
    }
}

}  // namespace

// The scaling rule (host only).  b0 = |B|_inf of B = xi . S from the closed forms; sigma = max(0, ceil(log2(b0 / 0.5)));
// b = b0 / 2^sigma <= 0.5; d = the smallest degree with b^d / d! < 1e-18 (the first dropped term bounds the tail to a
// factor 1 / (1 - b / (d+1)); d = 14..16 for b in (0.25, 0.5], d = 1 for xi = 0).
int qf_so3_plan(int N, const double xi[3], int *squarings, int *degree, double *b_scaled)
{
    if (N < 1 || !xi || !QF_FINITE(xi[0]) || !QF_FINITE(xi[1]) || !QF_FINITE(xi[2])) {
        qf_set_error("so3_exp: N = %d, the rotation vector must be three finite numbers", N);
        return QF_ERR_INVALID;
    }
    const double s = 0.5 * (double)(N - 1), off = 0.5 * std::sqrt(xi[0] * xi[0] + xi[1] * xi[1]), dia = std::fabs(xi[2]);
    double b0 = 0.0;
    for (int a = 0; a < N; ++a) {
        const double lo = a > 0 ? off * std::sqrt((double)a * (double)(N - a)) : 0.0;
        const double up = a < N - 1 ? off * std::sqrt((double)(a + 1) * (double)(N - 1 - a)) : 0.0;
        const double row = lo + dia * std::fabs((double)a - s) + up;
        if (row > b0) b0 = row;
    }
    if (!QF_FINITE(b0)) {
        qf_set_error("so3_exp: the rotation vector is too large (|xi . S|_inf overflows)");
        return QF_ERR_INVALID;
    }
    int sigma = 0;
    if (b0 > 0.5) sigma = (int)std::ceil(std::log2(b0 / 0.5));
    if (sigma < 0) sigma = 0;
    while (std::ldexp(b0, -sigma) > 0.5) ++sigma;             // (a log2 rounded down by an ulp at a power of two)
    if (sigma > 64) {
        qf_set_error("so3_exp: the rotation vector is too large (%d squarings)", sigma);
        return QF_ERR_INVALID;
    }
    const double b = std::ldexp(b0, -sigma);
    int d = 0;
    double term = 1.0;
    do {
        ++d;
        term *= b / (double)d;
    } while (term >= 1e-18);
    if (d > QF_SO3_MAX_DEGREE) {      // (cannot happen for b <= 0.5: d <= 16)
        qf_set_error("so3_exp: degree %d exceeds the kernel's window", d);
        return QF_ERR_INVALID;
    }
    if (squarings) *squarings = sigma;
    if (degree) *degree = d;
    if (b_scaled) *b_scaled = b;
    return QF_OK;
}

int qf_launch_so3_taylor(qf_ctx *ctx, const double xi[3], int squarings, int degree, cplx *T)
{
    const int N = ctx->N;
    if (degree < 1 || degree > QF_SO3_MAX_DEGREE || squarings < 0 || squarings > 64) {
        qf_set_error("so3_taylor: degree %d / %d squarings out of range", degree, squarings);
        return QF_ERR_INVALID;
    }
    const double alpha = std::ldexp(xi[0], -squarings - 1), beta = std::ldexp(xi[1], -squarings - 1);
    const double gamma = std::ldexp(xi[2], -squarings);
    hipLaunchKernelGGL(k_so3_taylor, dim3((N + QF_SO3_STRIP - 1) / QF_SO3_STRIP), dim3(256), 0, ctx->stream, N, degree, alpha,
                       beta, gamma, T);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_so3_grad(qf_ctx *ctx, const cplx *P, cplx *out)
{
    const int N = ctx->N;
    hipLaunchKernelGGL(k_so3_grad, dim3((N + 255) / 256, (N + QF_GRAD_ROWS - 1) / QF_GRAD_ROWS), dim3(256), 0, ctx->stream, N, P,
                       out);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
