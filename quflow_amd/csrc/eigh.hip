// Hermitian eigendecomposition H = V diag(lambda) V^H on the device: parallel one-sided (Hestenes) Jacobi on the shifted
// matrix A = H + c I, c = 2 |H|_inf, which is positive definite with condition number <= 3.
//
// The work matrix G starts as A and its ROWS are the vectors that get rotated (a row is contiguous; because A is
// Hermitian its rows are the columns of conj(A), so rotating rows runs the column algorithm on conj(A)).  A rotation makes
// two rows orthogonal; when all are, row j is sigma_j v_j^H with (sigma_j, v_j) an eigenpair of A: the normalised G IS V^H,
// no rotations are accumulated, and lambda_j = sigma_j - c.  The host (api_eigh.hip) drives the sweeps, refines every
// eigenvalue by its Rayleigh quotient with the unshifted H and sorts.
//
// A round is one launch over the ceil(n/2) disjoint pairs of a round-robin tournament of n = N + (N & 1) players, one
// 256-thread workgroup per pair, the pairing computed from (round, block).  Every reduction is a fixed tree -- xor
// butterfly inside a wave, the four wave results through LDS, summed in one order by every thread -- and the only
// atomics are an integer max (the bit pattern of a non-negative double orders as the double does) and an integer add:
// two calls return the same bits.
//
// Size classes: N <= 2048 keeps both rows in registers (QF_EIGH_EPT complex per thread and row) between the reductions
// and the rotation; above that the rows are read twice (the second read comes from L2).
#include "qf_internal.h"

#define QF_EIGH_EPT 8
#define QF_EIGH_REG_MAX_N (256 * QF_EIGH_EPT)

namespace {

__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the four sums of a pair, in every thread: part[] is 4 x 4 doubles of LDS
__device__ __forceinline__ void block_sum4(double &a, double &b, double &cr, double &ci, double *part)
{
    a = wave_sum64(a);
    b = wave_sum64(b);
    cr = wave_sum64(cr);
    ci = wave_sum64(ci);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[w * 4 + 0] = a;
        part[w * 4 + 1] = b;
        part[w * 4 + 2] = cr;
        part[w * 4 + 3] = ci;
    }
    __syncthreads();
    a = (part[0] + part[4]) + (part[8] + part[12]);
    b = (part[1] + part[5]) + (part[9] + part[13]);
    cr = (part[2] + part[6]) + (part[10] + part[14]);
    ci = (part[3] + part[7]) + (part[11] + part[15]);
}

__device__ __forceinline__ void accumulate(const cplx x, const cplx y, double &a, double &b, double &cr, double &ci)
{
    a += x.x * x.x + x.y * x.y;
    b += y.x * y.x + y.y * y.y;
    cr += x.x * y.x + x.y * y.y;      // conj(x) y
    ci += x.x * y.y - x.y * y.x;
}

// the rotation that makes rows p and q orthogonal: x' = cs x - sn conj(ph) y, y' = sn ph x + cs y, ph = c / |c|
struct rot {
    double cs, sr, si;      // sn ph = sr + i si
};
__device__ __forceinline__ void rotate(const rot r, cplx &x, cplx &y)
{
    const cplx x0 = x, y0 = y;
    //  conj(sn ph) y = (sr - i si)(y.x + i y.y)
    x.x = r.cs * x0.x - (r.sr * y0.x + r.si * y0.y);
    x.y = r.cs * x0.y - (r.sr * y0.y - r.si * y0.x);
    y.x = r.cs * y0.x + (r.sr * x0.x - r.si * x0.y);
    y.y = r.cs * y0.y + (r.sr * x0.y + r.si * x0.x);
}

// One round.  word[0]: the sweep's worst |c| / sqrt(a b) as the bits of a double; word[1]: rotations applied.
template <bool REG>
__global__ __launch_bounds__(256) void k_eigh_round(int N, int round, cplx *__restrict__ G, double tol,
                                                    unsigned long long *__restrict__ word)
{
    __shared__ double part[16];
    const int m = N + (N & 1) - 1, k = blockIdx.x;
    int p = k == 0 ? round : (round + k) % m;
    int q = k == 0 ? m : (round - k + m) % m;
    if (p > q) {
        const int t = p;
        p = q;
        q = t;
    }
    if (q >= N) return;            // the padding player of an odd N: its partner idles (uniform over the workgroup)
    cplx *gp = G + (size_t)p * N, *gq = G + (size_t)q * N;
    cplx x[REG ? QF_EIGH_EPT : 1], y[REG ? QF_EIGH_EPT : 1];
    double a = 0.0, b = 0.0, cr = 0.0, ci = 0.0;
    if (REG) {
#pragma unroll
        for (int e = 0; e < QF_EIGH_EPT; ++e) {
            const int j = threadIdx.x + 256 * e;
            x[e] = y[e] = make_double2(0.0, 0.0);
            if (j < N) {
                x[e] = gp[j];
                y[e] = gq[j];
            }
            accumulate(x[e], y[e], a, b, cr, ci);
        }
    } else {
        for (int j = threadIdx.x; j < N; j += 256) accumulate(gp[j], gq[j], a, b, cr, ci);
    }
    block_sum4(a, b, cr, ci, part);
    const double ab = a * b, cabs = sqrt(cr * cr + ci * ci);
    // (a, b > 0 for a positive definite A; anything else -- an overflow, a NaN -- rotates nothing and shows in the measure)
    const double ratio = ab > 0.0 ? cabs / sqrt(ab) : (ab == 0.0 && cabs == 0.0 ? 0.0 : __builtin_inf());
    const bool go = ratio > tol && ratio < __builtin_inf();
    if (threadIdx.x == 0) {
        atomicMax(word, (unsigned long long)__double_as_longlong(ratio == ratio ? ratio : __builtin_inf()));
        if (go) atomicAdd(word + 1, 1ull);
    }
    if (!go) return;
    const double zeta = (b - a) / (2.0 * cabs);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    rot r;
    r.cs = 1.0 / sqrt(1.0 + t * t);
    const double sn = r.cs * t;
    r.sr = sn * (cr / cabs);
    r.si = sn * (ci / cabs);
    if (REG) {
#pragma unroll
        for (int e = 0; e < QF_EIGH_EPT; ++e) {
            const int j = threadIdx.x + 256 * e;
            if (j < N) {
                rotate(r, x[e], y[e]);
                gp[j] = x[e];
                gq[j] = y[e];
            }
        }
    } else {
        for (int j = threadIdx.x; j < N; j += 256) {      // (every element is read and written by one thread only)
            cplx u = gp[j], v = gq[j];
            rotate(r, u, v);
            gp[j] = u;
            gq[j] = v;
        }
    }
}

// sig[j] = |row j|, row j /= sig[j]: one workgroup per row
__global__ __launch_bounds__(256) void k_eigh_normalise(int N, cplx *__restrict__ G, double *__restrict__ sig)
{
    __shared__ double part[16];
    cplx *g = G + (size_t)blockIdx.x * N;
    double a = 0.0, b = 0.0, cr = 0.0, ci = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) {
        const cplx x = g[j];
        a += x.x * x.x + x.y * x.y;
    }
    block_sum4(a, b, cr, ci, part);
    const double s = sqrt(a);
    if (threadIdx.x == 0) sig[blockIdx.x] = s;
    if (!(s > 0.0)) return;
    for (int j = threadIdx.x; j < N; j += 256) {
        const cplx x = g[j];
        g[j] = make_double2(x.x / s, x.y / s);
    }
}

// out[j] = sum_k T[j,k] conj(U[j,k]): one workgroup per row (Rayleigh quotients; diag(V^H W V))
__global__ __launch_bounds__(256) void k_eigh_rowdot(int N, const cplx *__restrict__ T, const cplx *__restrict__ U,
                                                     cplx *__restrict__ out)
{
    __shared__ double part[16];
    const cplx *t = T + (size_t)blockIdx.x * N, *u = U + (size_t)blockIdx.x * N;
    double a = 0.0, b = 0.0, cr = 0.0, ci = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) {
        const cplx x = u[j], y = t[j];
        cr += x.x * y.x + x.y * y.y;      // conj(u) t
        ci += x.x * y.y - x.y * y.x;
    }
    block_sum4(a, b, cr, ci, part);
    if (threadIdx.x == 0) out[blockIdx.x] = make_double2(cr, ci);
}

// out[k, j] = conj(U[perm ? perm[j] : j, k]) * (scale ? scale[j] : 1): V from V^H, its columns sorted and / or scaled
// (32 x 32 tiles through LDS, both global accesses row-coalesced)
__global__ __launch_bounds__(256) void k_eigh_conj_transpose(int N, const cplx *__restrict__ U, const int *__restrict__ perm,
                                                             const cplx *__restrict__ scale, cplx *__restrict__ out)
{
    __shared__ cplx Ts[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, kk = k0 + tx;
        cplx v = make_double2(0.0, 0.0);
        if (j < N && kk < N) {
            const cplx u = U[(size_t)(perm ? perm[j] : j) * N + kk];
            v = make_double2(u.x, -u.y);
            if (scale) {
                const cplx s = scale[j];
                v = make_double2(u.x * s.x + u.y * s.y, u.x * s.y - u.y * s.x);
            }
        }
        Ts[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int kk = k0 + r, j = j0 + tx;
        if (kk < N && j < N) out[(size_t)kk * N + j] = Ts[tx][r];
    }
}

// out = -i X (the Hermitian matrix of a skew-Hermitian one), or out = I (X == nullptr)
__global__ __launch_bounds__(256) void k_eigh_neg_i(int N, const cplx *X, cplx *out)
{
    const size_t n = (size_t)N * N;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        if (X) {
            const cplx x = X[e];
            out[e] = make_double2(x.y, -x.x);
        } else {
            out[e] = make_double2(e % ((size_t)N + 1) == 0 ? 1.0 : 0.0, 0.0);
        }
    }
}

int flat_blocks(int N)
{
    const size_t n = (size_t)N * N;
    const size_t blocks = (n + 255) / 256;
    return (int)(blocks > 4096 ? 4096 : blocks);
}

}  // namespace

int qf_launch_eigh_round(qf_ctx *ctx, cplx *G, int round, double tol, unsigned long long *word)
{
    const int N = ctx->N, pairs = (N + (N & 1)) / 2;
    if (N <= QF_EIGH_REG_MAX_N)
        hipLaunchKernelGGL(k_eigh_round<true>, dim3(pairs), dim3(256), 0, ctx->stream, N, round, G, tol, word);
    else
        hipLaunchKernelGGL(k_eigh_round<false>, dim3(pairs), dim3(256), 0, ctx->stream, N, round, G, tol, word);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_eigh_normalise(qf_ctx *ctx, cplx *G, double *sig)
{
    hipLaunchKernelGGL(k_eigh_normalise, dim3(ctx->N), dim3(256), 0, ctx->stream, ctx->N, G, sig);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_eigh_rowdot(qf_ctx *ctx, const cplx *T, const cplx *U, cplx *out)
{
    hipLaunchKernelGGL(k_eigh_rowdot, dim3(ctx->N), dim3(256), 0, ctx->stream, ctx->N, T, U, out);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_eigh_conj_transpose(qf_ctx *ctx, const cplx *U, const int *perm, const cplx *scale, cplx *out)
{
    const int tiles = (ctx->N + 31) / 32;
    hipLaunchKernelGGL(k_eigh_conj_transpose, dim3(tiles, tiles), dim3(256), 0, ctx->stream, ctx->N, U, perm, scale, out);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_eigh_neg_i(qf_ctx *ctx, const cplx *X, cplx *out)
{
    hipLaunchKernelGGL(k_eigh_neg_i, dim3(flat_blocks(ctx->N)), dim3(256), 0, ctx->stream, ctx->N, X, out);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
