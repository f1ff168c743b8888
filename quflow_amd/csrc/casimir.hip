// Casimirs of a state on the device: C_k = Re tr((iW)^k) / N for k <= 8 (qf_casimirs and its kin, include/quflow_hip.h).
// The powers A_j = W^j, j <= p = ceil(kmax / 2), come from at most three plain products (qf_launch_zgemm) into the
// per-iteration staging matrices; every trace is then a pair sum tr(W^(i+j)) = sum_ab (A_i)_ab (A_j)_ba with
// i = floor(k / 2), j = k - i, and ONE kernel (k_power_traces) forms all of them in one pass over the stored powers.
#include <cmath>

#include "qf_api.h"

#pragma clang fp contract(off)  // the compensation terms below are rounding errors: no product may fuse into a sum

namespace {

constexpr int CT = 32;              // tile of k_power_traces
constexpr int CAS_MAX_SUMS = 12;    // 8 Casimir sums + 4 cross sums
constexpr int CAS_MAX_BLOCKS = 1024;

struct cas_mats {
    const cplx *M[5];               // A_1 .. A_P, then (MHD) the matrix V of the cross sums tr(V A_k)
};

// (s, c) += t: the sum with the rounding error of the addition kept in c (Knuth's two-sum, any magnitudes)
__device__ __forceinline__ void cas_add(double &s, double &c, double t)
{
    const double n = s + t;
    const double b = n - s;
    c += (s - (n - b)) + (t - b);
    s = n;
}
// (s, c) += (s2, c2), the same through a reduction tree
__device__ __forceinline__ void cas_join(double &s, double &c, double s2, double c2)
{
    const double n = s + s2;
    const double b = n - s;
    c = (c + c2) + ((s - (n - b)) + (s2 - b));
    s = n;
}
__device__ __forceinline__ void cas_wave_join(double &s, double &c)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double s2 = __shfl_xor(s, off), c2 = __shfl_xor(c, off);
        cas_join(s, c, s2, c2);
    }
}
// the component of a b that survives the phase: Im for an odd power of i in front of the trace, Re for an even one
template <bool IM> __device__ __forceinline__ double cas_part(const cplx a, const cplx b)
{
    return IM ? a.x * b.y + a.y * b.x : a.x * b.x - a.y * b.y;
}

// Raw sums of the stored powers A_1 .. A_P (P <= 4), one real number each:
//   sum k - 1, k = 1 .. 2P:        Im (k odd) or Re (k even) of tr(A_1^k) = sum_ab (A_i)_ab (A_j)_ba, i = k / 2, j = k - i
//                                  (k = 1: the diagonal of A_1)
//   sum 2P + k - 1, k = 1 .. P:    (MHD) Re (k odd) or Im (k even) of tr(V A_k) = sum_ab V_ab (A_k)_ba
// A workgroup owns tile pairs (I, J), (J, I) with I <= J, `gridDim.x` apart: thread (r, c) of a pair holds x_q = A_q[I0 + r,
// J0 + c] from a row-coalesced 16-byte load and y_q = A_q[J0 + c, I0 + r] through a padded LDS tile that was filled by
// row-coalesced 16-byte loads of tile (J, I) (two tiles alternate, so one barrier per matrix).  Its terms of a pair sum are
// x_i y_j and, off the diagonal, y_i x_j.  Entries past the edge of the matrix are read as zeros.  Every thread keeps a
// compensation term per sum, the wavefront butterfly and the four waves' join carry it on, and the block's (sum,
// compensation) pairs go to partial[(2 q + {0, 1}) * CAS_MAX_BLOCKS + block]: k_power_traces_fold adds them in fixed order.
// No atomics anywhere: two launches give the same bits.
template <int P, bool MHD>
__global__ __launch_bounds__(256) void k_power_traces(int N, int nt, int npairs, cas_mats mats, double *__restrict__ partial)
{
    constexpr int NM = P + (MHD ? 1 : 0);
    constexpr int NS = 2 * P + (MHD ? P : 0);
    __shared__ cplx Ts[2][CT][CT + 1];
    __shared__ double part[4][NS][2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    double acc[NS], cmp[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = cmp[q] = 0.0;
    int buf = 0;
    for (int t = blockIdx.x; t < npairs; t += gridDim.x) {
        // t = I nt - I (I - 1) / 2 + (J - I)
        int I = (int)(((double)(2 * nt + 1) - sqrt((double)(2 * nt + 1) * (double)(2 * nt + 1) - 8.0 * (double)t)) * 0.5);
        if (I < 0) I = 0;
        if (I > nt - 1) I = nt - 1;
        while (I > 0 && I * nt - I * (I - 1) / 2 > t) --I;
        while (I + 1 < nt && (I + 1) * nt - (I + 1) * I / 2 <= t) ++I;
        const int J = I + (t - (I * nt - I * (I - 1) / 2));
        const int i0 = I * CT, j0 = J * CT;
        const bool off = I != J;
        cplx x[NM][4], y[NM][4];
#pragma unroll
        for (int q = 0; q < NM; ++q) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int r = ty + 8 * s;
                x[q][s] = make_double2(0.0, 0.0);
                y[q][s] = make_double2(0.0, 0.0);
                if (i0 + r < N && j0 + tx < N) x[q][s] = mats.M[q][(size_t)(i0 + r) * N + j0 + tx];
                if (j0 + r < N && i0 + tx < N) y[q][s] = mats.M[q][(size_t)(j0 + r) * N + i0 + tx];
            }
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) {
#pragma unroll
            for (int s = 0; s < 4; ++s) Ts[buf][ty + 8 * s][tx] = y[q][s];
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 4; ++s) y[q][s] = Ts[buf][tx][ty + 8 * s];      // A_q[j0 + tx, i0 + r]
            buf ^= 1;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (!off && tx == ty + 8 * s) cas_add(acc[0], cmp[0], x[0][s].y);     // k = 1: Im of the diagonal
#pragma unroll
            for (int k = 2; k <= 2 * P; ++k) {
                const int i = k / 2 - 1, j = k - k / 2 - 1;
                if (k & 1) {
                    cas_add(acc[k - 1], cmp[k - 1], cas_part<true>(x[i][s], y[j][s]));
                    if (off) cas_add(acc[k - 1], cmp[k - 1], cas_part<true>(y[i][s], x[j][s]));
                } else {
                    cas_add(acc[k - 1], cmp[k - 1], cas_part<false>(x[i][s], y[j][s]));
                    if (off) cas_add(acc[k - 1], cmp[k - 1], cas_part<false>(y[i][s], x[j][s]));
                }
            }
            if (MHD) {
#pragma unroll
                for (int k = 1; k <= P; ++k) {
                    const int q = 2 * P + k - 1;
                    if (k & 1) {
                        cas_add(acc[q], cmp[q], cas_part<false>(x[NM - 1][s], y[k - 1][s]));
                        if (off) cas_add(acc[q], cmp[q], cas_part<false>(y[NM - 1][s], x[k - 1][s]));
                    } else {
                        cas_add(acc[q], cmp[q], cas_part<true>(x[NM - 1][s], y[k - 1][s]));
                        if (off) cas_add(acc[q], cmp[q], cas_part<true>(y[NM - 1][s], x[k - 1][s]));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        cas_wave_join(acc[q], cmp[q]);
        if ((threadIdx.x & 63) == 0) {
            part[threadIdx.x >> 6][q][0] = acc[q];
            part[threadIdx.x >> 6][q][1] = cmp[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int q = threadIdx.x;
        double s = part[0][q][0], c = part[0][q][1];
        for (int w = 1; w < 4; ++w) cas_join(s, c, part[w][q][0], part[w][q][1]);
        partial[(size_t)(2 * q) * CAS_MAX_BLOCKS + blockIdx.x] = s;
        partial[(size_t)(2 * q + 1) * CAS_MAX_BLOCKS + blockIdx.x] = c;
    }
}

// out[q] = the blocks' (sum, compensation) pairs of sum q joined in fixed order -- lane l takes the blocks l, l + 64, ..
// ascending, then the butterfly -- and the compensation added in at the very end.  One workgroup of one wavefront.
__global__ __launch_bounds__(64) void k_power_traces_fold(int nblocks, int nsums, const double *__restrict__ partial,
                                                           double *__restrict__ out)
{
    for (int q = 0; q < nsums; ++q) {
        double s = 0.0, c = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += 64)
            cas_join(s, c, partial[(size_t)(2 * q) * CAS_MAX_BLOCKS + b], partial[(size_t)(2 * q + 1) * CAS_MAX_BLOCKS + b]);
        cas_wave_join(s, c);
        if (threadIdx.x == 0) out[q] = s + c;
    }
}

// complex64 -> complex128, exact
__global__ __launch_bounds__(256) void k_widen_c64(size_t n, const float2 *__restrict__ X, cplx *__restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float2 v = X[e];
        out[e] = make_double2((double)v.x, (double)v.y);
    }
}

template <int P, bool MHD> void launch_traces(qf_ctx *ctx, int grid, int nt, int npairs, const cas_mats &mats, double *partial)
{
    hipLaunchKernelGGL((k_power_traces<P, MHD>), dim3(grid), dim3(256), 0, ctx->stream, ctx->N, nt, npairs, mats, partial);
}

// The raw sums of k_power_traces for the P stored powers in `mats`, folded (ctx->cas_ev[2] behind the two launches), on
// their way to ctx->host_scalars[0 .. nsums)
int launch_power_traces(qf_ctx *ctx, int P, bool mhd, const cas_mats &mats)
{
    const int nt = (ctx->N + CT - 1) / CT;
    const int npairs = nt * (nt + 1) / 2;
    const int grid = npairs < CAS_MAX_BLOCKS ? npairs : CAS_MAX_BLOCKS;
    const int nsums = 2 * P + (mhd ? P : 0);
    double *partial = ctx->cas_part, *out = ctx->cas_part + (size_t)2 * CAS_MAX_SUMS * CAS_MAX_BLOCKS;
    switch (P * 2 + (mhd ? 1 : 0)) {
    case 2: launch_traces<1, false>(ctx, grid, nt, npairs, mats, partial); break;
    case 3: launch_traces<1, true>(ctx, grid, nt, npairs, mats, partial); break;
    case 4: launch_traces<2, false>(ctx, grid, nt, npairs, mats, partial); break;
    case 5: launch_traces<2, true>(ctx, grid, nt, npairs, mats, partial); break;
    case 6: launch_traces<3, false>(ctx, grid, nt, npairs, mats, partial); break;
    case 7: launch_traces<3, true>(ctx, grid, nt, npairs, mats, partial); break;
    case 8: launch_traces<4, false>(ctx, grid, nt, npairs, mats, partial); break;
    case 9: launch_traces<4, true>(ctx, grid, nt, npairs, mats, partial); break;
    default: qf_set_error("launch_power_traces: %d stored powers", P); return QF_ERR_INVALID;
    }
    QF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_power_traces_fold, dim3(1), dim3(64), 0, ctx->stream, grid, nsums, partial, out);
    QF_HIP(hipGetLastError());
    QF_HIP(hipEventRecord(ctx->cas_ev[2], ctx->stream));
    QF_HIP(hipMemcpyAsync(ctx->host_scalars, out, (size_t)nsums * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return QF_OK;
}

int check_kmax(const char *who, int kmax, const void *out)
{
    if (kmax < 1 || kmax > 8) {
        qf_set_error("%s: kmax=%d outside 1..8", who, kmax);
        return QF_ERR_INVALID;
    }
    if (!out) {
        qf_set_error("%s: null output", who);
        return QF_ERR_INVALID;
    }
    return QF_OK;
}

// Re(i^m z) from the one component of z the kernel kept (Im for odd m, Re for even m), divided by N
double phase_over_n(int m, double raw, int N)
{
    const double v = ((m & 3) == 1 || (m & 3) == 2) ? -raw : raw;      // i z, -z, -i z, z: real parts -Im, -Re, Im, Re
    return v / (double)N;
}

// C_k(A), k <= kmax, into out; with V: also Re tr((iV)(iA)^k) / N, k <= p, into cross.  A and V are device matrices that no
// staging matrix overlays (A may be ctx->stage); the powers go to Whalf, Phalf, PW.
int casimirs_run(qf_ctx *ctx, const char *who, const cplx *A, const cplx *V, int kmax, double *out, double *cross)
{
    const int N = ctx->N, p = (kmax + 1) / 2;
    if (!ctx->cas_part)
        QF_HIP(hipMalloc((void **)&ctx->cas_part, (size_t)(2 * CAS_MAX_SUMS * CAS_MAX_BLOCKS + 16) * sizeof(double)));
    for (hipEvent_t &e : ctx->cas_ev)
        if (!e) QF_HIP(hipEventCreate(&e));
    ctx->cas_timed = false;
    QF_HIP(hipEventRecord(ctx->cas_ev[0], ctx->stream));
    if (p >= 2) QF_TRY(qf_launch_zgemm(ctx, A, A, ctx->Whalf, nullptr));                   // A_2 = A A
    if (p >= 3) QF_TRY(qf_launch_zgemm(ctx, ctx->Whalf, A, ctx->Phalf, nullptr));          // A_3 = A_2 A
    if (p >= 4) QF_TRY(qf_launch_zgemm(ctx, ctx->Whalf, ctx->Whalf, ctx->PW, nullptr));    // A_4 = A_2 A_2
    QF_HIP(hipEventRecord(ctx->cas_ev[1], ctx->stream));
    cas_mats mats;
    mats.M[0] = A;
    mats.M[1] = ctx->Whalf;
    mats.M[2] = ctx->Phalf;
    mats.M[3] = ctx->PW;
    mats.M[4] = nullptr;
    mats.M[p] = V;
    QF_TRY(launch_power_traces(ctx, p, V != nullptr, mats));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->cas_timed = true;
    const double *raw = ctx->host_scalars;
    bool finite = true;
    for (int k = 1; k <= kmax; ++k) finite = finite && QF_FINITE(raw[k - 1]);
    for (int k = 1; V && k <= p; ++k) finite = finite && QF_FINITE(raw[2 * p + k - 1]);
    if (!finite) {
        qf_set_error("%s: a trace is inf or NaN", who);
        return QF_ERR_NONFINITE;
    }
    for (int k = 1; k <= kmax; ++k) out[k - 1] = phase_over_n(k, raw[k - 1], N);
    for (int k = 1; V && k <= p; ++k) cross[k - 1] = phase_over_n(k + 1, raw[2 * p + k - 1], N);
    return QF_OK;
}

}  // namespace

extern "C" {

int qf_casimirs(qf_ctx *ctx, const void *W_host, int kmax, double *out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_kmax("qf_casimirs", kmax, out));
    if (!W_host) {
        if (!ctx->w_c128_set) {
            qf_set_error("qf_casimirs: no complex128 state is resident on this context (qf_upload_W; pass W_host, or "
                         "qf_c64_casimirs for a complex64 state)");
            return QF_ERR_STATE;
        }
        return casimirs_run(ctx, "qf_casimirs", ctx->W, nullptr, kmax, out, nullptr);
    }
    QF_HIP(hipMemcpyAsync(ctx->stage, W_host, (size_t)ctx->N * ctx->N * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    return casimirs_run(ctx, "qf_casimirs", ctx->stage, nullptr, kmax, out, nullptr);
}

int qf_c64_casimirs(qf_ctx *ctx, int kmax, double *out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_kmax("qf_c64_casimirs", kmax, out));
    if (!ctx->c64 || !ctx->c64->w_set) {
        qf_set_error("qf_c64_casimirs: no complex64 state is resident on this context (qf_c64_upload_W)");
        return QF_ERR_STATE;
    }
    const size_t n = (size_t)ctx->N * ctx->N;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_widen_c64, dim3(blocks), dim3(256), 0, ctx->stream, n, ctx->c64->W, ctx->stage);
    QF_HIP(hipGetLastError());
    return casimirs_run(ctx, "qf_c64_casimirs", ctx->stage, nullptr, kmax, out, nullptr);
}

int qf_states_casimirs(qf_ctx *ctx, int j, int kmax, double *out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_kmax("qf_states_casimirs", kmax, out));
    if (ctx->stack_k < 1) {
        qf_set_error("qf_states_casimirs: no stack is resident (qf_states_upload; a host-in / host-out qf_isomp_states call discards it)");
        return QF_ERR_STATE;
    }
    if (j < 0 || j >= ctx->stack_k) {
        qf_set_error("qf_states_casimirs: member %d of a stack of %d", j, ctx->stack_k);
        return QF_ERR_INVALID;
    }
    return casimirs_run(ctx, "qf_states_casimirs", ctx->stack[5 * j], nullptr, kmax, out, nullptr);
}

int qf_mhd_casimirs(qf_ctx *ctx, int kmax, double *magnetic, double *cross)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_kmax("qf_mhd_casimirs", kmax, magnetic));
    if (!cross) {
        qf_set_error("qf_mhd_casimirs: null output");
        return QF_ERR_INVALID;
    }
    if (ctx->stack_k < 1) {
        qf_set_error("qf_mhd_casimirs: no stack is resident (qf_states_upload; a host-in / host-out qf_isomp_states call discards it)");
        return QF_ERR_STATE;
    }
    if (ctx->stack_k != 2) {
        qf_set_error("qf_mhd_casimirs: the resident stack must be the pair (W, Theta) (k=%d)", ctx->stack_k);
        return QF_ERR_INVALID;
    }
    return casimirs_run(ctx, "qf_mhd_casimirs", ctx->stack[5], ctx->stack[0], kmax, magnetic, cross);
}

int qf_casimirs_times(qf_ctx *ctx, double *products_ms, double *traces_ms)
{
    QF_TRY(check_ctx(ctx));
    if (!ctx->cas_timed) {
        qf_set_error("qf_casimirs_times: no completed Casimir call on this context");
        return QF_ERR_STATE;
    }
    float a = 0.f, b = 0.f;
    QF_HIP(hipEventElapsedTime(&a, ctx->cas_ev[0], ctx->cas_ev[1]));
    QF_HIP(hipEventElapsedTime(&b, ctx->cas_ev[1], ctx->cas_ev[2]));
    if (products_ms) *products_ms = (double)a;
    if (traces_ms) *traces_ms = (double)b;
    return QF_OK;
}

}  // extern "C"
