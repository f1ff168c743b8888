// Spherical-harmonic SYNTHESIS onto the MW grid (shc2fun / shr2fun, quflow/transforms.py:220-268, 422-438): at bandwidth L
//     f(theta_t, phi_p) = sqrt(4 pi) sum_{l<L, |m|<=l} w_l a_lm Y_lm(theta_t, phi_p),
//     theta_t = pi (2t+1)/(2L-1) (t < L),   phi_p = 2 pi p/(2L-1) (p < 2L-1),   Y_lm = lambda_lm(theta) e^{i m phi}
// (orthonormal, Condon-Shortley phase; w_l the Berezin multiplier or 1).  The reference hands this to pyssht / ducc0; here it
// is three stages, all fp64:
//   k_sht_pack     : the coefficients become m-major columns (l contiguous) scaled by sqrt(4 pi) w_l -- from a real shr
//                    array the conversion shr2shc (transforms.py:310-349) happens here, with numpy's operations;
//   k_sht_legendre : G_m(t) = sum_{l>=m} a_lm lambda_lm(theta_t), one lane per ring, m uniform per workgroup (m and L-1-m
//                    share one, so every workgroup walks L+1 degrees).  The normalised three-term recurrence in l
//                        lambda_lm = A_lm (x lambda_{l-1,m} - B_lm lambda_{l-2,m}),  x = cos theta,
//                        A_lm = sqrt((4l^2-1)/(l^2-m^2)),  B_lm = sqrt(((l-1)^2-m^2)/(4(l-1)^2-1)),
//                    starts from lambda_mm = c_m sin^m theta, which underflows fp64 long before it is negligible (m = 8000 at
//                    the first ring: ~1e-30000).  Every lane therefore carries its value as a mantissa p and a scale k <= 0,
//                    lambda = p 2^(600 k), as libsharp and ducc0 do: the seed is formed with an integer exponent, a mantissa
//                    that grows past 2^200 while k < 0 is multiplied by 2^-600 and k advances, and a term enters the sums
//                    once k >= -1 (k = -1: p 2^-600 is exact in fp64; k <= -2: |lambda| < 2^-1000, below 1e-300).  A_lm,
//                    B_lm and the coefficients are uniform across the workgroup and come from LDS in chunks of 256 degrees;
//   k_sht_fourier  : f[t, p] = sum_k At[k, t] T[k, p], a real GEMM (L or 2L rows, K = 2L, 2L-1 columns) on
//                    v_mfma_f64_16x16x4_f64 with guarded edge tiles.  T[2m, p] = cos(2 pi m p/(2L-1)), T[2m+1, p] = -sin(...)
//                    is never stored (2 GB at L = 8192): each tile of it is gathered from a table of 2L-1 twiddles at the
//                    exact integer reduction (m p) mod (2L-1).
// The length 2L-1 of a ring is odd with large prime factors (2047 = 23 * 89), so the ring transform is this GEMM and not an
// FFT; k_zgemm does not fit either (square N x N complex operands with the stepper's fused epilogues).
//
// Real synthesis (isreal: a real map, the m >= 0 half of the coefficients; Im a_l0 takes no part):
//     At[2m] = w_m Re G_m,  At[2m+1] = w_m Im G_m,  w_0 = 1, w_m = 2.
// Complex synthesis: G+_m from a_lm, G-_m from (-1)^m a_l,-m (lambda_l,-m = (-1)^m lambda_lm), f = sum G+ e^{im phi} + G- e^{-im phi}:
//     rows t      (Re f):  At[2m] = Re G+ + Re G-,   At[2m+1] = Im G+ - Im G-
//     rows L + t  (Im f):  At[2m] = Im G+ + Im G-,   At[2m+1] = Re G- - Re G+
// No kernel here uses scratch memory; every buffer is ctx->sht, sized by qf_sht_sizes.
#include "qf_internal.h"

namespace {

constexpr int SHT_RINGS = 256;    // lanes (rings) per workgroup of the Legendre stage
constexpr int SHT_CHUNK = 256;    // degrees staged through LDS at a time
constexpr int SHT_ESTEP = 600;    // lambda = p 2^(SHT_ESTEP k)
constexpr int SHT_EHIGH = 200;    // while k < 0, a mantissa above 2^SHT_EHIGH is rescaled
constexpr int SHT_BM = 64, SHT_BN = 64, SHT_BK = 16;   // Fourier-stage tile

__host__ __device__ __forceinline__ size_t col_offset(int m, int L) { return (size_t)m * L - (size_t)m * (m - 1) / 2; }
__host__ __device__ __forceinline__ int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---- coefficients -> m-major columns.  SHR: omega is a real shr array, converted as shr2shc does (m > 0:
// (1/sqrt 2) (-1)^m (omega[l,m] + i omega[l,-m]); m = 0: omega[l,0]) -- the same operations as numpy's, so that a complex
// array made by shr2shc packs to the same bits.  NEG: also the columns (-1)^m a_l,-m of the complex synthesis.
// Entries at or past n are zero (the reference pads omega to L^2).
template <bool SHR, bool NEG>
__global__ __launch_bounds__(256) void k_sht_pack(int L, long long n, const double *__restrict__ omega,
                                                  const double *__restrict__ scale, cplx *__restrict__ colp,
                                                  cplx *__restrict__ coln)
{
    const int m = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L - m) return;
    const long long l = m + j;
    const long long ip = l * l + l + m, im = l * l + l - m;
    const size_t o = col_offset(m, L) + j;
    const double s = scale[l];
    const cplx *oc = reinterpret_cast<const cplx *>(omega);
    cplx a;
    if (SHR) {
        const double xp = ip < n ? omega[ip] : 0.0;
        if (m == 0) {
            a = make_double2(xp, 0.0);
        } else {
            const double xm = im < n ? omega[im] : 0.0;
            const double c = (1.0 / sqrt(2.0)) * ((m & 1) ? -1.0 : 1.0);
            a = make_double2(c * xp, c * xm);
        }
    } else {
        a = ip < n ? oc[ip] : make_double2(0.0, 0.0);
    }
    colp[o] = make_double2(a.x * s, a.y * s);
    if (NEG) {
        const cplx b = (m > 0 && im < n) ? oc[im] : make_double2(0.0, 0.0);
        const double sg = (m & 1) ? -1.0 : 1.0;
        coln[o] = make_double2((sg * b.x) * s, (sg * b.y) * s);
    }
}

// ---- 2L-1 twiddles (cos, sin)(2 pi k/(2L-1)), the argument reduced to (-1, 1] half-turns
__global__ __launch_bounds__(256) void k_sht_twiddle(int P, double2 *__restrict__ tw)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P) return;
    const int j = 2 * k > P ? k - P : k;
    double s, c;
    sincospi(2.0 * (double)j / (double)P, &s, &c);
    tw[k] = make_double2(c, s);
}

__device__ __forceinline__ double sht_factor(int k) { return k == 0 ? 1.0 : (k == -1 ? 0x1p-600 : 0.0); }

// ---- Legendre stage: workgroup (ring block, y) handles m = y and m = L-1-y; seed[m] = lambda_mm / sin^m (sign included).
template <bool CPLX>
__global__ __launch_bounds__(SHT_RINGS) void k_sht_legendre(int L, const double *__restrict__ seed,
                                                            const cplx *__restrict__ colp, const cplx *__restrict__ coln,
                                                            double *__restrict__ At, int ldA)
{
    __shared__ double2 rec[SHT_CHUNK];
    __shared__ cplx cp[SHT_CHUNK];
    __shared__ cplx cn[CPLX ? SHT_CHUNK : 1];
    const int tid = threadIdx.x;
    const int t = blockIdx.x * SHT_RINGS + tid;
    const bool ring = t < L;
    const int tt = ring ? t : L - 1;          // lanes past the last ring compute a copy of it and store nothing
    double sn, x;
    sincospi((double)(2 * tt + 1) / (double)(2 * L - 1), &sn, &x);
    int se;
    const double sm = frexp(sn, &se);         // sin theta = sm 2^se, sm in [0.5, 1) (0 at the south pole)
    const int y = blockIdx.y;
    for (int half = 0; half < 2; ++half) {
        const int m = half == 0 ? y : L - 1 - y;
        if (half == 1 && m <= y) break;
        // sin^m theta = r 2^re by binary powering, renormalised at every product
        double r = 1.0, b = sm;
        int re = 0, be = se;
        for (int e = m; e != 0; e >>= 1) {
            int d;
            if (e & 1) {
                r = frexp(r * b, &d);
                re += be + d;
            }
            if (e > 1) {
                b = frexp(b * b, &d);
                be = 2 * be + d;
            }
        }
        // scale k <= 0 with re - 600 k in (-400, 200]: C's division truncates, i.e. rounds a negative quotient up.  While
        // k < 0 the mantissa stays at or below 2^200, so k <= -2 means |lambda| <= 2^-1000
        int k = re - SHT_EHIGH < 0 ? (re - SHT_EHIGH) / SHT_ESTEP : 0;
        double p1 = seed[m] * ldexp(r, re - SHT_ESTEP * k), p2 = 0.0;
        if (k < 0 && fabs(p1) > 0x1p200) {      // (|seed[m]| > 1 can lift it past 2^200: the recurrence's rule holds here too)
            p1 *= 0x1p-600;
            ++k;
        }
        double fac = sht_factor(k);
        double gr = 0.0, gi = 0.0, hr = 0.0, hi = 0.0;
        const cplx *cpm = colp + col_offset(m, L);
        const cplx *cnm = CPLX ? coln + col_offset(m, L) : nullptr;
        for (int l0 = m; l0 < L; l0 += SHT_CHUNK) {
            const int n = min(SHT_CHUNK, L - l0);
            __syncthreads();
            if (tid < n) {
                const int l = l0 + tid;
                double a = 0.0, bb = 0.0;
                if (l > m) {
                    const double dl = l, dm = m, dl1 = l - 1;
                    a = sqrt((4.0 * dl * dl - 1.0) / ((dl - dm) * (dl + dm)));
                    bb = sqrt(((dl1 - dm) * (dl1 + dm)) / (4.0 * dl1 * dl1 - 1.0));
                }
                rec[tid] = make_double2(a, bb);
                cp[tid] = cpm[l - m];
                if (CPLX) cn[tid] = cnm[l - m];
            }
            __syncthreads();
            int i0 = 0;
            if (l0 == m) {            // degree m: the seed itself
                const double v = p1 * fac;
                gr += cp[0].x * v;
                gi += cp[0].y * v;
                if (CPLX) {
                    hr += cn[0].x * v;
                    hi += cn[0].y * v;
                }
                i0 = 1;
            }
            for (int i = i0; i < n; ++i) {
                const double2 ab = rec[i];
                const double p = ab.x * (x * p1 - ab.y * p2);
                p2 = p1;
                p1 = p;
                if (k < 0 && fabs(p) > 0x1p200) {
                    p1 *= 0x1p-600;
                    p2 *= 0x1p-600;
                    ++k;
                    fac = sht_factor(k);
                }
                const double v = p1 * fac;
                const cplx c = cp[i];
                gr += c.x * v;
                gi += c.y * v;
                if (CPLX) {
                    const cplx d = cn[i];
                    hr += d.x * v;
                    hi += d.y * v;
                }
            }
        }
        if (ring) {
            double *c0 = At + (size_t)(2 * m) * ldA, *c1 = c0 + ldA;
            if (!CPLX) {
                const double w = m == 0 ? 1.0 : 2.0;
                c0[t] = w * gr;
                c1[t] = m == 0 ? 0.0 : w * gi;
            } else {
                c0[t] = gr + hr;
                c1[t] = m == 0 ? 0.0 : gi - hi;
                c0[L + t] = gi + hi;
                c1[L + t] = m == 0 ? 0.0 : hr - gr;
            }
        }
    }
}

// ---- Fourier stage: C (M x P) = At^T (M x K) T (K x P), 64 x 64 tile per workgroup, each wave a 32 x 32 quarter
// (2 x 2 MFMA blocks).  At is [K][ldA] (ldA a multiple of 64, K of 16: every load is in bounds); T is gathered per
// K-step into LDS.  Rows < L of the result are the real part, rows L..2L-1 (complex synthesis) the imaginary part.
typedef double qf_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_sht_fourier(int L, int M, int K, const double *__restrict__ At, int ldA,
                                                     const double2 *__restrict__ tw, double *__restrict__ f, int cplx_out)
{
    __shared__ double As[SHT_BK][SHT_BM];
    __shared__ double Bs[SHT_BK][SHT_BN];
    const unsigned P = 2u * L - 1u;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r16 = lane & 15, q4 = lane >> 4;
    const int row0 = blockIdx.y * SHT_BM, col0 = blockIdx.x * SHT_BN;
    qf_d4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = qf_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += SHT_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + 256 * r, kk = idx >> 6, c = idx & 63;
            As[kk][c] = At[(size_t)(k0 + kk) * ldA + row0 + c];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = tid + 256 * r, mm = idx >> 6, c = idx & 63;
            const unsigned m = (unsigned)(k0 >> 1) + mm, p = (unsigned)(col0 + c);
            double cs = 0.0, sn = 0.0;
            if (m < (unsigned)L && p < P) {
                const double2 w = tw[(m * p) % P];
                cs = w.x;
                sn = -w.y;
            }
            Bs[2 * mm][c] = cs;
            Bs[2 * mm + 1][c] = sn;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SHT_BK / 4; ++s) {
            double a[2], b[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = As[4 * s + q4][wm * 32 + mi * 16 + r16];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) b[ni] = Bs[4 * s + q4][wn * 32 + ni * 16 + r16];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }
    // D of v_mfma_f64_16x16x4_f64: lane holds rows q4 + 4 reg, column r16
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = row0 + wm * 32 + mi * 16 + q4 + 4 * reg;
                const unsigned col = (unsigned)(col0 + wn * 32 + ni * 16 + r16);
                if (row >= M || col >= P) continue;
                const double v = acc[mi][ni][reg];
                if (!cplx_out) f[(size_t)row * P + col] = v;
                else if (row < L) f[2 * ((size_t)row * P + col)] = v;
                else f[2 * ((size_t)(row - L) * P + col) + 1] = v;
            }
}

// Fourier-stage operand shape for (L, isreal)
void sht_shape(int L, int isreal, int *M, int *K, int *ldA)
{
    *M = isreal ? L : 2 * L;
    *K = round_up(2 * L, SHT_BK);
    *ldA = round_up(*M, SHT_BM);
}

}  // namespace

void qf_sht_sizes(int L, int isreal, size_t bytes[6])
{
    int M, K, ldA;
    sht_shape(L, isreal, &M, &K, &ldA);
    const size_t LL = (size_t)L * L, P = 2 * (size_t)L - 1, half = (size_t)L * (L + 1) / 2;
    bytes[0] = LL * sizeof(cplx);                              // omega (complex at most)
    bytes[1] = 2 * (size_t)L * sizeof(double);                 // tab
    bytes[2] = (isreal ? 1 : 2) * half * sizeof(cplx);         // col
    bytes[3] = (size_t)K * ldA * sizeof(double);               // At
    bytes[4] = P * sizeof(double2);                            // tw
    bytes[5] = (size_t)L * P * (isreal ? sizeof(double) : sizeof(cplx));   // f
}

int qf_launch_sht_synth(qf_ctx *ctx, int L, int shr, int isreal, const double *omega_dev, long long n_valid)
{
    qf_sht &S = ctx->sht;
    int M, K, ldA;
    sht_shape(L, isreal, &M, &K, &ldA);
    const int P = 2 * L - 1;
    cplx *colp = S.col, *coln = isreal ? nullptr : S.col + (size_t)L * (L + 1) / 2;
    const dim3 gp((L + 255) / 256, L);
    if (shr)
        hipLaunchKernelGGL((k_sht_pack<true, false>), gp, dim3(256), 0, ctx->stream, L, n_valid, omega_dev, S.tab, colp, coln);
    else if (isreal)
        hipLaunchKernelGGL((k_sht_pack<false, false>), gp, dim3(256), 0, ctx->stream, L, n_valid, omega_dev, S.tab, colp, coln);
    else
        hipLaunchKernelGGL((k_sht_pack<false, true>), gp, dim3(256), 0, ctx->stream, L, n_valid, omega_dev, S.tab, colp, coln);
    QF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sht_twiddle, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, P, S.tw);
    QF_HIP(hipGetLastError());
    // rows 2L..K-1 of At meet zero twiddles; zeroed so that nothing stale (a NaN of an earlier call) enters the sums
    if (K > 2 * L) QF_HIP(hipMemsetAsync(S.At + (size_t)2 * L * ldA, 0, (size_t)(K - 2 * L) * ldA * sizeof(double), ctx->stream));
    const dim3 gl((L + SHT_RINGS - 1) / SHT_RINGS, (L + 1) / 2);
    if (isreal)
        hipLaunchKernelGGL(k_sht_legendre<false>, gl, dim3(SHT_RINGS), 0, ctx->stream, L, S.tab + L, colp, coln, S.At, ldA);
    else
        hipLaunchKernelGGL(k_sht_legendre<true>, gl, dim3(SHT_RINGS), 0, ctx->stream, L, S.tab + L, colp, coln, S.At, ldA);
    QF_HIP(hipGetLastError());
    const dim3 gf((P + SHT_BN - 1) / SHT_BN, ldA / SHT_BM);
    hipLaunchKernelGGL(k_sht_fourier, gf, dim3(256), 0, ctx->stream, L, M, K, S.At, ldA, S.tw, S.f, isreal ? 0 : 1);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
