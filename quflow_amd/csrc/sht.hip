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
// The ANALYSIS (fun2shc / fun2shr) is the second half of this file.
// No kernel here uses scratch memory; every buffer is ctx->sht, sized by qf_sht_sizes / qf_sht_analysis_sizes.
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

// ---- the recurrence, shared by the Legendre stages of the synthesis and of the analysis
// a ring: x = cos theta, sin theta = sm 2^se with sm in [0.5, 1) (0 at the south pole)
struct sht_ring {
    double x, sm;
    int se;
};

__device__ __forceinline__ sht_ring sht_ring_of(int tt, int L)
{
    sht_ring g;
    double sn;
    sincospi((double)(2 * tt + 1) / (double)(2 * L - 1), &sn, &g.x);
    g.sm = frexp(sn, &g.se);
    return g;
}

// lambda_mm at the ring as mantissa p1 and scale k <= 0 (lambda_mm = p1 2^(600 k)); seedm = lambda_mm / sin^m
__device__ __forceinline__ void sht_seed(int m, double seedm, const sht_ring &g, double &p1, int &k)
{
    // sin^m theta = r 2^re by binary powering, renormalised at every product
    double r = 1.0, b = g.sm;
    int re = 0, be = g.se;
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
    k = re - SHT_EHIGH < 0 ? (re - SHT_EHIGH) / SHT_ESTEP : 0;
    p1 = seedm * ldexp(r, re - SHT_ESTEP * k);
    if (k < 0 && fabs(p1) > 0x1p200) {      // (|seed[m]| > 1 can lift it past 2^200: the recurrence's rule holds here too)
        p1 *= 0x1p-600;
        ++k;
    }
}

// (A_lm, B_lm) of the recurrence; (0, 0) at l = m
__device__ __forceinline__ double2 sht_ab(int l, int m)
{
    double a = 0.0, bb = 0.0;
    if (l > m) {
        const double dl = l, dm = m, dl1 = l - 1;
        a = sqrt((4.0 * dl * dl - 1.0) / ((dl - dm) * (dl + dm)));
        bb = sqrt(((dl1 - dm) * (dl1 + dm)) / (4.0 * dl1 * dl1 - 1.0));
    }
    return make_double2(a, bb);
}

// one degree up: returns lambda_lm as it enters a sum (0 while k <= -2)
__device__ __forceinline__ double sht_step(double2 ab, double x, double &p1, double &p2, int &k, double &fac)
{
    const double p = ab.x * (x * p1 - ab.y * p2);
    p2 = p1;
    p1 = p;
    if (k < 0 && fabs(p) > 0x1p200) {
        p1 *= 0x1p-600;
        p2 *= 0x1p-600;
        ++k;
        fac = sht_factor(k);
    }
    return p1 * fac;
}

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
    const sht_ring g = sht_ring_of(tt, L);
    const double x = g.x;
    const int y = blockIdx.y;
    for (int half = 0; half < 2; ++half) {
        const int m = half == 0 ? y : L - 1 - y;
        if (half == 1 && m <= y) break;
        int k;
        double p1, p2 = 0.0;
        sht_seed(m, seed[m], g, p1, k);
        double fac = sht_factor(k);
        double gr = 0.0, gi = 0.0, hr = 0.0, hi = 0.0;
        const cplx *cpm = colp + col_offset(m, L);
        const cplx *cnm = CPLX ? coln + col_offset(m, L) : nullptr;
        for (int l0 = m; l0 < L; l0 += SHT_CHUNK) {
            const int n = min(SHT_CHUNK, L - l0);
            __syncthreads();
            if (tid < n) {
                const int l = l0 + tid;
                rec[tid] = sht_ab(l, m);
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
                const double v = sht_step(rec[i], x, p1, p2, k, fac);
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

// =====================================================================================================================
// STACKED REAL SYNTHESIS (qf_state_fields): F <= 4 real fields of one bandwidth L from ONE real coefficient vector -- the
// reference's 'fun' / 'funL2' / 'funhalf' / 'funL2half' outputs differ by the per-degree multiplier w_l and by how many
// leading coefficients they keep, nothing else.  The recurrence lambda_lm(theta_t) is walked once per (ring, m) for all F
// fields and the Fourier stage gathers each twiddle tile once for M = F L rows.  Every field is formed by the operations of
// k_sht_pack<true, false>, k_sht_legendre<false> and k_sht_fourier in their order (the statements below are those kernels'
// statements, repeated per field; a row of the Fourier stage meets the same K-steps whatever its row index), so a field
// has the bits of qf_shr2fun of the same coefficients.  Layout: scale [F][L], col [F][L(L+1)/2], At [K][ldA] with field f
// in the columns f L .. f L + L - 1 (ldA = round_up(F L, 64)), the grids in F slots of L (2L-1) doubles each.
// =====================================================================================================================
struct sht_field_lengths {
    long long n[4];            // field f keeps the coefficients below n[f]; the rest count as zero
};

template <int F>
__global__ __launch_bounds__(256) void k_sht_pack_fields(int L, sht_field_lengths len, const double *__restrict__ omega,
                                                         const double *__restrict__ scale, cplx *__restrict__ col)
{
    const int m = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L - m) return;
    const long long l = m + j;
    const long long ip = l * l + l + m, im = l * l + l - m;
    const size_t o = col_offset(m, L) + j, half = (size_t)L * (L + 1) / 2;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const long long n = len.n[f];
        const double s = scale[(size_t)f * L + l];
        cplx a;
        const double xp = ip < n ? omega[ip] : 0.0;
        if (m == 0) {
            a = make_double2(xp, 0.0);
        } else {
            const double xm = im < n ? omega[im] : 0.0;
            const double c = (1.0 / sqrt(2.0)) * ((m & 1) ? -1.0 : 1.0);
            a = make_double2(c * xp, c * xm);
        }
        col[f * half + o] = make_double2(a.x * s, a.y * s);
    }
}

template <int F>
__global__ __launch_bounds__(SHT_RINGS) void k_sht_legendre_fields(int L, const double *__restrict__ seed,
                                                                   const cplx *__restrict__ col, double *__restrict__ At, int ldA)
{
    __shared__ double2 rec[SHT_CHUNK];
    __shared__ cplx cp[F][SHT_CHUNK];
    const int tid = threadIdx.x;
    const int t = blockIdx.x * SHT_RINGS + tid;
    const bool ring = t < L;
    const int tt = ring ? t : L - 1;          // lanes past the last ring compute a copy of it and store nothing
    const sht_ring g = sht_ring_of(tt, L);
    const double x = g.x;
    const int y = blockIdx.y;
    const size_t half = (size_t)L * (L + 1) / 2;
    for (int hf = 0; hf < 2; ++hf) {
        const int m = hf == 0 ? y : L - 1 - y;
        if (hf == 1 && m <= y) break;
        int k;
        double p1, p2 = 0.0;
        sht_seed(m, seed[m], g, p1, k);
        double fac = sht_factor(k);
        // the sums are k_sht_legendre<false>'s `g += c * v`, which the compiler contracts to one fused multiply-add: written
        // as fma() here, so that a field keeps those bits whatever a compiler decides about contraction in this kernel
        double gr[F], gi[F];
#pragma unroll
        for (int f = 0; f < F; ++f) gr[f] = gi[f] = 0.0;
        const cplx *cpm = col + col_offset(m, L);
        for (int l0 = m; l0 < L; l0 += SHT_CHUNK) {
            const int n = min(SHT_CHUNK, L - l0);
            __syncthreads();
            if (tid < n) {
                const int l = l0 + tid;
                rec[tid] = sht_ab(l, m);
#pragma unroll
                for (int f = 0; f < F; ++f) cp[f][tid] = cpm[f * half + (l - m)];
            }
            __syncthreads();
            int i0 = 0;
            if (l0 == m) {            // degree m: the seed itself
                const double v = p1 * fac;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    gr[f] = fma(cp[f][0].x, v, gr[f]);
                    gi[f] = fma(cp[f][0].y, v, gi[f]);
                }
                i0 = 1;
            }
            for (int i = i0; i < n; ++i) {
                const double v = sht_step(rec[i], x, p1, p2, k, fac);
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const cplx c = cp[f][i];
                    gr[f] = fma(c.x, v, gr[f]);
                    gi[f] = fma(c.y, v, gi[f]);
                }
            }
        }
        if (ring) {
            double *c0 = At + (size_t)(2 * m) * ldA, *c1 = c0 + ldA;
            const double w = m == 0 ? 1.0 : 2.0;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                c0[(size_t)f * L + t] = w * gr[f];
                c1[(size_t)f * L + t] = m == 0 ? 0.0 : w * gi[f];
            }
        }
    }
}

// The Fourier stage over M = F L stacked rows: k_sht_fourier's K-loop, statement for statement; the epilogue sends row r
// to field r / L, ring r % L (a 64-row tile may span two fields), as a double or, where bit r / L of f32mask is set, as a
// float by a plain conversion (round to nearest even: numpy's astype), packed at the start of the field's slot.
__global__ __launch_bounds__(256) void k_sht_fourier_fields(int L, int M, int K, const double *__restrict__ At, int ldA,
                                                            const double2 *__restrict__ tw, double *__restrict__ f,
                                                            unsigned f32mask)
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
    const size_t slot = (size_t)L * P;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = row0 + wm * 32 + mi * 16 + q4 + 4 * reg;
                const unsigned col = (unsigned)(col0 + wn * 32 + ni * 16 + r16);
                if (row >= M || col >= P) continue;
                const int fi = row / L, t = row - fi * L;
                const double v = acc[mi][ni][reg];
                double *slot_f = f + (size_t)fi * slot;
                const size_t e = (size_t)t * P + col;
                if ((f32mask >> fi) & 1u) reinterpret_cast<float *>(slot_f)[e] = (float)v;
                else slot_f[e] = v;
            }
}


// =====================================================================================================================
// ANALYSIS (fun2shc / fun2shr): McEwen-Wiaux analysis on the same grid, the synthesis run backwards.  With P = 2L-1,
//   F_m(t)  = (1/P) sum_p f[t, p] e^{-2 pi i m p/P}                          (ring DFT:      k_sht_gemm_nt<SHG_DFT>)
//   h_m     = Q_{m mod 2} F_m                                                 (theta operator: k_sht_gemm_nt<SHG_THETA>)
//   a_lm    = (2 pi/P) sum_{t<L} lambda_lm(theta_t) h_m(t)                    (k_sht_analysis, then k_sht_unpack)
// Q_even, Q_odd are two real L x L matrices that depend on L only: extend the L ring values of F_m to the 2L-1 nodes of
// the full circle with the sign (-1)^m (the ring theta = pi kept as it is), interpolate by a trigonometric polynomial,
// multiply by sin theta on [0, pi] and 0 beyond, project onto the degrees |k| < L, evaluate at the nodes and fold them
// back with the same sign.  In the cosine / sine bases of the nodes, with C[k, t] = cos(k theta_t), S[k, t] = sin(k theta_t),
// e_0 = 1, e_k = 2, r_t = 2 (r_{L-1} = 1), we(n) = int_0^pi cos(n x) sin x dx = 2/(1 - n^2) (n even), 0 (n odd):
//   Q_even[t, t'] = (r_t r_t'/P) sum_{k,j} e_k C[k, t] Wcc[k, j] e_j C[j, t'],   Wcc[k, j] = (we(j+k) + we(j-k))/2,
//   Q_odd[t, t']  = (16/P)       sum_{k,j}     S[k, t] Wss[k, j]     S[j, t'],   Wss[k, j] = (we(j-k) - we(j+k))/2
// for t, t' < L-1, and the ring theta = pi (not folded; its extension is the symmetric node polynomial) adds to Q_odd
//   Q_odd[t, L-1] = Q_odd[L-1, t] = (2 pi/P) (-1)^L sin((L-1) theta_t),   Q_odd[L-1, L-1] = Q_even[L-1, L-1]
// (int cos(k x) sin(j x) sin x dx is pi/4 at j - k = +-1 or j + k = 1 only, which leaves the one term k = L-1).
// qf_launch_sht_qbuild forms both by two products each with k_sht_gemm_nt<SHG_PLAIN>; they stay in ctx->sht.Q until
// another L is asked for.
// =====================================================================================================================

enum { SHG_DFT = 0, SHG_THETA = 1, SHG_PLAIN = 2 };

struct sht_gemm_args {
    int K;                     // every mode: length of the reduction (DFT: P;  THETA: L;  PLAIN: see qf_launch_sht_qbuild)
    int ld;                    // leading dimension of the k-major arrays F and h (DFT, THETA) or of the square ones (PLAIN)
    const double *A, *B;       // DFT: -, the grid;  THETA: F, Q (even, then odd);  PLAIN: A, B
    double *C;
    // DFT and THETA
    int L;                     // bandwidth
    int M;                     // DFT: rows of the grid operand (L, or 2L: re / im stacked)
    int P;                     // DFT: 2L - 1
    int cplx_in;               // DFT: the grid is complex128
    const double2 *tw;         // DFT: the twiddles
    int ldq;                   // THETA: order of each stored Q (L padded to a multiple of 64)
    // PLAIN
    int nout;                  // rows and columns of the result that are stored (the rest of the padded array stays zero)
    int weights;               // the result is scaled by r_i r_j, r = (2, ..., 2, 1) over nout
    double scale;
};

// C[i][j] = sum_k A(i, k) B(j, k): both operands contiguous along k, 64 x 64 tile per workgroup, each wave a 32 x 32
// quarter (2 x 2 MFMA blocks), every load and store guarded or inside a padded array.
//   SHG_DFT  : i = 2m + c (T[2m, p] = cos(2 pi m p/P), T[2m+1, p] = -sin: gathered per K-step at (m p) mod P),
//              j = row of the grid (t, or L + t for the imaginary part), k = p;  C[i][j] = sum / P
//   SHG_THETA: blockIdx.z = parity + 2 (re | im half); i counts the rows 2m + c with m of that parity, j = t, k = t'
//   SHG_PLAIN: square arrays padded with zeros to a multiple of 64
template <int MODE>
__global__ __launch_bounds__(256) void k_sht_gemm_nt(sht_gemm_args g)
{
    __shared__ double As[SHT_BK][SHT_BM + 2];
    __shared__ double Bs[SHT_BK][SHT_BN + 2];
    const int L = g.L;
    const unsigned P = (unsigned)g.P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r16 = lane & 15, q4 = lane >> 4;
    const int row0 = blockIdx.y * SHT_BM, col0 = blockIdx.x * SHT_BN;
    const int par = blockIdx.z & 1, off = (blockIdx.z >> 1) * L;
    const int K = g.K;
    const size_t ld = (size_t)g.ld;
    const double *Bq = MODE == SHG_THETA ? g.B + (size_t)par * g.ldq * g.ldq : g.B;
    qf_d4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = qf_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += SHT_BK) {
        if (MODE == SHG_DFT) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int idx = tid + 256 * r, mm = idx >> 4, kk = idx & 15;
                const unsigned m = (unsigned)(row0 >> 1) + mm, p = (unsigned)(k0 + kk);
                double cs = 0.0, sn = 0.0;
                if (m < (unsigned)L && p < P) {
                    const double2 w = g.tw[(m * p) % P];
                    cs = w.x;
                    sn = -w.y;
                }
                As[kk][2 * mm] = cs;
                As[kk][2 * mm + 1] = sn;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + 256 * r, rr = idx >> 4, kk = idx & 15;
            const int k = k0 + kk;
            if (MODE == SHG_DFT) {
                const int j = col0 + rr;
                double v = 0.0;
                if (j < g.M && k < g.P) {
                    if (g.cplx_in) v = g.B[2 * ((size_t)(j < L ? j : j - L) * P + k) + (j < L ? 0 : 1)];
                    else v = g.B[(size_t)j * P + k];
                }
                Bs[kk][rr] = v;
            } else if (MODE == SHG_THETA) {
                const int i = row0 + rr;
                const int row = 4 * (i >> 1) + 2 * par + (i & 1);
                As[kk][rr] = (row < 2 * L && k < L) ? g.A[(size_t)row * ld + off + k] : 0.0;
                Bs[kk][rr] = Bq[(size_t)(col0 + rr) * g.ldq + k];
            } else {
                As[kk][rr] = g.A[(size_t)(row0 + rr) * ld + k];
                Bs[kk][rr] = g.B[(size_t)(col0 + rr) * ld + k];
            }
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
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = row0 + wm * 32 + mi * 16 + q4 + 4 * reg;
                const int j = col0 + wn * 32 + ni * 16 + r16;
                const double v = acc[mi][ni][reg];
                if (MODE == SHG_DFT) {
                    if (i < 2 * L && j < g.M) g.C[(size_t)i * ld + j] = v / (double)g.P;
                } else if (MODE == SHG_THETA) {
                    const int row = 4 * (i >> 1) + 2 * par + (i & 1);
                    if (row < 2 * L && j < L) g.C[(size_t)row * ld + off + j] = v;
                } else {
                    if (i < g.nout && j < g.nout) {
                        const double wi = (g.weights && i != g.nout - 1) ? 2.0 : 1.0, wj = (g.weights && j != g.nout - 1) ? 2.0 : 1.0;
                        g.C[(size_t)i * ld + j] = (g.scale * (wi * wj)) * v;
                    }
                }
            }
}

// ---- the factors of Q (Lp x Lp, zero beyond L): TR[t][k] = e_k cos(k theta_t) (par 0) or sin(k theta_t) (par 1), the
// argument reduced exactly, k (2t+1) mod 2P; W[k][j] = Wcc or Wss
__global__ __launch_bounds__(256) void k_shq_factors(int L, int Lp, int par, double *__restrict__ TR, double *__restrict__ W)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= Lp) return;
    double tr = 0.0, w = 0.0;
    if (r < L && c < L) {
        const int P = 2 * L - 1;
        int n = (int)(((long long)c * (2 * r + 1)) % (2 * P));
        if (n > P) n -= 2 * P;
        double sn, cs;
        sincospi((double)n / (double)P, &sn, &cs);
        tr = par == 0 ? (c == 0 ? 1.0 : 2.0) * cs : sn;
        const double s = (double)(r + c), d = (double)(c - r);
        const double ws = ((r + c) & 1) ? 0.0 : 2.0 / (1.0 - s * s);          // the parities of r + c and c - r agree
        const double wd = ((r + c) & 1) ? 0.0 : 2.0 / (1.0 - d * d);
        w = par == 0 ? 0.5 * (ws + wd) : 0.5 * (wd - ws);
    }
    TR[(size_t)r * Lp + c] = tr;
    W[(size_t)r * Lp + c] = w;
}

// ---- the row and column of Q_odd that belong to the ring theta = pi
__global__ __launch_bounds__(256) void k_shq_border(int L, int Lp, const double *__restrict__ Qe, double *__restrict__ Qo)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const size_t last = (size_t)(L - 1);
    if (t == L - 1) {
        Qo[last * Lp + last] = Qe[last * Lp + last];
        return;
    }
    const int P = 2 * L - 1;
    int n = (int)(((long long)(L - 1) * (2 * t + 1)) % (2 * P));
    if (n > P) n -= 2 * P;
    const double v = (2.0 * 3.14159265358979323846 / (double)P) * ((L & 1) ? -1.0 : 1.0) * sinpi((double)n / (double)P);
    Qo[(size_t)t * Lp + last] = v;
    Qo[last * Lp + t] = v;
}

// ---- Legendre analysis: one workgroup per pair of orders (m = y and L-1-y) walks the ring blocks in index order, one
// lane per ring, the recurrence and its carrying shared with k_sht_legendre.  The sum over rings of every degree has a
// fixed order: 16 degrees at a time, a butterfly over the wave (each exchange halves the values a lane holds: lane i
// ends with the degree i / 4 summed over 16 lanes, two more exchanges add the four groups), the four waves are added in
// LDS in wave order, and the thread that owns the degree adds the ring block's partial to the column in ctx->sht.col --
// the same thread for every block, in block order, so no atomics and no partial array (32 blocks of L^2/2 complex at
// L = 8192 would be 17 GB).  h: [2m + c][t] from the theta operator; complex input has the imaginary part's rows at
// L + t, and F_m = (A_c - B_s) + i (B_c + A_s), F_-m = (A_c + B_s) + i (B_c - A_s) (A, B: real and imaginary grid).
// colp = sum lambda_lm h_m, coln = sum lambda_lm h_-m (the sign (-1)^m of lambda_l,-m is applied by k_sht_unpack).
constexpr int SHT_DEG = 16;    // degrees reduced together

template <bool CPLX>
__global__ __launch_bounds__(SHT_RINGS) void k_sht_analysis(int L, const double *__restrict__ seed,
                                                            const double *__restrict__ H, int ldA,
                                                            cplx *__restrict__ colp, cplx *__restrict__ coln)
{
    constexpr int NV = CPLX ? 4 : 2;
    __shared__ double2 rec[SHT_CHUNK];
    __shared__ double red[2][SHT_RINGS / 64][SHT_DEG][NV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y = blockIdx.x;
    const int nblocks = (L + SHT_RINGS - 1) / SHT_RINGS;
    int flip = 0;
    for (int half = 0; half < 2; ++half) {
        const int m = half == 0 ? y : L - 1 - y;
        if (half == 1 && m <= y) break;
        const double seedm = seed[m];
        double *outp = reinterpret_cast<double *>(colp + col_offset(m, L));
        double *outn = CPLX ? reinterpret_cast<double *>(coln + col_offset(m, L)) : nullptr;
        for (int blk = 0; blk < nblocks; ++blk) {
            const int t = blk * SHT_RINGS + tid;
            const bool ring = t < L;
            const int tt = ring ? t : L - 1;      // lanes past the last ring walk a copy of it with h = 0
            const sht_ring g = sht_ring_of(tt, L);
            const double x = g.x;
            int k;
            double p1, p2 = 0.0;
            sht_seed(m, seedm, g, p1, k);
            double fac = sht_factor(k);
            double h[NV];
#pragma unroll
            for (int c = 0; c < NV; ++c) h[c] = 0.0;
            if (ring) {
                const double *h0 = H + (size_t)(2 * m) * ldA, *h1 = h0 + ldA;
                if (!CPLX) {
                    h[0] = h0[t];
                    h[1] = h1[t];
                } else {
                    const double ac = h0[t], as = h1[t], bc = h0[L + t], bs = h1[L + t];
                    h[0] = ac - bs;
                    h[1] = bc + as;
                    h[2] = ac + bs;
                    h[3] = bc - as;
                }
            }
            for (int l0 = m; l0 < L; l0 += SHT_CHUNK) {
                const int n = min(SHT_CHUNK, L - l0);
                __syncthreads();
                if (tid < n) rec[tid] = sht_ab(l0 + tid, m);
                __syncthreads();
                for (int i0 = 0; i0 < n; i0 += SHT_DEG) {
                    double vals[SHT_DEG][NV];
#pragma unroll
                    for (int j = 0; j < SHT_DEG; ++j) {
                        const int i = i0 + j;
                        double v = 0.0;
                        if (i < n) {
                            if (l0 == m && i == 0) v = p1 * fac;           // degree m: the seed itself
                            else v = sht_step(rec[i], x, p1, p2, k, fac);
                        }
#pragma unroll
                        for (int c = 0; c < NV; ++c) vals[j][c] = v * h[c];
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int o = 32 >> s, hn = (SHT_DEG / 2) >> s;
                        const bool up = (lane & o) != 0;
#pragma unroll
                        for (int i = 0; i < hn; ++i)
#pragma unroll
                            for (int c = 0; c < NV; ++c) {
                                const double send = up ? vals[i][c] : vals[i + hn][c];
                                const double keep = up ? vals[i + hn][c] : vals[i][c];
                                vals[i][c] = keep + __shfl_xor(send, o);
                            }
                    }
#pragma unroll
                    for (int c = 0; c < NV; ++c) {
                        double v = vals[0][c];
                        v += __shfl_xor(v, 1);
                        v += __shfl_xor(v, 2);
                        if ((lane & 3) == 0) red[flip][wave][lane >> 2][c] = v;
                    }
                    __syncthreads();
                    if (tid < SHT_DEG * NV) {
                        const int d = tid / NV, c = tid % NV;
                        if (i0 + d < n) {
                            double sum = red[flip][0][d][c];
#pragma unroll
                            for (int w = 1; w < SHT_RINGS / 64; ++w) sum += red[flip][w][d][c];
                            double *dst = (c < 2 ? outp : outn) + 2 * (size_t)(l0 - m + i0 + d) + (c & 1);
                            *dst = blk == 0 ? sum : *dst + sum;
                        }
                    }
                    flip ^= 1;      // the next 16 degrees write the other half of red: one barrier per 16 degrees
                }
            }
        }
    }
}

// ---- m-major columns -> omega[l^2 + l + m]: a_lm = (col (2 pi/P)) / sqrt(4 pi).  SHR: the real coefficients, with
// shc2shr's operations (transforms.py:271-307: (sqrt(2) (-1)^m) Re a_lm at +m, the same factor times Im a_lm at -m).
// Complex output: NEG takes a_l,-m = (-1)^m coln (complex input); otherwise a_l,-m = (-1)^m conj(a_lm) (real input).
template <bool SHR, bool NEG>
__global__ __launch_bounds__(256) void k_sht_unpack(int L, const cplx *__restrict__ colp, const cplx *__restrict__ coln,
                                                    double c1, double rt4pi, double *__restrict__ omega)
{
    const int m = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L - m) return;
    const long long l = m + j;
    const long long ip = l * l + l + m, im = l * l + l - m;
    const size_t o = col_offset(m, L) + j;
    const cplx a = colp[o];
    const double ar = (a.x * c1) / rt4pi, ai = (a.y * c1) / rt4pi;
    const double sg = (m & 1) ? -1.0 : 1.0;
    if (SHR) {
        if (m == 0) {
            omega[ip] = ar;
        } else {
            const double c = sqrt(2.0) * sg;
            omega[ip] = c * ar;
            omega[im] = c * ai;
        }
    } else {
        cplx *oc = reinterpret_cast<cplx *>(omega);
        oc[ip] = make_double2(ar, ai);
        if (m > 0) {
            if (NEG) {
                const cplx b = coln[o];
                oc[im] = make_double2(sg * ((b.x * c1) / rt4pi), sg * ((b.y * c1) / rt4pi));
            } else {
                oc[im] = make_double2(sg * ar, -(sg * ai));
            }
        }
    }
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

// ---- stacked real synthesis: what each ctx->sht buffer needs for nf fields of bandwidth L (tab: nf scale rows, then the seeds)
void qf_sht_fields_sizes(int L, int nf, size_t bytes[6])
{
    const size_t LL = (size_t)L * L, P = 2 * (size_t)L - 1, half = (size_t)L * (L + 1) / 2;
    bytes[0] = LL * sizeof(double);
    bytes[1] = ((size_t)nf + 1) * L * sizeof(double);
    bytes[2] = (size_t)nf * half * sizeof(cplx);
    bytes[3] = (size_t)round_up(2 * L, SHT_BK) * round_up(nf * L, SHT_BM) * sizeof(double);
    bytes[4] = P * sizeof(double2);
    bytes[5] = (size_t)nf * L * P * sizeof(double);
}

namespace {

template <int F>
int launch_fields(qf_ctx *ctx, int L, const sht_field_lengths &len, const double *omega_dev, int ldA)
{
    qf_sht &S = ctx->sht;
    const dim3 gp((L + 255) / 256, L), gl((L + SHT_RINGS - 1) / SHT_RINGS, (L + 1) / 2);
    hipLaunchKernelGGL(k_sht_pack_fields<F>, gp, dim3(256), 0, ctx->stream, L, len, omega_dev, S.tab, S.col);
    QF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sht_legendre_fields<F>, gl, dim3(SHT_RINGS), 0, ctx->stream, L, S.tab + (size_t)F * L, S.col, S.At, ldA);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

}  // namespace

// nf real fields of bandwidth L from omega_dev into the nf slots of ctx->sht.f (slot f: L (2L-1) doubles, or as many floats
// packed at its start where bit f of f32mask is set).  ctx->sht.tab holds nf scale rows and the seeds.
int qf_launch_sht_fields(qf_ctx *ctx, int L, int nf, const long long *n_valid, unsigned f32mask, const double *omega_dev)
{
    qf_sht &S = ctx->sht;
    const int P = 2 * L - 1, M = nf * L, K = round_up(2 * L, SHT_BK), ldA = round_up(M, SHT_BM);
    sht_field_lengths len = {{0, 0, 0, 0}};
    for (int f = 0; f < nf; ++f) len.n[f] = n_valid[f];
    hipLaunchKernelGGL(k_sht_twiddle, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, P, S.tw);
    QF_HIP(hipGetLastError());
    // rows 2L..K-1 of At meet zero twiddles; zeroed so that nothing stale (a NaN of an earlier call) enters the sums
    if (K > 2 * L) QF_HIP(hipMemsetAsync(S.At + (size_t)2 * L * ldA, 0, (size_t)(K - 2 * L) * ldA * sizeof(double), ctx->stream));
    switch (nf) {
    case 1: QF_TRY(launch_fields<1>(ctx, L, len, omega_dev, ldA)); break;
    case 2: QF_TRY(launch_fields<2>(ctx, L, len, omega_dev, ldA)); break;
    case 3: QF_TRY(launch_fields<3>(ctx, L, len, omega_dev, ldA)); break;
    case 4: QF_TRY(launch_fields<4>(ctx, L, len, omega_dev, ldA)); break;
    default: qf_set_error("qf_launch_sht_fields: %d fields (1..4)", nf); return QF_ERR_INVALID;
    }
    const dim3 gf((P + SHT_BN - 1) / SHT_BN, ldA / SHT_BM);
    hipLaunchKernelGGL(k_sht_fourier_fields, gf, dim3(256), 0, ctx->stream, L, M, K, S.At, ldA, S.tw, S.f, f32mask);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

// ---- analysis: what each ctx->sht buffer needs for (L, isreal); [6] = h, [7] = Q.  f and h are also the workspace of
// the one-off Q build (two and one padded L x L factors)
void qf_sht_analysis_sizes(int L, int isreal, size_t bytes[8])
{
    qf_sht_sizes(L, isreal, bytes);
    const size_t Lp = (size_t)round_up(L, 64), sq = Lp * Lp * sizeof(double);
    bytes[5] = std::max(bytes[5], 2 * sq);
    bytes[6] = std::max(bytes[3], sq);
    bytes[7] = 2 * sq;
}

// Q_even, Q_odd for bandwidth L into ctx->sht.Q (ctx->sht.q_L says which L it holds)
int qf_launch_sht_qbuild(qf_ctx *ctx, int L)
{
    qf_sht &S = ctx->sht;
    S.q_L = 0;
    const int Lp = round_up(L, 64);
    const size_t sq = (size_t)Lp * Lp;
    double *TR = S.f, *W = S.f + sq, *T1 = S.H;
    QF_HIP(hipMemsetAsync(S.Q, 0, 2 * sq * sizeof(double), ctx->stream));
    const dim3 gg(Lp / SHT_BN, Lp / SHT_BM);
    for (int par = 0; par < 2; ++par) {
        hipLaunchKernelGGL(k_shq_factors, dim3((Lp + 255) / 256, Lp), dim3(256), 0, ctx->stream, L, Lp, par, TR, W);
        QF_HIP(hipGetLastError());
        sht_gemm_args g = {};
        g.K = Lp;                  // the factors are zero beyond L: the whole padded product is formed
        g.nout = Lp;
        g.ld = Lp;
        g.scale = 1.0;
        g.A = TR;                  // T1[t][i] = sum_k TR[t][k] W[i][k]
        g.B = W;
        g.C = T1;
        hipLaunchKernelGGL(k_sht_gemm_nt<SHG_PLAIN>, gg, dim3(256), 0, ctx->stream, g);
        QF_HIP(hipGetLastError());
        g.K = L;                   // Q[t][t'] = scale r_t r_t' sum_i TR[t][i] T1[t'][i]
        g.nout = L;
        g.weights = par == 0;
        g.scale = (par == 0 ? 1.0 : 16.0) / (double)(2 * L - 1);
        g.B = T1;
        g.C = S.Q + (size_t)par * sq;
        hipLaunchKernelGGL(k_sht_gemm_nt<SHG_PLAIN>, gg, dim3(256), 0, ctx->stream, g);
        QF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_shq_border, dim3((L + 255) / 256), dim3(256), 0, ctx->stream, L, Lp, S.Q, S.Q + sq);
    QF_HIP(hipGetLastError());
    S.q_L = L;
    return QF_OK;
}

// The grid in ctx->sht.f (doubles when isreal, else complex128) -> L^2 coefficients in omega_dev: real (shr) or complex.
int qf_launch_sht_analysis(qf_ctx *ctx, int L, int shr, int isreal, double *omega_dev)
{
    qf_sht &S = ctx->sht;
    int M, K, ldA;
    sht_shape(L, isreal, &M, &K, &ldA);
    const int P = 2 * L - 1, Lp = round_up(L, 64);
    cplx *colp = S.col, *coln = isreal ? nullptr : S.col + (size_t)L * (L + 1) / 2;
    hipLaunchKernelGGL(k_sht_twiddle, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, P, S.tw);
    QF_HIP(hipGetLastError());
    sht_gemm_args g = {};
    g.K = P;
    g.L = L;
    g.M = M;
    g.P = P;
    g.ld = ldA;
    g.cplx_in = isreal ? 0 : 1;
    g.B = S.f;
    g.tw = S.tw;
    g.C = S.At;
    hipLaunchKernelGGL(k_sht_gemm_nt<SHG_DFT>, dim3(ldA / SHT_BN, round_up(2 * L, SHT_BM) / SHT_BM), dim3(256), 0, ctx->stream, g);
    QF_HIP(hipGetLastError());
    g.K = L;
    g.ldq = Lp;
    g.A = S.At;
    g.B = S.Q;
    g.C = S.H;
    const int rows = 2 * ((L + 1) / 2);        // rows 2m + c with m even; the odd orders have no more
    hipLaunchKernelGGL(k_sht_gemm_nt<SHG_THETA>, dim3(Lp / SHT_BN, round_up(rows, SHT_BM) / SHT_BM, isreal ? 2 : 4), dim3(256), 0,
                       ctx->stream, g);
    QF_HIP(hipGetLastError());
    const dim3 ga((L + 1) / 2);
    if (isreal)
        hipLaunchKernelGGL(k_sht_analysis<false>, ga, dim3(SHT_RINGS), 0, ctx->stream, L, S.tab + L, S.H, ldA, colp, coln);
    else
        hipLaunchKernelGGL(k_sht_analysis<true>, ga, dim3(SHT_RINGS), 0, ctx->stream, L, S.tab + L, S.H, ldA, colp, coln);
    QF_HIP(hipGetLastError());
    const double c1 = 2.0 * 3.14159265358979323846 / (double)P, rt4pi = sqrt(4.0 * 3.14159265358979323846);
    const dim3 gp((L + 255) / 256, L);
    if (shr)
        hipLaunchKernelGGL((k_sht_unpack<true, false>), gp, dim3(256), 0, ctx->stream, L, colp, coln, c1, rt4pi, omega_dev);
    else if (isreal)
        hipLaunchKernelGGL((k_sht_unpack<false, false>), gp, dim3(256), 0, ctx->stream, L, colp, coln, c1, rt4pi, omega_dev);
    else
        hipLaunchKernelGGL((k_sht_unpack<false, true>), gp, dim3(256), 0, ctx->stream, L, colp, coln, c1, rt4pi, omega_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
