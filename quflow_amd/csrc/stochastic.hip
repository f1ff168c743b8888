// Stochastic band-limited forcing drawn and applied on the device (include/quflow_hip.h).
// Over the step n -> n + 1 of size dt the pattern of the installed forcing is F0_n = shr2mat(omega_n) with
//     omega_n[l^2 + l + m] = (sigma_l * (1 / sqrt(dt))) * xi_n(l, m),   l_min <= l <= l_max,  zero elsewhere,
// xi iid N(0,1) from the counter-based generator Philox4x32-10: key (seed lo, seed hi), counter (n lo, n hi, b, 0) with
// b = q >> 1, q = l^2 + l + m -- one block gives the two normals of the entries q = 2b (cosine) and 2b + 1 (sine) by
// Box-Muller.  A coefficient depends on (seed, n, l, m) alone, so a host mirror repeats it (StochasticForcing.draw_host).
// Per step three launches: k_stoch_draw here, then k_pack_coeffs and the slab k_block_matvec of quantization.hip on a band
// basis the context keeps (qf_launch_band_shr2mat), into ctx->forcing_f0 -- the buffer the forced loop already reads.
#include <cmath>

#include "qf_api.h"

#pragma clang fp contract(off)   // s = sigma * inv, omega = s * xi, r * cos(t): every product rounded on its own

namespace {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned x[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0;
    x[1] = c1;
    x[2] = c2;
    x[3] = c3;
}

// floor(sqrt(q)) for q < 2^26: the double root is within one of it, the two corrections make it exact
__device__ __forceinline__ int degree_of(long long q)
{
    long long l = (long long)sqrt((double)q);
    if (l * l > q) --l;
    if ((l + 1) * (l + 1) <= q) ++l;
    return (int)l;
}

// One Philox block per lane, consecutive lanes on consecutive blocks b0 + t: the entries q = 2b and 2b + 1 that lie in
// [q_lo, q_hi) = [l_min^2, (l_max + 1)^2) are written (both when both do).  sigma[l - l_min]; inv = 1 / sqrt(dt).
__global__ __launch_bounds__(256) void k_stoch_draw(unsigned seed_lo, unsigned seed_hi, unsigned n_lo, unsigned n_hi, long long b0,
                                                     long long blocks, long long q_lo, long long q_hi, int l_min,
                                                     const double *__restrict__ sigma, double inv, double *__restrict__ omega)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= blocks) return;
    const long long b = b0 + t;
    unsigned x[4];
    philox4x32_10(n_lo, n_hi, (unsigned)b, 0u, seed_lo, seed_hi, x);
    // (every operation exact in double: 27 + 26 bits)
    const double u = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6) + 1.0) * 0x1p-53;     // (0, 1]
    const double v = ((double)(x[2] >> 5) * 67108864.0 + (double)(x[3] >> 6)) * 0x1p-53;           // [0, 1)
    const double r = sqrt(-2.0 * log(u));
    const double ang = 6.283185307179586 * v;
    double sn, cs;
    sincos(ang, &sn, &cs);
    const long long q0 = 2 * b, q1 = q0 + 1;
    if (q0 >= q_lo && q0 < q_hi) {
        const double s = sigma[degree_of(q0) - l_min] * inv;
        omega[q0] = s * (r * cs);
    }
    if (q1 >= q_lo && q1 < q_hi) {
        const double s = sigma[degree_of(q1) - l_min] * inv;
        omega[q1] = s * (r * sn);
    }
}

int need_stochastic(const qf_ctx *ctx, const char *who)
{
    if (!ctx->forcing_on || !ctx->stoch.on) {
        qf_set_error("%s: no stochastic forcing is installed (qf_set_stochastic_forcing)", who);
        return QF_ERR_STATE;
    }
    return QF_OK;
}

}  // namespace

int qf_launch_stoch_pattern(qf_ctx *ctx, unsigned long long step, double dt)
{
    const qf_stoch &s = ctx->stoch;
    if (!(dt > 0.0) || !QF_FINITE(dt)) {
        qf_set_error("stochastic forcing: the step size must be positive and finite (dt=%g): the noise scales with 1/sqrt(dt)", dt);
        return QF_ERR_INVALID;
    }
    const double inv = 1.0 / std::sqrt(dt);
    const long long q_lo = (long long)s.l_min * s.l_min, q_hi = (long long)(s.l_max + 1) * (s.l_max + 1);
    const long long b0 = q_lo >> 1, blocks = ((q_hi - 1) >> 1) - b0 + 1;
    ctx->forcing_key = 0;       // forcing_f0 is rewritten: no later qf_set_forcing may trust the fingerprint of what it held
    hipLaunchKernelGGL(k_stoch_draw, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned)(s.seed & 0xffffffffull),
                       (unsigned)(s.seed >> 32), (unsigned)(step & 0xffffffffull), (unsigned)(step >> 32), b0, blocks, q_lo, q_hi,
                       s.l_min, s.sigma, inv, s.omega);
    QF_HIP(hipGetLastError());
    return qf_launch_band_shr2mat(ctx, s.nmax, s.basis, s.omega, s.stage, ctx->forcing_f0);
}

extern "C" {

int qf_set_stochastic_forcing(qf_ctx *ctx, int l_min, int l_max, const double *sigma, unsigned long long seed,
                              unsigned long long step, double a_W, double a_P, double a_lap, long long band_bytes_max)
{
    QF_TRY(check_ctx(ctx));
    const int N = ctx->N;
    if (l_min < 1 || l_max < l_min || l_max > N - 1) {
        qf_set_error("qf_set_stochastic_forcing: the band must satisfy 1 <= l_min <= l_max <= N - 1 (l_min=%d, l_max=%d, N=%d)",
                     l_min, l_max, N);
        return QF_ERR_INVALID;
    }
    if (!sigma) {
        qf_set_error("qf_set_stochastic_forcing: null sigma");
        return QF_ERR_INVALID;
    }
    for (int l = l_min; l <= l_max; ++l)
        if (!QF_FINITE(sigma[l - l_min]) || !(sigma[l - l_min] >= 0.0)) {
            qf_set_error("qf_set_stochastic_forcing: sigma must be finite and >= 0 (sigma[l=%d]=%g)", l, sigma[l - l_min]);
            return QF_ERR_INVALID;
        }
    if (!QF_FINITE(a_W) || !QF_FINITE(a_P) || !QF_FINITE(a_lap)) {
        qf_set_error("qf_set_stochastic_forcing: the coefficients must be finite (a_W=%g, a_P=%g, a_lap=%g)", a_W, a_P, a_lap);
        return QF_ERR_INVALID;
    }
    const int nmax = l_max + 1;
    const long long band_bytes = 8 * qf_slab_prefix(N, nmax, nmax);
    if (band_bytes > band_bytes_max) {       // refused before anything is allocated or changed
        qf_set_error("qf_set_stochastic_forcing: the band basis for N=%d, l_max=%d takes %lld bytes, more than the cap of %lld bytes",
                     N, l_max, band_bytes, band_bytes_max);
        return QF_ERR_INVALID;
    }
    qf_stoch &s = ctx->stoch;
    const size_t NN = (size_t)N * N;
    ctx->forcing_on = false;       // nothing is in force until everything is in place
    s.on = false;
    if (!ctx->forcing_f0) QF_HIP(hipMalloc((void **)&ctx->forcing_f0, NN * sizeof(cplx)));
    ctx->forcing_key = 0;
    // zero once: every step overwrites the diagonals |i - j| <= l_max and nothing else
    QF_HIP(hipMemsetAsync(ctx->forcing_f0, 0, NN * sizeof(cplx), ctx->stream));
    if (s.nmax != nmax || !s.basis) {
        if (s.basis) {
            QF_HIP(hipStreamSynchronize(ctx->stream));
            (void)hipFree(s.basis);
        }
        s.basis = nullptr;
        s.nmax = 0;
        QF_HIP(hipMalloc((void **)&s.basis, (size_t)band_bytes));
        QF_TRY(qf_launch_band_basis(ctx, nmax, s.basis));
        s.nmax = nmax;
    }
    if (s.cap < nmax) {
        QF_HIP(hipStreamSynchronize(ctx->stream));
        void *old[] = {s.omega, s.stage, s.sigma};
        for (void *p : old)
            if (p) (void)hipFree(p);
        s.omega = nullptr;
        s.stage = nullptr;
        s.sigma = nullptr;
        s.cap = 0;
        QF_HIP(hipMalloc((void **)&s.omega, (size_t)nmax * nmax * sizeof(double)));
        QF_HIP(hipMalloc((void **)&s.stage, (size_t)nmax * N * sizeof(cplx)));
        QF_HIP(hipMalloc((void **)&s.sigma, (size_t)nmax * sizeof(double)));
        s.cap = nmax;
    }
    // the entries below l_min^2 are zero for the forcing's life; the draw writes the rest every step
    QF_HIP(hipMemsetAsync(s.omega, 0, (size_t)nmax * nmax * sizeof(double), ctx->stream));
    // (pageable source: hipMemcpyAsync returns after staging, the caller's table is free on return)
    QF_HIP(hipMemcpyAsync(s.sigma, sigma, (size_t)(l_max - l_min + 1) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    s.l_min = l_min;
    s.l_max = l_max;
    s.seed = seed;
    s.step = step;
    ctx->forcing_aW = a_W;
    ctx->forcing_aP = a_P;
    ctx->forcing_alap = a_lap;
    ctx->forcing_f0_on = true;
    s.on = true;
    ctx->forcing_on = true;
    return QF_OK;
}

int qf_stochastic_tell(qf_ctx *ctx, unsigned long long *step)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stochastic(ctx, "qf_stochastic_tell"));
    if (!step) {
        qf_set_error("qf_stochastic_tell: null output");
        return QF_ERR_INVALID;
    }
    *step = ctx->stoch.step;
    return QF_OK;
}

int qf_stochastic_seek(qf_ctx *ctx, unsigned long long step)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stochastic(ctx, "qf_stochastic_seek"));
    ctx->stoch.step = step;
    return QF_OK;
}

int qf_stochastic_pattern(qf_ctx *ctx, unsigned long long step, double dt, double *omega_host, void *F0_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stochastic(ctx, "qf_stochastic_pattern"));
    const qf_stoch &s = ctx->stoch;
    // (forcing_f0 is the run's pattern buffer: every step of a run draws its own pattern over it before reading it)
    QF_TRY(qf_launch_stoch_pattern(ctx, step, dt));
    if (omega_host)
        QF_HIP(hipMemcpyAsync(omega_host, s.omega, (size_t)s.nmax * s.nmax * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (F0_host)
        QF_HIP(hipMemcpyAsync(F0_host, ctx->forcing_f0, (size_t)ctx->N * ctx->N * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    if (omega_host || F0_host) QF_HIP(hipStreamSynchronize(ctx->stream));     // both NULL: the three launches alone, queued (timing)
    return QF_OK;
}

}  // extern "C"
