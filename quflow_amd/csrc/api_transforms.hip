// C ABI of libquflow_hip.so, part 5 of 5: spherical-harmonics <-> matrix TRANSFORMS (quflow/quantization.py) and the
// plain matrix-product entry points (qf_zgemm, qf_zgemm_i8, qf_cgemm).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <chrono>
#include <algorithm>
#include <vector>

#include "qf_api.h"

extern "C" {

// ---- spherical-harmonics transforms (quflow/quantization.py) -------------------------------
static int need_basis(qf_ctx *ctx, const char *who)
{
    if (!ctx->basis) {
        qf_set_error("%s: no quantization basis on this context (call qf_basis_upload first)", who);
        return QF_ERR_STATE;
    }
    return QF_OK;
}

static int alloc_stage(qf_ctx *ctx);

// what a transform reads its blocks from: the streamed form (qf_basis_stream > 0) needs only the staging buffers, the
// resident one the basis
static int need_source(qf_ctx *ctx, const char *who)
{
    if (ctx->slab_budget > 0) return alloc_stage(ctx);
    return need_basis(ctx, who);
}

// band limit of a coefficient array with n entries: quantization.py:204-208,294-298 (parallel form)
static int band_limit(int N, long long n)
{
    if (n >= (long long)N * N) return N;
    return (int)std::sqrt((double)n);
}

static int alloc_sh(qf_ctx *ctx);

int qf_basis_upload(qf_ctx *ctx, const double *basis_host, long long count)
{
    QF_TRY(check_ctx(ctx));
    const long long N = ctx->N;
    const long long want = N * (N + 1) * (2 * N + 1) / 6;
    if (!basis_host || count != want) {
        qf_set_error("qf_basis_upload: the basis for N=%d has %lld entries (got %lld)", ctx->N, want, count);
        return QF_ERR_INVALID;
    }
    QF_TRY(alloc_sh(ctx));
    QF_HIP(hipMemcpyAsync(ctx->basis, basis_host, (size_t)want * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

// the m-major staging vectors and the device coefficients: every transform needs them, resident or streamed
static int alloc_stage(qf_ctx *ctx)
{
    const long long N = ctx->N;
    if (!ctx->sh_stage) QF_HIP(hipMalloc((void **)&ctx->sh_stage, (size_t)4 * (N * (N + 1) / 2) * sizeof(cplx)));
    if (!ctx->sh_omega) QF_HIP(hipMalloc((void **)&ctx->sh_omega, (size_t)2 * N * N * sizeof(double)));
    return QF_OK;
}

static int alloc_sh(qf_ctx *ctx)
{
    const long long N = ctx->N;
    const long long want = N * (N + 1) * (2 * N + 1) / 6;
    if (!ctx->basis) QF_HIP(hipMalloc((void **)&ctx->basis, (size_t)want * sizeof(double)));
    return alloc_stage(ctx);
}

int qf_basis_stream(qf_ctx *ctx, long long slab_bytes)
{
    QF_TRY(check_ctx(ctx));
    if (slab_bytes < 0) {
        qf_set_error("qf_basis_stream: negative slab budget %lld", slab_bytes);
        return QF_ERR_INVALID;
    }
    ctx->slab_budget = slab_bytes;
    return QF_OK;
}

int qf_basis_slab_plan(int N, int Nmax, long long slab_bytes, int *first_block, int capacity)
{
    std::vector<int> first;
    long long max_bytes = 0;
    const int rc = qf_slab_plan(N, Nmax, slab_bytes, first, &max_bytes);
    if (rc != QF_OK) return -rc;
    const int nslabs = (int)first.size() - 1;
    for (int s = 0; first_block && s < nslabs && s < capacity; ++s) first_block[s] = first[s];
    return nslabs;
}

int qf_basis_compute(qf_ctx *ctx)
{
    QF_TRY(check_ctx(ctx));
    const bool fresh = (ctx->basis == nullptr);
    QF_TRY(alloc_sh(ctx));
    const int rc = qf_launch_basis(ctx, ctx->basis);
    if (rc != QF_OK || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        if (fresh) {   // never leave a half-built basis behind
            (void)hipFree(ctx->basis);
            ctx->basis = nullptr;
        }
        if (rc == QF_OK) qf_set_error("qf_basis_compute: kernel failed");
        return rc == QF_OK ? QF_ERR_HIP : rc;
    }
    return QF_OK;
}

int qf_basis_download(qf_ctx *ctx, double *basis_host, long long count)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_basis(ctx, "qf_basis_download"));
    const long long N = ctx->N;
    const long long want = N * (N + 1) * (2 * N + 1) / 6;
    if (!basis_host || count != want) {
        qf_set_error("qf_basis_download: the basis for N=%d has %lld entries (got %lld)", ctx->N, want, count);
        return QF_ERR_INVALID;
    }
    QF_HIP(hipMemcpyAsync(basis_host, ctx->basis, (size_t)want * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_shr2mat(qf_ctx *ctx, const double *omega_host, long long n_omega, void *W_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_source(ctx, "qf_shr2mat"));
    if (n_omega < 1) {
        qf_set_error("qf_shr2mat: empty coefficient array");
        return QF_ERR_INVALID;
    }
    const long long NN = (long long)ctx->N * ctx->N;
    const int Nmax = band_limit(ctx->N, n_omega);
    const long long ncopy = n_omega < NN ? n_omega : NN;
    // omega_host == NULL: the coefficients the last qf_mat2shr left on the device
    if (omega_host) {
        QF_HIP(hipMemcpyAsync(ctx->sh_omega, omega_host, (size_t)ncopy * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        ctx->sh_shr_count = ncopy;
    }
    cplx *dst = W_host ? ctx->stage : ctx->W;
    if (!W_host) {       // the resident state is replaced: as after qf_rotate(NULL), no increment is carried
        ctx->w_skew_known = false;
        ctx->increment_valid = false;
        ctx->w_c128_set = true;
    }
    QF_TRY(qf_launch_shr2mat(ctx, Nmax, ctx->sh_omega, dst));
    if (W_host) QF_HIP(hipMemcpyAsync(W_host, dst, (size_t)NN * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_mat2shr(qf_ctx *ctx, const void *W_host, double *omega_host, long long n_omega)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_source(ctx, "qf_mat2shr"));
    if (n_omega < 1) {
        qf_set_error("qf_mat2shr: empty coefficient array");
        return QF_ERR_INVALID;
    }
    const long long NN = (long long)ctx->N * ctx->N;
    const int Nmax = band_limit(ctx->N, n_omega);
    const long long ncopy = n_omega < NN ? n_omega : NN;
    const cplx *src = ctx->W;
    if (W_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, W_host, (size_t)NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
        src = ctx->stage;
    }
    QF_HIP(hipMemsetAsync(ctx->sh_omega, 0, (size_t)ncopy * sizeof(double), ctx->stream));   // np.zeros, quantization.py:516
    QF_TRY(qf_launch_mat2shr(ctx, Nmax, src, ctx->sh_omega));
    ctx->sh_shr_count = ncopy;
    // omega_host == NULL: leave the coefficients on the device (a following qf_shr2mat(NULL) uses them)
    if (omega_host)
        QF_HIP(hipMemcpyAsync(omega_host, ctx->sh_omega, (size_t)ncopy * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    if (omega_host)
        for (long long i = ncopy; i < n_omega; ++i) omega_host[i] = 0.0;
    return QF_OK;
}

int qf_shc2mat(qf_ctx *ctx, const void *omega_host, void *W_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_source(ctx, "qf_shc2mat"));
    if (!omega_host) {
        qf_set_error("qf_shc2mat: null coefficient array");
        return QF_ERR_INVALID;
    }
    const size_t NN = (size_t)ctx->N * ctx->N;
    QF_HIP(hipMemcpyAsync(ctx->sh_omega, omega_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    ctx->sh_shr_count = 0;     // (complex now)
    cplx *dst = W_host ? ctx->stage : ctx->W;
    if (!W_host) {       // the resident state is replaced: as after qf_rotate(NULL), no increment is carried
        ctx->w_skew_known = false;
        ctx->increment_valid = false;
        ctx->w_c128_set = true;
    }
    QF_TRY(qf_launch_shc2mat(ctx, ctx->sh_omega, dst));
    if (W_host) QF_HIP(hipMemcpyAsync(W_host, dst, NN * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_mat2shc(qf_ctx *ctx, const void *W_host, void *omega_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_source(ctx, "qf_mat2shc"));
    if (!omega_host) {
        qf_set_error("qf_mat2shc: null coefficient array");
        return QF_ERR_INVALID;
    }
    const size_t NN = (size_t)ctx->N * ctx->N;
    const cplx *src = ctx->W;
    if (W_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, W_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
        src = ctx->stage;
    }
    QF_TRY(qf_launch_mat2shc(ctx, src, ctx->sh_omega));
    ctx->sh_shr_count = 0;
    QF_HIP(hipMemcpyAsync(omega_host, ctx->sh_omega, NN * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

// ---- the per-degree budget of a state (include/quflow_hip.h): Z_l, T_l, I_l from one sweep of the basis
// nv = 1: the spectrum alone (no solve, no product); 2: with the advective tendency; 3: with the installed forcing too.
// Where everything lives (all of it per-iteration scratch, free between stepper calls):
//   W       ctx->W (resident) or ctx->stage (uploaded)            -X^H, then F  ctx->Whalf
//   P, A    ctx->Phalf, ctx->PW, both left there for qf_download_buffer
//   packed diagonals  ctx->sh_stage parts 0..2;   z_0  part 3;   z_1, z_2  ctx->Whalf, ctx->stage (dead once packed)
//   omega, a  ctx->sh_omega (two halves);   f, the sums  ctx->sh_stage parts 0, 1 (dead after the sweep)
static int budget_run(qf_ctx *ctx, const char *who, const void *W_host, int Nmax, int nv, double *out, double *coeffs)
{
    QF_TRY(check_ctx(ctx));
    const int N = ctx->N;
    if (!out) {
        qf_set_error("%s: null output", who);
        return QF_ERR_INVALID;
    }
    if (Nmax <= 1 || Nmax > N) {
        qf_set_error("%s: band limit Nmax=%d outside 2..N=%d", who, Nmax, N);
        return QF_ERR_INVALID;
    }
    if (!W_host && ctx->c64 && !ctx->w_c128_set) {
        qf_set_error("%s: this context holds a complex64 state only; the budget is double precision (pass W_host)", who);
        return QF_ERR_STATE;
    }
    if (ctx->slab_budget > 0) {       // (the slab plan's refusal comes before anything is launched)
        std::vector<int> first;
        long long need = 0;
        QF_TRY(qf_slab_plan(N, Nmax, ctx->slab_budget, first, &need));
    }
    QF_TRY(need_source(ctx, who));
    const size_t NN = (size_t)N * N, half = (size_t)N * (N + 1) / 2;
    const cplx *W = ctx->W;
    if (W_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, W_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
        W = ctx->stage;
    }
    if (nv >= 2) {
        const double inv_hb = 1.0 / qf_hbar(N);
        QF_TRY(qf_launch_hamiltonian(ctx, W, ctx->Phalf, 1.0));                                    // P
        QF_TRY(qf_launch_zgemm(ctx, ctx->Phalf, W, ctx->PW, nullptr));                             // X = P @ W
        QF_TRY(qf_launch_neg_conj_transpose(ctx, ctx->PW, ctx->Whalf));                            // -X^H
        QF_TRY(qf_launch_lincomb(ctx, 1.0, ctx->PW, 1.0, ctx->Whalf, 0.0, ctx->PW));               // X - X^H
        QF_TRY(qf_launch_lincomb(ctx, inv_hb, ctx->PW, 0.0, (const cplx *)nullptr, 0.0, ctx->PW)); // A = (X - X^H) (1/hbar)
    }
    if (nv == 3) {
        // the affine terms only: a stochastic forcing's pattern belongs to a step (qf_forcing), and its counter stays
        const bool f0 = ctx->forcing_f0_on;
        if (ctx->stoch.on) ctx->forcing_f0_on = false;
        const int rc = qf_launch_forcing_affine(ctx, ctx->Phalf, W, ctx->Whalf, 1.0, 1.0);
        ctx->forcing_f0_on = f0;
        QF_TRY(rc);
    }
    const cplx *mats[3] = {W, ctx->PW, ctx->Whalf};
    cplx *z[3] = {ctx->sh_stage + 3 * half, ctx->Whalf, ctx->stage};
    double *omega[3] = {ctx->sh_omega, ctx->sh_omega + NN, reinterpret_cast<double *>(ctx->sh_stage)};
    double *sums = reinterpret_cast<double *>(ctx->sh_stage + half);
    ctx->sh_shr_count = 0;
    QF_TRY(qf_launch_degree_budget(ctx, Nmax, nv, mats, z, omega, sums));
    const size_t LL = (size_t)Nmax * Nmax;
    QF_HIP(hipMemcpyAsync(out, sums, (size_t)nv * Nmax * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    for (int v = 0; coeffs && v < nv; ++v)
        QF_HIP(hipMemcpyAsync(coeffs + v * LL, omega[v], LL * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sh_shr_count = (long long)LL;     // ctx->sh_omega starts with mat2shr of the state, band-limited to Nmax
    return QF_OK;
}

int qf_spectral_budget(qf_ctx *ctx, const void *W_host, int Nmax, double *out, double *coeffs)
{
    const int nv = (ctx && ctx->forcing_on) ? 3 : 2;
    QF_TRY(budget_run(ctx, "qf_spectral_budget", W_host, Nmax, nv, out, coeffs));
    if (nv == 2) {      // no forcing: I = 0, f = 0
        const size_t LL = (size_t)Nmax * Nmax;
        for (int l = 0; l < Nmax; ++l) out[2 * (size_t)Nmax + l] = 0.0;
        for (size_t i = 0; coeffs && i < LL; ++i) coeffs[2 * LL + i] = 0.0;
    }
    return QF_OK;
}

int qf_degree_spectrum(qf_ctx *ctx, const void *W_host, int Nmax, double *Z)
{
    return budget_run(ctx, "qf_degree_spectrum", W_host, Nmax, 1, Z, nullptr);
}

// ---- spherical-harmonic synthesis (quflow/transforms.py:220-268, 422-438; kernels in sht.hip) ----------------
static int sht_args(const char *who, long long n_omega, int L, const void *f_host)
{
    if (L < 1 || L > 8192) {
        qf_set_error("%s: bandwidth L=%d is outside 1..8192", who, L);
        return QF_ERR_INVALID;
    }
    if (n_omega < 1) {
        qf_set_error("%s: empty coefficient array (n_omega=%lld)", who, n_omega);
        return QF_ERR_INVALID;
    }
    if (!f_host) {
        qf_set_error("%s: null output grid", who);
        return QF_ERR_INVALID;
    }
    return QF_OK;
}

// ctx->sht grown to what (L, isreal) needs; a buffer that is too small is replaced (hipFree waits for the device)
static int sht_reserve_bytes(qf_ctx *ctx, const size_t want[8]);

static int sht_reserve(qf_ctx *ctx, int L, int isreal, bool analysis = false)
{
    size_t want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (analysis) qf_sht_analysis_sizes(L, isreal, want);
    else qf_sht_sizes(L, isreal, want);
    return sht_reserve_bytes(ctx, want);
}

static int sht_reserve_bytes(qf_ctx *ctx, const size_t want[8])
{
    qf_sht &S = ctx->sht;
    void **bufs[8] = {(void **)&S.omega, (void **)&S.tab, (void **)&S.col, (void **)&S.At, (void **)&S.tw, (void **)&S.f,
                      (void **)&S.H, (void **)&S.Q};
    for (int i = 0; i < 8; ++i) {
        if (want[i] <= S.cap[i]) continue;
        if (*bufs[i]) (void)hipFree(*bufs[i]);
        *bufs[i] = nullptr;
        S.cap[i] = 0;
        if (i == 7) S.q_L = 0;
        QF_HIP(hipMalloc(bufs[i], want[i]));
        S.cap[i] = want[i];
    }
    return QF_OK;
}

// The per-degree and per-order constants, in long double on the host (O(L)):
//   tab[l]     = sqrt(4 pi) w_l,  w_l^2 = prod_{j=1..l} (L-j)/(L+j) -- berezin_multipliers(L) (utils.py:108-135, whose
//                lgamma form is this product), or 1 without Berezin;
//   tab[L + m] = lambda_mm(theta) / sin^m(theta) = (-1)^m sqrt((2m+1)/(4 pi) prod_{k=1..m} (2k-1)/(2k)).
static void sht_multiplier_row(int L, int berezin, double *row)
{
    const long double fourpi = 4.0L * 3.141592653589793238462643383279502884L;
    const long double rt4pi = std::sqrt(fourpi);
    long double q = 1.0L;
    for (int l = 0; l < L; ++l) {
        if (l > 0) q *= (long double)(L - l) / (long double)(L + l);
        row[l] = (double)(berezin ? rt4pi * std::sqrt(q) : rt4pi);
    }
}

static void sht_seed_row(int L, double *row)
{
    const long double fourpi = 4.0L * 3.141592653589793238462643383279502884L;
    long double prod = 1.0L;
    for (int m = 0; m < L; ++m) {
        if (m > 0) prod *= (long double)(2 * m - 1) / (long double)(2 * m);
        const double v = (double)std::sqrt((long double)(2 * m + 1) / fourpi * prod);
        row[m] = (m & 1) ? -v : v;
    }
}

static int sht_tables(qf_ctx *ctx, int L, int berezin)
{
    std::vector<double> tab(2 * (size_t)L);
    sht_multiplier_row(L, berezin, tab.data());
    sht_seed_row(L, tab.data() + L);
    QF_HIP(hipMemcpyAsync(ctx->sht.tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));     // (tab is gone at return)
    return QF_OK;
}

static int sht_run(qf_ctx *ctx, const void *omega_host, const double *omega_dev, long long n_valid, int L, int berezin, int shr,
                   int isreal, void *f_host)
{
    QF_TRY(sht_reserve(ctx, L, isreal));
    QF_TRY(sht_tables(ctx, L, berezin));
    if (omega_host) {
        QF_HIP(hipMemcpyAsync(ctx->sht.omega, omega_host, (size_t)n_valid * (shr ? sizeof(double) : sizeof(cplx)),
                              hipMemcpyHostToDevice, ctx->stream));
        omega_dev = ctx->sht.omega;
    }
    QF_TRY(qf_launch_sht_synth(ctx, L, shr, isreal, omega_dev, n_valid));
    const size_t bytes = (size_t)L * (2 * (size_t)L - 1) * (isreal ? sizeof(double) : sizeof(cplx));
    QF_HIP(hipMemcpyAsync(f_host, ctx->sht.f, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_shr2fun(qf_ctx *ctx, const double *omega_host, long long n_omega, int L, int berezin, double *f_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(sht_args("qf_shr2fun", n_omega, L, f_host));
    long long n = n_omega;
    if (!omega_host) {
        if (!ctx->sh_omega || ctx->sh_shr_count < 1) {
            qf_set_error("qf_shr2fun: omega == NULL, but no qf_mat2shr has left real coefficients on this context");
            return QF_ERR_STATE;
        }
        n = std::min(n, ctx->sh_shr_count);
    }
    // shr2shc (transforms.py:310-349) converts whole degrees only -- a last degree cut short stays zero -- and shc2fun
    // then trims or pads to L^2: the entries below min(E^2, L^2), E^2 the largest square <= n, are used
    long long e = (long long)std::sqrt((double)n);
    while (e * e > n) --e;
    while ((e + 1) * (e + 1) <= n) ++e;
    n = std::min(e * e, (long long)L * L);
    return sht_run(ctx, omega_host, ctx->sh_omega, n, L, berezin, 1, 1, f_host);
}

int qf_shc2fun(qf_ctx *ctx, const void *omega_host, long long n_omega, int L, int berezin, int isreal, void *f_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(sht_args("qf_shc2fun", n_omega, L, f_host));
    if (!omega_host) {
        qf_set_error("qf_shc2fun: null coefficient array");
        return QF_ERR_INVALID;
    }
    const long long n = std::min(n_omega, (long long)L * L);
    return sht_run(ctx, omega_host, nullptr, n, L, berezin, 0, isreal ? 1 : 0, f_host);
}

// ---- function-space output of a state (include/quflow_hip.h): mat2shr once, one stacked synthesis per bandwidth
int qf_state_fields(qf_ctx *ctx, const void *W_host, int nfields, const qf_field *fields, void *const *f_host)
{
    QF_TRY(check_ctx(ctx));
    const char *who = "qf_state_fields";
    constexpr int MAXF = 8, MAXG = 4;
    if (nfields < 1 || nfields > MAXF) {
        qf_set_error("%s: %d fields (1..%d in all, at most %d of one bandwidth)", who, nfields, MAXF, MAXG);
        return QF_ERR_INVALID;
    }
    if (!fields || !f_host) {
        qf_set_error("%s: null field list", who);
        return QF_ERR_INVALID;
    }
    // the groups: fields of one bandwidth, in the order of their first member
    struct group {
        int L, nf, idx[MAXG];
    } groups[MAXF];
    int ngroups = 0, Lmax = 0;
    long long nvalid[MAXF];
    for (int i = 0; i < nfields; ++i) {
        const qf_field &fd = fields[i];
        if (fd.n_omega < 1) {
            qf_set_error("%s: field %d: empty coefficient array (n_omega=%lld)", who, i, fd.n_omega);
            return QF_ERR_INVALID;
        }
        if (fd.dtype != 0 && fd.dtype != 1) {
            qf_set_error("%s: field %d: dtype %d (0 = float64, 1 = float32)", who, i, fd.dtype);
            return QF_ERR_INVALID;
        }
        if (!f_host[i]) {
            qf_set_error("%s: field %d: null output grid", who, i);
            return QF_ERR_INVALID;
        }
        // whole degrees only, as qf_shr2fun: E^2 the largest square <= n_omega enters, the bandwidth is E, or E + 1 when
        // n_omega is no square (the last degree, cut short, stays zero)
        long long e = (long long)std::sqrt((double)fd.n_omega);
        while (e * e > fd.n_omega) --e;
        while ((e + 1) * (e + 1) <= fd.n_omega) ++e;
        const long long L = e * e == fd.n_omega ? e : e + 1;
        if (L > ctx->N || L > 8192) {      // (8192: the synthesis kernels' limit, as in sht_args)
            qf_set_error("%s: field %d: bandwidth L=%lld of n_omega=%lld exceeds %s", who, i, L, fd.n_omega,
                         L > ctx->N ? "the context's N" : "8192");
            return QF_ERR_INVALID;
        }
        nvalid[i] = e * e;
        int g = 0;
        while (g < ngroups && groups[g].L != (int)L) ++g;
        if (g == ngroups) {
            groups[ngroups].L = (int)L;
            groups[ngroups].nf = 0;
            ++ngroups;
        }
        if (groups[g].nf == MAXG) {
            qf_set_error("%s: field %d: more than %d fields of bandwidth L=%lld", who, i, MAXG, L);
            return QF_ERR_INVALID;
        }
        groups[g].idx[groups[g].nf++] = i;
        Lmax = std::max(Lmax, (int)L);
    }
    if (!W_host && ctx->c64 && !ctx->w_c128_set) {
        qf_set_error("%s: this context holds a complex64 state only; the fields are double precision (pass W_host)", who);
        return QF_ERR_STATE;
    }
    // Resident basis: a column of the sweep is summed over its rows in an order that does not depend on the band limit, so
    // the leading L^2 coefficients of the sweep to Lmax are those of the sweep to L, bit for bit: one sweep serves every
    // bandwidth.  Streamed basis: the blocks are generated per band limit; one sweep per bandwidth, as qf_mat2shr does.
    const bool one_sweep = ctx->slab_budget == 0;
    if (!one_sweep)
        for (int g = 0; g < ngroups; ++g) {       // (the slab plan's refusal comes before anything is launched)
            std::vector<int> first;
            long long need = 0;
            QF_TRY(qf_slab_plan(ctx->N, groups[g].L, ctx->slab_budget, first, &need));
        }
    QF_TRY(need_source(ctx, who));
    size_t want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < ngroups; ++g) {
        size_t b[6];
        qf_sht_fields_sizes(groups[g].L, groups[g].nf, b);
        for (int i = 0; i < 6; ++i) want[i] = std::max(want[i], b[i]);
    }
    want[0] = 0;      // (the coefficients stay in ctx->sh_omega)
    QF_TRY(sht_reserve_bytes(ctx, want));
    const size_t NN = (size_t)ctx->N * ctx->N;
    const cplx *src = ctx->W;
    if (W_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, W_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
        src = ctx->stage;
    }
    ctx->sh_shr_count = 0;
    // the host tables are the pageable sources of asynchronous copies: they live until the stream is synchronised, which
    // happens below on the error path too
    std::vector<double> tabs[MAXF];
    auto enqueue = [&]() -> int {
    for (int g = 0; g < ngroups; ++g) {
        const int L = groups[g].L, nf = groups[g].nf;
        if (g == 0 || !one_sweep) {
            const int Ls = one_sweep ? Lmax : L;
            ctx->sh_shr_count = 0;
            QF_HIP(hipMemsetAsync(ctx->sh_omega, 0, (size_t)Ls * Ls * sizeof(double), ctx->stream));
            QF_TRY(qf_launch_mat2shr(ctx, Ls, src, ctx->sh_omega));
            ctx->sh_shr_count = (long long)Ls * Ls;
        }
        std::vector<double> &tab = tabs[g];
        tab.resize(((size_t)nf + 1) * L);
        long long n[MAXG] = {0, 0, 0, 0};
        unsigned f32mask = 0;
        for (int f = 0; f < nf; ++f) {
            const qf_field &fd = fields[groups[g].idx[f]];
            sht_multiplier_row(L, fd.berezin, tab.data() + (size_t)f * L);
            n[f] = nvalid[groups[g].idx[f]];
            if (fd.dtype == 1) f32mask |= 1u << f;
        }
        sht_seed_row(L, tab.data() + (size_t)nf * L);
        QF_HIP(hipMemcpyAsync(ctx->sht.tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QF_TRY(qf_launch_sht_fields(ctx, L, nf, n, f32mask, ctx->sh_omega));
        const size_t slot = (size_t)L * (2 * (size_t)L - 1);
        for (int f = 0; f < nf; ++f) {
            const int i = groups[g].idx[f];
            QF_HIP(hipMemcpyAsync(f_host[i], ctx->sht.f + (size_t)f * slot, slot * (fields[i].dtype == 1 ? sizeof(float) : sizeof(double)),
                                  hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    return QF_OK;
    };
    const int rc = enqueue();
    if (rc != QF_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_shr_held(qf_ctx *ctx, double *omega_host, long long n_omega)
{
    QF_TRY(check_ctx(ctx));
    if (!omega_host || n_omega < 1) {
        qf_set_error("qf_shr_held: null or empty output (n_omega=%lld)", n_omega);
        return QF_ERR_INVALID;
    }
    if (!ctx->sh_omega || ctx->sh_shr_count < n_omega) {
        qf_set_error("qf_shr_held: the device copy holds %lld real coefficients, %lld were asked for", ctx->sh_omega ? ctx->sh_shr_count : 0LL,
                     n_omega);
        return QF_ERR_STATE;
    }
    QF_HIP(hipMemcpyAsync(omega_host, ctx->sh_omega, (size_t)n_omega * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

// ---- spherical-harmonic analysis (quflow/transforms.py:189-217, 404-419; kernels in sht.hip) ------------------
// f_host (L, 2L-1) -> L^2 coefficients: real (shr) or complex.  out_dev == NULL: into ctx->sht.omega; the result goes to
// omega_host when that is given.  Q_even / Q_odd are rebuilt when the bandwidth differs from the one they were made for.
static int sht_analyse(qf_ctx *ctx, const char *who, const void *f_host, int L, int isreal, int shr, double *out_dev,
                       void *omega_host)
{
    if (L < 1 || L > 8192) {
        qf_set_error("%s: bandwidth L=%d is outside 1..8192", who, L);
        return QF_ERR_INVALID;
    }
    if (!f_host) {
        qf_set_error("%s: null grid", who);
        return QF_ERR_INVALID;
    }
    QF_TRY(sht_reserve(ctx, L, isreal, true));
    QF_TRY(sht_tables(ctx, L, 0));
    if (ctx->sht.q_L != L) QF_TRY(qf_launch_sht_qbuild(ctx, L));     // (uses f as workspace: before the upload)
    const size_t LL = (size_t)L * L;
    QF_HIP(hipMemcpyAsync(ctx->sht.f, f_host, (size_t)L * (2 * (size_t)L - 1) * (isreal ? sizeof(double) : sizeof(cplx)),
                          hipMemcpyHostToDevice, ctx->stream));
    if (!out_dev) out_dev = ctx->sht.omega;
    QF_TRY(qf_launch_sht_analysis(ctx, L, shr, isreal, out_dev));
    if (omega_host)
        QF_HIP(hipMemcpyAsync(omega_host, out_dev, LL * (shr ? sizeof(double) : sizeof(cplx)), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_fun2shc(qf_ctx *ctx, const void *f_host, int L, int isreal, void *omega_host)
{
    QF_TRY(check_ctx(ctx));
    if (!omega_host) {
        qf_set_error("qf_fun2shc: null coefficient array");
        return QF_ERR_INVALID;
    }
    return sht_analyse(ctx, "qf_fun2shc", f_host, L, isreal ? 1 : 0, 0, nullptr, omega_host);
}

int qf_fun2shr(qf_ctx *ctx, const void *f_host, int L, int isreal, double *omega_host)
{
    QF_TRY(check_ctx(ctx));
    if (omega_host) return sht_analyse(ctx, "qf_fun2shr", f_host, L, isreal ? 1 : 0, 1, nullptr, omega_host);
    // omega_host == NULL: the coefficients stay in ctx->sh_omega, where qf_shr2mat(NULL) and qf_shr2fun(NULL) read them
    if (L > ctx->N) {
        qf_set_error("qf_fun2shr: omega == NULL keeps L^2 coefficients on a context of N^2: L=%d exceeds N=%d", L, ctx->N);
        return QF_ERR_INVALID;
    }
    QF_TRY(alloc_stage(ctx));
    ctx->sh_shr_count = 0;
    QF_TRY(sht_analyse(ctx, "qf_fun2shr", f_host, L, isreal ? 1 : 0, 1, ctx->sh_omega, nullptr));
    ctx->sh_shr_count = (long long)L * L;
    return QF_OK;
}


int qf_zgemm_i8(qf_ctx *ctx, const void *A_host, const void *B_host, void *C_host)
{
    QF_TRY(check_ctx(ctx));
    if (!A_host || !B_host || !C_host) {
        qf_set_error("qf_zgemm_i8: null buffer");
        return QF_ERR_INVALID;
    }
    if (ctx->N % 64 != 0) {
        qf_set_error("qf_zgemm_i8: N=%d is not a multiple of 64", ctx->N);
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_oz_alloc(ctx));
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stage, A_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipMemcpyAsync(ctx->Phalf, B_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    qf_oz_jobs jobs;
    jobs.n = 2;
    jobs.j[0].X = ctx->stage;
    jobs.j[0].planes = ctx->oz_planes[0];
    jobs.j[0].scale = ctx->oz_scale[0];
    jobs.j[1].X = ctx->Phalf;                  // B skew-Hermitian, sliced by rows like A (ozaki.hip)
    jobs.j[1].planes = ctx->oz_planes[1];
    jobs.j[1].scale = ctx->oz_scale[1];
    QF_TRY(qf_launch_oz_slice(ctx, jobs));
    QF_TRY(qf_launch_oz_gemm(ctx, ctx->oz_planes[0], ctx->oz_scale[0], ctx->oz_planes[1], ctx->oz_scale[1], ctx->PW));
    QF_HIP(hipMemcpyAsync(C_host, ctx->PW, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_zgemm(qf_ctx *ctx, const void *A_host, const void *B_host, void *C_host)
{
    QF_TRY(check_ctx(ctx));
    if (!A_host || !B_host || !C_host) {
        qf_set_error("qf_zgemm: null buffer");
        return QF_ERR_INVALID;
    }
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stage, A_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipMemcpyAsync(ctx->Phalf, B_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_zgemm(ctx, ctx->stage, ctx->Phalf, ctx->PW, nullptr));
    QF_HIP(hipMemcpyAsync(C_host, ctx->PW, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

// commutator_skewherm / commutator_generic (isospectral.py:22-57) with the combination on the device: the staging
// matrices of the context (stage, Phalf, PW, Whalf) are per-iteration temporaries, free between stepper calls
int qf_commutator(qf_ctx *ctx, const void *W_host, const void *P_host, void *C_host, int skewherm)
{
    QF_TRY(check_ctx(ctx));
    if (!W_host || !P_host || !C_host) {
        qf_set_error("qf_commutator: null buffer");
        return QF_ERR_INVALID;
    }
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipMemcpyAsync(ctx->Phalf, P_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_zgemm(ctx, ctx->stage, ctx->Phalf, ctx->PW, nullptr));                       // X = W @ P
    if (skewherm) {
        QF_TRY(qf_launch_neg_conj_transpose(ctx, ctx->PW, ctx->Whalf));                            // -X^H
        QF_TRY(qf_launch_lincomb(ctx, 1.0, ctx->PW, 1.0, ctx->Whalf, 0.0, ctx->PW));               // X - X^H      (:52)
    } else {
        QF_TRY(qf_launch_zgemm(ctx, ctx->Phalf, ctx->stage, ctx->Whalf, nullptr));                 // P @ W
        QF_TRY(qf_launch_lincomb(ctx, 1.0, ctx->PW, -1.0, ctx->Whalf, 0.0, ctx->PW));              // W @ P - P @ W (:33-34)
    }
    QF_HIP(hipMemcpyAsync(C_host, ctx->PW, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}


int qf_cgemm(qf_ctx *ctx, const void *A_host, const void *B_host, void *C_host)
{
    QF_TRY(qf_need_c64(ctx));
    if (!A_host || !B_host || !C_host) {
        qf_set_error("qf_cgemm: null buffer");
        return QF_ERR_INVALID;
    }
    qf_c64 *f = ctx->c64;
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(float2);
    QF_HIP(hipMemcpyAsync(f->stage, A_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipMemcpyAsync(f->Phalf, B_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_cgemm(ctx, f->stage, f->Phalf, f->PW, nullptr));
    QF_HIP(hipMemcpyAsync(C_host, f->PW, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}


}  // extern "C"
