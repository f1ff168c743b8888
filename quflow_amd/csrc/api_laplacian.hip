// C ABI of libquflow_hip.so, part 2 of 5: the LAPLACIAN backend -- coefficient tables, solve_poisson / laplace, the
// cached factorisations of caller-supplied tridiagonal tables (solve_heat / helmholtz / viscdamp / globalqg), the
// diagnostics that need a solve, and the same entry points for complex64 data (float32 arithmetic).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <chrono>

#include "qf_api.h"

namespace {
// fingerprint of a caller's array of n doubles: 4096 entries spread over it and the last one (FNV-1a over their bit
// patterns).  A key is a caller-side hash; the fingerprint catches a key that returns with different content.
unsigned long long sample_fingerprint(const double *a, size_t n)
{
    unsigned long long fp = 1469598103934665603ull;
    const size_t stride = n / 4096 ? n / 4096 : 1;
    for (size_t i = 0; i < n; i += stride) {
        unsigned long long bits;
        memcpy(&bits, a + i, sizeof(bits));
        fp = (fp ^ bits) * 1099511628211ull;
    }
    unsigned long long bits;
    memcpy(&bits, a + (n - 1), sizeof(bits));
    fp = (fp ^ bits) * 1099511628211ull;
    return fp;
}
}  // namespace

extern "C" {

int qf_laplacian_table(qf_ctx *ctx, int bc, double *lap_host)
{
    QF_TRY(check_ctx(ctx));
    if (!lap_host) {
        qf_set_error("qf_laplacian_table: null output");
        return QF_ERR_INVALID;
    }
    const size_t bytes = 2 * (size_t)ctx->N * ctx->N * sizeof(double);
    double *dst = ctx->lap;
    if (!bc) {
        if (!ctx->lap_user) QF_HIP(hipMalloc((void **)&ctx->lap_user, bytes));
        dst = ctx->lap_user;
        QF_TRY(qf_launch_lap_table(ctx, 0, dst));
    }
    QF_HIP(hipMemcpyAsync(lap_host, dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_solve_poisson(qf_ctx *ctx, const void *W_host, void *P_host, int skewh)
{
    QF_TRY(check_ctx(ctx));
    if (!W_host || !P_host) {
        qf_set_error("qf_solve_poisson: null buffer");
        return QF_ERR_INVALID;
    }
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_solve(ctx, ctx->poisson, ctx->stage, ctx->Phalf, 1.0, skewh));
    QF_HIP(hipMemcpyAsync(P_host, ctx->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_laplace(qf_ctx *ctx, const void *P_host, void *W_host)
{
    QF_TRY(check_ctx(ctx));
    if (!W_host || !P_host) {
        qf_set_error("qf_laplace: null buffer");
        return QF_ERR_INVALID;
    }
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stage, P_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_laplace(ctx, ctx->stage, ctx->Phalf));
    QF_HIP(hipMemcpyAsync(W_host, ctx->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_solve_tridiagonal(qf_ctx *ctx, const double *lap_host, unsigned long long table_key,
                         const void *W_host, void *P_host, int skewh)
{
    QF_TRY(check_ctx(ctx));
    const bool resident = !W_host && !P_host;     // on the context's state, in place
    if (!lap_host || (!resident && (!W_host || !P_host))) {
        qf_set_error("qf_solve_tridiagonal: null buffer");
        return QF_ERR_INVALID;
    }
    const size_t NN = (size_t)ctx->N * ctx->N;
    const unsigned long long fp = sample_fingerprint(lap_host, 2 * NN);
    qf_factors f;
    auto it = ctx->user_factors.find(table_key);
    const bool hit = table_key != 0 && it != ctx->user_factors.end() && it->second.fingerprint == fp;
    if (hit) {
        f = it->second.f;
        it->second.last_used = ++ctx->factor_clock;
    } else {
        if (!ctx->lap_user) QF_HIP(hipMalloc((void **)&ctx->lap_user, 2 * NN * sizeof(double)));
        if (it != ctx->user_factors.end()) {
            f = it->second.f;                    // same key (or the anonymous slot 0), other table: refactor in place
        } else {
            // new key: a fresh pair while the budget lasts, else the least recently used entry's buffers
            // (no hipFree: work queued on the stream may still read them, and the stream orders the reuse)
            const size_t entry_bytes = 2 * NN * sizeof(double);
            if ((ctx->user_factors.size() + 1) * entry_bytes > ctx->factor_budget_bytes && !ctx->user_factors.empty()) {
                auto lru = ctx->user_factors.begin();
                for (auto jt = ctx->user_factors.begin(); jt != ctx->user_factors.end(); ++jt)
                    if (jt->second.last_used < lru->second.last_used) lru = jt;
                f = lru->second.f;
                ctx->user_factors.erase(lru);
            } else {
                QF_TRY(alloc_factors(ctx, &f));
            }
        }
        qf_ctx::factor_entry &e = ctx->user_factors[table_key];
        e.f = f;
        e.fingerprint = fp;
        e.last_used = ++ctx->factor_clock;
        QF_HIP(hipMemcpyAsync(ctx->lap_user, lap_host, 2 * NN * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        QF_TRY(qf_launch_build_factors(ctx, ctx->lap_user, f));
        // (lap_host must stay valid until the copy has been queued from pageable memory: hipMemcpyAsync
        // from pageable memory returns after staging, so the caller's buffer is free on return)
    }
    if (resident) {     // W <- T^-1 W (a Strang half step of a viscous / damped run between device steps)
        // (a carried increment stays, as through qf_upload_W: the reference's dW lives through strang_splitting,
        // isospectral.py:466-482; only `stage` is written besides W)
        if (!skewh) ctx->w_skew_known = false;   // (the skew-Hermitian solve mirrors exactly: the property survives)
        QF_HIP(hipMemcpyAsync(ctx->stage, ctx->W, NN * sizeof(cplx), hipMemcpyDeviceToDevice, ctx->stream));
        QF_TRY(qf_launch_solve(ctx, f, ctx->stage, ctx->W, 1.0, skewh));
        return QF_OK;
    }
    QF_HIP(hipMemcpyAsync(ctx->stage, W_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_solve(ctx, f, ctx->stage, ctx->Phalf, 1.0, skewh));
    QF_HIP(hipMemcpyAsync(P_host, ctx->Phalf, NN * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

// ---- the installed Hamiltonian of the flow (include/quflow_hip.h; launched through qf_launch_hamiltonian, poisson.hip)
int qf_set_hamiltonian(qf_ctx *ctx, const double *table_host, unsigned long long table_key, const void *offset_host,
                       unsigned long long offset_key)
{
    QF_TRY(check_ctx(ctx));
    const size_t NN = (size_t)ctx->N * ctx->N;
    // nothing is in force until both parts are in place: an error below leaves the built-in Hamiltonian
    ctx->ham_table = false;
    ctx->ham_offset_on = false;
    if (table_host) {
        const unsigned long long fp = sample_fingerprint(table_host, 2 * NN);
        if (!(ctx->ham.tab && table_key != 0 && ctx->ham_key == table_key && ctx->ham_fp == fp)) {
            if (!ctx->ham.tab) QF_TRY(alloc_factors(ctx, &ctx->ham));
            if (!ctx->lap_user) QF_HIP(hipMalloc((void **)&ctx->lap_user, 2 * NN * sizeof(double)));
            ctx->ham_key = 0;      // (what the pair holds is undefined until the factorisation has been queued)
            // (pageable source: hipMemcpyAsync returns after staging, the caller's table is free on return)
            QF_HIP(hipMemcpyAsync(ctx->lap_user, table_host, 2 * NN * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            QF_TRY(qf_launch_build_factors(ctx, ctx->lap_user, ctx->ham));
            ctx->ham_key = table_key;
            ctx->ham_fp = fp;
        }
    }
    if (offset_host) {
        const unsigned long long fp = sample_fingerprint(static_cast<const double *>(offset_host), 2 * NN);
        if (!(ctx->ham_offset && offset_key != 0 && ctx->ham_offset_key == offset_key && ctx->ham_offset_fp == fp)) {
            if (!ctx->ham_offset) QF_HIP(hipMalloc((void **)&ctx->ham_offset, NN * sizeof(cplx)));
            ctx->ham_offset_key = 0;
            QF_HIP(hipMemcpyAsync(ctx->ham_offset, offset_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
            ctx->ham_offset_key = offset_key;
            ctx->ham_offset_fp = fp;
        }
    }
    ctx->ham_table = table_host != nullptr;
    ctx->ham_offset_on = offset_host != nullptr;
    return QF_OK;
}

int qf_clear_hamiltonian(qf_ctx *ctx)
{
    QF_TRY(check_ctx(ctx));
    ctx->ham_table = false;
    ctx->ham_offset_on = false;
    return QF_OK;
}

int qf_hamiltonian(qf_ctx *ctx, const void *W_host, void *P_host)
{
    QF_TRY(check_ctx(ctx));
    if (!W_host || !P_host) {
        qf_set_error("qf_hamiltonian: null buffer");
        return QF_ERR_INVALID;
    }
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_hamiltonian(ctx, ctx->stage, ctx->Phalf, 1.0));
    QF_HIP(hipMemcpyAsync(P_host, ctx->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_hamiltonian_energy(qf_ctx *ctx, double *H)
{
    QF_TRY(check_ctx(ctx));
    if (!H) {
        qf_set_error("qf_hamiltonian_energy: null output");
        return QF_ERR_INVALID;
    }
    // D = W - F once (stage), P = T^-1 D (Phalf), then <P, D>: the sum the definition names, no difference of two sums
    const cplx *D = ctx->W;
    if (ctx->ham_offset_on) {
        QF_TRY(qf_launch_lincomb(ctx, 1.0, ctx->W, -1.0, ctx->ham_offset, 0.0, ctx->stage));
        D = ctx->stage;
    }
    QF_TRY(qf_launch_solve(ctx, ctx->ham_table ? ctx->ham : ctx->poisson, D, ctx->Phalf, 1.0, 1));
    QF_TRY(qf_launch_inner(ctx, ctx->Phalf, D, ctx->scalars + 2));
    double pd = 0.0;
    QF_TRY(read_scalar(ctx, ctx->scalars + 2, &pd));
    *H = -(pd / ctx->N) / 2.0;
    return QF_OK;
}

// ---- the installed forcing of the flow (include/quflow_hip.h; applied by qf_launch_forcing_affine, hooks.hip)
int qf_set_forcing(qf_ctx *ctx, const void *F0_host, unsigned long long F0_key, double a_W, double a_P, double a_lap)
{
    QF_TRY(check_ctx(ctx));
    if (!QF_FINITE(a_W) || !QF_FINITE(a_P) || !QF_FINITE(a_lap)) {
        qf_set_error("qf_set_forcing: the coefficients must be finite (a_W=%g, a_P=%g, a_lap=%g)", a_W, a_P, a_lap);
        return QF_ERR_INVALID;
    }
    const size_t NN = (size_t)ctx->N * ctx->N;
    ctx->forcing_on = false;       // nothing is in force until the pattern is in place
    ctx->stoch.on = false;         // (an affine forcing replaces a stochastic one)
    if (F0_host) {
        const unsigned long long fp = sample_fingerprint(static_cast<const double *>(F0_host), 2 * NN);
        if (!(ctx->forcing_f0 && F0_key != 0 && ctx->forcing_key == F0_key && ctx->forcing_fp == fp)) {
            if (!ctx->forcing_f0) QF_HIP(hipMalloc((void **)&ctx->forcing_f0, NN * sizeof(cplx)));
            ctx->forcing_key = 0;
            // (pageable source: hipMemcpyAsync returns after staging, the caller's matrix is free on return)
            QF_HIP(hipMemcpyAsync(ctx->forcing_f0, F0_host, NN * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
            ctx->forcing_key = F0_key;
            ctx->forcing_fp = fp;
        }
    }
    ctx->forcing_f0_on = F0_host != nullptr;
    ctx->forcing_aW = a_W;
    ctx->forcing_aP = a_P;
    ctx->forcing_alap = a_lap;
    ctx->forcing_on = true;
    return QF_OK;
}

int qf_clear_forcing(qf_ctx *ctx)
{
    QF_TRY(check_ctx(ctx));
    ctx->forcing_on = false;
    ctx->forcing_f0_on = false;
    ctx->stoch.on = false;
    return QF_OK;
}

int qf_forcing(qf_ctx *ctx, const void *P_host, const void *W_host, void *F_host)
{
    QF_TRY(check_ctx(ctx));
    const bool on_device = !P_host && !W_host && !F_host;
    if (!on_device && (!P_host || !W_host || !F_host)) {
        qf_set_error("qf_forcing: null buffer");
        return QF_ERR_INVALID;
    }
    if (!ctx->forcing_on) {
        qf_set_error("qf_forcing: no forcing is installed (qf_set_forcing)");
        return QF_ERR_STATE;
    }
    if (ctx->stoch.on) {
        qf_set_error("qf_forcing: a stochastic forcing is installed (qf_set_stochastic_forcing): its pattern belongs to a step, "
                     "a bare evaluation has none (qf_stochastic_pattern gives the pattern of a step)");
        return QF_ERR_UNSUPPORTED;
    }
    if (on_device)      // the kernel alone, queued on the stream: resident state, the stream-matrix buffer as it stands
        return qf_launch_forcing_affine(ctx, ctx->Phalf, ctx->W, ctx->PW, 1.0, 1.0);
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->Phalf, P_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_HIP(hipMemcpyAsync(ctx->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_forcing_affine(ctx, ctx->Phalf, ctx->stage, ctx->PW, 1.0, 1.0));
    QF_HIP(hipMemcpyAsync(F_host, ctx->PW, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_factor_cache_stats(qf_ctx *ctx, int *entries, unsigned long long *device_bytes)
{
    QF_TRY(check_ctx(ctx));
    if (entries) *entries = (int)ctx->user_factors.size();
    if (device_bytes) *device_bytes = (unsigned long long)ctx->user_factors.size() * 2ull * ctx->N * ctx->N * sizeof(double);
    return QF_OK;
}


int qf_diagnostics(qf_ctx *ctx, double *energy_euler, double *enstrophy)
{
    QF_TRY(check_ctx(ctx));
    const int N = ctx->N;
    // P = solve_poisson(W); energy = -inner_L2(W, P)/2; enstrophy = inner_L2(W, W)/2
    QF_TRY(qf_enqueue_diagnostics(ctx));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    const double wp = ctx->host_scalars[0], ww = ctx->host_scalars[1];
    if (energy_euler) *energy_euler = -(wp / N) / 2.0;
    if (enstrophy) *enstrophy = (ww / N) / 2.0;
    return QF_OK;
}


// ---- complex64 data: float32 arithmetic, as the reference computes it (cpu.py:725, isospectral.py:440-448) ----

int qf_need_c64(qf_ctx *ctx)
{
    QF_TRY(check_ctx(ctx));
    return qf_c64_alloc(ctx);
}

int qf_c64_laplacian_table(qf_ctx *ctx, int bc, float *lap_host)
{
    QF_TRY(qf_need_c64(ctx));
    if (!lap_host) {
        qf_set_error("qf_c64_laplacian_table: null buffer");
        return QF_ERR_INVALID;
    }
    qf_c64 *f = ctx->c64;
    const size_t bytes = 2 * (size_t)ctx->N * ctx->N * sizeof(float);
    // (the resident table is the bc = True one: any other goes through the staging matrix, which has the same size)
    float *dst = bc ? f->lap : reinterpret_cast<float *>(f->stage);
    if (!bc) QF_TRY(qf_launch_lap_table(ctx, 0, dst));
    QF_HIP(hipMemcpyAsync(lap_host, dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_c64_solve_poisson(qf_ctx *ctx, const void *W_host, void *P_host, int skewh)
{
    QF_TRY(qf_need_c64(ctx));
    if (!W_host || !P_host) {
        qf_set_error("qf_c64_solve_poisson: null buffer");
        return QF_ERR_INVALID;
    }
    qf_c64 *f = ctx->c64;
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(float2);
    QF_HIP(hipMemcpyAsync(f->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_solve(ctx, f->tab, f->stage, f->Phalf, 1.0f, skewh));
    QF_HIP(hipMemcpyAsync(P_host, f->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_c64_solve_tridiagonal(qf_ctx *ctx, const float *lap_host, const void *W_host, void *P_host, int skewh)
{
    QF_TRY(qf_need_c64(ctx));
    if (!lap_host || !W_host || !P_host) {
        qf_set_error("qf_c64_solve_tridiagonal: null buffer");
        return QF_ERR_INVALID;
    }
    qf_c64 *f = ctx->c64;
    const size_t NN = (size_t)ctx->N * ctx->N, bytes = NN * sizeof(float2);
    // the caller's float32 table and its factorisation live in two scratch matrices of the float32 working set
    // (no cache: this is the secondary, host-in / host-out route; a factorisation is one sequential sweep per walk)
    float *lap_dev = reinterpret_cast<float *>(f->PW);
    float2 *tab_dev = f->dW[1];
    QF_HIP(hipMemcpyAsync(lap_dev, lap_host, 2 * NN * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_build_factors(ctx, lap_dev, tab_dev));
    QF_HIP(hipMemcpyAsync(f->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_solve(ctx, tab_dev, f->stage, f->Phalf, 1.0f, skewh));
    QF_HIP(hipMemcpyAsync(P_host, f->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    f->increment_valid = false;      // (dW[1] was scratch)
    return QF_OK;
}

int qf_c64_laplace(qf_ctx *ctx, const void *P_host, void *W_host)
{
    QF_TRY(qf_need_c64(ctx));
    if (!W_host || !P_host) {
        qf_set_error("qf_c64_laplace: null buffer");
        return QF_ERR_INVALID;
    }
    qf_c64 *f = ctx->c64;
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(float2);
    QF_HIP(hipMemcpyAsync(f->stage, P_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_laplace(ctx, f->stage, f->Phalf));
    QF_HIP(hipMemcpyAsync(W_host, f->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}


int qf_c64_diagnostics(qf_ctx *ctx, double *energy_euler, double *enstrophy)
{
    QF_TRY(qf_need_c64(ctx));
    qf_c64 *f = ctx->c64;
    const int N = ctx->N;
    // P = solve_poisson(W); energy = -inner_L2(W, P)/2; enstrophy = inner_L2(W, W)/2  (physics.py:26-38)
    QF_TRY(qf_launch_solve(ctx, f->tab, f->W, f->stage, 1.0f, 1));
    QF_TRY(qf_launch_inner2(ctx, f->W, f->stage, ctx->scalars + 2));
    QF_HIP(hipMemcpyAsync(ctx->host_scalars, ctx->scalars + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    const double wp = ctx->host_scalars[0], ww = ctx->host_scalars[1];
    if (energy_euler) *energy_euler = -(wp / N) / 2.0;
    if (enstrophy) *enstrophy = (ww / N) / 2.0;
    return QF_OK;
}


}  // extern "C"
