// Shared by the api_*.hip translation units (the C ABI of include/quflow_hip.h) and hooks.hip: the per-launch event scope,
// small host helpers, and the few functions one unit defines and another calls.  Host code only.
#pragma once

#include "qf_internal.h"

#include <sched.h>

namespace {
int drain_events(qf_ctx *ctx);

struct prof_scope {
    qf_ctx *ctx;
    qf_event_pair ev;
    bool active;
    prof_scope(qf_ctx *c, int id) : ctx(c), active(((c->profile_mask >> id) & 1) != 0)
    {
        ctx->plan_role = id;       // (qf_plan_note: the launchers inside this scope describe what they launch for it)
        if (!active) return;
        // sampling: one launch in profile_stride carries the event pair (the events themselves cost
        // host time and stream slots: ~6 % of the step rate when every product launch is bracketed)
        if ((ctx->prof_seen[id]++ % ctx->profile_stride) != 0) {
            active = false;
            return;
        }
        if (ctx->events_free.empty()) {
            if (hipEventCreate(&ev.start) != hipSuccess || hipEventCreate(&ev.stop) != hipSuccess) {
                active = false;
                return;
            }
        } else {
            ev = ctx->events_free.back();
            ctx->events_free.pop_back();
        }
        ev.kernel_id = id;
        (void)hipEventRecord(ev.start, ctx->stream);
    }
    ~prof_scope()
    {
        ctx->plan_role = -1;
        if (!active) return;
        (void)hipEventRecord(ev.stop, ctx->stream);
        ctx->events_busy.push_back(ev);
        if (ctx->events_busy.size() >= 8192) (void)drain_events(ctx);
    }
};

int drain_events(qf_ctx *ctx)
{
    if (ctx->events_busy.empty()) return QF_OK;
    QF_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &ev : ctx->events_busy) {
        float ms = 0.f;
        QF_HIP(hipEventElapsedTime(&ms, ev.start, ev.stop));
        ctx->prof_launches[ev.kernel_id] += 1;
        ctx->prof_ms[ev.kernel_id] += (double)ms;
        ctx->events_free.push_back(ev);
    }
    ctx->events_busy.clear();
    return QF_OK;
}

int alloc_factors(qf_ctx *ctx, qf_factors *f)
{
    const size_t NN = (size_t)ctx->N * ctx->N;
    QF_HIP(hipMalloc((void **)&f->tab, NN * sizeof(double2)));
    return QF_OK;
}

int check_ctx(const qf_ctx *ctx)
{
    if (!ctx) {
        qf_set_error("null qf_ctx");
        return QF_ERR_INVALID;
    }
    QF_HIP(hipSetDevice(ctx->device));
    return QF_OK;
}

int read_scalar(qf_ctx *ctx, const double *dev, double *out)
{
    QF_HIP(hipMemcpyAsync(ctx->host_scalars, dev, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    *out = ctx->host_scalars[0];
    return QF_OK;
}

// the two iteration arguments of every fixed-point stepper (isospectral.py:400-401; mhd.py: the same assertions)
int check_iteration_args(int minit, int maxit)
{
    if (minit < 1) {
        qf_set_error("minit must be at least 1.");
        return QF_ERR_INVALID;
    }
    if (maxit < minit) {
        qf_set_error("maxit must be at minit.");
        return QF_ERR_INVALID;
    }
    return QF_OK;
}

// what a stepper reports; the caller may not want it
void fill_stats(qf_isomp_stats *stats_out, long long total_iterations, long long number_of_maxit, double tol, double resnorm)
{
    if (!stats_out) return;
    stats_out->total_iterations = total_iterations;
    stats_out->number_of_maxit = number_of_maxit;
    stats_out->tol_used = tol;
    stats_out->last_resnorm = resnorm;
}

// The automatic tolerance (isospectral.py:440-452): *tol = prefactor * |X|_inf, the norm through scalars[0] and one read-back.
// The prefactor is the caller's own expression, so each stepper keeps its rounding.
int auto_tolerance(qf_ctx *ctx, const cplx *X, double prefactor, double *tol)
{
    double nrm = 0.0;
    QF_TRY(qf_launch_norm_inf(ctx, X, ctx->scalars));
    QF_TRY(read_scalar(ctx, ctx->scalars, &nrm));
    *tol = prefactor * nrm;
    return QF_OK;
}

// The exit test's read-back for a stack of k states (isospectral.py:523-534).  The loops have put state j's residual norm
// into scalars[16 + j] for j < 48 and folded the states beyond those 48 slots into scalars[8] (through scalars[9]): one copy
// of min(k, 48) doubles, the fold flag when k > 48, one synchronisation.  *resnorm is state 0's norm, or with `per_state`
// (one stream matrix per state) the maximum over the states as numpy forms it (`resnormvec.max()`, :527-532: a NaN wins).
// scipy.linalg.norm checks the WHOLE stack for infs / NaNs before it reduces (check_finite, :528, :534): a norm that is
// not finite, of a passively advected state too, is the error it raises.
int read_stack_resnorm(qf_ctx *ctx, int k, bool per_state, double *resnorm)
{
    const int kk = k < 48 ? k : 48;
    QF_HIP(hipMemcpyAsync(ctx->host_scalars, ctx->scalars + 16, (size_t)kk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (k > 48) QF_HIP(hipMemcpyAsync(ctx->host_scalars + 48, ctx->scalars + 8, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    double r0 = ctx->host_scalars[0];
    bool finite = QF_FINITE(r0) && (k <= 48 || QF_FINITE(ctx->host_scalars[48]));
    for (int j = 1; j < kk; ++j) {
        const double r = ctx->host_scalars[j];
        finite = finite && QF_FINITE(r);
        if (per_state && r > r0) r0 = r;
    }
    if (!finite) {
        qf_set_error("array must not contain infs or NaNs");
        return QF_ERR_NONFINITE;
    }
    *resnorm = r0;
    return QF_OK;
}

// *out = X is exactly skew-Hermitian (max_ij |X[i,j] + conj(X[j,i])| == 0): what lets a product stand for its mirror image
int qf_exactly_skew(qf_ctx *ctx, const cplx *X, bool *out)
{
    QF_TRY(qf_launch_skew_defect(ctx, X, ctx->scalars + 4));
    QF_HIP(hipMemcpyAsync(ctx->host_scalars, ctx->scalars + 4, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    *out = (ctx->host_scalars[0] == 0.0);
    return QF_OK;
}

// `v` (ctx->multi or ctx->stack) holds at least `count` N x N device matrices: grown on demand, kept
int qf_need_matrices(qf_ctx *ctx, std::vector<cplx *> &v, size_t count)
{
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    while (v.size() < count) {
        cplx *p = nullptr;
        QF_HIP(hipMalloc((void **)&p, mbytes));
        v.push_back(p);
    }
    return QF_OK;
}

// the three pinned staging buffers of the host hooks hold k N x N matrices each
int qf_need_hook_host(qf_ctx *ctx, int k)
{
    const size_t bytes = (size_t)k * ctx->N * ctx->N * sizeof(cplx);
    if (ctx->hook_host_bytes < bytes) {
        for (int q = 0; q < 3; ++q) {
            if (ctx->hook_host[q]) (void)hipHostFree(ctx->hook_host[q]);
            ctx->hook_host[q] = nullptr;
        }
        ctx->hook_host_bytes = 0;
        for (int q = 0; q < 3; ++q) QF_HIP(hipHostMalloc((void **)&ctx->hook_host[q], bytes, hipHostMallocDefault));
        ctx->hook_host_bytes = bytes;
    }
    return QF_OK;
}

int hook_failed(const char *which, int rc)
{
    qf_set_error("%s hook returned %d", which, rc);
    return QF_ERR_CALLBACK;
}

}  // namespace

// ---- defined in one api_*.hip, used by another (plain C++ linkage, not part of the exported C ABI) ----
extern "C" {
int qf_need_c64(qf_ctx *ctx);                 // api_laplacian.hip: the complex64 working set exists (qf_c64_upload_W or a c64 entry point made it)
int qf_oz_alloc(qf_ctx *ctx);                 // api_isomp.hip: digit planes and scales of the int8 products
int qf_rowpart_slots(const qf_ctx *ctx);      // api_isomp.hip: column-tile slots of the residual row sums for the selected second product
int qf_enqueue_diagnostics(qf_ctx *ctx);      // api_isomp.hip: P = solve(W); <W, P>, <W, W> on their way to the pinned scalars
}
