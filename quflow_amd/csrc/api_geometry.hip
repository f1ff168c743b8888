// C ABI of libquflow_hip.so: ROTATIONS AND GRADIENTS (geometry.hip) -- qf_so3_exp_plan (host only), qf_so3_exp,
// qf_rotate (W' = R W R^H on a host matrix or on the resident state) and qf_grad (quflow/geometry.py:154-207).
// exp(xi . S) is the Taylor start of k_so3_taylor squared sigma times with the ordinary product.
#include "qf_api.h"

namespace {

int geom_alloc(qf_ctx *ctx, bool grad)
{
    qf_geom_ws &w = ctx->geom;
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    if (grad) {
        if (!w.grad) QF_HIP(hipMalloc((void **)&w.grad, 3 * mbytes));
        return QF_OK;
    }
    for (int q = 0; q < 2; ++q)
        if (!w.R[q]) QF_HIP(hipMalloc((void **)&w.R[q], mbytes));
    for (int q = 0; q < 3; ++q)
        if (!w.ev[q]) QF_HIP(hipEventCreate(&w.ev[q]));
    return QF_OK;
}

// |A|_inf is finite, or QF_ERR_NONFINITE (one read-back)
int check_finite(qf_ctx *ctx, const cplx *A, const char *what)
{
    double norm = 0.0;
    QF_TRY(qf_launch_norm_inf(ctx, A, ctx->scalars));
    QF_TRY(read_scalar(ctx, ctx->scalars, &norm));
    if (!QF_FINITE(norm)) {
        qf_set_error("%s: the matrix has an inf or NaN entry", what);
        return QF_ERR_NONFINITE;
    }
    return QF_OK;
}

// Enqueues R = exp(xi . S): *cur names the buffer of ctx->geom.R that holds it, the other one is free.
int so3_exp_core(qf_ctx *ctx, const double xi[3], int *cur)
{
    int sigma = 0, degree = 0;
    QF_TRY(qf_so3_plan(ctx->N, xi, &sigma, &degree, nullptr));
    QF_TRY(geom_alloc(ctx, false));
    qf_geom_ws &w = ctx->geom;
    w.timed = false;
    int c = 0;
    QF_HIP(hipEventRecord(w.ev[0], ctx->stream));
    QF_TRY(qf_launch_so3_taylor(ctx, xi, sigma, degree, w.R[0]));
    QF_HIP(hipEventRecord(w.ev[1], ctx->stream));
    for (int q = 0; q < sigma; ++q) {
        QF_TRY(qf_launch_zgemm(ctx, w.R[c], w.R[c], w.R[c ^ 1], nullptr));
        c ^= 1;
    }
    QF_HIP(hipEventRecord(w.ev[2], ctx->stream));
    *cur = c;
    return QF_OK;
}

}  // namespace

extern "C" {

int qf_so3_exp_plan(int N, const double xi[3], int *squarings, int *degree)
{
    if (N < 2 || N > 8192) {
        qf_set_error("qf_so3_exp_plan: N = %d is outside 2..8192", N);
        return QF_ERR_INVALID;
    }
    return qf_so3_plan(N, xi, squarings, degree, nullptr);
}

int qf_so3_exp(qf_ctx *ctx, const double xi[3], void *R_host)
{
    QF_TRY(check_ctx(ctx));
    int cur = 0;
    QF_TRY(so3_exp_core(ctx, xi, &cur));
    if (R_host)
        QF_HIP(hipMemcpyAsync(R_host, ctx->geom.R[cur], (size_t)ctx->N * ctx->N * sizeof(cplx), hipMemcpyDeviceToHost,
                              ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->geom.timed = true;
    return QF_OK;
}

int qf_so3_exp_times(qf_ctx *ctx, double *taylor_ms, double *squarings_ms)
{
    QF_TRY(check_ctx(ctx));
    if (!ctx->geom.timed || !taylor_ms || !squarings_ms) {
        qf_set_error("qf_so3_exp_times: no completed qf_so3_exp / qf_rotate on this context, or a null argument");
        return QF_ERR_STATE;
    }
    float a = 0.f, b = 0.f;
    QF_HIP(hipEventElapsedTime(&a, ctx->geom.ev[0], ctx->geom.ev[1]));
    QF_HIP(hipEventElapsedTime(&b, ctx->geom.ev[1], ctx->geom.ev[2]));
    *taylor_ms = (double)a;
    *squarings_ms = (double)b;
    return QF_OK;
}

// W' = R W R^H.  The products go through the context's per-iteration staging matrices (stage, PW, Whalf), which are free
// between stepper calls.  In place (W_host == NULL) the context is left as qf_upload_W leaves it: nothing is known about
// the new state's symmetry, and the increment of an earlier stepper call does not belong to it any more.
int qf_rotate(qf_ctx *ctx, const double xi[3], const void *W_host, void *out_host)
{
    QF_TRY(check_ctx(ctx));
    if (W_host && !out_host) {
        qf_set_error("qf_rotate: a host matrix needs a host result");
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_so3_plan(ctx->N, xi, nullptr, nullptr, nullptr));        // a bad xi is refused before anything is launched
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    const cplx *W = ctx->W;
    if (W_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        W = ctx->stage;
    }
    QF_TRY(check_finite(ctx, W, "rotate"));
    int cur = 0;
    QF_TRY(so3_exp_core(ctx, xi, &cur));
    qf_geom_ws &w = ctx->geom;
    cplx *dest = W_host ? ctx->Whalf : ctx->W;
    QF_TRY(qf_launch_zgemm(ctx, w.R[cur], W, ctx->PW, nullptr));                               // M = R W
    QF_TRY(qf_launch_eigh_conj_transpose(ctx, w.R[cur], nullptr, nullptr, w.R[cur ^ 1]));      // R^H
    QF_TRY(qf_launch_zgemm(ctx, ctx->PW, w.R[cur ^ 1], dest, nullptr));                        // W' = M R^H
    if (!W_host) {
        ctx->w_skew_known = false;
        ctx->increment_valid = false;
    }
    if (out_host) QF_HIP(hipMemcpyAsync(out_host, dest, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    w.timed = true;
    return QF_OK;
}

int qf_grad(qf_ctx *ctx, const void *P_host, void *dP_host)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(geom_alloc(ctx, true));
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    const cplx *P = ctx->W;
    if (P_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, P_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        P = ctx->stage;
    }
    QF_TRY(check_finite(ctx, P, "grad"));
    QF_TRY(qf_launch_so3_grad(ctx, P, ctx->geom.grad));
    if (dP_host) QF_HIP(hipMemcpyAsync(dP_host, ctx->geom.grad, 3 * bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

}  // extern "C"
