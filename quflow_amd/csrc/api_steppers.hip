// C ABI of libquflow_hip.so, part 4 of 5: the OTHER steppers on the same kernels -- isomp_simple / isomp_quasinewton
// (isospectral.py:155-335), isomp / magmp on stacks of states (host loop per iteration) and the resident stack.
// (euler / heun / rk4: api_erk.hip.)
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <chrono>

#include "qf_api.h"

extern "C" {

// ---- isomp_simple / isomp_quasinewton (quflow/integrators/isospectral.py:155-335) -----------
// Both need X = A^-1 W and Wtilde = A^-1 (-X^H) with A = I - E, E = (stepsize/2) Ptilde
// skew-Hermitian.  The reference factors A with LAPACK (lu_factor / lu_solve).  On this machine
// the inverse is formed on the fp64 matrix cores instead: A^H A = I + E^H E, so A has its singular
// values in [1, sqrt(1 + |E|_2^2)] and Newton-Schulz
//      Y <- Y + Y (I - A Y),     Y0 = A^H / (1 + |E|_inf^2)  (or the previous inverse, warm)
// converges quadratically from a residual whose 2-norm is <= |E|^2/(1+|E|^2) < 1: 2 iterations of two N^3
// products on white data, 4-8 per cold start on smooth data at |E|_inf = 0.1 ... 2, no pivoting, no
// triangular solves.  Same stepper, same result to rounding; only the linear-solve method differs from the reference.
// The loop measures the INFINITY norm, which is not bounded by 1 at the start: for large E it begins above 1 and rises
// for several iterations before the quadratic phase takes it down (|E|_inf = 1000, N = 257: 1.19, 1.29, ... 2.21 at
// iteration 13, 0.96 at 17, done after 23).  Only once it has been below 1 is r_{k+1} <= r_k^2 guaranteed in this norm,
// so only then does a rise mean that the inverse cannot be had.
// How large E may be: cond(A)^2 = (1 + s_max^2)/(1 + s_min^2) of E's singular values.  A stream function without a
// null vector: the scale of E drops out, 1e149 takes the iterations of 1e3.  With one (s_min = 0): cond(A) = |E|_2, the
// residual's rounding noise eps cond(A) stays above the 1e-8 exit level from |E|_2 ~ 1e8 on and the call ends with the
// error below, never with a state (LAPACK's LU has lost the state there as well: eps cond(A)^2).
struct ns_work {
    cplx *E, *Y, *R, *T;     // E = (stepsize/2) P;  Y ~ A^-1;  R, T scratch
    bool warm = false;
    bool general = false;    // E is not known to be skew-Hermitian (foreign Hamiltonian): conservative start
    double floor = 0.0;      // |I - A Y|_inf behind the last update: the rounding noise of this inverse
};

static int ns_invert(qf_ctx *ctx, ns_work &w)
{
    long long *count = ctx->ns_counts;       // inversions, cold starts, inverses kept, iterations (qf_ns_stats)
    count[0] += 1;
    // R = I - A Y = I - Y + E Y
    auto residual = [&](double *r_out) -> int {
        QF_TRY(qf_launch_zgemm(ctx, w.E, w.Y, w.T, nullptr));
        QF_TRY(qf_launch_lincomb(ctx, -1.0, w.Y, 1.0, w.T, 1.0, w.R));
        QF_TRY(qf_launch_norm_inf(ctx, w.R, ctx->scalars + 6));
        return read_scalar(ctx, ctx->scalars + 6, r_out);
    };
    double r = 2.0;
    if (w.warm) {
        QF_TRY(residual(&r));
        // E moved by no more than the rounding noise of the inverse: Y stays as it is.  An update from a residual at the noise
        // level only reshuffles Y's last bits, and with them the two solves' -- the quasi-Newton iteration's exit test asks for a
        // bit-level fixed point (|Wt - Wt_new|_inf < eps * stepsize * |W|, isospectral.py:190-191,227), which a Y that keeps
        // moving reaches one to three passes late or not before maxit (the reference's LU is a fixed function of A)
        if (w.floor > 0.0 && r <= 2.0 * w.floor) {
            count[2] += 1;
            return QF_OK;
        }
    }
    if (!(r < 0.5)) {
        count[1] += 1;
        // cold start: Y0 = A^H / (1 + |E|_inf^2) = (I + E) / (1 + c)
        double en = 0.0;
        QF_TRY(qf_launch_norm_inf(ctx, w.E, ctx->scalars + 6));
        QF_TRY(read_scalar(ctx, ctx->scalars + 6, &en));
        if (!QF_FINITE(en)) {       // (scipy.linalg.lu_factor checks its argument: isospectral.py:211, 290)
            qf_set_error("array must not contain infs or NaNs");
            return QF_ERR_NONFINITE;
        }
        if (en > 1e150) {
            // finite, but 1 + |E|^2 overflows: the Newton-Schulz start has no scale.  The reference's LU would go on (and
            // produce nothing usable): an error of this implementation, named as one -- not the reference's ValueError
            qf_set_error("isomp_simple / isomp_quasinewton: |dt/(2 hbar) P|_inf = %.3g is too large for the Newton-Schulz inverse (limit 1e150)", en);
            return QF_ERR_STATE;
        }
        // skew-Hermitian E: A A^H = I + E E^H, spectrum in [1, 1 + |E|^2].  A Hamiltonian that is not
        // skew-Hermitian (foreign hook): A A^H has its spectrum in [(1 - |E|)^2, (1 + |E|)^2]
        const double s = w.general ? 1.0 / ((1.0 + en) * (1.0 + en)) : 1.0 / (1.0 + en * en);
        if (w.general) {
            // Y0 = s A^H = s (I - E^H): -E^H through the transpose kernel
            QF_TRY(qf_launch_neg_conj_transpose(ctx, w.E, w.T));
            QF_TRY(qf_launch_lincomb(ctx, s, w.T, 0.0, nullptr, s, w.Y));
        } else {
            QF_TRY(qf_launch_lincomb(ctx, s, w.E, 0.0, nullptr, s, w.Y));
        }
        QF_TRY(residual(&r));
    }
    bool below_one = r < 1.0;      // the infinity-norm residual contracts for certain only from here on (see above)
    for (int it = 0; it < 200; ++it) {
        // Y <- Y + Y R
        QF_TRY(qf_launch_zgemm(ctx, w.Y, w.R, w.T, nullptr));
        QF_TRY(qf_launch_lincomb(ctx, 1.0, w.Y, 1.0, w.T, 0.0, w.Y));
        count[3] += 1;
        if (r < 1e-8) {          // the update just applied leaves a residual ~ r^2 < eps: what is measured now is the noise floor
            w.warm = true;
            QF_TRY(residual(&w.floor));
            return QF_OK;
        }
        const double r_prev = r;
        QF_TRY(residual(&r));
        if (!(r == r) || (below_one && r > r_prev)) break;
        below_one = below_one || r < 1.0;
    }
    qf_set_error("isomp linear solve: Newton-Schulz did not converge (residual %.3e)", r);
    return QF_ERR_STATE;
}

// one pass of the two solves: X = A^-1 Wrhs;  Wt_out = A^-1 (-X^H)    (isospectral.py:214-218, 293-297)
static int ns_two_solves(qf_ctx *ctx, ns_work &w, const cplx *Wrhs, cplx *X, cplx *Wt_out)
{
    QF_TRY(qf_launch_zgemm(ctx, w.Y, Wrhs, X, nullptr));
    QF_TRY(qf_launch_neg_conj_transpose(ctx, X, w.T));
    QF_TRY(qf_launch_zgemm(ctx, w.Y, w.T, Wt_out, nullptr));
    return QF_OK;
}

// W <- A^H Wt A = (I + E) Wt (I - E)    (isospectral.py:232, 300; A^H = I + E for the skew-Hermitian E of the
// built-in Hamiltonian).  EH != nullptr: a scratch matrix -- E need not be skew-Hermitian (foreign Hamiltonian, the
// general Poisson branch): A^H = I - E^H is formed explicitly.
static int ns_update_W(qf_ctx *ctx, ns_work &w, const cplx *Wt, cplx *Wout, cplx *EH = nullptr)
{
    if (EH) {
        QF_TRY(qf_launch_neg_conj_transpose(ctx, w.E, EH));                 // -E^H
        QF_TRY(qf_launch_zgemm(ctx, EH, Wt, w.T, nullptr));                 // -E^H Wt
        QF_TRY(qf_launch_lincomb(ctx, 1.0, Wt, 1.0, w.T, 0.0, w.R));        // V = (I - E^H) Wt
        QF_TRY(qf_launch_zgemm(ctx, w.R, w.E, w.T, nullptr));               // V E
        QF_TRY(qf_launch_lincomb(ctx, 1.0, w.R, -1.0, w.T, 0.0, Wout));     // V - V E
        return QF_OK;
    }
    QF_TRY(qf_launch_zgemm(ctx, w.E, Wt, w.T, nullptr));                    // E Wt
    QF_TRY(qf_launch_lincomb(ctx, 1.0, Wt, 1.0, w.T, 0.0, w.R));            // V = Wt + E Wt
    QF_TRY(qf_launch_zgemm(ctx, w.R, w.E, w.T, nullptr));                   // V E
    QF_TRY(qf_launch_lincomb(ctx, 1.0, w.R, -1.0, w.T, 0.0, Wout));         // V - V E
    return QF_OK;
}

static int ns_setup(qf_ctx *ctx, ns_work &w)
{
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    if (!ctx->ns_inv) QF_HIP(hipMalloc((void **)&ctx->ns_inv, mbytes));
    if (!ctx->ns_tmp) QF_HIP(hipMalloc((void **)&ctx->ns_tmp, mbytes));
    w.E = ctx->Phalf;
    w.Y = ctx->ns_inv;
    w.R = ctx->ns_tmp;
    w.T = ctx->PW;
    for (long long &c : ctx->ns_counts) c = 0;      // qf_ns_stats speaks of the call that starts here
    return QF_OK;
}

// what the Newton-Schulz inverse did in the last isomp_simple / isomp_quasinewton call of this context (read-only)
int qf_ns_stats(qf_ctx *ctx, long long out[4])
{
    QF_TRY(check_ctx(ctx));
    if (!out) {
        qf_set_error("qf_ns_stats: null output");
        return QF_ERR_INVALID;
    }
    for (int j = 0; j < 4; ++j) out[j] = ctx->ns_counts[j];
    return QF_OK;
}

// E = (stepsize/2) Ptilde with Ptilde = hamiltonian(Wtilde): the built-in Delta^-1 on the device, or the
// caller's hook on pinned host copies (isospectral.py:207, 286: `Ptilde = hamiltonian(Wtilde)`)
static int lu_hamiltonian(qf_ctx *ctx, ns_work &w, const cplx *Wt, double half_stepsize, const qf_isomp_hooks *hooks)
{
    // (the Laplacian backend's select_skewherm flag picks the solve's branch, cpu.py:563-591)
    if (!hooks || !hooks->hamiltonian) {
        if (!hooks || hooks->solve_skewh) return qf_launch_hamiltonian(ctx, Wt, w.E, half_stepsize);
        return qf_launch_solve(ctx, ctx->poisson, Wt, w.E, half_stepsize, 0);
    }
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_TRY(qf_need_hook_host(ctx, 1));
    cplx *hW = ctx->hook_host[0], *hP = ctx->hook_host[1];
    QF_HIP(hipMemcpyAsync(hW, Wt, mbytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    const int rc = hooks->hamiltonian(hooks->user, hW, hP, 0.0);
    if (rc != 0) {
        qf_set_error("hamiltonian hook returned %d", rc);
        return QF_ERR_CALLBACK;
    }
    QF_HIP(hipMemcpyAsync(w.T, hP, mbytes, hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_lincomb(ctx, half_stepsize, w.T, 0.0, nullptr, 0.0, w.E));
    return QF_OK;
}

static int isomp_simple_impl(qf_ctx *ctx, double dt, int steps, const qf_isomp_hooks *hooks)
{
    QF_TRY(check_ctx(ctx));
    if (steps < 0) {
        qf_set_error("qf_isomp_simple: steps must be >= 0");
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, hooks ? "qf_isomp_simple_hooked" : "qf_isomp_simple"));
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    const double stepsize = dt / qf_hbar(ctx->N);           // isospectral.py:281
    ctx->w_skew_known = false;
    ctx->increment_valid = false;    // (the state is replaced: no increment for qf_isomp_continue to carry)
    ns_work w;
    QF_TRY(ns_setup(ctx, w));
    const bool general_branch = hooks && !hooks->skewh;      // select_skewherm(False): isospectral.py:303-314
    w.general = (hooks && (hooks->hamiltonian || !hooks->solve_skewh)) || general_branch;
    cplx *Wt = ctx->Whalf, *X = ctx->stage;
    QF_HIP(hipMemcpyAsync(Wt, ctx->W, mbytes, hipMemcpyDeviceToDevice, ctx->stream));   // Wtilde = W.copy()
    ns_work w2;                                               // general branch: the inverse of Aalt = I + E
    if (general_branch) {
        QF_TRY(qf_need_matrices(ctx, ctx->multi, 2));
        w2.E = ctx->multi[0];        // -E
        w2.Y = ctx->multi[1];
        w2.R = w.R;
        w2.T = w.T;
        w2.general = true;
    }
    for (int k = 0; k < steps; ++k) {
        QF_TRY(lu_hamiltonian(ctx, w, Wt, stepsize / 2.0, hooks));                     // E = (stepsize/2) Ptilde
        QF_TRY(ns_invert(ctx, w));
        if (general_branch) {
            // X = A^-1 W;  Wtilde = (Aalt^-H X^H)^H = X Aalt^-1, Aalt = I + E;  W = Aalt Wtilde A   (:305-314)
            QF_TRY(qf_launch_lincomb(ctx, -1.0, w.E, 0.0, nullptr, 0.0, w2.E));
            QF_TRY(ns_invert(ctx, w2));
            QF_TRY(qf_launch_zgemm(ctx, w.Y, ctx->W, X, nullptr));
            QF_TRY(qf_launch_zgemm(ctx, X, w2.Y, Wt, nullptr));
            QF_TRY(ns_update_W(ctx, w, Wt, ctx->W));
            continue;
        }
        QF_TRY(ns_two_solves(ctx, w, ctx->W, X, Wt));
        QF_TRY(ns_update_W(ctx, w, Wt, ctx->W, w.general ? X : nullptr));
    }
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_isomp_simple(qf_ctx *ctx, double dt, int steps) { return isomp_simple_impl(ctx, dt, steps, nullptr); }

// ... with a foreign `hamiltonian(Wtilde)` (the `hamiltonian` and `user` members of the hook table): the state, the
// Newton-Schulz inverse and the products stay on the device, Wtilde goes down and Ptilde comes up once per pass
int qf_isomp_simple_hooked(qf_ctx *ctx, double dt, int steps, const qf_isomp_hooks *hooks)
{
    return isomp_simple_impl(ctx, dt, steps, hooks);
}

static int isomp_quasinewton_impl(qf_ctx *ctx, double dt, int steps, double tol, int maxit, qf_isomp_stats *stats_out,
                                  const qf_isomp_hooks *hooks);

int qf_isomp_quasinewton(qf_ctx *ctx, double dt, int steps, double tol, int maxit, qf_isomp_stats *stats_out)
{
    return isomp_quasinewton_impl(ctx, dt, steps, tol, maxit, stats_out, nullptr);
}

int qf_isomp_quasinewton_hooked(qf_ctx *ctx, double dt, int steps, double tol, int maxit, qf_isomp_stats *stats_out,
                                const qf_isomp_hooks *hooks)
{
    return isomp_quasinewton_impl(ctx, dt, steps, tol, maxit, stats_out, hooks);
}

static int isomp_quasinewton_impl(qf_ctx *ctx, double dt, int steps, double tol, int maxit, qf_isomp_stats *stats_out,
                                  const qf_isomp_hooks *hooks)
{
    QF_TRY(check_ctx(ctx));
    if (steps < 0 || maxit < 1) {
        qf_set_error("qf_isomp_quasinewton: steps must be >= 0 and maxit >= 1");
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, hooks ? "qf_isomp_quasinewton_hooked" : "qf_isomp_quasinewton"));
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    const double stepsize = dt / qf_hbar(ctx->N);           // isospectral.py:187
    ctx->w_skew_known = false;
    ctx->increment_valid = false;    // (dW[0], dW[1] are Wtilde_new and the residual below)
    if (tol < 0) {                                          // isospectral.py:190-191
        double nrm = 0.0;
        QF_TRY(qf_norm_inf_W(ctx, &nrm));
        tol = std::numeric_limits<double>::epsilon() * stepsize * nrm;
    }
    ns_work w;
    QF_TRY(ns_setup(ctx, w));
    w.general = hooks && (hooks->hamiltonian || !hooks->solve_skewh);
    cplx *Wt = ctx->Whalf, *Wt_new = ctx->dW[0], *X = ctx->stage, *D = ctx->dW[1];
    QF_HIP(hipMemcpyAsync(Wt, ctx->W, mbytes, hipMemcpyDeviceToDevice, ctx->stream));   // Wtilde = W.copy()
    long long total_iterations = 0, number_of_maxit = 0;
    double resnorm = 0.0;
    for (int k = 0; k < steps; ++k) {
        bool converged = false;
        for (int i = 0; i < maxit; ++i) {
            total_iterations += 1;
            QF_TRY(lu_hamiltonian(ctx, w, Wt, stepsize / 2.0, hooks));                 // A = Id - (stepsize/2) Ptilde
            QF_TRY(ns_invert(ctx, w));
            QF_TRY(ns_two_solves(ctx, w, ctx->W, X, Wt_new));
            // resnorm = |Wtilde - Wtilde_new|_inf    (isospectral.py:221)
            QF_TRY(qf_launch_lincomb(ctx, 1.0, Wt, -1.0, Wt_new, 0.0, D));
            QF_TRY(qf_launch_norm_inf(ctx, D, ctx->scalars + 7));
            QF_TRY(read_scalar(ctx, ctx->scalars + 7, &resnorm));
            if (!QF_FINITE(resnorm)) {       // scipy.linalg.norm raises here (isospectral.py:221)
                qf_set_error("array must not contain infs or NaNs");
                return QF_ERR_NONFINITE;
            }
            cplx *t = Wt; Wt = Wt_new; Wt_new = t;                                     // Wtilde = Wtilde_new
            if (resnorm < tol) {                                                      // isospectral.py:227
                converged = true;
                break;
            }
        }
        if (!converged) number_of_maxit += 1;
        QF_TRY(ns_update_W(ctx, w, Wt, ctx->W, w.general ? X : nullptr));
    }
    // leave Wtilde where later calls expect scratch only; nothing to restore
    QF_HIP(hipStreamSynchronize(ctx->stream));
    fill_stats(stats_out, total_iterations, number_of_maxit, tol, resnorm);
    return QF_OK;
}

// ---- isomp on a stack of states / magmp -------------------------------------------------------
// isomp_fixedpoint with W.shape = (k,N,N) (quflow/integrators/isospectral.py:463-611, 3-D
// branches): P comes from state 0 only (cpu.py:696-697), every state runs the same products, the
// exit test uses state 0's residual (isospectral.py:527-532).  magnetic != 0 (k == 2): magmp,
// quflow/integrators/mhd.py:235-456 with hamiltonian = solve_mhd (mhd.py:10-18): B = Delta Theta
// and the vorticity state gets [B, Theta] on top.  The iteration control is
// host-side (one scalar read-back per iteration, as the reference does): these are the secondary
// steppers, their products (>= 4 per iteration) dwarf the read-back.
// The loop is written once (states_body) on the stack's resident buffers ctx->stack: qf_isomp_states is upload + body +
// download, qf_states_advance the body alone on a stack that qf_states_upload left there.
}  // extern "C"

namespace {

int stack_upload(qf_ctx *ctx, const void *states_host, int k)
{
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_TRY(qf_need_matrices(ctx, ctx->stack, (size_t)5 * k));
    for (int j = 0; j < k; ++j)
        QF_HIP(hipMemcpyAsync(ctx->stack[5 * j], (const char *)states_host + (size_t)j * mbytes, mbytes, hipMemcpyHostToDevice, ctx->stream));
    return QF_OK;
}

// P = Delta^-1 W (k_solve), then the five sums in one pass (k_mhd_sums), on their way to the pinned scalars
int enqueue_mhd_diagnostics(qf_ctx *ctx)
{
    if (!ctx->mhd_part) QF_HIP(hipMalloc((void **)&ctx->mhd_part, (size_t)(5 * 1024 + 8) * sizeof(double)));
    double *out = ctx->mhd_part + 5 * 1024;
    QF_TRY(qf_launch_solve(ctx, ctx->poisson, ctx->stack[0], ctx->stage, 1.0, 1));
    QF_TRY(qf_launch_mhd_sums(ctx, ctx->stack[0], ctx->stage, ctx->stack[5], ctx->mhd_part, out));
    QF_HIP(hipMemcpyAsync(ctx->host_scalars, out, 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return QF_OK;
}

// (the forms of qf_diagnostics: -(<W,P>/N)/2 and (<W,W>/N)/2, inner_L2 = sum / N)
void mhd_from_sums(const qf_ctx *ctx, double out[5])
{
    const int N = ctx->N;
    const double *h = ctx->host_scalars;
    out[0] = -(h[0] / N) / 2.0;      // Ek = -<W, Delta^-1 W>/2
    out[1] = -(h[1] / N) / 2.0;      // Em = -<Theta, Delta Theta>/2
    out[2] = h[2] / N;               // X  = <W, Theta>
    out[3] = (h[3] / N) / 2.0;       // A  = <Theta, Theta>/2
    out[4] = (h[4] / N) / 2.0;       // S  = <W, W>/2
}

// `steps` steps of the k states in ctx->stack[5 j]: dX restarts from zero, the exit test is state 0's, the finite check covers
// every state.  states_host != nullptr: the result is downloaded there;  mhd_out != nullptr (magnetic): the diagnostics of
// the new state -- either one under the closing synchronisation.
int states_body(qf_ctx *ctx, void *states_host, int k, double dt, int steps, double tol, int minit, int maxit, int reinitialize,
                int magnetic, qf_isomp_stats *stats_out, double *mhd_out)
{
    const int N = ctx->N;
    const size_t NN = (size_t)N * N, mbytes = NN * sizeof(cplx);
    const double hb = qf_hbar(N);
    const double vareps = dt / (2 * hb);
    // per state: X, dX[2], Xhalf, PXc;  magnetic: Bhalf, BT, BTP
    QF_TRY(qf_need_matrices(ctx, ctx->stack, (size_t)5 * k + (magnetic ? 3 : 0)));
    const int slots32 = (N + 31) / 32;
    if (!ctx->multi_rowpart) QF_HIP(hipMalloc((void **)&ctx->multi_rowpart, (size_t)2 * slots32 * N * sizeof(double)));   // (sized as hooks.hip sizes it)
    struct st { cplx *X, *dX[2], *Xhalf, *PXc; int cur; };
    std::vector<st> S((size_t)k);
    for (int j = 0; j < k; ++j) {
        S[j].X = ctx->stack[5 * j];
        S[j].dX[0] = ctx->stack[5 * j + 1];
        S[j].dX[1] = ctx->stack[5 * j + 2];
        S[j].Xhalf = ctx->stack[5 * j + 3];
        S[j].PXc = ctx->stack[5 * j + 4];
        S[j].cur = 0;
        QF_HIP(hipMemsetAsync(S[j].dX[0], 0, mbytes, ctx->stream));                          // dW = zeros_like(W)
        QF_HIP(hipMemcpyAsync(S[j].Xhalf, S[j].X, mbytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    cplx *Bhalf = magnetic ? ctx->stack[5 * k] : nullptr;
    cplx *BT = magnetic ? ctx->stack[5 * k + 1] : nullptr;
    cplx *BTP = magnetic ? ctx->stack[5 * k + 2] : nullptr;

    // the upper-triangle second product wants every state exactly skew-Hermitian
    bool tri = ctx->gemm_tri_allowed && ctx->sk_partial && N >= ctx->gemm_tri_min_n;
    for (int j = 0; j < k && tri; ++j) QF_TRY(qf_exactly_skew(ctx, S[j].X, &tri));
    // (the context's own selection comes back however the loop is left)
    struct tri_guard {
        qf_ctx *ctx;
        bool tri, tri32;
        ~tri_guard() { ctx->gemm_tri = tri; ctx->gemm_tri32 = tri32; }
    } guard{ctx, ctx->gemm_tri, ctx->gemm_tri32};
    ctx->gemm_tri = tri;
    ctx->gemm_tri32 = false;       // (stacks below N = 768 keep the full product)

    // tolerance from state 0 (isospectral.py:440-452; magmp uses sqrt(eps) always, mhd.py:331-341)
    if (tol < 0) QF_TRY(auto_tolerance(ctx, S[0].X, std::sqrt(std::numeric_limits<double>::epsilon()) * dt / hb, &tol));

    long long total_iterations = 0, number_of_maxit = 0;
    double resnorm = 0.0;
    for (int step = 0; step < steps; ++step) {
        resnorm = std::numeric_limits<double>::infinity();
        bool broke = false;
        for (int i = 0; i < maxit; ++i) {
            total_iterations += 1;
            // Phalf = vareps * Delta^-1 Whalf[0]   (+ Bhalf = vareps * Delta Thetahalf)
            // (magmp's Hamiltonian is solve_mhd: Poisson as such; a stack of isomp states follows the flow's)
            if (magnetic) QF_TRY(qf_launch_solve(ctx, ctx->poisson, S[0].Xhalf, ctx->Phalf, vareps, 1));
            else QF_TRY(qf_launch_hamiltonian(ctx, S[0].Xhalf, ctx->Phalf, vareps));
            if (magnetic) {
                QF_TRY(qf_launch_laplace_scaled(ctx, S[1].Xhalf, Bhalf, vareps));      // (one launch, the bits of laplace + lincomb)
            }
            for (int j = 0; j < k; ++j)                                   // Pstatecomm = Phalf @ statehalf
                QF_TRY(qf_launch_zgemm(ctx, ctx->Phalf, S[j].Xhalf, S[j].PXc, nullptr));
            if (magnetic) {
                QF_TRY(qf_launch_zgemm(ctx, Bhalf, S[1].Xhalf, BT, nullptr));       // BThetacomm
                QF_TRY(qf_launch_zgemm(ctx, BT, ctx->Phalf, BTP, nullptr));         // BThetaPhalf
            }
            for (int j = 0; j < k; ++j) {
                // dX = PXc @ Phalf + (PXc - PXc^H);  Xhalf = X + dX;  row sums of |dX_old - dX|
                qf_epilogue ep;
                ep.PW = S[j].PXc;
                ep.W = S[j].X;
                ep.dW[0] = S[j].dX[S[j].cur];
                ep.dW[1] = S[j].dX[S[j].cur ^ 1];
                ep.Whalf = S[j].Xhalf;
                ep.rowpart = ctx->rowpart;
                QF_TRY(qf_launch_zgemm(ctx, S[j].PXc, ctx->Phalf, nullptr, &ep));
                if (j == 0) {
                    if (magnetic) {
                        QF_TRY(qf_launch_magnetic_fix(ctx, BTP, BT, S[0].dX[S[0].cur ^ 1], S[0].dX[S[0].cur], S[0].X,
                                                      S[0].Xhalf, ctx->multi_rowpart));
                        QF_TRY(qf_launch_norm_from_rowpart(ctx, ctx->multi_rowpart, slots32, ctx->scalars + 16));
                    } else {
                        QF_TRY(qf_launch_norm_from_rowpart(ctx, ctx->rowpart, qf_rowpart_slots(ctx), ctx->scalars + 16));
                    }
                } else if (i + 1 >= minit) {
                    // the exit test looks at state 0's residual, but scipy.linalg.norm checks the WHOLE stack for infs / NaNs
                    // before it reduces (check_finite, isospectral.py:528): the other states' norms are formed for that check --
                    // the slots of read_stack_resnorm, the states beyond 48 folded on the device into scalars[8]
                    QF_TRY(qf_launch_norm_from_rowpart(ctx, ctx->rowpart, qf_rowpart_slots(ctx), ctx->scalars + (j < 48 ? 16 + j : 9)));
                    if (j == 48) QF_HIP(hipMemsetAsync(ctx->scalars + 8, 0, sizeof(double), ctx->stream));
                    if (j >= 48) QF_TRY(qf_launch_fold_nonfinite(ctx, ctx->scalars + 9, ctx->scalars + 8));
                }
                S[j].cur ^= 1;
            }
            if (i + 1 >= minit) {
                const double resnorm_old = resnorm;
                // (scipy.linalg.norm raises for a non-finite state here: isospectral.py:534, mhd.py: same test)
                QF_TRY(read_stack_resnorm(ctx, k, false, &resnorm));
                if (resnorm <= tol || resnorm >= resnorm_old) {
                    broke = true;
                    break;
                }
            }
        }
        if (!broke) number_of_maxit += 1;
        // W += 2 (PXc - PXc^H) for every state; Xhalf = X + dX for the next step
        for (int j = 0; j < k; ++j)
            QF_TRY(qf_launch_update(ctx, S[j].PXc, S[j].X, S[j].dX[S[j].cur], S[j].dX[S[j].cur], S[j].Xhalf, nullptr,
                                    reinitialize));
        if (magnetic)
            QF_TRY(qf_launch_magnetic_update(ctx, BT, S[0].X, reinitialize ? nullptr : S[0].dX[S[0].cur], S[0].Xhalf));
    }
    // what the caller queues behind the last step rides on the call's closing synchronisation: the MHD diagnostics
    // (qf_states_advance_diag) or the download (qf_isomp_states)
    if (mhd_out) QF_TRY(enqueue_mhd_diagnostics(ctx));
    if (states_host)
        for (int j = 0; j < k; ++j)
            QF_HIP(hipMemcpyAsync((char *)states_host + (size_t)j * mbytes, S[j].X, mbytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    if (mhd_out) mhd_from_sums(ctx, mhd_out);
    fill_stats(stats_out, total_iterations, number_of_maxit, tol, resnorm);
    return QF_OK;
}

}  // namespace

extern "C" {

int qf_isomp_states(qf_ctx *ctx, void *states_host, int k, double dt, int steps, double tol, int minit, int maxit,
                    int reinitialize, int magnetic, qf_isomp_stats *stats_out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_iteration_args(minit, maxit));
    if (!states_host || k < 1 || steps < 0 || (magnetic && k != 2)) {
        qf_set_error("qf_isomp_states: bad arguments (k=%d, steps=%d, magnetic=%d)", k, steps, magnetic);
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, "qf_isomp_states"));
    ctx->stack_k = 0;        // (host in / host out: the stack's buffers are this call's scratch)
    QF_TRY(stack_upload(ctx, states_host, k));
    return states_body(ctx, states_host, k, dt, steps, tol, minit, maxit, reinitialize, magnetic, stats_out, nullptr);
}

// ---- the resident stack --------------------------------------------------------------------------------------
int qf_states_upload(qf_ctx *ctx, const void *states_host, int k)
{
    QF_TRY(check_ctx(ctx));
    if (!states_host || k < 1) {
        qf_set_error("qf_states_upload: bad arguments (k=%d)", k);
        return QF_ERR_INVALID;
    }
    ctx->stack_k = 0;
    QF_TRY(stack_upload(ctx, states_host, k));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stack_k = k;
    return QF_OK;
}

static int need_stack(const qf_ctx *ctx, const char *who)
{
    if (ctx->stack_k < 1) {
        qf_set_error("%s: no stack is resident (qf_states_upload; a host-in / host-out qf_isomp_states call discards it)", who);
        return QF_ERR_STATE;
    }
    return QF_OK;
}

int qf_states_download(qf_ctx *ctx, void *states_host, int k)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stack(ctx, "qf_states_download"));
    if (!states_host || k != ctx->stack_k) {
        qf_set_error("qf_states_download: bad arguments (k=%d, resident %d)", k, ctx->stack_k);
        return QF_ERR_INVALID;
    }
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    for (int j = 0; j < k; ++j)
        QF_HIP(hipMemcpyAsync((char *)states_host + (size_t)j * mbytes, ctx->stack[5 * j], mbytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

int qf_states_advance_diag(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int reinitialize, int magnetic,
                           qf_isomp_stats *stats_out, double *mhd_out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_iteration_args(minit, maxit));
    QF_TRY(need_stack(ctx, "qf_states_advance"));
    if (steps < 0 || (magnetic && ctx->stack_k != 2) || (mhd_out && !magnetic)) {
        qf_set_error("qf_states_advance: bad arguments (resident k=%d, steps=%d, magnetic=%d)", ctx->stack_k, steps, magnetic);
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, "qf_states_advance"));
    return states_body(ctx, nullptr, ctx->stack_k, dt, steps, tol, minit, maxit, reinitialize, magnetic, stats_out, mhd_out);
}

int qf_states_advance(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int reinitialize, int magnetic,
                      qf_isomp_stats *stats_out)
{
    return qf_states_advance_diag(ctx, dt, steps, tol, minit, maxit, reinitialize, magnetic, stats_out, nullptr);
}

static int stack_member(qf_ctx *ctx, int j, const char *who)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stack(ctx, who));
    if (j < 0 || j >= ctx->stack_k) {
        qf_set_error("%s: member %d of a stack of %d", who, j, ctx->stack_k);
        return QF_ERR_INVALID;
    }
    return QF_OK;
}

int qf_states_select(qf_ctx *ctx, int j)
{
    QF_TRY(stack_member(ctx, j, "qf_states_select"));
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->W, ctx->stack[5 * j], mbytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->w_skew_known = false;       // (as after qf_upload_W)
    ctx->w_c128_set = true;
    ctx->increment_valid = false;
    return QF_OK;
}

int qf_states_store(qf_ctx *ctx, int j)
{
    QF_TRY(stack_member(ctx, j, "qf_states_store"));
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    QF_HIP(hipMemcpyAsync(ctx->stack[5 * j], ctx->W, mbytes, hipMemcpyDeviceToDevice, ctx->stream));
    return QF_OK;
}

int qf_states_inner(qf_ctx *ctx, double *out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stack(ctx, "qf_states_inner"));
    if (!out) {
        qf_set_error("qf_states_inner: null output");
        return QF_ERR_INVALID;
    }
    // k_inner2 per member (the launch of qf_diagnostics), 32 members per read-back of the pinned scalars
    const int N = ctx->N, k = ctx->stack_k;
    for (int j0 = 0; j0 < k; j0 += 32) {
        const int n = k - j0 < 32 ? k - j0 : 32;
        for (int j = 0; j < n; ++j) {
            QF_TRY(qf_launch_inner2(ctx, ctx->stack[5 * (j0 + j)], ctx->stack[0], ctx->scalars + 2));
            QF_HIP(hipMemcpyAsync(ctx->host_scalars + 2 * j, ctx->scalars + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        }
        QF_HIP(hipStreamSynchronize(ctx->stream));
        for (int j = 0; j < n; ++j) {
            out[2 * (j0 + j)] = ctx->host_scalars[2 * j] / N;
            out[2 * (j0 + j) + 1] = (ctx->host_scalars[2 * j + 1] / N) / 2.0;
        }
    }
    return QF_OK;
}

int qf_mhd_diagnostics(qf_ctx *ctx, double out[5])
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stack(ctx, "qf_mhd_diagnostics"));
    if (!out || ctx->stack_k != 2) {
        qf_set_error("qf_mhd_diagnostics: the resident stack must be the pair (W, Theta) (k=%d)", ctx->stack_k);
        return QF_ERR_INVALID;
    }
    QF_TRY(enqueue_mhd_diagnostics(ctx));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    mhd_from_sums(ctx, out);
    return QF_OK;
}

// out = (X Y - (X Y)^H) (1/hbar), the bracket [X, Y]/hbar of two skew-Hermitian matrices: the launches of the hydrodynamic
// budget's tendency (budget_run, api_transforms.hip) in its order of operations; ctx->PW and ctx->Whalf are the scratch
static int mhd_bracket(qf_ctx *ctx, const cplx *X, const cplx *Y, double inv_hb, cplx *out)
{
    QF_TRY(qf_launch_zgemm(ctx, X, Y, ctx->PW, nullptr));                                       // Z = X @ Y
    QF_TRY(qf_launch_neg_conj_transpose(ctx, ctx->PW, ctx->Whalf));                             // -Z^H
    QF_TRY(qf_launch_lincomb(ctx, 1.0, ctx->PW, 1.0, ctx->Whalf, 0.0, ctx->PW));                // Z - Z^H
    QF_TRY(qf_launch_lincomb(ctx, inv_hb, ctx->PW, 0.0, (const cplx *)nullptr, 0.0, out));      // (Z - Z^H) (1/hbar)
    return QF_OK;
}

// Where everything lives: W, Theta are the stack's members 0 and 1 (read only); P, B, [P,W]/hbar, [B,Theta]/hbar,
// [P,Theta]/hbar in ctx->mhdb_mats; the packed diagonals and the sweep's results in the ten parts of ctx->mhdb_vec, the
// coefficient arrays over the packed diagonals (dead after the sweep); the nine rows in ctx->mhdb_sums.
int qf_mhd_spectral_budget(qf_ctx *ctx, int Nmax, double *out, double *coeffs)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(need_stack(ctx, "qf_mhd_spectral_budget"));
    const int N = ctx->N;
    if (ctx->stack_k != 2) {
        qf_set_error("qf_mhd_spectral_budget: the resident stack must be the pair (W, Theta) (k=%d)", ctx->stack_k);
        return QF_ERR_INVALID;
    }
    if (!out) {
        qf_set_error("qf_mhd_spectral_budget: null output");
        return QF_ERR_INVALID;
    }
    if (Nmax <= 1 || Nmax > N) {
        qf_set_error("qf_mhd_spectral_budget: band limit Nmax=%d outside 2..N=%d", Nmax, N);
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, "qf_mhd_spectral_budget"));
    if (ctx->ham_table || ctx->ham_offset_on) {
        qf_set_error("qf_mhd_spectral_budget: a Hamiltonian is installed on this context (qf_set_hamiltonian); the MHD "
                     "budget is that of the built-in system P = Delta^-1 W, B = Delta Theta");
        return QF_ERR_UNSUPPORTED;
    }
    if (ctx->slab_budget > 0) {       // (the slab plan's refusal comes before anything is launched)
        std::vector<int> first;
        long long need = 0;
        QF_TRY(qf_slab_plan(N, Nmax, ctx->slab_budget, first, &need));
    } else if (!ctx->basis) {
        qf_set_error("qf_mhd_spectral_budget: no quantization basis on this context (qf_basis_compute, or qf_basis_stream)");
        return QF_ERR_STATE;
    }
    const size_t NN = (size_t)N * N, half = (size_t)N * (N + 1) / 2, LL = (size_t)Nmax * Nmax;
    if (!ctx->mhdb_sums) QF_HIP(hipMalloc((void **)&ctx->mhdb_sums, (size_t)9 * N * sizeof(double)));
    if (!ctx->mhdb_vec) QF_HIP(hipMalloc((void **)&ctx->mhdb_vec, 10 * half * sizeof(cplx)));
    if (!ctx->mhdb_mats) QF_HIP(hipMalloc((void **)&ctx->mhdb_mats, 5 * NN * sizeof(cplx)));
    const cplx *W = ctx->stack[0], *Theta = ctx->stack[5];
    cplx *P = ctx->mhdb_mats, *B = P + NN, *adv = P + 2 * NN, *lor = P + 3 * NN, *ind = P + 4 * NN;
    const double inv_hb = 1.0 / qf_hbar(N);
    QF_TRY(qf_launch_hamiltonian(ctx, W, P, 1.0));             // P = Delta^-1 W (nothing is installed: ctx->poisson)
    QF_TRY(qf_launch_laplace(ctx, Theta, B));                  // B = Delta Theta
    QF_TRY(mhd_bracket(ctx, P, W, inv_hb, adv));
    QF_TRY(mhd_bracket(ctx, B, Theta, inv_hb, lor));
    QF_TRY(mhd_bracket(ctx, P, Theta, inv_hb, ind));
    const cplx *mats[5] = {W, Theta, adv, lor, ind};
    cplx *d[5], *z[5];
    double *omega[5];
    for (int v = 0; v < 5; ++v) {
        d[v] = ctx->mhdb_vec + (size_t)v * half;
        z[v] = ctx->mhdb_vec + (size_t)(5 + v) * half;
        omega[v] = reinterpret_cast<double *>(d[v]);
    }
    QF_TRY(qf_launch_mhd_degree_budget(ctx, Nmax, mats, d, z, omega, ctx->mhdb_sums));
    QF_HIP(hipMemcpyAsync(out, ctx->mhdb_sums, (size_t)9 * Nmax * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    for (int v = 0; coeffs && v < 5; ++v)
        QF_HIP(hipMemcpyAsync(coeffs + v * LL, omega[v], LL * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

}  // extern "C"
