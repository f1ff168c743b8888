// C ABI of libquflow_hip.so: the HERMITIAN EIGENSOLVER (eigh.hip) and what is built on it -- qf_eigh / qf_eigh_skew on
// host matrices, qf_eigh_state on the resident state, and qf_scale_decomposition (quflow/analysis.py:8-34 for a
// skew-Hermitian stream matrix).  The sweeps are driven from here: n - 1 round launches, then one 16-byte read-back.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

#include "qf_api.h"

namespace {

// Stop when no pair of a sweep had |c| > tol sqrt(a b); rotate only such pairs.  8 eps: a rotation leaves its pair
// orthogonal to a few eps (rounding of the two rows and of the angle), so a smaller threshold would rotate rounding noise
// for ever, and the off-diagonal of V^H V -- which is this very quantity -- stays below the N eps scale of the tests from
// N = 2 on.  Sweeps needed: 2 at N = 2, 7-12 at N = 16..256, 15 at N = 2048, 16 on a three-cluster spectrum at N = 65; the
// count grows like log N, so 60 is a generous cap: reaching it is an error (QF_ERR_NOCONVERGE), never a silent result.
const double EIGH_TOL = 8.0 * std::numeric_limits<double>::epsilon();
const int EIGH_MAX_SWEEPS = 60;

int eigh_alloc(qf_ctx *ctx)
{
    qf_eigh_ws &w = ctx->eigh;
    const size_t N = (size_t)ctx->N, mbytes = N * N * sizeof(cplx);
    if (!w.H) QF_HIP(hipMalloc((void **)&w.H, mbytes));
    if (!w.G) QF_HIP(hipMalloc((void **)&w.G, mbytes));
    if (!w.V) QF_HIP(hipMalloc((void **)&w.V, mbytes));
    if (!w.ray) QF_HIP(hipMalloc((void **)&w.ray, N * sizeof(cplx)));
    if (!w.sig) QF_HIP(hipMalloc((void **)&w.sig, N * sizeof(double)));
    if (!w.perm) QF_HIP(hipMalloc((void **)&w.perm, N * sizeof(int)));
    if (!w.word) QF_HIP(hipMalloc((void **)&w.word, 2 * sizeof(unsigned long long)));
    return QF_OK;
}

// Decomposes the Hermitian matrix in ctx->eigh.H.  On return ctx->eigh.G holds V^H with its rows in the order the sweeps
// left them, `lam` the ascending eigenvalues, and -- with sorted_V -- ctx->eigh.V the matrix V whose column j belongs to
// lam[j].  Everything is queued on the context's stream; the stream is idle on return except for the last transpose.
int eigh_core(qf_ctx *ctx, std::vector<double> &lam, bool sorted_V, qf_eigh_stats *stats)
{
    qf_eigh_ws &w = ctx->eigh;
    const int N = ctx->N, n = N + (N & 1);
    double norm = 0.0;
    QF_TRY(qf_launch_norm_inf(ctx, w.H, ctx->scalars));
    QF_TRY(read_scalar(ctx, ctx->scalars, &norm));
    if (!QF_FINITE(norm)) {
        qf_set_error("eigh: the matrix has an inf or NaN entry");
        return QF_ERR_NONFINITE;
    }
    const double shift = 2.0 * norm;
    if (stats) *stats = qf_eigh_stats{0, 0, 0.0};
    lam.assign((size_t)N, 0.0);
    if (!(shift > 0.0) || !QF_FINITE(shift)) {
        if (shift > 0.0) {
            qf_set_error("eigh: |H|_inf = %g is too large to shift by", norm);
            return QF_ERR_NONFINITE;
        }
        // H = 0: lambda = 0, V = I (nothing to divide by)
        QF_TRY(qf_launch_eigh_neg_i(ctx, nullptr, w.G));
        if (sorted_V) QF_TRY(qf_launch_eigh_neg_i(ctx, nullptr, w.V));
        return QF_OK;
    }
    QF_TRY(qf_launch_lincomb(ctx, 1.0, w.H, 0.0, (const cplx *)nullptr, shift, w.G));     // A = H + c I
    unsigned long long *host_word = reinterpret_cast<unsigned long long *>(ctx->host_scalars + 8);
    int sweeps = 0;
    long long rotations = 0;
    double off = 0.0;
    for (;;) {
        if (sweeps == EIGH_MAX_SWEEPS) {
            qf_set_error("eigh: %d sweeps did not bring every |c|/sqrt(ab) below %.3g (last sweep: %.3g)", sweeps, EIGH_TOL, off);
            return QF_ERR_NOCONVERGE;
        }
        QF_HIP(hipMemsetAsync(w.word, 0, 2 * sizeof(unsigned long long), ctx->stream));
        for (int round = 0; round < n - 1; ++round) QF_TRY(qf_launch_eigh_round(ctx, w.G, round, EIGH_TOL, w.word));
        QF_HIP(hipMemcpyAsync(host_word, w.word, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        QF_HIP(hipStreamSynchronize(ctx->stream));
        ++sweeps;
        memcpy(&off, &host_word[0], sizeof(double));
        rotations += (long long)host_word[1];
        if (stats) *stats = qf_eigh_stats{sweeps, rotations, off};
        if (!QF_FINITE(off)) {
            qf_set_error("eigh: a row norm overflowed or vanished (|H|_inf = %g)", norm);
            return QF_ERR_NONFINITE;
        }
        if (off <= EIGH_TOL) break;
    }
    // V^H = G with unit rows; lambda_j = Re(v_j^H H v_j), the Rayleigh quotient with the unshifted matrix
    QF_TRY(qf_launch_eigh_normalise(ctx, w.G, w.sig));
    QF_TRY(qf_launch_zgemm(ctx, w.G, w.H, w.V, nullptr));
    QF_TRY(qf_launch_eigh_rowdot(ctx, w.V, w.G, w.ray));
    std::vector<cplx> ray((size_t)N);
    QF_HIP(hipMemcpyAsync(ray.data(), w.ray, (size_t)N * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int> perm((size_t)N);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int i, int j) { return ray[(size_t)i].x < ray[(size_t)j].x; });
    for (int j = 0; j < N; ++j) lam[(size_t)j] = ray[(size_t)perm[(size_t)j]].x;
    if (sorted_V) {
        QF_HIP(hipMemcpyAsync(w.perm, perm.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        QF_TRY(qf_launch_eigh_conj_transpose(ctx, w.G, w.perm, nullptr, w.V));
        QF_HIP(hipStreamSynchronize(ctx->stream));      // (`perm` is host memory of this frame)
    }
    return QF_OK;
}

int eigh_finish(qf_ctx *ctx, const std::vector<double> &lam, double *lambda_host, void *V_host)
{
    memcpy(lambda_host, lam.data(), lam.size() * sizeof(double));
    if (V_host) {
        QF_HIP(hipMemcpyAsync(V_host, ctx->eigh.V, (size_t)ctx->N * ctx->N * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
        QF_HIP(hipStreamSynchronize(ctx->stream));
    }
    return QF_OK;
}

}  // namespace

extern "C" {

int qf_eigh(qf_ctx *ctx, const void *H_host, double *lambda_host, void *V_host, qf_eigh_stats *stats)
{
    QF_TRY(check_ctx(ctx));
    if (!H_host || !lambda_host) {
        qf_set_error("qf_eigh: null buffer");
        return QF_ERR_INVALID;
    }
    QF_TRY(eigh_alloc(ctx));
    QF_HIP(hipMemcpyAsync(ctx->eigh.H, H_host, (size_t)ctx->N * ctx->N * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    std::vector<double> lam;
    QF_TRY(eigh_core(ctx, lam, V_host != nullptr, stats));
    return eigh_finish(ctx, lam, lambda_host, V_host);
}

int qf_eigh_skew(qf_ctx *ctx, const void *W_host, double *lambda_host, void *V_host, qf_eigh_stats *stats)
{
    QF_TRY(check_ctx(ctx));
    if (!W_host || !lambda_host) {
        qf_set_error("qf_eigh_skew: null buffer");
        return QF_ERR_INVALID;
    }
    QF_TRY(eigh_alloc(ctx));
    QF_HIP(hipMemcpyAsync(ctx->eigh.G, W_host, (size_t)ctx->N * ctx->N * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    QF_TRY(qf_launch_eigh_neg_i(ctx, ctx->eigh.G, ctx->eigh.H));
    std::vector<double> lam;
    QF_TRY(eigh_core(ctx, lam, V_host != nullptr, stats));
    return eigh_finish(ctx, lam, lambda_host, V_host);
}

int qf_eigh_state(qf_ctx *ctx, double *lambda_host, qf_eigh_stats *stats)
{
    QF_TRY(check_ctx(ctx));
    if (!lambda_host) {
        qf_set_error("qf_eigh_state: null buffer");
        return QF_ERR_INVALID;
    }
    QF_TRY(eigh_alloc(ctx));
    QF_TRY(qf_launch_eigh_neg_i(ctx, ctx->W, ctx->eigh.H));
    std::vector<double> lam;
    QF_TRY(eigh_core(ctx, lam, false, stats));
    return eigh_finish(ctx, lam, lambda_host, nullptr);
}

// Ws = V diag(diag(V^H W V)) V^H with V the eigenvectors of P, Wr = W - Ws.  Uses the context's per-iteration staging
// matrices (stage, Phalf, PW, Whalf), which are free between stepper calls; the resident state and a carried increment
// are not touched.
int qf_scale_decomposition(qf_ctx *ctx, const void *W_host, const void *P_host, void *Ws_host, void *Wr_host)
{
    QF_TRY(check_ctx(ctx));
    if (!Ws_host || !Wr_host) {
        qf_set_error("qf_scale_decomposition: null output");
        return QF_ERR_INVALID;
    }
    QF_TRY(eigh_alloc(ctx));
    qf_eigh_ws &w = ctx->eigh;
    const size_t bytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    const cplx *W = ctx->W;
    if (W_host) {
        QF_HIP(hipMemcpyAsync(ctx->stage, W_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        W = ctx->stage;
    }
    if (P_host) QF_HIP(hipMemcpyAsync(ctx->Phalf, P_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    else QF_TRY(qf_launch_solve(ctx, ctx->poisson, W, ctx->Phalf, 1.0, 1));
    QF_TRY(qf_launch_eigh_neg_i(ctx, ctx->Phalf, w.H));
    std::vector<double> lam;
    QF_TRY(eigh_core(ctx, lam, false, nullptr));
    QF_TRY(qf_launch_zgemm(ctx, w.G, W, w.V, nullptr));                              // V^H W
    QF_TRY(qf_launch_eigh_rowdot(ctx, w.V, w.G, w.ray));                             // d_j = v_j^H W v_j
    QF_TRY(qf_launch_eigh_conj_transpose(ctx, w.G, nullptr, w.ray, ctx->PW));        // V diag(d)
    QF_TRY(qf_launch_zgemm(ctx, ctx->PW, w.G, ctx->Whalf, nullptr));                 // Ws = V diag(d) V^H
    QF_TRY(qf_launch_lincomb(ctx, 1.0, W, -1.0, ctx->Whalf, 0.0, ctx->Phalf));       // Wr = W - Ws
    QF_HIP(hipMemcpyAsync(Ws_host, ctx->Whalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipMemcpyAsync(Wr_host, ctx->Phalf, bytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

}  // extern "C"
