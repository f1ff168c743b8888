// isomp_fixedpoint with HOST HOOKS (quflow/integrators/isospectral.py:338-613): `forcing(P, W[, time])`, a foreign
// `hamiltonian(W[, time])`,
// `strang_splitting(h, W)`, `callback(W, dW)`, the general (not skew-Hermitian) branch of
// select_skewherm(False), and all of these -- plus compsum -- on (k,N,N) stacks of states.
//
// The state, the iteration vector dW, Whalf, the products and the Kahan term stay on the device for the
// whole call.  A hook is a C function pointer; what it needs crosses PCIe through pinned staging
// buffers, and nothing else does:
//     foreign hamiltonian : Whalf down, P up                       (2 matrices per iteration)
//     forcing             : P and Whalf down (Whalf only once if the Hamiltonian took it), F up
//     strang_splitting    : W down and up, twice per step          (or a resident tridiagonal solve: none)
//     callback            : W and the commutator down, once per step
// An AFFINE forcing installed on the context (qf_set_forcing) is no hook: k_forcing_affine forms it from Phalf and Whalf where
// the loop would call the hook, and nothing crosses PCIe for it; qf_isomp_forced is the same loop on the context's resident
// state (no transfer at all).
// A STOCHASTIC forcing (qf_set_stochastic_forcing) is that affine forcing with a pattern F0 redrawn on the device at the top of
// every step (stochastic.hip): three more launches per step, nothing else in the loop changes.
// The two products run on the fp64 matrix cores (k_zgemm, plain stores), one pass (k_hook_assemble)
// forms the commutator, dW, Whalf and the residual row sums, one pass (k_hook_update) the step's
// update; the exit test reads one scalar back per iteration (the hooks synchronise the host anyway).
#include <cmath>
#include <limits>
#include <vector>

#include "qf_api.h"

#pragma clang fp contract(off)   // the reference's passes are separate numpy operations: no fused multiply-adds

namespace {

constexpr int TH = 32;   // tile of the assemble / update passes

// One pass after the two products of an iteration (isospectral.py:499-534):
//     comm = SKEW ? PW - PW^H (conj_subtract_, :66-81, :503) : PW as it comes (the caller has already
//            subtracted Whalf @ Phalf, :505)
//     dW   = T + comm [+ F]          T = PW @ Phalf came into the dW buffer (:499), F = forcing * dt/2 (:519-520)
//     Whalf = W + dW                 (:481-482 of the next iteration)
//     rowpart[slot][row] = sum over the slot's columns of |dW_old - dW|      (:526-534)
// comm replaces PW in place (the update and the callback want it, :547-551).  Block (bi, bj), bi <= bj,
// handles the tile pair (bi,bj), (bj,bi): the in-place transposed difference needs both before either is
// overwritten.
template <bool SKEW>
__global__ __launch_bounds__(256) void k_hook_assemble(int N, cplx *__restrict__ PW, cplx *__restrict__ dW, const cplx *__restrict__ F,
                                                        const cplx *__restrict__ W, cplx *__restrict__ Whalf,
                                                        const cplx *__restrict__ dW_old, double *__restrict__ rowpart)
{
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (SKEW && bj < bi) return;
    __shared__ cplx Ta[TH][TH + 1], Tb[TH][TH + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int i0 = bi * TH, j0 = bj * TH;
    if (SKEW) {
        for (int r = ty; r < TH; r += 8) {
            const int gi = i0 + r, gj = j0 + tx;              // tile (bi,bj), row-coalesced
            Ta[r][tx] = (gi < N && gj < N) ? PW[(size_t)gi * N + gj] : make_double2(0.0, 0.0);
            const int hi = j0 + r, hj = i0 + tx;              // tile (bj,bi)
            Tb[r][tx] = (hi < N && hj < N) ? PW[(size_t)hi * N + hj] : make_double2(0.0, 0.0);
        }
        __syncthreads();
    }
    // the two tiles of the pair (one when bi == bj, or in the general branch)
    const int ntiles = (SKEW && bi != bj) ? 2 : 1;
    for (int which = 0; which < ntiles; ++which) {
        const int r0 = which ? j0 : i0, c0 = which ? i0 : j0, slot = which ? bi : bj;
        for (int r = ty; r < TH; r += 8) {
            const int gi = r0 + r, gj = c0 + tx;
            double a = 0.0;
            if (gi < N && gj < N) {
                const size_t e = (size_t)gi * N + gj;
                cplx c;
                if (SKEW) {
                    const cplx p = which ? Tb[r][tx] : Ta[r][tx];
                    const cplx q = which ? Ta[tx][r] : Tb[tx][r];     // PW[gj, gi]
                    c = make_double2(p.x - q.x, p.y + q.y);           // a - conj(a^T)
                } else {
                    c = PW[e];            // general branch: PW - Whalf @ Phalf was formed by the caller (:505)
                }
                if (SKEW) PW[e] = c;
                cplx d = dW[e];
                d.x += c.x;
                d.y += c.y;
                if (F) {
                    const cplx f = F[e];
                    d.x += f.x;
                    d.y += f.y;
                }
                dW[e] = d;
                const cplx w = W[e];
                Whalf[e] = make_double2(w.x + d.x, w.y + d.y);
                const cplx o = dW_old[e];
                const double er = o.x - d.x, ei = o.y - d.y;
                a = qf_modulus(er, ei);
            }
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);   // the 32 columns of this tile row
            if (rowpart && tx == 0 && gi < N) rowpart[(size_t)slot * N + gi] = a;
        }
    }
}

// End of a step (isospectral.py:547-596): W += 2 comm (`PWcomm *= 2; W += PWcomm`, Kahan-compensated
// with the persistent term kc when KAHAN, :553-586), then W += 2 F (`FW *= 2; W += FW`, :594-596);
// Whalf = W + dW for the next step (dW zeroed first when `reinitialize`, :471-472).
template <bool KAHAN>
__global__ __launch_bounds__(256) void k_hook_update(size_t n, const cplx *__restrict__ comm, const cplx *__restrict__ F,
                                                      cplx *__restrict__ W, cplx *__restrict__ kc, cplx *__restrict__ dW,
                                                      int reinitialize, cplx *__restrict__ Whalf)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const cplx c = comm[e];
        const double dr = 2.0 * c.x, di = 2.0 * c.y;
        cplx w = W[e];
        if (KAHAN) {
            cplx k = kc[e];
            const double yr = dr - k.x, yi = di - k.y;
            const double tr = w.x + yr, ti = w.y + yi;
            k.x = (tr - w.x) - yr;
            k.y = (ti - w.y) - yi;
            kc[e] = k;
            w.x = tr;
            w.y = ti;
        } else {
            w.x += dr;
            w.y += di;
        }
        if (F) {
            const cplx f = F[e];
            w.x += 2.0 * f.x;
            w.y += 2.0 * f.y;
        }
        W[e] = w;
        if (reinitialize) {
            dW[e] = make_double2(0.0, 0.0);
            Whalf[e] = w;
        } else {
            const cplx d = dW[e];
            Whalf[e] = make_double2(w.x + d.x, w.y + d.y);
        }
    }
}

// magmp with forcing: the force term joins the iteration vector AFTER the magnetic terms (mhd.py:389-402:
// dW += PWcomm; the three magnetic updates of dW[0]; then dW += FW): dW += F, Whalf = W + dW, and -- state 0 --
// the row sums of |dW_old - dW| again (one slot per 32-column tile, as k_magnetic_fix leaves them)
__global__ __launch_bounds__(256) void k_hook_add_forcing(int N, const cplx *__restrict__ F, cplx *__restrict__ dW,
                                                          const cplx *__restrict__ dW_old, const cplx *__restrict__ W,
                                                          cplx *__restrict__ Whalf, double *__restrict__ rowpart)
{
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int i0 = blockIdx.y * TH, j0 = blockIdx.x * TH;
    for (int r = ty; r < TH; r += 8) {
        const int gi = i0 + r, gj = j0 + tx;
        double a = 0.0;
        if (gi < N && gj < N) {
            const size_t e = (size_t)gi * N + gj;
            const cplx f = F[e];
            cplx d = dW[e];
            d.x += f.x;
            d.y += f.y;
            dW[e] = d;
            const cplx w = W[e];
            Whalf[e] = make_double2(w.x + d.x, w.y + d.y);
            if (rowpart) {
                const cplx o = dW_old[e];
                const double er = o.x - d.x, ei = o.y - d.y;
                a = qf_modulus(er, ei);
            }
        }
        if (rowpart) {
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
            if (tx == 0 && gi < N) rowpart[(size_t)blockIdx.x * N + gi] = a;
        }
    }
}

// The installed affine forcing (qf_set_forcing), one pass, one entry per lane (16-byte loads and stores, consecutive lanes
// on consecutive entries):
//     p = Ph * pscale;  f = F0;  f += a_W X;  f += a_P p;  f += a_lap (Delta X);  out = s f
// on real and imaginary parts separately, every product and sum rounded on its own (no fused multiply-add), a term whose
// coefficient is zero (or an absent F0) skipped altogether: which terms there are is the template argument TERMS (bit 0 F0,
// 1 a_W, 2 a_P, 3 a_lap), decided by the launcher.  Delta X is qf_laplace_entry: k_laplace's bits.  N <= 8192: the flat
// index (and one grid stride past its end) fits 32 bits.
template <int TERMS>
__global__ __launch_bounds__(256) void k_forcing_affine(int N, unsigned n, const cplx *__restrict__ F0, const cplx *__restrict__ X,
                                                         const cplx *__restrict__ Ph, cplx *__restrict__ out, double aW, double aP,
                                                         double alap, double pscale, double s)
{
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < n; e += gridDim.x * 256u) {
        double fr = 0.0, fi = 0.0;
        if (TERMS & 1) {
            const cplx f = F0[e];
            fr = f.x;
            fi = f.y;
        }
        if (TERMS & 2) {
            const cplx x = X[e];
            fr = fr + aW * x.x;
            fi = fi + aW * x.y;
        }
        if (TERMS & 4) {
            const cplx p = Ph[e];
            const double pr = p.x * pscale, pi = p.y * pscale;
            fr = fr + aP * pr;
            fi = fi + aP * pi;
        }
        if (TERMS & 8) {
            const int i = (int)(e / (unsigned)N), j = (int)(e - (unsigned)i * (unsigned)N);
            const cplx l = qf_laplace_entry<double, cplx>(N, X, i, j);
            fr = fr + alap * l.x;
            fi = fi + alap * l.y;
        }
        out[e] = make_double2(s * fr, s * fi);
    }
}

template <int TERMS>
void launch_forcing_terms(qf_ctx *ctx, const cplx *Ph, const cplx *X, cplx *out, double pscale, double s)
{
    const unsigned n = (unsigned)ctx->N * (unsigned)ctx->N;
    const unsigned blocks = (n + 255u) / 256u < 2048u ? (n + 255u) / 256u : 2048u;      // (8 per CU; the rest by the grid stride)
    hipLaunchKernelGGL(k_forcing_affine<TERMS>, dim3(blocks), dim3(256), 0, ctx->stream, ctx->N, n, ctx->forcing_f0, X, Ph,
                       out, ctx->forcing_aW, ctx->forcing_aP, ctx->forcing_alap, pscale, s);
}

int launch_assemble(qf_ctx *ctx, bool skew, cplx *PW, cplx *dW, const cplx *F, const cplx *W, cplx *Whalf, const cplx *dW_old,
                    double *rowpart)
{
    const int tiles = (ctx->N + TH - 1) / TH;
    if (skew)
        hipLaunchKernelGGL(k_hook_assemble<true>, dim3(tiles, tiles), dim3(256), 0, ctx->stream, ctx->N, PW, dW, F, W, Whalf, dW_old,
                           rowpart);
    else
        hipLaunchKernelGGL(k_hook_assemble<false>, dim3(tiles, tiles), dim3(256), 0, ctx->stream, ctx->N, PW, dW, F, W, Whalf, dW_old,
                           rowpart);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int launch_update(qf_ctx *ctx, const cplx *comm, const cplx *F, cplx *W, cplx *kc, cplx *dW, int reinitialize, cplx *Whalf)
{
    const size_t n = (size_t)ctx->N * ctx->N;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    if (kc) hipLaunchKernelGGL(k_hook_update<true>, dim3(blocks), dim3(256), 0, ctx->stream, n, comm, F, W, kc, dW, reinitialize, Whalf);
    else hipLaunchKernelGGL(k_hook_update<false>, dim3(blocks), dim3(256), 0, ctx->stream, n, comm, F, W, kc, dW, reinitialize, Whalf);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

}  // namespace

int qf_launch_forcing_affine(qf_ctx *ctx, const cplx *Ph, const cplx *X, cplx *out, double pscale, double s)
{
    if (!ctx->forcing_on) {
        qf_set_error("qf_launch_forcing_affine: no forcing is installed");
        return QF_ERR_STATE;
    }
    typedef void (*launcher)(qf_ctx *, const cplx *, const cplx *, cplx *, double, double);
    static const launcher table[16] = {
        launch_forcing_terms<0>,  launch_forcing_terms<1>,  launch_forcing_terms<2>,  launch_forcing_terms<3>,
        launch_forcing_terms<4>,  launch_forcing_terms<5>,  launch_forcing_terms<6>,  launch_forcing_terms<7>,
        launch_forcing_terms<8>,  launch_forcing_terms<9>,  launch_forcing_terms<10>, launch_forcing_terms<11>,
        launch_forcing_terms<12>, launch_forcing_terms<13>, launch_forcing_terms<14>, launch_forcing_terms<15>};
    const int terms = (ctx->forcing_f0_on ? 1 : 0) | (ctx->forcing_aW != 0.0 ? 2 : 0) | (ctx->forcing_aP != 0.0 ? 4 : 0) |
                      (ctx->forcing_alap != 0.0 ? 8 : 0);
    table[terms](ctx, Ph, X, out, pscale, s);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

namespace {

// The loop of qf_isomp_hooked and of qf_isomp_forced, written once: what its stages share, and the stages in the order
// hooked_body runs them.  states_host != nullptr: the (k,N,N) state comes from the host and goes back there;  nullptr
// (k == 1): it is taken from the context's resident state ctx->W and returned to it by device copies -- no N^2 transfer in
// either direction, no pinned staging.
struct hooked_loop {
    qf_ctx *ctx;
    void *states_host;
    int k;
    double dt, tol;
    int compsum, reinitialize;
    const qf_isomp_hooks *hooks;

    // per state: W, dW[2], Whalf, PW (-> comm), F, Kahan term; shared: C3 (general branch), magmp: Bhalf, BT, BTP
    static constexpr size_t per = 7;
    struct st { cplx *W, *dW[2], *Whalf, *PW, *F, *kc; int cur; };
    std::vector<st> S;
    bool resident = false, dev_forced = false, magnetic = false, skew = false, forced = false, foreign = false;
    bool per_state = false, states_p_open = false;
    int N = 0, slots = 0;
    size_t NN = 0, mbytes = 0;
    double vareps = 0.0, time = 0.0;
    cplx *C3 = nullptr, *Bhalf = nullptr, *BT = nullptr, *BTP = nullptr, *hW = nullptr, *hP = nullptr, *hF = nullptr;

    cplx *Pj(int j) const { return per_state ? ctx->multi[per * k + 4 + j] : ctx->Phalf; }     // state j's Phalf

    int too_many_stream_matrices() const
    {
        qf_set_error("qf_isomp_hooked: a Hamiltonian with one stream matrix per state takes at most 48 states (k=%d)", k);
        return QF_ERR_UNSUPPORTED;
    }

    // ---- set-up, first half: what the call may be asked, and what kind of run it is
    int setup(int steps)
    {
        resident = states_host == nullptr;
        if (!hooks || k < 1 || steps < 0 || (resident && k != 1)) {
            qf_set_error("qf_isomp_hooked: bad arguments (k=%d, steps=%d)", k, steps);
            return QF_ERR_INVALID;
        }
        // an installed forcing (qf_set_forcing) is applied on the device where the host hook is absent: one (N,N) state, not magmp
        if (ctx->forcing_on && (k > 1 || hooks->magnetic)) return qf_refuse_forcing(ctx, k > 1 ? "qf_isomp_hooked on a stack" : "qf_isomp_hooked (magmp)");
        if (ctx->forcing_on && hooks->forcing) {
            qf_set_error("qf_isomp_hooked: a forcing is installed on this context (qf_set_forcing) and a `forcing` hook is given as well");
            return QF_ERR_UNSUPPORTED;
        }
        dev_forced = ctx->forcing_on;
        if (compsum && (hooks->forcing || dev_forced) && steps > 0) {   // isospectral.py:588-589
            qf_set_error("Compensated sum with forcing is not yet implemented.");
            return QF_ERR_UNSUPPORTED;
        }
        N = ctx->N;
        NN = (size_t)N * N;
        mbytes = NN * sizeof(cplx);
        vareps = dt / (2 * qf_hbar(N));           // isospectral.py:436-437
        magnetic = hooks->magnetic != 0;
        if (magnetic && (k != 2 || compsum || !hooks->skewh || hooks->strang || hooks->strang_table)) {
            qf_set_error("qf_isomp_hooked: magmp (mhd.py:235-456) takes a (2,N,N) state, skew-Hermitian matrices, no compsum, no strang_splitting");
            return QF_ERR_INVALID;
        }
        skew = hooks->skewh != 0;
        forced = hooks->forcing != nullptr || dev_forced;
        foreign = hooks->hamiltonian != nullptr;
        time = hooks->time;
        ctx->w_skew_known = false;
        ctx->increment_valid = false;

        // states_p: the foreign Hamiltonian returns one stream matrix PER STATE ((k,N,N): np.matmul batches the products)
        // states_p < 0: the caller does not know yet -- the hook stores 0 or 1 into the field during its FIRST call and the
        // answer is read back behind that call (no entry probe: the user's function is evaluated as often as the reference
        // evaluates it); the k stream matrices are reserved up front while that is open
        per_state = foreign && hooks->states_p > 0 && !magnetic && k > 1;
        states_p_open = foreign && hooks->states_p < 0 && !magnetic && k > 1;
        if (per_state && k > 48) return too_many_stream_matrices();
        return QF_OK;
    }

    // ---- set-up, second half: the buffers, the state on the device, the tolerance
    int buffers()
    {
        QF_TRY(qf_need_matrices(ctx, ctx->multi, per * k + 4 + ((per_state || (states_p_open && k <= 48)) ? (size_t)k : 0)));
        if (!resident) QF_TRY(qf_need_hook_host(ctx, k));
        S.resize((size_t)k);
        for (int j = 0; j < k; ++j) {
            cplx **b = &ctx->multi[per * j];
            S[j] = {b[0], {b[1], b[2]}, b[3], b[4], b[5], b[6], 0};
            if (resident) QF_HIP(hipMemcpyAsync(S[j].W, ctx->W, mbytes, hipMemcpyDeviceToDevice, ctx->stream));
            else QF_HIP(hipMemcpyAsync(S[j].W, (const char *)states_host + (size_t)j * mbytes, mbytes, hipMemcpyHostToDevice, ctx->stream));
            QF_HIP(hipMemsetAsync(S[j].dW[0], 0, mbytes, ctx->stream));                      // dW = zeros_like(W), :430
            QF_HIP(hipMemcpyAsync(S[j].Whalf, S[j].W, mbytes, hipMemcpyDeviceToDevice, ctx->stream));
            if (compsum) QF_HIP(hipMemsetAsync(S[j].kc, 0, mbytes, ctx->stream));             // :457
        }
        C3 = ctx->multi[per * k];
        Bhalf = ctx->multi[per * k + 1], BT = ctx->multi[per * k + 2], BTP = ctx->multi[per * k + 3];
        hW = ctx->hook_host[0], hP = ctx->hook_host[1], hF = ctx->hook_host[2];
        slots = (N + TH - 1) / TH;
        if (!ctx->multi_rowpart) QF_HIP(hipMalloc((void **)&ctx->multi_rowpart, (size_t)2 * slots * N * sizeof(double)));   // (second half: magmp's second state, finite check)

        // tolerance from state 0 (isospectral.py:440-452)
        if (tol < 0) {
            double mach_eps = std::numeric_limits<double>::epsilon();
            if (!compsum) mach_eps = std::sqrt(mach_eps);
            QF_TRY(auto_tolerance(ctx, S[0].W, mach_eps * dt / qf_hbar(N), &tol));
        }
        return QF_OK;
    }

    int download_stack(cplx *dst, int which)      // which: 0 W, 1 Whalf, 2 comm (in PW)
    {
        for (int j = 0; j < k; ++j) {
            const cplx *src = which == 0 ? S[j].W : which == 1 ? S[j].Whalf : S[j].PW;
            QF_HIP(hipMemcpyAsync(dst + (size_t)j * NN, src, mbytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        QF_HIP(hipStreamSynchronize(ctx->stream));
        return QF_OK;
    }

    // half a Strang step on the state (isospectral.py:466-467, 598-599); Whalf = W + dW afterwards
    int strang_half()
    {
        if (hooks->strang_table) {
            for (int j = 0; j < k; ++j) {
                cplx *saveW = ctx->W;
                ctx->W = S[j].W;                 // the resident form of qf_solve_tridiagonal works on ctx->W
                const int rc = qf_solve_tridiagonal(ctx, hooks->strang_table, hooks->strang_key, nullptr, nullptr, hooks->solve_skewh);
                ctx->W = saveW;
                QF_TRY(rc);
            }
        } else if (hooks->strang) {
            QF_TRY(download_stack(hW, 0));
            const int rc = hooks->strang(hooks->user, dt / 2, hW);
            if (rc) return hook_failed("strang_splitting", rc);
            for (int j = 0; j < k; ++j)
                QF_HIP(hipMemcpyAsync(S[j].W, hW + (size_t)j * NN, mbytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            return QF_OK;
        }
        for (int j = 0; j < k; ++j) QF_TRY(qf_launch_lincomb(ctx, 1.0, S[j].W, 1.0, S[j].dW[S[j].cur], 0.0, S[j].Whalf));
        return QF_OK;
    }

    // ---- Phalf = vareps * hamiltonian(Whalf)             :488-492
    // *have_whalf_host: the foreign Hamiltonian took Whalf down, the forcing hook need not
    int stream_matrices(bool *have_whalf_host)
    {
        *have_whalf_host = foreign;
        if (foreign) {
            QF_TRY(download_stack(hW, 1));
            const int rc = hooks->hamiltonian(hooks->user, hW, hP, hooks->hamiltonian_takes_time ? time + dt / 2 : 0.0);
            if (rc) return hook_failed("hamiltonian", rc);
            if (states_p_open) {
                states_p_open = false;
                per_state = hooks->states_p > 0;
                if (per_state && k > 48) return too_many_stream_matrices();
            }
            for (size_t e = 0; e < (magnetic ? 2 * NN : per_state ? (size_t)k * NN : NN); ++e) {   // Phalf *= vareps (magmp: Bhalf *= vareps too, mhd.py:375-376)
                hP[e].x *= vareps;
                hP[e].y *= vareps;
            }
            if (per_state) {
                for (int j = 0; j < k; ++j) QF_HIP(hipMemcpyAsync(Pj(j), hP + (size_t)j * NN, mbytes, hipMemcpyHostToDevice, ctx->stream));
            } else {
                QF_HIP(hipMemcpyAsync(ctx->Phalf, hP, mbytes, hipMemcpyHostToDevice, ctx->stream));
            }
            if (magnetic) QF_HIP(hipMemcpyAsync(Bhalf, hP + NN, mbytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            // (the flow's Hamiltonian: an installed one in the skew-Hermitian, non-magnetic mode -- magmp's is solve_mhd)
            if (hooks->solve_skewh && !magnetic) QF_TRY(qf_launch_hamiltonian(ctx, S[0].Whalf, ctx->Phalf, vareps));
            else QF_TRY(qf_launch_solve(ctx, ctx->poisson, S[0].Whalf, ctx->Phalf, vareps, hooks->solve_skewh ? 1 : 0));
            if (magnetic) {      // solve_mhd (mhd.py:10-18): B = laplace(Theta)
                QF_TRY(qf_launch_laplace(ctx, S[1].Whalf, Bhalf));
                QF_TRY(qf_launch_lincomb(ctx, vareps, Bhalf, 0.0, nullptr, 0.0, Bhalf));
            }
        }
        return QF_OK;
    }

    // ---- the products                                    :496-505
    int products()
    {
        for (int j = 0; j < k; ++j) {
            QF_TRY(qf_launch_zgemm(ctx, Pj(j), S[j].Whalf, S[j].PW, nullptr));                       // PWcomm = Phalf @ Whalf
            QF_TRY(qf_launch_zgemm(ctx, S[j].PW, Pj(j), S[j].dW[S[j].cur ^ 1], nullptr));            // dW = PWcomm @ Phalf
            if (!skew) {                                                                             // PWcomm -= Whalf @ Phalf
                QF_TRY(qf_launch_zgemm(ctx, S[j].Whalf, Pj(j), C3, nullptr));
                QF_TRY(qf_launch_lincomb(ctx, 1.0, S[j].PW, -1.0, C3, 0.0, S[j].PW));
            }
        }
        if (magnetic) {                                         // mhd.py:381,385
            QF_TRY(qf_launch_zgemm(ctx, Bhalf, S[1].Whalf, BT, nullptr));       // BThetacomm = Bhalf @ Thetahalf
            QF_TRY(qf_launch_zgemm(ctx, BT, ctx->Phalf, BTP, nullptr));         // BThetaPhalf = BThetacomm @ Phalf
        }
        return QF_OK;
    }

    // ---- forcing(Phalf / vareps, Whalf[, time + dt/2]) * dt/2     :512-520  (before Whalf is rewritten)
    int force_term(bool have_whalf_host)
    {
        if (dev_forced) {
            // the installed forcing, straight into the loop's F: p = Phalf * (1/vareps), F = (dt/2) f -- the roundings of the
            // host route below
            QF_TRY(qf_launch_forcing_affine(ctx, ctx->Phalf, S[0].Whalf, S[0].F, 1.0 / vareps, dt / 2));
        } else if (forced) {
            if (!foreign) QF_HIP(hipMemcpyAsync(hP, ctx->Phalf, mbytes, hipMemcpyDeviceToHost, ctx->stream));
            if (!have_whalf_host) QF_TRY(download_stack(hW, 1));
            else QF_HIP(hipStreamSynchronize(ctx->stream));
            const double inv = 1.0 / vareps;                    // `Phalf /= vareps`: numpy multiplies by the reciprocal
            for (size_t e = 0; e < (per_state ? (size_t)k * NN : NN); ++e) {
                hP[e].x *= inv;
                hP[e].y *= inv;
            }
            const int rc = hooks->forcing(hooks->user, hP, hW, hF, hooks->forcing_takes_time ? time + dt / 2 : 0.0);
            if (rc) return hook_failed("forcing", rc);
            const double half = dt / 2;
            for (size_t e = 0; e < (size_t)k * NN; ++e) {       // FW *= dt/2
                hF[e].x *= half;
                hF[e].y *= half;
            }
            for (int j = 0; j < k; ++j)
                QF_HIP(hipMemcpyAsync(S[j].F, hF + (size_t)j * NN, mbytes, hipMemcpyHostToDevice, ctx->stream));
        }
        return QF_OK;
    }

    // ---- comm, dW += comm [+ F], Whalf = W + dW, residual row sums      :500-534
    // `norms` (from minit on): every state's residual norm is formed, into the slots of read_stack_resnorm -- with one
    // stream matrix per state the exit test looks at all of them, with a shared one at state 0's, and the finite check
    // covers the whole stack either way; the states beyond the 48 slots (shared stream matrix only) are folded on the device
    // into scalars[8] (through scalars[9]).  magmp: state 0's row sums are completed by the magnetic terms, so its norm is
    // formed by exit_norm; the second state's is formed here, for the finite check alone (its force term has not joined yet:
    // a non-finite force shows in the next iteration's Whalf).
    int assemble_and_norms(bool norms)
    {
        if (norms && !magnetic && k > 48) QF_HIP(hipMemsetAsync(ctx->scalars + 8, 0, sizeof(double), ctx->stream));
        for (int j = 0; j < k; ++j) {
            double *rp = (j == 0 || !magnetic) ? ctx->multi_rowpart : ctx->multi_rowpart + (size_t)slots * N;
            QF_TRY(launch_assemble(ctx, skew, S[j].PW, S[j].dW[S[j].cur ^ 1], (forced && !magnetic) ? S[j].F : nullptr, S[j].W,
                                   S[j].Whalf, S[j].dW[S[j].cur], rp));
            if (norms && !magnetic) {
                QF_TRY(qf_launch_norm_from_rowpart(ctx, ctx->multi_rowpart, slots, ctx->scalars + (j < 48 ? 16 + j : 9)));
                if (j >= 48) QF_TRY(qf_launch_fold_nonfinite(ctx, ctx->scalars + 9, ctx->scalars + 8));
            }
            if (norms && magnetic && j == 1) QF_TRY(qf_launch_norm_from_rowpart(ctx, rp, slots, ctx->scalars + 17));
        }
        if (magnetic) {
            // the three magnetic updates of dW[0] (mhd.py:389-392), then the force term (:395-402), in that order
            QF_TRY(qf_launch_magnetic_fix(ctx, BTP, BT, S[0].dW[S[0].cur ^ 1], S[0].dW[S[0].cur], S[0].W, S[0].Whalf,
                                          ctx->multi_rowpart));
            if (forced) {
                for (int j = 0; j < k; ++j) {
                    hipLaunchKernelGGL(k_hook_add_forcing, dim3(slots, slots), dim3(256), 0, ctx->stream, N, S[j].F,
                                       S[j].dW[S[j].cur ^ 1], S[j].dW[S[j].cur], S[j].W, S[j].Whalf,
                                       j == 0 ? ctx->multi_rowpart : nullptr);
                    QF_HIP(hipGetLastError());
                }
            }
        }
        for (int j = 0; j < k; ++j) S[j].cur ^= 1;
        return QF_OK;
    }

    // ---- the exit test's residual norm                   :523-536
    int exit_norm(double *resnorm)
    {
        if (magnetic) QF_TRY(qf_launch_norm_from_rowpart(ctx, ctx->multi_rowpart, slots, ctx->scalars + 16));
        return read_stack_resnorm(ctx, k, per_state, resnorm);
    }

    // ---- callback(W, 2 comm) :547-551, then W += 2 comm [+ 2 F];  Whalf = W + dW :553-596, the clock :598-599
    int step_end()
    {
        if (hooks->callback) {
            QF_TRY(download_stack(hW, 0));
            QF_TRY(download_stack(hF, 2));
            for (size_t e = 0; e < (size_t)k * NN; ++e) {
                hF[e].x *= 2.0;
                hF[e].y *= 2.0;
            }
            const int rc = hooks->callback(hooks->user, hW, hF);
            if (rc) return hook_failed("callback", rc);
        }
        for (int j = 0; j < k; ++j)
            QF_TRY(launch_update(ctx, S[j].PW, forced ? S[j].F : nullptr, S[j].W, compsum ? S[j].kc : nullptr, S[j].dW[S[j].cur],
                                 reinitialize, S[j].Whalf));
        if (magnetic)                                               // W[0] += 2 BThetacomm (mhd.py:431,438)
            QF_TRY(qf_launch_magnetic_update(ctx, BT, S[0].W, reinitialize ? nullptr : S[0].dW[S[0].cur], S[0].Whalf));
        if (hooks->has_time) time += dt;
        return QF_OK;
    }
};

int hooked_body(qf_ctx *ctx, void *states_host, int k, double dt, int steps, double tol, int minit, int maxit,
                int compsum, int reinitialize, const qf_isomp_hooks *hooks, qf_isomp_stats *stats_out)
{
    QF_TRY(check_ctx(ctx));
    QF_TRY(check_iteration_args(minit, maxit));
    hooked_loop L{ctx, states_host, k, dt, tol, compsum, reinitialize, hooks};
    QF_TRY(L.setup(steps));
    QF_TRY(L.buffers());
    long long total_iterations = 0, number_of_maxit = 0;
    double resnorm = 0.0;
    const bool stochastic = L.dev_forced && ctx->stoch.on;
    for (int step = 0; step < steps; ++step) {
        // a stochastic forcing: this step's pattern F0_n, n = the run's counter, drawn into forcing_f0 (three launches,
        // stochastic.hip); constant over the step's iterations
        if (stochastic) QF_TRY(qf_launch_stoch_pattern(ctx, ctx->stoch.step + (unsigned long long)step, dt));
        QF_TRY(L.strang_half());
        resnorm = std::numeric_limits<double>::infinity();          // :470
        // (`reinitialize`: dW was zeroed and Whalf = W set by the previous step's update, or is so at entry)
        bool broke = false;
        for (int i = 0; i < maxit; ++i) {
            total_iterations += 1;                                  // :478
            const bool test = i + 1 >= minit;
            bool have_whalf_host = false;
            QF_TRY(L.stream_matrices(&have_whalf_host));
            QF_TRY(L.products());
            QF_TRY(L.force_term(have_whalf_host));
            QF_TRY(L.assemble_and_norms(test));
            if (test) {
                const double resnorm_old = resnorm;
                QF_TRY(L.exit_norm(&resnorm));
                if (resnorm <= L.tol || resnorm >= resnorm_old) {
                    broke = true;
                    break;
                }
            }
        }
        if (!broke) number_of_maxit += 1;                           // :538-540
        QF_TRY(L.step_end());
        QF_TRY(L.strang_half());
    }
    if (stochastic) ctx->stoch.step += (unsigned long long)steps;
    if (L.resident) QF_HIP(hipMemcpyAsync(ctx->W, L.S[0].W, L.mbytes, hipMemcpyDeviceToDevice, ctx->stream));
    for (int j = 0; j < k && !L.resident; ++j)
        QF_HIP(hipMemcpyAsync((char *)states_host + (size_t)j * L.mbytes, L.S[j].W, L.mbytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    fill_stats(stats_out, total_iterations, number_of_maxit, L.tol, resnorm);
    return QF_OK;
}

}  // namespace

extern "C" {

int qf_isomp_hooked(qf_ctx *ctx, void *states_host, int k, double dt, int steps, double tol, int minit, int maxit,
                    int compsum, int reinitialize, const qf_isomp_hooks *hooks, qf_isomp_stats *stats_out)
{
    if (ctx && !states_host) {
        qf_set_error("qf_isomp_hooked: bad arguments (k=%d, steps=%d)", k, steps);
        return QF_ERR_INVALID;
    }
    return hooked_body(ctx, states_host, k, dt, steps, tol, minit, maxit, compsum, reinitialize, hooks, stats_out);
}

// The hooked loop on the context's RESIDENT state with the installed forcing (none: no force term) and Hamiltonian: k = 1,
// the skew-Hermitian branch, no host hook; the Strang half step is the resident tridiagonal solve.
int qf_isomp_forced(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int reinitialize,
                    const double *strang_table, unsigned long long strang_key, qf_isomp_stats *stats_out)
{
    qf_isomp_hooks hooks = {};
    hooks.skewh = 1;
    hooks.solve_skewh = 1;
    hooks.strang_table = strang_table;
    hooks.strang_key = strang_key;
    return hooked_body(ctx, nullptr, 1, dt, steps, tol, minit, maxit, 0, reinitialize, &hooks, stats_out);
}

}  // extern "C"
