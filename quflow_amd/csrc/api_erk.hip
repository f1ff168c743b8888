// C ABI of libquflow_hip.so: the explicit Runge-Kutta steppers euler / heun / rk4 (quflow/integrators/erk.py:19-160), written
// once.  erk_body owns the Butcher sequence (a table per method), the per-state loop -- products A = P_j @ X_j, B = X_j @ P_j,
// then the stage kernel -- the skew-Hermitian probe that saves the second product, and the transfers of a host-in / host-out
// call.  The four entry points validate their arguments, name their buffers and say where P (and F) come from:
//     qf_erk                 ctx->W resident        the flow's Hamiltonian (skewh) or the general Poisson solve
//     qf_erk_states          (k,N,N) from the host  the same, from state 0, for every state
//     qf_erk_hooked          (N,N) from the host    host hooks through pinned staging, or the installed affine forcing
//     qf_erk_states_hooked   (k,N,N) from the host  host hooks; a foreign Hamiltonian may return one stream matrix per state
#include <functional>
#include <vector>

#include "qf_api.h"

namespace {

// One row per stage: the right-hand side K is taken at the state itself (from_state) or at the previous row's stage argument;
//     acc = c_acc == 0 ? K : acc + c_acc K;   want_wp: Xp = X + (dt / wp_div) K;   fin: X += (dt / fin_div) acc
// The step factors are dt DIVIDED by 1, 2, 6 (erk.py's `dt / 2.0`, `dt / 6.0`), never multiplied by a reciprocal.
struct erk_row { bool from_state; double c_acc; bool want_wp; double wp_div; bool fin; double fin_div; };
const erk_row EULER[] = {{true, 0.0, false, 1.0, true, 1.0}};                                 // erk.py:53-56
const erk_row HEUN[] = {{true, 0.0, true, 1.0, false, 1.0},                                   // F0; Wprime = W + dt*F0   (erk.py:91-110)
                        {false, 1.0, false, 1.0, true, 2.0}};                                 // F += F0; F *= dt/2; W += F
const erk_row RK4[] = {{true, 0.0, true, 2.0, false, 1.0},                                    // K1                       (erk.py:139-156)
                       {false, 2.0, true, 2.0, false, 1.0},                                   // K1 + 2 K2
                       {false, 2.0, true, 1.0, false, 1.0},                                   // ... + 2 K3
                       {false, 1.0, false, 1.0, true, 6.0}};                                  // ... + K4; W += (dt/6) * (...)
const struct { const erk_row *rows; int n; } METHODS[] = {{EULER, 1}, {HEUN, 2}, {RK4, 4}};   // by QF_ERK_EULER / _HEUN / _RK4

// a state's buffers: X the state, Xp the stage argument, acc the running combination of the slopes, F its force term
// (nullptr: none), P the stream matrix its products take (the source below may redirect it between stages)
struct erk_state { cplx *X, *Xp, *acc, *F, *P; };

// where the right-hand side comes from: `eval` fills every state's P (and F) for the stage argument -- X when from_state, else
// Xp -- before the products are launched; `late` (optional) runs behind the products of a state, before its stage kernel
struct erk_source { std::function<int(bool from_state)> eval, late; };

// host != nullptr: the states come from there and go back there.  probe: one product per stage (X@P = (P@X)^H) if every state
// is exactly skew-Hermitian.  clears_skew: ctx->w_skew_known is cleared and a carried increment ended -- the state is replaced and
// ctx->dW[0] is the stage accumulator -- (every entry but qf_erk_states, which leaves ctx->W and ctx->dW[] alone).
int erk_body(qf_ctx *ctx, std::vector<erk_state> &S, void *host, bool probe, bool clears_skew, int method, double dt, int steps,
             const erk_source &src)
{
    const size_t mbytes = (size_t)ctx->N * ctx->N * sizeof(cplx);
    const double inv_hb = 1.0 / qf_hbar(ctx->N);
    if (clears_skew) {
        ctx->w_skew_known = false;
        ctx->increment_valid = false;
    }
    bool one_product = probe;
    for (size_t j = 0; j < S.size(); ++j) {
        if (host) QF_HIP(hipMemcpyAsync(S[j].X, (const char *)host + j * mbytes, mbytes, hipMemcpyHostToDevice, ctx->stream));
        if (one_product) QF_TRY(qf_exactly_skew(ctx, S[j].X, &one_product));
    }
    cplx *A = ctx->PW, *B = one_product ? nullptr : ctx->stage;
    for (int s = 0; s < steps; ++s) {
        for (int r = 0; r < METHODS[method].n; ++r) {
            const erk_row &row = METHODS[method].rows[r];
            {
                prof_scope p(ctx, QF_KERNEL_POISSON);
                QF_TRY(src.eval(row.from_state));
            }
            // (every P is complete before state 0's stage overwrites its stage argument; the other states need only P)
            for (erk_state &st : S) {
                const cplx *Xarg = row.from_state ? st.X : st.Xp;
                {
                    prof_scope p(ctx, QF_KERNEL_GEMM1);
                    QF_TRY(qf_launch_zgemm(ctx, st.P, Xarg, A, nullptr));      // bracket(P, X) = (P@X - X@P)/hbar, geometry.py:41-49
                }
                if (B) {
                    prof_scope p(ctx, QF_KERNEL_GEMM2);
                    QF_TRY(qf_launch_zgemm(ctx, Xarg, st.P, B, nullptr));
                }
                if (src.late) QF_TRY(src.late(row.from_state));
                prof_scope p(ctx, QF_KERNEL_UPDATE);
                const bool no_acc = row.c_acc == 0.0 && !row.want_wp && row.fin;     // euler: the slope is used once
                QF_TRY(qf_launch_erk_stage(ctx, A, B, st.F, inv_hb, st.X, no_acc ? nullptr : st.acc, row.c_acc,
                                           row.want_wp ? st.Xp : nullptr, row.want_wp ? dt / row.wp_div : 0.0,
                                           row.fin ? st.X : nullptr, row.fin ? dt / row.fin_div : 0.0));
            }
        }
    }
    for (size_t j = 0; j < S.size() && host; ++j)
        QF_HIP(hipMemcpyAsync((char *)host + j * mbytes, S[j].X, mbytes, hipMemcpyDeviceToHost, ctx->stream));
    QF_HIP(hipStreamSynchronize(ctx->stream));
    return QF_OK;
}

// the plain entries: the flow's Hamiltonian (an installed one included) when skewh, else the general Poisson solve; state 0's
// stage argument gives the one stream matrix of a stack (solve_poisson reduces a stack to its first state, cpu.py:672-674,696-697)
erk_source plain_source(qf_ctx *ctx, std::vector<erk_state> &S, int skewh)
{
    return {[ctx, &S, skewh](bool from_state) -> int {
                const cplx *X = from_state ? S[0].X : S[0].Xp;
                if (skewh) return qf_launch_hamiltonian(ctx, X, S[0].P, 1.0);
                return qf_launch_solve(ctx, ctx->poisson, X, S[0].P, 1.0, 0);
            },
            nullptr};
}

// The hooked entries: a hook is a C function pointer on pinned copies (ctx->hook_host: stage arguments, P, F).  Per stage a
// foreign Hamiltonian moves the stage arguments down and P up; forcing moves P and the stage arguments down (those only once
// if the Hamiltonian already took them) and F up.  The stream is synchronised before either hook is called.
struct hooked_source {
    qf_ctx *ctx;
    const qf_isomp_hooks *hooks;
    std::vector<erk_state> &S;
    // hooks->states_p: the foreign Hamiltonian fills one stream matrix PER STATE of a stack (bracket(P, W) batched, erk.py with a
    // (k,N,N) P), otherwise one for all states; < 0: open until the hook's first call has stored the answer there
    bool per_state, states_p_open;
    bool have_x = false;     // this stage's arguments are in hook_host[0]

    hooked_source(qf_ctx *c, const qf_isomp_hooks *h, std::vector<erk_state> &s, bool stacked)
        : ctx(c), hooks(h), S(s), per_state(stacked && h->hamiltonian && h->states_p > 0),
          states_p_open(stacked && h->hamiltonian && h->states_p < 0) {}

    size_t NN() const { return (size_t)ctx->N * ctx->N; }
    int args_down(bool from_state)
    {
        if (have_x) return QF_OK;
        for (size_t j = 0; j < S.size(); ++j)
            QF_HIP(hipMemcpyAsync(ctx->hook_host[0] + j * NN(), from_state ? S[j].X : S[j].Xp, NN() * sizeof(cplx), hipMemcpyDeviceToHost,
                                  ctx->stream));
        have_x = true;
        return QF_OK;
    }
    int stream_matrix(bool from_state)
    {
        const size_t mbytes = NN() * sizeof(cplx);
        cplx *hX = ctx->hook_host[0], *hP = ctx->hook_host[1];
        have_x = false;
        if (!hooks->hamiltonian)
            return qf_launch_solve(ctx, ctx->poisson, from_state ? S[0].X : S[0].Xp, ctx->Phalf, 1.0, hooks->solve_skewh ? 1 : 0);
        QF_TRY(args_down(from_state));
        QF_HIP(hipStreamSynchronize(ctx->stream));
        const int rc = hooks->hamiltonian(hooks->user, hX, hP, 0.0);
        if (rc) return hook_failed("hamiltonian", rc);
        if (states_p_open) {
            states_p_open = false;
            per_state = hooks->states_p > 0;
        }
        for (size_t j = 0; j < S.size(); ++j) {
            S[j].P = per_state ? ctx->multi[5 * j + 4] : ctx->Phalf;
            if (per_state || j == 0) QF_HIP(hipMemcpyAsync(S[j].P, hP + (per_state ? j * NN() : 0), mbytes, hipMemcpyHostToDevice, ctx->stream));
        }
        return QF_OK;
    }
    int force_term(bool from_state)
    {
        const size_t mbytes = NN() * sizeof(cplx);
        cplx *hX = ctx->hook_host[0], *hP = ctx->hook_host[1], *hF = ctx->hook_host[2];
        // the installed affine forcing (qf_erk_hooked alone admits one): formed on the device, unscaled as the hook's is
        if (ctx->forcing_on) return qf_launch_forcing_affine(ctx, S[0].P, from_state ? S[0].X : S[0].Xp, S[0].F, 1.0, 1.0);
        if (!hooks->forcing) return QF_OK;
        if (!hooks->hamiltonian) QF_HIP(hipMemcpyAsync(hP, ctx->Phalf, mbytes, hipMemcpyDeviceToHost, ctx->stream));
        QF_TRY(args_down(from_state));
        QF_HIP(hipStreamSynchronize(ctx->stream));
        const int rc = hooks->forcing(hooks->user, hP, hX, hF, 0.0);
        if (rc) return hook_failed("forcing", rc);
        for (size_t j = 0; j < S.size(); ++j) QF_HIP(hipMemcpyAsync(S[j].F, hF + j * NN(), mbytes, hipMemcpyHostToDevice, ctx->stream));
        return QF_OK;
    }
};

}  // namespace

extern "C" {

// On the context's resident state, which keeps the result.  For skew-Hermitian data X@P = (P@X)^H: one product per stage.
int qf_erk(qf_ctx *ctx, int method, double dt, int steps, int skewh)
{
    QF_TRY(check_ctx(ctx));
    if (method < QF_ERK_EULER || method > QF_ERK_RK4) {
        qf_set_error("qf_erk: unknown method %d", method);
        return QF_ERR_INVALID;
    }
    if (steps < 0) {
        qf_set_error("qf_erk: steps must be >= 0");
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, "qf_erk"));
    std::vector<erk_state> S = {{ctx->W, ctx->Whalf, ctx->dW[0], nullptr, ctx->Phalf}};
    return erk_body(ctx, S, nullptr, skewh != 0, true, method, dt, steps, plain_source(ctx, S, skewh));
}

// On a stack of k states (erk.py:19-160 with W.shape = (k,N,N)): bracket(P, W) broadcasts state 0's stream matrix over the
// stack (geometry.py:41-49: P@W - W@P with numpy's batched matmul) -- every state is advected by state 0's flow, stage by
// stage.  Host in / host out; ctx->W is not touched.
int qf_erk_states(qf_ctx *ctx, void *states_host, int k, int method, double dt, int steps, int skewh)
{
    QF_TRY(check_ctx(ctx));
    if (method < QF_ERK_EULER || method > QF_ERK_RK4 || steps < 0 || k < 1 || !states_host) {
        qf_set_error("qf_erk_states: bad arguments (method %d, steps %d, k %d)", method, steps, k);
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, "qf_erk_states"));
    QF_TRY(qf_need_matrices(ctx, ctx->multi, (size_t)3 * k));          // per state: X (state), Xp (stage argument), acc
    std::vector<erk_state> S;
    for (int j = 0; j < k; ++j) S.push_back({ctx->multi[3 * j], ctx->multi[3 * j + 1], ctx->multi[3 * j + 2], nullptr, ctx->Phalf});
    return erk_body(ctx, S, states_host, skewh != 0, false, method, dt, steps, plain_source(ctx, S, skewh));
}

// With `forcing(P, W)` and / or a foreign `hamiltonian(W)`, or the installed affine forcing: both products always; the force
// term is formed behind the products' launches.
int qf_erk_hooked(qf_ctx *ctx, void *W_host, int method, double dt, int steps, const qf_isomp_hooks *hooks)
{
    QF_TRY(check_ctx(ctx));
    if (!W_host || !hooks || method < QF_ERK_EULER || method > QF_ERK_RK4 || steps < 0) {
        qf_set_error("qf_erk_hooked: bad arguments (method=%d, steps=%d)", method, steps);
        return QF_ERR_INVALID;
    }
    if (ctx->forcing_on && hooks->forcing) {
        qf_set_error("qf_erk_hooked: a forcing is installed on this context (qf_set_forcing) and a `forcing` hook is given as well");
        return QF_ERR_UNSUPPORTED;
    }
    if (ctx->forcing_on && ctx->stoch.on) {
        qf_set_error("qf_erk_hooked: a stochastic forcing is installed (qf_set_stochastic_forcing): noise inside Runge-Kutta "
                     "stages is not defined here; qf_isomp_forced and qf_isomp_hooked (k = 1) follow it");
        return QF_ERR_UNSUPPORTED;
    }
    QF_TRY(qf_need_hook_host(ctx, 1));
    QF_TRY(qf_need_matrices(ctx, ctx->multi, 1));
    std::vector<erk_state> S = {{ctx->W, ctx->Whalf, ctx->dW[0], (hooks->forcing || ctx->forcing_on) ? ctx->multi[0] : nullptr, ctx->Phalf}};
    hooked_source h(ctx, hooks, S, false);
    return erk_body(ctx, S, W_host, false, true, method, dt, steps,
                    {[&h](bool from_state) { return h.stream_matrix(from_state); }, [&h](bool from_state) { return h.force_term(from_state); }});
}

// The same on a (k,N,N) stack (erk.py with batched input): `hamiltonian(stack)` returns ONE (N,N) stream matrix (the built-in
// one solves for state 0, cpu.py:696-697) or one per state, `forcing(P, stack)` returns a stack; it is called before the
// products are launched.
int qf_erk_states_hooked(qf_ctx *ctx, void *states_host, int k, int method, double dt, int steps, const qf_isomp_hooks *hooks)
{
    QF_TRY(check_ctx(ctx));
    if (!states_host || !hooks || k < 1 || method < QF_ERK_EULER || method > QF_ERK_RK4 || steps < 0) {
        qf_set_error("qf_erk_states_hooked: bad arguments (k=%d, method=%d, steps=%d)", k, method, steps);
        return QF_ERR_INVALID;
    }
    QF_TRY(qf_refuse_forcing(ctx, "qf_erk_states_hooked"));
    QF_TRY(qf_need_hook_host(ctx, k));
    QF_TRY(qf_need_matrices(ctx, ctx->multi, (size_t)5 * k));          // per state: X, stage argument, accumulator, forcing term, stream matrix
    std::vector<erk_state> S;
    for (int j = 0; j < k; ++j) {
        cplx **b = &ctx->multi[(size_t)5 * j];
        S.push_back({b[0], b[1], b[2], hooks->forcing ? b[3] : nullptr, ctx->Phalf});
    }
    hooked_source h(ctx, hooks, S, true);
    auto both = [&h](bool from_state) -> int {
        QF_TRY(h.stream_matrix(from_state));
        return h.force_term(from_state);
    };
    return erk_body(ctx, S, states_host, false, true, method, dt, steps, {both, nullptr});
}

}  // extern "C"
