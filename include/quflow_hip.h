/*
 * quflow_hip.h -- C ABI of libquflow_hip.so, the MI355X (gfx950) implementation of
 * quflow's isospectral hot path:  W' = (1/hbar)[P, W],  Delta P = W  on su(N).
 *
 * The reference (klasmodin/quflow) is pure Python and has NO C/FFI boundary; its
 * plug points are Python call protocols.  Each entry point
 * below therefore names the reference *Python* interface it stands under; the
 * ctypes binding a maintainer adds on the reference side is in INTEGRATION.md and
 * the in-repo mirror of those protocols is quflow_amd/ (Python).
 *
 * Conventions
 *   - every function returns int: 0 = ok, non-zero = error; the message is
 *     available from qf_last_error() (thread-local).  Nothing throws across the ABI.
 *   - matrices are N x N, C order (row major), complex128 as interleaved
 *     (re, im) doubles -- exactly numpy's layout, so host buffers are passed as-is.
 *   - the caller owns host memory; the ctx owns device memory and a HIP stream.
 *     No host pointer is retained after a call returns.
 *   - one ctx is used by one host thread at a time; independent ctxs may run
 *     concurrently -- from separate processes (one per GPU) and from separate host
 *     threads of one process, several ctxs per GPU included (thread-local error text,
 *     per-ctx stream and control state; tests/test_hip_envelope.py proves it: two
 *     threads, N = 512 and N = 1024, bit-identical to the sequential runs).
 *   - N: 2 <= N <= 8192 (qf_ctx_create refuses anything else); every size class in
 *     that range is tested against the CPU oracle.
 *   - there is NO CPU fallback: every compute entry point fails with
 *     QF_ERR_NO_DEVICE when no HIP device is present.
 */
#ifndef QUFLOW_HIP_H
#define QUFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define QF_OK 0
#define QF_ERR_INVALID 1    /* bad argument */
#define QF_ERR_NO_DEVICE 2  /* no HIP device / device index out of range */
#define QF_ERR_HIP 3        /* a HIP runtime call failed */
#define QF_ERR_STATE 4      /* call sequence violated */
#define QF_ERR_CALLBACK 5   /* a host hook of qf_isomp_hooked / qf_erk_hooked returned non-zero */
#define QF_ERR_UNSUPPORTED 6 /* a combination the reference itself rejects (NotImplementedError) */
#define QF_ERR_NONFINITE 7  /* the residual a stepper's exit test looks at is inf or NaN: the reference's scipy.linalg.norm
                             * raises ValueError("array must not contain infs or NaNs") there (isospectral.py:534, check_finite).
                             * The call is closed ON THE DEVICE at that iteration (no later launch runs, nothing is written
                             * into W): the state is left as it was after the last completed step, as the reference's array is.
                             * (Residual entries above 1.3e154 count as non-finite here -- their squares overflow --, the
                             * reference's scaled abs() gives up at 1.8e308.) */
#define QF_ERR_NOCONVERGE 8 /* qf_eigh and its kin: the sweep cap was reached before every pair of vectors was orthogonal */

#define QF_VERSION 100      /* 0.1.0, tracks quflow.__version__ (quflow/__init__.py:18) */

typedef struct qf_ctx qf_ctx;

/* ---- library ---------------------------------------------------------- */
int qf_version(void);
const char *qf_last_error(void);
/* number of visible HIP devices (0 when there is none; never an error) */
int qf_device_count(void);

/* ---- context: mirrors IsompCUDA.__init__(N, dtype) / DiagTriDiagOp.__init__ of the
 *      reference's device precedent (quflow/experimental/isospectral_cuda.py:52-80,
 *      quflow/experimental/cuda.py:240-354): all device buffers, the factor tables of
 *      the tridiagonal Laplacian and the stream are created once per (device, N). --- */
int qf_ctx_create(int N, int device, qf_ctx **out);
int qf_ctx_destroy(qf_ctx *ctx);
int qf_ctx_size(const qf_ctx *ctx);                 /* N */
int qf_sync(qf_ctx *ctx);                           /* hipStreamSynchronize on the ctx stream */

/* ---- geometry: quflow/geometry.py:7-9  hbar(N) = 2/sqrt(N^2-1) ---------------- */
double qf_hbar(int N);

/* ---- Laplacian backend module protocol (quflow/laplacian/__init__.py:1,
 *      tests/test_laplacian.py:134-152,226-252) -------------------------------- */

/* laplacian(N, bc): quflow/laplacian/cpu.py:55-95,604-625.  Writes the (N,N,2) float64
 * coefficient table to host memory (computed by a device kernel). */
int qf_laplacian_table(qf_ctx *ctx, int bc, double *lap_host);

/* solve_poisson(W): quflow/laplacian/cpu.py:681-734 -> _solve_cpu_skewh (cpu.py:281-362)
 * when skewh != 0, _solve_cpu_nonskewh (cpu.py:200-278) when skewh == 0
 * (select_skewherm, cpu.py:563-591).  Host in, host out. */
int qf_solve_poisson(qf_ctx *ctx, const void *W_host, void *P_host, int skewh);

/* laplace(P): quflow/laplacian/cpu.py:628-669 -> _dot_cpu_generic (cpu.py:98-108). */
int qf_laplace(qf_ctx *ctx, const void *P_host, void *W_host);

/* _solve_cpu(lap, W, P, ...) with a caller-supplied (N,N,2) coefficient table: the
 * solver underneath solve_heat / solve_helmholtz / solve_viscdamp (cpu.py:737-943).
 * The factorisation of `lap_host` is cached in the ctx under `table_key` (any
 * non-zero caller-chosen id; pass 0 to refactor on every call).  The key must IDENTIFY
 * the content: two tables that differ anywhere need two keys (an id of the parameters the
 * table was built from, or a digest of all of its bytes).
 * W_host == P_host == NULL: the solve is applied to the context's resident state in place,
 * W <- T^-1 W, asynchronously -- a `strang_splitting` half step (solve_viscdamp with theta = 1,
 * isospectral.py:466-467, 598-599) between qf_isomp / qf_isomp_continue calls without PCIe. */
int qf_solve_tridiagonal(qf_ctx *ctx, const double *lap_host, unsigned long long table_key,
                         const void *W_host, void *P_host, int skewh);
/* The factor cache is bounded: least-recently-used entries are recycled once
 * QUFLOW_HIP_FACTOR_CACHE_MB (default 512) of device memory is reached, and a key that returns
 * with a different fingerprint is refactored.  The fingerprint is a safety net, not an identity: it
 * reads 4096 strided doubles of the 2 N^2 (stride 2 N^2 / 4096: from N = 64 on only diagonal
 * coefficients, never a coupling coefficient) plus the last one, and must not be relied on to tell
 * two tables apart.  Entries / bytes held: */
int qf_factor_cache_stats(qf_ctx *ctx, int *entries, unsigned long long *device_bytes);

/* ---- the Hamiltonian of the flow.  Built in: P = Delta^-1 W.  Installed: P = T^-1 (W - F) with T any tridiagonal
 * (N,N,2) coefficient table (global quasi-geostrophic, Charney-Hasegawa-Mima, Helmholtz-type operators) and F a fixed
 * N x N complex128 offset (Coriolis term, topography).  Every complex128 stepper of this library that forms the stream
 * matrix of the flow with the skew-Hermitian solve -- qf_isomp / _continue / _diag / _multi / _states, the native branch
 * of qf_isomp_hooked, qf_erk / qf_erk_states, qf_isomp_simple / _quasinewton -- follows what is installed on its context,
 * on the device: the offset is subtracted inside the solve kernel while it loads its right-hand side.
 *   table_host  (N,N,2) doubles, NULL = the built-in Laplacian.  Factorised into a pair the context owns (never recycled
 *               by the qf_solve_tridiagonal cache).
 *   offset_host N x N complex128, NULL = none.  Must be exactly skew-Hermitian: the solve reads its upper triangle only
 *               (the caller checks; quflow_amd.TridiagonalHamiltonian does).
 *   *_key       caller-chosen ids (0: always refactor / upload again).  A call that repeats the key AND the fingerprint
 *               of what the context still holds neither refactors nor uploads, so each key must IDENTIFY its content: two
 *               tables or two offsets that differ anywhere need two keys (quflow_amd.TridiagonalHamiltonian digests every
 *               byte, once, when it is constructed).  The fingerprint, as in qf_solve_tridiagonal, reads 4096 strided
 *               doubles plus the last one -- from N = 64 on real parts only of an offset, diagonal coefficients only of a
 *               table -- and must not be relied on to tell contents apart.
 * Not followed (they keep the built-in solve): the complex64 entry points, the general (skewh = 0) branches, magmp,
 * qf_solve_poisson, qf_diagnostics / qf_isomp_diag (energy_euler stays the Euler energy -<W, Delta^-1 W>/2),
 * qf_scale_decomposition. */
int qf_set_hamiltonian(qf_ctx *ctx, const double *table_host, unsigned long long table_key, const void *offset_host,
                       unsigned long long offset_key);
int qf_clear_hamiltonian(qf_ctx *ctx);      /* back to the built-in Poisson Hamiltonian (the buffers are kept) */
/* P = T^-1 (W - F) with what is installed; host in, host out */
int qf_hamiltonian(qf_ctx *ctx, const void *W_host, void *P_host);
/* H = -inner_L2(P, W - F)/2 of the resident state, P = T^-1 (W - F): the conserved energy when T is symmetric */
int qf_hamiltonian_energy(qf_ctx *ctx, double *H);

/* ---- the forcing of the flow.  None by default.  Installed: the affine forcing
 *          F(P, W) = F0 + a_W W + a_P P + a_lap Delta W      (a_* real, F0 a fixed N x N complex128 pattern)
 * -- a fixed pattern, Rayleigh friction, a large-scale drag on the stream function and viscosity -- evaluated by one kernel
 * (k_forcing_affine, csrc/hooks.hip) where a stepper's loop reaches `forcing(P, W)` (isospectral.py:512-520, 591-596;
 * erk.py:47-49), instead of the host hook's PCIe round trip.  Where a loop evaluates it at a matrix X (Whalf in the isomp
 * loop, the stage argument in the explicit ones) with the stream matrix Ph as the loop holds it, a stream-matrix scale
 * pscale and an output scale s, the device computes per entry, on real and imaginary parts separately, every product and
 * sum rounded on its own (no fused multiply-add):
 *          p = Ph * pscale
 *          f = F0[e]                     (0 when there is no F0)
 *          f = f + a_W * X[e]            (term skipped entirely when a_W == 0.0)
 *          f = f + a_P * p               (skipped when a_P == 0.0)
 *          f = f + a_lap * (Delta X)[e]  (skipped when a_lap == 0.0; Delta X as qf_laplace forms it)
 *          out = s * f
 * isomp loop: pscale = 1 / (dt / (2 hbar)), s = dt / 2;  explicit loops and qf_forcing: pscale = s = 1 -- the roundings of
 * the host-hook route, so a host callable that repeats the lines above gives the same trajectory bit for bit.
 *   F0_host   N x N complex128, NULL = none; kept in a buffer the context owns.  Meant to be skew-Hermitian (the caller
 *             checks; quflow_amd.AffineForcing does).
 *   F0_key    caller-chosen id (0: always upload again).  A call that repeats the key AND the fingerprint of what the
 *             context still holds does not upload again, so the key must IDENTIFY the pattern: two patterns that differ
 *             anywhere need two keys (quflow_amd.AffineForcing digests every byte, once, when it is constructed).  The
 *             fingerprint reads 4096 strided doubles plus the last one -- from N = 64 on real parts only -- and must not
 *             be relied on to tell patterns apart.
 *   a_*       finite, else QF_ERR_INVALID.
 * FOLLOW an installed forcing: qf_isomp_forced; qf_isomp_hooked with k = 1, not magnetic, and qf_erk_hooked -- both when
 * their hook table has no `forcing` member (with one as well: QF_ERR_UNSUPPORTED); qf_forcing.
 * REFUSE with QF_ERR_UNSUPPORTED while one is installed, rather than drop the force: qf_isomp / _continue / _diag / _multi,
 * qf_c64_isomp / _continue / _multi, qf_isomp_states, qf_states_advance / _diag, qf_erk, qf_erk_states / _hooked,
 * qf_isomp_simple / _quasinewton (plain and hooked), qf_isomp_hooked with k > 1 or magnetic.  compsum with an installed
 * forcing: QF_ERR_UNSUPPORTED, "Compensated sum with forcing is not yet implemented." (isospectral.py:588-589). */
int qf_set_forcing(qf_ctx *ctx, const void *F0_host, unsigned long long F0_key, double a_W, double a_P, double a_lap);
int qf_clear_forcing(qf_ctx *ctx);          /* no forcing again (the buffer is kept) */
/* F = F(P, W) of what is installed, pscale = s = 1; host in, host out.  QF_ERR_STATE when nothing is installed.
 * All three pointers NULL: the kernel alone, queued on the context's stream without a synchronisation, on the resident
 * state and the stream-matrix buffer as the last call left it, the result left on the device (timing between
 * qf_timer_start / qf_timer_stop: tools/forcing_resident.py). */
int qf_forcing(qf_ctx *ctx, const void *P_host, const void *W_host, void *F_host);

/* ---- stochastic band-limited forcing: the affine forcing above with a pattern F0 that is redrawn ON THE DEVICE for every
 * step (csrc/stochastic.hip).  Over the step n -> n + 1 of size dt
 *          F0_n = shr2mat(omega_n),   omega_n[l^2 + l + m] = (sigma_l * (1 / sqrt(dt))) * xi_n(l, m),  l_min <= l <= l_max,
 * zero elsewhere, xi iid N(0,1): white in time, injected in a band of wavenumbers.  The generator is counter based,
 * Philox4x32-10 (multipliers D2511F53, CD9E8D57; Weyl constants 9E3779B9, BB67AE85) with key (seed & 0xffffffff, seed >> 32)
 * and counter (n & 0xffffffff, n >> 32, b, 0), b = q >> 1, q = l^2 + l + m.  From the output words x0..x3:
 *          u = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53  in (0, 1],     v = ((x2 >> 5) 2^26 + (x3 >> 6)) 2^-53  in [0, 1)
 *          r = sqrt(-2 log(u)),  t = 6.283185307179586 * v,  xi = r cos(t) for even q, r sin(t) for odd q
 *          s = sigma_l * inv,  inv = 1.0 / sqrt(dt) formed once on the host,  omega = s * xi       (each product rounded)
 * so a coefficient depends on (seed, n, l, m) alone: not on N, the band, how a run is cut into calls, or its neighbours.
 * Per step: k_stoch_draw, then the pack and the slab matvec of the transforms on a band basis the context keeps -- the
 * blocks m <= l_max, columns j <= l_max - m, 8 qf_slab_prefix(N, l_max + 1, l_max + 1) bytes (4 MB for l_max = 31 at
 * N = 1024), built at install and kept while l_max does not change -- into the forcing's pattern buffer: F0_n has the bits
 * of qf_shr2mat (streamed form) on the same coefficients.  The transforms' own staging buffers are not touched.
 *   l_min, l_max   1 <= l_min <= l_max <= N - 1, else QF_ERR_INVALID
 *   sigma          l_max - l_min + 1 amplitudes, finite and >= 0, else QF_ERR_INVALID
 *   seed, step     the stream's key and the counter n of the next step a run takes
 *   a_*            as qf_set_forcing
 *   band_bytes_max the band basis may take at most this many bytes: more is QF_ERR_INVALID before anything is allocated
 * The run's counter: a call that runs `steps` steps with the forcing installed uses the counters step .. step + steps - 1
 * and leaves step + steps (qf_stochastic_tell); qf_stochastic_seek sets it.  qf_clear_forcing clears a stochastic forcing,
 * qf_set_forcing replaces it.  FOLLOW: qf_isomp_forced, qf_isomp_hooked (k = 1, not magnetic, no `forcing` hook; dt > 0).
 * REFUSE with QF_ERR_UNSUPPORTED: every entry point that refuses an affine forcing, and qf_erk_hooked (noise inside
 * Runge-Kutta stages is out of scope) and qf_forcing (a bare evaluation has no step). */
int qf_set_stochastic_forcing(qf_ctx *ctx, int l_min, int l_max, const double *sigma, unsigned long long seed,
                              unsigned long long step, double a_W, double a_P, double a_lap, long long band_bytes_max);
int qf_stochastic_tell(qf_ctx *ctx, unsigned long long *step);
int qf_stochastic_seek(qf_ctx *ctx, unsigned long long step);
/* The pattern of counter `step` for step size dt (> 0), without touching the run's counter: omega_host receives the
 * (l_max + 1)^2 coefficients, F0_host the N x N complex128 pattern; either may be NULL (both: the three launches alone,
 * queued on the context's stream without a synchronisation -- timing between qf_timer_start / qf_timer_stop).
 * QF_ERR_STATE when no stochastic forcing is installed. */
int qf_stochastic_pattern(qf_ctx *ctx, unsigned long long step, double dt, double *omega_host, void *F0_host);

/* ---- stepper protocol: isomp_fixedpoint (quflow/integrators/isospectral.py:338-613),
 *      called by simulation.solve (quflow/simulation.py:788) ---------------------- */
int qf_upload_W(qf_ctx *ctx, const void *W_host);     /* host -> ctx state W */
int qf_download_W(qf_ctx *ctx, void *W_host);         /* ctx state W -> host */

typedef struct qf_isomp_stats {
    long long total_iterations;   /* isospectral.py:426,478 */
    long long number_of_maxit;    /* steps that exhausted maxit, isospectral.py:427,540 */
    double tol_used;              /* tol actually applied (tol_auto when tol < 0), :440-452 */
    double last_resnorm;          /* residual of the last iteration performed, :534 */
} qf_isomp_stats;

/* Advances the ctx state W by `steps` isospectral-midpoint steps of length dt with the
 * built-in Hamiltonian P = Delta^-1 W (hamiltonian=solve_poisson, isospectral.py:341).
 *   tol   < 0  -> 'auto' (isospectral.py:440-452);  minit >= 1, maxit >= minit (:400-401)
 *   compsum    -> Kahan-compensated W update (:553-586), tolerance eps instead of sqrt(eps)
 *   reinitialize -> zero the iteration vector dW at every step (:471-472)
 * dW is zeroed at entry of every call (:430), so chunked calls behave like the reference.
 * Everything stays on the device, the data-dependent exit of isospectral.py:535 included: the last
 * workgroup of an iteration's second product (or k_norm_decide in the two-kernel protocol) takes the
 * decision, launches are tagged (step, iteration) and return at once when they are not due, and the
 * host only polls an 8-byte progress word in pinned memory while it enqueues ahead. */
int qf_isomp(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit,
             int compsum, int reinitialize, qf_isomp_stats *stats_out);
/* As qf_isomp, but the iteration vector dW (and the Kahan term) of the previous qf_isomp /
 * qf_isomp_continue call on this context carries over instead of being zeroed: one call of the
 * reference spans many steps and zeroes dW once (isospectral.py:430), so a host that must act
 * between the steps -- strang_splitting (isospectral.py:466-467, 598-599) or callback (:549-550) --
 * issues the first step with qf_isomp and every further one with qf_isomp_continue (the state may
 * be re-uploaded in between: Whalf restarts as W + dW, isospectral.py:481-482).
 * What ends a carried increment (the next qf_isomp_continue then starts from dW = 0, as qf_isomp does): every other call
 * that replaces the state or uses dW[] as scratch -- qf_erk / qf_erk_hooked, qf_isomp_simple / _quasinewton (plain and hooked),
 * qf_isomp_hooked / qf_isomp_forced, qf_rotate(NULL), qf_shr2mat(NULL) / qf_shc2mat(NULL), qf_states_select --, a call that
 * ended in an error, and for the complex64 state qf_c64_upload_W and qf_c64_solve_tridiagonal.  What keeps it: qf_upload_W
 * and the resident form of qf_solve_tridiagonal (the two ways a Strang half step reaches the state) and every host-in /
 * host-out or read-only entry point (tests/test_hip_context_carry.py runs each of them between the two calls). */
int qf_isomp_continue(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit,
                      int compsum, int reinitialize, qf_isomp_stats *stats_out);

/* Ensembles on one GPU: k independent trajectories, one context each (all on the same device), advanced
 * by `steps` steps in one call.  Every context runs exactly the launches qf_isomp would issue for it --
 * own Hamiltonian, own exit decisions, own statistics (stats_out[k]), results bit-identical to k separate
 * qf_isomp calls -- but their streams are fed by one host loop, so the GPU overlaps the replicas (dependent-
 * launch gaps of one are filled by another; for N < 768 two replicas' workgroups share the CUs).
 * Default stepper options only (no compsum / reinitialize); dW restarts from zero as in qf_isomp.
 * How many at once: FOUR, created back to back.  The runtime gives every stream the next hardware queue when it is first
 * used and a queue's number mod 4 is the pipe that dispatches it; two replicas on one pipe lose 40 % of their combined rate
 * (N = 512: sum 18,100 timesteps/s for k = 4, 13,000 for k = 5, 16,100 for k = 8).  The call takes any k; the
 * Python mirror passes larger ensembles four contexts at a time.
 * A member that fails (QF_ERR_NONFINITE: its residual turned inf / NaN) does not stop the others: every member runs to its
 * end, and the call returns the first member's error.  The failed member holds what its own qf_isomp call would leave (the
 * state after its last completed step) and reports total_iterations = number_of_maxit = -1, last_resnorm = NaN in its
 * stats_out entry; every other member holds its state after all `steps` steps and its own statistics.  Afterwards every
 * context is marked as after a failed call (its increment is not carried, its skew check is redone at the next entry). */
int qf_isomp_multi(qf_ctx **ctxs, int k, double dt, int steps, double tol, int minit, int maxit,
                   qf_isomp_stats *stats_out);
/* The same for contexts that hold complex64 states (qf_c64_upload_W): each runs the float32 launches qf_c64_isomp would
 * issue for it; results bit-identical to k separate qf_c64_isomp calls. */
int qf_c64_isomp_multi(qf_ctx **ctxs, int k, double dt, int steps, double tol, int minit, int maxit, qf_isomp_stats *stats_out);

/* ---- explicit (non-isospectral) steppers on the ctx state W with the built-in Hamiltonian:
 *      euler / heun / rk4, quflow/integrators/erk.py:19-59, 62-112, 115-160 (forcing = None);
 *      rhs = bracket(P, W) = (P@W - W@P)/hbar, quflow/geometry.py:41-49.
 *      skewh: the Laplacian backend's select_skewherm flag (cpu.py:563-591) for P = Delta^-1 W;
 *      with skewh != 0 and an exactly skew-Hermitian state W@P = (P@W)^H is used. ------- */
#define QF_ERK_EULER 0
#define QF_ERK_HEUN 1
#define QF_ERK_RK4 2
int qf_erk(qf_ctx *ctx, int method, double dt, int steps, int skewh);
/* the same on a stack of k states (erk.py with W.shape = (k,N,N)): P from state 0 (cpu.py:696-697), bracket(P, W)
 * broadcast over the stack (geometry.py:41-49).  states_host: (k,N,N) complex128, overwritten with the result. */
int qf_erk_states(qf_ctx *ctx, void *states_host, int k, int method, double dt, int steps, int skewh);

/* ---- isomp_simple (isospectral.py:254-335) and isomp_quasinewton (isospectral.py:155-251) on the
 *      ctx state W, hamiltonian = solve_poisson, skew-Hermitian case.  The reference's two
 *      lu_solve calls per pass (A = I - (stepsize/2) Ptilde) are replaced by a Newton-Schulz
 *      inverse on the matrix cores (cond(A) = sqrt(1 + |E|_2^2) for skew-Hermitian E = (stepsize/2) Ptilde).
 *      qf_isomp_quasinewton: tol < 0 -> 'auto' (eps*stepsize*|W|_inf, :190-191);
 *      stats: total_iterations, number_of_maxit (steps whose loop ran out), tol_used.
 *      Envelope of the inverse: states agree with the reference's LU to 1e-12 up to |E|_inf = 100 and to 8 times the
 *      spread of two CPU evaluations at 1000 (tests/test_hip_lu_steppers.py).  Beyond: cond(A)^2 = (1 + s_max^2) /
 *      (1 + s_min^2) of E's singular values, so for a stream function without a null vector the scale of E does not
 *      matter up to the refusal; with one, cond(A) = |E|_2 and from |E|_2 ~ 1e8 on the residual's rounding noise stays
 *      above the iteration's exit level: QF_ERR_STATE ("Newton-Schulz did not converge"; the reference's LU has lost
 *      the state there too, eps cond(A)^2).  |E|_inf > 1e150 is refused at once, QF_ERR_STATE ("too large for the
 *      Newton-Schulz inverse").  An error, never a wrong state. ------ */
int qf_isomp_simple(qf_ctx *ctx, double dt, int steps);
int qf_isomp_quasinewton(qf_ctx *ctx, double dt, int steps, double tol, int maxit, qf_isomp_stats *stats_out);
/* ... with a foreign `hamiltonian(Wtilde)` (isospectral.py:207, 286): the `hamiltonian` / `user` members of a
 * qf_isomp_hooks table (declared below).  Wtilde goes down and Ptilde comes up once per pass; the inverse, the
 * two solves and the update stay on the device.  (`forcing` is accepted and ignored by the reference's
 * isomp_simple / isomp_quasinewton -- an `assert` on an exception object, :185-186, 283-284 -- so there is no
 * forcing member to honour here.) */
struct qf_isomp_hooks;
int qf_isomp_simple_hooked(qf_ctx *ctx, double dt, int steps, const struct qf_isomp_hooks *hooks);
int qf_isomp_quasinewton_hooked(qf_ctx *ctx, double dt, int steps, double tol, int maxit, qf_isomp_stats *stats_out,
                                const struct qf_isomp_hooks *hooks);

/* ---- isomp on a stack of k states (isospectral.py:463-611 with W.shape = (k,N,N): P from state 0,
 *      the same products for every state, exit test on state 0) and, with magnetic != 0 and
 *      k == 2, magmp (quflow/integrators/mhd.py:235-456, hamiltonian = solve_mhd: P = Delta^-1 W,
 *      B = Delta Theta).  states_host: (k,N,N) complex128, overwritten with the result.
 *      tol < 0 -> 'auto' (sqrt(eps)*dt/hbar*|state 0|_inf). ------------------------------- */
int qf_isomp_states(qf_ctx *ctx, void *states_host, int k, double dt, int steps, double tol, int minit, int maxit,
                    int reinitialize, int magnetic, qf_isomp_stats *stats_out);

/* ---- the same stack RESIDENT on the device across calls: what qf_upload_W / qf_isomp / qf_download_W are to one state.
 *      qf_states_upload makes the (k,N,N) complex128 stack resident (buffers of the context's own, kept until the context
 *      is destroyed); qf_states_advance is one qf_isomp_states call on it without the transfers -- the same loop, the same
 *      bits: dX restarts from zero per call, the exit test is state 0's, the finite check covers every state; magnetic != 0
 *      (k == 2) is magmp.  qf_states_download copies the stack out (k must be the resident k).
 *      Errors: QF_ERR_STATE when no stack is resident -- before the first upload, and after a host-in / host-out
 *      qf_isomp_states call on the same context, which uses the stack's buffers as its scratch (the hooked steppers keep
 *      buffers of their own and leave a resident stack alone); QF_ERR_INVALID for magnetic with k != 2, a member index out
 *      of range, a k mismatch on download; QF_ERR_NONFINITE as qf_isomp_states (the stack then holds the states after the
 *      last completed step; qf_states_upload starts afresh). ---- */
int qf_states_upload(qf_ctx *ctx, const void *states_host, int k);
int qf_states_download(qf_ctx *ctx, void *states_host, int k);
int qf_states_advance(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int reinitialize, int magnetic,
                      qf_isomp_stats *stats_out);
/* Member access: qf_states_select copies member j into the context's state W (device copy, no transfer), after which every
 * entry point that takes a NULL host pointer for "the resident state" works on it -- qf_mat2shr, qf_shr2fun, qf_eigh_state,
 * qf_rotate, qf_grad, qf_diagnostics; qf_states_store copies W back into member j. */
int qf_states_select(qf_ctx *ctx, int j);
int qf_states_store(qf_ctx *ctx, int j);
/* out[2 j] = <X_j, X_0>, out[2 j + 1] = <X_j, X_j>/2 for the k members of the resident stack (2 k doubles): what a run
 * of passive tracers logs next to qf_diagnostics of member 0. */
int qf_states_inner(qf_ctx *ctx, double *out);
/* Diagnostics of the resident MHD pair (W, Theta), k == 2, with <.,.> = inner_L2 (quflow/geometry.py:72-76):
 *   out[0] Ek = -<W, Delta^-1 W>/2   out[1] Em = -<Theta, Delta Theta>/2   out[2] X = <W, Theta>   (cross-helicity)
 *   out[3] A  = <Theta, Theta>/2     out[4] S  = <W, W>/2;                  the conserved Hamiltonian is Ek + Em.
 * One Poisson solve, then one pass over W, P and Theta that applies the Laplacian's stencil on the fly and reduces in a
 * fixed order (no float atomics: bit-reproducible).  Ek and S are qf_diagnostics' values for W and A its enstrophy for
 * Theta, bit for bit. */
int qf_mhd_diagnostics(qf_ctx *ctx, double out[5]);
/* qf_states_advance (magnetic != 0) followed by qf_mhd_diagnostics of the new state, queued behind the last step under the
 * call's closing synchronisation.  Same results as the two calls.  mhd_out == NULL: qf_states_advance. */
int qf_states_advance_diag(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int reinitialize, int magnetic,
                           qf_isomp_stats *stats_out, double *mhd_out);
/* The per-degree budget of the resident MHD pair (W, Theta), k == 2, of the built-in system (mhd.py:10-18, 361-393):
 *     P = Delta^-1 W,  B = Delta Theta,   W' = ([P, W] + [B, Theta]) / hbar,   Theta' = [P, Theta] / hbar.
 * Band limit 1 < Nmax <= N; the transforms' mode set as for qf_mat2shr (qf_basis_compute / _upload, or qf_basis_stream).
 * Each bracket is formed as qf_spectral_budget forms its tendency, (X Y - (X Y)^H) (1/hbar) with one plain product, and
 *     omega, theta, a, b, c = mat2shr of W, Theta, [P,W]/hbar, [B,Theta]/hbar, [P,Theta]/hbar band-limited to Nmax
 * come from ONE sweep of the basis that carries all five; each has the bits qf_mat2shr gives for that matrix alone.
 * out[r][l], l < Nmax, is scale_r sum_{m=-l..l} u_lm v_lm, summed in the order qf_spectral_budget fixes:
 *     r      0            1            2            3          4          5          6        7        8
 *     u v    omega omega  theta theta  omega theta  omega a    omega b    theta c    theta a  theta b  omega c
 *     scale  1            1            1            2          2          2          1        1        1
 * With ll = l (l + 1): out[0]/ll and ll out[1] are the kinetic and magnetic energy spectra (their sums over l, halved, are
 * qf_mhd_diagnostics' Ek and Em), out[1] the mean-square potential, out[2] the cross helicity; out[3]/ll, out[4]/ll and
 * ll out[5] the kinetic transfer by advection, by the Lorentz term, and the magnetic transfer; out[6] + out[7] + out[8]
 * the transfer of cross helicity.  coeffs: NULL, or [5][Nmax^2] for omega, theta, a, b, c.
 * P, B and the three tendency matrices stay readable (qf_download_buffer, QF_BUF_MHD_*) until the next such call.
 * The call reads the two members of the stack and writes buffers of its own (allocated on the first call, about
 * 10 N^2 complex128, freed with the context), the staging matrices Whalf and PW, and in streamed mode the slab: the
 * stack, its increments, the state W of the context, the device copy of the coefficients (what qf_mat2shr left for
 * qf_shr2mat / qf_shr2fun) and the transforms' staging are left as they were, and a resident run continues bit for bit as
 * if the call had not happened.
 * QF_ERR_STATE without a resident stack, and without a basis in resident mode; QF_ERR_INVALID for k != 2, a null `out`,
 * Nmax outside 2..N or a slab budget too small for block 0; QF_ERR_UNSUPPORTED while a forcing or a Hamiltonian is
 * installed on the context (the system above is the built-in one) -- each before anything is launched. */
int qf_mhd_spectral_budget(qf_ctx *ctx, int Nmax, double *out, double *coeffs);

/* ---- the stepper with HOST HOOKS: isomp_fixedpoint's `forcing`, foreign `hamiltonian`, `strang_splitting`,
 *      `callback` (isospectral.py:338-353, 403-423, 466-467, 488-492, 512-520, 547-551, 598-603), the
 *      general branch of select_skewherm(False) (:504-505), and all of them -- with compsum -- on
 *      (k,N,N) stacks (P from the Hamiltonian, exit test on state 0, :527-532).  The state, dW, Whalf,
 *      the products and the Kahan term stay on the device; a hook receives / fills pinned host matrices
 *      owned by the library (valid during the call only), (k,N,N) or (N,N) complex128 as noted, and
 *      returns 0 (anything else aborts the call with QF_ERR_CALLBACK).  NULL pointers = hook absent;
 *      hamiltonian == NULL: the built-in P = Delta^-1 W[0] on the device. ------------------------------ */
typedef struct qf_isomp_hooks {
    void *user;
    /* P (N,N) = hamiltonian(Whalf (k,N,N)[, time = t + dt/2 when hamiltonian_takes_time]) */
    int (*hamiltonian)(void *user, const void *Whalf, void *P, double time);
    /* F (k,N,N) = forcing(P (N,N), Whalf (k,N,N)[, time = t + dt/2 when forcing_takes_time]) */
    int (*forcing)(void *user, const void *P, const void *Whalf, void *F, double time);
    /* W (k,N,N) <- strang_splitting(h, W), in place, h = dt/2, before and after every step */
    int (*strang)(void *user, double h, void *W);
    /* callback(W, dW2): the state before the step's update and 2 (PW - PW^H) (k,N,N each) */
    int (*callback)(void *user, const void *W, const void *dW2);
    int hamiltonian_takes_time, forcing_takes_time;   /* the autonomy probing (:403-423) is the caller's */
    int has_time;                                     /* `time` is not None: advanced by dt per step */
    double time;
    int skewh;                                        /* integrators' select_skewherm flag (isospectral.py:96-118):
                                                         commutator as PW - PW^H or as PW - Whalf@Phalf */
    int solve_skewh;                                  /* the Laplacian backend's flag (cpu.py:563-591) for the built-in P */
    /* instead of `strang`: W <- T^-1 W with this (N,N,2) table, on the device (solve_viscdamp half step) */
    const double *strang_table;
    unsigned long long strang_key;
    /* magmp_fixedpoint (quflow/integrators/mhd.py:235-456) on a (2,N,N) state (W, Theta), k == 2: the vorticity
     * state gets the magnetic terms [B, Theta] on top.  `hamiltonian` then fills P with TWO (N,N) matrices,
     * (P, B) -- the pair solve_mhd returns (mhd.py:10-18); NULL: the built-in P = Delta^-1 W, B = Delta Theta.
     * `forcing` receives P (the first of the two) and the (2,N,N) state; `callback` as above. */
    int magnetic;
    /* stacks (qf_isomp_hooked with k > 1, qf_erk_states_hooked): 1 = `hamiltonian` fills ONE stream matrix per state of
     * the stack (k matrices: a Hamiltonian that returns a (k,N,N) array, bracket(P, W) is then a batched product), 0 = one
     * for all states; -1 = not known yet: the hook stores 0 or 1 here during its first call and the library reads the
     * field back behind that call (the reference never asks in advance, isospectral.py:488-491). */
    int states_p;
} qf_isomp_hooks;
/* states_host: (k,N,N) complex128, overwritten with the result.  compsum with forcing: QF_ERR_UNSUPPORTED (:588-589) */
int qf_isomp_hooked(qf_ctx *ctx, void *states_host, int k, double dt, int steps, double tol, int minit, int maxit,
                    int compsum, int reinitialize, const qf_isomp_hooks *hooks, qf_isomp_stats *stats_out);
/* The loop of qf_isomp_hooked on the context's RESIDENT state (qf_upload_W / qf_download_W), with the forcing installed by
 * qf_set_forcing (none installed: no force term) and the Hamiltonian installed by qf_set_hamiltonian: k = 1, skew-Hermitian
 * branch, no host hook, no N^2 transfer in either direction.  strang_table != NULL: the half step W <- T^-1 W with that
 * (N,N,2) table before and after every step, on the device (as the hook table's strang_table / strang_key members).
 * The same bits as qf_isomp_hooked gives for the same state, forcing and half step; dW restarts from zero per call; one
 * scalar is read back per iteration for the exit test.  Arguments otherwise as qf_isomp. */
int qf_isomp_forced(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int reinitialize,
                    const double *strang_table, unsigned long long strang_key, qf_isomp_stats *stats_out);
/* euler / heun / rk4 (erk.py:19-160) with `forcing(P, W)` and / or a foreign `hamiltonian(W)` (the `hamiltonian`,
 * `forcing`, `user` and `skewh` members of the hook table; k = 1).  W_host: (N,N), overwritten. */
int qf_erk_hooked(qf_ctx *ctx, void *W_host, int method, double dt, int steps, const qf_isomp_hooks *hooks);
/* The same on a (k,N,N) stack (quflow/integrators/erk.py with batched input): `hamiltonian(stack)` fills ONE (N,N) stream
 * matrix, `forcing(P, stack)` a stack; the built-in Hamiltonian solves for state 0 (cpu.py:696-697). */
int qf_erk_states_hooked(qf_ctx *ctx, void *states_host, int k, int method, double dt, int steps, const qf_isomp_hooks *hooks);

/* ---- spherical-harmonics <-> matrix transforms (quflow/quantization.py).  The quantization
 *      basis (compute_basis, quantization.py:68-113: N(N+1)(2N+1)/6 doubles, block m row-major at
 *      basis_break_index(m, N)) is uploaded once and stays resident in HBM; a transform is one
 *      HBM-bound sweep over it (or, after qf_basis_stream, rebuilds the blocks it needs slab by slab).  A NULL matrix pointer means "the ctx state W" (initial data /
 *      'shr' output of a resident trajectory without moving W over PCIe). ------------------ */
int qf_basis_upload(qf_ctx *ctx, const double *basis_host, long long count);
/* compute_basis(N) (quantization.py:68-113) on the device, straight into the resident copy: the
 * eigenvectors of the tridiagonal blocks of the direct Laplacian (laplacian/direct.py:19-62) by
 * one twisted factorisation per vector at the known eigenvalues -el(el+1) (the reference calls
 * LAPACK's tridiagonal eigensolver), scaled and oriented as quantization.py:45-65,99-106. */
int qf_basis_compute(qf_ctx *ctx);
int qf_basis_download(qf_ctx *ctx, double *basis_host, long long count);
/* The streamed form, a per-context mode.  slab_bytes > 0: from now on qf_shr2mat, qf_mat2shr, qf_shc2mat and qf_mat2shc
 * (their NULL forms included) do not read a resident basis.  Each call rebuilds the blocks it needs -- of every block
 * m < Nmax only the columns j < Nmax - m, by the same per-column arithmetic as qf_basis_compute, so the same bits -- into a
 * slab of at most slab_bytes on the device and applies them there, whole blocks in m order, slab after slab: memory
 * stays near N^2 instead of N^3/3, and the results equal the resident path's bit for bit.  They stream whether or not
 * the context also holds a resident basis.  A call whose block m = 0 (N x Nmax doubles) does not fit slab_bytes fails
 * with QF_ERR_INVALID before it touches anything.  The slab is grown on demand and freed with the context.
 * slab_bytes == 0: back to the resident basis (the default; the transforms then need qf_basis_upload or
 * qf_basis_compute).  Negative: QF_ERR_INVALID.  qf_basis_download always needs the resident basis. */
int qf_basis_stream(qf_ctx *ctx, long long slab_bytes);
/* The streamed form's plan, host only: how many slabs a transform with band limit Nmax (1..N) takes under slab_bytes,
 * and the first block of each of them in first_block[0 .. min(count, capacity) - 1] (first_block may be NULL).  Slabs
 * hold whole blocks in m order, as many as fit.  Returns the count, or -QF_ERR_INVALID when block 0 does not fit. */
int qf_basis_slab_plan(int N, int Nmax, long long slab_bytes, int *first_block, int capacity);
/* shr2mat_(omega, basis, W_out), quantization.py:188-245 (W_out zeroed first as in shr2mat, :474);
 * n_omega < N^2 band-limits to el < int(sqrt(n_omega)) (:204-208) */
int qf_shr2mat(qf_ctx *ctx, const double *omega_host, long long n_omega, void *W_host);
/* (omega_host == NULL in either direction: the coefficients stay on / come from the device copy
 *  the previous transform left, so that a filter "mat2shr -> scale -> shr2mat" or a timing loop
 *  never crosses PCIe) */
/* mat2shr_(W, basis, omega_out), quantization.py:286-327, omega_out zeroed first (:516) */
int qf_mat2shr(qf_ctx *ctx, const void *W_host, double *omega_host, long long n_omega);
/* shc2mat_ / mat2shc_, quantization.py:331-396: omega is N^2 complex128 */
int qf_shc2mat(qf_ctx *ctx, const void *omega_host, void *W_host);
int qf_mat2shc(qf_ctx *ctx, const void *W_host, void *omega_host);
/* The per-degree budget of a state W (NULL: the resident state ctx->W), double precision, skew-Hermitian W, band limit
 * 1 < Nmax <= N; needs the transforms' mode set as qf_mat2shr does (qf_basis_compute / _upload, or qf_basis_stream).  With
 *     P = the context's Hamiltonian of W (the built-in solve, or what qf_set_hamiltonian installed),
 *     A = (P W - (P W)^H) (1/hbar)             the advective tendency [P, W]/hbar; P and A are left in the Phalf and PW
 *                                              buffers (qf_download_buffer),
 *     F = the installed forcing at (P, W)      formed as qf_forcing forms it; of a stochastic forcing only the affine terms
 *                                              a_W, a_P, a_lap enter -- the noise pattern does not, its counter is not touched,
 *     omega, a, f = mat2shr of W, A, F band-limited to Nmax -- ONE sweep of the basis carries all three, and each has the
 *                                              bits qf_mat2shr gives for that matrix alone,
 * out[0][l] = Z_l = sum_m omega_lm^2,  out[1][l] = T_l = 2 sum_m omega_lm a_lm,  out[2][l] = I_l = 2 sum_m omega_lm f_lm
 * (zeros without a forcing) for l < Nmax, m = -l..l.  Each sum is formed by one wavefront in a fixed order: lane t adds the
 * products at l^2 + t, l^2 + t + 64, ... in ascending order, then the xor butterfly 32, 16, .., 1 joins the 64 lanes; the
 * results are reproducible from run to run.  sum_l Z_l / 2 is the enstrophy, sum_l Z_l / (l (l+1)) / 2 the energy.
 * coeffs: NULL, or [3][Nmax^2] for omega, a, f (f zeros without a forcing).
 * Only per-iteration scratch of the context is written (the staging matrices and the transforms' staging; the device
 * copy of the coefficients then holds omega): the state, the increment, what is installed and the stochastic counter stay,
 * and a resident run continues bit for bit as if the call had not happened.  QF_ERR_INVALID (before anything is launched)
 * for a bad argument or a slab budget too small for block 0; QF_ERR_STATE without a basis in resident mode, and for
 * W_host == NULL on a context that holds a complex64 state only. */
int qf_spectral_budget(qf_ctx *ctx, const void *W_host, int Nmax, double *out, double *coeffs);
/* Z_l alone, l < Nmax: the same route with the state as its only column -- no solve, no product, Nmax doubles come back. */
int qf_degree_spectrum(qf_ctx *ctx, const void *W_host, int Nmax, double *Z);
/* shc2fun / shr2fun (quflow/transforms.py:220-268, 422-438) at bandwidth L (1..8192, independent of ctx->N):
 * MW grid (L, 2L-1), row-major.  omega_host == NULL: the coefficients the last qf_mat2shr left on ctx
 * (as qf_shr2mat's NULL).  omega is trimmed or zero-padded to L^2 entries (qf_shr2fun: after dropping a last degree
 * cut short, which shr2shc leaves zero); berezin != 0 multiplies
 * coefficient (l, m) by berezin_multipliers(L)[l].  Neither call needs the quantization basis. */
int qf_shr2fun(qf_ctx *ctx, const double *omega_host, long long n_omega, int L, int berezin, double *f_host);
/* omega: n_omega complex128; isreal: f_host is double (L, 2L-1) (the m >= 0 half of omega, a real map), else complex128 */
int qf_shc2fun(qf_ctx *ctx, const void *omega_host, long long n_omega, int L, int berezin, int isreal, void *f_host);
/* Function-space output of a state (the reference's 'fun', 'funL2', 'funhalf', 'funL2half' rows, quflow/simulation.py:
 * 287-344): nfields real grids of W (NULL: the resident state ctx->W -- for a resident stack the member qf_states_select
 * chose; else an N x N complex128 matrix, uploaded to the staging matrix as qf_mat2shr does).  Field i is
 *     qf_shr2fun(mat2shr(W)[:n_omega], L, berezin)   with L = sqrt(n_omega) (n_omega no square: the next integer above;
 *                                                    the last degree, cut short, stays zero as in qf_shr2fun),
 * bit for bit, written to f_host[i] as (L, 2L-1), row-major, doubles (dtype 0) or floats (dtype 1: each double converted
 * with round-to-nearest-even on the device, what numpy's astype does).  The state goes through mat2shr ONCE, band-limited to
 * the largest L asked for (with a streamed basis: once per bandwidth); the fields of one bandwidth share ONE synthesis --
 * one walk of the Legendre recurrence and one gather of the twiddles for all of them.
 * Needs the transforms' mode set as qf_mat2shr does.  Only the transforms' staging, ctx->sht and the device copy of the
 * coefficients (which then holds mat2shr of the state, band-limited to the largest L) are written: the state, the carried
 * increment, the statistics and what is installed stay, and a resident run continues bit for bit as if the call had not
 * happened.  QF_ERR_INVALID, before anything is launched and with the field named: nfields outside 1..8 or more than 4
 * fields of one bandwidth, a null pointer, a dtype other than 0 / 1, n_omega < 1, L > ctx->N or L > 8192; QF_ERR_STATE for W_host == NULL
 * on a context that holds a complex64 state only, and without a basis in resident mode. */
typedef struct { long long n_omega; int berezin; int dtype; } qf_field;   /* dtype: 0 = float64, 1 = float32 */
int qf_state_fields(qf_ctx *ctx, const void *W_host, int nfields, const qf_field *fields, void *const *f_host);
/* The first n_omega real coefficients of the device copy (what the last qf_mat2shr, qf_state_fields, qf_shr2mat or
 * qf_fun2shr(NULL) left there), copied out without another sweep: after qf_state_fields with a field of bandwidth N they are
 * qf_mat2shr of the same state, bit for bit.  QF_ERR_STATE when the copy holds fewer than n_omega real coefficients. */
int qf_shr_held(qf_ctx *ctx, double *omega_host, long long n_omega);
/* fun2shc / fun2shr (quflow/transforms.py:189-217, 404-419): McEwen-Wiaux analysis of the MW grid f (L, 2L-1), row-major,
 * double when isreal != 0, else complex128; 1 <= L <= 8192, independent of ctx->N, no quantization basis needed.
 * qf_fun2shc writes L^2 complex128 (index l^2 + l + m), qf_fun2shr the L^2 doubles shc2shr makes of them.  The inverse of
 * qf_shc2fun / qf_shr2fun with berezin == 0 on band-limited grids.  Two real L x L operators that depend on L only are
 * built on the first call at a bandwidth and kept on ctx until another bandwidth is asked for.
 * qf_fun2shr with omega_host == NULL leaves the coefficients in the device copy that qf_shr2mat(ctx, NULL, L*L, ...) and
 * qf_shr2fun(ctx, NULL, ...) read; that form needs L <= ctx->N. */
int qf_fun2shc(qf_ctx *ctx, const void *f_host, int L, int isreal, void *omega_host);
int qf_fun2shr(qf_ctx *ctx, const void *f_host, int L, int isreal, double *omega_host);

/* ---- diagnostics on the ctx state W: quflow/physics.py:26-38 with
 *      inner_L2 (quflow/geometry.py:72-76) -------------------------------------- */
int qf_diagnostics(qf_ctx *ctx, double *energy_euler, double *enstrophy);
/* qf_isomp followed by qf_diagnostics with ONE synchronisation: the diagnostics' launches are queued behind
 * the last step (an output chunk of simulation.solve / of an ensemble rank: advance, then log energy and
 * enstrophy, quflow/simulation.py:788-803).  Same results as the two calls. */
int qf_isomp_diag(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int compsum,
                  int reinitialize, qf_isomp_stats *stats, double *energy_euler, double *enstrophy);
/* matrix infinity norm of the state, np.linalg.norm(W, inf) (isospectral.py:448) */
int qf_norm_inf_W(qf_ctx *ctx, double *out);

/* ---- Casimirs: out[k-1] = C_k(W) = Re tr((iW)^k) / N for k = 1..kmax, 1 <= kmax <= 8 -- what the isospectral steppers
 *      conserve (csrc/casimir.hip).  Defined for ANY complex W: nothing assumes a skew-Hermitian matrix, a
 *      host matrix with rounding in its symmetry gets the trace of its actual powers, as np.trace of numpy's products.
 *      C_2 = <W, W> = 2 enstrophy.  complex128 arithmetic.
 *      The powers A_j = W^j for j <= p = ceil(kmax / 2) are stored: A_2 = W W, A_3 = A_2 W, A_4 = A_2 A_2, at most three plain
 *      products of the stepper's own product kernel, into the per-iteration staging matrices Whalf, Phalf, PW (a host-in W and
 *      a widened complex64 state go to `stage`; all free between stepper calls).  Then tr(W^(i+j)) = sum_ab (A_i)_ab (A_j)_ba
 *      with i = floor(k / 2), j = k - i (k = 1: the diagonal of W; k = 2 needs no product), all pair sums from ONE pass of one
 *      kernel (k_power_traces) over the stored powers: a workgroup reads the tiles (I,J) and (J,I) of every power once, every
 *      thread and every level of the reduction tree carries a two-sum compensation term, block partials are added by a second
 *      one-block launch in fixed order -- no float atomics, two calls return the same bits.  The phase i^k and the real part
 *      are applied to the raw sum on the host, followed by a true division by N.
 *      On matrices whose entries have integer real and imaginary parts the result is exact whenever 4 tr(|W|^k) < 2^53.
 *      Every form leaves the run untouched -- the state W, the carried increment (qf_isomp_continue), the stack and its
 *      increments, the device copy of the coefficients, the stochastic counter -- and a resident run continues bit for bit as
 *      if the call had not happened.
 *      QF_ERR_INVALID for kmax outside 1..8, a null output or a member index out of range, QF_ERR_STATE without the resident
 *      state or stack the form reads -- each before anything is launched; QF_ERR_NONFINITE when a returned sum is inf or NaN
 *      (an inf or NaN entry of the matrix). ---- */
/* W_host: N x N complex128, or NULL for the context's resident complex128 state.  out: kmax doubles. */
int qf_casimirs(qf_ctx *ctx, const void *W_host, int kmax, double *out);
/* The resident complex64 state (qf_c64_upload_W), widened on the device to complex128 -- exact -- into `stage`, then the
 * double path above: the instrument stays below the float32 stepper's own drift. */
int qf_c64_casimirs(qf_ctx *ctx, int kmax, double *out);
/* Member j of the resident stack (qf_states_upload), read in place. */
int qf_states_casimirs(qf_ctx *ctx, int j, int kmax, double *out);
/* The resident MHD pair (W, Theta), k == 2 (else QF_ERR_INVALID), what magmp conserves:
 *   magnetic[k-1] = C_k(Theta), k = 1..kmax;
 *   cross[k-1]    = Re tr((iW)(iTheta)^k) / N, k = 1..p = ceil(kmax / 2) -- the members of the cross-helicity family that the
 *                   stored powers of Theta give without a further product; W is read in place.
 * magnetic[1] = 2 magnetic_casimir and cross[0] = cross_helicity of qf_mhd_diagnostics. */
int qf_mhd_casimirs(qf_ctx *ctx, int kmax, double *magnetic, double *cross);
/* HIP-event times of this context's most recent completed call of the four above, in milliseconds: the products that
 * stored the powers (0 for kmax <= 2), and the traces kernel with its fold.  QF_ERR_STATE before the first one. */
int qf_casimirs_times(qf_ctx *ctx, double *products_ms, double *traces_ms);

/* ---- Hermitian eigendecomposition H = V diag(lambda) V^H on the device (csrc/eigh.hip): parallel one-sided Jacobi on
 *      H + 2 |H|_inf I, eigenvalues refined by their Rayleigh quotients with H.  complex128 only.  lambda: N doubles,
 *      ascending; V: (N,N) complex128, unitary, column j belongs to lambda[j].  Deterministic: two calls return the same
 *      bits, and lambda has the same bits with and without V.  An inf or NaN entry: QF_ERR_NONFINITE; the sweep cap (60)
 *      reached: QF_ERR_NOCONVERGE.  The work matrices (3 N^2 complex128) are allocated on the context's first such call
 *      and freed with it.  (The reference calls LAPACK through numpy: np.linalg.eig in quflow/analysis.py:28.) -------- */
typedef struct qf_eigh_stats {
    int sweeps;               /* sweeps run, the last one (which rotated nothing) included; 0 for H = 0 */
    long long rotations;      /* rotations applied */
    double off;               /* the last sweep's worst |g_p^H g_q| / (|g_p| |g_q|) */
} qf_eigh_stats;
/* H_host: Hermitian (N,N).  V_host may be NULL (eigenvalues only); stats may be NULL. */
int qf_eigh(qf_ctx *ctx, const void *H_host, double *lambda_host, void *V_host, qf_eigh_stats *stats);
/* W_host: skew-Hermitian (N,N).  Decomposes -i W, formed on the device: W = V diag(i lambda) V^H. */
int qf_eigh_skew(qf_ctx *ctx, const void *W_host, double *lambda_host, void *V_host, qf_eigh_stats *stats);
/* The same for the context's resident state W: the invariant of the isospectral flow.  Only lambda crosses the bus. */
int qf_eigh_state(qf_ctx *ctx, double *lambda_host, qf_eigh_stats *stats);
/* scale_decomposition(W, P) of quflow/analysis.py:8-34 for a skew-Hermitian stream matrix P: with V the eigenvectors of
 * -i P, Ws = V diag(diag(V^H W V)) V^H (the part of W that commutes with P) and Wr = W - Ws, all on the device.
 * W_host == NULL: the context's resident state.  P_host == NULL: P = Delta^-1 W by the context's own solver
 * (skew-Hermitian form).  Ws_host, Wr_host: (N,N) complex128 each. */
int qf_scale_decomposition(qf_ctx *ctx, const void *W_host, const void *P_host, void *Ws_host, void *Wr_host);

/* ---- Rotations and gradients on the sphere (csrc/geometry.hip; quflow/geometry.py:132-207).  With s = (N-1)/2 and
 *      c_a = sqrt((a+1)(N-1-a)) the generators of so(3) in u(N) are S3 = i diag(a - s), S1[a,a+1] = S1[a+1,a] = i c_a / 2,
 *      S2[a,a+1] = c_a / 2 = -S2[a+1,a]; no kernel stores them.  R = exp(xi . S) by scaling and squaring: with
 *      b0 = |xi . S|_inf (from the closed forms), sigma = max(0, ceil(log2(b0 / 0.5))) and b = b0 / 2^sigma <= 0.5, the
 *      degree-d Taylor polynomial of exp(xi . S / 2^sigma), d the smallest degree with b^d / d! < 1e-18, is written by one
 *      banded kernel and squared sigma times with the ordinary product.  Rounding grows like 2^sigma ~ N |xi|: the
 *      entrywise error of R is a few N max(1, |xi|) eps.  |xi| is NOT reduced modulo 2 pi (for even N a full turn is
 *      -I).  complex128 only.  The work set (two N^2 matrices, 3 N^2 for the gradient) is allocated on the context's
 *      first such call and freed with it. -------- */
/* Host only, no context: the squarings sigma and the degree d the rule above gives for (N, xi); either may be NULL.
 * xi = 0: sigma = 0, d = 1.  A non-finite xi (or one that needs more than 64 squarings), N outside 2..8192: QF_ERR_INVALID. */
int qf_so3_exp_plan(int N, const double xi[3], int *squarings, int *degree);
/* R_host: (N,N) complex128 = exp(xi[0] S1 + xi[1] S2 + xi[2] S3); NULL leaves the matrix on the device (timing).
 * A non-finite xi: QF_ERR_INVALID before any launch. */
int qf_so3_exp(qf_ctx *ctx, const double xi[3], void *R_host);
/* HIP-event times of the most recent exponential of this context (qf_so3_exp, or the one inside qf_rotate): the Taylor
 * launch and the sigma squarings, in milliseconds.  QF_ERR_STATE before the first one. */
int qf_so3_exp_times(qf_ctx *ctx, double *taylor_ms, double *squarings_ms);
/* out = R W R^H (quflow/geometry.py:154-170) for ANY complex W, R = exp(xi . S).  W_host == NULL: the context's resident
 * state, rotated in place (out_host may then be NULL; otherwise it receives the new state as well); the context is left
 * as qf_upload_W leaves it -- the increment of an earlier stepper call is dropped.  An inf or NaN in W:
 * QF_ERR_NONFINITE, nothing is changed. */
int qf_rotate(qf_ctx *ctx, const double xi[3], const void *W_host, void *out_host);
/* dP_host: (3,N,N) complex128, dP[k] = [S_{k+1}, P] -- the reference's grad(P) = bracket(X_k, P) (geometry.py:197-207,
 * X_k = hbar S_k) up to rounding, in one memory-bound pass instead of six dense products.  P_host == NULL: the
 * resident state.  dP_host == NULL: the result stays on the device (timing).  An inf or NaN in P: QF_ERR_NONFINITE. */
int qf_grad(qf_ctx *ctx, const void *P_host, void *dP_host);

/* ---- measurement support (bench.py): HIP-event timing on the ctx stream -------- */
#define QF_KERNEL_POISSON 0
#define QF_KERNEL_GEMM1 1
#define QF_KERNEL_GEMM2 2
#define QF_KERNEL_NORM 3
#define QF_KERNEL_UPDATE 4
#define QF_KERNEL_SLICE 5      /* digit slicing of the int8 products' operands (QUFLOW_HIP_GEMM=i8) */
#define QF_KERNEL_COUNT 6

/* `mask` selects kernels (bit QF_KERNEL_x); every launch of a selected hot-path kernel
 * inside qf_isomp is bracketed by a hipEvent pair on the ctx stream and qf_profile_read
 * sums the elapsed times.  mask = 0 switches the instrumentation off. */
int qf_profile_enable(qf_ctx *ctx, int mask);
int qf_profile_reset(qf_ctx *ctx);
int qf_profile_read(qf_ctx *ctx, int kernel_id, long long *launches, double *total_ms);
/* Sampling: bracket only every `stride`-th launch of an enabled kernel id (default 1 = every launch);
 * qf_profile_read then returns the measured launches and their time, qf_profile_seen all launches
 * of that id since the last reset (bench.py scales the measured mean to them). */
int qf_profile_stride(qf_ctx *ctx, int stride);
int qf_profile_seen(qf_ctx *ctx, int kernel_id, long long *seen);
/* The HIP device with ordinal `device` as this process sees it: a JSON object {"ordinal":.., "pci_bus_id":"0000:05:00.0",
 * "name":"..", "gcn_arch":"gfx950..", "compute_units":.., "memory_bytes":..} -- what a rank of a multi-GPU launch prints
 * about the device it bound (bench.py).  Returns the length of the text (as snprintf), a negative status on error. */
int qf_device_info(int device, char *buf, int n);
/* What this context LAUNCHED for each role of the hot path -- recorded by the launchers themselves at the moment of the
 * launch (not re-derived from the selection rules): a JSON object
 *   {"N":.., "laplacian_inverse":{..}, "first_product":{..}, "second_product":{..}, "slicing":{..}}
 * with, per role that has run since the context was created, the kernel, its tile, workgroups and threads, and for the
 * second product the tiles it multiplies and their share of the full grid ("tile_share"); null for a role that has not
 * run.  bench.py labels its `roofline` object with this.  Returns the length of the text (as snprintf: the text is
 * truncated to n - 1 bytes when n is smaller), a negative status on error. */
int qf_plan_describe(qf_ctx *ctx, char *buf, int n);
/* stream-ordered stopwatch: start/stop record events on the ctx stream */
int qf_timer_start(qf_ctx *ctx);
int qf_timer_stop(qf_ctx *ctx, double *elapsed_ms);

/* ---- debug / parity access to device intermediates (tests only) ---------------- */
#define QF_BUF_W 0
#define QF_BUF_DW 1
#define QF_BUF_WHALF 2
#define QF_BUF_PHALF 3
#define QF_BUF_PW 4
/* what the last qf_mhd_spectral_budget left: P, B and the three tendencies (QF_ERR_STATE before the first such call) */
#define QF_BUF_MHD_P 5
#define QF_BUF_MHD_B 6
#define QF_BUF_MHD_ADVECTION 7
#define QF_BUF_MHD_LORENTZ 8
#define QF_BUF_MHD_INDUCTION 9
int qf_download_buffer(qf_ctx *ctx, int which, void *host);
/* Guard zones around every device allocation of the library (QUFLOW_HIP_DEBUG_GUARD=1 in the environment when the process
 * starts; csrc/guard.hip): reads back the zones of every live allocation and reports how many allocations were made under
 * the guard, how many zones were found damaged so far (live ones now, released ones when they were released) and a
 * description of the first one (truncated to n - 1 bytes).  All zero / empty when the variable is not set.  Stores that
 * land outside an operand are otherwise swallowed by the allocator's granularity; the GPU suite and the size sweeps are
 * run once per round under the variable (tests/conftest.py fails such a session on damage). */
int qf_debug_guard_check(long long *allocations, long long *damaged, char *first, int n);
/* n pairs (er[i], ei[i]) -> out_modulus[i] = |er + i ei| as every residual row sum of the stepper forms it (the library's
 * own square-root sequence, isospectral.py:526,534), out_sqrt[i] = the compiler's sqrt of the same argument: the two
 * must agree bit for bit in the normal range -- the iteration counts rest on it.  n <= N*N of the context. */
int qf_debug_modulus(qf_ctx *ctx, int n, const double *er_host, const double *ei_host, double *out_modulus_host,
                     double *out_sqrt_host);
/* What the Newton-Schulz inverse did in the last qf_isomp_simple / qf_isomp_quasinewton call (plain or hooked) of this
 * context: out[0] inversions asked for, out[1] cold starts (no inverse yet, or the previous one's residual against the new
 * A was not below 0.5), out[2] inverses kept as they were (A moved by no more than the inverse's rounding noise), out[3]
 * Newton-Schulz iterations in all.  The general branch of isomp_simple inverts twice per step; both count.  Counted on the
 * host, reset when such a call starts, read-only. */
int qf_ns_stats(qf_ctx *ctx, long long out[4]);
/* C = A @ B for host matrices through the MFMA zgemm of the stepper (parity tests of
 * the commutator pair, isospectral.py:496,499). */
int qf_zgemm(qf_ctx *ctx, const void *A_host, const void *B_host, void *C_host);
/* The commutators of quflow/integrators/isospectral.py:22-57 on host matrices, product(s) AND combination on the device
 * (round 6: one PCIe round trip, no host pass):  skewherm = 1: X - X^H with X = W @ P (commutator_skewherm, one product);
 * skewherm = 0: W @ P - P @ W (commutator_generic, two products).  The subtraction is the reference's elementwise one
 * (x - y, x - conj(y^T): exact negation, one rounding), so the result has the bits of the product followed by numpy's
 * `VF -= ...`.  Uses the context's per-iteration staging matrices (stage, Phalf, PW, Whalf), which are free between
 * stepper calls -- the resident state W and a carried increment are not touched. */
int qf_commutator(qf_ctx *ctx, const void *W_host, const void *P_host, void *C_host, int skewherm);
/* C = A @ B on the INT8 matrix cores by digit splitting (ozaki.hip; BASELINE.json config 3's
 * low-precision-MFMA commutator): A general, B SKEW-HERMITIAN (as every right operand of the
 * iteration is); truncation error 2^-35 of (row scale of A) x (column scale of B). N % 64 == 0. */
int qf_zgemm_i8(qf_ctx *ctx, const void *A_host, const void *B_host, void *C_host);
/* The two products of ONE fixed-point iteration with their fused epilogue, on host operands
 * (isospectral.py:496-509,481-482,526-534):  PW = Phalf @ Whalf;  dW_new = PW @ Phalf + (PW - PW^H);
 * Whalf_new = W + dW_new;  rowsum[i] = sum_j |dW_old[i,j] - dW_new[i,j]|  (N doubles).
 * variant (low 4 bits) 0: full second product; 1: the upper-triangle stream-K form the stepper uses
 * for skew-Hermitian W at the large sizes (N % 64 == 0 only); 2: the upper triangle of 32 x 32 tiles (smaller sizes, any N
 * >= 64).  The parity tests also choose the partition here, which the stepper takes from rules: kind 1: bits 8-15 = least
 * K-tiles per workgroup, bits 16-23 = 64 + epilogue weight (0: the rule); kind 2: bits 8-11 / 12-15 = K pieces per
 * off-diagonal / diagonal tile (1, 2, 4; 0: the rule).  Parity-test entry: the stepper itself never round-trips through
 * the host. */
int qf_fixedpoint_products(qf_ctx *ctx, const void *Phalf_host, const void *Whalf_host, const void *W_host,
                           const void *dW_old_host, int variant, void *dW_new_host, void *Whalf_new_host,
                           double *rowsum_host);

/* ---- complex64 data.  The reference computes complex64 input in single precision throughout: float32
 *      coefficient tables and a float32 Thomas solve (quflow/laplacian/cpu.py:725, `dtype=type(W[0,0].real)`),
 *      complex64 np.matmul for the two products (quflow/integrators/isospectral.py:496,499), complex64
 *      elementwise passes (:481-592), and the automatic tolerance from the float32 machine epsilon
 *      (np.finfo(W.dtype).eps, :440-448).  These entry points are that path on the device: matrices are
 *      N x N, C order, complex64 as interleaved (re, im) floats; the solve runs on float32 factor tables, the
 *      products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), Kahan summation (compsum) in float32.  The
 *      float32 working set of a context is allocated on first use; its state is separate from the complex128
 *      one.  Scalars (dt, tol, statistics, diagnostics) stay double. -------------------------------------- */
/* laplacian(N, bc, dtype=float32): cpu.py:55-95.  (N,N,2) float32 to host memory. */
int qf_c64_laplacian_table(qf_ctx *ctx, int bc, float *lap_host);
/* solve_poisson(W) for complex64 W: cpu.py:681-734 with float32 tables (:725).  Host in, host out. */
int qf_c64_solve_poisson(qf_ctx *ctx, const void *W_host, void *P_host, int skewh);
/* _solve_cpu(lap, W, P, ...) with a caller-supplied (N,N,2) float32 table on complex64 data: solve_heat /
 * solve_helmholtz / solve_viscdamp / solve_globalqg on complex64 input (cpu.py:737-943 build their tables with
 * dtype=type(W[0,0].real)).  Host in, host out; the table is factorised on every call. */
int qf_c64_solve_tridiagonal(qf_ctx *ctx, const float *lap_host, const void *W_host, void *P_host, int skewh);
/* laplace(P) for complex64 P: cpu.py:628-669 with the float32 table (:664). */
int qf_c64_laplace(qf_ctx *ctx, const void *P_host, void *W_host);
int qf_c64_upload_W(qf_ctx *ctx, const void *W_host);     /* host complex64 -> the context's complex64 state */
int qf_c64_download_W(qf_ctx *ctx, void *W_host);
/* isomp_fixedpoint on the complex64 state (arguments as qf_isomp); tol < 0 -> 'auto' with the float32 machine
 * epsilon: sqrt(eps32)*dt/hbar*|W|_inf, or eps32*... with compsum (isospectral.py:440-448). */
int qf_c64_isomp(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int compsum, int reinitialize,
                 qf_isomp_stats *stats_out);
int qf_c64_isomp_continue(qf_ctx *ctx, double dt, int steps, double tol, int minit, int maxit, int compsum, int reinitialize,
                          qf_isomp_stats *stats_out);
/* energy_euler / enstrophy of the complex64 state (quflow/physics.py:26-38) */
int qf_c64_diagnostics(qf_ctx *ctx, double *energy_euler, double *enstrophy);
/* C = A @ B for complex64 host matrices through the stepper's fp32-MFMA product (parity tests; isospectral.py:496,499) */
int qf_cgemm(qf_ctx *ctx, const void *A_host, const void *B_host, void *C_host);
/* the two products of one fixed-point iteration with the fused epilogue on complex64 host operands (as
 * qf_fixedpoint_products, full second product); rowsum: N doubles */
int qf_c64_fixedpoint_products(qf_ctx *ctx, const void *Phalf_host, const void *Whalf_host, const void *W_host,
                               const void *dW_old_host, void *dW_new_host, void *Whalf_new_host, double *rowsum_host);
/* The same through the upper-triangle second product on 32 x 32 tiles (any N >= 64, skew-Hermitian operands): the kernel the
 * complex64 stepper uses at every N >= 64 on an exactly skew-Hermitian state.  dW comes back completed by its mirror image. */
int qf_c64_fixedpoint_products_tri(qf_ctx *ctx, const void *Phalf_host, const void *Whalf_host, const void *W_host,
                                   const void *dW_old_host, void *dW_new_host, void *Whalf_new_host, double *rowsum_host);

/* ---- ensemble diagnostics gather over RCCL, one process per GPU (the reference
 *      has no distributed code -- this row has no reference interface to cite).  Torch-free alternative to
 *      the torch.distributed route of quflow_amd/ensemble.py: rank 0 draws the id, the ranks exchange its
 *      128 bytes themselves (quflow_amd/comm.py: a TCP hand-out on MASTER_ADDR), every rank creates its
 *      communicator.  librccl.so is dlopen'ed on first use (QUFLOW_HIP_RCCL_LIB overrides the name). ---- */
#define QF_COMM_ID_BYTES 128
typedef struct qf_comm qf_comm;
int qf_comm_unique_id(void *id128);
int qf_comm_create(qf_comm **out, int device, int nranks, int rank, const void *id128);
/* recv_host holds nranks * count doubles, rank r's block at r * count; every rank passes the same count */
int qf_comm_allgather_f64(qf_comm *comm, const double *send_host, int count, double *recv_host);
int qf_comm_barrier(qf_comm *comm);
int qf_comm_destroy(qf_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* QUFLOW_HIP_H */
