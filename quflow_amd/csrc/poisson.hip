// Per-diagonal tridiagonal Laplacian kernels for gfx950.
//
// Reference semantics: quflow/laplacian/cpu.py
//   _compute_cpu_laplacian  :55-95    coefficient table lap[i,j,{0,1}]
//   _solve_cpu_skewh        :281-362  Thomas solve of the N upper diagonals + mirror
//   _solve_cpu_nonskewh     :200-278  Thomas solve of all 2N-1 diagonals
//   _dot_cpu_generic        :98-108   3-point stencil along diagonals
//
// Design (MI355X-first, not a translation of the numba loops)
// ---------------------------------------------------------
// * Flat walk.  Entry (i,j) has flat index e = i*N + j; stepping along a diagonal is
//   e += N+1.  Starting from e = t (t = 0..N) the walk covers upper diagonal t and then
//   wraps into lower diagonal -(N+1-t); the coupling coefficient a_0 at the head of every
//   diagonal is 0, so chained diagonals decouple.  At a fixed step k the entries of
//   consecutive walks t, t+1, ... are CONSECUTIVE in memory: every load/store of the
//   sweeps is a unit-stride, fully coalesced access with no gather.
// * The matrix T_m is data independent, so its LU factors are computed once per (N, table)
//   by k_build_factors (multipliers w_k = a_k/b'_{k-1}, reciprocal pivots 1/b'_k).  A solve
//   is then two first-order linear recurrences
//        forward   y_k = f_k - w_k y_{k-1}
//        backward  p_k = y_k/b'_k - w_{k+1} p_{k+1}
//   i.e. one dependent FMA per step instead of the reference's divide chain.
// * Depth reduction.  Each walk is cut into chunks of L steps (8 for N <= 512, 16 below 768; 9 / 17 in the folded
//   layout of the skew-Hermitian solve from N = 768 on; 32 beyond N = 2175); a thread owns one chunk in registers.  Pass 1 sweeps every chunk with a zero
//   carry-in (all chunks of all diagonals in parallel); pass 2 forms the chunk carries by a
//   wavefront scan of the affine maps y -> a y + b over the chunks of a walk (DPP row_shr /
//   row_bcast lane moves, registers only: log2(C) + 1 steps for C <= 64 chunks, two chunks per lane up to 128; the
//   sequential pass over the chunks is left for longer walks only); pass 3 adds
//   carry * prod(-w) to every entry.  Sequential depth drops from 2N to about
//   2(2L + log2(N/L)) dependent FMAs; HBM/L2 traffic is the algorithmic minimum (W once, the
//   factor table once, P once).
// * Folded walk slots (skew-Hermitian solve, 768 <= N <= 2175): the upper triangle's walks have lengths N .. 1; slot f
//   carries walk f FOLLOWED BY walk N-1-f as one sequence of N + 1 entries -- the zero multiplier at the head of a walk
//   restarts both recurrences at the junction -- so every slot is full: half the workgroups, none of them half idle.
// * The kernel is instantiated for double (complex128 data) and for float (complex64 data: the
//   reference solves those with float32 tables and float32 arithmetic, cpu.py:725).
// * m = 0: tr(W)/N is removed from the right-hand side and tr(P)/N from the solution
//   (cpu.py:311-317,342-352) with deterministic block reductions.
#include "qf_internal.h"
#include "qf_step_end.h"

#pragma clang fp contract(off)  // table arithmetic mirrors the reference's op order; FMAs are explicit

// Diagnostic builds only (tools/solve_probe.hip): switches that drop parts of k_solve so that
// their cost can be read off timing differences.  Never defined in the shipped library.
#ifdef QF_PROBE
__device__ int qf_probe_flags = 0;
__device__ unsigned long long *qf_probe_stamps = nullptr;  // [blocks*waves][16]
#define QF_PROBE_SKIP(bit_) (qf_probe_flags & (1 << (bit_)))
#define QF_PROBE_STAMP(slot_)                                                                     \
    if (qf_probe_stamps && (threadIdx.x & 63) == 0)                                               \
        qf_probe_stamps[((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (slot_)] = __builtin_amdgcn_s_memtime();
#else
#define QF_PROBE_SKIP(bit_) 0
#define QF_PROBE_STAMP(slot_)
#endif

namespace {

// R = float: the reference's float32 table for complex64 input (cpu.py:55-95 with dtype=float32, cpu.py:725):
// the integer-valued diagonal cast to float32 (exact below 2^24), the double-precision square root rounded
// to float32, the boundary condition subtracted in float32.
template <typename R>
__global__ void k_lap_table(int N, int bc, R *__restrict__ lap)
{
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)N * N) return;
    int i = (int)(e / N), j = (int)(e % N);
    R b = (R)qf_lap_b(N, i, j);
    if (bc && e == 0) b -= R(0.5);  // cpu.py:90
    lap[2 * e] = b;
    lap[2 * e + 1] = (R)qf_lap_a(N, i, j);
}

// One thread per flat walk t = 0..N; sequential (runs once per table).
// Same operation order as cpu.py:309,324-325: w = a/b'_{k-1}; b'_k = b_k - w a_k.
template <typename R, typename C2>
__global__ void k_build_factors(int N, const R *__restrict__ lap, C2 *__restrict__ tab)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > N) return;
    size_t NN = (size_t)N * N;
    R bp_prev = R(1);
    for (size_t e = t; e < NN; e += (size_t)N + 1) {
        int i = (int)(e / N), j = (int)(e % N);
        R b = lap[2 * e], a = lap[2 * e + 1];
        R w, bp;
        if (i == 0 || j == 0) {  // head of a diagonal: the reference starts its sweep at k = 1
            w = R(0);
            bp = b;
        } else {
            w = a / bp_prev;
            bp = b - w * a;
        }
        C2 f;
        f.x = w;
        f.y = R(1) / bp;
        tab[e] = f;
        bp_prev = bp;
    }
}

// _dot_cpu_generic, cpu.py:98-108 (coefficients recomputed on the fly: no table traffic)
template <typename R, typename C2>
__global__ void k_laplace(int N, const C2 *__restrict__ P, C2 *__restrict__ W)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int i = blockIdx.y;
    if (j >= N) return;
    W[(size_t)i * N + j] = qf_laplace_entry<R, C2>(N, P, i, j);
}

// W = scale * (Delta P): magmp's Bhalf = vareps * Delta Thetahalf without the second pass.  The stencil sum is rounded as
// k_laplace rounds it, then multiplied once (what k_lincomb does to k_laplace's output: same bits).
__global__ void k_laplace_scaled(int N, const double2 *__restrict__ P, double2 *__restrict__ W, double scale)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int i = blockIdx.y;
    if (j >= N) return;
    const double2 o = qf_laplace_entry<double, double2>(N, P, i, j);
    W[(size_t)i * N + j] = make_double2(scale * o.x, scale * o.y);
}

// ---- real-type traits: the solve is instantiated for double (complex128 data) and float (complex64 data: the
// reference solves complex64 input with float32 tables and float32 arithmetic, cpu.py:725)
template <typename R> struct rt;
template <> struct rt<double> { typedef double2 C; };
template <> struct rt<float> { typedef float2 C; };
template <typename R> __device__ __forceinline__ typename rt<R>::C mkc(R x, R y);
template <> __device__ __forceinline__ double2 mkc<double>(double x, double y) { return make_double2(x, y); }
template <> __device__ __forceinline__ float2 mkc<float>(float x, float y) { return make_float2(x, y); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return __fma_rn(a, b, c); }
__device__ __forceinline__ float fma_r(float a, float b, float c) { return __fmaf_rn(a, b, c); }

// DPP lane moves of a double (two dwords) or a float: no LDS crossbar, ~2 VALU issues instead of two
// ds_bpermute round trips (a __shfl_up of a double).  Lanes without a valid source keep their own value.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_mov(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float v)
{
    int x = __float_as_int(v);
    x = __builtin_amdgcn_update_dpp(x, x, CTRL, ROW_MASK, 0xf, false);
    return __int_as_float(x);
}

// the same move with 0.0 where a lane has no source (reductions)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_mov_or_zero(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov_or_zero(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ double read_lane63(double v)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ float read_lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }

// sum over the 64 lanes of a wavefront in a fixed order, returned in every lane: running sums inside the
// rows of 16 (row_shr 1, 2, 4, 8), row totals handed on (row_bcast:15, row_bcast:31), lane 63 read back.
// Registers only -- a __shfl_xor butterfly on doubles is 12 ds_bpermute round trips.
template <typename R>
__device__ __forceinline__ R wave_total(R v)
{
    v += dpp_mov_or_zero<0x111, 0xf>(v);
    v += dpp_mov_or_zero<0x112, 0xf>(v);
    v += dpp_mov_or_zero<0x114, 0xf>(v);
    v += dpp_mov_or_zero<0x118, 0xf>(v);
    v += dpp_mov_or_zero<0x142, 0xa>(v);
    v += dpp_mov_or_zero<0x143, 0xc>(v);
    return read_lane63(v);
}

// deterministic block-wide sum of a complex value in two halves: wave_total inside each wavefront, the wave totals
// left in red[wave] (post); after ONE barrier of the caller's -- an existing one where there is one -- every thread
// adds the wave totals in wave order (read).  red[] must not be written again before every thread has read it.
template <typename R>
__device__ __forceinline__ void block_sum_post(typename rt<R>::C v, typename rt<R>::C *red, int tid)
{
    v.x = wave_total(v.x);
    v.y = wave_total(v.y);
    if ((tid & 63) == 0) red[tid >> 6] = v;
}
template <typename R>
__device__ __forceinline__ typename rt<R>::C block_sum_read(const typename rt<R>::C *red, int nthreads)
{
    typename rt<R>::C r = mkc<R>(R(0), R(0));
    for (int w = 0; w < (nthreads >> 6); ++w) {
        r.x += red[w].x;
        r.y += red[w].y;
    }
    return r;
}

// Inclusive scan of affine maps y -> a*y + b over segments of `width` consecutive lanes (width a power
// of two <= 64, lane = index inside the wavefront): after the call a lane holds the composition of the
// maps of its segment's lanes up to and including itself.  Kogge-Stone inside the rows of 16 lanes
// (DPP row_shr 1, 2, 4, 8), then the row totals are handed on with row_bcast:15 (rows 1 and 3 take
// lane 15 of the row before) and row_bcast:31 (rows 2 and 3 take lane 31): six steps, registers only.
template <typename R>
__device__ __forceinline__ void scan_affine(R &a, typename rt<R>::C &b, int lane, int width)
{
    const int l = lane & (width - 1);
#define QF_SCAN_STEP(D_)                                                               \
    if (width > (D_)) {                                                                \
        const R ap = dpp_mov<0x110 + (D_), 0xf>(a);                                    \
        const R bx = dpp_mov<0x110 + (D_), 0xf>(b.x);                                  \
        const R by = dpp_mov<0x110 + (D_), 0xf>(b.y);                                  \
        if (l >= (D_) && (lane & 15) >= (D_)) {                                        \
            b.x = fma_r(a, bx, b.x);                                                   \
            b.y = fma_r(a, by, b.y);                                                   \
            a *= ap;                                                                   \
        }                                                                              \
    }
    QF_SCAN_STEP(1)
    QF_SCAN_STEP(2)
    QF_SCAN_STEP(4)
    QF_SCAN_STEP(8)
#undef QF_SCAN_STEP
    if (width > 16) {      // row_bcast:15 into rows 1 and 3
        const R ap = dpp_mov<0x142, 0xa>(a);
        const R bx = dpp_mov<0x142, 0xa>(b.x);
        const R by = dpp_mov<0x142, 0xa>(b.y);
        if (lane & 16) {
            b.x = fma_r(a, bx, b.x);
            b.y = fma_r(a, by, b.y);
            a *= ap;
        }
    }
    if (width > 32) {      // row_bcast:31 into rows 2 and 3
        const R ap = dpp_mov<0x143, 0xc>(a);
        const R bx = dpp_mov<0x143, 0xc>(b.x);
        const R by = dpp_mov<0x143, 0xc>(b.y);
        if (lane & 32) {
            b.x = fma_r(a, bx, b.x);
            b.y = fma_r(a, by, b.y);
            a *= ap;
        }
    }
}

// value of the lane before (wave_shr:1), for the exclusive carries; lane 0 keeps its own
template <typename R> __device__ __forceinline__ R lane_before(R v) { return dpp_mov<0x138, 0xf>(v); }

// chunk carries of one recurrence for up to 64 chunks per walk: lane l of a segment of Cp lanes takes chunk l
// (REVERSE: chunk C-1-l), the segment scans the chunks' affine maps, and the carry INTO a chunk is the value at the end
// of the chunk before it.  CPW = 64: the segment is the whole wavefront (33..64 chunks: N = 512's 64 chunks of 8
// entries), known at compile time -- no runtime width in the six scan steps, no division by it; CPW = 0: runtime Cp.
template <typename R, int CPW, bool REVERSE>
__device__ __forceinline__ void scan_chunks(int C, int G, int CE, int CR, int GP, const R *endc, const typename rt<R>::C *endv,
                                            typename rt<R>::C *carry, int lane, int wave, int nwaves)
{
    typedef typename rt<R>::C cplx;
    int Cp = CPW;
    if (!CPW) {
        Cp = 1;
        while (Cp < C) Cp <<= 1;
    }
    const int dpw = 64 / Cp;                 // walks per wavefront
    const int l = lane & (Cp - 1);
    const int q = REVERSE ? C - 1 - l : l;
    for (int gd = wave * dpw + (CPW == 64 ? 0 : lane / Cp); gd < G; gd += nwaves * dpw) {
        R a = R(0);
        cplx b = mkc<R>(R(0), R(0));
        if (l < C) {
            a = endc[gd * CR + q];
            b = endv[gd * CE + q];
        }
        scan_affine(a, b, lane, Cp);
        const R cx = lane_before(b.x), cy = lane_before(b.y);
        if (l < C) carry[q * GP + gd] = (l == 0) ? mkc<R>(R(0), R(0)) : mkc<R>(cx, cy);
    }
}

// Chunked two-level Thomas solve.  Block = G walks x C chunks (G*C threads, lane-fastest in g).
//   SKEWH = 1: walks t = 0..N-1 restricted to the upper triangle (length N-t), result
//              mirrored as P[j,i] = -conj(P[i,j])           (cpu.py:281-362)
//   SKEWH = 0: walks t = 0..N over the whole matrix          (cpu.py:200-278)
// Chunk carries: with C <= 64 one wavefront scans all chunks of a walk with shuffles
// (log2 C steps); longer walks fall back to a sequential pass over the chunks.
// Mirror: the block's results are staged in LDS and written as 16*G-byte row segments
// (the entries (k+t, k) of G consecutive walks t are G consecutive columns of row k+t).
// FOLD = 1 (skew-Hermitian solve of the larger sizes): walk slot f carries walk t = f (length N - f) FOLLOWED BY walk
//   N-1-f (length f + 1) as one sequence of N + 1 entries -- the table's multiplier at the head of a walk is zero, so
//   the recurrences restart at the junction by themselves (the flat walks of SKEWH = 0 rely on the same).  Every slot
//   is full: half the workgroups of the triangle's walk-per-slot layout, none of them half idle.
template <typename R, int L, int SKEWH, int FOLD = 0>
__global__ __launch_bounds__(L <= 17 ? 512 : 256) void k_solve(int N, int G, int C, const typename rt<R>::C *__restrict__ W,
                        typename rt<R>::C *__restrict__ P, const typename rt<R>::C *__restrict__ tab, R scale,
                        qf_guard guard, qf_decide dec, int tail_off)
#define QF_SOLVE_OFFSET 0
#include "poisson_solve_body.h"
#undef QF_SOLVE_OFFSET

// P = scale * T^-1 (W - F), the installed Hamiltonian with an offset (qf_set_hamiltonian): double precision, skew-Hermitian
// solve, every chunk class of pick_cfg.  A second kernel NAME: k_solve keeps its template parameters.
template <int L, int FOLD>
__global__ __launch_bounds__(L <= 17 ? 512 : 256) void k_solve_off(int N, int G, int C, const double2 *__restrict__ W,
                        double2 *__restrict__ P, const double2 *__restrict__ tab, const double2 *__restrict__ F, double scale,
                        qf_guard guard, qf_decide dec, int tail_off)
#define QF_SOLVE_OFFSET 1
#include "poisson_solve_body.h"
#undef QF_SOLVE_OFFSET

// the deferred decision alone: behind the last second product of a call there is no solve to take it
__global__ __launch_bounds__(256) void k_decide(int N, qf_decide dec)
{
    __shared__ double scratch[40];
    if (!dec.state_rw->pending) return;
    const qf_new_state ns = qf_decide_compute(N, dec.slots, dec.rowpart, dec.state_rw, scratch);
    if (threadIdx.x == 0) qf_decide_apply(dec.state_rw, dec.rec, dec.ticket, ns);
}

struct solve_cfg {
    int L, G, C, threads, fold, T;
    size_t smem;
};

// folded walk slots (k_solve<.., FOLD = 1>) for the skew-Hermitian solve from N = 768 on.  Above N = 1024 the
// walk-per-slot layout needs 32-entry chunks (256 VGPRs + spills, one wavefront per SIMD) and, at N = 2048, two rounds
// of 256 workgroups: 50.1 -> 36.9 us there, 40.2 -> 27.0 at N = 1536 (tools/solve_probe.hip); at N = 768 / 1024 the
// 9-entry chunks shorten the four sweeps (17.0 -> 14.5, 19.6 -> 17.8 us; stepper +1.9 % / +0.7 % with two slots per
// workgroup, i.e. 256 workgroups at N = 1024); below, the stepper loses (N = 512: 9,168 -> 8,895 timesteps/s).
// (QUFLOW_HIP_SOLVE_FOLD=0 / 1: never / from N = 256 on, for A/B runs)
bool fold_wanted(int N, int skewh)
{
    const char *e = getenv("QUFLOW_HIP_SOLVE_FOLD");     // (read per launch: the tests switch it inside one process)
    const int forced = e ? atoi(e) : -1;
    if (!skewh || N + 1 > 17 * 128) return false;
    if (forced == 0) return false;
    if (forced == 1) return N >= 256;
    return N >= 768;
}

solve_cfg pick_cfg(int N, size_t csize = sizeof(cplx), bool fold = false)
{
    solve_cfg c;
    c.fold = fold ? 1 : 0;
    c.T = N;
    if (fold) {
        // N + 1 entries per slot, at most 128 chunks (two per lane of the scanning wavefront)
        c.L = (N + 1 <= 9 * 128) ? 9 : 17;
        c.C = (N + 1 + c.L - 1) / c.L;
        c.T = (N + 1) / 2;
        int G = 64;
        while (G > 1 && G * c.C > 512) G >>= 1;
        // a workgroup per CU matters more than 64-byte row segments (N = 1024: two slots, 256 workgroups)
        while (G > 2 && (c.T + G - 1) / G < 256) G >>= 1;
        c.G = G;
        c.threads = ((G * c.C + 63) / 64) * 64;
        const size_t scan_bytes = (size_t)(c.C + 2) * G * csize + (size_t)c.C * (G + 1) * csize + (size_t)c.threads * csize +
                                  (size_t)(c.C + 4) * G * (csize / 2);
        const size_t tile_bytes = (size_t)c.C * c.L * G * csize;
        c.smem = (((scan_bytes > tile_bytes ? scan_bytes : tile_bytes) + 15) & ~(size_t)15) + 8 * csize;   // + red2[] (16-byte aligned): the tr(P) wave totals
        return c;
    }
    c.L = 16;
    c.C = (N + c.L - 1) / c.L;
    // more than 64 chunks per walk cannot be scanned by one wavefront (the serial carry pass takes over):
    // longer chunks from N > 1024 on
    if (c.C > 64) {
        c.L = 32;
        c.C = (N + c.L - 1) / c.L;
    } else if ((N + 3) / 4 <= 64) {
        // N <= 256 (round 6): 4-step chunks, still one chunk per scanning lane -- N = 256 14,891 -> 15,145-15,201 timesteps/s
        // (+1.9 %, three same-box pairs, profiles/r06_solve_l4_ab.txt).  At N = 512 four-step chunks mean 128 chunks per walk,
        // scanned two per lane: 9,783-9,831 -> 9,755-9,787 with 4 walks per workgroup, 9,698-9,708 with 2 -- not taken.
        c.L = 4;
        c.C = (N + 3) / 4;
    } else if ((N + 7) / 8 <= 64) {
        // N <= 512: 8-step chunks still fit one wavefront's scan (<= 64 chunks per walk) -- half the serial depth
        // of the four sweeps for one scan step more: N=512 13.6 -> 12.4 us in tools/solve_probe.hip, 8,749 -> 8,922
        // timesteps/s; N=256 12.2 -> 10.7 us
        c.L = 8;
        c.C = (N + 7) / 8;
    }
    const int max_threads = c.L <= 16 ? 512 : 256;  // register budget of k_solve<L>
    int G = 64;
    while (G > 1 && G * c.C > max_threads) G >>= 1;
    // The solve is bound by per-CU load/store bandwidth, not by HBM: spread it over all 256
    // CUs (64-byte row segments per walk group are still whole L2 requests)
    while (G > 4 && (N + G - 1) / G < 256) G >>= 1;
    c.G = G;
    c.threads = ((G * c.C + 63) / 64) * 64;
    // chunk-end values and carries (complex), chunk-end products (real), reduction scratch (complex)
    const size_t scan_bytes = (size_t)(c.C + 2) * G * csize + (size_t)c.C * (G + 1) * csize + (size_t)c.threads * csize +
                              (size_t)(c.C + 4) * G * (csize / 2);        // (padded strides: see the kernel)
    const size_t tile_bytes = (size_t)c.C * (c.L + 1) * G * csize;   // mirror staging (skew-Hermitian solve), one padding row per chunk
    c.smem = (((scan_bytes > tile_bytes ? scan_bytes : tile_bytes) + 15) & ~(size_t)15) + 8 * csize;   // + red2[] (16-byte aligned): the tr(P) wave totals
    return c;
}

template <typename R>
int launch_solve(qf_ctx *ctx, const typename rt<R>::C *tab, const typename rt<R>::C *W, typename rt<R>::C *P, R scale, int skewh,
                 const qf_guard &guard, const qf_decide *decp = nullptr, const typename rt<R>::C *F = nullptr)
{
    if (F && (sizeof(R) != sizeof(double) || !skewh)) {
        qf_set_error("qf_launch_solve: the offset form exists for the double-precision skew-Hermitian solve only");
        return QF_ERR_UNSUPPORTED;
    }
    qf_decide dec;
    if (decp) dec = *decp;
    const int N = ctx->N;
    solve_cfg c = pick_cfg(N, sizeof(typename rt<R>::C), fold_wanted(N, skewh));
    if (c.G * c.C > (c.L <= 17 ? 512 : 256)) {
        qf_set_error("qf_launch_solve: N=%d too large for the chunked solver", N);
        return QF_ERR_INVALID;
    }
    const int T = c.fold ? c.T : (skewh ? N : N + 1);
    unsigned blocks = (unsigned)((T + c.G - 1) / c.G);
    dim3 grid(blocks), block(c.threads);
    if (c.smem > 160 * 1024) {
        qf_set_error("qf_launch_solve: N=%d needs %zu bytes of LDS", N, c.smem);
        return QF_ERR_INVALID;
    }
#define QF_SOLVE_F(LL, SK, FO)                                                                      \
    {                                                                                               \
        static qf_smem_attr attr;                                                                   \
        QF_TRY(qf_smem_attr_set(attr, (const void *)k_solve<R, LL, SK, FO>, ctx->device, c.smem));  \
        hipLaunchKernelGGL((k_solve<R, LL, SK, FO>), grid, block, c.smem, ctx->stream, N, c.G, c.C, W, P, tab,  \
                           scale, guard, dec, (int)c.smem - 8 * (int)sizeof(typename rt<R>::C)); \
    }
#define QF_SOLVE(LL, SK) QF_SOLVE_F(LL, SK, 0)
    qf_plan_note(ctx, 0x4000000ull | (unsigned long long)(c.L << 16 | c.G << 8 | (F ? 8 : 0) | c.fold << 2 | (skewh ? 2 : 0) | (sizeof(R) == 4 ? 1 : 0)),
                 "{\"kernel\": \"k_solve%s<%s, L=%d, %s%s>\", \"chunk\": %d, \"chunks_per_walk\": %d, \"walks_per_workgroup\": %d, "
                 "\"workgroups\": %u, \"threads\": %d, \"lds_bytes\": %zu, \"step_end\": \"%s\"}",
                 F ? "_off" : "", sizeof(R) == 4 ? "float" : "double", c.L, skewh ? "skew-Hermitian" : "general", c.fold ? ", folded walk slots" : "", c.L, c.C,
                 c.G, blocks, c.threads, c.smem, dec.state_rw ? "takes the deferred decision of the previous iteration" : "none");
    if constexpr (sizeof(R) == sizeof(double)) {
        if (F) {
#define QF_SOLVE_OFF(LL, FO)                                                                        \
    {                                                                                               \
        static qf_smem_attr attr;                                                                   \
        QF_TRY(qf_smem_attr_set(attr, (const void *)k_solve_off<LL, FO>, ctx->device, c.smem));     \
        hipLaunchKernelGGL((k_solve_off<LL, FO>), grid, block, c.smem, ctx->stream, N, c.G, c.C, W, P, tab, F,  \
                           scale, guard, dec, (int)c.smem - 8 * (int)sizeof(typename rt<R>::C)); \
    }
            if (c.fold) {
                if (c.L == 9) QF_SOLVE_OFF(9, 1) else QF_SOLVE_OFF(17, 1)
            } else if (c.L == 4) QF_SOLVE_OFF(4, 0)
            else if (c.L == 8) QF_SOLVE_OFF(8, 0)
            else if (c.L == 16) QF_SOLVE_OFF(16, 0)
            else QF_SOLVE_OFF(32, 0)
#undef QF_SOLVE_OFF
            QF_HIP(hipGetLastError());
            return QF_OK;
        }
    }
    if (c.fold) {
        if (c.L == 9) QF_SOLVE_F(9, 1, 1) else QF_SOLVE_F(17, 1, 1)
    } else if (c.L == 4) {
        if (skewh) QF_SOLVE(4, 1) else QF_SOLVE(4, 0)
    } else if (c.L == 8) {
        if (skewh) QF_SOLVE(8, 1) else QF_SOLVE(8, 0)
    } else if (c.L == 16) {
        if (skewh) QF_SOLVE(16, 1) else QF_SOLVE(16, 0)
    } else {
        if (skewh) QF_SOLVE(32, 1) else QF_SOLVE(32, 0)
    }
#undef QF_SOLVE
#undef QF_SOLVE_F
    QF_HIP(hipGetLastError());
    return QF_OK;
}

}  // namespace

int qf_launch_lap_table(qf_ctx *ctx, int bc, double *lap_dev)
{
    size_t NN = (size_t)ctx->N * ctx->N;
    int threads = 256;
    unsigned blocks = (unsigned)((NN + threads - 1) / threads);
    hipLaunchKernelGGL(k_lap_table<double>, dim3(blocks), dim3(threads), 0, ctx->stream, ctx->N, bc, lap_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_build_factors(qf_ctx *ctx, const double *lap_dev, qf_factors f)
{
    int threads = 64;
    unsigned blocks = (unsigned)((ctx->N + 1 + threads - 1) / threads);
    hipLaunchKernelGGL((k_build_factors<double, double2>), dim3(blocks), dim3(threads), 0, ctx->stream, ctx->N, lap_dev, f.tab);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_solve(qf_ctx *ctx, const qf_factors &f, const cplx *W, cplx *P, double scale, int skewh,
                    qf_guard guard, const qf_decide *dec)
{
    return launch_solve<double>(ctx, f.tab, W, P, scale, skewh, guard, dec);
}

// The stream matrix OF THE FLOW: the built-in Delta^-1 W, or what qf_set_hamiltonian installed -- other factors, an offset,
// or both.  With nothing installed this is qf_launch_solve(ctx, ctx->poisson, ..., 1, ...), launch for launch.
int qf_launch_hamiltonian(qf_ctx *ctx, const cplx *W, cplx *P, double scale, qf_guard guard, const qf_decide *dec)
{
    const qf_factors &f = ctx->ham_table ? ctx->ham : ctx->poisson;
    return launch_solve<double>(ctx, f.tab, W, P, scale, 1, guard, dec, ctx->ham_offset_on ? ctx->ham_offset : nullptr);
}

int qf_launch_decide(qf_ctx *ctx, const qf_decide &dec)
{
    hipLaunchKernelGGL(k_decide, dim3(1), dim3(256), 0, ctx->stream, ctx->N, dec);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_laplace(qf_ctx *ctx, const cplx *P, cplx *W)
{
    const int N = ctx->N;
    dim3 block(256), grid((N + 255) / 256, N);
    hipLaunchKernelGGL((k_laplace<double, double2>), grid, block, 0, ctx->stream, N, P, W);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_laplace_scaled(qf_ctx *ctx, const cplx *P, cplx *W, double scale)
{
    const int N = ctx->N;
    dim3 block(256), grid((N + 255) / 256, N);
    hipLaunchKernelGGL(k_laplace_scaled, grid, block, 0, ctx->stream, N, P, W, scale);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

// ---- complex64 data: float32 tables, float32 arithmetic (cpu.py:725) ----
int qf_launch_lap_table(qf_ctx *ctx, int bc, float *lap_dev)
{
    size_t NN = (size_t)ctx->N * ctx->N;
    int threads = 256;
    unsigned blocks = (unsigned)((NN + threads - 1) / threads);
    hipLaunchKernelGGL(k_lap_table<float>, dim3(blocks), dim3(threads), 0, ctx->stream, ctx->N, bc, lap_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_build_factors(qf_ctx *ctx, const float *lap_dev, float2 *tab)
{
    int threads = 64;
    unsigned blocks = (unsigned)((ctx->N + 1 + threads - 1) / threads);
    hipLaunchKernelGGL((k_build_factors<float, float2>), dim3(blocks), dim3(threads), 0, ctx->stream, ctx->N, lap_dev, tab);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_solve(qf_ctx *ctx, const float2 *tab, const float2 *W, float2 *P, float scale, int skewh, qf_guard guard)
{
    return launch_solve<float>(ctx, tab, W, P, scale, skewh, guard, nullptr);
}

int qf_launch_laplace(qf_ctx *ctx, const float2 *P, float2 *W)
{
    const int N = ctx->N;
    dim3 block(256), grid((N + 255) / 256, N);
    hipLaunchKernelGGL((k_laplace<float, float2>), grid, block, 0, ctx->stream, N, P, W);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
