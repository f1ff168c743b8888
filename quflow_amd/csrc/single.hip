// complex64 data: the float32 arithmetic path of the stepper.
//
// Reference: complex64 input is computed in single precision throughout -- float32 coefficient tables and a
// float32 Thomas solve (quflow/laplacian/cpu.py:725, `dtype=type(W[0,0].real)`), complex64 np.matmul for the two
// products (quflow/integrators/isospectral.py:496,499), complex64 elementwise passes, and the automatic tolerance
// from the float32 machine epsilon (isospectral.py:440-448).  This file holds the float32 kernels that are not
// instantiations of the double-precision ones (poisson.hip instantiates the solve for float, elementwise.hip the end-of-step
// update, the infinity norm, the diagnostics' inner products and the skew-Hermitian check for float2):
//   * k_cgemm<TILE, EPI, EXACT, KS>: complex64 N x N x N product on the fp32 matrix cores (v_mfma_f32_32x32x2_f32 on
//     64 x 64 block tiles, 16x16x4 on 32 x 32: exact f32 fma chains at 64 flop/clk/SIMD = 157.3 TFLOP/s,
//     MI355X_MICROARCH.md), 3M form like the fp64 kernel.  EPI: the fused epilogue of the second product
//     (isospectral.py:499-509, 481-482, 526-534) and the fused step end, on 32 x 32 tiles only.  KS > 1: the plain product
//     with the K range cut between KS groups of wavefronts of one workgroup (launches with one tile per CU);
//   * k_cgemm_tri32: the second product on the upper triangle only (skew-Hermitian state), 32 x 32 tiles, K pieces per
//     tile exchanged through memory, the last arrival combines and runs the epilogue for the tile and its mirror image.
// The K loop (cg_k_loop) and the epilogue's arithmetic (cg_stage_pw_mirror, cg_epilogue_entry) are written once for all of them.
// The control plane is shared with the double-precision path: tagged launches, device-side exit decision on double row
// sums (in the second product's last tile, qf_step_end.h; k_norm_decide in the two-kernel protocol), progress record --
// see api_isomp.hip.
#include "qf_internal.h"
#include "qf_step_end.h"

#pragma clang fp contract(off)  // the epilogues' elementwise arithmetic is the reference's: not re-associated or fused

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

namespace {

// two neighbouring complex64 entries as one 16-byte load.  With an exact tiling (N a multiple of the tile) every such
// address is 16-byte aligned; on the guarded paths N may be odd, and then the entries of an odd row sit on 8-byte
// boundaries only -- the access is typed accordingly (a plain float4 dereference promises 16 to the compiler;
// global_load_dwordx4 itself takes any dword-aligned address).
// (ONE vector load with the alignment it really has.  A struct of four floats typed 8-byte aligned was tried first: the
// optimiser takes it apart into scalar loads and re-merges them with the single-entry load of the guard's other arm --
// two 8-byte loads per site where there was one 16-byte load, N = 1000 / 1500 at 0.84 of their round-3 rate,
// profiles/r04_size_sweep.jsonl.)
typedef float qf_v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));
template <bool ALIGNED16>
__device__ __forceinline__ float4 ld4(const float2 *p)
{
    if constexpr (ALIGNED16) return *reinterpret_cast<const float4 *>(p);
    else {
        const qf_v4f_a8 v = *reinterpret_cast<const qf_v4f_a8 *>(p);
        return make_float4(v[0], v[1], v[2], v[3]);
    }
}

// the entries (or zeros) at row gr, columns gc and gc + 1 of an N x N matrix, gc = c0 + c1: the guarded form of ld4.
// (The column comes in two parts, the tile's or K-tile's origin and the lane's offset, and both are added to the address
// in 64 bits: the uniform part then stays in scalar registers and the lane's part outside the K loop.)
template <bool EXACT>
__device__ __forceinline__ float4 ld4_guarded(const float2 *__restrict__ M, int N, int gr, int c0, int c1)
{
    const int gc = c0 + c1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EXACT || (gr < N && gc + 1 < N)) v = ld4<EXACT>(M + (size_t)gr * N + c0 + c1);
    else if (gr < N && gc < N) { const float2 t = M[(size_t)gr * N + c0 + c1]; v = make_float4(t.x, t.y, 0.f, 0.f); }
    return v;
}

// ---- block tiles.  A workgroup (or each of its K groups) is 4 wavefronts (2 x 2), one MF x MF MFMA tile each; K-tiles
// of CBK complex entries.  MFMA lane maps (cdna_hip_programming.md section 3), lm = lane % MF, lk = lane / MF:
// A[i = lm][k = lk], B[k = lk][j = lm], C/D[row = (reg & 3) + 8 (reg >> 2) + 4 lk][col = lm] -- f32 32x32x2: 16
// accumulator registers, two k per instruction; f32 16x16x4: 4 registers (row = 4 lk + reg), four k.
// The B image is row-major [CBK][BN] for both.  The two A images differ on purpose (a_at).
constexpr int CBK = 16;
template <int TILE> struct cg_tile;
template <> struct cg_tile<64> {
    typedef v16f acc;
    static constexpr int BM = 64, BN = 64, MF = 32, KM = 2, Q = 16;
    static constexpr int SA = BM + 1;             // k-major A image: row stride padded by one entry (transposing
                                                  // ds_write_b64 of 8 k-pairs x 2 rows: 16 distinct 8-byte slots)
    static constexpr int A_BYTES = CBK * SA * (int)sizeof(float2);
    static constexpr int B_BYTES = CBK * BN * (int)sizeof(float2);
    static constexpr int MAIN_BYTES = 2 * (A_BYTES + B_BYTES);      // double-buffered
    static __device__ __forceinline__ int a_at(int i, int k) { return k * SA + i; }
    static __device__ __forceinline__ acc mfma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
// below N = 768 a 64 x 64 tiling leaves most CUs without a workgroup (64 tiles at N = 512): 32 x 32 block tiles
// there, one 16 x 16 MFMA tile (v_mfma_f32_16x16x4_f32) per wavefront.  Its A image stays row-major with an odd
// row stride: the fragment read of lane (i = l & 15, k = l >> 4) then hits 32 distinct bank pairs per lane group
// (34 i mod 64 are sixteen distinct even banks, the k-neighbours sit two banks further), and so do the staging
// writes (rows r, r+1 x eight k-pairs).
template <> struct cg_tile<32> {
    typedef v4f acc;
    static constexpr int BM = 32, BN = 32, MF = 16, KM = 4, Q = 4;
    static constexpr int SAK = CBK + 1;           // row stride (complex entries) of the row-major A image
    static constexpr int A_BYTES = BM * SAK * (int)sizeof(float2);
    static constexpr int B_BYTES = CBK * BN * (int)sizeof(float2);
    static constexpr int MAIN_BYTES = 2 * (A_BYTES + B_BYTES);
    static constexpr int TT = BN + 1;             // row stride of the mirrored PW tile staged for the epilogue
    static constexpr int TT_BYTES = BM * TT * (int)sizeof(float2);
    static constexpr int EPI_BYTES = TT_BYTES + (2 * BM + 16) * (int)sizeof(double);      // + row sums [2][BM] + step end
    static __device__ __forceinline__ int a_at(int i, int k) { return i * SAK + k; }
    static __device__ __forceinline__ acc mfma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
typedef cg_tile<QF_C64_TILE> cg_small;            // the second product's tile
static_assert(cg_small::EPI_BYTES <= cg_small::MAIN_BYTES, "the square epilogue reuses the K loop's LDS");

__device__ __forceinline__ int xcd_remap(int bid, int nwg)
{
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// The K loop of every complex64 product: the 3M sums (T1 = sum ar br, T2 = sum ai bi, T3 = sum (ar+ai)(br+bi)) of tile
// (i0, j0) over the K-tiles kb .. kb + KTp - 1, run by the 256 threads of one K group on the group's LDS
// (cg_tile<TILE>::MAIN_BYTES at `smem`).  K-tiles double-buffered in LDS, two K-tiles in flight global -> registers.
// The barriers are the workgroup's: all K groups of one workgroup pass the same KTp.
// EXACT = false: loads guarded, out-of-range operands are zeros (they add nothing to the products).
// Staging maps: A rows tid / 8 (+ 32 for the second load of a 64-row tile), k-pair tid % 8;  B k-rows tid / (BN / 2)
// (+ 8 likewise), column pair tid % (BN / 2).
// (The accumulators are the loop's own and come back by value.  Taken by reference from the kernel, the MFMAs of the
// 32 x 32 kernels no longer accumulated in place -- the three accumulators rotated through eight more registers, 66-70
// VGPRs for 58-62, seven wavefronts per SIMD for eight.)
template <int TILE> struct cg_acc3 { typename cg_tile<TILE>::acc t1, t2, t3; };
template <int TILE, bool EXACT>
__device__ __forceinline__ cg_acc3<TILE> cg_k_loop(const float2 *__restrict__ A, const float2 *__restrict__ B, int N, int i0, int j0, int kb,
                                                   int KTp, unsigned char *smem)
{
    typedef cg_tile<TILE> T;
    typename T::acc t1, t2, t3;
#pragma unroll
    for (int q = 0; q < T::Q; ++q) { t1[q] = 0.f; t2[q] = 0.f; t3[q] = 0.f; }
    constexpr int R = TILE / 32;                  // 16-byte loads per thread, operand and K-tile
    constexpr int JP = T::BN / 2;                 // column pairs of a B row
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lm = lane % T::MF, lk = lane / T::MF;
    const int a_row = tid >> 3, a_kp = tid & 7;
    const int b_k = tid / JP, b_jp = tid % JP;
    float4 ra[2][R], rb[2][R];

    auto load_tile = [&](int kt, float4 (&a)[R], float4 (&b)[R]) __attribute__((always_inline)) {
        const int k0 = (kb + kt) * CBK;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = ld4_guarded<EXACT>(A, N, i0 + a_row + 32 * r, k0, 2 * a_kp);
            b[r] = ld4_guarded<EXACT>(B, N, k0 + b_k + (256 / JP) * r, j0, 2 * b_jp);
        }
    };
    auto store_tile = [&](int buf, const float4 (&a)[R], const float4 (&b)[R]) __attribute__((always_inline)) {
        float2 *As = reinterpret_cast<float2 *>(smem + buf * T::A_BYTES);
        float2 *Bs = reinterpret_cast<float2 *>(smem + 2 * T::A_BYTES + buf * T::B_BYTES);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            As[T::a_at(a_row + 32 * r, 2 * a_kp)] = make_float2(a[r].x, a[r].y);
            As[T::a_at(a_row + 32 * r, 2 * a_kp + 1)] = make_float2(a[r].z, a[r].w);
            *reinterpret_cast<float4 *>(Bs + (b_k + (256 / JP) * r) * T::BN + 2 * b_jp) = b[r];
        }
    };
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const float2 *As = reinterpret_cast<const float2 *>(smem + buf * T::A_BYTES) + T::a_at(wm * T::MF + lm, lk);
        const float2 *Bs = reinterpret_cast<const float2 *>(smem + 2 * T::A_BYTES + buf * T::B_BYTES) + lk * T::BN + wn * T::MF + lm;
#pragma unroll
        for (int s = 0; s < CBK / T::KM; ++s) {
            const float2 a = As[T::a_at(0, T::KM * s)];
            const float2 b = Bs[T::KM * s * T::BN];
            t1 = T::mfma(a.x, b.x, t1);
            t2 = T::mfma(a.y, b.y, t2);
            t3 = T::mfma(a.x + a.y, b.x + b.y, t3);
        }
    };

    load_tile(0, ra[0], rb[0]);
    if (KTp > 1) load_tile(1, ra[1], rb[1]);
    store_tile(0, ra[0], rb[0]);
    __syncthreads();
    if (KTp > 2) load_tile(2, ra[0], rb[0]);
    int kt = 0;
    // two K-tiles per trip: LDS buffer and register-set indices are literals.  (Staging K-tile kt+1 and issuing
    // the loads of kt+3 AHEAD of K-tile kt's MFMAs instead of behind them measured slower: 81.9 against 78.5 us
    // at N=1024, 456 against 437 at N=2048 -- the waves then meet the LDS store path all at once.)
    for (; kt + 1 < KTp; kt += 2) {
        compute(0);
        store_tile(1, ra[1], rb[1]);                       // K-tile kt+1 (arrived two K-tiles ago)
        if (kt + 3 < KTp) load_tile(kt + 3, ra[1], rb[1]);
        __syncthreads();
        compute(1);
        if (kt + 2 < KTp) {
            store_tile(0, ra[0], rb[0]);
            if (kt + 4 < KTp) load_tile(kt + 4, ra[0], rb[0]);
        }
        __syncthreads();
    }
    if (kt < KTp) compute(0);
    return {t1, t2, t3};
}

// ---- the second product's epilogue (32 x 32 tiles), shared by the full and the upper-triangle kernel.
// The mirrored PW tile (rows j0.., columns i0..) goes through LDS (Tt[BN][TT]) so that both global reads of PW are
// row-coalesced; conj_subtract_ (isospectral.py:71-74) needs PW[i,j] - conj(PW[j,i]).
template <bool EXACT>
__device__ __forceinline__ void cg_stage_pw_mirror(const float2 *__restrict__ PW, int N, int i0, int j0, int tid, float2 *Tt)
{
    typedef cg_small T;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = (tid >> 4) + 16 * r, cp = tid & 15;
        const float4 v = ld4_guarded<EXACT>(PW, N, j0 + row, i0, 2 * cp);
        Tt[row * T::TT + 2 * cp] = make_float2(v.x, v.y);
        Tt[row * T::TT + 2 * cp + 1] = make_float2(v.z, v.w);
    }
}

// One entry: pw = PW[i,j], pwt = PW[j,i], (re, im) = (PW @ Phalf)[i,j], w = W[i,j], o = dW_old[i,j].  Returns |dW_old - dW|.
__device__ __forceinline__ float cg_epilogue_entry(float2 pw, float2 pwt, float re, float im, float2 w, float2 o, float2 &dv, float2 &whv,
                                                   float2 &wnv, float2 &whs)
{
    const float cr = pw.x - pwt.x, ci = pw.y + pwt.y;
    const float dr = re + cr, di = im + ci;                      // dW = (PW @ Phalf) + comm   (:499,509)
    dv = make_float2(dr, di);
    whv = make_float2(w.x + dr, w.y + di);                       // Whalf = W + dW             (:481-482)
    // should this be the step's last iteration: W_next = W + 2 comm (:547,592), next Whalf = W_next + dW
    const float wr = w.x + 2.0f * cr, wi = w.y + 2.0f * ci;
    wnv = make_float2(wr, wi);
    whs = make_float2(wr + dr, wi + di);
    const float er = o.x - dr, ei = o.y - di;                    // |dW_old - dW|              (:526,534)
    return sqrtf(er * er + ei * ei);
}

// C = A @ B (EPI = false) or the second product with its fused epilogue (EPI = true):
//   dW_new = A @ B + (PW - PW^H);  Whalf = W + dW_new;  rowpart[tile column][i] = sum_j |dW_old - dW_new|
// KS > 1, the plain product with the K range of a tile cut into KS parts INSIDE the workgroup: KS groups of four
// wavefronts, each with its own LDS buffers and its own 1/KS of the K-tiles, partial tiles added in group order at the end.
// Why: at N = 1024 a launch is one 64 x 64 tile per CU, i.e. one wavefront per SIMD, and the fp32 matrix pipe idles
// while that wavefront waits for its LDS reads and barriers -- the same kernel reaches 0.81 of the peak at N = 2048,
// where four workgroups share a CU, against 0.59 at N = 1024.  More wavefronts per SIMD on the SAME tile give the
// scheduler that choice without a second tile.  (N % (16 KS) == 0: every group runs the same number of barriers.)
// Instantiated (qf_launch_cgemm): <32, false, true, 1 / 2 / 4>, <32, false, false, 1>, <32, true, true / false, 1>,
// <64, false, true, 1 / 2 / 4>.  The second product lives on 32 x 32 tiles only: its 64 x 64 form lost at every size.
template <int TILE, bool EPI, bool EXACT, int KS>
__global__ __launch_bounds__(256 * KS) void k_cgemm(int N, int tiles_n, const float2 *__restrict__ A, const float2 *__restrict__ B,
                                                    float2 *__restrict__ C, qf_epilogue_f ep, qf_guard guard)
{
    typedef cg_tile<TILE> T;
    static_assert(!EPI || TILE == QF_C64_TILE, "the second product lives on 32 x 32 tiles");
    static_assert(KS == 1 || (!EPI && EXACT), "K groups: plain product on an exact tiling");
    static_assert(TILE == 32 || EXACT, "64 x 64 tiles: exact tilings only");
    static_assert((KS - 1) * T::Q * 256 * (int)sizeof(float2) <= KS * T::MAIN_BYTES, "the groups' partial tiles fit the K loop's LDS");
    if (!qf_guard_iter(guard)) return;
    // fused step end: the first product of a step's first iteration takes the Whalf prepared for it
    if (!EPI && guard.alt && guard.state->wh_sel) B = static_cast<const float2 *>(guard.alt);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int grp = KS > 1 ? (int)(threadIdx.x >> 8) : 0;
    unsigned char *const smem = KS > 1 ? smem_all + grp * T::MAIN_BYTES : smem_all;
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lm = lane % T::MF, lk = lane / T::MF;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = lid / tiles_n, tn = lid % tiles_n;
    const int i0 = tm * T::BM, j0 = tn * T::BN;

    const int KT = ((N + CBK - 1) / CBK) / KS;             // this group's K-tiles: grp KT .. grp KT + KT - 1
    const cg_acc3<TILE> acc = cg_k_loop<TILE, EXACT>(A, B, N, i0, j0, grp * KT, KT, smem);
    const typename T::acc t1 = acc.t1, t2 = acc.t2, t3 = acc.t3;

    if constexpr (!EPI) {
        // the groups' partial tiles through LDS ([group - 1][q][thread]: conflict-free), added in group order
        float2 *X = reinterpret_cast<float2 *>(smem_all);
        if constexpr (KS > 1) {
            __syncthreads();
            if (grp > 0) {
#pragma unroll
                for (int q = 0; q < T::Q; ++q) X[((grp - 1) * T::Q + q) * 256 + tid] = make_float2(t1[q] - t2[q], (t3[q] - t1[q]) - t2[q]);
            }
            __syncthreads();
            if (grp > 0) return;
        }
#pragma unroll
        for (int q = 0; q < T::Q; ++q) {
            const int gi = i0 + wm * T::MF + (q & 3) + 8 * (q >> 2) + 4 * lk;
            const int gj = j0 + wn * T::MF + lm;
            float re = t1[q] - t2[q], im = (t3[q] - t1[q]) - t2[q];
            if constexpr (KS > 1) {
#pragma unroll
                for (int g = 1; g < KS; ++g) {
                    const float2 v = X[((g - 1) * T::Q + q) * 256 + tid];
                    re += v.x;
                    im += v.y;
                }
            }
            if (EXACT || (gi < N && gj < N)) C[(size_t)gi * N + gj] = make_float2(re, im);
        }
    } else {
        const int parity = guard.state ? guard.state->dw_parity : 0;
        const float2 *__restrict__ dW_old = ep.dW[parity];
        float2 *__restrict__ dW_new = ep.dW[parity ^ 1];
        // fused step end: the state is Wpair[w_parity]; the candidate next state goes to the other buffer
        const int wpar = (ep.fused && guard.state) ? guard.state->w_parity : 0;
        const float2 *__restrict__ ep_W = ep.fused ? ep.Wpair[wpar] : ep.W;
        float2 *__restrict__ ep_Wnext = ep.fused ? ep.Wpair[wpar ^ 1] : nullptr;
        __syncthreads();      // every wave is done with the K-loop buffers
        float2 *Tt = reinterpret_cast<float2 *>(smem);
        double *rs = reinterpret_cast<double *>(smem + T::TT_BYTES);   // [2][BM]
        cg_stage_pw_mirror<EXACT>(ep.PW, N, i0, j0, tid, Tt);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < T::Q; ++q) {
            const int li = wm * T::MF + 4 * lk + q;
            const int lj = wn * T::MF + lm;
            const int gi = i0 + li, gj = j0 + lj;
            float a = 0.f;
            if (EXACT || (gi < N && gj < N)) {
                const size_t e = (size_t)gi * N + gj;
                float2 dv, whv, wnv, whs;
                a = cg_epilogue_entry(ep.PW[e], Tt[lj * T::TT + li], t1[q] - t2[q], (t3[q] - t1[q]) - t2[q], ep_W[e], dW_old[e], dv, whv, wnv, whs);
                dW_new[e] = dv;
                ep.Whalf[e] = whv;
                if (ep.fused) {
                    ep_Wnext[e] = wnv;
                    ep.Whalf_step[e] = whs;
                }
            }
            // sum over the 16 lanes that share this row (fixed butterfly: deterministic), in double
            double rsum = (double)a;
            rsum = qf_row16_sum(rsum);      // (xor butterfly 1, 2, 4, 8 on DPP: same tree, same bits as four __shfl_xor steps)
            if (lm == 0) rs[wn * T::BM + li] = rsum;
        }
        __syncthreads();
        if (tid < T::BM && (EXACT || i0 + tid < N)) {
            const double v = rs[tid] + rs[T::BM + tid];
            if (ep.fused) __hip_atomic_store(ep.rowpart + (size_t)tn * N + i0 + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else ep.rowpart[(size_t)tn * N + i0 + tid] = v;
        }
        if (ep.fused) {
            // the last tile to get here closes the iteration (ticket: guide section 6 G16, counter form)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            unsigned *last_flag = reinterpret_cast<unsigned *>(rs + 2 * T::BM);
            if (tid == 0) {
                const unsigned old = __hip_atomic_fetch_add(ep.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *last_flag = (old == (unsigned)(ep.n_tiles - 1)) ? 1u : 0u;
            }
            __syncthreads();
            if (*last_flag != 0u)
                qf_fused_step_end<1>(N, tiles_n, ep.rowpart, ep.ticket, ep.state_rw, ep.rec, guard.iter, tid, rs + 2 * T::BM + 2);
        }
    }
}

// ---- the second product on the upper triangle (complex64) ----
// With Phalf and Whalf skew-Hermitian, dW = PW @ Phalf + (PW - PW^H) is skew-Hermitian: only the nt (nt + 1) / 2 tiles
// on and above the diagonal are multiplied, and the finishing workgroup writes the tile of Whalf AND its mirror image
// -conj(.)^T (DESIGN.md 3.1b / 3.1c for the double-precision kernels).  At N = 1024 that is 136 tiles for 256 CUs, so
// the K range of every tile is cut into `split` pieces, one workgroup each (k_zgemm_tri32's exchange): a workgroup
// parks its partial tile (write-through), drains, takes a ticket on the tile's arrival counter and leaves unless it
// came last; the last arrival adds ALL pieces from memory in piece order (its own included: the same bits whoever is
// last) and runs the epilogue.  Nobody waits; the counters are monotone (`split` arrivals per executed launch).
// Below the diagonal only Whalf is written (the next first product's right operand): W and dW are read back on and
// above the diagonal tiles only and restored once at the end of a call (k_mirror_lower<float2>, elementwise.hip).
// On 32 x 32 tiles (any N >= 64; edge tiles guarded): one 16 x 16 MFMA tile per wavefront.  Partial tiles are 8 KiB, the
// epilogue's LDS 18 KiB: many workgroups share a CU.  (A 64 x 64-tile form of this kernel existed in rounds 3-4: slower
// at every size -- N = 1024 71.6 against 59.2 us, N = 2048 320 against 299 -- removed in round 5.)
typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
constexpr int SBM = cg_small::BM, SBN = cg_small::BN, STT = cg_small::TT;
constexpr int ST_TILE_BYTES = cg_small::TT_BYTES;
constexpr int ST_EPI_BYTES = 2 * ST_TILE_BYTES + (4 * SBM + 16) * (int)sizeof(double);
constexpr int ST_SMEM = cg_small::MAIN_BYTES > ST_EPI_BYTES ? cg_small::MAIN_BYTES : ST_EPI_BYTES;

// EXACT = false: N is no multiple of 32 -- nt = ceil(N / 32) tile rows, loads, stores and row sums of the edge tiles guarded
// (out-of-range operands are zeros: they add nothing to the products), K-tiles = ceil(N / 16).
template <bool EXACT>
__global__ __launch_bounds__(256) void k_cgemm_tri32(int N, int nt, const float2 *__restrict__ A, const float2 *__restrict__ B,
                                                     qf_epilogue_f ep, qf_guard guard, qf_ctri sx)
{
    if (!qf_guard_iter(guard)) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, lq = lane >> 4;
    const int nd_pieces = nt * sx.split_diag, noff = nt * (nt - 1) / 2;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn, h, S, t;
    if (lid < nd_pieces) {
        tm = tn = lid / sx.split_diag;
        h = lid % sx.split_diag;
        S = sx.split_diag;
        t = tm;
    } else {
        const int o2 = lid - nd_pieces;
        int o = o2 % noff;
        h = o2 / noff;
        S = sx.split;
        t = nt + o;
        tm = 0;
        int rowlen = nt - 1;
        while (o >= rowlen) {
            o -= rowlen;
            ++tm;
            --rowlen;
        }
        tn = tm + 1 + o;
    }
    const int i0 = tm * SBM, j0 = tn * SBN;
    const bool offdiag = (tm != tn);
    const int parity = guard.state ? guard.state->dw_parity : 0;
    const float2 *__restrict__ dW_old = ep.dW[parity];
    float2 *__restrict__ dW_new = ep.dW[parity ^ 1];
    const int wpar = (ep.fused && guard.state) ? guard.state->w_parity : 0;
    const float2 *__restrict__ ep_W = ep.fused ? ep.Wpair[wpar] : ep.W;
    float2 *__restrict__ ep_Wnext = ep.fused ? ep.Wpair[wpar ^ 1] : nullptr;

    // this piece's K-tiles: kb .. kb + KTp - 1 (N % 32 == 0 makes the K-tile count even, not a multiple of 4: the pieces
    // of a tile may differ by one K-tile)
    const int KTN = (N + CBK - 1) / CBK;
    const int kb = (int)((long long)KTN * h / S), KTp = (int)((long long)KTN * (h + 1) / S) - kb;
    const cg_acc3<QF_C64_TILE> acc = cg_k_loop<QF_C64_TILE, EXACT>(A, B, N, i0, j0, kb, KTp, smem);
    const v4f t1 = acc.t1, t2 = acc.t2, t3 = acc.t3;

    float re[4], im[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        re[q] = t1[q] - t2[q];
        im[q] = (t3[q] - t1[q]) - t2[q];
    }
    unsigned *flagw = reinterpret_cast<unsigned *>(smem + 2 * ST_TILE_BYTES + 4 * SBM * sizeof(double));
    if (S > 1) {
        const __amdgpu_buffer_rsrc_t rsrcP = __builtin_amdgcn_make_buffer_rsrc(sx.partial, 0, 0x7fffffff, 0x00020000);
        const unsigned p_voff = (unsigned)(tid * sizeof(float2));
        const unsigned slot_bytes = (unsigned)(SBM * SBN * sizeof(float2));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float2 v = make_float2(re[q], im[q]);
            __builtin_amdgcn_raw_buffer_store_b64(*reinterpret_cast<const v2u_t *>(&v), rsrcP, p_voff + (unsigned)(q * 256 * sizeof(float2)),
                                                  (unsigned)(4 * t + h) * slot_bytes, 16);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const unsigned old = __hip_atomic_fetch_add(sx.arrive + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flagw = ((old % (unsigned)S) == (unsigned)(S - 1)) ? 1u : 0u;
        }
        __syncthreads();
        if (*flagw == 0u) return;
#pragma unroll 1
        for (int hh = 0; hh < S; ++hh) {
            float2 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v2u_t raw = __builtin_amdgcn_raw_buffer_load_b64(rsrcP, p_voff + (unsigned)(q * 256 * sizeof(float2)),
                                                                       (unsigned)(4 * t + hh) * slot_bytes, 16);
                v[q] = *reinterpret_cast<const float2 *>(&raw);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                re[q] = hh == 0 ? v[q].x : re[q] + v[q].x;
                im[q] = hh == 0 ? v[q].y : im[q] + v[q].y;
            }
        }
    }

    __syncthreads();
    float2 *Tt = reinterpret_cast<float2 *>(smem);
    float2 *Th = reinterpret_cast<float2 *>(smem + ST_TILE_BYTES);
    double *rs = reinterpret_cast<double *>(smem + 2 * ST_TILE_BYTES);   // [2][32] row sums
    double *cs = rs + 2 * SBM;                                           // [2][32] column sums
    cg_stage_pw_mirror<EXACT>(ep.PW, N, i0, j0, tid, Tt);
    __syncthreads();
    float2 dv[4], whv[4], wnv[4], whs[4];
    double csum = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int li = wm * 16 + 4 * lq + q;
        const int lj = wn * 16 + l15;
        const size_t e = (size_t)(i0 + li) * N + (j0 + lj);
        const bool in = EXACT || (i0 + li < N && j0 + lj < N);
        double a = 0.0;
        dv[q] = whv[q] = wnv[q] = whs[q] = make_float2(0.f, 0.f);
        if (in) a = (double)cg_epilogue_entry(ep.PW[e], Tt[lj * STT + li], re[q], im[q], ep_W[e], dW_old[e], dv[q], whv[q], wnv[q], whs[q]);
        csum += a;
        double rsum = a;
        rsum = qf_row16_sum(rsum);      // (xor butterfly 1, 2, 4, 8 on DPP: same tree, same bits as four __shfl_xor steps)
        if (l15 == 0) rs[wn * SBM + li] = rsum;
    }
    csum += __shfl_xor(csum, 16, 64);     // the four lane groups hold rows 4 lq .. 4 lq + 3 of this column
    csum += __shfl_xor(csum, 32, 64);
    if (lq == 0) cs[wm * SBN + wn * 16 + l15] = csum;
    __syncthreads();
    if (tid < SBM) {
        if (EXACT || i0 + tid < N)
            __hip_atomic_store(ep.rowpart + (size_t)tn * N + i0 + tid, rs[tid] + rs[SBM + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (offdiag && tid >= 64 && tid < 64 + SBN) {
        const int lj = tid - 64;
        if (EXACT || j0 + lj < N)
            __hip_atomic_store(ep.rowpart + (size_t)tm * N + j0 + lj, cs[lj] + cs[SBN + lj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned ticket_old = 0u;
    if (ep.fused) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) ticket_old = __hip_atomic_fetch_add(ep.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int li = wm * 16 + 4 * lq + q;
        const int lj = wn * 16 + l15;
        const size_t e = (size_t)(i0 + li) * N + (j0 + lj);
        const bool in = EXACT || (i0 + li < N && j0 + lj < N);
        if (in) {
            dW_new[e] = dv[q];
            ep.Whalf[e] = whv[q];
        }
        Th[li * STT + lj] = whv[q];
        if (ep.fused) {
            if (in) {
                ep_Wnext[e] = wnv[q];
                ep.Whalf_step[e] = whs[q];
            }
            Tt[li * STT + lj] = whs[q];
        }
    }
    __syncthreads();
    if (offdiag) {
        // row j0 + jl of the mirrored tile is column jl of this one (32 entries = 256 bytes): two per wave instruction
        const int il = lane & 31;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jl = wave * 8 + r * 2 + (lane >> 5);
            if (!EXACT && (j0 + jl >= N || i0 + il >= N)) continue;
            const float2 wv = Th[il * STT + jl];
            ep.Whalf[(size_t)(j0 + jl) * N + i0 + il] = make_float2(-wv.x, wv.y);
            if (ep.fused) {
                const float2 ws = Tt[il * STT + jl];
                ep.Whalf_step[(size_t)(j0 + jl) * N + i0 + il] = make_float2(-ws.x, ws.y);
            }
        }
    }
    if (ep.fused) {
        __syncthreads();
        unsigned *last_flag = reinterpret_cast<unsigned *>(rs);
        if (tid == 0) *last_flag = (ticket_old == (unsigned)(ep.n_tiles - 1)) ? 1u : 0u;
        __syncthreads();
        if (*last_flag != 0u) qf_fused_step_end<1>(N, nt, ep.rowpart, ep.ticket, ep.state_rw, ep.rec, guard.iter, tid, rs + 2);
    }
}

}  // namespace

// Tile sizes of the complex64 products.  The 32 x 32 kernels are small (17-18 KiB of LDS, about 60 registers): several
// workgroups share a CU, so they neither leave CUs idle when the tile count is no multiple of 256 nor need N % 64 == 0.
// Measured (bench.py --dtype c64, timesteps/s, all products on 64 x 64 / on 32 x 32 tiles): N = 768 9,698 / 12,315; 832
// 9,275 / 11,092; 896 8,856 / 9,232; 960 8,391 / 8,434; 1024 7,216 / 7,757; 1056 3,016 / 6,475 (64 x 64: generic path);
// 1088 4,644 / 6,144; 1152 4,438 / 5,332; 1280 4,058 / 4,307; 1536 2,461 / 2,922; 1792 1,651 / 1,873; 2048 1,339 / 1,328.
// By kernel: the SECOND product (triangle, exchange, epilogue) is faster on 32 x 32 tiles at every size (N = 1024 59.2
// against 71.6 us, N = 2048 299 against 320); the plain FIRST product is faster on 64 x 64 tiles where those fill the
// chip (us, 64 / 32: N = 896 52.3 / 54.2, 960 56.1 / 58.2, 1024 59.0 / 61.8, 2048 402 / 433) and slower elsewhere (768
// 46.1 / 38.5, 1088 113 / 78, 1280 132 / 124, 1536 230 / 188, 1792 348 / 305).
// (No exact tiling: guarded 32 x 32 kernels -- N = 1000 3,586 -> 5,922 timesteps/s against the generic 64 x 64 path, N = 900
// 3,907 -> 6,406, N = 1500 1,666 -> 2,180.)
// Rules: second product 32 x 32 at every N (QF_C64_TILE);
// first product 64 x 64 for N % 64 == 0 with 896 <= N <= 1024 or, from N = 2048 on, tiles filling >= 85 % of their rounds.
int qf_c64_tile_first(const qf_ctx *ctx)
{
    const int N = ctx->N;
    if (N % 64 != 0) return 32;
    if (N >= 896 && N <= 1024) return 64;
    if (N >= 2048) {
        const long long tiles = (long long)(N / 64) * (N / 64), rounds = (tiles + 255) / 256;
        return tiles * 100 >= rounds * 256 * 85 ? 64 : 32;
    }
    return 32;
}

int qf_c64_alloc(qf_ctx *ctx)
{
    if (ctx->c64) return QF_OK;
    const int N = ctx->N;
    const size_t NN = (size_t)N * N, mbytes = NN * sizeof(float2);
    qf_c64 *f = new qf_c64();
    float2 **mats[] = {&f->W, &f->dW[0], &f->dW[1], &f->Whalf, &f->Phalf, &f->PW, &f->stage};
    for (float2 **m : mats) {
        if (hipMalloc((void **)m, mbytes) != hipSuccess || hipMemsetAsync(*m, 0, mbytes, ctx->stream) != hipSuccess) {
            qf_set_error("qf_c64_alloc: out of device memory (N=%d)", N);
            qf_c64_free(f);
            return QF_ERR_HIP;
        }
    }
    if (hipMalloc((void **)&f->lap, 2 * NN * sizeof(float)) != hipSuccess || hipMalloc((void **)&f->tab, mbytes) != hipSuccess) {
        qf_set_error("qf_c64_alloc: out of device memory (N=%d)", N);
        qf_c64_free(f);
        return QF_ERR_HIP;
    }
    f->rowpart_tiles = (N + QF_C64_TILE - 1) / QF_C64_TILE;     // column tiles of the second product
    if (hipMalloc((void **)&f->rowpart, (size_t)f->rowpart_tiles * N * sizeof(double)) != hipSuccess) {
        qf_set_error("qf_c64_alloc: out of device memory (N=%d)", N);
        qf_c64_free(f);
        return QF_ERR_HIP;
    }
    ctx->c64 = f;
    // float32 coefficient table (bc = True) and its factorisation, once per N (cpu.py:725)
    QF_TRY(qf_launch_lap_table(ctx, 1, f->lap));
    QF_TRY(qf_launch_build_factors(ctx, f->lap, f->tab));
    return QF_OK;
}

void qf_c64_free(qf_c64 *f)
{
    if (!f) return;
    void *ptrs[] = {f->W, f->dW[0], f->dW[1], f->Whalf, f->Phalf, f->PW, f->stage, f->kahan_c, f->lap, f->tab, f->rowpart, f->W2,
                    f->Whalf2, f->tri_partial, f->tri_arrive};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete f;
}

// qf_plan_describe: what a complex64 product launcher launches (the role is the caller's open prof_scope)
static void note_c64(qf_ctx *ctx, const char *kernel, int tile, int tiles, int grid_tiles, int wgs, int threads, const char *mfma,
                     const char *step_end)
{
    unsigned long long key = 0x7000000ull ^ ((unsigned long long)tile << 20) ^ ((unsigned long long)wgs << 8) ^ (unsigned long long)threads;
    for (const char *c = kernel; *c; ++c) key = key * 131ull + (unsigned char)*c;
    qf_plan_note(ctx, key | 1ull,
                 "{\"kernel\": \"%s\", \"arithmetic\": \"fp32 3M, %s\", \"tile\": [%d, %d], \"tiles\": %d, \"tile_share\": %.6f, "
                 "\"workgroups\": %d, \"threads\": %d, \"step_end\": \"%s\"}",
                 kernel, mfma, tile, tile, tiles, (double)tiles / (double)grid_tiles, wgs, threads, step_end);
}

// one square product: KS groups of 256 threads per tile, each with the K loop's LDS (a request above 64 KiB needs the
// dynamic-LDS limit of the kernel raised first: qf_smem_attr_set does that, once per instantiation and device)
template <int TILE, bool EPI, bool EXACT, int KS>
static int launch_cgemm(qf_ctx *ctx, int tiles_n, const float2 *A, const float2 *B, float2 *C, const qf_epilogue_f &ep, qf_guard guard)
{
    constexpr int smem = KS * cg_tile<TILE>::MAIN_BYTES;
    static qf_smem_attr attr;
    QF_TRY(qf_smem_attr_set(attr, (const void *)k_cgemm<TILE, EPI, EXACT, KS>, ctx->device, smem));
    hipLaunchKernelGGL((k_cgemm<TILE, EPI, EXACT, KS>), dim3(tiles_n * tiles_n), dim3(256 * KS), smem, ctx->stream, ctx->N, tiles_n, A, B, C, ep,
                       guard);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
template <int TILE>
static int launch_cgemm_plain(qf_ctx *ctx, int ks, int tiles_n, const float2 *A, const float2 *B, float2 *C, qf_guard guard)
{
    const qf_epilogue_f none;
    return ks == 4   ? launch_cgemm<TILE, false, true, 4>(ctx, tiles_n, A, B, C, none, guard)
           : ks == 2 ? launch_cgemm<TILE, false, true, 2>(ctx, tiles_n, A, B, C, none, guard)
                     : launch_cgemm<TILE, false, true, 1>(ctx, tiles_n, A, B, C, none, guard);
}

int qf_launch_cgemm(qf_ctx *ctx, const float2 *A, const float2 *B, float2 *C, const qf_epilogue_f *ep_in, qf_guard guard)
{
    const int N = ctx->N;
    const int tile = ep_in ? QF_C64_TILE : qf_c64_tile_first(ctx);      // (64 x 64: only for N % 64 == 0)
    const int nt = (N + tile - 1) / tile, tiles = nt * nt;
    const bool exact = N % tile == 0;
    // plain product on an exact tiling with two tiles per CU or fewer: K groups, more wavefronts per SIMD on the same tile
    // (every group takes an even number of K-tiles)
    int ks = 1;
    if (!ep_in && exact) {
        const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
        ks = tiles <= cus ? 4 : tiles <= 2 * cus ? 2 : 1;
        while (ks > 1 && (N / CBK) % (2 * ks) != 0) ks >>= 1;
    }
    const char *name = tile == 32 ? (ks == 4   ? "k_cgemm32<plain, 4 K groups>"
                                     : ks == 2 ? "k_cgemm32<plain, 2 K groups>"
                                     : ep_in   ? "k_cgemm32<EPI>"
                                               : "k_cgemm32<plain>")
                                  : (ks == 4 ? "k_cgemm_ks<4>" : ks == 2 ? "k_cgemm_ks<2>" : "k_cgemm<plain>");
    note_c64(ctx, name, tile, tiles, tiles, tiles, 256 * ks, tile == 32 ? "v_mfma_f32_16x16x4_f32" : "v_mfma_f32_32x32x2_f32",
             !ep_in ? "none" : ep_in->fused ? "fused (last tile decides)" : "two-kernel");
    if (ep_in) {
        qf_epilogue_f ep = *ep_in;
        if (ep.fused) {     // tile ticket + what the last tile's workgroup updates
            ep.ticket = ctx->ticket + 403;
            ep.n_tiles = tiles;
            ep.state_rw = ctx->state;
            ep.rec = ctx->host_rec;
        }
        return exact ? launch_cgemm<QF_C64_TILE, true, true, 1>(ctx, nt, A, B, C, ep, guard)
                     : launch_cgemm<QF_C64_TILE, true, false, 1>(ctx, nt, A, B, C, ep, guard);
    }
    if (!exact) return launch_cgemm<32, false, false, 1>(ctx, nt, A, B, C, qf_epilogue_f(), guard);
    return tile == 32 ? launch_cgemm_plain<32>(ctx, ks, nt, A, B, C, guard) : launch_cgemm_plain<64>(ctx, ks, nt, A, B, C, guard);
}

int qf_c64_tri_alloc(qf_ctx *ctx)
{
    qf_c64 *f = ctx->c64;
    const int tb = QF_C64_TILE;
    if (!f || ctx->N < 64) {
        qf_set_error("qf_c64_tri_alloc: the upper-triangle product needs N >= 64 (N=%d)", ctx->N);
        return QF_ERR_INVALID;
    }
    if (f->tri_arrive) return QF_OK;
    const int nt = (ctx->N + tb - 1) / tb;
    const size_t tiles = (size_t)nt * (nt + 1) / 2;
    // K pieces per off-diagonal / diagonal tile.  A workgroup is small (18 KiB of LDS, 62 registers), several share a CU
    // and the pieces of a tile spread over them.  Measured (timesteps/s; full product / pieces 1,1 / 2,2 / 4,4 / 4,2):
    // N = 512 20,175 / 21,603 / 22,982 / 23,663 / 23,753; N = 704 12,498 / 14,331 / 15,224 / 15,415 / 14,759; N = 256
    // 30,769 / 32,017 / 32,632 / 33,249 / 33,335.
    f->tri_split = 4;
    f->tri_split_diag = 4;
    // (a piece must be at least two K-tiles of 16)
    while (f->tri_split > 1 && (ctx->N + CBK - 1) / CBK / f->tri_split < 2) f->tri_split >>= 1;
    while (f->tri_split_diag > 1 && (ctx->N + CBK - 1) / CBK / f->tri_split_diag < 2) f->tri_split_diag >>= 1;
    QF_HIP(hipMalloc((void **)&f->tri_partial, tiles * 4 * tb * tb * sizeof(float2)));
    QF_HIP(hipMalloc((void **)&f->tri_arrive, tiles * sizeof(unsigned)));
    f->tri_arrive_count = tiles;
    QF_HIP(hipMemsetAsync(f->tri_arrive, 0, tiles * sizeof(unsigned), ctx->stream));
    return QF_OK;
}

int qf_launch_cgemm_tri(qf_ctx *ctx, const float2 *A, const float2 *B, const qf_epilogue_f *ep_in, qf_guard guard)
{
    const int N = ctx->N;
    qf_c64 *f = ctx->c64;
    if (!ep_in || !f || !f->tri_arrive) {
        qf_set_error("qf_launch_cgemm_tri: not available for this context (N=%d)", N);
        return QF_ERR_STATE;
    }
    const int nt = (N + SBM - 1) / SBM;
    qf_epilogue_f ep = *ep_in;
    if (ep.fused) {     // tile ticket + what the last tile's workgroup updates
        ep.ticket = ctx->ticket + 404;
        ep.n_tiles = nt * (nt + 1) / 2;
        ep.state_rw = ctx->state;
        ep.rec = ctx->host_rec;
    }
    qf_ctri sx;
    sx.partial = f->tri_partial;
    sx.arrive = f->tri_arrive;
    sx.split = f->tri_split;
    sx.split_diag = f->tri_split_diag;
    const int grid = nt * sx.split_diag + nt * (nt - 1) / 2 * sx.split;
    note_c64(ctx, "k_cgemm_tri32 (upper triangle, K pieces per tile)", SBM, nt * (nt + 1) / 2, nt * nt, grid, 256, "v_mfma_f32_16x16x4_f32",
             ep.fused ? "fused (last tile decides)" : "two-kernel");
    if (N % SBM == 0) hipLaunchKernelGGL(k_cgemm_tri32<true>, dim3(grid), dim3(256), ST_SMEM, ctx->stream, N, nt, A, B, ep, guard, sx);
    else hipLaunchKernelGGL(k_cgemm_tri32<false>, dim3(grid), dim3(256), ST_SMEM, ctx->stream, N, nt, A, B, ep, guard, sx);
    QF_HIP(hipGetLastError());
    return QF_OK;
}
