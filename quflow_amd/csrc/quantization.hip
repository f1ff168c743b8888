// Spherical-harmonics <-> matrix transforms (quflow/quantization.py:116-396): for every
// diagonal offset m the m-th diagonal of W and the coefficients omega[(el, +-m)], el >= m, are
// related by the dense real (N-m) x (N-m) block B_m of the quantization basis,
//      shr2mat_/shc2mat_ :  diag_m = B_m @ x_m          (quantization.py:188-245, 331-365)
//      mat2shr_/mat2shc_ :  z_m    = diag_m @ B_m       (quantization.py:286-327, 368-396)
// i.e. one sweep over the N^3/3-entry basis (2.9 GB at N=1024) per transform: HBM-bound.
// The basis lives in HBM for the life of the context (qf_basis_upload), or -- the streamed form, qf_basis_stream, for
// the N where it cannot (183 GB at N=4096) -- it is not stored at all: every call rebuilds the blocks m < Nmax, columns
// j < Nmax - m, into a bounded slab (k_basis_slab, the same column arithmetic as k_basis) and applies them there with
// the slab instantiations of the two main kernels, slab after slab (whole blocks in m order, qf_slab_plan).
//
// Layouts.  omega is indexed el^2 + el + m (quflow/utils.py:91-105): for fixed m its entries
// are strided by ~2 el, one cache line each.  Small pack/unpack kernels therefore move the
// coefficients to/from an m-major staging array (x_m contiguous, entry j <-> el = m + j, block m
// at offset m N - m (m-1)/2) and apply the real/complex convention factors; the diagonals are
// packed the same way.  The two main kernels then only see contiguous vectors:
//   k_block_matvec : 32 rows of B_m per workgroup (8 per wave), x_m staged through LDS in 256-column chunks,
//                    row-coalesced 512-byte loads of B, wavefront-shuffle reductions;
//   k_block_vecmat : 64 columns of B_m per workgroup, the four waves split the rows, B read in
//                    512-byte row segments, d_m broadcast from LDS, partial sums combined in LDS.
// The spectral budget (qf_spectral_budget: Z_l, T_l, I_l per degree) needs mat2shr of up to three matrices -- the state,
// its advective tendency, the forcing -- and pays ONE sweep for them: k_block_vecmat_multi carries all their packed
// diagonals through the row loop k_block_vecmat runs (block_vecmat_rows, written once), so each entry of the basis is
// read once and every coefficient column keeps the bits of mat2shr alone; k_degree_sums then reduces the products
// omega_lm v_lm over m, one wavefront per degree.  The MHD budget (qf_mhd_spectral_budget) carries five matrices through
// the same row loop (k_block_vecmat_five) and reduces nine pairs of columns (k_degree_pair_sums).
#include "qf_internal.h"

#pragma clang fp contract(off)   // the table of the direct Laplacian follows the reference's op order

namespace {

__device__ __forceinline__ size_t mmajor_offset(int m, int N) { return (size_t)m * N - (size_t)m * (m - 1) / 2; }
__device__ __forceinline__ size_t basis_offset(int m, int N)
{
    // basis_break_index(m, N), quantization.py:24-42
    const long long a = (long long)m - 1;
    long long ind = a + 2 * a * a - 6 * a * N + 6LL * N * N;
    ind *= 1 + a;
    return (size_t)(ind / 6);
}


// ---- the quantization basis itself (compute_basis, quantization.py:68-113) on the device.
// Block m of the basis holds the eigenvectors of the (N-m)x(N-m) tridiagonal block T_m of the
// direct Laplacian (quflow/laplacian/direct.py:19-62), column j <-> el = m + j, scaled to norm
// sqrt(N) and oriented by adjust_basis_orientation_ (quantization.py:45-65).  The reference calls
// LAPACK (scipy.linalg.eigh_tridiagonal).  Here the spectrum is known in closed form -- the
// Hoppe-Yau Laplacian has the eigenvalues -el(el+1) exactly -- so every eigenvector is ONE
// twisted factorisation of T_m - lambda I (the getvec step of MRRR, Parlett & Dhillon):
//     forward   D+_k = (d_k - lambda) - e_k^2 / D+_{k-1}
//     backward  D-_k = (d_k - lambda) - e_{k+1}^2 / D-_{k+1}
//     gamma_k = D+_k + D-_k - (d_k - lambda),  twist r = argmin |gamma_k|,  z_r = 1,
//     z_k = -(e_{k+1}/D+_k) z_{k+1} (k < r),   z_k = -(e_k/D-_k) z_{k-1} (k > r),
// repeated once with the Rayleigh-corrected shift lambda + gamma_r/|z|^2 (the matrix entries carry
// rounding errors, so its eigenvalues sit ~eps |T| off the integers).  One thread per eigenvector,
// threads of a block = consecutive columns j: every access B[k*n + j] is coalesced; the vector's
// own storage doubles as the scratch for D+ / D-.
__device__ __forceinline__ double direct_lap_diag(int N, int m, int k)
{
    const double s = (N - 1) / 2.0;
    const double m2 = -s + k, m1 = m2 + m;
    const double c = 2 * (s * (s + 1) - m1 * m2);                 // direct.py:40
    return fabs(c) > 1e-10 ? -c : 0.0;
}
__device__ __forceinline__ double direct_lap_off(int N, int m, int k)   // couples k-1 and k (k >= 1)
{
    const double s = (N - 1) / 2.0;
    const double a2 = -s + (k - 1), a1 = a2 + m;
    const double c = -sqrt(s * (s + 1) - a1 * (a1 + 1)) * sqrt(s * (s + 1) - a2 * (a2 + 1));   // direct.py:50
    return fabs(c) > 1e-10 ? -c : 0.0;
}

// Column j of block m (n = N - m entries, entry k at B[k * ld]): the twisted factorisation, its Rayleigh-corrected
// repeat, the scaling and the orientation.  Both basis kernels call this one function, so a column built into a slab
// (ld = J_m) has the same bits as the resident one (ld = n): the arithmetic never sees ld.
__device__ __forceinline__ void basis_column(int N, int m, int j, double *__restrict__ B, size_t ld)
{
    const int n = N - m;
    const size_t nn = ld;
    const long long el = m + j;
    double lambda = -(double)(el * (el + 1));
    // a pivot this small is replaced (LAPACK's pivmin idea): |T| ~ N^2/2, so 1e-30 |T| is far below
    // rounding and e^2/pivmin stays finite
    const double pivmin = 1e-30 * (1.0 + 0.5 * (double)N * (double)N);
#define QF_PIV(x_) if (fabs(x_) < pivmin) x_ = ((x_) < 0.0 ? -pivmin : pivmin)
    double znorm2 = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
        // (1) forward: D+ into the slots
        double dp = direct_lap_diag(N, m, 0) - lambda;
        QF_PIV(dp);
        B[0] = dp;
        for (int k = 1; k < n; ++k) {
            const double e = direct_lap_off(N, m, k);
            dp = (direct_lap_diag(N, m, k) - lambda) - (e / dp) * e;
            QF_PIV(dp);
            B[k * nn] = dp;
        }
        // (2) backward: twist index
        double dm = direct_lap_diag(N, m, n - 1) - lambda;
        QF_PIV(dm);
        int r = n - 1;
        double gam = dp + dm - (direct_lap_diag(N, m, n - 1) - lambda);
        double gbest = fabs(gam);
        for (int k = n - 2; k >= 0; --k) {
            const double e = direct_lap_off(N, m, k + 1);
            const double dk = direct_lap_diag(N, m, k) - lambda;
            dm = dk - (e / dm) * e;
            QF_PIV(dm);
            const double g = B[k * nn] + dm - dk;
            if (fabs(g) < gbest) {
                gbest = fabs(g);
                gam = g;
                r = k;
            }
        }
        // (3) backward again, D- into the slots above the twist
        dm = direct_lap_diag(N, m, n - 1) - lambda;
        QF_PIV(dm);
        if (n - 1 > r) B[(n - 1) * nn] = dm;
        for (int k = n - 2; k > r; --k) {
            const double e = direct_lap_off(N, m, k + 1);
            dm = (direct_lap_diag(N, m, k) - lambda) - (e / dm) * e;
            QF_PIV(dm);
            B[k * nn] = dm;
        }
        // (4) the vector
        znorm2 = 1.0;
        double z = 1.0;
        for (int k = r - 1; k >= 0; --k) {
            z = -(direct_lap_off(N, m, k + 1) / B[k * nn]) * z;
            B[k * nn] = z;
            znorm2 += z * z;
        }
        z = 1.0;
        for (int k = r + 1; k < n; ++k) {
            z = -(direct_lap_off(N, m, k) / B[k * nn]) * z;
            B[k * nn] = z;
            znorm2 += z * z;
        }
        B[r * nn] = 1.0;
        if (pass == 0) lambda += gam / znorm2;
    }
#undef QF_PIV
    // w2 *= sqrt(N) on unit vectors, then the orientation rule (quantization.py:45-65)
    const double par = (m % 2 == 1) ? -1.0 : 1.0;
    double mult = par;
    const double val = B[(n - 1) * nn];
    if (val < 0.0) {
        mult = -par;
    } else if (val == 0.0) {
        for (int jj = 2; jj < n; ++jj) {
            const double a = B[(n - jj) * nn], b = B[(n - jj - 1) * nn];
            if (fabs(a) > 1e-16 && fabs(b) > 1e-16) {
                const double this_sign = a > 0.0 ? 1.0 : -1.0, prev_sign = b > 0.0 ? 1.0 : -1.0;
                if (this_sign * prev_sign == -1.0) mult = this_sign * par * ((jj % 2 == 0) ? -1.0 : 1.0);
                else mult = this_sign * par;
                break;
            }
        }
    }
    const double scale = mult * (sqrt((double)N) / sqrt(znorm2));
    for (int k = 0; k < n; ++k) B[k * nn] *= scale;
}

__global__ __launch_bounds__(256) void k_basis(int N, double *__restrict__ basis)
{
    const int m = blockIdx.y;
    const int n = N - m;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    basis_column(N, m, j, basis + basis_offset(m, N) + j, (size_t)n);
}

// ---- the streamed form: blocks m0 <= m < m0 + gridDim.y of a band limit Nmax, only the columns j < J_m = Nmax - m
// that carry coefficients, block m row-major (N - m) x J_m at slab_prefix(m) - slab_prefix(m0) of a bounded slab
__global__ __launch_bounds__(256) void k_basis_slab(int N, int Nmax, int m0, double *__restrict__ slab)
{
    const int m = m0 + blockIdx.y;
    const int J = Nmax - m;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= J) return;
    basis_column(N, m, j, slab + (qf_slab_prefix(N, Nmax, m) - qf_slab_prefix(N, Nmax, m0)) + j, (size_t)J);
}

constexpr int MODE_SHR = 0, MODE_SHC = 1;

// ---- coefficients -> m-major vectors x (shr: one complex vector per m; shc: two)
// shr (quantization.py:223-241): m = 0: x = omega[el,0];  m > 0: x = (omega[el,m] - i omega[el,-m]) / sqrt(2)
// shc (quantization.py:352-362): x0 = omega[el,m] (lower diagonal), x1 = omega[el,-m] (upper, m != 0)
template <int MODE>
__global__ void k_pack_coeffs(int N, int Nmax, const double *__restrict__ omega, cplx *__restrict__ x0,
                              cplx *__restrict__ x1)
{
    const int m = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nmax || j >= Nmax - m) return;
    const long long el = m + j;
    const size_t o = mmajor_offset(m, N) + j;
    if (MODE == MODE_SHR) {
        if (m == 0) {
            x0[o] = make_double2(omega[el * el + el], 0.0);
        } else {
            const double c1dsq2 = 1.0 / sqrt(2.0);
            x0[o] = make_double2(c1dsq2 * omega[el * el + el + m], c1dsq2 * -omega[el * el + el - m]);
        }
    } else {
        const cplx *oc = reinterpret_cast<const cplx *>(omega);
        x0[o] = oc[el * el + el + m];
        if (m != 0) x1[o] = oc[el * el + el - m];
    }
}

// Where block m of a launch starts and its row stride: the resident basis (SLAB false: basis_offset, ld = N - m) or a
// slab of the streamed form (blocks from m0 on, ld = J_m).  The summation orders below depend on row and column indices
// only, so both sources give the same bits.
template <bool SLAB>
__device__ __forceinline__ const double *block_base(const double *basis, int N, int Nmax, int m0, int m, size_t &ld)
{
    if (SLAB) {
        ld = (size_t)(Nmax - m);
        return basis + (qf_slab_prefix(N, Nmax, m) - qf_slab_prefix(N, Nmax, m0));
    }
    ld = (size_t)(N - m);
    return basis + basis_offset(m, N);
}

// ---- y_m = B_m[:, :J] @ x_m and the assignment to the diagonals of W (followed by W *= 1j); blocks m0 + blockIdx.y
template <int MODE, bool SLAB>
__global__ __launch_bounds__(256) void k_block_matvec(int N, int Nmax, int m0, const double *__restrict__ basis,
                                                       const cplx *__restrict__ x0, const cplx *__restrict__ x1,
                                                       cplx *__restrict__ W)
{
    constexpr int RW = 8;                      // rows per wave: 8 x 4 independent 512-byte row loads in flight
    constexpr int ROWS = 4 * RW, CH = 256, NV = (MODE == MODE_SHC) ? 2 : 1;
    __shared__ cplx xs[NV][CH];
    const int m = m0 + blockIdx.y;
    const int n = N - m;
    const int row0 = blockIdx.x * ROWS;
    if (m >= Nmax || row0 >= n) return;
    const int J = Nmax - m;                   // columns that carry coefficients
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    size_t ld;
    const double *B = block_base<SLAB>(basis, N, Nmax, m0, m, ld);
    const size_t xo = mmajor_offset(m, N);
    double acc[RW][NV][2];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[r][v][0] = acc[r][v][1] = 0.0;
    // rows of this wave (clamped: a row past the block's end re-reads the last one and is dropped)
    const double *Brow[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        int i = row0 + wave * RW + r;
        if (i > n - 1) i = n - 1;
        Brow[r] = B + (size_t)i * ld;
    }
    for (int c0 = 0; c0 < J; c0 += CH) {
        __syncthreads();
        {
            const int j = c0 + threadIdx.x;
            cplx a = make_double2(0.0, 0.0), b = a;
            if (j < J) {
                a = x0[xo + j];
                if (NV == 2 && m != 0) b = x1[xo + j];
            }
            xs[0][threadIdx.x] = a;
            if (NV == 2) xs[NV - 1][threadIdx.x] = b;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < CH / 64; ++t) {
            const int jj = lane + 64 * t;
            if (c0 + jj < J) {
                double b[RW];
#pragma unroll
                for (int r = 0; r < RW; ++r) b[r] = Brow[r][c0 + jj];
                cplx x[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) x[v] = xs[v][jj];
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        acc[r][v][0] += b[r] * x[v].x;
                        acc[r][v][1] += b[r] * x[v].y;
                    }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int i = row0 + wave * RW + r;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                double s = acc[r][v][q];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
                acc[r][v][q] = s;
            }
        if (lane == 0 && i < n) {
            const double sgn = (m % 2 == 0) ? 1.0 : -1.0;
            if (MODE == MODE_SHR) {
                // diag_m *= sgn; lower = conj(diag_m), upper = diag_m; W *= 1j   (quantization.py:238-245)
                const double dr = sgn * acc[r][0][0], di = sgn * acc[r][0][1];
                if (m == 0) {
                    W[(size_t)i * N + i] = make_double2(-di, dr);              // 1j * (dr + i di), di == 0
                } else {
                    W[(size_t)i * N + (i + m)] = make_double2(-di, dr);        // 1j * diag_m
                    W[(size_t)(i + m) * N + i] = make_double2(di, dr);         // 1j * conj(diag_m)
                }
            } else {
                // lower: B_m @ omega[el, m]; upper (m != 0): sgn * B_m @ omega[el, -m]; W *= 1j  (:352-365)
                W[(size_t)(i + m) * N + i] = make_double2(-acc[r][0][1], acc[r][0][0]);
                if (m != 0) W[(size_t)i * N + (i + m)] = make_double2(-sgn * acc[r][NV - 1][1], sgn * acc[r][NV - 1][0]);
            }
        }
    }
}

// ---- diagonals of W -> m-major vectors d (lower diagonal m: W[k+m, k]; shc also upper: W[k, k+m])
template <int MODE>
__global__ void k_pack_diags(int N, int Nmax, const cplx *__restrict__ W, cplx *__restrict__ d0, cplx *__restrict__ d1)
{
    const int m = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nmax || k >= N - m) return;
    const size_t o = mmajor_offset(m, N) + k;
    d0[o] = W[(size_t)(k + m) * N + k];
    if (MODE == MODE_SHC && m != 0) d1[o] = W[(size_t)k * N + (k + m)];
}

// ---- z_m[j] = sum_k d_m[k] B_m[k, j], j < J; blocks m0 + blockIdx.y
// The packed diagonals and results of the NV vectors one sweep carries (mat2shc: lower and upper diagonal; the spectral
// budget: the state, its advective tendency and the forcing).  Passed by value: indexed by unrolled constants only.
template <int NV>
struct vecmat_vectors {
    const cplx *d[NV];
    cplx *z[NV];
};

// The row loop, written once for every kernel that sweeps B_m from the left.  Each entry of B is read once and multiplied
// into all NV vectors; vectors v >= nload are not loaded (their d counts as zero: mat2shc's upper diagonal at m = 0).
// The accumulation order of a vector depends on the row and column indices alone -- wave w takes the rows w, w + 4, ... of
// every 256-row chunk in ascending order, then (wave 0 + wave 1) + (wave 2 + wave 3) -- never on NV or on the other
// vectors, so every column has the bits it has when it is swept alone.
// FOLD: the waves' partial sums take the place of the staged diagonals once the row loop is over (one barrier more), which
// halves the LDS of a workgroup -- the arithmetic and its order are the same.
template <int NV, bool FOLD>
struct vecmat_lds {
    cplx ds[NV][256];
    double part[4][NV][2][64];
};
template <int NV>
struct vecmat_lds<NV, true> {
    union {
        cplx ds[NV][256];
        double part[4][NV][2][64];
    };
};

template <int NV, bool SLAB, bool FOLD = false>
__device__ __forceinline__ void block_vecmat_rows(int N, int Nmax, int m0, const double *__restrict__ basis,
                                                  const vecmat_vectors<NV> &p, int m, int nload)
{
    constexpr int KCH = 256;
    __shared__ vecmat_lds<NV, FOLD> lds;
    const int n = N - m;
    const int J = Nmax - m;
    const int j0 = blockIdx.x * 64;
    if (m >= Nmax || j0 >= J) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = j0 + lane;
    const bool live = j < J;
    size_t ld;
    const double *B = block_base<SLAB>(basis, N, Nmax, m0, m, ld) + (live ? j : j0);
    const size_t dof = mmajor_offset(m, N);
    double acc[NV][2];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v][0] = acc[v][1] = 0.0;
    for (int k0 = 0; k0 < n; k0 += KCH) {
        __syncthreads();
        {
            const int k = k0 + threadIdx.x;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                cplx a = make_double2(0.0, 0.0);
                if (k < n && v < nload) a = p.d[v][dof + k];
                lds.ds[v][threadIdx.x] = a;
            }
        }
        __syncthreads();
        const int kend = (n - k0 < KCH) ? n - k0 : KCH;
        // the four waves interleave the rows of the chunk; 8 independent row loads in flight per wave
        for (int kk = wave; kk < kend; kk += 32) {
            double b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = kk + 4 * u;
                b[u] = (k < kend) ? B[(size_t)(k0 + k) * ld] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = kk + 4 * u;
                if (k < kend) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const cplx d = lds.ds[v][k];
                        acc[v][0] += d.x * b[u];
                        acc[v][1] += d.y * b[u];
                    }
                }
            }
        }
    }
    if (FOLD) __syncthreads();      // (every wave is done reading lds.ds before lds.part overwrites it)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        lds.part[wave][v][0][lane] = acc[v][0];
        lds.part[wave][v][1][lane] = acc[v][1];
    }
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const double re = (lds.part[0][v][0][lane] + lds.part[1][v][0][lane]) + (lds.part[2][v][0][lane] + lds.part[3][v][0][lane]);
            const double im = (lds.part[0][v][1][lane] + lds.part[1][v][1][lane]) + (lds.part[2][v][1][lane] + lds.part[3][v][1][lane]);
            p.z[v][dof + j] = make_double2(re, im);
        }
    }
}

template <int MODE, bool SLAB>
__global__ __launch_bounds__(256) void k_block_vecmat(int N, int Nmax, int m0, const double *__restrict__ basis,
                                                       const cplx *__restrict__ d0, const cplx *__restrict__ d1,
                                                       cplx *__restrict__ z0, cplx *__restrict__ z1)
{
    constexpr int NV = (MODE == MODE_SHC) ? 2 : 1;
    vecmat_vectors<NV> p;
    p.d[0] = d0;
    p.z[0] = z0;
    p.d[NV - 1] = (NV == 2) ? d1 : d0;
    p.z[NV - 1] = (NV == 2) ? z1 : z0;
    const int m = m0 + blockIdx.y;
    block_vecmat_rows<NV, SLAB>(N, Nmax, m0, basis, p, m, (NV == 2 && m == 0) ? 1 : NV);
}

// ---- the same sweep for NV packed diagonals of NV different matrices (mat2shr of each of them in one pass over the basis)
template <int NV, bool SLAB>
__global__ __launch_bounds__(256) void k_block_vecmat_multi(int N, int Nmax, int m0, const double *__restrict__ basis,
                                                             vecmat_vectors<NV> p)
{
    block_vecmat_rows<NV, SLAB>(N, Nmax, m0, basis, p, m0 + blockIdx.y, NV);
}

// ---- ... and for the five matrices of the MHD budget (W, Theta, advection, Lorentz term, induction), folded: 20 KB of LDS
// per workgroup where the unfolded loop would take 40 KB.  Measured (N = 2048, kernel time): folded 5.66 ms,
// unfolded 5.79 ms, two sweeps of three and two vectors 4.97 + 4.87 ms; mat2shr's one-vector sweep 4.70 ms.
template <bool SLAB>
__global__ __launch_bounds__(256) void k_block_vecmat_five(int N, int Nmax, int m0, const double *__restrict__ basis,
                                                            vecmat_vectors<5> p)
{
    block_vecmat_rows<5, SLAB, true>(N, Nmax, m0, basis, p, m0 + blockIdx.y, 5);
}

// ---- m-major results z -> omega with the convention factors
// shr (quantization.py:303-327): m = 0: omega[el,0] = Re(z / 1j) = Im z;  m > 0:
//   omega[el,m] = sqrt2*sgn*Im z,  omega[el,-m] = -sqrt2*sgn*Re z;  finally omega /= N
// shc (quantization.py:381-396): omega[el,m] = z0, omega[el,-m] = sgn*z1 (m != 0); omega /= 1j*N
//   (numpy divides by the complex scalar 0 + N i by multiplying with 1/N: out = (Im, -Re) * (1/N))
template <int MODE>
__global__ void k_unpack_coeffs(int N, int Nmax, const cplx *__restrict__ z0, const cplx *__restrict__ z1,
                                double *__restrict__ omega)
{
    const int m = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Nmax || j >= Nmax - m) return;
    const long long el = m + j;
    const size_t o = mmajor_offset(m, N) + j;
    const double sgn = (m % 2 == 0) ? 1.0 : -1.0;
    const cplx a = z0[o];
    if (MODE == MODE_SHR) {
        if (m == 0) {
            omega[el * el + el] = a.y / (double)N;
        } else {
            const double sqrt2 = sqrt(2.0);
            omega[el * el + el + m] = (sqrt2 * sgn * a.y) / (double)N;
            omega[el * el + el - m] = (-sqrt2 * sgn * a.x) / (double)N;
        }
    } else {
        cplx *oc = reinterpret_cast<cplx *>(omega);
        const double invN = 1.0 / (double)N;
        oc[el * el + el + m] = make_double2(a.y * invN, -a.x * invN);
        if (m != 0) {
            const cplx b = z1[o];
            oc[el * el + el - m] = make_double2((sgn * b.y) * invN, -(sgn * b.x) * invN);
        }
    }
}

// ---- per-degree sums of products of real coefficient arrays: out[r * Nmax + l] = sum_{m=-l..l} u[l^2+l+m] v_r[l^2+l+m]
// for l < Nmax, r = blockIdx.y (the rows Z, T/2, I/2 of the spectral budget: v_0 = u).  One wavefront per degree, four
// degrees per workgroup.  The order is fixed: lane t sums the entries l^2 + t, l^2 + t + 64, ... of the degree in
// ascending order (product and sum rounded separately), then the xor butterfly 32, 16, 8, 4, 2, 1 over the 64 lanes.
// `scale` (1 or 2) multiplies the finished sum, which is exact.
struct degree_rows {
    const double *v[3];
    double scale[3];
};
// the sum of degree l over the 64 lanes of one wavefront, in every lane: written once for both kernels below
__device__ __forceinline__ double degree_sum(const double *__restrict__ u, const double *__restrict__ v, int l, int lane)
{
    const size_t base = (size_t)l * l;
    const int count = 2 * l + 1;
    double s = 0.0;
    for (int t = lane; t < count; t += 64) s += u[base + t] * v[base + t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}
__global__ __launch_bounds__(256) void k_degree_sums(int Nmax, const double *__restrict__ u, degree_rows rows,
                                                      double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= Nmax) return;                    // (whole wavefronts leave: the shuffles below see all 64 lanes)
    const int r = blockIdx.y;
    const double *__restrict__ v = r == 0 ? rows.v[0] : (r == 1 ? rows.v[1] : rows.v[2]);
    const double sc = r == 0 ? rows.scale[0] : (r == 1 ? rows.scale[1] : rows.scale[2]);
    const double s = degree_sum(u, v, l, lane);
    if (lane == 0) out[(size_t)r * Nmax + l] = sc * s;
}

// ---- the pair form: out[r * Nmax + l] = scale_r sum_m u_r[l^2+l+m] v_r[l^2+l+m] for a table of (u, v, scale), one grid row
// per pair (the nine rows of the MHD budget).  The table is a kernel argument: it is read from the argument segment at
// blockIdx.y, never copied to private memory.
constexpr int QF_DEGREE_PAIRS = 9;
struct degree_pairs {
    const double *u[QF_DEGREE_PAIRS];
    const double *v[QF_DEGREE_PAIRS];
    double scale[QF_DEGREE_PAIRS];
};
__global__ __launch_bounds__(256) void k_degree_pair_sums(int Nmax, degree_pairs pairs, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= Nmax) return;                    // (whole wavefronts leave)
    const int r = blockIdx.y;
    const double s = degree_sum(pairs.u[r], pairs.v[r], l, lane);
    if (lane == 0) out[(size_t)r * Nmax + l] = pairs.scale[r] * s;
}

// The streamed form's slabs for band limit Nmax, planned and the slab grown to the largest of them (hipFree waits for the
// device).  Called before anything is launched, so a refusal leaves W and the coefficients as they were.
int reserve_slabs(qf_ctx *ctx, int Nmax, std::vector<int> &first)
{
    long long need = 0;
    QF_TRY(qf_slab_plan(ctx->N, Nmax, ctx->slab_budget, first, &need));
    if ((size_t)need > ctx->slab_cap) {
        if (ctx->slab) (void)hipFree(ctx->slab);
        ctx->slab = nullptr;
        ctx->slab_cap = 0;
        QF_HIP(hipMalloc((void **)&ctx->slab, (size_t)need));
        ctx->slab_cap = (size_t)need;
    }
    return QF_OK;
}

// blocks first[s] <= m < first[s + 1] of the band limit Nmax into ctx->slab
int generate_slab(qf_ctx *ctx, int Nmax, int m0, int m1)
{
    dim3 grid((Nmax - m0 + 255) / 256, m1 - m0);
    hipLaunchKernelGGL(k_basis_slab, grid, dim3(256), 0, ctx->stream, ctx->N, Nmax, m0, ctx->slab);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

// Pack once; then either one launch over the resident basis, or generate -> apply for each slab (ctx->slab_budget > 0)
template <int MODE>
int forward(qf_ctx *ctx, int Nmax, const double *omega_dev, cplx *W_dev)
{
    const int N = ctx->N;
    cplx *x0 = ctx->sh_stage, *x1 = ctx->sh_stage + (size_t)N * (N + 1) / 2;
    std::vector<int> first;
    if (ctx->slab_budget > 0) QF_TRY(reserve_slabs(ctx, Nmax, first));
    QF_HIP(hipMemsetAsync(W_dev, 0, (size_t)N * N * sizeof(cplx), ctx->stream));   // np.zeros((N,N)), quantization.py:474
    dim3 gp((Nmax + 255) / 256, Nmax);
    hipLaunchKernelGGL(k_pack_coeffs<MODE>, gp, dim3(256), 0, ctx->stream, N, Nmax, omega_dev, x0, x1);
    QF_HIP(hipGetLastError());
    if (ctx->slab_budget == 0) {
        dim3 gm((N + 31) / 32, Nmax);   // 32 rows per workgroup
        hipLaunchKernelGGL((k_block_matvec<MODE, false>), gm, dim3(256), 0, ctx->stream, N, Nmax, 0, ctx->basis, x0, x1, W_dev);
        QF_HIP(hipGetLastError());
        return QF_OK;
    }
    for (size_t s = 0; s + 1 < first.size(); ++s) {
        const int m0 = first[s], m1 = first[s + 1];
        QF_TRY(generate_slab(ctx, Nmax, m0, m1));
        dim3 gm((N + 31) / 32, m1 - m0);
        hipLaunchKernelGGL((k_block_matvec<MODE, true>), gm, dim3(256), 0, ctx->stream, N, Nmax, m0, ctx->slab, x0, x1, W_dev);
        QF_HIP(hipGetLastError());
    }
    return QF_OK;
}

template <int MODE>
int backward(qf_ctx *ctx, int Nmax, const cplx *W_dev, double *omega_dev)
{
    const int N = ctx->N;
    const size_t half = (size_t)N * (N + 1) / 2;
    cplx *d0 = ctx->sh_stage, *d1 = d0 + half, *z0 = d1 + half, *z1 = z0 + half;
    std::vector<int> first;
    if (ctx->slab_budget > 0) QF_TRY(reserve_slabs(ctx, Nmax, first));
    dim3 gp((N + 255) / 256, Nmax);
    hipLaunchKernelGGL(k_pack_diags<MODE>, gp, dim3(256), 0, ctx->stream, N, Nmax, W_dev, d0, d1);
    QF_HIP(hipGetLastError());
    if (ctx->slab_budget == 0) {
        dim3 gm((Nmax + 63) / 64, Nmax);
        hipLaunchKernelGGL((k_block_vecmat<MODE, false>), gm, dim3(256), 0, ctx->stream, N, Nmax, 0, ctx->basis, d0, d1, z0, z1);
        QF_HIP(hipGetLastError());
    } else {
        for (size_t s = 0; s + 1 < first.size(); ++s) {
            const int m0 = first[s], m1 = first[s + 1];
            QF_TRY(generate_slab(ctx, Nmax, m0, m1));
            dim3 gm((Nmax - m0 + 63) / 64, m1 - m0);
            hipLaunchKernelGGL((k_block_vecmat<MODE, true>), gm, dim3(256), 0, ctx->stream, N, Nmax, m0, ctx->slab, d0, d1, z0, z1);
            QF_HIP(hipGetLastError());
        }
    }
    dim3 gu((Nmax + 255) / 256, Nmax);
    hipLaunchKernelGGL(k_unpack_coeffs<MODE>, gu, dim3(256), 0, ctx->stream, N, Nmax, z0, z1, omega_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

template <int NV, bool SLAB>
void launch_vecmat_multi(qf_ctx *ctx, dim3 grid, int Nmax, int m0, const double *basis, cplx *const d[3], cplx *const z[3])
{
    vecmat_vectors<NV> p;
    for (int v = 0; v < NV; ++v) {
        p.d[v] = d[v];
        p.z[v] = z[v];
    }
    hipLaunchKernelGGL((k_block_vecmat_multi<NV, SLAB>), grid, dim3(256), 0, ctx->stream, ctx->N, Nmax, m0, basis, p);
}

template <bool SLAB>
int vecmat_multi(qf_ctx *ctx, int nv, dim3 grid, int Nmax, int m0, const double *basis, cplx *const d[3], cplx *const z[3])
{
    // one vector: mat2shr's own kernel
    if (nv == 1)
        hipLaunchKernelGGL((k_block_vecmat<MODE_SHR, SLAB>), grid, dim3(256), 0, ctx->stream, ctx->N, Nmax, m0, basis, d[0],
                           (const cplx *)nullptr, z[0], (cplx *)nullptr);
    else if (nv == 2) launch_vecmat_multi<2, SLAB>(ctx, grid, Nmax, m0, basis, d, z);
    else launch_vecmat_multi<3, SLAB>(ctx, grid, Nmax, m0, basis, d, z);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

// the five vectors of the MHD budget over one slab or the resident basis
template <bool SLAB>
int vecmat_five(qf_ctx *ctx, dim3 grid, int Nmax, int m0, const double *basis, cplx *const d[5], cplx *const z[5])
{
    vecmat_vectors<5> p;
    for (int v = 0; v < 5; ++v) {
        p.d[v] = d[v];
        p.z[v] = z[v];
    }
    hipLaunchKernelGGL((k_block_vecmat_five<SLAB>), grid, dim3(256), 0, ctx->stream, ctx->N, Nmax, m0, basis, p);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

}  // namespace

// mat2shr of nv matrices in ONE sweep of the basis, then the per-degree sums of omega_0 * omega_r.  The diagonals are
// packed and the coefficients unpacked by mat2shr's own kernels, launched once per matrix (two N^2-sized passes per matrix
// beside a sweep of N^3/3): with the shared row loop every omega_r has the bits of qf_launch_mat2shr of that matrix alone.
int qf_launch_degree_budget(qf_ctx *ctx, int Nmax, int nv, const cplx *const mats[3], cplx *const z[3], double *const omega[3],
                            double *sums_dev)
{
    const int N = ctx->N;
    const size_t half = (size_t)N * (N + 1) / 2;
    cplx *d[3] = {ctx->sh_stage, ctx->sh_stage + half, ctx->sh_stage + 2 * half};
    std::vector<int> first;
    if (ctx->slab_budget > 0) QF_TRY(reserve_slabs(ctx, Nmax, first));
    dim3 gp((N + 255) / 256, Nmax);
    for (int v = 0; v < nv; ++v) {
        hipLaunchKernelGGL(k_pack_diags<MODE_SHR>, gp, dim3(256), 0, ctx->stream, N, Nmax, mats[v], d[v], (cplx *)nullptr);
        QF_HIP(hipGetLastError());
    }
    if (ctx->slab_budget == 0) {
        QF_TRY(vecmat_multi<false>(ctx, nv, dim3((Nmax + 63) / 64, Nmax), Nmax, 0, ctx->basis, d, z));
    } else {
        for (size_t s = 0; s + 1 < first.size(); ++s) {
            const int m0 = first[s], m1 = first[s + 1];
            QF_TRY(generate_slab(ctx, Nmax, m0, m1));
            QF_TRY(vecmat_multi<true>(ctx, nv, dim3((Nmax - m0 + 63) / 64, m1 - m0), Nmax, m0, ctx->slab, d, z));
        }
    }
    dim3 gu((Nmax + 255) / 256, Nmax);
    degree_rows rows;
    for (int v = 0; v < 3; ++v) {
        rows.v[v] = omega[v < nv ? v : 0];
        rows.scale[v] = v == 0 ? 1.0 : 2.0;
    }
    for (int v = 0; v < nv; ++v) {
        hipLaunchKernelGGL(k_unpack_coeffs<MODE_SHR>, gu, dim3(256), 0, ctx->stream, N, Nmax, z[v], (const cplx *)nullptr, omega[v]);
        QF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_degree_sums, dim3((Nmax + 3) / 4, nv), dim3(256), 0, ctx->stream, Nmax, omega[0], rows, sums_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

// The MHD budget's transform stage (qf_api.h): as qf_launch_degree_budget, for five matrices and nine rows.
int qf_launch_mhd_degree_budget(qf_ctx *ctx, int Nmax, const cplx *const mats[5], cplx *const d[5], cplx *const z[5],
                                double *const omega[5], double *sums_dev)
{
    const int N = ctx->N;
    std::vector<int> first;
    if (ctx->slab_budget > 0) QF_TRY(reserve_slabs(ctx, Nmax, first));
    dim3 gp((N + 255) / 256, Nmax);
    for (int v = 0; v < 5; ++v) {
        hipLaunchKernelGGL(k_pack_diags<MODE_SHR>, gp, dim3(256), 0, ctx->stream, N, Nmax, mats[v], d[v], (cplx *)nullptr);
        QF_HIP(hipGetLastError());
    }
    if (ctx->slab_budget == 0) {
        QF_TRY(vecmat_five<false>(ctx, dim3((Nmax + 63) / 64, Nmax), Nmax, 0, ctx->basis, d, z));
    } else {
        for (size_t s = 0; s + 1 < first.size(); ++s) {
            const int m0 = first[s], m1 = first[s + 1];
            QF_TRY(generate_slab(ctx, Nmax, m0, m1));
            QF_TRY(vecmat_five<true>(ctx, dim3((Nmax - m0 + 63) / 64, m1 - m0), Nmax, m0, ctx->slab, d, z));
        }
    }
    dim3 gu((Nmax + 255) / 256, Nmax);
    for (int v = 0; v < 5; ++v) {
        hipLaunchKernelGGL(k_unpack_coeffs<MODE_SHR>, gu, dim3(256), 0, ctx->stream, N, Nmax, z[v], (const cplx *)nullptr, omega[v]);
        QF_HIP(hipGetLastError());
    }
    // rows 0..8: ww, tt, wt, 2 wa, 2 wb, 2 tc, ta, tb, wc   (0 omega, 1 theta, 2 advection, 3 Lorentz, 4 induction)
    static const int iu[QF_DEGREE_PAIRS] = {0, 1, 0, 0, 0, 1, 1, 1, 0};
    static const int iv[QF_DEGREE_PAIRS] = {0, 1, 1, 2, 3, 4, 2, 3, 4};
    degree_pairs pairs;
    for (int r = 0; r < QF_DEGREE_PAIRS; ++r) {
        pairs.u[r] = omega[iu[r]];
        pairs.v[r] = omega[iv[r]];
        pairs.scale[r] = (r >= 3 && r <= 5) ? 2.0 : 1.0;
    }
    hipLaunchKernelGGL(k_degree_pair_sums, dim3((Nmax + 3) / 4, QF_DEGREE_PAIRS), dim3(256), 0, ctx->stream, Nmax, pairs, sums_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_slab_plan(int N, int Nmax, long long slab_bytes, std::vector<int> &first, long long *max_bytes)
{
    first.clear();
    *max_bytes = 0;
    if (N < 1 || Nmax < 1 || Nmax > N) {
        qf_set_error("qf_slab_plan: band limit Nmax=%d outside 1..N=%d", Nmax, N);
        return QF_ERR_INVALID;
    }
    const long long block0 = 8LL * N * Nmax;     // the largest block: every other one is smaller
    if (slab_bytes < block0) {
        qf_set_error("streamed basis: block m=0 for N=%d, Nmax=%d takes %lld bytes, more than the slab budget of %lld bytes",
                     N, Nmax, block0, slab_bytes);
        return QF_ERR_INVALID;
    }
    int m0 = 0;
    first.push_back(0);
    for (int m = 1; m <= Nmax; ++m) {
        const long long bytes = 8 * (qf_slab_prefix(N, Nmax, m) - qf_slab_prefix(N, Nmax, m0));
        const bool last = (m == Nmax);
        const long long next = last ? 0 : 8LL * (N - m) * (Nmax - m);
        if (last || bytes + next > slab_bytes) {
            if (bytes > *max_bytes) *max_bytes = bytes;
            first.push_back(m);
            m0 = m;
        }
    }
    return QF_OK;
}

int qf_launch_basis(qf_ctx *ctx, double *basis_dev)
{
    const int N = ctx->N;
    dim3 grid((N + 255) / 256, N);
    hipLaunchKernelGGL(k_basis, grid, dim3(256), 0, ctx->stream, N, basis_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_band_basis(qf_ctx *ctx, int Nmax, double *band_dev)
{
    dim3 grid((Nmax + 255) / 256, Nmax);
    hipLaunchKernelGGL(k_basis_slab, grid, dim3(256), 0, ctx->stream, ctx->N, Nmax, 0, band_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_band_shr2mat(qf_ctx *ctx, int Nmax, const double *band_dev, const double *omega_dev, cplx *stage, cplx *W_dev)
{
    const int N = ctx->N;
    dim3 gp((Nmax + 255) / 256, Nmax);
    hipLaunchKernelGGL(k_pack_coeffs<MODE_SHR>, gp, dim3(256), 0, ctx->stream, N, Nmax, omega_dev, stage, (cplx *)nullptr);
    QF_HIP(hipGetLastError());
    dim3 gm((N + 31) / 32, Nmax);   // 32 rows per workgroup
    hipLaunchKernelGGL((k_block_matvec<MODE_SHR, true>), gm, dim3(256), 0, ctx->stream, N, Nmax, 0, band_dev, stage,
                       (const cplx *)nullptr, W_dev);
    QF_HIP(hipGetLastError());
    return QF_OK;
}

int qf_launch_shr2mat(qf_ctx *ctx, int Nmax, const double *omega_dev, cplx *W_dev) { return forward<MODE_SHR>(ctx, Nmax, omega_dev, W_dev); }
int qf_launch_shc2mat(qf_ctx *ctx, const double *omega_dev, cplx *W_dev) { return forward<MODE_SHC>(ctx, ctx->N, omega_dev, W_dev); }
int qf_launch_mat2shr(qf_ctx *ctx, int Nmax, const cplx *W_dev, double *omega_dev) { return backward<MODE_SHR>(ctx, Nmax, W_dev, omega_dev); }
int qf_launch_mat2shc(qf_ctx *ctx, const cplx *W_dev, double *omega_dev) { return backward<MODE_SHC>(ctx, ctx->N, W_dev, omega_dev); }
