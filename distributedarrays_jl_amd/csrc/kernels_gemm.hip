// kernels_gemm.hip — local dense C = alpha*A*B + beta*C, COLUMN-major
// (Julia layout), MFMA-tiled for gfx950 (CDNA4).
//
// Replaces the worker-side `localpart(A) * Bjk` of the reference's
// src/linalg.jl:224 (the per-tile GEMM inside _matmatmul!,
// linalg.jl:190-253).  The reference runs OpenBLAS gemm on the host; here
// the chunk lives in HBM and Float64/Float32 run on the exact-input MFMA
// pipes (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32; the f32 one is
// bitwise an fmaf chain).
//
// Structure: one kernel template, gemm_mfma<T>.  128x128 block tile,
// BK=16, 512 threads = 8 waves (2x4), each wave a 64x32 sub-tile = 4x2
// fragments of 16x16, so the accumulators are 64 VGPRs and 4 waves/SIMD
// stay co-resident: one block's stage phase hides under another's MFMA
// phase.  Operands are LDS-staged with a 17-element row stride; tile t+1's
// global loads issue before tile t's MFMA phase and land in LDS after the
// barrier (two barriers per K-tile); blocks are remapped bijectively so
// each XCD's L2 sees neighbouring tiles.  Sizes that are not whole tiles,
// and Int64, take a naive per-thread kernel (parity path for small
// chunks).  The variants this layout was measured against are recorded in
// profiles/r01_kernel_stats.md ("GEMM variant ladder").
#include "common.hpp"

namespace da {

constexpr int BM = 128, BN = 128, BK = 16;
constexpr int LSTR = 17;   // LDS row stride (odd: staging writes 2-way not 4-way conflicted; frag reads stay conflict-free — profiles/r01 PMC)
constexpr int NTHR = 512;

// What differs between the two exact-input 16x16x4 MFMAs.  Both put C/D
// column lane&15 in each lane; the row of accumulator register q is
// ROW_Q*q + ROW_L*(lane>>4) — the q/lane roles are opposite in f64 and
// f32 (probed on hardware: tests/test_gpu_mfma_probe.py,
// tools/probe_f32.py).  vec_t is one 16-byte staging load of VL elements.
template <typename T> struct Mfma;
template <> struct Mfma<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    typedef double vec_t __attribute__((ext_vector_type(2)));
    static constexpr int VL = 2, ROW_Q = 4, ROW_L = 1;
    static __device__ __forceinline__ acc_t mfma(double a, double b,
                                                 acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    typedef float vec_t __attribute__((ext_vector_type(4)));
    static constexpr int VL = 4, ROW_Q = 1, ROW_L = 4;
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
};

template <typename T>
__global__ __launch_bounds__(512, 4)
void gemm_mfma(const T* __restrict__ A, const T* __restrict__ B,
               T* __restrict__ C, int64_t m, int64_t n, int64_t k,
               int64_t lda, int64_t ldb, int64_t ldc, T alpha, T beta) {
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    using vec_t = typename M::vec_t;
    constexpr int VL = M::VL;
    constexpr int NP = BM * BK / (NTHR * VL);   // staging pieces per thread
    __shared__ T As[BM * LSTR];   // As[mm][kk] at mm*LSTR + kk
    __shared__ T Bs[BN * LSTR];   // Bs[nn][kk] at nn*LSTR + kk

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int l4 = lane >> 4;
    const int wr = (wave >> 2) * 64;   // 2 wave-rows of 64
    const int wc = (wave & 3) * 32;    // 4 wave-cols of 32

    // bijective XCD remap (dispatcher places block b on XCD b%8)
    const int gx = gridDim.x, nwg = gridDim.x * gridDim.y;
    int w = blockIdx.y * gx + blockIdx.x;
    int q = nwg >> 3, rmd = nwg & 7, xcd = w & 7, idx = w >> 3;
    int sw = (xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q)
             + idx;
    const int64_t bm = (int64_t)(sw % gx) * BM;
    const int64_t bn = (int64_t)(sw / gx) * BN;

    acc_t acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = {0, 0, 0, 0};

    // staging: each tile is BM*BK elements = NTHR * NP pieces of VL.
    // Piece r of this thread: A column a_c, rows a_r..a_r+VL-1 (contiguous
    // in column-major A); B column b_n, k-rows b_k..b_k+VL-1.  Coordinates
    // are recomputed where used — keeping them in arrays costs VGPRs
    // against the __launch_bounds__(512,4) budget — and stay unsigned so
    // the divisions fold to the shifts and masks they are.
    auto piece = [&](int r) { return (unsigned)tid + r * NTHR; };
    auto a_c = [&](int r) { return (int)(piece(r) / (BM / VL)); };
    auto a_r = [&](int r) { return (int)(piece(r) % (BM / VL) * VL); };
    auto b_n = [&](int r) { return (int)(piece(r) / (BK / VL)); };
    auto b_k = [&](int r) { return (int)(piece(r) % (BK / VL) * VL); };

    // The global->register and register->LDS steps are written out at
    // both of their uses (prologue and K loop) rather than as capturing
    // lambdas: with those the f64 instantiation schedules its prologue
    // differently, and it has no register to spare (128 VGPRs, one spill).
    // Each piece stores through one base pointer so that element e is a
    // constant offset; indexing As[(a_r + e) * LSTR + a_c] spills a second
    // VGPR.  Store order per piece: A elements, then B elements.
    vec_t pa[NP], pb[NP];
    const int64_t ktiles = k / BK;
#pragma unroll
    for (int r = 0; r < NP; ++r) {   // prologue: tile 0 -> regs -> LDS
        pa[r] = *reinterpret_cast<const vec_t*>(
            A + (int64_t)a_c(r) * lda + bm + a_r(r));
        pb[r] = *reinterpret_cast<const vec_t*>(
            B + (bn + b_n(r)) * ldb + b_k(r));
    }
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        T* ap = &As[a_r(r) * LSTR + a_c(r)];
        T* bp = &Bs[b_n(r) * LSTR + b_k(r)];
#pragma unroll
        for (int e = 0; e < VL; ++e) ap[e * LSTR] = pa[r][e];
#pragma unroll
        for (int e = 0; e < VL; ++e) bp[e] = pb[r][e];
    }

    for (int64_t kt = 0; kt < ktiles; ++kt) {
        __syncthreads();   // LDS tile kt visible to all
        if (kt + 1 < ktiles) {   // tile kt+1 -> regs, in flight over the MFMAs
            const int64_t k0 = (kt + 1) * BK;
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                pa[r] = *reinterpret_cast<const vec_t*>(
                    A + (k0 + a_c(r)) * lda + bm + a_r(r));
                pb[r] = *reinterpret_cast<const vec_t*>(
                    B + (bn + b_n(r)) * ldb + k0 + b_k(r));
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            T a[4], b[2];
            const int kof = kk * 4 + l4;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                a[i] = As[(wr + i * 16 + l16) * LSTR + kof];
#pragma unroll
            for (int j = 0; j < 2; ++j)
                b[j] = Bs[(wc + j * 16 + l16) * LSTR + kof];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = M::mfma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();   // MFMA phase done; LDS reusable
        if (kt + 1 < ktiles) {
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                T* ap = &As[a_r(r) * LSTR + a_c(r)];
                T* bp = &Bs[b_n(r) * LSTR + b_k(r)];
#pragma unroll
                for (int e = 0; e < VL; ++e) ap[e * LSTR] = pa[r][e];
#pragma unroll
                for (int e = 0; e < VL; ++e) bp[e] = pb[r][e];
            }
        }
    }

    // Epilogue.  beta == 0 never reads C.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int64_t col = bn + wc + j * 16 + l16;
            T* cp = C + col * ldc + bm + wr + i * 16 + M::ROW_L * l4;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                T v = alpha * acc[i][j][qq];
                cp[M::ROW_Q * qq] = (beta == (T)0)
                    ? v : v + beta * cp[M::ROW_Q * qq];
            }
        }
    }
}

// Naive kernel for arbitrary shapes (small parity chunks) and Int64.
template <typename T>
__global__ void gemm_naive_t(const T* __restrict__ A,
                             const T* __restrict__ B, T* __restrict__ C,
                             int64_t m, int64_t n, int64_t k,
                             int64_t lda, int64_t ldb, int64_t ldc,
                             T alpha, T beta) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t j = (int64_t)blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= m || j >= n) return;
    T s = (T)0;
    for (int64_t kk = 0; kk < k; ++kk)
        s += A[kk * lda + i] * B[j * ldb + kk];
    T v = alpha * s;
    C[j * ldc + i] = (beta == (T)0) ? v : v + beta * C[j * ldc + i];
}

// beta-only scaling when k == 0 (fill!/rmul! branch of linalg.jl:232-240)
template <typename T>
__global__ void scale_c_t(T* __restrict__ C, int64_t m, int64_t n,
                          int64_t ldc, T beta) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t j = (int64_t)blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= m || j >= n) return;
    C[j * ldc + i] = (beta == (T)0) ? (T)0 : beta * C[j * ldc + i];
}

// Debug probe: one 16x16x4 MFMA with the lane mapping this file assumes.
// out_raw = acc[q] per (lane,q), so a test can reverse-engineer the true
// map if the assumption is wrong; out_c (optional) = 16x16 col-major under
// the assumed C/D map.  Exported as dbg_mfma_probe_f64 / _f32.
template <typename T>
__global__ void mfma_probe_kernel(const T* __restrict__ A,
                                  const T* __restrict__ B,
                                  T* __restrict__ out_c,
                                  T* __restrict__ out_raw) {
    using M = Mfma<T>;
    int l = threadIdx.x;
    T a = A[(l & 15) + 16 * (l >> 4)];   // A[row, k] col-major 16x4
    T b = B[(l >> 4) + 4 * (l & 15)];    // B[k, col] col-major 4x16
    typename M::acc_t acc = {0, 0, 0, 0};
    acc = M::mfma(a, b, acc);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        out_raw[l * 4 + q] = acc[q];
        int row = M::ROW_Q * q + M::ROW_L * (l >> 4), col = l & 15;
        if (out_c) out_c[row + 16 * col] = acc[q];
    }
}

template <typename T>
static int launch_mfma_probe(const void* A, const void* B, void* out_c,
                             void* out_raw, hipStream_t s) {
    hipLaunchKernelGGL(mfma_probe_kernel<T>, dim3(1), dim3(64), 0, s,
                       (const T*)A, (const T*)B, (T*)out_c, (T*)out_raw);
    DA_CHECK_HIP(hipGetLastError());
    DA_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int dbg_mfma_probe_impl(int dtype, const void* A, const void* B,
                        void* out_c, void* out_raw, hipStream_t s) {
    return dtype == DA_F64 ? launch_mfma_probe<double>(A, B, out_c, out_raw, s)
                           : launch_mfma_probe<float>(A, B, out_c, out_raw, s);
}

// Host-only MFMA-vs-naive choice shared by launch_gemm_f64/f32 (exported
// as dbg_gemm_path): the MFMA kernel needs whole 128x128x16 tiles.
int gemm_path(int64_t m, int64_t n, int64_t k) {
    return (m % BM == 0 && n % BN == 0 && k % BK == 0) ? DA_GEMM_MFMA
                                                       : DA_GEMM_NAIVE;
}

template <typename T>
static int launch_gemm_float(const char* who, void* Cv, const void* Av,
                             const void* Bv, int64_t m, int64_t n, int64_t k,
                             int64_t lda, int64_t ldb, int64_t ldc,
                             double alpha, double beta, hipStream_t s) {
    if (m < 0 || n < 0 || k < 0) return set_err(-3, "%s: bad shape", who);
    if (m == 0 || n == 0) return 0;
    const T* A = (const T*)Av;
    const T* B = (const T*)Bv;
    T* C = (T*)Cv;
    const T al = (T)alpha, be = (T)beta;
    const dim3 t(64, 4), g((m + 63) / 64, (n + 3) / 4);   // per-element grid
    if (k == 0 || al == (T)0)
        hipLaunchKernelGGL(scale_c_t<T>, g, t, 0, s, C, m, n, ldc, be);
    else if (gemm_path(m, n, k) == DA_GEMM_MFMA)
        hipLaunchKernelGGL(gemm_mfma<T>, dim3(m / BM, n / BN), dim3(NTHR), 0,
                           s, A, B, C, m, n, k, lda, ldb, ldc, al, be);
    else
        hipLaunchKernelGGL(gemm_naive_t<T>, g, t, 0, s,
                           A, B, C, m, n, k, lda, ldb, ldc, al, be);
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_gemm_f64(void* C, const void* A, const void* B,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    double alpha, double beta, hipStream_t s) {
    return launch_gemm_float<double>("da_gemm_f64", C, A, B, m, n, k,
                                     lda, ldb, ldc, alpha, beta, s);
}

int launch_gemm_f32(void* C, const void* A, const void* B,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    double alpha, double beta, hipStream_t s) {
    return launch_gemm_float<float>("da_gemm_f32", C, A, B, m, n, k,
                                    lda, ldb, ldc, alpha, beta, s);
}

int launch_gemm_i64(void* Cv, const void* Av, const void* Bv,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    int64_t alpha, int64_t beta, hipStream_t s) {
    if (m <= 0 || n <= 0) return 0;
    dim3 t(64, 4), g((m + 63) / 64, (n + 3) / 4);
    hipLaunchKernelGGL(gemm_naive_t<int64_t>, g, t, 0, s,
                       (const int64_t*)Av, (const int64_t*)Bv,
                       (int64_t*)Cv, m, n, k, lda, ldb, ldc, alpha, beta);
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

} // namespace da
