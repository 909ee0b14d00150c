// kernels_elementwise.hip — fill / philox-rand / map / map2 / fused
// broadcast / axpby / add / scale / cast / transpose / diag for gfx950
// (CDNA4).
//
// These replace the reference's per-worker Base loops on localparts:
//   map!            /root/reference/src/mapreduce.jl:5-12
//   elementwise ops /root/reference/src/mapreduce.jl:180-189
//   broadcast       /root/reference/src/broadcast.jl:65-85
//   fill!/rand!     /root/reference/src/darray.jl:468-532,822-834
//   add!/axpy!/rmul!/root/reference/src/linalg.jl:24-76
//
// All HBM-bound, no LDS needed.  Every pointwise kernel is one instance of
// pointwise_kernel: a grid-stride loop over vectors of W lanes (W = 4 is
// 32 B/lane for 8-byte types, W = 2 is 16 B, W = 1 scalar) and a scalar
// tail; the functor passed in owns only the arithmetic of one element (its
// operator() is force-inlined: left to the inliner, the runtime-op switch
// becomes a function call).
// The five rand kernels are rand_kernel over a generator.  This file is
// compiled with -ffp-contract=off so that a*b+c keeps Julia-Base/numpy bit
// semantics (separate mul, add); transcendentals use OCML and are
// parity-tested at 2-3 ulp tolerance.
#include "common.hpp"
#include "philox_device.hpp"
#include "mapops.hpp"
#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace da {

constexpr int TPB = 256;
constexpr int MAXBLOCKS = 8192;   // 1024 workgroups per XCD — fills the chip

// Blocks per launcher, as each was last measured.  The formulas disagree
// with the lane widths on purpose: making them agree changes speed and is
// not a tidy-up.
//
//   launcher            lanes               blocks from
//   fill                W2, NT gate         n/2 + 1
//   rand                2 per philox block  n/2 + 1 (uniform f32: 4, n/4 + 1)
//   map hot/cold/i64    W4|W2 / W2 / W1     n/2 + 1  (W2-sized for all three)
//   map2 float/i64      W2 / W1             n/2 + 1  (i64: twice the lanes)
//   map2_scalar         W1                  n
//   bcast_fma           W4, or W2 + NT gate n/2 + 1  (W2-sized for W4 too)
//   axpby, add, scale   W4                  n        (scalar-sized)
//   cast                W1                  n
//   diag_scale          W1                  m*n
static inline int nblocks(uint64_t work) {
    uint64_t b = (work + TPB - 1) / TPB;
    if (b > (uint64_t)MAXBLOCKS) b = MAXBLOCKS;
    if (b == 0) b = 1;
    return (int)b;
}

// A/B switches, read once per process; profiles/ record the measured
// winners.
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// nontemporal stores on write-only streams (gfx950 `nt` flag)
static bool use_nt() {
    static const int v = env_int("DA_NT", 0);
    return v == 1;
}
// hot map ops: W4 sin 0.878 ms vs W2 0.946 (and vs same-box hipMemcpy 0.881)
static bool map_w4() {
    static const int v = env_int("DA_MAP_W", 4);
    return v == 4;
}
// bcast_fma: W4 1.21 vs W2 1.37 ms on 2^28; the NT kernel exists as W2 only
static bool bcast_w4() {
    static const int v = env_int("DA_BC_W", 4);
    return v == 4 && !use_nt();
}

// -------------------------------------------------------------- pointwise
// dst[j] = f(src[j]...), or f(dst[j], src[j]...) when F::reads_dst: the
// in-place kernels (axpby, add, scale) reach their destination through
// this one pointer only.  NT: nontemporal vector stores.
//
// Caller contract: dst may be exactly one of the sources (map_(op, d, d))
// — element j is read before it is written and no other thread touches it
// — but may never partially overlap one.
template <typename T, int W>
using vec = T __attribute__((ext_vector_type(W)));

// lane K of the result, from lane K of every operand
template <int K, typename F, typename... V>
__device__ __forceinline__ auto lane(const F& f, const V&... v) {
    return f(v[K]...);
}
// all W lanes at dv: one vector per source in v, the old destination vector
// in front of them for an in-place functor
template <typename F, typename TD, int... K, typename... V>
__device__ __forceinline__ vec<TD, sizeof...(K)> lanes(
        const F& f, const vec<TD, sizeof...(K)>* dv,
        std::integer_sequence<int, K...>, const V&... v) {
    if constexpr (F::reads_dst) {
        const vec<TD, sizeof...(K)> old = *dv;
        return {lane<K>(f, old, v...)...};
    } else {
        return {lane<K>(f, v...)...};
    }
}

template <int W, bool NT, typename F, typename TD, typename... TS>
__global__ void pointwise_kernel(F f, TD* __restrict__ dst, uint64_t n,
                                 const TS* __restrict__... src) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t tail = 0;
    if constexpr (W > 1) {
        uint64_t nv = n / W;
        tail = W * nv;
        vec<TD, W>* dv = reinterpret_cast<vec<TD, W>*>(dst);
        for (uint64_t j = i; j < nv; j += stride) {
            const vec<TD, W> r = lanes(
                f, dv + j, std::make_integer_sequence<int, W>{},
                reinterpret_cast<const vec<TS, W>*>(src)[j]...);
            if constexpr (NT) __builtin_nontemporal_store(r, dv + j);
            else dv[j] = r;
        }
    }
    for (uint64_t j = tail + i; j < n; j += stride) {
        if constexpr (F::reads_dst) dst[j] = f(dst[j], src[j]...);
        else dst[j] = f(src[j]...);
    }
}

template <int W, bool NT, typename F, typename TD, typename... TS>
static void stream(int g, hipStream_t s, F f, TD* dst, uint64_t n,
                   const TS*... src) {
    hipLaunchKernelGGL((pointwise_kernel<W, NT, F, TD, TS...>), dim3(g),
                       dim3(TPB), 0, s, f, dst, n, src...);
}

// float and i64 op tables of mapops.hpp behind one name
template <typename T>
__device__ __forceinline__ T map1(int op, T x) {
    if constexpr (std::is_same<T, int64_t>::value) return apply_map_i64(op, x);
    else return apply_map<T>(op, x);
}
template <typename T>
__device__ __forceinline__ T map2(int op, T a, T b) {
    if constexpr (std::is_same<T, int64_t>::value)
        return apply_map2_i64(op, a, b);
    else return apply_map2<T>(op, a, b);
}

// ------------------------------------------------------------------- fill
template <typename T>
struct Fill {
    static constexpr bool reads_dst = false;
    T v;
    __device__ __forceinline__ T operator()() const { return v; }
};

int launch_fill(void* chunk, double v, uint64_t n, int dtype, hipStream_t s) {
    if (n == 0) return 0;
    int g = nblocks(n / 2 + 1);
    return dispatch_dtype<DT_ALL>(dtype, "da_fill", [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (use_nt()) stream<2, true>(g, s, Fill<T>{(T)v}, (T*)chunk, n);
        else stream<2, false>(g, s, Fill<T>{(T)v}, (T*)chunk, n);
    });
}

// ------------------------------------------------------------------- rand
// Element mapping documented in oracle/philox.py (bit-identical contract):
// philox block b yields elements PER*b .. PER*b + PER-1 of the stream, of
// which this call writes [offset, offset + n).
// A generator turns one block into PER outputs: prep() does the work they
// share, elem<J>() makes output J.  J is a template constant, not a loop
// variable: with both outputs of a normal in one expression the compiler
// merges the cos and sin argument reductions and runs the large-argument
// path unconditionally (measured 0.81 vs 0.71 ms per 2^27 f64).
struct UniformF64 {
    using T = double;
    static constexpr int PER = 2;
    static __device__ __forceinline__ u32x4 prep(const u32x4& o) { return o; }
    template <int J>
    static __device__ __forceinline__ T elem(const u32x4& o) {
        return u01_f64(o.v[2 * J], o.v[2 * J + 1]);
    }
};
struct UniformF32 {
    using T = float;
    static constexpr int PER = 4;
    static __device__ __forceinline__ u32x4 prep(const u32x4& o) { return o; }
    template <int J>
    static __device__ __forceinline__ T elem(const u32x4& o) {
        return u01_f32(o.v[J]);
    }
};
struct RawI64 {
    using T = int64_t;
    static constexpr int PER = 2;
    static __device__ __forceinline__ u32x4 prep(const u32x4& o) { return o; }
    template <int J>
    static __device__ __forceinline__ T elem(const u32x4& o) {
        return (int64_t)(((uint64_t)o.v[2 * J + 1] << 32) | o.v[2 * J]);
    }
};
template <typename F> struct Polar { F r, th; };   // Box-Muller on one block
struct NormalF64 {
    using T = double;
    static constexpr int PER = 2;
    static __device__ __forceinline__ Polar<double> prep(const u32x4& o) {
        double u1 = u01_f64(o.v[0], o.v[1]);
        double u2 = u01_f64(o.v[2], o.v[3]);
        return {sqrt(-2.0 * log1p(-u1)), 2.0 * M_PI * u2};
    }
    template <int J>
    static __device__ __forceinline__ T elem(const Polar<double>& p) {
        if constexpr (J == 0) return p.r * cos(p.th);
        else return p.r * sin(p.th);
    }
};
struct NormalF32 {
    using T = float;
    static constexpr int PER = 2;
    static __device__ __forceinline__ Polar<float> prep(const u32x4& o) {
        float u1 = u01_f32(o.v[0]);
        float u2 = u01_f32(o.v[1]);
        return {sqrtf(-2.0f * log1pf(-u1)), 2.0f * (float)M_PI * u2};
    }
    template <int J>
    static __device__ __forceinline__ T elem(const Polar<float>& p) {
        if constexpr (J == 0) return p.r * cosf(p.th);
        else return p.r * sinf(p.th);
    }
};

// outputs J... of block b, each stored only if this call covers it
template <typename G, typename S, int... J>
__device__ __forceinline__ void rand_store(
        typename G::T* __restrict__ p, uint64_t n, uint64_t offset,
        uint64_t b, const S& st, std::integer_sequence<int, J...>) {
    ((G::PER * b + J >= offset && G::PER * b + J < offset + n
          ? (void)(p[G::PER * b + J - offset] = G::template elem<J>(st))
          : (void)0), ...);
}

template <typename G>
__global__ void rand_kernel(typename G::T* __restrict__ p, uint64_t n,
                            uint64_t seed, uint64_t offset) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t first_blk = offset / G::PER, last_blk = (offset + n - 1) / G::PER;
    for (uint64_t b = first_blk + t; b <= last_blk; b += stride)
        rand_store<G>(p, n, offset, b, G::prep(philox4x32_10(b, seed)),
                      std::make_integer_sequence<int, G::PER>{});
}

template <typename G>
static void rand_stream(void* chunk, uint64_t n, uint64_t seed,
                        uint64_t offset, hipStream_t s) {
    hipLaunchKernelGGL(rand_kernel<G>, dim3(nblocks(n / G::PER + 1)),
                       dim3(TPB), 0, s, (typename G::T*)chunk, n, seed,
                       offset);
}

int launch_rand(void* chunk, uint64_t n, int dtype, uint64_t seed, int kind,
                uint64_t offset, hipStream_t s) {
    if (n == 0) return 0;
    if (kind != DA_RAND_UNIFORM && kind != DA_RAND_NORMAL)
        return set_err(-3, "da_rand: bad kind %d", kind);
    const bool normal = kind == DA_RAND_NORMAL;
    if (normal && dtype != DA_F64 && dtype != DA_F32)
        return set_err(-3, "da_rand: normal needs float dtype");
    return dispatch_dtype<DT_ALL>(dtype, "da_rand", [&](auto tag) {
        using T = typename decltype(tag)::type;
        if constexpr (std::is_same<T, double>::value) {
            if (normal) rand_stream<NormalF64>(chunk, n, seed, offset, s);
            else rand_stream<UniformF64>(chunk, n, seed, offset, s);
        } else if constexpr (std::is_same<T, float>::value) {
            if (normal) rand_stream<NormalF32>(chunk, n, seed, offset, s);
            else rand_stream<UniformF32>(chunk, n, seed, offset, s);
        } else {
            rand_stream<RawI64>(chunk, n, seed, offset, s);
        }
    });
}

// -------------------------------------------------------------------- map
struct MapOp {                      // op chosen at run time
    static constexpr bool reads_dst = false;
    int op;
    template <typename T>
    __device__ __forceinline__ T operator()(T x) const {
        return map1<T>(op, x);
    }
};

// Hot ops get compile-time instantiations: the 63-case runtime switch
// inflates register pressure (map!(sin) measured 1.08 -> 1.99 ms when
// the extended op set landed); with OP a template constant the switch
// folds to one case.
template <int OP>
struct MapFixed {
    static constexpr bool reads_dst = false;
    template <typename T>
    __device__ __forceinline__ T operator()(T x) const {
        return apply_map<T>(OP, x);
    }
};

#define DA_HOT_OPS(X)                                                   \
    X(DA_OP_IDENTITY) X(DA_OP_NEG) X(DA_OP_ABS) X(DA_OP_ABS2)           \
    X(DA_OP_INV) X(DA_OP_SQRT) X(DA_OP_EXP) X(DA_OP_LOG)                \
    X(DA_OP_SIN) X(DA_OP_COS) X(DA_OP_TAN) X(DA_OP_TANH)                \
    X(DA_OP_FLOOR) X(DA_OP_SIGN) X(DA_OP_LOG1P) X(DA_OP_EXPM1)

// float map: hot ops at W4 (or W2), every other op through the runtime
// switch at W2
template <typename T>
static void map_float(int opcode, T* dst, const T* src, uint64_t n, int g,
                      hipStream_t s) {
    switch (opcode) {
#define DA_CASE(OPC)                                                    \
    case OPC:                                                           \
        if (map_w4()) stream<4, false>(g, s, MapFixed<OPC>{}, dst, n, src); \
        else stream<2, false>(g, s, MapFixed<OPC>{}, dst, n, src);      \
        return;
    DA_HOT_OPS(DA_CASE)
#undef DA_CASE
    }
    stream<2, false>(g, s, MapOp{opcode}, dst, n, src);
}

int launch_map(int opcode, void* dst, const void* src, uint64_t n, int dtype,
               hipStream_t s) {
    if (n == 0) return 0;
    if (opcode < 0 || opcode >= DA_OP__N)
        return set_err(-3, "da_map: bad opcode %d", opcode);
    if (dtype == DA_I64 &&
        !(opcode == DA_OP_IDENTITY || opcode == DA_OP_NEG ||
          opcode == DA_OP_ABS || opcode == DA_OP_ABS2 ||
          opcode == DA_OP_SIGN))
        return set_err(-3, "da_map: opcode %d invalid for i64", opcode);
    int g = nblocks(n / 2 + 1);
    return dispatch_dtype<DT_ALL>(dtype, "da_map", [&](auto tag) {
        using T = typename decltype(tag)::type;
        if constexpr (std::is_same<T, int64_t>::value)
            stream<1, false>(g, s, MapOp{opcode}, (T*)dst, n, (const T*)src);
        else
            map_float<T>(opcode, (T*)dst, (const T*)src, n, g, s);
    });
}

// ------------------------------------------------------------------- map2
struct Map2Op {
    static constexpr bool reads_dst = false;
    int op;
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const {
        return map2<T>(op, a, b);
    }
};

int launch_map2(int opcode, void* dst, const void* a, const void* b,
                uint64_t n, int dtype, hipStream_t s) {
    if (n == 0) return 0;
    if (opcode < 0 || opcode >= DA_OP2__N)
        return set_err(-3, "da_map2: bad opcode %d", opcode);
    int g = nblocks(n / 2 + 1);
    return dispatch_dtype<DT_ALL>(dtype, "da_map2", [&](auto tag) {
        using T = typename decltype(tag)::type;
        constexpr int W = std::is_same<T, int64_t>::value ? 1 : 2;
        stream<W, false>(g, s, Map2Op{opcode}, (T*)dst, n, (const T*)a,
                         (const T*)b);
    });
}

// scalar-broadcast forms: D .= f.(src, c) / f.(c, src) (e.g. D .+ 1,
// the cfg-1 plumbing op; Base broadcast with a scalar argument —
// broadcast.jl:124-133 treats singletons as local, no distribution)
template <typename T>
struct Map2Scalar {
    static constexpr bool reads_dst = false;
    int op;
    T c;
    int rev;
    __device__ __forceinline__ T operator()(T a) const {
        return rev ? map2<T>(op, c, a) : map2<T>(op, a, c);
    }
};

int launch_map2_scalar(int opcode, void* dst, const void* src, double c,
                       int rev, uint64_t n, int dtype, hipStream_t s) {
    if (n == 0) return 0;
    if (opcode < 0 || opcode >= DA_OP2__N)
        return set_err(-3, "da_map2_scalar: bad opcode %d", opcode);
    int g = nblocks(n);
    return dispatch_dtype<DT_ALL>(dtype, "da_map2_scalar", [&](auto tag) {
        using T = typename decltype(tag)::type;
        stream<1, false>(g, s, Map2Scalar<T>{opcode, (T)c, rev}, (T*)dst, n,
                         (const T*)src);
    });
}


// ---------------------------------------------------- transpose / diag
// Local 2-D transpose (dst = src^T), LDS-tiled so both sides stay
// coalesced — the per-chunk piece of copy(::Transpose{<:DArray})
// (linalg.jl:10-17).
template <typename T>
__global__ void transpose_kernel(T* __restrict__ dst,
                                 const T* __restrict__ src,
                                 uint64_t m, uint64_t n) {
    __shared__ T tile[32][33];
    uint64_t bi = (uint64_t)blockIdx.x * 32;
    uint64_t bj = (uint64_t)blockIdx.y * 32;
    int tx = threadIdx.x, ty = threadIdx.y;   // 32 x 8
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint64_t i = bi + tx, j = bj + ty + r * 8;
        if (i < m && j < n) tile[ty + r * 8][tx] = src[i + j * m];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint64_t j = bj + tx, i = bi + ty + r * 8;   // dst is n x m
        if (j < n && i < m) dst[j + i * n] = tile[tx][ty + r * 8];
    }
}

int launch_transpose(void* dst, const void* src, uint64_t m, uint64_t n,
                     int dtype, hipStream_t s) {
    if (m == 0 || n == 0) return 0;
    dim3 t(32, 8), g((m + 31) / 32, (n + 31) / 32);
    return dispatch_dtype<DT_ALL>(dtype, "da_transpose", [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(transpose_kernel<T>, g, t, 0, s, (T*)dst,
                           (const T*)src, m, n);
    });
}

// Diagonal scaling: side=0 rows (lmul!(Diagonal(d), A), linalg.jl:169-177),
// side=1 cols (rmul!(A, Diagonal(d)), linalg.jl:179-187).
template <typename T>
__global__ void diag_scale_kernel(T* __restrict__ a, uint64_t m, uint64_t n,
                                  const T* __restrict__ diag, int side) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t total = m * n;
    for (uint64_t t = e; t < total; t += stride) {
        uint64_t i = t % m, j = t / m;
        a[t] = a[t] * diag[side == 0 ? i : j];
    }
}

int launch_diag_scale(void* a, uint64_t m, uint64_t n, const void* diag,
                      int side, int dtype, hipStream_t s) {
    if (m == 0 || n == 0) return 0;
    int g = nblocks(m * n);
    return dispatch_dtype<DT_FLOAT>(dtype, "da_diag_scale", [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(diag_scale_kernel<T>, dim3(g), dim3(TPB), 0, s,
                           (T*)a, m, n, (const T*)diag, side);
    });
}

// ------------------------------------------- fused broadcast & BLAS-1 like
template <typename T>
struct MulAdd {                     // d = a * b + c
    static constexpr bool reads_dst = false;
    T c;
    // -ffp-contract=off: mul then add (Julia Base)
    __device__ __forceinline__ T operator()(T a, T b) const {
        return a * b + c;
    }
};

int launch_bcast_fma(void* d, const void* a, const void* b, double c,
                     uint64_t n, int dtype, hipStream_t s) {
    if (n == 0) return 0;
    int g = nblocks(n / 2 + 1);
    return dispatch_dtype<DT_FLOAT>(dtype, "da_bcast_fma", [&](auto tag) {
        using T = typename decltype(tag)::type;
        MulAdd<T> f{(T)c};
        T* dp = (T*)d;
        const T *ap = (const T*)a, *bp = (const T*)b;
        if (bcast_w4()) stream<4, false>(g, s, f, dp, n, ap, bp);
        else if (use_nt()) stream<2, true>(g, s, f, dp, n, ap, bp);
        else stream<2, false>(g, s, f, dp, n, ap, bp);
    });
}

template <typename T>
struct Axpby {                      // y = alpha * x + beta * y
    static constexpr bool reads_dst = true;
    T alpha, beta;
    __device__ __forceinline__ T operator()(T y, T x) const {
        return alpha * x + beta * y;
    }
};

int launch_axpby(void* y, const void* x, double alpha, double beta,
                 uint64_t n, int dtype, hipStream_t s) {
    if (n == 0) return 0;
    int g = nblocks(n);
    return dispatch_dtype<DT_FLOAT>(dtype, "da_axpby", [&](auto tag) {
        using T = typename decltype(tag)::type;
        stream<4, false>(g, s, Axpby<T>{(T)alpha, (T)beta}, (T*)y, n,
                         (const T*)x);
    });
}

// add! (linalg.jl:62-76): scale==1 adds without multiplying, matching the
// reference's fast path numerics exactly.
template <typename T>
struct Add {
    static constexpr bool reads_dst = true;
    T scale;
    int unit;
    __device__ __forceinline__ T operator()(T d, T s_) const {
        return unit ? d + s_ : d + scale * s_;
    }
};

int launch_add(void* dest, const void* src, double scale, uint64_t n,
               int dtype, hipStream_t s) {
    if (n == 0) return 0;
    int g = nblocks(n);
    int unit = (scale == 1.0);
    return dispatch_dtype<DT_ALL>(dtype, "da_add", [&](auto tag) {
        using T = typename decltype(tag)::type;
        stream<4, false>(g, s, Add<T>{(T)scale, unit}, (T*)dest, n,
                         (const T*)src);
    });
}

template <typename T>
struct Scale {
    static constexpr bool reads_dst = true;
    T v;
    __device__ __forceinline__ T operator()(T a) const { return a * v; }
};

int launch_scale(void* a, double s_, uint64_t n, int dtype, hipStream_t s) {
    if (n == 0) return 0;
    int g = nblocks(n);
    return dispatch_dtype<DT_ALL>(dtype, "da_scale", [&](auto tag) {
        using T = typename decltype(tag)::type;
        stream<4, false>(g, s, Scale<T>{(T)s_}, (T*)a, n);
    });
}


// ------------------------------------------------------------------ cast
// dtype conversion (the DArray{T2}(D) / convert family): dst[i] =
// (TD)src[i].  float->i64 rounds half-even (Julia round(Int, x)); the
// strict InexactError convert is a host-side concern.
template <typename TD>
struct Cast {
    static constexpr bool reads_dst = false;
    template <typename TS>
    __device__ __forceinline__ TD operator()(TS x) const {
        if constexpr (std::is_same<TD, int64_t>::value) {
            if constexpr (std::is_same<TS, float>::value)
                return (TD)rintf(x);
            else return (TD)rint(x);
        } else {
            return (TD)x;
        }
    }
};

int launch_cast(void* dst, int dst_dtype, const void* src, int src_dtype,
                uint64_t n, hipStream_t s) {
    if (n == 0) return 0;
    if (dst_dtype == src_dtype)
        return set_err(-3, "da_cast: same dtype (use da_d2d)");
    if (!dtype_size(dst_dtype) || !dtype_size(src_dtype))
        return set_err(-3, "da_cast: bad dtypes %d<-%d", dst_dtype,
                       src_dtype);
    int g = nblocks(n);
    // both dtypes are valid here; the inner dispatch reports the launch
    int rc = 0;
    dispatch_dtype<DT_ALL>(dst_dtype, "da_cast", [&](auto dtag) {
        using TD = typename decltype(dtag)::type;
        rc = dispatch_dtype<DT_ALL>(src_dtype, "da_cast", [&](auto stag) {
            using TS = typename decltype(stag)::type;
            if constexpr (!std::is_same<TD, TS>::value)
                stream<1, false>(g, s, Cast<TD>{}, (TD*)dst, n,
                                 (const TS*)src);
        });
    });
    return rc;
}

} // namespace da
