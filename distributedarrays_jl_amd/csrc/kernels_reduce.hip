// kernels_reduce.hip — per-chunk mapreduce stage for gfx950.
//
// Replaces the worker-side hot loop `mapreduce(f, op, localpart(d))` of
// /root/reference/src/mapreduce.jl:29-35 (and the specials :97-131).
// Two-stage tree: grid-stride vectorized loads -> per-thread partial ->
// 64-wide wavefront __shfl_down reduction -> LDS across the block's 4
// waves -> one partial per block; the last block to finish folds the
// block partials in the same launch (DA_RED_FUSED=0: a single-block
// second kernel does, in the same order) and writes the result to a
// pinned host slot.  Integer add/mul wrap mod 2^64, so any order is
// bit-exact (test/darray.jl:286-294 exactness contract); float order is
// a tree, within the 1e-6 contract of BASELINE.json (the reference's own
// fold order is likewise unspecified: docs/src/index.md:208-236).
#include "common.hpp"
#include "reduce_core.hpp"
#include "reduce_wait.hpp"
#include <stdlib.h>

namespace da {

// reduce_grid: blocks of a flat reduce over `want` blocks' worth of work,
// capped (DA_RBLOCKS, default 2048).
int reduce_grid(uint64_t want) {
    static int cap = -1;
    if (cap < 0) {
        const char* e = getenv("DA_RBLOCKS");
        cap = e ? atoi(e) : 2048;
        if (cap < 1 || cap > RMAXB) cap = 2048;
    }
    if (want < 1) want = 1;
    return (int)(want > (uint64_t)cap ? (uint64_t)cap : want);
}

static inline bool reduce_v4() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("DA_RV4");
        v = e ? atoi(e) : 0;
    }
    return v == 1;
}

template <typename T>
__device__ __forceinline__ T mapf(int mapop, T x) {
    switch (mapop) {
    case DA_REDF_IDENTITY: return x;
    case DA_REDF_ABS: return fabs(x);   // abs(-0.0) = +0.0
    case DA_REDF_ABS2: return x * x;
    case DA_REDF_ISNAN: return (T)(x != x ? 1 : 0);
    case DA_REDF_ISFINITE: return (T)(isfinite((double)x) ? 1 : 0);
    case DA_REDF_NONZERO: return (T)(x != (T)0 ? 1 : 0);
    }
    return x;
}
__device__ __forceinline__ int64_t mapf(int mapop, int64_t x) {
    switch (mapop) {
    case DA_REDF_IDENTITY: return x;
    case DA_REDF_ABS: return x < 0 ? (int64_t)(0ull - (uint64_t)x) : x;
    case DA_REDF_ABS2: return (int64_t)((uint64_t)x * (uint64_t)x);
    case DA_REDF_ISNAN: return 0;
    case DA_REDF_ISFINITE: return 1;
    case DA_REDF_NONZERO: return x != 0 ? 1 : 0;
    }
    return x;
}

template <typename T>
__device__ __forceinline__ T block_reduce(int redop, T v) {
    __shared__ T lds[RTPB / 64];
    return block_reduce_in(redop, v, lds);
}

// The grid-stride accumulate loop of every flat reduce kernel: W-wide
// vector loads over the first n/W*W elements, then the scalar tail.
// fold(acc, x) absorbs one source element.  Every caller is launched
// with RTPB threads per block; the constant keeps the stride in SGPRs.
// The vector loads are non-temporal (global_load_dwordx4 ... nt): the
// source is read once, so keeping it in the caches only costs — 338 ->
// 308 us per sum of 2^28 f64, same bits (profiles/r5_reduce_wait.md).
template <int W, typename T, typename A, typename F>
__device__ __forceinline__ A grid_accumulate(const T* __restrict__ src,
                                             uint64_t n, A acc, F fold) {
    uint64_t i = (uint64_t)blockIdx.x * RTPB + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * RTPB;
    using V = T __attribute__((ext_vector_type(W)));
    uint64_t nv = n / W;
    const V* sv = reinterpret_cast<const V*>(src);
    for (uint64_t j = i; j < nv; j += stride) {
        V v = __builtin_nontemporal_load(&sv[j]);
#pragma unroll
        for (int k = 0; k < W; ++k) acc = fold(acc, (T)v[k]);
    }
    for (uint64_t j = W * nv + i; j < n; j += stride)
        acc = fold(acc, src[j]);
    return acc;
}

// MOP/ROP >= 0 fold the op switches at compile time for the hot
// combos (same trick as map_fixed/dims-reduce); -1 = runtime args.
template <typename T, int MOP = -1, int ROP = -1>
__global__ void reduce_stage1(int mapop, int redop, const T* __restrict__ src,
                              uint64_t n, T* __restrict__ partials) {
    if (MOP >= 0) mapop = MOP;
    if (ROP >= 0) redop = ROP;
    T acc = grid_accumulate<2>(src, n, RedIdent<T>::get(redop),
        [=](T a, T x) { return red_comb(redop, a, mapf<T>(mapop, x)); });
    acc = block_reduce(redop, acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// 32 B/thread-iteration variant (two dwordx4 per lane): more memory-
// level parallelism per wave — A/B-gated via DA_RV4.
template <typename T, int MOP = -1, int ROP = -1>
__global__ void reduce_stage1_v4(int mapop, int redop,
                                 const T* __restrict__ src, uint64_t n,
                                 T* __restrict__ partials) {
    if (MOP >= 0) mapop = MOP;
    if (ROP >= 0) redop = ROP;
    T acc = grid_accumulate<4>(src, n, RedIdent<T>::get(redop),
        [=](T a, T x) { return red_comb(redop, a, mapf<T>(mapop, x)); });
    acc = block_reduce(redop, acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// The single-launch fan-in (publish_partial, fanin_finish) and its
// ticket invariant are in reduce_core.hpp.
//
// `partials` is deliberately not __restrict__/const: its loads must stay
// vector loads behind the acquire.  `out` is the host-visible pinned slot;
// `seq` is published next to the value (publish_result).
template <typename T, int MOP = -1, int ROP = -1>
__global__ void reduce_fused(int mapop, int redop, const T* __restrict__ src,
                             uint64_t n, T* partials, unsigned int* ticket,
                             unsigned int base, T* out,
                             unsigned long long seq) {
    if (MOP >= 0) mapop = MOP;
    if (ROP >= 0) redop = ROP;
    __shared__ T sh[RTPB / 64 + 1];
    T acc = grid_accumulate<2>(src, n, RedIdent<T>::get(redop),
        [=](T a, T x) { return red_comb(redop, a, mapf<T>(mapop, x)); });
    acc = block_reduce_in(redop, acc, sh);
    fanin_finish(redop, acc, partials, ticket, base, out, seq, sh);
}

template <typename T>
__global__ void reduce_stage2(int redop, const T* __restrict__ partials,
                              int np, T* __restrict__ out) {
    T acc = RedIdent<T>::get(redop);
    for (int j = threadIdx.x; j < np; j += blockDim.x)
        acc = red_comb(redop, acc, partials[j]);
    acc = block_reduce(redop, acc);
    if (threadIdx.x == 0) out[0] = acc;
}

// DA_RED_FUSED: unset or nonzero = single launch; 0 = stage 1 + stage 2.
bool reduce_fused_on() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("DA_RED_FUSED");
        v = e ? (atoi(e) != 0) : 1;
    }
    return v == 1;
}

template <typename T> struct FlatArgs {
    bool fused;
    int grid, mapop, redop;
    const T* src;
    uint64_t n;
    T *parts, *out;
    hipStream_t s;
};

template <typename T, int MOP, int ROP>
static int launch_flat(const FlatArgs<T>& a) {
    if (a.fused)
        return fanin_launch_seq(a.grid, [&](unsigned int base,
                                            unsigned long long seq) {
            hipLaunchKernelGGL((reduce_fused<T, MOP, ROP>), dim3(a.grid),
                               dim3(RTPB), 0, a.s, a.mapop, a.redop, a.src,
                               a.n, a.parts, st().red_ticket, base, a.out,
                               seq);
            return hipGetLastError();
        });
    hipLaunchKernelGGL((reduce_stage1<T, MOP, ROP>), dim3(a.grid),
                       dim3(RTPB), 0, a.s, a.mapop, a.redop, a.src, a.n,
                       a.parts);
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
static int do_reduce(int mapop, int redop, const T* src, uint64_t n,
                     void* out_host, hipStream_t s) {
    if (n == 0) {  // fold identity (empty-chunk semantics)
        *(T*)out_host = RedIdent<T>::get(redop);
        return 0;
    }
    bool v4 = reduce_v4();
    uint64_t want = (n / (v4 ? 4 : 2) + RTPB - 1) / RTPB;
    int g = reduce_grid(want);
    int rc = ensure_partials(RMAXB * sizeof(double));
    if (rc) return rc;
    FlatArgs<T> a = {reduce_fused_on() && !v4, g, mapop, redop, src, n,
                     (T*)st().partials, (T*)st().red_host_dev, s};
    if (v4) {
        hipLaunchKernelGGL((reduce_stage1_v4<T>), dim3(g), dim3(RTPB),
                           0, s, mapop, redop, src, n, a.parts);
        DA_CHECK_HIP(hipGetLastError());
    } else if (mapop == DA_REDF_IDENTITY && redop == DA_RED_ADD)
        rc = launch_flat<T, DA_REDF_IDENTITY, DA_RED_ADD>(a);
    else if (mapop == DA_REDF_ABS2 && redop == DA_RED_ADD)
        rc = launch_flat<T, DA_REDF_ABS2, DA_RED_ADD>(a);
    else if (mapop == DA_REDF_ABS && redop == DA_RED_ADD)
        rc = launch_flat<T, DA_REDF_ABS, DA_RED_ADD>(a);
    else if (mapop == DA_REDF_IDENTITY && redop == DA_RED_MAX)
        rc = launch_flat<T, DA_REDF_IDENTITY, DA_RED_MAX>(a);
    else if (mapop == DA_REDF_IDENTITY && redop == DA_RED_MIN)
        rc = launch_flat<T, DA_REDF_IDENTITY, DA_RED_MIN>(a);
    else
        rc = launch_flat<T, -1, -1>(a);
    if (rc) return rc;
    if (!a.fused) {
        hipLaunchKernelGGL(reduce_stage2<T>, dim3(1), dim3(RTPB), 0, s,
                           redop, a.parts, g, a.out);
        DA_CHECK_HIP(hipGetLastError());
    }
    return reduce_result(out_host, sizeof(T), s, published_seq(a.fused));
}

// Exact predicate count: the 0/1 predicate of a T source is accumulated
// in int64_t (a float accumulator rounds above 2^24 / 2^53), then the
// block partials fold through the ordinary i64 stage 2.
template <typename T>
__device__ __forceinline__ int64_t predf(int mapop, T x) {
    switch (mapop) {
    case DA_REDF_ISNAN: return x != x ? 1 : 0;
    case DA_REDF_ISFINITE: return isfinite((double)x) ? 1 : 0;
    }
    return x != (T)0 ? 1 : 0;   // DA_REDF_NONZERO
}
template <>
__device__ __forceinline__ int64_t predf<int64_t>(int mapop, int64_t x) {
    return mapf(mapop, x);
}

template <typename T>
__global__ void count_stage1(int mapop, const T* __restrict__ src,
                             uint64_t n, int64_t* __restrict__ partials) {
    int64_t acc = grid_accumulate<2>(src, n, (int64_t)0,
        [=](int64_t a, T x) { return a + predf<T>(mapop, x); });
    acc = block_reduce(DA_RED_ADD, acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// single-launch count: count_stage1's loop, then the fan-in of
// reduce_fused on the int64 partials
template <typename T>
__global__ void count_fused(int mapop, const T* __restrict__ src, uint64_t n,
                            int64_t* partials, unsigned int* ticket,
                            unsigned int base, int64_t* out,
                            unsigned long long seq) {
    __shared__ int64_t sh[RTPB / 64 + 1];
    int64_t acc = grid_accumulate<2>(src, n, (int64_t)0,
        [=](int64_t a, T x) { return a + predf<T>(mapop, x); });
    acc = block_reduce_in((int)DA_RED_ADD, acc, sh);
    fanin_finish((int)DA_RED_ADD, acc, partials, ticket, base, out, seq,
                 sh);
}

template <typename T>
static int do_count(int mapop, const T* src, uint64_t n, int64_t* out_host,
                    hipStream_t s) {
    int g = reduce_grid((n / 2 + RTPB - 1) / RTPB);
    int rc = ensure_partials(RMAXB * sizeof(double));
    if (rc) return rc;
    int64_t* parts = (int64_t*)st().partials;
    int64_t* out = (int64_t*)st().red_host_dev;
    if (reduce_fused_on()) {
        rc = fanin_launch_seq(g, [&](unsigned int base,
                                     unsigned long long seq) {
            hipLaunchKernelGGL(count_fused<T>, dim3(g), dim3(RTPB), 0, s,
                               mapop, src, n, parts, st().red_ticket, base,
                               out, seq);
            return hipGetLastError();
        });
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(count_stage1<T>, dim3(g), dim3(RTPB), 0, s,
                           mapop, src, n, parts);
        DA_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(reduce_stage2<int64_t>, dim3(1), dim3(RTPB), 0, s,
                           (int)DA_RED_ADD, parts, g, out);
        DA_CHECK_HIP(hipGetLastError());
    }
    return reduce_result(out_host, sizeof(int64_t), s,
                         published_seq(reduce_fused_on()));
}

int launch_count(int mapop, const void* src, uint64_t n, int dtype,
                 int64_t* out_host, hipStream_t s) {
    if (mapop < DA_REDF_ISNAN || mapop > DA_REDF_NONZERO)
        return set_err(-3, "da_count: mapop %d is not a predicate", mapop);
    if (!out_host) return set_err(-3, "da_count: null out");
    if (dtype != DA_F64 && dtype != DA_F32 && dtype != DA_I64)
        return set_err(-3, "da_count: bad dtype %d", dtype);
    if (n == 0) { *out_host = 0; return 0; }
    switch (dtype) {
    case DA_F64: return do_count<double>(mapop, (const double*)src, n,
                                         out_host, s);
    case DA_F32: return do_count<float>(mapop, (const float*)src, n,
                                        out_host, s);
    }
    return do_count<int64_t>(mapop, (const int64_t*)src, n, out_host, s);
}

// ---- dims-reduction (mapreduce.jl:42-94: per-chunk mapreduce(dims=..))
// The chunk is viewed column-major as (inner, axis, outer):
// src[i + a*inner + o*inner*axis] -> dst[i + o*inner], reduced over a.
// Variant A (inner >= 64): one thread per (i,o), serial over axis —
// coalesced across inner.  Variant B (inner < 64): one 64-lane wave per
// (i,o), lanes stride the axis (coalesced along the axis), then a
// wavefront shuffle tree.
// MOP/ROP >= 0 are compile-time op constants (the switches fold, the
// same 2x-recovery trick as map_fixed_kernel); -1 defers to the runtime
// arguments (long-tail combos).
template <typename T, int MOP, int ROP>
__global__ void reduce_dims_threads(int mapop, int redop,
                                    const T* __restrict__ src,
                                    uint64_t inner, uint64_t axis,
                                    uint64_t outer, T* __restrict__ dst) {
    const int mop_ = MOP >= 0 ? MOP : mapop;
    const int rop_ = ROP >= 0 ? ROP : redop;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t total = inner * outer;
    for (uint64_t e = t; e < total; e += stride) {
        uint64_t i = e % inner, o = e / inner;
        const T* p = src + i + o * inner * axis;
        T acc = RedIdent<T>::get(rop_);
        for (uint64_t a = 0; a < axis; ++a)
            acc = red_comb(rop_, acc, mapf(mop_, p[a * inner]));
        dst[i + o * inner] = acc;
    }
}

template <typename T, int MOP, int ROP>
__global__ void reduce_dims_waves(int mapop, int redop,
                                  const T* __restrict__ src,
                                  uint64_t inner, uint64_t axis,
                                  uint64_t outer, T* __restrict__ dst) {
    const int mop_ = MOP >= 0 ? MOP : mapop;
    const int rop_ = ROP >= 0 ? ROP : redop;
    uint64_t wid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) / 64;
    int lane = threadIdx.x & 63;
    uint64_t total = inner * outer;
    for (uint64_t e = wid; e < total; e += nw) {
        uint64_t i = e % inner, o = e / inner;
        const T* p = src + i + o * inner * axis;
        T acc = RedIdent<T>::get(rop_);
        for (uint64_t a = lane; a < axis; a += 64)
            acc = red_comb(rop_, acc, mapf(mop_, p[a * inner]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            acc = red_comb(rop_, acc, (T)__shfl_down(acc, off, 64));
        if (lane == 0) dst[i + o * inner] = acc;
    }
}

// Variant C: one 256-thread block per output element — for few outputs
// over a long axis (e.g. sum(D, dims=2) of a square matrix), where the
// thread/wave variants leave the chip underfilled (measured 137 GB/s vs
// 3+ TB/s; profiles/r01_kernel_stats.md).
template <typename T, int MOP, int ROP>
__global__ void reduce_dims_blocks(int mapop, int redop,
                                   const T* __restrict__ src,
                                   uint64_t inner, uint64_t axis,
                                   uint64_t outer, T* __restrict__ dst) {
    const int mop_ = MOP >= 0 ? MOP : mapop;
    const int rop_ = ROP >= 0 ? ROP : redop;
    uint64_t total = inner * outer;
    for (uint64_t e = blockIdx.x; e < total; e += gridDim.x) {
        uint64_t i = e % inner, o = e / inner;
        const T* p = src + i + o * inner * axis;
        T acc = RedIdent<T>::get(rop_);
        for (uint64_t a = threadIdx.x; a < axis; a += blockDim.x)
            acc = red_comb(rop_, acc, mapf(mop_, p[a * inner]));
        acc = block_reduce(rop_, acc);
        if (threadIdx.x == 0) dst[i + o * inner] = acc;
        __syncthreads();   // LDS in block_reduce reused next iteration
    }
}

// Variant D: few outputs, LARGE inner (e.g. sum(8192x8192, dims=2)):
// split the axis into NB column slices; each block walks a row tile of
// its slice with fully coalesced reads (consecutive threads =
// consecutive rows), producing NB partial rows; a second kernel folds
// the NB partials per row.
template <typename T, int MOP, int ROP>
__global__ void reduce_dims_slices1(int mapop, int redop,
                                    const T* __restrict__ src,
                                    uint64_t inner, uint64_t axis,
                                    int nb, T* __restrict__ partials) {
    const int mop_ = MOP >= 0 ? MOP : mapop;
    const int rop_ = ROP >= 0 ? ROP : redop;
    uint64_t o = blockIdx.z;
    const T* base = src + o * inner * axis;
    uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= inner) return;
    uint64_t a0 = axis * blockIdx.y / nb;
    uint64_t a1 = axis * (blockIdx.y + 1) / nb;
    T acc = RedIdent<T>::get(rop_);
    for (uint64_t a = a0; a < a1; ++a)
        acc = red_comb(rop_, acc, mapf(mop_, base[row + a * inner]));
    partials[(o * nb + blockIdx.y) * inner + row] = acc;
}

template <typename T>
__global__ void reduce_dims_slices2(int redop, const T* __restrict__ partials,
                                    uint64_t inner, int nb,
                                    T* __restrict__ dst, uint64_t outer) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = e; t < inner * outer; t += stride) {
        uint64_t row = t % inner, o = t / inner;
        T acc = RedIdent<T>::get(redop);
        for (int b = 0; b < nb; ++b)
            acc = red_comb(redop, acc,
                           partials[(o * nb + b) * inner + row]);
        dst[row + o * inner] = acc;
    }
}

// Host-only variant choice of the dims-reduce dispatcher (exported as
// dbg_reduce_dims_variant so tests can pin which kernel a shape reaches).
int reduce_dims_variant(uint64_t inner, uint64_t axis, uint64_t outer) {
    uint64_t total = inner * outer;
    if (total < 262144 && inner >= 64 && axis >= 64 && outer <= 64)
        return DA_DIMS_SLICES;   // few outputs, large inner, long axis
    if (total >= 262144 && inner >= 64)
        return DA_DIMS_THREADS;  // plenty of outputs, coalesced across inner
    if (inner < 64 && axis >= 64 && total >= 16384)
        return DA_DIMS_WAVES;    // inner tiny: lanes stride the axis
    return DA_DIMS_BLOCKS;       // few outputs / long axis
}

template <typename T, int MOP, int ROP>
static int do_reduce_dims_t(int mapop, int redop, const T* src,
                            uint64_t inner, uint64_t axis, uint64_t outer,
                            T* dst, hipStream_t s) {
    uint64_t total = inner * outer;
    if (total == 0) return 0;
    // axis == 0 still runs: the loop body never executes and dst gets
    // the fold identity.
    const int variant = reduce_dims_variant(inner, axis, outer);
    if (variant == DA_DIMS_SLICES) {
        // fill ~2048 workgroups: (inner/256 row tiles) x nb slices
        uint64_t row_tiles = (inner + RTPB - 1) / RTPB;
        int nb = (int)(2048 / row_tiles);
        if (nb < 1) nb = 1;
        if (nb > 64) nb = 64;
        if ((uint64_t)nb > axis) nb = (int)axis;
        int rc = ensure_partials((uint64_t)nb * inner * outer * sizeof(T));
        if (rc) return rc;
        T* parts = (T*)st().partials;
        dim3 g((inner + RTPB - 1) / RTPB, nb, outer);
        hipLaunchKernelGGL((reduce_dims_slices1<T, MOP, ROP>), g,
                           dim3(RTPB), 0, s,
                           mapop, redop, src, inner, axis, nb, parts);
        DA_CHECK_HIP(hipGetLastError());
        uint64_t want = (total + RTPB - 1) / RTPB;
        int g2 = (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
        hipLaunchKernelGGL(reduce_dims_slices2<T>, dim3(g2), dim3(RTPB), 0,
                           s, redop, parts, inner, nb, dst, outer);
        DA_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (variant == DA_DIMS_THREADS) {
        // plenty of outputs, coalesced across inner: thread-per-output
        uint64_t want = (total + RTPB - 1) / RTPB;
        int g = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
        hipLaunchKernelGGL((reduce_dims_threads<T, MOP, ROP>), dim3(g),
                           dim3(RTPB), 0,
                           s, mapop, redop, src, inner, axis, outer, dst);
    } else if (variant == DA_DIMS_WAVES) {
        // inner tiny (reduce over leading dim): wave-per-output, lanes
        // stride the axis (coalesced along the axis)
        uint64_t want = (total * 64 + RTPB - 1) / RTPB;
        int g = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
        hipLaunchKernelGGL((reduce_dims_waves<T, MOP, ROP>), dim3(g),
                           dim3(RTPB), 0,
                           s, mapop, redop, src, inner, axis, outer, dst);
    } else {
        // few outputs / long axis: block-per-output
        int g = (int)(total < 1 ? 1 : (total > 8192 ? 8192 : total));
        hipLaunchKernelGGL((reduce_dims_blocks<T, MOP, ROP>), dim3(g),
                           dim3(RTPB), 0,
                           s, mapop, redop, src, inner, axis, outer, dst);
    }
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

// hot (mapop, redop) combos get constant-folded instantiations — the
// dims-reduce analog of the map_fixed 2x recovery; everything else
// rides the runtime-switch fallback.
template <typename T>
static int do_reduce_dims(int mapop, int redop, const T* src,
                          uint64_t inner, uint64_t axis, uint64_t outer,
                          T* dst, hipStream_t s) {
    if (redop == DA_RED_ADD) {
        if (mapop == DA_REDF_IDENTITY)
            return do_reduce_dims_t<T, DA_REDF_IDENTITY, DA_RED_ADD>(
                mapop, redop, src, inner, axis, outer, dst, s);
        if (mapop == DA_REDF_ABS2)
            return do_reduce_dims_t<T, DA_REDF_ABS2, DA_RED_ADD>(
                mapop, redop, src, inner, axis, outer, dst, s);
    }
    if (redop == DA_RED_MAX && mapop == DA_REDF_IDENTITY)
        return do_reduce_dims_t<T, DA_REDF_IDENTITY, DA_RED_MAX>(
            mapop, redop, src, inner, axis, outer, dst, s);
    if (redop == DA_RED_MIN && mapop == DA_REDF_IDENTITY)
        return do_reduce_dims_t<T, DA_REDF_IDENTITY, DA_RED_MIN>(
            mapop, redop, src, inner, axis, outer, dst, s);
    return do_reduce_dims_t<T, -1, -1>(mapop, redop, src, inner, axis,
                                       outer, dst, s);
}

int launch_reduce_dims(int mapop, int redop, const void* src,
                       uint64_t inner, uint64_t axis, uint64_t outer,
                       int dtype, void* dst, hipStream_t s) {
    if (mapop < 0 || mapop > DA_REDF_NONZERO || redop < 0 || redop > DA_RED_MAX)
        return set_err(-3, "da_reduce_dims: bad op (%d,%d)", mapop, redop);
    switch (dtype) {
    case DA_F64: return do_reduce_dims<double>(mapop, redop,
        (const double*)src, inner, axis, outer, (double*)dst, s);
    case DA_F32: return do_reduce_dims<float>(mapop, redop,
        (const float*)src, inner, axis, outer, (float*)dst, s);
    case DA_I64: return do_reduce_dims<int64_t>(mapop, redop,
        (const int64_t*)src, inner, axis, outer, (int64_t*)dst, s);
    }
    return set_err(-3, "da_reduce_dims: bad dtype %d", dtype);
}

int launch_reduce(int mapop, int redop, const void* src, uint64_t n,
                  int dtype, void* out_host, hipStream_t s) {
    if (mapop < 0 || mapop > DA_REDF_NONZERO || redop < 0 || redop > DA_RED_MAX)
        return set_err(-3, "da_reduce: bad op (%d,%d)", mapop, redop);
    switch (dtype) {
    case DA_F64: return do_reduce<double>(mapop, redop, (const double*)src,
                                          n, out_host, s);
    case DA_F32: return do_reduce<float>(mapop, redop, (const float*)src,
                                         n, out_host, s);
    case DA_I64: return do_reduce<int64_t>(mapop, redop, (const int64_t*)src,
                                           n, out_host, s);
    }
    return set_err(-3, "da_reduce: bad dtype %d", dtype);
}

// reduce_stage2 for callers outside this file (the expression reduce under
// DA_RED_FUSED=0): one block folds the g partials of `dtype` in
// st().partials into the pinned slot.
int reduce_stage2_launch(int redop, int g, int dtype, hipStream_t s) {
    switch (dtype) {
    case DA_F64:
        hipLaunchKernelGGL(reduce_stage2<double>, dim3(1), dim3(RTPB), 0, s,
                           redop, (const double*)st().partials, g,
                           (double*)st().red_host_dev);
        break;
    case DA_F32:
        hipLaunchKernelGGL(reduce_stage2<float>, dim3(1), dim3(RTPB), 0, s,
                           redop, (const float*)st().partials, g,
                           (float*)st().red_host_dev);
        break;
    default:
        hipLaunchKernelGGL(reduce_stage2<int64_t>, dim3(1), dim3(RTPB), 0, s,
                           redop, (const int64_t*)st().partials, g,
                           (int64_t*)st().red_host_dev);
    }
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

// DA_RED_SPIN_US: how long reduce_result polls the pinned slot before it
// falls back to the stream sync (read once; default 2000; 0 = never poll).
static uint64_t red_spin_us() {
    static int64_t v = -1;
    if (v < 0) {
        const char* e = getenv("DA_RED_SPIN_US");
        v = e ? atoll(e) : 2000;
        if (v < 0) v = 2000;
    }
    return (uint64_t)v;
}

static uint64_t g_red_polled = 0, g_red_synced = 0;

void reduce_waits(uint64_t* polled, uint64_t* synced) {
    if (polled) *polled = g_red_polled;
    if (synced) *synced = g_red_synced;
}
void reduce_waits_reset() { g_red_polled = g_red_synced = 0; }

// Returns the result of the reduce just launched on `s`.  seq != 0: a
// single-launch kernel publishes {value, seq} into the pinned slot
// (publish_result), so the host watches the slot itself for up to
// DA_RED_SPIN_US and, when seq arrives, returns WITHOUT a runtime call:
// the stream is then NOT known to be drained (only this kernel's reads of
// its source and its result store are known to be done).  Budget spent,
// DA_RED_SPIN_US=0, or seq == 0 (the two-kernel path, which publishes no
// sequence): the stream sync, after which the slot holds the result; a
// kernel that faulted never publishes and its error comes back here.
int reduce_result(void* out_host, size_t bytes, hipStream_t s,
                  uint64_t seq) {
    const RedSlot* slot = (const RedSlot*)st().red_host;
    const uint64_t budget = seq ? red_spin_us() : 0;
    if (budget && red_wait(slot, seq, budget, out_host, bytes)) {
        ++g_red_polled;
        return 0;
    }
    DA_CHECK_HIP(hipStreamSynchronize(s));
    if (seq && __atomic_load_n(&slot->seq, __ATOMIC_ACQUIRE) != seq)
        return set_err(-6, "flat reduce: the stream drained but the result "
                       "slot holds sequence %llu, not %llu",
                       (unsigned long long)__atomic_load_n(
                           &slot->seq, __ATOMIC_RELAXED),
                       (unsigned long long)seq);
    memcpy(out_host, slot->value, bytes);
    ++g_red_synced;
    return 0;
}

} // namespace da
