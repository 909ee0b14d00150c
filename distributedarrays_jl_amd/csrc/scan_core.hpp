// scan_core.hpp — device-only primitives of the inclusive prefix scan
// (kernels_scan.hip): the 64-lane wave scan, the 256-thread tile scans
// with a running carry, and the contiguous-range walker built from them.
// The combiner, the identities and the publish/ticket protocol are the
// flat reduce's own (reduce_core.hpp), so min/max propagate NaN and i64
// wraps exactly as every reduction of the library does.
//
// No identity ever enters a result: lanes combine only with EARLIER lanes
// (guarded shuffles), and "is there a prefix yet" is a flag next to the
// running carry, not a neutral element.  So with no carry the first
// element of a line is stored bit for bit (-0.0, a NaN payload), and the
// padding of a partial tile, which sits BEHIND the valid lanes, never
// reaches one.
//
// dst == src: every routine loads all of a thread's elements of a tile
// before it stores any of them, and a thread stores exactly the elements
// it loaded, so an in-place scan never reads a value it has overwritten.
// Hence no __restrict__ on src / dst anywhere in this file.
#pragma once
#include "reduce_core.hpp"

namespace da {

constexpr int SCAN_TILE = 2048;            // elements per full tile, any dtype
constexpr int SCAN_LDS = SCAN_TILE / 64;   // wave totals of one tile (W = 1)

// Identity for the FOLD of a span (launch 1 of the spans family), where
// threads without elements need one: RedIdent, but -0.0 for a float sum,
// the only exact additive identity (-0.0 + x == x for every x, while
// +0.0 + -0.0 == +0.0).
template <typename T>
__device__ __forceinline__ T scan_ident(int redop) {
    if (redop == DA_RED_ADD) return (T)(-0.0f);
    return RedIdent<T>::get(redop);
}
template <>
__device__ __forceinline__ int64_t scan_ident<int64_t>(int redop) {
    return RedIdent<int64_t>::get(redop);
}

// Running state of one block walking a line: the prefix of everything
// before the next tile (valid iff `have`) and the LDS buffer parity.
template <typename T> struct ScanState {
    T carry;
    bool have;
    int par;
};

template <typename T>
__device__ __forceinline__ T wave_scan_incl(int redop, T v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        T u = (T)__shfl_up(v, off, 64);
        if (lane >= off) v = red_comb(redop, u, v);
    }
    return v;
}

template <typename T, int W> struct ScanVec {
    using type = T __attribute__((ext_vector_type(W)));
};
template <typename T> struct ScanVec<T, 1> {
    struct type {
        T x;
        __device__ __forceinline__ T& operator[](int) { return x; }
    };
};

// `lds`: 2 * SCAN_LDS elements, double-buffered by st.par so that ONE
// barrier per tile suffices: a wave can write buffer p again only after
// the barrier of the tile in between, which every wave reaches after its
// reads of buffer p.
//
// Partial tile: the first cnt (1..256) elements at src, one per thread.
template <typename T>
__device__ __forceinline__ void scan_tile_part(int redop, const T* src,
                                               T* dst, int cnt,
                                               ScanState<T>& st, T* lds) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool valid = t < cnt;
    T v = valid ? src[t] : (T)0;
    v = wave_scan_incl(redop, v, lane);
    T* L = lds + st.par * SCAN_LDS;
    st.par ^= 1;
    // the wave's total is its LAST VALID lane's prefix
    int last = cnt - 1 - wave * 64;
    if (last > 63) last = 63;
    if (lane == last) L[wave] = v;
    __syncthreads();
    const int nw = (cnt + 63) >> 6;
    T run = st.carry, pre = st.carry;
    bool have = st.have, hp = st.have;
#pragma unroll
    for (int w = 0; w < RTPB / 64; ++w) {
        if (w == wave) { pre = run; hp = have; }
        if (w < nw) {
            T x = L[w];
            run = have ? red_comb(redop, run, x) : x;
            have = true;
        }
    }
    if (valid) dst[t] = hp ? red_comb(redop, pre, v) : v;
    st.carry = run;
    st.have = true;
}

// Full tile of SCAN_TILE elements as U rows of RTPB W-wide vectors
// (W * sizeof(T) == 16: one dwordx4 per lane and row, all U loads issued
// before the first use).  src and dst must be W*sizeof(T)-aligned.
template <typename T, int W, int U>
__device__ __forceinline__ void scan_tile_full(int redop, const T* src,
                                               T* dst, ScanState<T>& st,
                                               T* lds) {
    static_assert(RTPB * W * U == SCAN_TILE, "tile shape");
    using V = typename ScanVec<T, W>::type;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    V v[U];
    T tot[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        v[u] = reinterpret_cast<const V*>(src)[u * RTPB + t];
    T* L = lds + st.par * SCAN_LDS;
    st.par ^= 1;
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 1; k < W; ++k)
            v[u][k] = red_comb(redop, (T)v[u][k - 1], (T)v[u][k]);
        tot[u] = wave_scan_incl(redop, (T)v[u][W - 1], lane);
        if (lane == 63) L[u * (RTPB / 64) + wave] = tot[u];
    }
    __syncthreads();
    T run = st.carry;
    bool have = st.have;
    T pre[U];
    bool hp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int w = 0; w < RTPB / 64; ++w) {
            if (w == wave) { pre[u] = run; hp[u] = have; }
            T x = L[u * (RTPB / 64) + w];
            run = have ? red_comb(redop, run, x) : x;
            have = true;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // prefix of everything before this thread's W elements
        T ex = (T)__shfl_up(tot[u], 1, 64);
        T p = hp[u] ? (lane > 0 ? red_comb(redop, pre[u], ex) : pre[u]) : ex;
        if (hp[u] || lane > 0) {
#pragma unroll
            for (int k = 0; k < W; ++k)
                v[u][k] = red_comb(redop, p, (T)v[u][k]);
        }
        reinterpret_cast<V*>(dst)[u * RTPB + t] = v[u];
    }
    st.carry = run;
    st.have = true;
}

// Inclusive scan of the n contiguous elements at src into dst by one
// block, continuing st.  16-byte vectors when src and dst are equally
// misaligned (a scalar head brings both to 16 bytes), scalar rows
// otherwise; then a scalar tail.  All control flow is block-uniform.
template <typename T>
__device__ __forceinline__ void scan_range(int redop, const T* src, T* dst,
                                           uint64_t n, ScanState<T>& st,
                                           T* lds) {
    constexpr int W = 16 / (int)sizeof(T);
    uint64_t pos = 0;
    const uint64_t sa = (uint64_t)src, da_ = (uint64_t)dst;
    if (((sa ^ da_) & 15) == 0) {
        uint64_t h = ((16 - (sa & 15)) & 15) / sizeof(T);
        if (h > n) h = n;
        if (h) {
            scan_tile_part(redop, src, dst, (int)h, st, lds);
            pos = h;
        }
        for (; pos + SCAN_TILE <= n; pos += SCAN_TILE)
            scan_tile_full<T, W, SCAN_TILE / (RTPB * W)>(
                redop, src + pos, dst + pos, st, lds);
    } else {
        for (; pos + SCAN_TILE <= n; pos += SCAN_TILE)
            scan_tile_full<T, 1, SCAN_TILE / RTPB>(redop, src + pos,
                                                   dst + pos, st, lds);
    }
    for (; pos < n; pos += RTPB) {
        uint64_t c = n - pos;
        scan_tile_part(redop, src + pos, dst + pos,
                       (int)(c < (uint64_t)RTPB ? c : (uint64_t)RTPB), st,
                       lds);
    }
}

// Fold of n contiguous elements by one block (launch 1 of the spans
// family): thread-strided 16-byte loads behind a scalar head, scalar
// tail, then the block tree.  The total is valid in thread 0.
template <typename T>
__device__ __forceinline__ T fold_range(int redop, const T* src, uint64_t n,
                                        T* lds) {
    constexpr int W = 16 / (int)sizeof(T);
    using V = typename ScanVec<T, W>::type;
    const uint64_t t = threadIdx.x;
    T acc = scan_ident<T>(redop);
    uint64_t h = ((16 - ((uint64_t)src & 15)) & 15) / sizeof(T);
    if (h > n) h = n;
    if (t < h) acc = red_comb(redop, acc, src[t]);
    const uint64_t nv = (n - h) / W;
    const V* sv = reinterpret_cast<const V*>(src + h);
    // 4 independent loads in flight per thread: a span is a few dozen
    // rows, so one load per trip leaves the block latency-bound
    uint64_t j = t;
    for (; j + 3 * RTPB < nv; j += 4 * RTPB) {
        V v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = sv[j + q * RTPB];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < W; ++k)
                acc = red_comb(redop, acc, (T)v[q][k]);
    }
    for (; j < nv; j += RTPB) {
        V v = sv[j];
#pragma unroll
        for (int k = 0; k < W; ++k) acc = red_comb(redop, acc, (T)v[k]);
    }
    for (j = h + nv * W + t; j < n; j += RTPB)
        acc = red_comb(redop, acc, src[j]);
    return block_reduce_in(redop, acc, lds);
}

} // namespace da
