// kernels_compact.hip — stream compaction (filter / findall / D[mask]) and
// its inverse (D[mask] = v) of a local chunk, for gfx950.
//
// Three stream-ordered steps, each a plain launch on the rank's stream:
//
//  1. counts   one workgroup per tile of DA_COMPACT_TILE mask elements
//              (a bounded grid strides over the tiles) writes the tile's
//              number of true elements as one int64_t into the scratch.
//  2. scan     the library's own inclusive scan (launch_scan, ADD, i64,
//              in place) turns the counts into tile offsets: tile t starts
//              at incl[t - 1].
//  3. scatter  every workgroup re-reads its mask tile, ranks its true
//              lanes and moves the elements.
//
// NO BLOCK EVER WAITS FOR ANOTHER BLOCK (the rule of kernels_scan.hip): no
// look-back, no flag spin, and no global atomic cursor either — a cursor
// would hand out positions in arrival order and the output must be stable.
// The price is a second read of the mask.
//
// A tile is CROWS rows of RTPB elements; element (row, wave, lane) sits at
// tile*TILE + row*RTPB + wave*64 + lane, which is memory order.  So every
// row is one coalesced load per wave, the rank of a true lane inside its
// 64-lane row is the popcount of the ballot bits below it, and the
// CROWS * RTPB/64 row totals, scanned in (row, wave) order, give the rest:
// kept neighbours land on adjacent destinations.
//
// Mask truth is element != 0 in the mask's own dtype: NaN is true, -0.0 is
// false (the DA_REDF_NONZERO rule of da_count).  Data moves as raw 4- or
// 8-byte words.  Every index and position is 64-bit.
#include "common.hpp"
#include "reduce_core.hpp"
#include "scan_core.hpp"

namespace da {

constexpr int CTILE = DA_COMPACT_TILE;
constexpr int CROWS = CTILE / RTPB;            // 8 rows of 256
constexpr int CWAVES = RTPB / 64;              // 4 waves per row
constexpr int CSLOTS = CROWS * CWAVES;         // 32 row totals per tile
constexpr uint64_t CGRID = 65536;              // blocks per launch, at most
static_assert(CROWS * RTPB == CTILE, "tile shape");

enum { C_COPY = 0, C_IOTA = 1, C_EXPAND = 2 };

// One tile's mask as CROWS predicates per thread; positions >= n are false.
template <typename M>
__device__ __forceinline__ void load_preds(const M* mask, uint64_t base,
                                           uint64_t n, bool* p) {
    const uint64_t i0 = base + threadIdx.x;
    M m[CROWS];
    if (base + CTILE <= n) {
#pragma unroll
        for (int r = 0; r < CROWS; ++r) m[r] = mask[i0 + r * RTPB];
    } else {
#pragma unroll
        for (int r = 0; r < CROWS; ++r) {
            const uint64_t i = i0 + r * RTPB;
            m[r] = i < n ? mask[i] : (M)0;
        }
    }
#pragma unroll
    for (int r = 0; r < CROWS; ++r) p[r] = m[r] != (M)0;
}

// Step 1.  lds is double-buffered by parity, so one barrier per tile is
// enough: a wave writes buffer p again only after the barrier of the tile
// in between, which every wave reaches after its reads of buffer p.
template <typename M>
__global__ void __launch_bounds__(RTPB)
compact_counts(const M* mask, uint64_t n, uint64_t ntiles, int64_t* counts) {
    __shared__ int lds[2][CWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        bool p[CROWS];
        load_preds(mask, tile * CTILE, n, p);
        int c = 0;
#pragma unroll
        for (int r = 0; r < CROWS; ++r) c += __popcll(__ballot(p[r]));
        if (lane == 0) lds[par][wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
#pragma unroll
            for (int w = 0; w < CWAVES; ++w) tot += lds[par][w];
            counts[tile] = tot;
        }
        par ^= 1;
    }
}

// Step 3.  W is the raw data word (4 or 8 bytes), M the mask's dtype.
//   C_COPY    dst[j] = src[i]             for the j-th true i, j < cap
//   C_IOTA    dst[j] = index_base + i     (W is 8 bytes)
//   C_EXPAND  dst[i] = bcast ? src[0] : src[j]
// dst == mask (C_EXPAND, equal element sizes): a thread loads all its mask
// elements of a tile before it stores any, and stores only at positions it
// loaded, so no thread reads a mask element another one has overwritten.
// Hence no __restrict__ here.
template <typename W, typename M, int MODE>
__global__ void __launch_bounds__(RTPB)
compact_scatter(W* dst, const W* src, uint64_t cap, const M* mask,
                uint64_t n, uint64_t ntiles, const int64_t* incl,
                int64_t index_base, int bcast) {
    __shared__ int lds[2][CSLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below_mask = (1ull << lane) - 1ull;
    W one = (W)0;
    if (MODE == C_EXPAND && bcast && cap) one = src[0];
    int par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * CTILE;
        bool p[CROWS];
        load_preds(mask, base, n, p);
        int below[CROWS];
        int* L = lds[par];
        par ^= 1;
#pragma unroll
        for (int r = 0; r < CROWS; ++r) {
            const unsigned long long b = __ballot(p[r]);
            below[r] = __popcll(b & below_mask);
            if (lane == 0) L[r * CWAVES + wave] = __popcll(b);
        }
        __syncthreads();
        // exclusive scan of the row totals in (row, wave) order
        int pre[CROWS];
        int run = 0;
#pragma unroll
        for (int k = 0; k < CSLOTS; ++k) {
            if ((k % CWAVES) == wave) pre[k / CWAVES] = run;
            run += L[k];
        }
        const uint64_t off = tile ? (uint64_t)incl[tile - 1] : 0ull;
#pragma unroll
        for (int r = 0; r < CROWS; ++r) {
            if (!p[r]) continue;
            const uint64_t j = off + (uint64_t)(pre[r] + below[r]);
            if (j >= cap) continue;
            const uint64_t i = base + (uint64_t)(r * RTPB) + threadIdx.x;
            if (MODE == C_COPY) dst[j] = src[i];
            else if (MODE == C_IOTA)
                dst[j] = (W)((uint64_t)index_base + i);
            else dst[i] = bcast ? one : src[j];
        }
    }
}

static bool ranges_overlap(const void* a, uint64_t na, const void* b,
                           uint64_t nb) {
    uint64_t x = (uint64_t)a, y = (uint64_t)b;
    return na && nb && x < y + nb && y < x + na;
}

// Host-only argument checks (no GPU work, no da_init needed):
// 0 = launch, 1 = nothing to do, < 0 = error.
int compact_check(const void* dst, uint64_t dst_cap, const void* src,
                  int dtype, const void* mask, int mask_dtype, uint64_t n) {
    // findall (src == NULL) writes int64_t whatever dtype says
    const uint64_t esz = src ? dtype_size(dtype) : 8;
    if (!dtype_size(dtype))
        return set_err(-3, "da_compact: bad dtype %d", dtype);
    const uint64_t msz = dtype_size(mask_dtype);
    if (!msz) return set_err(-3, "da_compact: bad mask_dtype %d", mask_dtype);
    uint64_t sbytes, mbytes, dbytes;
    if (__builtin_mul_overflow(n, esz, &sbytes) ||
        __builtin_mul_overflow(n, msz, &mbytes) ||
        __builtin_mul_overflow(dst_cap, esz, &dbytes))
        return set_err(-3, "da_compact: size n=%llu dst_cap=%llu overflows "
                       "64 bits", (unsigned long long)n,
                       (unsigned long long)dst_cap);
    if (n == 0) return 1;
    if (!mask) return set_err(-3, "da_compact: null mask");
    if (dst_cap == 0) return 1;
    if (!dst) return set_err(-3, "da_compact: null dst");
    if (src && ranges_overlap(dst, dbytes, src, sbytes))
        return set_err(-3, "da_compact: dst overlaps src");
    if (ranges_overlap(dst, dbytes, mask, mbytes))
        return set_err(-3, "da_compact: dst overlaps mask");
    return 0;
}

int expand_check(const void* dst, int dtype, const void* mask,
                 int mask_dtype, uint64_t n, const void* src,
                 uint64_t src_n, int src_broadcast) {
    const uint64_t esz = dtype_size(dtype);
    if (!esz) return set_err(-3, "da_expand: bad dtype %d", dtype);
    const uint64_t msz = dtype_size(mask_dtype);
    if (!msz) return set_err(-3, "da_expand: bad mask_dtype %d", mask_dtype);
    uint64_t dbytes, mbytes, sbytes;
    if (__builtin_mul_overflow(n, esz, &dbytes) ||
        __builtin_mul_overflow(n, msz, &mbytes) ||
        __builtin_mul_overflow(src_n, esz, &sbytes))
        return set_err(-3, "da_expand: size n=%llu src_n=%llu overflows "
                       "64 bits", (unsigned long long)n,
                       (unsigned long long)src_n);
    if (n == 0) return 1;
    if (!dst || !mask) return set_err(-3, "da_expand: null dst or mask");
    if (src_n == 0) return 1;
    if (!src) return set_err(-3, "da_expand: null src");
    if (src_broadcast) sbytes = esz;
    // dst == mask is in place only when thread i's mask element IS its dst
    // element, i.e. with equal element sizes
    if (!(dst == mask && esz == msz) &&
        ranges_overlap(dst, dbytes, mask, mbytes))
        return set_err(-3, "da_expand: dst overlaps mask without being "
                       "equal to it (same element size)");
    if (ranges_overlap(dst, dbytes, src, sbytes))
        return set_err(-3, "da_expand: dst overlaps src");
    return 0;
}

template <typename W, typename M>
static int run_steps(int mode, W* dst, const W* src, uint64_t cap,
                     const M* mask, uint64_t n, int64_t index_base,
                     int bcast, hipStream_t s) {
    const uint64_t ntiles = (n + CTILE - 1) / CTILE;
    const int g = (int)(ntiles > CGRID ? CGRID : ntiles);
    int64_t* counts = nullptr;
    if (ntiles > 1) {   // a single tile starts at 0: no offsets needed
        uint64_t bytes;
        if (__builtin_mul_overflow(ntiles, (uint64_t)sizeof(int64_t),
                                   &bytes))
            return set_err(-3, "da_compact: tile count overflows");
        int rc = ensure_scratch(bytes);
        if (rc) return rc;
        counts = (int64_t*)st().scratch;
        hipLaunchKernelGGL((compact_counts<M>), dim3(g), dim3(RTPB), 0, s,
                           mask, n, ntiles, counts);
        DA_CHECK_HIP(hipGetLastError());
        rc = launch_scan(DA_RED_ADD, counts, counts, 1, ntiles, 1, DA_I64,
                         nullptr, s);
        if (rc) return rc;
    }
#define DA_SCATTER(MODE)                                                    \
    hipLaunchKernelGGL((compact_scatter<W, M, MODE>), dim3(g), dim3(RTPB),  \
                       0, s, dst, src, cap, mask, n, ntiles,                \
                       (const int64_t*)counts, index_base, bcast)
    if (mode == C_COPY) DA_SCATTER(C_COPY);
    else if (mode == C_EXPAND) DA_SCATTER(C_EXPAND);
    else if constexpr (sizeof(W) == 8) DA_SCATTER(C_IOTA);
    else return set_err(-3, "da_compact: index output needs 8-byte words");
#undef DA_SCATTER
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename W>
static int by_mask(int mode, void* dst, const void* src, uint64_t cap,
                   const void* mask, int mask_dtype, uint64_t n,
                   int64_t index_base, int bcast, hipStream_t s) {
    switch (mask_dtype) {
    case DA_F64:
        return run_steps<W, double>(mode, (W*)dst, (const W*)src, cap,
                                    (const double*)mask, n, index_base,
                                    bcast, s);
    case DA_F32:
        return run_steps<W, float>(mode, (W*)dst, (const W*)src, cap,
                                   (const float*)mask, n, index_base, bcast,
                                   s);
    case DA_I64:
        return run_steps<W, int64_t>(mode, (W*)dst, (const W*)src, cap,
                                     (const int64_t*)mask, n, index_base,
                                     bcast, s);
    }
    return set_err(-3, "bad mask_dtype %d", mask_dtype);
}

int launch_compact(void* dst, uint64_t dst_cap, const void* src, int dtype,
                   const void* mask, int mask_dtype, uint64_t n,
                   int64_t index_base, hipStream_t s) {
    if (!src)
        return by_mask<uint64_t>(C_IOTA, dst, nullptr, dst_cap, mask,
                                 mask_dtype, n, index_base, 0, s);
    if (dtype_size(dtype) == 4)
        return by_mask<uint32_t>(C_COPY, dst, src, dst_cap, mask, mask_dtype,
                                 n, 0, 0, s);
    return by_mask<uint64_t>(C_COPY, dst, src, dst_cap, mask, mask_dtype, n,
                             0, 0, s);
}

int launch_expand(void* dst, int dtype, const void* mask, int mask_dtype,
                  uint64_t n, const void* src, uint64_t src_n,
                  int src_broadcast, hipStream_t s) {
    const int bc = src_broadcast ? 1 : 0;
    // a broadcast source reaches every true position (src_n > 0 here)
    if (bc) src_n = ~0ull;
    if (dtype_size(dtype) == 4)
        return by_mask<uint32_t>(C_EXPAND, dst, src, src_n, mask, mask_dtype,
                                 n, 0, bc, s);
    return by_mask<uint64_t>(C_EXPAND, dst, src, src_n, mask, mask_dtype, n,
                             0, bc, s);
}

} // namespace da
