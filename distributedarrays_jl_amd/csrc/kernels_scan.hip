// kernels_scan.hip — inclusive prefix scan (Base.accumulate / cumsum /
// cumprod) of a local chunk viewed column-major as (inner, axis, outer),
// along `axis`, for gfx950.  Three kernel families (scan_variant):
//
//  cols   inner > 1: one thread per line (i, o), adjacent threads on
//         adjacent i, so every step along the axis is a coalesced row of
//         loads and stores; the running value stays in a register.
//  block  inner == 1, many lines (or short ones): one workgroup walks a
//         line in tiles of SCAN_TILE elements (scan_core.hpp).
//  spans  inner == 1, few long lines: each line is cut into g spans.
//         Launch 1 folds every span to one total; the last block to
//         arrive (the flat reduce's never-reset ticket) turns the g
//         totals of each line into inclusive span prefixes, in span
//         order.  Launch 2 scans every span as `block` does, starting
//         from carry (op) prefix of the spans before it.  Stream order
//         between the two launches is the only synchronisation.
//
// NO BLOCK EVER WAITS FOR ANOTHER BLOCK: no look-back, no flag spin, no
// grid barrier — the invariant reduce_core.hpp states for the fan-in.
// The spans family pays a second read of the source for it.
#include "common.hpp"
#include "scan_core.hpp"

namespace da {

constexpr uint64_t SCAN_BLOCK_LINES = 512;  // >= this many lines: block
constexpr uint64_t SCAN_GMAX = 2048;        // spans blocks per launch
constexpr int SCAN_CTPB = 64;               // cols: one wave per block
constexpr int SCAN_CUNROLL = 32;            // cols: loads in flight/thread

int scan_variant(uint64_t inner, uint64_t axis, uint64_t outer) {
    if (inner > 1) return DA_SCAN_COLS;
    if (outer >= SCAN_BLOCK_LINES || axis <= (uint64_t)SCAN_TILE)
        return DA_SCAN_BLOCK;
    return DA_SCAN_SPANS;
}

// B steps of one line: all B loads are issued before the first store, so
// they overlap even though dst may be src (a thread reads its own
// elements before it overwrites them).
template <typename T, int B>
__device__ __forceinline__ T cols_batch(int rop, const T* s, T* d,
                                        uint64_t inner, uint64_t a, T acc) {
    T x[B];
#pragma unroll
    for (int k = 0; k < B; ++k) x[k] = s[(a + k) * inner];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        acc = red_comb(rop, acc, x[k]);
        d[(a + k) * inner] = acc;
    }
    return acc;
}

// ROP >= 0 folds the op switch at compile time (the hot sum); -1 defers
// to the runtime argument, as in the reduce kernels.
template <typename T, int ROP>
__global__ void __launch_bounds__(SCAN_CTPB)
scan_cols(int redop, T* dst, const T* src, uint64_t inner, uint64_t axis,
          uint64_t outer, const T* carry) {
    const int rop = ROP >= 0 ? ROP : redop;
    const uint64_t total = inner * outer;
    const uint64_t stride = (uint64_t)gridDim.x * SCAN_CTPB;
    for (uint64_t e = (uint64_t)blockIdx.x * SCAN_CTPB + threadIdx.x;
         e < total; e += stride) {
        const uint64_t i = e % inner, o = e / inner;
        const uint64_t base = i + inner * axis * o;
        const T* s = src + base;
        T* d = dst + base;
        T acc = s[0];
        if (carry) acc = red_comb(rop, carry[e], acc);
        d[0] = acc;
        uint64_t a = 1;
        for (; a + SCAN_CUNROLL <= axis; a += SCAN_CUNROLL)
            acc = cols_batch<T, SCAN_CUNROLL>(rop, s, d, inner, a, acc);
        for (; a + 4 <= axis; a += 4)
            acc = cols_batch<T, 4>(rop, s, d, inner, a, acc);
        for (; a < axis; ++a) {
            acc = red_comb(rop, acc, s[a * inner]);
            d[a * inner] = acc;
        }
    }
}

template <typename T, int ROP>
__global__ void __launch_bounds__(RTPB)
scan_block(int redop, T* dst, const T* src, uint64_t axis, uint64_t lines,
           const T* carry) {
    const int rop = ROP >= 0 ? ROP : redop;
    __shared__ T lds[2 * SCAN_LDS];
    ScanState<T> st;
    st.par = 0;
    for (uint64_t l = blockIdx.x; l < lines; l += gridDim.x) {
        st.have = carry != nullptr;
        st.carry = carry ? carry[l] : (T)0;
        scan_range(rop, src + l * axis, dst + l * axis, axis, st, lds);
    }
}

// Launch 1 of spans.  Block b folds span b % g of line b / g (spans are
// `span` elements long, a multiple of SCAN_TILE; the last one of a line
// may be shorter, none is empty) and publishes the total; the last
// arriver scans each line's g totals in place, inclusively and in span
// order.  `totals` is deliberately not __restrict__/const: its loads
// must stay vector loads behind the acquire.
template <typename T, int ROP>
__global__ void __launch_bounds__(RTPB)
scan_spans_fold(int redop, const T* src, uint64_t axis, uint64_t span,
                unsigned int g, T* totals, unsigned int* ticket,
                unsigned int base) {
    const int rop = ROP >= 0 ? ROP : redop;
    __shared__ T lds[2 * SCAN_LDS];
    __shared__ unsigned int is_last;
    const uint64_t line = blockIdx.x / g, j = blockIdx.x % g;
    const uint64_t a0 = j * span;
    const uint64_t len = axis - a0 < span ? axis - a0 : span;
    T tot = fold_range(rop, src + line * axis + a0, len, lds);
    if (threadIdx.x == 0) {
        publish_partial(totals + blockIdx.x, tot);
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned int t = __hip_atomic_fetch_add(
            ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (t - base == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    // guide order: the fence, that lane's vmcnt wait, the barrier
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const unsigned int lines = gridDim.x / g;
    ScanState<T> st;
    st.par = 0;
    for (unsigned int l = 0; l < lines; ++l) {
        st.have = false;
        st.carry = (T)0;
        T* p = totals + (uint64_t)l * g;
        // in place: GMAX totals are one full tile, one barrier
        scan_range(rop, (const T*)p, p, (uint64_t)g, st, lds);
    }
}

// Launch 2 of spans: block b scans its span, starting from
// [carry[line] (op)] prefix of the spans before it.
template <typename T, int ROP>
__global__ void __launch_bounds__(RTPB)
scan_spans_apply(int redop, T* dst, const T* src, uint64_t axis,
                 uint64_t span, unsigned int g, const T* prefixes,
                 const T* carry) {
    const int rop = ROP >= 0 ? ROP : redop;
    __shared__ T lds[2 * SCAN_LDS];
    const uint64_t line = blockIdx.x / g, j = blockIdx.x % g;
    const uint64_t a0 = j * span;
    const uint64_t len = axis - a0 < span ? axis - a0 : span;
    ScanState<T> st;
    st.par = 0;
    st.have = carry != nullptr || j > 0;
    st.carry = carry ? carry[line] : (T)0;
    if (j > 0) {
        T p = prefixes[blockIdx.x - 1];
        st.carry = carry ? red_comb(rop, st.carry, p) : p;
    }
    const uint64_t off = line * axis + a0;
    scan_range(rop, src + off, dst + off, len, st, lds);
}

template <typename T, int ROP>
static int do_scan_t(int redop, T* dst, const T* src, uint64_t inner,
                     uint64_t axis, uint64_t outer, const T* carry,
                     hipStream_t s) {
    const int variant = scan_variant(inner, axis, outer);
    if (variant == DA_SCAN_COLS) {
        uint64_t want = (inner * outer + SCAN_CTPB - 1) / SCAN_CTPB;
        int g = (int)(want > (1u << 20) ? (1u << 20) : want);
        hipLaunchKernelGGL((scan_cols<T, ROP>), dim3(g), dim3(SCAN_CTPB), 0,
                           s, redop, dst, src, inner, axis, outer, carry);
        DA_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (variant == DA_SCAN_BLOCK) {
        int g = (int)(outer > 16384 ? 16384 : outer);
        hipLaunchKernelGGL((scan_block<T, ROP>), dim3(g), dim3(RTPB), 0, s,
                           redop, dst, src, axis, outer, carry);
        DA_CHECK_HIP(hipGetLastError());
        return 0;
    }
    // spans: outer < SCAN_BLOCK_LINES lines of more than one tile each
    uint64_t gmax = SCAN_GMAX / outer;   // >= 4
    uint64_t tiles = (axis + SCAN_TILE - 1) / SCAN_TILE;
    uint64_t span = (tiles + gmax - 1) / gmax * SCAN_TILE;
    unsigned int g = (unsigned int)((axis + span - 1) / span);
    int grid = (int)(g * outer);         // <= SCAN_GMAX <= RMAXB
    int rc = ensure_partials(RMAXB * sizeof(double));
    if (rc) return rc;
    T* totals = (T*)st().partials;
    rc = fanin_launch(grid, [&](unsigned int base) {
        hipLaunchKernelGGL((scan_spans_fold<T, ROP>), dim3(grid), dim3(RTPB),
                           0, s, redop, src, axis, span, g, totals,
                           st().red_ticket, base);
        return hipGetLastError();
    });
    if (rc) return rc;
    hipLaunchKernelGGL((scan_spans_apply<T, ROP>), dim3(grid), dim3(RTPB), 0,
                       s, redop, dst, src, axis, span, g, (const T*)totals,
                       carry);
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
static int do_scan(int redop, void* dst, const void* src, uint64_t inner,
                   uint64_t axis, uint64_t outer, const void* carry,
                   hipStream_t s) {
    if (redop == DA_RED_ADD)
        return do_scan_t<T, DA_RED_ADD>(redop, (T*)dst, (const T*)src, inner,
                                        axis, outer, (const T*)carry, s);
    return do_scan_t<T, -1>(redop, (T*)dst, (const T*)src, inner, axis,
                            outer, (const T*)carry, s);
}

static bool ranges_overlap(const void* a, uint64_t na, const void* b,
                           uint64_t nb) {
    uint64_t x = (uint64_t)a, y = (uint64_t)b;
    return x < y + nb && y < x + na;
}

// Host-only argument check of da_scan (no GPU work, no da_init needed):
// 0 = launch, 1 = nothing to do, < 0 = error.
int scan_check(int redop, const void* dst, const void* src, uint64_t inner,
               uint64_t axis, uint64_t outer, int dtype, const void* carry) {
    if (redop < DA_RED_ADD || redop > DA_RED_MAX)
        return set_err(-3, "da_scan: bad redop %d", redop);
    const uint64_t esz = dtype_size(dtype);
    if (!esz) return set_err(-3, "da_scan: bad dtype %d", dtype);
    uint64_t lines, n, bytes;
    if (__builtin_mul_overflow(inner, outer, &lines) ||
        __builtin_mul_overflow(lines, axis, &n) ||
        __builtin_mul_overflow(n, esz, &bytes))
        return set_err(-3, "da_scan: size (%llu, %llu, %llu) overflows "
                       "64 bits", (unsigned long long)inner,
                       (unsigned long long)axis, (unsigned long long)outer);
    if (n == 0) return 1;
    if (!dst || !src) return set_err(-3, "da_scan: null dst or src");
    bytes = n * esz;
    if (dst != src && ranges_overlap(dst, bytes, src, bytes))
        return set_err(-3, "da_scan: dst overlaps src without being equal "
                       "to it");
    if (carry && ranges_overlap(dst, bytes, carry, lines * esz))
        return set_err(-3, "da_scan: dst overlaps carry");
    return 0;
}

int launch_scan(int redop, void* dst, const void* src, uint64_t inner,
                uint64_t axis, uint64_t outer, int dtype, const void* carry,
                hipStream_t s) {
    switch (dtype) {
    case DA_F64: return do_scan<double>(redop, dst, src, inner, axis, outer,
                                        carry, s);
    case DA_F32: return do_scan<float>(redop, dst, src, inner, axis, outer,
                                       carry, s);
    case DA_I64: return do_scan<int64_t>(redop, dst, src, inner, axis, outer,
                                         carry, s);
    }
    return set_err(-3, "da_scan: bad dtype %d", dtype);
}

} // namespace da
