// kernels_index.hip — da_copy_nd: one N-D selection-to-selection copy
// between two column-major device buffers (strided / index-vector
// getindex, setindex! and view materialisation; the SubArray paths of
// src/darray.jl:584-610, :661, :679-687 of the reference).
//
// Per side and per dimension an index is affine (start + j*step) or an
// explicit int64 vector.  The host folds each side into
//     offset = base + sum_d mul_d * (vec_d ? vec_d[j_d] : j_d)
// so the kernels see one multiplier (and an optional device vector) per
// dimension.  Work unit = one wavefront on one tile: a stretch of up to
// `tile0` consecutive j_0 of one outer multi-index (j_1..j_{nd-1}).  The
// tile id is wave-uniform, so the outer decomposition (the only divisions
// in the kernel) runs once per tile on the scalar unit; lanes walk j_0.
//
//   runs    : dimension 0 affine with step +1 on both sides — every tile
//             is a contiguous stretch on both sides, loads and stores are
//             coalesced; a 16-byte-per-lane body runs when both run bases
//             are 16-byte aligned for every outer index
//   general : anything else (strided / reversed / vector dimension 0)
//
// Raw 4- or 8-byte words are moved: no arithmetic, bit-exact.
#include "common.hpp"
#include <algorithm>
#include <vector>

namespace da {

struct CopyNdSide {
    int64_t base;                       // elements
    int64_t mul[DA_COPY_MAXND];         // element multiplier per dimension
    const int64_t* idx[DA_COPY_MAXND];  // device index vector or null
};

struct CopyNdArgs {
    CopyNdSide d, s;
    uint64_t count[DA_COPY_MAXND];
    uint64_t tile0;          // j_0 per tile
    uint64_t tiles_per_run;  // ceil(count[0] / tile0)
    uint64_t ntiles;         // tiles_per_run * prod(count[1..])
    int nd;
};

__device__ __forceinline__ void udivmod(uint64_t a, uint64_t b, uint64_t& q,
                                        uint64_t& r) {
    // wave-uniform operands; the 32-bit form covers all but huge launches
    if (((a | b) >> 32) == 0) {
        uint32_t q32 = (uint32_t)a / (uint32_t)b;
        q = q32;
        r = (uint32_t)a - q32 * (uint32_t)b;
    } else {
        q = a / b;
        r = a - q * b;
    }
}

__device__ __forceinline__ int64_t side_term(const CopyNdSide& sd, int dim,
                                             uint64_t j) {
    const int64_t* v = sd.idx[dim];
    return sd.mul[dim] * (v ? v[j] : (int64_t)j);
}

// FAMILY 0 = runs, 1 = runs with 16-byte lanes, 2 = general
template <typename T, int FAMILY>
__global__ __launch_bounds__(256) void copy_nd_kernel(
        T* __restrict__ dst, const T* __restrict__ src, CopyNdArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4u +
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
    for (uint64_t t = wave; t < a.ntiles; t += nwaves) {
        uint64_t run, c;
        udivmod(t, a.tiles_per_run, run, c);
        int64_t doff = a.d.base, soff = a.s.base;
        for (int dim = 1; dim < a.nd; ++dim) {
            uint64_t q, j;
            udivmod(run, a.count[dim], q, j);
            run = q;
            doff += side_term(a.d, dim, j);
            soff += side_term(a.s, dim, j);
        }
        const uint64_t j0 = c * a.tile0;
        const uint64_t j1 = min(j0 + a.tile0, a.count[0]);
        if (FAMILY == 2) {
            const int64_t* dv = a.d.idx[0];
            const int64_t* sv = a.s.idx[0];
            const int64_t dm = a.d.mul[0], sm = a.s.mul[0];
            for (uint64_t j = j0 + lane; j < j1; j += 64) {
                const int64_t di = dv ? dv[j] : (int64_t)j;
                const int64_t si = sv ? sv[j] : (int64_t)j;
                dst[doff + dm * di] = src[soff + sm * si];
            }
        } else if (FAMILY == 1) {
            // both run bases 16-byte aligned (host-checked); tile0 is a
            // multiple of the vector width, so only the last tile of a run
            // has a scalar tail
            constexpr uint32_t V = 16 / sizeof(T);
            typedef T vec_t __attribute__((ext_vector_type(V)));
            T* dp = dst + doff;
            const T* sp = src + soff;
            const uint64_t nv = (j1 - j0) / V;
            vec_t* dpv = reinterpret_cast<vec_t*>(dp + j0);
            const vec_t* spv = reinterpret_cast<const vec_t*>(sp + j0);
            uint64_t i = lane;
            for (; i + 192 < nv; i += 256) {
                vec_t v0 = spv[i], v1 = spv[i + 64], v2 = spv[i + 128],
                      v3 = spv[i + 192];
                dpv[i] = v0; dpv[i + 64] = v1; dpv[i + 128] = v2;
                dpv[i + 192] = v3;
            }
            for (; i < nv; i += 64) dpv[i] = spv[i];
            for (uint64_t j = j0 + nv * V + lane; j < j1; j += 64)
                dp[j] = sp[j];
        } else {
            T* dp = dst + doff;
            const T* sp = src + soff;
            uint64_t j = j0 + lane;
            for (; j + 192 < j1; j += 256) {
                T v0 = sp[j], v1 = sp[j + 64], v2 = sp[j + 128],
                  v3 = sp[j + 192];
                dp[j] = v0; dp[j + 64] = v1; dp[j + 128] = v2;
                dp[j + 192] = v3;
            }
            for (; j < j1; j += 64) dp[j] = sp[j];
        }
    }
}

// ---- host-side validation -------------------------------------------------

struct SideView {
    const uint64_t* shape;
    const int64_t* start;
    const int64_t* step;
    const int64_t* const* idx;
    int64_t start_of(int d) const { return start ? start[d] : 0; }
    int64_t step_of(int d) const { return step ? step[d] : 1; }
    const int64_t* idx_of(int d) const { return idx ? idx[d] : nullptr; }
};

static int check_side(const char* who, const SideView& v,
                      const uint64_t* count, int nd, bool is_dst) {
    unsigned __int128 numel = 1;
    for (int d = 0; d < nd; ++d) {
        numel *= v.shape[d];
        if (numel >> 60)
            return set_err(-3, "da_copy_nd: %s shape overflows", who);
    }
    for (int d = 0; d < nd; ++d) {
        const uint64_t n = count[d];
        const uint64_t sh = v.shape[d];
        if (n >> 60)
            return set_err(-3, "da_copy_nd: count[%d] too large", d);
        const int64_t* vec = v.idx_of(d);
        if (vec) {
            for (uint64_t j = 0; j < n; ++j)
                if (vec[j] < 0 || (uint64_t)vec[j] >= sh)
                    return set_err(-3, "da_copy_nd: %s index vector %d "
                                   "entry %llu = %lld outside [0, %llu)",
                                   who, d, (unsigned long long)j,
                                   (long long)vec[j],
                                   (unsigned long long)sh);
            if (is_dst && n > 1) {
                std::vector<int64_t> tmp(vec, vec + n);
                std::sort(tmp.begin(), tmp.end());
                for (uint64_t j = 1; j < n; ++j)
                    if (tmp[j] == tmp[j - 1])
                        return set_err(-3, "da_copy_nd: duplicate "
                                       "destination index %lld in dimension "
                                       "%d (a parallel scatter has no write "
                                       "order)", (long long)tmp[j], d);
            }
            continue;
        }
        const int64_t st = v.start_of(d), sp = v.step_of(d);
        if (is_dst && sp == 0 && n > 1)
            return set_err(-3, "da_copy_nd: destination step 0 with count "
                           "%llu in dimension %d selects one element "
                           "repeatedly", (unsigned long long)n, d);
        const __int128 last = (__int128)st + (__int128)(n - 1) * sp;
        if (st < 0 || (uint64_t)st >= sh || last < 0 ||
            last >= (__int128)sh)
            return set_err(-3, "da_copy_nd: %s dimension %d selects "
                           "%lld..%lld (step %lld), outside [0, %llu)", who,
                           d, (long long)st, (long long)last, (long long)sp,
                           (unsigned long long)sh);
    }
    return 0;
}

static int plan_views(const SideView& dv, const SideView& sv,
                      const uint64_t* count, int nd, int dtype) {
    if (nd < 1 || nd > DA_COPY_MAXND)
        return set_err(-3, "da_copy_nd: nd %d outside 1..%d", nd,
                       DA_COPY_MAXND);
    if (dtype_size(dtype) == 0)
        return set_err(-3, "da_copy_nd: bad dtype %d", dtype);
    if (!dv.shape || !sv.shape || !count)
        return set_err(-3, "da_copy_nd: null shape/count");
    const bool runs = !dv.idx_of(0) && !sv.idx_of(0) &&
                      dv.step_of(0) == 1 && sv.step_of(0) == 1;
    const int family = runs ? DA_COPY_RUNS : DA_COPY_GENERAL;
    for (int d = 0; d < nd; ++d)
        if (count[d] == 0) return family;   // nothing is touched
    int rc = check_side("destination", dv, count, nd, true);
    if (rc) return rc;
    rc = check_side("source", sv, count, nd, false);
    if (rc) return rc;
    return family;
}

// ---- index-vector staging -------------------------------------------------
// Vectors are copied into a pinned host buffer (so the caller's memory is
// free on return), then uploaded on the rank's stream into a persistent
// device buffer.  Stream order protects the device buffer between calls;
// an event protects the pinned buffer from being rewritten mid-upload.
static int64_t* g_idx_host = nullptr;
static int64_t* g_idx_dev = nullptr;
static uint64_t g_idx_cap = 0;          // elements
static hipEvent_t g_idx_ev = nullptr;
static bool g_idx_pending = false;

int copy_nd_release() {
    if (g_idx_ev) { (void)hipEventDestroy(g_idx_ev); g_idx_ev = nullptr; }
    if (g_idx_host) { (void)hipHostFree(g_idx_host); g_idx_host = nullptr; }
    if (g_idx_dev) { (void)hipFree(g_idx_dev); g_idx_dev = nullptr; }
    g_idx_cap = 0;
    g_idx_pending = false;
    return 0;
}

static int stage_reserve(uint64_t n, hipStream_t s) {
    if (!g_idx_ev)
        DA_CHECK_HIP(hipEventCreateWithFlags(&g_idx_ev,
                                             hipEventDisableTiming));
    if (g_idx_pending) {
        DA_CHECK_HIP(hipEventSynchronize(g_idx_ev));
        g_idx_pending = false;
    }
    if (n <= g_idx_cap) return 0;
    // kernels of earlier calls may still read the device buffer
    DA_CHECK_HIP(hipStreamSynchronize(s));
    if (g_idx_host) { (void)hipHostFree(g_idx_host); g_idx_host = nullptr; }
    if (g_idx_dev) { (void)hipFree(g_idx_dev); g_idx_dev = nullptr; }
    g_idx_cap = 0;
    uint64_t cap = std::max<uint64_t>(n, 4096);
    DA_CHECK_HIP(hipHostMalloc((void**)&g_idx_host, cap * sizeof(int64_t),
                               hipHostMallocDefault));
    DA_CHECK_HIP(hipMalloc((void**)&g_idx_dev, cap * sizeof(int64_t)));
    g_idx_cap = cap;
    return 0;
}

static void fold_side(const SideView& v, int nd, CopyNdSide& out,
                      const uint64_t* vec_off) {
    int64_t stride = 1;
    out.base = 0;
    for (int d = 0; d < DA_COPY_MAXND; ++d) {
        out.mul[d] = 0;
        out.idx[d] = nullptr;
    }
    for (int d = 0; d < nd; ++d) {
        if (v.idx_of(d)) {
            out.mul[d] = stride;
            out.idx[d] = g_idx_dev + vec_off[d];
        } else {
            out.base += v.start_of(d) * stride;
            out.mul[d] = v.step_of(d) * stride;
        }
        stride *= (int64_t)v.shape[d];
    }
}

// true when dst/src + (base + any outer term) is 16-byte aligned: the
// pointer and base are, and every outer multiplier (times any index value)
// keeps the alignment
static bool side_vec_aligned(const void* p, const CopyNdSide& sd, int nd,
                             size_t esz) {
    const uint64_t V = 16 / esz;
    if (((uintptr_t)p & 15u) != 0) return false;
    if ((uint64_t)sd.base % V != 0) return false;
    for (int d = 1; d < nd; ++d)
        if ((uint64_t)sd.mul[d] % V != 0) return false;
    return true;
}

template <typename T>
static void launch_family(int fam, void* dst, const void* src,
                          const CopyNdArgs& a, unsigned grid, hipStream_t s) {
    T* d = static_cast<T*>(dst);
    const T* sp = static_cast<const T*>(src);
    if (fam == 0)
        hipLaunchKernelGGL((copy_nd_kernel<T, 0>), dim3(grid), dim3(256), 0,
                           s, d, sp, a);
    else if (fam == 1)
        hipLaunchKernelGGL((copy_nd_kernel<T, 1>), dim3(grid), dim3(256), 0,
                           s, d, sp, a);
    else
        hipLaunchKernelGGL((copy_nd_kernel<T, 2>), dim3(grid), dim3(256), 0,
                           s, d, sp, a);
}

int launch_copy_nd(void* dst, const uint64_t* dst_shape,
                   const int64_t* dst_start, const int64_t* dst_step,
                   const int64_t* const* dst_idx,
                   const void* src, const uint64_t* src_shape,
                   const int64_t* src_start, const int64_t* src_step,
                   const int64_t* const* src_idx,
                   const uint64_t* count, int nd, int dtype, hipStream_t s) {
    const SideView dv{dst_shape, dst_start, dst_step, dst_idx};
    const SideView sv{src_shape, src_start, src_step, src_idx};
    const int family = plan_views(dv, sv, count, nd, dtype);
    if (family < 0) return family;
    for (int d = 0; d < nd; ++d)
        if (count[d] == 0) return 0;
    if (!dst || !src) return set_err(-3, "da_copy_nd: null buffer");
    if (dst == src) return set_err(-3, "da_copy_nd: dst and src overlap");
    const size_t esz = dtype_size(dtype);

    // stage the index vectors
    uint64_t doff[DA_COPY_MAXND] = {0}, soff[DA_COPY_MAXND] = {0};
    uint64_t total = 0;
    for (int d = 0; d < nd; ++d) {
        if (dv.idx_of(d)) { doff[d] = total; total += count[d]; }
        if (sv.idx_of(d)) { soff[d] = total; total += count[d]; }
    }
    if (total) {
        int rc = stage_reserve(total, s);
        if (rc) return rc;
        for (int d = 0; d < nd; ++d) {
            if (dv.idx_of(d))
                memcpy(g_idx_host + doff[d], dv.idx_of(d),
                       count[d] * sizeof(int64_t));
            if (sv.idx_of(d))
                memcpy(g_idx_host + soff[d], sv.idx_of(d),
                       count[d] * sizeof(int64_t));
        }
        DA_CHECK_HIP(hipMemcpyAsync(g_idx_dev, g_idx_host,
                                    total * sizeof(int64_t),
                                    hipMemcpyHostToDevice, s));
        DA_CHECK_HIP(hipEventRecord(g_idx_ev, s));
        g_idx_pending = true;
    }

    CopyNdArgs a;
    memset(&a, 0, sizeof(a));
    a.nd = nd;
    fold_side(dv, nd, a.d, doff);
    fold_side(sv, nd, a.s, soff);
    uint64_t runs = 1;
    for (int d = 0; d < DA_COPY_MAXND; ++d) {
        a.count[d] = d < nd ? count[d] : 1;
        if (d >= 1 && d < nd) runs *= count[d];
    }
    int fam = family == DA_COPY_RUNS ? 0 : 2;
    if (fam == 0 && count[0] >= 2 * (16 / esz) &&
        side_vec_aligned(dst, a.d, nd, esz) &&
        side_vec_aligned(src, a.s, nd, esz))
        fam = 1;
    // a tile is one wavefront's stretch of a run: 2048 words keeps the
    // per-tile scalar decomposition far below the copy time while short
    // runs still spread one run per wavefront
    a.tile0 = 2048;
    a.tiles_per_run = (count[0] + a.tile0 - 1) / a.tile0;
    a.ntiles = a.tiles_per_run * runs;
    // 4 wavefronts per block; grid-stride beyond 8 blocks per CU x 256 CUs
    uint64_t blocks = (a.ntiles + 3) / 4;
    const uint64_t cap = 256 * 8 * 2;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, cap);
    if (esz == 8)
        launch_family<uint64_t>(fam, dst, src, a, grid, s);
    else
        launch_family<uint32_t>(fam, dst, src, a, grid, s);
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

int copy_nd_plan(const uint64_t* dst_shape, const int64_t* dst_start,
                 const int64_t* dst_step, const int64_t* const* dst_idx,
                 const uint64_t* src_shape, const int64_t* src_start,
                 const int64_t* src_step, const int64_t* const* src_idx,
                 const uint64_t* count, int nd, int dtype) {
    const SideView dv{dst_shape, dst_start, dst_step, dst_idx};
    const SideView sv{src_shape, src_start, src_step, src_idx};
    return plan_views(dv, sv, count, nd, dtype);
}

} // namespace da
