// common.hpp — shared state & error plumbing for libdarray_hip.so.
// MI355X-native (gfx950) implementation; no CUDA compatibility paths.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <unordered_map>

#include "darray_hip.h"

namespace da {

// Global per-process state: one device, one stream, one communicator
// (stream order == remotecall_wait order).
struct State {
    bool inited = false;
    int device = 0;
    int rank = 0;
    int nranks = 1;
    hipStream_t stream = nullptr;
    // second stream for point-to-point overlap (matmul partial exchange
    // rides xGMI while the next local GEMM runs); p2p ops route here
    // while p2p_comm is set (da_p2p_stream)
    hipStream_t comm_stream = nullptr;
    bool p2p_comm = false;
    hipEvent_t ev_main = nullptr, ev_comm = nullptr;
    ncclComm_t comm = nullptr;
    // small persistent device scratch for scalar allreduce / reduce outputs
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    // reduction partials buffer
    void* partials = nullptr;
    size_t partials_bytes = 0;
    // single-launch reduce fan-in ticket (dedicated 4 bytes, zeroed at
    // init and never reset; must NOT live in `partials`, which
    // dims-reduce reuses as slabs).  red_base is the value the counter
    // holds before the next launch (kernels_reduce.hip, ticket invariant)
    unsigned int* red_ticket = nullptr;
    unsigned int red_base = 0;
    // pinned host slot the flat reduce / count kernels write their result
    // to, 16 bytes { 8-byte value, 64-bit sequence } in coherent mapped
    // memory, and the device's address of it.  red_seq is the sequence of
    // the last launch that publishes into it (0 = none yet; 64 bits, so
    // it never wraps); the slot's sequence word trails it by at most the
    // launch in flight
    void* red_host = nullptr;
    void* red_host_dev = nullptr;
    uint64_t red_seq = 0;
    std::mutex mem_mtx;
    std::unordered_map<void*, uint64_t> allocs;
    uint64_t bytes_in_use = 0;
    // caching allocator: freed chunks kept per exact (256 B-rounded) size
    // — hipMalloc/hipFree of multi-GiB staging buffers costs ~100 ms,
    // which dominated the matmul leg (profiles/r01_kernel_stats.md)
    std::unordered_map<uint64_t, std::vector<void*>> pool;
    uint64_t pool_bytes = 0;
};

State& st();

// error reporting: negative codes; message captured in a buffer
extern char g_errbuf[1024];
int set_err(int code, const char* fmt, ...);

#define DA_CHECK_HIP(expr) do {                                          \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess)                                                \
        return da::set_err(-(1000 + (int)_e), "%s:%d hip error: %s",     \
                           __FILE__, __LINE__, hipGetErrorString(_e));   \
} while (0)

#define DA_CHECK_NCCL(expr) do {                                         \
    ncclResult_t _e = (expr);                                            \
    if (_e != ncclSuccess)                                               \
        return da::set_err(-(2000 + (int)_e), "%s:%d rccl error: %s",    \
                           __FILE__, __LINE__, ncclGetErrorString(_e));  \
} while (0)

#define DA_REQUIRE_INIT() do {                                           \
    if (!da::st().inited)                                                \
        return da::set_err(-1, "libdarray_hip: da_init() not called");   \
} while (0)

inline size_t dtype_size(int dtype) {
    switch (dtype) {
        case DA_F64: return 8;
        case DA_F32: return 4;
        case DA_I64: return 8;
    }
    return 0;
}

// One dtype switch for a launcher.  ALLOWED is a mask of the DT_* bits the
// caller accepts; body is a generic lambda called with a dtype_tag<T> of the
// element type (`using T = typename decltype(tag)::type;`) and launches.
// It is instantiated for allowed types only, so a launcher emits no kernel
// for a dtype it refuses.  Returns -3 "<who>: bad dtype %d" for any other
// dtype, else the status of the launch.
enum : unsigned { DT_F64 = 1u << DA_F64, DT_F32 = 1u << DA_F32,
                  DT_I64 = 1u << DA_I64, DT_FLOAT = DT_F64 | DT_F32,
                  DT_ALL = DT_FLOAT | DT_I64 };
template <typename T> struct dtype_tag { using type = T; };

template <unsigned ALLOWED, typename L>
inline int dispatch_dtype(int dtype, const char* who, L body) {
    if (dtype == DA_F64 && (ALLOWED & DT_F64)) {
        if constexpr ((ALLOWED & DT_F64) != 0) body(dtype_tag<double>{});
    } else if (dtype == DA_F32 && (ALLOWED & DT_F32)) {
        if constexpr ((ALLOWED & DT_F32) != 0) body(dtype_tag<float>{});
    } else if (dtype == DA_I64 && (ALLOWED & DT_I64)) {
        if constexpr ((ALLOWED & DT_I64) != 0) body(dtype_tag<int64_t>{});
    } else {
        return set_err(-3, "%s: bad dtype %d", who, dtype);
    }
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

int ensure_scratch(size_t bytes);
int ensure_partials(size_t bytes);

// ---- flat-reduce plumbing shared by da_reduce, da_count and the fused
// expression reduce (kernels_reduce.hip)
constexpr int RMAXB = 8192;        // block partials (fits scratch)
int reduce_grid(uint64_t want);    // min(want, DA_RBLOCKS cap), >= 1
bool reduce_fused_on();            // DA_RED_FUSED != 0
int reduce_stage2_launch(int redop, int g, int dtype, hipStream_t s);
// seq: the sequence the launched kernel publishes (published_seq), or 0
// for the two-kernel path, which publishes none and is always synced
int reduce_result(void* out_host, size_t bytes, hipStream_t s, uint64_t seq);
// results taken from the poll / from the stream sync since da_init
void reduce_waits(uint64_t* polled, uint64_t* synced);
void reduce_waits_reset();

// Ticket hand-out of EVERY single-launch fan-in kernel (ticket invariant,
// reduce_core.hpp): launch(base) starts a g-block kernel whose blocks
// each take one ticket against `base` and returns its hipError_t; only a
// launch that succeeded advances red_base.
template <typename L>
inline int fanin_launch(int g, L launch) {
    DA_CHECK_HIP(launch(st().red_base));
    st().red_base += (unsigned int)g;
    return 0;
}

// The same for the kernels whose result the host waits for (reduce,
// count, expression reduce): launch(base, seq) also hands the kernel the
// sequence it publishes next to its result, red_seq + 1, committed like
// red_base only when the launch succeeded.
template <typename L>
inline int fanin_launch_seq(int g, L launch) {
    const uint64_t seq = st().red_seq + 1;
    int rc = fanin_launch(g, [&](unsigned int base) {
        return launch(base, (unsigned long long)seq);
    });
    if (rc == 0) st().red_seq = seq;
    return rc;
}
// what to wait for after a launch: its sequence, or 0 (two-kernel path)
inline uint64_t published_seq(bool fused) {
    return fused ? st().red_seq : 0;
}

// kernel-side entry points (implemented in kernels_*.hip)
int launch_fill(void* chunk, double v, uint64_t n, int dtype, hipStream_t s);
int launch_rand(void* chunk, uint64_t n, int dtype, uint64_t seed, int kind,
                uint64_t offset, hipStream_t s);
int launch_map(int opcode, void* dst, const void* src, uint64_t n, int dtype,
               hipStream_t s);
int launch_map2(int opcode, void* dst, const void* a, const void* b,
                uint64_t n, int dtype, hipStream_t s);
int launch_bcast_fma(void* d, const void* a, const void* b, double c,
                     uint64_t n, int dtype, hipStream_t s);
int launch_map2_scalar(int opcode, void* dst, const void* src, double c,
                       int rev, uint64_t n, int dtype, hipStream_t s);
int launch_expr(const int32_t* prog, int plen, void* dst,
                const uint64_t* dst_dims, int nd,
                void* const* srcs, const uint64_t* src_strides, int nsrcs,
                const double* consts, int nconsts,
                uint64_t n, int dtype, hipStream_t s);
// hipRTC path (expr_jit.hip): 0 = launched, 1 = unavailable (use the
// interpreter), <0 = error
int launch_expr_jit(const int32_t* prog, int plen, void* dst,
                    const uint64_t* dst_dims, int nd,
                    void* const* srcs, const uint64_t* src_strides,
                    int nsrcs, const double* consts, int nconsts,
                    uint64_t n, int dtype, hipStream_t s);
// Fused mapreduce over a program (kernels_expr.hip): redop is a da_redop,
// or DA_EXPR_COUNT (darray_hip.h) for the exact count of nonzero terms
// (out: int64_t).
int validate_expr(const char* who, const int32_t* prog, int plen, int nsrcs,
                  int nconsts);
int launch_expr_reduce(const int32_t* prog, int plen, const uint64_t* dims,
                       int nd, void* const* srcs,
                       const uint64_t* src_strides, int nsrcs,
                       const double* consts, int nconsts, uint64_t n,
                       int dtype, int redop, void* out_host, hipStream_t s);
// hipRTC path of the above: launches only the g-block first kernel (with
// the in-kernel fan-in when `fused`); 0 / 1 / <0 as launch_expr_jit
int launch_expr_reduce_jit(const int32_t* prog, int plen,
                           const uint64_t* dims, int nd, void* const* srcs,
                           const uint64_t* src_strides, int nsrcs,
                           const double* consts, int nconsts, uint64_t n,
                           int dtype, int redop, int g, bool fused,
                           hipStream_t s);
// Fused dims-reduction over a program (kernels_expr.hip, loops in
// expr_dims_core.hpp).  expr_dims_select is the host-only selector (schedule
// EDIMS_*, nb slices of `chunk` terms, gridDim.x); expr_dims_check the
// host-only argument check (0 = launch, 1 = nothing to do, < 0 = error).
struct ExprDimsPlan {
    uint64_t K, R;             // outputs; terms folded into each
    int sched;
    uint32_t nb, gx, chunk;
};
struct ExprDimsArgs;
int expr_dims_select(const uint64_t* dims, int nd, uint32_t mask,
                     ExprDimsPlan* pl);
int expr_dims_check(const int32_t* prog, int plen, const uint64_t* dims,
                    int nd, void* const* srcs, const uint64_t* src_strides,
                    int nsrcs, const double* consts, int nconsts, int dtype,
                    uint32_t mask, int redop, const void* dst,
                    ExprDimsPlan* pl);
int launch_expr_reduce_dims(const int32_t* prog, int plen,
                            const uint64_t* dims, int nd, void* const* srcs,
                            const uint64_t* src_strides, int nsrcs,
                            const double* consts, int nconsts, int dtype,
                            int redop, uint32_t mask, void* dst,
                            const ExprDimsPlan& pl, hipStream_t s);
// hipRTC path of the first kernel; 0 / 1 / <0 as launch_expr_jit
int launch_expr_dims_jit(const int32_t* prog, int plen, int nsrcs, int dtype,
                         int redop, int sched, const ExprDimsArgs& a,
                         unsigned int gx, unsigned int nb, hipStream_t s);
int expr_jit_state();
const char* expr_jit_err();
int launch_transpose(void* dst, const void* src, uint64_t m, uint64_t n,
                     int dtype, hipStream_t s);
int launch_diag_scale(void* a, uint64_t m, uint64_t n, const void* diag,
                      int side, int dtype, hipStream_t s);
int launch_axpby(void* y, const void* x, double alpha, double beta,
                 uint64_t n, int dtype, hipStream_t s);
int launch_add(void* dest, const void* src, double scale, uint64_t n,
               int dtype, hipStream_t s);
int launch_scale(void* a, double s_, uint64_t n, int dtype, hipStream_t s);
int launch_cast(void* dst, int dst_dtype, const void* src, int src_dtype,
                uint64_t n, hipStream_t s);
int launch_reduce(int mapop, int redop, const void* src, uint64_t n,
                  int dtype, void* out_host, hipStream_t s);
int launch_count(int mapop, const void* src, uint64_t n, int dtype,
                 int64_t* out_host, hipStream_t s);
int launch_reduce_dims(int mapop, int redop, const void* src,
                       uint64_t inner, uint64_t axis, uint64_t outer,
                       int dtype, void* dst, hipStream_t s);
int launch_gemm_f64(void* C, const void* A, const void* B,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    double alpha, double beta, hipStream_t s);
int launch_gemm_i64(void* C, const void* A, const void* B,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    int64_t alpha, int64_t beta, hipStream_t s);
int launch_gemm_f32(void* C, const void* A, const void* B,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    double alpha, double beta, hipStream_t s);
// Inclusive prefix scan (kernels_scan.hip).  scan_check is the host-only
// argument check (0 = launch, 1 = nothing to do, < 0 = error).
int scan_check(int redop, const void* dst, const void* src, uint64_t inner,
               uint64_t axis, uint64_t outer, int dtype, const void* carry);
int launch_scan(int redop, void* dst, const void* src, uint64_t inner,
                uint64_t axis, uint64_t outer, int dtype, const void* carry,
                hipStream_t s);
// Stream compaction and its inverse (kernels_compact.hip).  The *_check
// functions are the host-only argument checks (0 = launch, 1 = nothing to
// do, < 0 = error).
int compact_check(const void* dst, uint64_t dst_cap, const void* src,
                  int dtype, const void* mask, int mask_dtype, uint64_t n);
int launch_compact(void* dst, uint64_t dst_cap, const void* src, int dtype,
                   const void* mask, int mask_dtype, uint64_t n,
                   int64_t index_base, hipStream_t s);
int expand_check(const void* dst, int dtype, const void* mask,
                 int mask_dtype, uint64_t n, const void* src,
                 uint64_t src_n, int src_broadcast);
int launch_expand(void* dst, int dtype, const void* mask, int mask_dtype,
                  uint64_t n, const void* src, uint64_t src_n,
                  int src_broadcast, hipStream_t s);
// N-D selection copy (kernels_index.hip).  copy_nd_plan is the host-only
// validator / family selector; launch_copy_nd calls it before launching.
int copy_nd_plan(const uint64_t* dst_shape, const int64_t* dst_start,
                 const int64_t* dst_step, const int64_t* const* dst_idx,
                 const uint64_t* src_shape, const int64_t* src_start,
                 const int64_t* src_step, const int64_t* const* src_idx,
                 const uint64_t* count, int nd, int dtype);
int launch_copy_nd(void* dst, const uint64_t* dst_shape,
                   const int64_t* dst_start, const int64_t* dst_step,
                   const int64_t* const* dst_idx,
                   const void* src, const uint64_t* src_shape,
                   const int64_t* src_start, const int64_t* src_step,
                   const int64_t* const* src_idx,
                   const uint64_t* count, int nd, int dtype, hipStream_t s);
int copy_nd_release();   // frees the index-vector staging (da_shutdown)
// host-only dispatcher selectors (the launchers call these themselves)
int reduce_dims_variant(uint64_t inner, uint64_t axis, uint64_t outer);
int gemm_path(int64_t m, int64_t n, int64_t k);
int scan_variant(uint64_t inner, uint64_t axis, uint64_t outer);
// dtype DA_F64 or DA_F32; out_c may be null (only out_raw is written)
int dbg_mfma_probe_impl(int dtype, const void* A, const void* B,
                        void* out_c, void* out_raw, hipStream_t s);

} // namespace da
