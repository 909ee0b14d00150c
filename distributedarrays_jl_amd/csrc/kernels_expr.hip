// kernels_expr.hip — fused broadcast-composition interpreter for gfx950.
//
// The reference materializes an ARBITRARY Broadcasted tree in one local
// pass per worker (copyto!(localpart, bclocal(bc)),
// /root/reference/src/broadcast.jl:65-98; nested broadcast pinned at
// test/darray.jl:880-912: `a .- m .* sin.(c)` with a dims-expanded `m`).
// Round 1 had only the fixed opcode table plus one fused ternary; this
// kernel closes the gap: a postfix program over the SAME scalar functor
// tables (mapops.hpp — bit-identical numerics to da_map/da_map2)
// evaluates any unary/binary composition in ONE pass, algorithmic
// traffic only (one read per distinct operand element, one write).
//
// Program encoding (include/darray_hip.h): int32 instructions,
//   kind = ins >> 8, idx = ins & 0xff
//   kind 0: unary da_mapop idx applied to the stack top
//   kind 1: push element of argument idx
//   kind 2: push constant idx
//   kind 3: binary da_map2op idx (pops rhs, then lhs; pushes f(l, r))
// Stack depth <= DA_EXPR_MAXSTACK, validated host-side by simulation.
//
// Two variants:
//   flat    — every argument is dense over the destination's local chunk
//             (index i); 2-wide vectorized like map_kernel;
//   strided — per-argument element strides (0 on Julia-broadcast
//             singleton dims, e.g. the mean row of `a .- mean(a,dims=1)`);
//             the destination multi-index is decoded once per element
//             (u32 div chain) and shared by all arguments.
// Both HBM-bound; compiled -ffp-contract=off (Julia Base numerics).
#include "common.hpp"
#include "mapops.hpp"
#include "reduce_core.hpp"
#include "expr_dims_core.hpp"
#include <math.h>

namespace da {

namespace {
constexpr int TPB = 256;
constexpr int MAXBLOCKS = 8192;   // 1024 workgroups/XCD

static inline int nblocks(uint64_t work) {
    uint64_t b = (work + TPB - 1) / TPB;
    if (b > (uint64_t)MAXBLOCKS) b = MAXBLOCKS;
    if (b == 0) b = 1;
    return (int)b;
}
}  // namespace

// Program shipped BY VALUE in the kernel arguments (<= ~500 B: no
// device staging buffers, no extra H2D latency per launch).
struct ExprProg {
    int32_t ins[DA_EXPR_MAXLEN];
    int len;
    const void* srcs[DA_EXPR_MAXARGS];
    double consts[DA_EXPR_MAXCONSTS];
};

struct ExprStrides {
    uint32_t dims[DA_EXPR_MAXND];                      // dest local shape
    uint32_t str[DA_EXPR_MAXARGS][DA_EXPR_MAXND];      // elem strides; 0=expand
    int nd;
};

template <typename T>
__device__ __forceinline__ T expr_eval(const ExprProg& p, uint64_t i) {
    T stack[DA_EXPR_MAXSTACK];
    int sp = 0;
    for (int pc = 0; pc < p.len; ++pc) {
        int ins = p.ins[pc];
        int kind = ins >> 8, idx = ins & 0xff;
        switch (kind) {
        case 1: stack[sp++] = ((const T*)p.srcs[idx])[i]; break;
        case 2: stack[sp++] = (T)p.consts[idx]; break;
        case 0: stack[sp - 1] = apply_map<T>(idx, stack[sp - 1]); break;
        default: {
            T b = stack[--sp];
            stack[sp - 1] = apply_map2<T>(idx, stack[sp - 1], b);
        }
        }
    }
    return stack[0];
}

__device__ __forceinline__ int64_t expr_eval_i64(const ExprProg& p,
                                                 uint64_t i) {
    int64_t stack[DA_EXPR_MAXSTACK];
    int sp = 0;
    for (int pc = 0; pc < p.len; ++pc) {
        int ins = p.ins[pc];
        int kind = ins >> 8, idx = ins & 0xff;
        switch (kind) {
        case 1: stack[sp++] = ((const int64_t*)p.srcs[idx])[i]; break;
        case 2: stack[sp++] = (int64_t)p.consts[idx]; break;
        case 0: stack[sp - 1] = apply_map_i64(idx, stack[sp - 1]); break;
        default: {
            int64_t b = stack[--sp];
            stack[sp - 1] = apply_map2_i64(idx, stack[sp - 1], b);
        }
        }
    }
    return stack[0];
}

template <typename T>
__global__ void expr_flat_kernel(ExprProg p, T* __restrict__ dst,
                                 uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // 2 adjacent elements per lane: the compiler merges the two
    // interleaved evaluations' loads into 16-B accesses on dense args
    uint64_t nv = n / 2;
    for (uint64_t jp = i; jp < nv; jp += stride) {
        uint64_t j = 2 * jp;
        T r0 = expr_eval<T>(p, j);
        T r1 = expr_eval<T>(p, j + 1);
        dst[j] = r0;
        dst[j + 1] = r1;
    }
    for (uint64_t j = 2 * nv + i; j < n; j += stride)
        dst[j] = expr_eval<T>(p, j);
}

__global__ void expr_flat_kernel_i64(ExprProg p, int64_t* __restrict__ dst,
                                     uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = i; j < n; j += stride)
        dst[j] = expr_eval_i64(p, j);
}

// Strided variant: decode the destination's column-major multi-index
// once per element, then each argument reads at sum(idx_d * str[a][d])
// (stride 0 expands a singleton dim, the bclocal localisation of
// broadcast.jl:140-152 after gather).
template <typename T>
__device__ __forceinline__ T expr_strided_eval(const ExprProg& p,
                                               const ExprStrides& s,
                                               uint64_t i) {
    uint32_t idx[DA_EXPR_MAXND];
    uint32_t rem = (uint32_t)i;   // local chunks are < 2^32 elements
    for (int d = 0; d < s.nd; ++d) {
        idx[d] = rem % s.dims[d];
        rem /= s.dims[d];
    }
    uint64_t off[DA_EXPR_MAXARGS];
    for (int a = 0; a < DA_EXPR_MAXARGS; ++a) off[a] = 0;
    for (int d = 0; d < s.nd; ++d)
        for (int a = 0; a < DA_EXPR_MAXARGS; ++a)
            off[a] += (uint64_t)idx[d] * s.str[a][d];

    T stack[DA_EXPR_MAXSTACK];
    int sp = 0;
    for (int pc = 0; pc < p.len; ++pc) {
        int ins = p.ins[pc];
        int kind = ins >> 8, opi = ins & 0xff;
        switch (kind) {
        case 1: stack[sp++] = ((const T*)p.srcs[opi])[off[opi]]; break;
        case 2: stack[sp++] = (T)p.consts[opi]; break;
        case 0: stack[sp - 1] = apply_map<T>(opi, stack[sp - 1]); break;
        default: {
            T b = stack[--sp];
            stack[sp - 1] = apply_map2<T>(opi, stack[sp - 1], b);
        }
        }
    }
    return stack[0];
}

template <typename T>
__device__ __forceinline__ void expr_strided_body(const ExprProg& p,
                                                  const ExprStrides& s,
                                                  T* dst, uint64_t n) {
    uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = i0; i < n; i += gstride)
        dst[i] = expr_strided_eval<T>(p, s, i);
}

template <typename T>
__global__ void expr_strided_kernel(ExprProg p, ExprStrides s,
                                    T* __restrict__ dst, uint64_t n) {
    expr_strided_body<T>(p, s, dst, n);
}

// Program validation shared by da_expr and da_expr_reduce / da_expr_count:
// lengths, arg/const bounds and a host-side stack simulation.
int validate_expr(const char* who, const int32_t* prog, int plen, int nsrcs,
                  int nconsts) {
    if (plen <= 0 || plen > DA_EXPR_MAXLEN)
        return set_err(-3, "%s: bad program length %d", who, plen);
    if (nsrcs < 0 || nsrcs > DA_EXPR_MAXARGS || nconsts < 0 ||
        nconsts > DA_EXPR_MAXCONSTS)
        return set_err(-3, "%s: too many args/consts", who);
    // host-side validation by stack simulation
    int sp = 0;
    for (int pc = 0; pc < plen; ++pc) {
        int kind = prog[pc] >> 8, idx = prog[pc] & 0xff;
        switch (kind) {
        case 1:
            if (idx >= nsrcs) return set_err(-3, "%s: arg %d oob", who, idx);
            ++sp; break;
        case 2:
            if (idx >= nconsts)
                return set_err(-3, "%s: const %d oob", who, idx);
            ++sp; break;
        case 0:
            if (sp < 1 || idx >= DA_OP__N)
                return set_err(-3, "%s: bad unary at %d", who, pc);
            break;
        case 3:
            if (sp < 2 || !(idx < DA_OP2__N ||
                            (idx >= DA_CMP_EQ && idx < DA_CMP__END)))
                return set_err(-3, "%s: bad binary at %d", who, pc);
            --sp; break;
        default:
            return set_err(-3, "%s: bad kind at %d", who, pc);
        }
        if (sp > DA_EXPR_MAXSTACK)
            return set_err(-3, "%s: stack overflow at %d", who, pc);
    }
    if (sp != 1)
        return set_err(-3, "%s: program leaves %d values", who, sp);
    return 0;
}

int launch_expr(const int32_t* prog, int plen, void* dst,
                const uint64_t* dst_dims, int nd,
                void* const* srcs, const uint64_t* src_strides, int nsrcs,
                const double* consts, int nconsts,
                uint64_t n, int dtype, hipStream_t s) {
    int vrc = validate_expr("da_expr", prog, plen, nsrcs, nconsts);
    if (vrc) return vrc;
    if (n == 0) return 0;

    // preferred path: hipRTC-compiled kernel for this exact program
    // (register pressure of the expression only; numerics identical —
    // generated code calls the same functor tables).  Falls back to
    // the interpreter below when disabled or compilation fails.
    {
        int rc = launch_expr_jit(prog, plen, dst, dst_dims, nd, srcs,
                                 src_strides, nsrcs, consts, nconsts, n,
                                 dtype, s);
        if (rc <= 0) return rc;
    }

    ExprProg P;
    memset(&P, 0, sizeof(P));
    for (int i = 0; i < plen; ++i) P.ins[i] = prog[i];
    P.len = plen;
    for (int i = 0; i < nsrcs; ++i) P.srcs[i] = srcs[i];
    for (int i = 0; i < nconsts; ++i) P.consts[i] = consts[i];

    if (src_strides == nullptr) {
        int g = nblocks(n / 2 + 1);
        switch (dtype) {
        case DA_F64:
            hipLaunchKernelGGL((expr_flat_kernel<double>), dim3(g),
                               dim3(TPB), 0, s, P, (double*)dst, n);
            break;
        case DA_F32:
            hipLaunchKernelGGL((expr_flat_kernel<float>), dim3(g),
                               dim3(TPB), 0, s, P, (float*)dst, n);
            break;
        case DA_I64:
            hipLaunchKernelGGL(expr_flat_kernel_i64, dim3(nblocks(n)),
                               dim3(TPB), 0, s, P, (int64_t*)dst, n);
            break;
        default: return set_err(-3, "da_expr: bad dtype %d", dtype);
        }
        DA_CHECK_HIP(hipGetLastError());
        return 0;
    }

    if (nd < 1 || nd > DA_EXPR_MAXND)
        return set_err(-3, "da_expr: nd %d unsupported (max %d)", nd,
                       DA_EXPR_MAXND);
    if (n >> 32)
        return set_err(-3, "da_expr: strided variant needs n < 2^32");
    ExprStrides S;
    memset(&S, 0, sizeof(S));
    S.nd = nd;
    uint64_t total = 1;
    for (int d = 0; d < nd; ++d) {
        S.dims[d] = (uint32_t)dst_dims[d];
        total *= dst_dims[d];
    }
    if (total != n)
        return set_err(-3, "da_expr: dims/numel mismatch");
    for (int a = 0; a < nsrcs; ++a)
        for (int d = 0; d < nd; ++d)
            S.str[a][d] = (uint32_t)src_strides[(size_t)a * nd + d];
    int g = nblocks(n);
    switch (dtype) {
    case DA_F64:
        hipLaunchKernelGGL((expr_strided_kernel<double>), dim3(g),
                           dim3(TPB), 0, s, P, S, (double*)dst, n);
        break;
    case DA_F32:
        hipLaunchKernelGGL((expr_strided_kernel<float>), dim3(g),
                           dim3(TPB), 0, s, P, S, (float*)dst, n);
        break;
    default:
        return set_err(-3, "da_expr: strided variant is float-only");
    }
    DA_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- fused mapreduce over a program (da_expr_reduce / da_expr_count) --
// The evaluators above feed the accumulate loop and fan-in of the flat
// reduce (reduce_core.hpp) with the element-to-thread assignment and fold
// order of da_reduce's kernels: thread i absorbs terms 2j, 2j+1 for
// j = i, i+stride, ..., then the scalar tail; wave shuffle tree; 4-slot
// LDS fold; the last arriver folds the block partials.  So the result
// has the bits of materialising the program and reducing the temporary.
// This interpreter form serves DA_EXPR_JIT=0 and hipRTC failures; the
// generated kernels of expr_jit.hip run the same loop.
template <typename T> struct ExprTerm {
    static __device__ __forceinline__ T at(const ExprProg& p, uint64_t i) {
        return expr_eval<T>(p, i);
    }
};
template <> struct ExprTerm<int64_t> {
    static __device__ __forceinline__ int64_t at(const ExprProg& p,
                                                 uint64_t i) {
        return expr_eval_i64(p, i);
    }
};

// COUNT: +1 per nonzero term (a NaN is nonzero), in int64 whatever T
template <bool COUNT, typename A, typename T>
__device__ __forceinline__ A expr_absorb(int redop, A acc, T x) {
    if constexpr (COUNT) return acc + (x != (T)0 ? 1 : 0);
    else return red_comb(redop, acc, x);
}

// `partials` is not __restrict__/const: see reduce_fused
template <typename T, typename A, bool COUNT, bool STRIDED>
__global__ void expr_reduce_kernel(ExprProg p, ExprStrides s, uint64_t n,
                                   int redop, A* partials,
                                   unsigned int* ticket, unsigned int base,
                                   int fused, A* out,
                                   unsigned long long seq) {
    __shared__ A sh[RTPB / 64 + 1];
    auto term = [&](uint64_t i) -> T {
        if constexpr (STRIDED) return expr_strided_eval<T>(p, s, i);
        else return ExprTerm<T>::at(p, i);
    };
    if (COUNT) redop = DA_RED_ADD;
    uint64_t i = (uint64_t)blockIdx.x * RTPB + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * RTPB;
    A acc = RedIdent<A>::get(redop);
    uint64_t nv = n / 2;
    for (uint64_t j = i; j < nv; j += stride) {
        T r0 = term(2 * j);
        T r1 = term(2 * j + 1);
        acc = expr_absorb<COUNT>(redop, acc, r0);
        acc = expr_absorb<COUNT>(redop, acc, r1);
    }
    for (uint64_t j = 2 * nv + i; j < n; j += stride)
        acc = expr_absorb<COUNT>(redop, acc, term(j));
    acc = block_reduce_in(redop, acc, sh);
    if (fused)
        fanin_finish(redop, acc, partials, ticket, base, out, seq, sh);
    else if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

namespace {
struct ExprRedArgs {
    ExprProg P;
    ExprStrides S;
    uint64_t n;
    int redop, g;
    bool fused;
    hipStream_t s;
};

template <typename T, typename A, bool COUNT, bool STRIDED>
int expr_reduce_interp(const ExprRedArgs& a) {
    A* parts = (A*)st().partials;
    A* out = (A*)st().red_host_dev;
    auto launch = [&](unsigned int base, unsigned long long seq) {
        hipLaunchKernelGGL((expr_reduce_kernel<T, A, COUNT, STRIDED>),
                           dim3(a.g), dim3(RTPB), 0, a.s, a.P, a.S, a.n,
                           a.redop, parts, st().red_ticket, base,
                           a.fused ? 1 : 0, out, seq);
        return hipGetLastError();
    };
    if (a.fused) return fanin_launch_seq(a.g, launch);
    DA_CHECK_HIP(launch(0u, 0ull));
    return 0;
}

template <typename T, bool STRIDED>
int expr_reduce_interp_t(const ExprRedArgs& a, bool count) {
    return count ? expr_reduce_interp<T, int64_t, true, STRIDED>(a)
                 : expr_reduce_interp<T, T, false, STRIDED>(a);
}
}  // namespace

int launch_expr_reduce(const int32_t* prog, int plen, const uint64_t* dims,
                       int nd, void* const* srcs,
                       const uint64_t* src_strides, int nsrcs,
                       const double* consts, int nconsts, uint64_t n,
                       int dtype, int redop, void* out_host, hipStream_t s) {
    const bool count = redop == DA_EXPR_COUNT;
    const char* who = count ? "da_expr_count" : "da_expr_reduce";
    int rc = validate_expr(who, prog, plen, nsrcs, nconsts);
    if (rc) return rc;
    if (!count && (redop < 0 || redop > DA_RED_MAX))
        return set_err(-3, "%s: bad redop %d", who, redop);
    if (!out_host) return set_err(-3, "%s: null out", who);
    if (dtype != DA_F64 && dtype != DA_F32 && dtype != DA_I64)
        return set_err(-3, "%s: bad dtype %d", who, dtype);
    if (nsrcs > 0 && !srcs) return set_err(-3, "%s: null srcs", who);
    const bool strided = src_strides != nullptr;
    if (strided) {
        if (dtype == DA_I64)
            return set_err(-3, "%s: strided variant is float-only", who);
        if (nd < 1 || nd > DA_EXPR_MAXND || !dims)
            return set_err(-3, "%s: nd %d unsupported (max %d)", who, nd,
                           DA_EXPR_MAXND);
        if (n >> 32)
            return set_err(-3, "%s: strided variant needs n < 2^32", who);
        uint64_t total = 1;
        for (int d = 0; d < nd; ++d) total *= dims[d];
        if (total != n) return set_err(-3, "%s: dims/numel mismatch", who);
    }
    if (n == 0) {  // fold identity / zero count, no launch
        if (count) *(int64_t*)out_host = 0;
        else if (dtype == DA_F64)
            *(double*)out_host = RedIdent<double>::get(redop);
        else if (dtype == DA_F32)
            *(float*)out_host = RedIdent<float>::get(redop);
        else *(int64_t*)out_host = RedIdent<int64_t>::get(redop);
        return 0;
    }
    // da_reduce's grid for n elements, whatever the program or layout
    const int g = reduce_grid((n / 2 + RTPB - 1) / RTPB);
    rc = ensure_partials(RMAXB * sizeof(double));
    if (rc) return rc;
    const bool fused = reduce_fused_on();

    rc = launch_expr_reduce_jit(prog, plen, dims, nd, srcs, src_strides,
                                nsrcs, consts, nconsts, n, dtype, redop, g,
                                fused, s);
    if (rc < 0) return rc;
    if (rc == 1) {   // interpreter (DA_EXPR_JIT=0 or hipRTC failed)
        ExprRedArgs a;
        memset(&a, 0, sizeof(a));
        for (int i = 0; i < plen; ++i) a.P.ins[i] = prog[i];
        a.P.len = plen;
        for (int i = 0; i < nsrcs; ++i) a.P.srcs[i] = srcs[i];
        for (int i = 0; i < nconsts; ++i) a.P.consts[i] = consts[i];
        if (strided) {
            a.S.nd = nd;
            for (int d = 0; d < nd; ++d) a.S.dims[d] = (uint32_t)dims[d];
            for (int k = 0; k < nsrcs; ++k)
                for (int d = 0; d < nd; ++d)
                    a.S.str[k][d] =
                        (uint32_t)src_strides[(size_t)k * nd + d];
        }
        a.n = n;
        a.redop = redop;
        a.g = g;
        a.fused = fused;
        a.s = s;
        if (dtype == DA_I64)
            rc = expr_reduce_interp_t<int64_t, false>(a, count);
        else if (dtype == DA_F64)
            rc = strided ? expr_reduce_interp_t<double, true>(a, count)
                         : expr_reduce_interp_t<double, false>(a, count);
        else
            rc = strided ? expr_reduce_interp_t<float, true>(a, count)
                         : expr_reduce_interp_t<float, false>(a, count);
        if (rc) return rc;
    }
    if (!fused) {
        rc = reduce_stage2_launch(count ? (int)DA_RED_ADD : redop, g,
                                  count ? (int)DA_I64 : dtype, s);
        if (rc) return rc;
    }
    return reduce_result(out_host, count ? sizeof(int64_t)
                                         : dtype_size(dtype), s,
                         published_seq(fused));
}

// ---- fused dims-reduction over a program (da_expr_reduce_dims) ---------
// mapreduce(f, op, A...; dims) with f a broadcast tree: every operand
// element is read once, nothing of the domain's size is stored.  The loops
// and the fan-in are expr_dims_core.hpp's, shared with the generated
// kernels of expr_jit.hip; this interpreter form serves DA_EXPR_JIT=0 and
// hipRTC failures.  Its evaluator is one out-of-line function per element
// type: the 18 kernels below would otherwise each inline the functor
// switch five times.
template <typename T> struct ExprIsI64 { static constexpr bool v = false; };
template <> struct ExprIsI64<int64_t> { static constexpr bool v = true; };

template <typename T>
__device__ __noinline__ T expr_eval_off(const ExprProg& p,
                                        const unsigned long long* off) {
    T stack[DA_EXPR_MAXSTACK];
    int sp = 0;
    for (int pc = 0; pc < p.len; ++pc) {
        int ins = p.ins[pc];
        int kind = ins >> 8, opi = ins & 0xff;
        switch (kind) {
        case 1: stack[sp++] = ((const T*)p.srcs[opi])[off[opi]]; break;
        case 2: stack[sp++] = (T)p.consts[opi]; break;
        case 0:
            if constexpr (ExprIsI64<T>::v)
                stack[sp - 1] = apply_map_i64(opi, stack[sp - 1]);
            else
                stack[sp - 1] = apply_map<T>(opi, stack[sp - 1]);
            break;
        default: {
            T b = stack[--sp];
            if constexpr (ExprIsI64<T>::v)
                stack[sp - 1] = apply_map2_i64(opi, stack[sp - 1], b);
            else
                stack[sp - 1] = apply_map2<T>(opi, stack[sp - 1], b);
        }
        }
    }
    return stack[0];
}

template <typename T, typename A, bool COUNT, int SCHED>
__global__ void __launch_bounds__(RTPB)
expr_dims_kernel(ExprProg p, ExprDimsArgs a, int redop) {
    __shared__ A sh[RTPB / 64 + 1];
    expr_dims_body<T, A, COUNT, SCHED, DA_EXPR_MAXARGS, -1, -1>(
        a, redop,
        [&](const unsigned long long* off) -> T {
            return expr_eval_off<T>(p, off);
        },
        sh);
}

template <typename A>
__global__ void __launch_bounds__(RTPB)
expr_dims_fold_kernel(const A* part, A* dst, unsigned int K, unsigned int nb,
                      int redop) {
    expr_dims_fold_body<A>(part, dst, K, nb, redop);
}

namespace {
constexpr uint32_t EDIMS_SPLIT_BLOCKS = 1024;  // split while fewer workgroups
constexpr uint32_t EDIMS_MAXBLOCKS = 4096;     // gridDim.x cap (grid-stride)

template <typename T, typename A, bool COUNT>
hipError_t expr_dims_interp_s(const ExprProg& P, const ExprDimsArgs& a,
                              int redop, const ExprDimsPlan& pl,
                              hipStream_t s) {
    dim3 g(pl.gx, pl.nb), b(RTPB);
    switch (pl.sched) {
    case EDIMS_LANES:
        hipLaunchKernelGGL((expr_dims_kernel<T, A, COUNT, EDIMS_LANES>), g, b,
                           0, s, P, a, redop);
        break;
    case EDIMS_WAVE:
        hipLaunchKernelGGL((expr_dims_kernel<T, A, COUNT, EDIMS_WAVE>), g, b,
                           0, s, P, a, redop);
        break;
    default:
        hipLaunchKernelGGL((expr_dims_kernel<T, A, COUNT, EDIMS_BLOCK>), g, b,
                           0, s, P, a, redop);
    }
    return hipGetLastError();
}

template <typename A>
hipError_t expr_dims_fold(const void* part, void* dst, uint32_t K,
                          uint32_t nb, int redop, hipStream_t s) {
    uint32_t g = (K + RTPB - 1) / RTPB;
    if (g > EDIMS_MAXBLOCKS) g = EDIMS_MAXBLOCKS;
    hipLaunchKernelGGL((expr_dims_fold_kernel<A>), dim3(g), dim3(RTPB), 0, s,
                       (const A*)part, (A*)dst, K, nb, redop);
    return hipGetLastError();
}
}  // namespace

// Host-only: schedule, slices and grid for a chunk shape and a mask of
// reduced dimensions (exported as dbg_expr_dims_variant).  < 0: bad shape.
int expr_dims_select(const uint64_t* dims, int nd, uint32_t mask,
                     ExprDimsPlan* pl) {
    const char* who = "da_expr_reduce_dims";
    if (nd < 1 || nd > DA_EXPR_MAXND)
        return set_err(-3, "%s: nd %d unsupported (1..%d)", who, nd,
                       DA_EXPR_MAXND);
    if (!dims) return set_err(-3, "%s: null dims", who);
    if (mask >> nd)
        return set_err(-3, "%s: bad mask 0x%x for nd %d", who, mask, nd);
    uint64_t K = 1, R = 1;
    bool lead_seen = false, lead_reduced = false;
    for (int d = 0; d < nd; ++d) {
        const bool red = (mask >> d) & 1u;
        uint64_t& acc = red ? R : K;
        if (dims[d] >> 32 || (acc *= dims[d]) >> 32 || (K * R) >> 32)
            return set_err(-3, "%s: chunk too large: the index decode needs "
                           "fewer than 2^32 elements", who);
        if (!lead_seen && dims[d] > 1) {
            lead_seen = true;
            lead_reduced = red;
        }
    }
    pl->K = K;
    pl->R = R;
    pl->sched = !lead_reduced ? EDIMS_LANES
                : R < EDIMS_BLOCK_R ? EDIMS_WAVE : EDIMS_BLOCK;
    if (K == 0 || R == 0) {      // nothing to launch / identity fill
        pl->sched = EDIMS_LANES;
        pl->nb = pl->gx = pl->chunk = 0;
        return 0;
    }
    // outputs per workgroup; fewest terms worth a slice of their own
    const uint64_t opb = pl->sched == EDIMS_LANES ? RTPB
                         : pl->sched == EDIMS_WAVE ? RTPB / 64 : 1;
    const uint64_t minchunk = pl->sched == EDIMS_LANES ? 8
                              : pl->sched == EDIMS_WAVE ? 256 : 1024;
    const uint64_t blocks = (K + opb - 1) / opb;
    uint64_t nb = EDIMS_SPLIT_BLOCKS / blocks;
    if (nb > R / minchunk) nb = R / minchunk;
    if (nb < 1) nb = 1;
    const uint64_t chunk = (R + nb - 1) / nb;
    pl->chunk = (uint32_t)chunk;
    pl->nb = (uint32_t)((R + chunk - 1) / chunk);
    pl->gx = (uint32_t)(blocks < EDIMS_MAXBLOCKS ? blocks : EDIMS_MAXBLOCKS);
    return 0;
}

// Host-only argument check of da_expr_reduce_dims: 0 = launch, 1 = nothing
// to do (no outputs), < 0 = error.  Touches no device memory.
int expr_dims_check(const int32_t* prog, int plen, const uint64_t* dims,
                    int nd, void* const* srcs, const uint64_t* src_strides,
                    int nsrcs, const double* consts, int nconsts, int dtype,
                    uint32_t mask, int redop, const void* dst,
                    ExprDimsPlan* pl) {
    const char* who = "da_expr_reduce_dims";
    if (!prog) return set_err(-3, "%s: null prog", who);
    int rc = validate_expr(who, prog, plen, nsrcs, nconsts);
    if (rc) return rc;
    if (redop != DA_EXPR_COUNT && (redop < 0 || redop > DA_RED_MAX))
        return set_err(-3, "%s: bad redop %d", who, redop);
    if (dtype != DA_F64 && dtype != DA_F32 && dtype != DA_I64)
        return set_err(-3, "%s: bad dtype %d", who, dtype);
    if (nsrcs > 0 && !srcs) return set_err(-3, "%s: null srcs", who);
    if (nconsts > 0 && !consts) return set_err(-3, "%s: null consts", who);
    // the size limit comes before anything that could reach the JIT
    rc = expr_dims_select(dims, nd, mask, pl);
    if (rc) return rc;
    if (src_strides)
        for (int i = 0; i < nsrcs * nd; ++i)
            if (src_strides[i] >> 32)
                return set_err(-3, "%s: stride %d too large", who, i);
    if (pl->K == 0) return 1;
    if (!dst) return set_err(-3, "%s: null dst", who);
    return 0;
}

int launch_expr_reduce_dims(const int32_t* prog, int plen,
                            const uint64_t* dims, int nd, void* const* srcs,
                            const uint64_t* src_strides, int nsrcs,
                            const double* consts, int nconsts, int dtype,
                            int redop, uint32_t mask, void* dst,
                            const ExprDimsPlan& pl, hipStream_t s) {
    const bool count = redop == DA_EXPR_COUNT;
    const int rop = count ? (int)DA_RED_ADD : redop;
    const bool acc64 = count || dtype == DA_I64;   // int64 accumulator
    const uint32_t K = (uint32_t)pl.K;
    auto fold = [&](const void* part, uint32_t nb) {
        if (acc64) return expr_dims_fold<int64_t>(part, dst, K, nb, rop, s);
        if (dtype == DA_F64)
            return expr_dims_fold<double>(part, dst, K, nb, rop, s);
        return expr_dims_fold<float>(part, dst, K, nb, rop, s);
    };
    if (pl.R == 0) {   // an empty fold: the identity (0 for a count)
        DA_CHECK_HIP(fold(nullptr, 0));
        return 0;
    }

    // kept / reduced dimension lists: extents of 1 dropped, neighbours
    // merged where every operand's stride lets one index run across both
    ExprDimsArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nsrcs; ++i) a.srcs[i] = srcs[i];
    for (int i = 0; i < nconsts; ++i) a.consts[i] = consts[i];
    a.K = K;
    a.R = (uint32_t)pl.R;
    a.chunk = pl.chunk;
    uint64_t dense = 1;
    for (int d = 0; d < nd; ++d) {
        uint32_t str[DA_EXPR_MAXARGS];
        for (int k = 0; k < nsrcs; ++k)
            str[k] = (uint32_t)(src_strides ? src_strides[(size_t)k * nd + d]
                                            : dense);
        dense *= dims[d];
        if (dims[d] == 1) continue;
        const bool red = (mask >> d) & 1u;
        int& n = red ? a.nr : a.nk;
        uint32_t* ext = red ? a.rext : a.kext;
        uint32_t (*st_)[DA_EXPR_MAXND] = red ? a.rstr : a.kstr;
        bool merge = n > 0;
        for (int k = 0; merge && k < nsrcs; ++k)
            merge = (uint64_t)st_[k][n - 1] * ext[n - 1] == str[k];
        if (merge) {
            ext[n - 1] *= (uint32_t)dims[d];
        } else {
            ext[n] = (uint32_t)dims[d];
            for (int k = 0; k < nsrcs; ++k) st_[k][n] = str[k];
            ++n;
        }
    }

    void* out = dst;
    if (pl.nb > 1) {
        int rc = ensure_partials((size_t)pl.nb * K * sizeof(double));
        if (rc) return rc;
        out = st().partials;
    }
    a.dst = out;

    int rc = launch_expr_dims_jit(prog, plen, nsrcs, dtype, redop, pl.sched,
                                  a, pl.gx, pl.nb, s);
    if (rc < 0) return rc;
    if (rc == 1) {   // interpreter (DA_EXPR_JIT=0 or hipRTC failed)
        ExprProg P;
        memset(&P, 0, sizeof(P));
        for (int i = 0; i < plen; ++i) P.ins[i] = prog[i];
        P.len = plen;
        for (int i = 0; i < nsrcs; ++i) P.srcs[i] = srcs[i];
        for (int i = 0; i < nconsts; ++i) P.consts[i] = consts[i];
        hipError_t he;
        if (dtype == DA_I64)
            he = count ? expr_dims_interp_s<int64_t, int64_t, true>(P, a, rop,
                                                                    pl, s)
                       : expr_dims_interp_s<int64_t, int64_t, false>(
                             P, a, rop, pl, s);
        else if (dtype == DA_F64)
            he = count ? expr_dims_interp_s<double, int64_t, true>(P, a, rop,
                                                                   pl, s)
                       : expr_dims_interp_s<double, double, false>(P, a, rop,
                                                                   pl, s);
        else
            he = count ? expr_dims_interp_s<float, int64_t, true>(P, a, rop,
                                                                  pl, s)
                       : expr_dims_interp_s<float, float, false>(P, a, rop,
                                                                 pl, s);
        DA_CHECK_HIP(he);
    }
    if (pl.nb > 1) DA_CHECK_HIP(fold(out, pl.nb));
    return 0;
}

} // namespace da
