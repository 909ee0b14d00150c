// expr_dims_core.hpp — the accumulate loops and the fan-in of the fused
// dims-reduction over a broadcast program (da_expr_reduce_dims).  ONE text
// for the interpreter kernel (kernels_expr.hip) and the hipRTC-generated
// kernels (expr_jit.hip embeds this file next to reduce_core.hpp): both
// hand `expr_dims_body` a callable that evaluates the program at one set
// of operand offsets, so they walk the terms in the same order and give
// the same bits.
//
// The host (expr_dims_plan, kernels_expr.hip) splits the chunk's
// dimensions into the KEPT ones (K = their product, the outputs, in
// column-major order) and the REDUCED ones (R = their product, the terms
// folded into each output), drops extents of 1 and merges neighbours an
// index can run across.  An output index decodes over kext / kstr, a term
// index over rext / rstr; an operand's element is at the sum of both.
//
// Schedules (the host picks by shape alone, expr_dims_select):
//   LANES  the chunk's leading dimension is kept: a thread owns an output,
//          consecutive lanes own consecutive outputs (coalesced along the
//          leading dimension) and walk the terms serially;
//   WAVE   the leading dimension is reduced, R < EDIMS_BLOCK_R: a wave
//          owns an output, lanes stride the terms (fastest along the
//          leading dimension), then the shuffle tree;
//   BLOCK  the same with a whole workgroup and the LDS tree
//          (block_reduce_in) for longer folds.
// gridDim.y = nb cuts the terms into nb slices of `chunk`; with nb > 1 the
// destination is nb rows of K partials, folded afterwards in ascending
// slice order by expr_dims_fold (no atomics: the bits depend on the shape
// alone).  Fold order of one output: each thread absorbs its terms in
// ascending index order, then the tree, then the slices ascending.
#pragma once
#include "reduce_core.hpp"

namespace da {

enum { EDIMS_LANES = 0, EDIMS_WAVE = 1, EDIMS_BLOCK = 2 };
constexpr unsigned int EDIMS_BLOCK_R = 512;   // shortest fold BLOCK takes

struct ExprDimsArgs {
    const void* srcs[DA_EXPR_MAXARGS];
    double consts[DA_EXPR_MAXCONSTS];
    void* dst;                  // K outputs, or nb rows of K partials
    unsigned int K, R;          // outputs; terms per output (both < 2^32)
    unsigned int chunk;         // terms per slice (gridDim.y slices)
    int nk, nr;                 // kept / reduced dimensions after merging
    unsigned int kext[DA_EXPR_MAXND], rext[DA_EXPR_MAXND];
    unsigned int kstr[DA_EXPR_MAXARGS][DA_EXPR_MAXND];   // element strides,
    unsigned int rstr[DA_EXPR_MAXARGS][DA_EXPR_MAXND];   // 0 = singleton
};

// COUNT: +1 per nonzero term (a NaN is nonzero), in int64 whatever T
template <bool COUNT, typename A, typename T>
__device__ __forceinline__ A edims_absorb(int redop, A acc, T x) {
    if constexpr (COUNT) return acc + (x != (T)0 ? 1 : 0);
    else return red_comb(redop, acc, (A)x);
}

// operand offsets of index i decoded over ext[0..n) with strides str
template <int NS>
__device__ __forceinline__ void edims_decode(
    unsigned int i, int n, const unsigned int* ext,
    const unsigned int (*str)[DA_EXPR_MAXND], unsigned long long* off) {
#pragma unroll
    for (int d = 0; d < DA_EXPR_MAXND; ++d) {
        if (d < n) {
            unsigned int e = ext[d];
            unsigned int q = i / e, x = i - q * e;
            i = q;
#pragma unroll
            for (int k = 0; k < NS; ++k)
                off[k] += (unsigned long long)x * str[k][d];
        }
    }
}

// NS: operands whose offsets are maintained (DA_EXPR_MAXARGS in the
// interpreter, the program's count in generated code).  NK / NR: a.nk /
// a.nr as constants, or -1 to read them.  `term(off)` evaluates the
// program with operand k at element off[k].  `sh`: RTPB/64 workgroup-shared
// elements (BLOCK only).
template <typename T, typename A, bool COUNT, int SCHED, int NS, int NK,
          int NR, typename F>
__device__ __forceinline__ void expr_dims_body(const ExprDimsArgs& a,
                                               int redop, F term, A* sh) {
    const int nk = NK >= 0 ? NK : a.nk;
    const int nr = NR >= 0 ? NR : a.nr;
    if (COUNT) redop = DA_RED_ADD;
    A* dst = (A*)a.dst + (unsigned long long)blockIdx.y * a.K;
    const unsigned long long r0l = (unsigned long long)blockIdx.y * a.chunk;
    const unsigned int r0 = r0l < a.R ? (unsigned int)r0l : a.R;
    const unsigned int r1 = r0l + a.chunk < a.R ? (unsigned int)(r0l + a.chunk)
                                                : a.R;
    if constexpr (SCHED == EDIMS_LANES) {
        // the first reduced dimension is walked in runs: one decode per
        // run, then 4 independent evaluations per step absorbed in order
        const unsigned int e0 = nr > 0 ? a.rext[0] : 1u;
        for (unsigned long long o = (unsigned long long)blockIdx.x * RTPB +
                                    threadIdx.x;
             o < a.K; o += (unsigned long long)gridDim.x * RTPB) {
            unsigned long long base[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) base[k] = 0;
            edims_decode<NS>((unsigned int)o, nk, a.kext, a.kstr, base);
            A acc = RedIdent<A>::get(redop);
            unsigned int r = r0;
            while (r < r1) {
                unsigned long long off[NS], o1[NS], o2[NS], o3[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) off[k] = base[k];
                edims_decode<NS>(r, nr, a.rext, a.rstr, off);
                unsigned int run = e0 - r % e0;
                if (run > r1 - r) run = r1 - r;
                unsigned int j = 0;
                for (; j + 4 <= run; j += 4) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        unsigned long long s0 = nr > 0 ? a.rstr[k][0] : 0;
                        o1[k] = off[k] + s0;
                        o2[k] = o1[k] + s0;
                        o3[k] = o2[k] + s0;
                    }
                    T t0 = term(off), t1 = term(o1), t2 = term(o2),
                      t3 = term(o3);
                    acc = edims_absorb<COUNT>(redop, acc, t0);
                    acc = edims_absorb<COUNT>(redop, acc, t1);
                    acc = edims_absorb<COUNT>(redop, acc, t2);
                    acc = edims_absorb<COUNT>(redop, acc, t3);
#pragma unroll
                    for (int k = 0; k < NS; ++k)
                        off[k] = o3[k] + (nr > 0 ? a.rstr[k][0] : 0);
                }
                for (; j < run; ++j) {
                    acc = edims_absorb<COUNT>(redop, acc, term(off));
#pragma unroll
                    for (int k = 0; k < NS; ++k)
                        off[k] += nr > 0 ? a.rstr[k][0] : 0;
                }
                r += run;
            }
            dst[o] = acc;
        }
    } else {
        // W lanes own an output and stride its terms
        constexpr unsigned int W = SCHED == EDIMS_WAVE ? 64u : (unsigned)RTPB;
        constexpr unsigned int G = RTPB / W;      // outputs per workgroup
        const unsigned int t = threadIdx.x % W;
        for (unsigned long long o = (unsigned long long)blockIdx.x * G +
                                    threadIdx.x / W;
             o < a.K; o += (unsigned long long)gridDim.x * G) {
            unsigned long long base[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) base[k] = 0;
            edims_decode<NS>((unsigned int)o, nk, a.kext, a.kstr, base);
            A acc = RedIdent<A>::get(redop);
            unsigned long long r = (unsigned long long)r0 + t;
            for (; r + 3ull * W < r1; r += 4ull * W) {
                unsigned long long off[NS], o1[NS], o2[NS], o3[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    off[k] = o1[k] = o2[k] = o3[k] = base[k];
                edims_decode<NS>((unsigned int)r, nr, a.rext, a.rstr, off);
                edims_decode<NS>((unsigned int)(r + W), nr, a.rext, a.rstr,
                                 o1);
                edims_decode<NS>((unsigned int)(r + 2 * W), nr, a.rext,
                                 a.rstr, o2);
                edims_decode<NS>((unsigned int)(r + 3 * W), nr, a.rext,
                                 a.rstr, o3);
                T t0 = term(off), t1 = term(o1), t2 = term(o2),
                  t3 = term(o3);
                acc = edims_absorb<COUNT>(redop, acc, t0);
                acc = edims_absorb<COUNT>(redop, acc, t1);
                acc = edims_absorb<COUNT>(redop, acc, t2);
                acc = edims_absorb<COUNT>(redop, acc, t3);
            }
            for (; r < r1; r += W) {
                unsigned long long off[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) off[k] = base[k];
                edims_decode<NS>((unsigned int)r, nr, a.rext, a.rstr, off);
                acc = edims_absorb<COUNT>(redop, acc, term(off));
            }
            if constexpr (SCHED == EDIMS_WAVE) {
#pragma unroll
                for (int s = 32; s > 0; s >>= 1)
                    acc = red_comb(redop, acc, (A)__shfl_down(acc, s, 64));
                if (t == 0) dst[o] = acc;
            } else {
                // o is the same in every thread of the workgroup, so all
                // of them reach these barriers together
                acc = block_reduce_in(redop, acc, sh);
                if (threadIdx.x == 0) dst[o] = acc;
                __syncthreads();   // sh is written again next round
            }
        }
    }
}

// Second step of a split fold, and the fill of an empty one (nb == 0):
// thread o folds part[0*K + o], part[1*K + o], ... in that order.
template <typename A>
__device__ __forceinline__ void expr_dims_fold_body(const A* part, A* dst,
                                                    unsigned int K,
                                                    unsigned int nb,
                                                    int redop) {
    for (unsigned long long o = (unsigned long long)blockIdx.x * RTPB +
                                threadIdx.x;
         o < K; o += (unsigned long long)gridDim.x * RTPB) {
        A acc = RedIdent<A>::get(redop);
        for (unsigned int s = 0; s < nb; ++s)
            acc = red_comb(redop, acc, part[(unsigned long long)s * K + o]);
        dst[o] = acc;
    }
}

} // namespace da
