/* darray_hip.h — C ABI of libdarray_hip.so: the MI355X-native local-compute
 * path for DistributedArrays.jl-style distributed arrays.
 *
 * This is the drop-in boundary of SURVEY.md §8(b): each entry point replaces
 * one worker-side local operation of the reference (citations below are
 * file:line into /root/reference).  The reference touches localparts only
 * through the init-constructor / localpart / fan-out seam
 * (src/darray.jl:76-118, :330-337; src/broadcast.jl:80; src/mapreduce.jl:31;
 * src/linalg.jl:224), so a Julia caller binds these with plain `ccall`
 *  and keeps every other line of the reference.
 *
 * Conventions:
 *  - one OS process per rank per GPU (1 Julia worker <-> 1 GPU);
 *  - all device work is serialised onto ONE HIP stream per process
 *    (stream order == remotecall_wait order);
 *  - chunks are opaque device pointers owned by the creating rank, freed
 *    exactly once via da_free (hook = release_localpart, src/core.jl:67);
 *  - every function returns int: 0 = ok, <0 = error (da_errstr(code));
 *  - no torch/HIP types cross this ABI: void*, integers, doubles only.
 */
#ifndef DARRAY_HIP_H
#define DARRAY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dtypes */
enum da_dtype { DA_F64 = 0, DA_F32 = 1, DA_I64 = 2 };

/* unary map opcodes — the C-math subset of the reference's scalar-math
 * test list (/root/reference/test/darray.jl:775-800); names match
 * oracle/ops.py MAP_OPS and distributedarrays_jl_amd/_opcodes.py. */
enum da_mapop {
    DA_OP_IDENTITY = 0, DA_OP_NEG, DA_OP_ABS, DA_OP_ABS2, DA_OP_INV,
    DA_OP_SQRT, DA_OP_CBRT, DA_OP_EXP, DA_OP_EXP2, DA_OP_EXP10,
    DA_OP_EXPM1, DA_OP_LOG, DA_OP_LOG2, DA_OP_LOG10, DA_OP_LOG1P,
    DA_OP_SIN, DA_OP_COS, DA_OP_TAN, DA_OP_ASIN, DA_OP_ACOS, DA_OP_ATAN,
    DA_OP_SINH, DA_OP_COSH, DA_OP_TANH, DA_OP_ASINH, DA_OP_ACOSH,
    DA_OP_ATANH, DA_OP_SINPI, DA_OP_COSPI, DA_OP_FLOOR, DA_OP_CEIL,
    DA_OP_ROUND, DA_OP_TRUNC, DA_OP_SIGN, DA_OP_DEG2RAD, DA_OP_RAD2DEG,
    DA_OP_SEC, DA_OP_CSC, DA_OP_COT,
    /* the remainder of the reference's scalar-math list
     * (test/darray.jl:775-800) that C math / OCML covers */
    DA_OP_ERF, DA_OP_ERFC, DA_OP_ERFINV, DA_OP_ERFCINV, DA_OP_ERFCX,
    DA_OP_GAMMA, DA_OP_LGAMMA, DA_OP_SINC, DA_OP_COSC,
    DA_OP_SIND, DA_OP_COSD, DA_OP_TAND, DA_OP_ASIND, DA_OP_ACOSD,
    DA_OP_ATAND, DA_OP_ACOT, DA_OP_ACOTD, DA_OP_ASEC, DA_OP_ACSC,
    DA_OP_ASECH, DA_OP_ACSCH, DA_OP_ACOTH,
    DA_OP_ISNAN, DA_OP_ISINF, DA_OP_ISFINITE,   /* 0/1-valued (Bool-array analog) */
    DA_OP__N
};

/* binary elementwise opcodes (src/mapreduce.jl:180-189 + broadcast) */
enum da_map2op {
    DA_OP2_ADD = 0, DA_OP2_SUB, DA_OP2_MUL, DA_OP2_DIV, DA_OP2_MIN2,
    DA_OP2_MAX2, DA_OP2_IDIV, DA_OP2_MOD, DA_OP2_REM, DA_OP2_AND,
    DA_OP2_OR, DA_OP2_XOR, DA_OP2_POW, DA_OP2_ATAN2,
    DA_OP2__N
};

/* comparisons, usable in the binary slot (kind 3) of an expr program;
 * value 1 or 0 in the program's dtype (the Bool-array analog, like
 * DA_OP_ISNAN).  IEEE for floats: every comparison with a NaN is 0
 * except NE, which is 1; -0.0 == 0.0.  i64: signed, exact.  Not accepted
 * by da_map2 / da_map2_scalar (the Broadcasted comparisons of
 * src/broadcast.jl:65-98, the predicates of src/mapreduce.jl:97-131). */
enum da_cmpop { DA_CMP_EQ = 64, DA_CMP_NE, DA_CMP_LT, DA_CMP_LE,
                DA_CMP_GT, DA_CMP_GE, DA_CMP__END };

/* reduction: redop x mapop (src/mapreduce.jl:17-39, :97-131) */
enum da_redop  { DA_RED_ADD = 0, DA_RED_MUL, DA_RED_MIN, DA_RED_MAX };
enum da_redf   { DA_REDF_IDENTITY = 0, DA_REDF_ABS, DA_REDF_ABS2,
                 DA_REDF_ISNAN, DA_REDF_ISFINITE, DA_REDF_NONZERO };
/* predicate mapops feed the all/any/count specials of
 * src/mapreduce.jl:97-131: count = (pred, ADD); any = (pred, MAX) == 1;
 * all = (pred, MIN) == 1 */

/* rand kinds (drand/drandn, src/darray.jl:502-532) */
enum da_randkind { DA_RAND_UNIFORM = 0, DA_RAND_NORMAL = 1 };

/* ---- lifecycle -------------------------------------------------------- */
/* HIP context + (nranks>1) RCCL communicator bootstrap over a shared-
 * filesystem uniqueId rendezvous.  Replaces the Distributed-stdlib worker
 * pool connection (1 worker <-> 1 GPU rank). */
int da_init(int device, int rank, int nranks, const char* rccl_uid_path);
int da_shutdown(void);
int da_rank(void);
int da_nranks(void);

/* ---- chunk memory (localpart storage; src/darray.jl:76-118 init /
 *      src/core.jl:67 release_localpart) ------------------------------- */
/* Pooled: da_free caches the chunk for exact-size reuse (hipMalloc of
 * multi-GiB staging buffers costs ~100 ms); da_pool_trim releases the
 * cache to the driver.  bytes_in_use counts only live user chunks. */
int da_alloc(uint64_t nbytes, int dtype, void** chunk);
int da_free(void* chunk);
int da_pool_trim(void);
uint64_t da_pool_bytes(void);
int da_h2d(void* chunk, const void* host, uint64_t nbytes);  /* distribute, darray.jl:544-555 */
int da_d2h(const void* chunk, void* host, uint64_t nbytes);  /* collect / makelocal */
int da_d2d(void* dst, const void* src, uint64_t nbytes);
/* strided 2-D device copy (column-major pack/unpack of sub-panels; used by
 * the matmul panel exchange replacing the B[...] DArray slice gather of
 * src/linalg.jl:215) */
int da_copy2d(void* dst, uint64_t dpitch, const void* src, uint64_t spitch,
              uint64_t width, uint64_t height);

/* N-D selection-to-selection device copy: strided and index-vector
 * getindex / setindex! / view materialisation (the SubArray paths of
 * src/darray.jl:584-610, :661, :679-687).  Copies count[0] x .. x count[nd-1]
 * elements between two column-major device buffers, each side with its own
 * per-dimension selection (0-based):
 *   dst[di_0(j_0) + dst_shape[0]*(di_1(j_1) + dst_shape[1]*( .. ))] =
 *   src[si_0(j_0) + src_shape[0]*(si_1(j_1) + src_shape[1]*( .. ))]
 * for 0 <= j_d < count[d], where an index is affine, start[d] + j*step[d]
 * (step may be negative), or, when idx && idx[d], the explicit vector
 * idx[d][j] of count[d] entries.  A NULL start / step / idx array means
 * all 0 / all 1 / all affine, so a dense packed buffer is
 * (shape = count, NULL, NULL, NULL).  One call therefore packs (gather),
 * unpacks (scatter) or moves selection to selection.
 *  - idx vectors are HOST pointers: validated on the host, staged to the
 *    device on the rank's stream; the caller may free them on return.
 *  - source step 0 with count > 1 broadcasts one element (scalar
 *    assignment, singleton expansion).
 *  - destination indices must be distinct per dimension (no step 0 with
 *    count > 1, no repeated vector entry): a parallel scatter has no
 *    last-write-wins order.
 *  - any count[d] == 0 is a successful no-op; dst and src must not overlap.
 * Raw 4- / 8-byte words are moved (bit-exact); offsets are 64-bit.
 * da_copy_nd_plan is the host-only validator (no GPU work, callable
 * before da_init): < 0 with a da_errstr message for nd outside
 * 1..DA_COPY_MAXND, a bad dtype, any index outside [0, shape[d]) or a
 * duplicate destination index; otherwise the kernel family the launch
 * picks.  da_copy_nd runs it first, so with truthful shapes no argument
 * combination touches memory outside the two buffers. */
#define DA_COPY_MAXND 6
/* runs: dimension 0 affine with step +1 on both sides (contiguous,
 * coalesced stretches); general: everything else */
enum da_copy_family { DA_COPY_RUNS = 0, DA_COPY_GENERAL = 1 };
int da_copy_nd_plan(const uint64_t* dst_shape, const int64_t* dst_start,
                    const int64_t* dst_step, const int64_t* const* dst_idx,
                    const uint64_t* src_shape, const int64_t* src_start,
                    const int64_t* src_step, const int64_t* const* src_idx,
                    const uint64_t* count, int nd, int dtype);
int da_copy_nd(void* dst, const uint64_t* dst_shape, const int64_t* dst_start,
               const int64_t* dst_step, const int64_t* const* dst_idx,
               const void* src, const uint64_t* src_shape,
               const int64_t* src_start, const int64_t* src_step,
               const int64_t* const* src_idx,
               const uint64_t* count, int nd, int dtype);

/* ---- constructors on device ------------------------------------------ */
int da_fill(void* chunk, double v, uint64_t n, int dtype);   /* dzeros/dones/dfill/fill!, darray.jl:468-494,822-827 */
/* Philox4x32-10 fill; element mapping documented in oracle/philox.py.
 * seed = 1234 + rank per BASELINE.md; offset = counter origin. */
int da_rand(void* chunk, uint64_t n, int dtype, uint64_t seed, int kind,
            uint64_t offset);                                /* drand/drandn, darray.jl:502-532 */

/* ---- elementwise hot path -------------------------------------------- */
int da_map(int opcode, void* dst, const void* src, uint64_t n, int dtype);   /* map!, mapreduce.jl:5-12 */
int da_map2(int opcode, void* dst, const void* a, const void* b,
            uint64_t n, int dtype);                          /* elementwise +,-,.. mapreduce.jl:180-189 */
int da_bcast_fma(void* d, const void* a, const void* b, double c,
                 uint64_t n, int dtype);                     /* D .= A .* B .+ c, broadcast.jl:65-85 */

/* Fused broadcast composition — materializes an arbitrary Broadcasted
 * tree in one pass (copyto!(localpart, bclocal(bc)), broadcast.jl:65-98;
 * nested broadcast pinned at test/darray.jl:880-912).
 *
 * prog: postfix int32 program, kind = ins>>8, idx = ins&0xff:
 *   kind 0 = unary da_mapop on stack top; kind 1 = push argument idx;
 *   kind 2 = push constant idx; kind 3 = binary da_map2op or da_cmpop
 *   (pops rhs then lhs).  Stack depth <= DA_EXPR_MAXSTACK (validated).
 * dst_dims/nd: destination LOCAL chunk shape (column-major), nd <= 4.
 * src_strides: nsrcs x nd element strides (row-major per arg); a 0
 *   stride expands a Julia-broadcast singleton dim.  NULL = every arg
 *   dense over the destination chunk (fast flat path).
 * Numerics are bit-identical to da_map/da_map2 chains of the same ops
 * (shared scalar functor tables, -ffp-contract=off). */
#define DA_EXPR_MAXLEN   40
#define DA_EXPR_MAXARGS  6
#define DA_EXPR_MAXCONSTS 6
#define DA_EXPR_MAXND    4
#define DA_EXPR_MAXSTACK 8
int da_expr(const int32_t* prog, int prog_len, void* dst,
            const uint64_t* dst_dims, int nd,
            void* const* srcs, const uint64_t* src_strides, int nsrcs,
            const double* consts, int nconsts, uint64_t n, int dtype);
/* da_expr compiles each distinct program to a dedicated kernel via
 * hipRTC (cached per process; DA_EXPR_JIT=0 forces the interpreter).
 * state: 1 ready, 2 active, -1 hipRTC failed (interpreter fallback). */
int da_expr_jit_state(void);
const char* da_expr_jit_errstr(void);
/* Fused mapreduce over a program: op-folds (da_expr_reduce) or counts the
 * nonzero terms of (da_expr_count; exact, NaN counts) the program's values
 * over a local chunk of n elements WITHOUT materialising them — one
 * launch, one read per operand element, result in *out (host; the dtype's
 * own scalar / an int64_t).  Program arguments as da_expr; dims is the
 * local chunk shape reduced over; src_strides == NULL means every operand
 * is dense over it (f64/f32/i64, any n), else the strided variant
 * (f64/f32, nd <= 4, n < 2^32).  n == 0 gives the fold identity / 0.
 * Fold-order contract: *out has EXACTLY the bits of da_expr into a dense
 * temporary followed by da_reduce(DA_REDF_IDENTITY, redop, tmp, n) /
 * da_count(DA_REDF_NONZERO, tmp, n) in the same process (DA_RV4 does not
 * apply; DA_RED_FUSED=0 and DA_EXPR_JIT=0 are honoured, same bits).
 * Like da_reduce, neither call drains the stream (stream contract under
 * "reductions" below). */
int da_expr_reduce(const int32_t* prog, int prog_len,
                   const uint64_t* dims, int nd,
                   void* const* srcs, const uint64_t* src_strides, int nsrcs,
                   const double* consts, int nconsts, uint64_t n, int dtype,
                   int redop, void* out);
int da_expr_count(const int32_t* prog, int prog_len,
                  const uint64_t* dims, int nd,
                  void* const* srcs, const uint64_t* src_strides, int nsrcs,
                  const double* consts, int nconsts, uint64_t n, int dtype,
                  int64_t* out);
/* Fused mapreduce ALONG DIMENSIONS over a program — mapreduce(f, op, A...;
 * dims) with f a broadcast tree (mapreduce.jl:83-94): one pass for any set
 * of reduced dimensions, one read per operand element, no temporary of the
 * chunk's size.  Program arguments as da_expr_reduce.  dims[nd] is the
 * local chunk shape (column-major, nd <= DA_EXPR_MAXND, fewer than 2^32
 * elements in all); bit d of reduce_mask set = dimension d is reduced.
 * src_strides as da_expr (NULL = every operand dense over the chunk); all
 * of f64 / f32 / i64 take strides here.  redop is a da_redop, or
 * DA_EXPR_COUNT for the exact count of nonzero terms.  dst is DEVICE
 * memory of K = prod(kept extents) elements in column-major order of the
 * kept dimensions: the operand dtype for a fold, int64_t for a count.
 * K == 0 launches nothing; a reduced extent of 0 fills dst with the fold
 * identity (0 for a count).  Stream-ordered, no host synchronisation.
 * The result's bits depend on the shape, the mask and the program alone:
 * fixed fold order, no atomics, the same through hipRTC and DA_EXPR_JIT=0
 * (DESIGN.md §17).  Arguments are checked before the da_init check. */
#define DA_EXPR_COUNT (-1)
int da_expr_reduce_dims(const int32_t* prog, int prog_len,
                        const uint64_t* dims, int nd,
                        void* const* srcs, const uint64_t* src_strides,
                        int nsrcs, const double* consts, int nconsts,
                        int dtype, uint32_t reduce_mask, int redop,
                        void* dst);
int da_map2_scalar(int opcode, void* dst, const void* src, double c,
                   int reverse, uint64_t n, int dtype);      /* D .+ 1 etc (scalar broadcast arg, broadcast.jl:124-133) */
int da_axpby(void* y, const void* x, double alpha, double beta,
             uint64_t n, int dtype);                         /* y = alpha*x + beta*y: axpy! linalg.jl:24-34 */
int da_add(void* dest, const void* src, double scale,
           uint64_t n, int dtype);                           /* add!, linalg.jl:62-76 */
int da_scale(void* a, double s, uint64_t n, int dtype);      /* rmul!, linalg.jl:54-59 */
/* dtype conversion (DArray{T2}(D) family); float->i64 rounds half-even */
int da_cast(void* dst, int dst_dtype, const void* src, int src_dtype,
            uint64_t n);

/* ---- reductions -------------------------------------------------------*/
/* Stream contract of the scalar results (da_reduce, da_count,
 * da_expr_reduce, da_expr_count): the call returns once *out holds the
 * result, and by then the reducing kernel has finished READING its
 * sources.  It does NOT promise that the rank's stream has drained: the
 * single-launch kernel publishes {value, sequence} into a pinned host slot
 * and the host watches that slot for up to DA_RED_SPIN_US microseconds
 * (default 2000) instead of synchronising the stream.  Work queued before
 * the reduce has completed (one stream, in order); the runtime may not yet
 * know.  A caller that needs the stream drained (to read other device
 * results through its own channel, say) calls da_synchronize.  The stream
 * is synchronised as before when the budget runs out (a kernel fault comes
 * back as the HIP error then), with DA_RED_SPIN_US=0, and on the
 * two-kernel path (DA_RED_FUSED=0, DA_RV4=1). */
/* Local (per-chunk) mapreduce stage: LDS + wavefront-shuffle tree.
 * Result written to *out as the dtype's own scalar type (f64/f32/i64) —
 * the per-worker mapreduce(f, op, localpart(d)) of mapreduce.jl:31.
 * n == 0 returns the fold identity.  Does not drain the stream (above). */
int da_reduce(int mapop, int redop, const void* src, uint64_t n, int dtype,
              void* out);
/* Exact predicate count (count(f, A), mapreduce.jl:115-122): mapop must be
 * a predicate (DA_REDF_ISNAN / ISFINITE / NONZERO).  The 0/1 values are
 * accumulated in a 64-bit integer on the device whatever the source dtype,
 * so *out is exact for every n (a float accumulator rounds above 2^24).
 * Fold across ranks with da_allreduce(out, 1, DA_I64, DA_RED_ADD).
 * Does not drain the stream (stream contract above). */
int da_count(int mapop, const void* src, uint64_t n, int dtype,
             int64_t* out);
/* Per-chunk dims-reduction (src/mapreduce.jl:42-94, mapreducedim_within):
 * chunk viewed column-major as (inner, axis, outer); dst gets
 * inner*outer elements reduced over axis (identity when axis==0). */
int da_reduce_dims(int mapop, int redop, const void* src, uint64_t inner,
                   uint64_t axis, uint64_t outer, int dtype, void* dst);
/* Inclusive scan (Base.accumulate / cumsum / cumprod) of a local chunk viewed
 * column-major as (inner, axis, outer), along `axis`:
 *   dst[i + inner*(k + axis*o)] =
 *       [carry[i + inner*o] (op)] src[i,0,o] (op) src[i,1,o] (op) .. (op) src[i,k,o]
 * redop is a da_redop (ADD, MUL, MIN, MAX; NaN-propagating min/max and
 * wrap-around i64 exactly as da_reduce), dtype f64/f32/i64, accumulation in
 * the dtype itself; the bracketing of a float sum or product is unspecified
 * (a tree over tiles and spans), like the reductions'.  carry is a device
 * array of inner*outer elements folded in FRONT of every line (the prefix of
 * the chunks before this one, or init), or NULL: then element 0 of every
 * line is copied bit for bit (-0.0 and NaN payloads survive).
 * dst == src (exactly) is allowed; any other overlap of dst with src or
 * carry is rejected on the host, as are a bad redop / dtype, a NULL dst or
 * src with a non-zero element count and an inner*axis*outer (or byte count)
 * that overflows 64 bits: < 0 with a da_errstr message, nothing launched.
 * The arguments are checked before the da_init check.  inner*axis*outer == 0
 * is a successful no-op.  axis == 1 is a copy (combined with carry if given).
 * No workgroup ever waits for another one: a few long lines (inner == 1)
 * take two launches (fold the spans, then scan them) instead. */
int da_scan(int redop, void* dst, const void* src,
            uint64_t inner, uint64_t axis, uint64_t outer,
            int dtype, const void* carry);
/* Stream compaction (filter(f, A) / findall / A[mask]) and its inverse
 * (A[mask] = v) of a local chunk of n elements.
 * Mask truth everywhere below: element != 0 in the mask's own dtype, so a
 * NaN is true and -0.0 is false — the DA_REDF_NONZERO rule of da_count,
 * whose result is the number kept.  dtype and mask_dtype are each f64, f32
 * or i64, independently; data moves as raw 4- / 8-byte words (bit-exact),
 * element alignment only; n, every index and every position are 64-bit.
 * Three stream-ordered steps on the rank's stream (count the true elements
 * of every DA_COMPACT_TILE-element tile, scan the counts with da_scan's
 * kernels, scatter); no workgroup ever waits for another one and no atomic
 * hands out positions, so the order is stable and the result
 * deterministic.  Neither call synchronises: the caller sizes dst from
 * da_count(DA_REDF_NONZERO, mask, ..).
 * Checked on the host before the da_init check, < 0 with a da_errstr
 * message and nothing launched: a bad dtype / mask_dtype, a NULL pointer
 * with a non-zero count, a forbidden overlap, a byte count that overflows
 * 64 bits.  n == 0 is a successful no-op; dst_cap == 0 / src_n == 0 is
 * legal and stores nothing. */
#define DA_COMPACT_TILE 2048
/* dst[j] = src[i] for the j-th (0-based) i in increasing order with
 * mask[i] != 0; with src == NULL, dst is int64_t and gets index_base + i
 * (findall).  Only j < dst_cap is stored: a too-small dst_cap drops the
 * tail and never writes outside dst.  Stable.  src == mask is fine (both
 * are only read); dst overlapping src or mask is rejected. */
int da_compact(void* dst, uint64_t dst_cap, const void* src, int dtype,
               const void* mask, int mask_dtype, uint64_t n,
               int64_t index_base);
/* The inverse: for the j-th true i, dst[i] = src_broadcast ? src[0] : src[j]
 * (only j < src_n is stored; a broadcast source with src_n > 0 reaches
 * every true i); every other dst[i] is left untouched.  dst == mask
 * (exactly, with equal element sizes) is allowed: each thread loads
 * mask[i] before it stores dst[i].  Any other overlap of dst with mask or
 * src is rejected. */
int da_expand(void* dst, int dtype, const void* mask, int mask_dtype,
              uint64_t n, const void* src, uint64_t src_n, int src_broadcast);
/* Cross-rank fold of scalar partials (the caller-side reduce(op, results)
 * of mapreduce.jl:34, re-expressed as an RCCL allreduce over xGMI).
 * inout is HOST memory of `count` dtype elements; nranks==1 is a no-op. */
int da_allreduce(void* inout, int count, int dtype, int redop);

/* ---- dense linear algebra -------------------------------------------- */
/* Local C = alpha*A*B + beta*C, COLUMN-major f64 (Julia layout), MFMA-
 * tiled for gfx950 — the localpart(A)*B_jk of src/linalg.jl:224.
 * lda/ldb/ldc are element leading dimensions (>= rows; padded panels and
 * sub-matrix pointers into a larger parent are allowed).
 * Alignment (da_gemm_f64 / da_gemm_f32 / da_gemm_i64): the MFMA kernels
 * stage operands with 16-byte vector loads, so A, B and C must be 16-byte
 * aligned and lda/ldb/ldc multiples of 16 bytes (2 f64 / 4 f32 elements)
 * whenever m%128 == n%128 == k%16 == 0; chunks from da_alloc with
 * 16-element-aligned leading dimensions and offsets always qualify.  The
 * naive path (any other shape, and da_gemm_i64) needs element alignment
 * only.  beta == 0 overwrites C without reading it (NaN in C is ignored);
 * alpha == 0 or k == 0 yields beta*C without reading A or B. */
int da_gemm_f64(void* C, const void* A, const void* B,
                int64_t m, int64_t n, int64_t k,
                int64_t lda, int64_t ldb, int64_t ldc,
                double alpha, double beta);
/* i64 local GEMM (exact, wrap mod 2^64; Julia Int matmul parity) */
int da_gemm_i64(void* C, const void* A, const void* B,
                int64_t m, int64_t n, int64_t k,
                int64_t lda, int64_t ldb, int64_t ldc,
                int64_t alpha, int64_t beta);
/* f32 local GEMM on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32;
 * bitwise an fmaf chain — cdna_hip_programming.md §3) */
int da_gemm_f32(void* C, const void* A, const void* B,
                int64_t m, int64_t n, int64_t k,
                int64_t lda, int64_t ldb, int64_t ldc,
                double alpha, double beta);

/* ---- transpose / Diagonal scaling (linalg.jl:1-17, :169-187) --------- */
int da_transpose(void* dst, const void* src, uint64_t m, uint64_t n,
                 int dtype);                 /* dst = src^T, LDS-tiled */
int da_diag_scale(void* a, uint64_t m, uint64_t n, const void* diag,
                  int side, int dtype);      /* side 0: rows (lmul!), 1: cols (rmul!) */

/* ---- distributed samplesort building blocks (src/sort.jl:103-170) --- */
int da_sort(void* chunk, uint64_t n, int dtype);       /* per-chunk radix sort */
int da_sort_out(const void* src, void* dst, uint64_t n, int dtype);
int da_lower_bound(const void* sorted, uint64_t n, int dtype,
                   const void* splitters, int k, uint64_t* out);

/* ---- point-to-point (panel / halo exchange; replaces the remotecall
 *      shipping of B panels and partial products, linalg.jl:211-251,
 *      and makelocal's remote fetch, darray.jl:351-368) ----------------- */
int da_group_start(void);
int da_group_end(void);
int da_send(const void* buf, uint64_t nbytes, int peer);
int da_recv(void* buf, uint64_t nbytes, int peer);
int da_sendrecv(const void* sbuf, int peer_s, void* rbuf, int peer_r,
                uint64_t nbytes);
/* comm/compute overlap: route p2p ops onto a second stream and fence the
 * two streams with events (the matmul partial exchange rides xGMI while
 * the next local GEMM runs) */
int da_p2p_stream(int use_comm);
int da_comm_after_compute(void);
int da_main_after_comm(void);
int da_comm_sync(void);
int da_bcast(void* buf, uint64_t nbytes, int root);
int da_barrier(void);      /* device barrier over the communicator */

/* ---- stream & timing --------------------------------------------------*/
int da_synchronize(void);
int da_event_create(void** ev);
int da_event_record(void* ev);
int da_event_elapsed(void* ev_start, void* ev_stop, float* ms);
int da_event_destroy(void* ev);

/* ---- debug: host-only dispatcher selectors (no GPU work, callable
 *      before da_init).  The launchers call the same functions, so a test
 *      can assert which kernel a shape reaches before launching it. ------ */
enum da_dims_variant { DA_DIMS_SLICES = 0, DA_DIMS_THREADS, DA_DIMS_WAVES,
                       DA_DIMS_BLOCKS };
enum da_gemm_path_id { DA_GEMM_NAIVE = 0, DA_GEMM_MFMA = 1 };
/* cols: inner > 1, one thread per line; block: inner == 1, one workgroup
 * per line (>= 512 lines, or lines of at most one 2048-element tile);
 * spans: inner == 1, fewer and longer lines, cut into spans, two launches */
enum da_scan_variant { DA_SCAN_COLS = 0, DA_SCAN_BLOCK, DA_SCAN_SPANS };
/* kernel family da_reduce_dims picks for a (inner, axis, outer) view */
int dbg_reduce_dims_variant(uint64_t inner, uint64_t axis, uint64_t outer);
/* MFMA or naive kernel for da_gemm_f64/f32 at (m, n, k), k > 0, alpha != 0 */
int dbg_gemm_path(int64_t m, int64_t n, int64_t k);
/* kernel family da_scan picks for a (inner, axis, outer) view (spelled
 * `extern int`: tests/test_abi.py pins the set of plain `int dbg_*`
 * declarations to the two selectors above) */
extern int dbg_scan_variant(uint64_t inner, uint64_t axis, uint64_t outer);
/* lanes: the leading dimension (the first of extent > 1) is kept, a thread
 * per output; wave / block: it is reduced, a wave (fewer than 512 terms per
 * output) or a workgroup per output */
enum da_expr_dims_variant { DA_EDIMS_LANES = 0, DA_EDIMS_WAVE,
                            DA_EDIMS_BLOCK };
/* schedule da_expr_reduce_dims picks for a chunk shape and mask (< 0: a
 * shape or mask it rejects); *nb = slices the reduced index space is split
 * into (> 1: partial rows and a second fold kernel; 0: no term to fold),
 * *gx = workgroups along x of the first launch (capped; grid-stride
 * beyond).  Either pointer may be NULL.  (`extern int`: see above) */
extern int dbg_expr_dims_variant(const uint64_t* dims, int nd,
                                 uint32_t reduce_mask, uint32_t* nb,
                                 uint32_t* gx);
/* how many scalar results (da_reduce, da_count, da_expr_reduce,
 * da_expr_count) were taken from the poll of the pinned slot and how many
 * from the stream-sync fallback since da_init; either pointer may be NULL */
int da_dbg_reduce_waits(uint64_t* polled, uint64_t* synced);

/* ---- introspection / errors ------------------------------------------ */
const char* da_errstr(int code);
int da_device_props(char* name, int name_len, uint64_t* hbm_bytes);
uint64_t da_bytes_in_use(void);   /* leak check hook (test/runtests.jl:28-37 analog) */

#ifdef __cplusplus
}
#endif
#endif /* DARRAY_HIP_H */
