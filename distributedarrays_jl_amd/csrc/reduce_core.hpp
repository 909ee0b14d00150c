// reduce_core.hpp — the device-only primitives of the flat reduce: fold
// identities, the combiner, the block tree and the single-launch fan-in.
// ONE text for the static kernels (kernels_reduce.hip, kernels_expr.hip)
// and the hipRTC-generated expression-reduce kernels (expr_jit.hip embeds
// this file next to mapops.hpp), so every flat reduction of the library
// folds in the same order and gives the same bits.
//
// hipRTC has no <math.h> / <stdint.h> macros: infinity and the int64
// limits come from compiler builtins.
#pragma once
#include "darray_hip.h"

namespace da {

constexpr int RTPB = 256;          // 4 waves per block

template <typename T> struct RedIdent {
    static __device__ __host__ T get(int redop) {
        switch (redop) {
        case DA_RED_ADD: return (T)0;
        case DA_RED_MUL: return (T)1;
        case DA_RED_MIN: return (T)__builtin_inff();
        case DA_RED_MAX: return (T)(-__builtin_inff());
        }
        return (T)0;
    }
};
template <> struct RedIdent<int64_t> {
    static __device__ __host__ int64_t get(int redop) {
        switch (redop) {
        case DA_RED_ADD: return 0;
        case DA_RED_MUL: return 1;
        case DA_RED_MIN: return __INT64_MAX__;
        case DA_RED_MAX: return -__INT64_MAX__ - 1;
        }
        return 0;
    }
};

template <typename T>
__device__ __forceinline__ T red_comb(int redop, T a, T b) {
    switch (redop) {
    case DA_RED_ADD: return a + b;
    case DA_RED_MUL: return a * b;
    case DA_RED_MIN:  // NaN-propagating (Julia min)
        return a != a ? a : (b != b ? b : (a < b ? a : b));
    case DA_RED_MAX:
        return a != a ? a : (b != b ? b : (a > b ? a : b));
    }
    return a;
}
__device__ __forceinline__ int64_t red_comb(int redop, int64_t a, int64_t b) {
    switch (redop) {
    case DA_RED_ADD: return (int64_t)((uint64_t)a + (uint64_t)b);
    case DA_RED_MUL: return (int64_t)((uint64_t)a * (uint64_t)b);
    case DA_RED_MIN: return a < b ? a : b;
    case DA_RED_MAX: return a > b ? a : b;
    }
    return a;
}

// `lds`: RTPB/64 workgroup-shared elements, one per wave.
template <typename T>
__device__ __forceinline__ T block_reduce_in(int redop, T v, T* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = red_comb(redop, v, (T)__shfl_down(v, off, 64));
    int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (wave == 0) {
        T w = lane < (RTPB / 64) ? lds[lane]
                                 : RedIdent<T>::get(redop);
#pragma unroll
        for (int off = 2; off > 0; off >>= 1)
            w = red_comb(redop, w, (T)__shfl_down(w, off, 64));
        return w;
    }
    return v;
}

// ---- single-launch fan-in (cdna_hip_programming.md §5, "In-launch
// split-K reduction", in its fence-free form; §6 Guideline 16 R1).
// Each block's payload is ONE partial of <= 8 bytes, so it is published
// by a relaxed agent-scope atomic store — a write-through (sc1) store
// that needs no release fence — drained by the storing wave's
// s_waitcnt vmcnt(0) before that same lane takes its ticket.  Only the
// last arriver pays a fence: one agent-scope acquire, then plain loads
// of all partials in reduce_stage2's fold order (thread t folds
// t, t+256, ...; then block_reduce), so both paths give the same bits.
// No block waits for another, so residency is irrelevant.
//
// Ticket invariant: the counter is zeroed once in da_init and never
// reset.  Every launch of g blocks adds exactly g, and launches of the
// one library stream run in order, so before a launch the counter
// equals State::red_base (mod 2^32), which the host advances by g per
// launch (fanin_launch, common.hpp).  A block is last iff
// ticket - base == g - 1 in unsigned arithmetic; that holds across
// wrap-around, any sequence of grid sizes, and interleaved dtypes /
// reduce / count / expression-reduce calls.
template <typename A>
__device__ __forceinline__ void publish_partial(A* p, A v) {
    if constexpr (sizeof(A) == 8)
        __hip_atomic_store((unsigned long long*)p,
                           __builtin_bit_cast(unsigned long long, v),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        __hip_atomic_store((unsigned int*)p,
                           __builtin_bit_cast(unsigned int, v),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The result hand-off to the host.  `out` is the device address of the
// 16-byte pinned host slot { 8-byte value, 64-bit sequence } (RedSlot,
// reduce_wait.hpp).  One lane, once per launch: a system-scope store of
// the value, then a system-scope RELEASE store of this launch's `seq`
// into out + 8, so a host whose acquire load of the sequence word
// returns `seq` reads this launch's value.  The release stays a release:
// the guide's fence-free write-through form (§6 Guideline 16 R1) is
// stated for agent-scope hand-offs inside a launch, not for host-visible
// memory at system scope.  Two stores, never one 16-byte one: nothing
// promises that arrives untorn.
template <typename A>
__device__ __forceinline__ void publish_result(A* out, A v,
                                               unsigned long long seq) {
    if constexpr (sizeof(A) == 8)
        __hip_atomic_store((unsigned long long*)out,
                           __builtin_bit_cast(unsigned long long, v),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else
        __hip_atomic_store((unsigned int*)out,
                           __builtin_bit_cast(unsigned int, v),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((unsigned long long*)((char*)out + 8), seq,
                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// `acc`: the block's partial (valid in thread 0).  `sh`: RTPB/64 + 1
// shared elements — block_reduce_in's scratch plus the "I am last"
// flag, kept in ONE __shared__ object.  Reusing sh[0..3] for the final
// fold is safe: wave 0 read them before it wrote the flag, and every
// other wave writes them again only after the barriers below.
template <typename A>
__device__ __forceinline__ void fanin_finish(int redop, A acc, A* partials,
                                             unsigned int* ticket,
                                             unsigned int base, A* out,
                                             unsigned long long seq,
                                             A* sh) {
    if (threadIdx.x == 0) {
        publish_partial(partials + blockIdx.x, acc);
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned int t = __hip_atomic_fetch_add(
            ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh[RTPB / 64] = (t - base == gridDim.x - 1) ? (A)1 : (A)0;
    }
    __syncthreads();
    if (sh[RTPB / 64] == (A)0) return;
    // guide order: the fence, that lane's vmcnt wait, the barrier
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    A facc = RedIdent<A>::get(redop);
    for (unsigned int j = threadIdx.x; j < gridDim.x; j += RTPB)
        facc = red_comb(redop, facc, partials[j]);
    facc = block_reduce_in(redop, facc, sh);
    if (threadIdx.x == 0) publish_result(out, facc, seq);
}

} // namespace da
