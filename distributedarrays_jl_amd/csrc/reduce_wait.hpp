// reduce_wait.hpp — the host side of the flat reduce's result hand-off:
// a bounded spin on the sequence word of the pinned result slot.  Plain
// C++, no HIP: kernels_reduce.hip calls it on memory the device writes,
// tests/reduce_wait_host.cpp on memory another thread writes.
//
// Slot layout (16 bytes, 8-byte aligned): { 8-byte value, 64-bit seq }.
// The writer stores the value, then release-stores seq; a reader whose
// acquire load returns seq may read the value.  seq grows by one per
// waited launch and never repeats (64 bits), so "equals" cannot match a
// stale publication.
#pragma once
#include <stdint.h>
#include <string.h>
#include <chrono>

namespace da {

struct RedSlot {
    unsigned char value[8];
    uint64_t seq;
};
static_assert(sizeof(RedSlot) == 16, "pinned result slot is 16 bytes");

inline void cpu_pause() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ volatile("yield");
#endif
}

constexpr unsigned RED_POLLS_PER_CLOCK = 256;

// Polls slot->seq (acquire) until it equals `seq` or `budget_us` has
// passed; the clock is read once per RED_POLLS_PER_CLOCK polls.  true:
// seq arrived and `bytes` (<= 8) of the value are in *out.  false: the
// budget ran out, *out is untouched.  Never blocks longer than the
// budget plus one batch of polls.
inline bool red_wait(const RedSlot* slot, uint64_t seq, uint64_t budget_us,
                     void* out, size_t bytes) {
    using clock = std::chrono::steady_clock;
    const clock::time_point deadline =
        clock::now() + std::chrono::microseconds(budget_us);
    for (;;) {
        for (unsigned k = 0; k < RED_POLLS_PER_CLOCK; ++k) {
            if (__atomic_load_n(&slot->seq, __ATOMIC_ACQUIRE) == seq) {
                memcpy(out, slot->value, bytes);
                return true;
            }
            cpu_pause();
        }
        if (clock::now() >= deadline) return false;
    }
}

} // namespace da
