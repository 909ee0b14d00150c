// Stand-alone host check of the flat reduce's result waiter
// (distributedarrays_jl_amd/csrc/reduce_wait.hpp): a thread plays the
// device.  Built by tests/test_reduce_wait_host.py with -fsanitize=thread,
// so a waiter that reads the value without the acquire, or a publish
// order the protocol does not cover, is a reported race (exit 66).
//
//   1. late publish: the writer stores the value and release-stores the
//      sequence 3 ms after the waiter began; the waiter returns it.
//   2. 2000 back-to-back launches, 8- and 4-byte values alternating into
//      the same slot: every wait returns its own launch's value.
//   3. never published (the slot holds the previous sequence, as after a
//      faulted kernel): "timed out" within budget + margin, *out untouched.
//   4. budget 0: one batch of polls, then "timed out".
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "reduce_wait.hpp"

using clk = std::chrono::steady_clock;

static da::RedSlot g_slot;              // zeroed, like the pinned slot
static std::atomic<uint64_t> g_req{0};  // launch k requested

static uint64_t value_of(uint64_t k) { return k * 0x9E3779B97F4A7C15ull + 1; }
static size_t bytes_of(uint64_t k) { return (k & 1) ? 8 : 4; }

// the device side of publish_result: value first, then release the seq
static void publish(uint64_t k) {
    uint64_t v = value_of(k);
    memcpy(g_slot.value, &v, bytes_of(k));
    __atomic_store_n(&g_slot.seq, k, __ATOMIC_RELEASE);
}

static int fail(const char* what, uint64_t k) {
    fprintf(stderr, "FAIL: %s (k=%llu)\n", what, (unsigned long long)k);
    return 1;
}

int main() {
    const uint64_t N = 2000, LONG_US = 5000000;
    std::thread writer([&] {
        for (uint64_t k = 1; k <= N; ++k) {
            while (g_req.load(std::memory_order_acquire) < k)
                da::cpu_pause();
            if (k == 1)
                std::this_thread::sleep_for(std::chrono::milliseconds(3));
            publish(k);
        }
    });
    for (uint64_t k = 1; k <= N; ++k) {
        g_req.store(k, std::memory_order_release);
        uint64_t got = 0, want = 0, v = value_of(k);
        memcpy(&want, &v, bytes_of(k));
        if (!da::red_wait(&g_slot, k, LONG_US, &got, bytes_of(k))) {
            writer.detach();
            return fail("published result timed out", k);
        }
        if (got != want) {
            writer.join();
            return fail("wrong value", k);
        }
    }
    writer.join();

    // 3: nobody publishes N + 1
    const uint64_t budget_us = 20000, margin_us = 2000000;
    uint64_t out = 0x5a5a5a5a5a5a5a5aull;
    clk::time_point t0 = clk::now();
    bool ok = da::red_wait(&g_slot, N + 1, budget_us, &out, 8);
    uint64_t us = (uint64_t)std::chrono::duration_cast<
        std::chrono::microseconds>(clk::now() - t0).count();
    if (ok) return fail("unpublished sequence reported as arrived", N + 1);
    if (out != 0x5a5a5a5a5a5a5a5aull) return fail("timeout wrote *out", N + 1);
    if (us < budget_us) return fail("gave up before the budget", us);
    if (us > budget_us + margin_us) return fail("overran the budget", us);
    const uint64_t timeout_us = us;

    // 4: budget 0
    t0 = clk::now();
    ok = da::red_wait(&g_slot, N + 1, 0, &out, 8);
    us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
        clk::now() - t0).count();
    if (ok) return fail("budget 0 reported an arrival", N + 1);
    if (us > margin_us) return fail("budget 0 overran", us);

    printf("reduce_wait_host ok: %llu publishes, timeout after %llu us\n",
           (unsigned long long)N, (unsigned long long)timeout_us);
    return 0;
}
