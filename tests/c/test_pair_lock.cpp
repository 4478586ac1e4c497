// Host test of the two-keyset helpers of picotls_amd/csrc/host/runtime.h that need no device (PairLock and
// check_quic_args; launch_and_note_both records events) on stub keysets, for a thread sanitizer: no HIP call is made.
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Ipicotls_amd/csrc \
//       tests/c/test_pair_lock.cpp -o tests/c/_bin/test_pair_lock -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lpthread
//   tests/c/_bin/test_pair_lock        (exit status 0 and no sanitizer report = pass)
//
// Two threads take the pair with the roles swapped, 20000 times each, while a third takes one keyset in both roles:
// with the mutexes taken in role order the first two deadlock, and a second lock of the one mutex would never return.
// What the pair guards is a plain counter per keyset, so a lock that did not hold would show as a data race.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "picotls/mi355x.h"

typedef uint32_t u32;
typedef uint64_t u64;
struct KeyEntry {  // (runtime.h's pools hold pointers to it)
    uint8_t bytes[512];
};

#include "host/runtime.h"

static int set_kernel_attrs(void) { return 0; }  // (declared by runtime.h, defined by host/aesgcm.h in the engine)

struct StubKeyset {  // what PairLock, launch_and_note_both and check_quic_args use of a keyset
    std::mutex mu;
    StreamUses uses;
    DeviceState *ds = nullptr;
    int device = 0;
    long calls = 0;  // guarded by mu
};

static void hammer(StubKeyset *ks, StubKeyset *hp_ks, int rounds)
{
    for (int i = 0; i < rounds; ++i) {
        PairLock<StubKeyset> locks(ks, hp_ks);
        if (!locks.ks_lock.owns_lock() || locks.hp_lock.owns_lock() != (hp_ks != ks))
            abort();
        ++ks->calls;
        if (hp_ks != ks)
            ++hp_ks->calls;
    }
}

int main(void)
{
    (void)set_kernel_attrs;
    StubKeyset a, b;
    const int rounds = 20000;
    std::thread t1(hammer, &a, &b, rounds), t2(hammer, &b, &a, rounds), t3(hammer, &a, &a, rounds);
    t1.join(), t2.join(), t3.join();
    int fails = 0;
    if (a.calls != 3L * rounds || b.calls != 2L * rounds)
        fails += printf("FAIL: %ld and %ld guarded increments, expected %ld and %ld\n", a.calls, b.calls, 3L * rounds, 2L * rounds);

    // the argument check: its messages carry the caller's prefix
    uint8_t x = 0;
    StubKeyset other;
    other.device = 1;
    if (check_quic_args("quic packets", &a, &b, true, &x, 1, &x, &x, &x, &x) != 0 ||
        check_quic_args("quic packets", &a, &b, false, &x, 1, &x, &x, nullptr, nullptr) != 0 ||
        check_quic_args("quic packets", &a, &b, true, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != 0)
        fails += printf("FAIL: good arguments refused\n");
    if (check_quic_args("quic packets", &a, (StubKeyset *)nullptr, false, &x, 1, &x, &x, nullptr, nullptr) != -1 ||
        strcmp(g_err, "quic packets: invalid arguments") != 0)
        fails += printf("FAIL: a missing hp_ks: %s\n", g_err);
    if (check_quic_args("chacha quic packets", &a, &b, true, &x, 1, &x, &x, &x, nullptr) != -1 ||
        strcmp(g_err, "chacha quic packets: invalid arguments") != 0)
        fails += printf("FAIL: an open without results: %s\n", g_err);
    if (check_quic_args("chacha quic packets", &a, &other, false, &x, 1, &x, &x, nullptr, nullptr) != -1 ||
        strcmp(g_err, "chacha quic packets: hp_ks is on another device than ks") != 0)
        fails += printf("FAIL: another device: %s\n", g_err);
    printf(fails ? "test_pair_lock: FAILED\n" : "test_pair_lock: ok\n");
    return fails != 0;
}
