// switches_host.cc -- what the accessors of csrc/zkc_switches.h return, printed for tests/test_switches_cpu.py (which holds the expected values) and built by it with
// g++ -fsanitize=address,undefined.  One representative switch of each kind, each fed: unset, "", "0", "1", "2", "abc", "-5" and a value above its clamp.
//   switches_host live      the LIVE switches, value after value in this one process (that they follow the environment is part of what is shown)
//   switches_host process   the PROCESS switches under the environment the caller set, then the caching contract
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_switches.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace sw = zkc::sw;

static void put(const char* name, const char* v) { if (v) setenv(name, v, 1); else unsetenv(name); }
template <sw::Id I> static void show_given(const char* label) {
    const auto g = sw::given<I>();
    if (g) printf("%s %s given %lld\n", sw::rows[I].name, label, *g); else printf("%s %s absent\n", sw::rows[I].name, label);
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "live")) {
        const char* vals[] = {nullptr, "", "0", "1", "2", "abc", "-5", "100000", "18446744073709551615"};
        const char* labels[] = {"unset", "empty", "0", "1", "2", "abc", "-5", "100000", "2^64-1"};
        for (int k = 0; k < 9; k++) {
            const char* v = vals[k]; const char* l = labels[k];
            if (k == 8) {      // past 63 bits: for the one switch that is parsed as an unsigned 64-bit number
                put("ZKC_SMT_WAVE_MAX", v); printf("ZKC_SMT_WAVE_MAX %s value %zu\n", l, (size_t)sw::value<sw::ZKC_SMT_WAVE_MAX>(64)); break;
            }
            for (const char* n : {"ZKC_NO_FOLD", "ZKC_BLIND_TREE", "ZKC_DEVICE_BLOCKING_SYNC", "ZKC_INFLIGHT", "ZKC_C_DEEP", "ZKC_SERVICE_BUSY_WAIT_US", "ZKC_TEST_FAIL_ALLOC",
                                  "ZKC_VERIFY_BATCH_GPU", "ZKC_VERIFY_CHUNK", "ZKC_SMT_WAVE_MAX", "ZKC_DEVICE"}) put(n, v);
            printf("ZKC_NO_FOLD %s on %d\n", l, (int)sw::on<sw::ZKC_NO_FOLD>());
            printf("ZKC_BLIND_TREE %s on %d\n", l, (int)sw::on<sw::ZKC_BLIND_TREE>());
            printf("ZKC_DEVICE_BLOCKING_SYNC %s on %d\n", l, (int)sw::on<sw::ZKC_DEVICE_BLOCKING_SYNC>());
            show_given<sw::ZKC_INFLIGHT>(l); show_given<sw::ZKC_C_DEEP>(l); show_given<sw::ZKC_SERVICE_BUSY_WAIT_US>(l); show_given<sw::ZKC_TEST_FAIL_ALLOC>(l);
            printf("ZKC_VERIFY_BATCH_GPU %s value %d\n", l, (int)sw::value<sw::ZKC_VERIFY_BATCH_GPU>(-1));
            printf("ZKC_VERIFY_CHUNK %s value %u\n", l, (unsigned)sw::value<sw::ZKC_VERIFY_CHUNK>(16384));
            printf("ZKC_SMT_WAVE_MAX %s value %zu\n", l, (size_t)sw::value<sw::ZKC_SMT_WAVE_MAX>(64));
            const char* t = sw::text<sw::ZKC_DEVICE>();
            printf("ZKC_DEVICE %s text %s\n", l, t ? (*t ? t : "(empty)") : "(null)");
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "process")) {
        printf("ZKC_G2_LATE on %d\n", (int)sw::on<sw::ZKC_G2_LATE>());
        printf("ZKC_MATVEC_UNITS on %d\n", (int)sw::on<sw::ZKC_MATVEC_UNITS>());
        printf("ZKC_REDUCE_STREAM on %d\n", (int)sw::on<sw::ZKC_REDUCE_STREAM>());
        printf("ZKC_WITNESS_GROUP value %d\n", (int)sw::value<sw::ZKC_WITNESS_GROUP>(8));
        printf("ZKC_DEEP_WIRES value %zu\n", (size_t)sw::value<sw::ZKC_DEEP_WIRES>(16000));
        printf("ZKC_VW_BIG value %u\n", (uint32_t)sw::value<sw::ZKC_VW_BIG>(0));
        // a PROCESS switch keeps its first value ...
        put("ZKC_WITNESS_GROUP", "3"); put("ZKC_G2_LATE", "1"); put("ZKC_REDUCE_STREAM", "1");
        printf("again ZKC_WITNESS_GROUP value %d\n", (int)sw::value<sw::ZKC_WITNESS_GROUP>(8));
        printf("again ZKC_G2_LATE on %d\n", (int)sw::on<sw::ZKC_G2_LATE>());
        printf("again ZKC_REDUCE_STREAM on %d\n", (int)sw::on<sw::ZKC_REDUCE_STREAM>());
        // ... but only from ITS first read: another one, set after those reads and not read before, sees its value
        put("ZKC_NTT_RADIX", "1"); put("ZKC_G2_ACC_HOLD", "0");
        printf("late ZKC_NTT_RADIX value %d\n", (int)sw::value<sw::ZKC_NTT_RADIX>(4));
        printf("late ZKC_G2_ACC_HOLD on %d\n", (int)sw::on<sw::ZKC_G2_ACC_HOLD>());
        put("ZKC_NTT_RADIX", nullptr);
        printf("again ZKC_NTT_RADIX value %d\n", (int)sw::value<sw::ZKC_NTT_RADIX>(4));
        // a LIVE one follows the environment
        put("ZKC_INFLIGHT", "5"); show_given<sw::ZKC_INFLIGHT>("first");
        put("ZKC_INFLIGHT", "7"); show_given<sw::ZKC_INFLIGHT>("second");
        put("ZKC_INFLIGHT", nullptr); show_given<sw::ZKC_INFLIGHT>("third");
        return 0;
    }
    fprintf(stderr, "usage: switches_host live | process\n");
    return 2;
}
