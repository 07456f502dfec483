// zkc_switches.h -- every ZKC_* environment switch of libzkcensus: one table, and the only getenv of csrc/ (tests/test_switches_cpu.py).
// Host-only and free of HIP headers: zkc_hostparse.h and the sanitizer-built programs under tests/host/ include it.
//
// A call site names the switch and never how to parse it: sw::on<sw::ZKC_NO_FOLD>(), sw::given<sw::ZKC_INFLIGHT>(), sw::value<sw::ZKC_NTT_RADIX>(4), sw::text<sw::ZKC_DEVICE>().
// The accessor is checked against the row's kind at compile time.  INTEGRATION.md "Switches" is the same list for operators.
//
// Kinds -- what the value of the variable means:
//   SET          on when the variable exists, WHATEVER its value: =0 and the empty string switch it on too (kept as it always was; unset the variable to switch it off)
//   OFF_IF_ZERO  on by default; off when the value reads as the number 0 ("0", "", "abc": atoi)
//   ON_IF_ONE    off by default; on when the value reads as the number 1
//   NUMBER       atoi: no digits in front reads as 0; then clamped to [lo, hi] where the row has bounds (ANY: none on that side)
//   NUMBER_LONG  the same through atol (64 bits)
//   NUMBER_U64   the same through strtoull: the caller casts the result back to an unsigned 64-bit type
//   TEXT         the string itself
// Read times -- when the environment is looked at:
//   PROCESS      at the first read of THAT switch, and never again in the process (each switch on its own: reading one does not fix another)
//   LIVE         at every read: every key load, service creation, lane growth, context creation or call, as the row says.  Tests, tools and bench.py set these between two
//                key loads or calls of one process, so a LIVE row must not become a cached one.
#pragma once
#include <climits>
#include <cstdlib>
#include <optional>

namespace zkc { namespace sw {

enum Kind { SET, OFF_IF_ZERO, ON_IF_ONE, NUMBER, NUMBER_LONG, NUMBER_U64, TEXT };
enum When { PROCESS, LIVE };
constexpr long long ANY = LLONG_MIN;      // no bound on this side of a clamp

// X(name, kind, lo, hi, read time, what it is for).  Fixed upper bounds that are constants of the prover (MSM_C_BIG = 17, MSM_MAX_JOBS / 4 = 128, MAX_LANES = 4) are
// written out here, because this header sees no HIP code, and pinned to those constants by static_asserts in zkc_prover.h.
#define ZKC_SWITCHES(X)                                                                                                                                                   \
    /* ---- operator knobs ---- */                                                                                                                                        \
    X(ZKC_DEVICE,               TEXT,        ANY, ANY,   LIVE,    "service creation: the GPUs of the default proving service: \"2\", \"0,1,2,3\", \"all\"; unset: every visible device") \
    X(ZKC_INFLIGHT,             NUMBER,      1,   128,   LIVE,    "key load: proofs per pipeline pass (census key 64, any other 96, fewer for a large circuit); at most MSM_MAX_JOBS / 4") \
    X(ZKC_LANES,                NUMBER,      1,   4,     LIVE,    "key load: pipeline lanes the passes of a batch call rotate over (census key MAX_LANES = 4, any other 1)")      \
    X(ZKC_LANE_STREAMS,         NUMBER,      1,   3,     LIVE,    "key load: streams of a lane that a pass of a call rotating over several lanes uses: 1 all on the G1 stream (default), 2 the G2 MSM on its own, 3 the blinding too") \
    X(ZKC_DEEP_TABLES,          NUMBER,      ANY, ANY,   LIVE,    "key load: 0 leaves out the second section tables that passes of deep voters take, 2 builds them for a census key of any size (default 1)") \
    X(ZKC_G2_LONE_TABLE,        OFF_IF_ZERO, ANY, ANY,   LIVE,    "key load: =0 skips the 8-bit-window G2 table of the lone-proof path")                                          \
    X(ZKC_BLIND_TREE,           OFF_IF_ZERO, ANY, ANY,   LIVE,    "key load: =0 gives a key whose passes of one or two proofs take the general blinding kernels")                 \
    X(ZKC_SERVICE_WORKERS,      NUMBER,      1,   4,     LIVE,    "service creation: workers (= lanes of a service key) per GPU (4); at most MAX_LANES")                          \
    X(ZKC_SERVICE_PASS,         NUMBER,      1,   128,   LIVE,    "service creation: proofs per pass of a service key (64); at most MSM_MAX_JOBS / 4")                            \
    X(ZKC_SERVICE_KEYS,         NUMBER,      1,   64,    LIVE,    "service creation: keys kept resident per GPU (4)")                                                             \
    X(ZKC_SERVICE_MAX_BATCH,    NUMBER,      1,   4096,  LIVE,    "service creation: requests one worker takes per call (256)")                                                   \
    X(ZKC_SERVICE_MIN_BATCH,    NUMBER,      1,   ANY,   LIVE,    "service creation: requests a collecting worker waits for before it goes (16)")                                 \
    X(ZKC_SERVICE_SPILL,        NUMBER,      1,   ANY,   LIVE,    "service creation: queue length at which a cold GPU is brought up (32)")                                        \
    X(ZKC_SERVICE_BUSY_WAIT_US, NUMBER,      0,   ANY,   LIVE,    "service creation: microseconds a collecting worker waits for more requests (300)")                             \
    X(ZKC_SERVICE_RESERVE,      OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: a service key load does not reserve a full pass of work space on every lane; the lanes grow on demand")    \
    X(ZKC_DEVICE_BLOCKING_SYNC, ON_IF_ONE,   ANY, ANY,   LIVE,    "context creation: =1 asks HIP for blocking waits on the device (hipDeviceScheduleBlockingSync)")               \
    X(ZKC_SPIN_WAIT,            SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): host waits use hipEventSynchronize instead of polling with short sleeps")         \
    X(ZKC_VERIFY_BATCH_GPU,     NUMBER,      ANY, ANY,   LIVE,    "per verify call: 0 keeps the Miller loops of zkc_verify_batch on the host, positive forces the GPU, negative or unset: GPU from 128 proofs") \
    X(ZKC_NO_SHA_NI,            SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): portable SHA-256 instead of the CPU's SHA extensions")                            \
    /* ---- measurement and A/B switches ---- */                                                                                                                          \
    X(ZKC_NO_FOLD,              SET,         ANY, ANY,   LIVE,    "key load: set (any value, 0 included): no constant folding of the voter-independent witness part for this key") \
    X(ZKC_SERIAL_STREAMS,       SET,         ANY, ANY,   LIVE,    "key load: set (any value, 0 included): every stage of this key's passes on the context's one stream (isolated stage times)") \
    X(ZKC_C_SECTIONS,           NUMBER,      8,   17,    LIVE,    "key load: window bits of the witness sections (census key 12, any other by its wire count); at most MSM_C_BIG") \
    X(ZKC_C_H,                  NUMBER,      8,   17,    LIVE,    "key load: window bits of the H section (census key 17, any other by its domain size); at most MSM_C_BIG")      \
    X(ZKC_C_DEEP,               NUMBER,      13,  17,    LIVE,    "key load: window bits of the second section tables (by the wire count); at most MSM_C_BIG")                    \
    X(ZKC_DEEP_WIRES,           NUMBER_LONG, ANY, ANY,   PROCESS, "live wires per section and proof from which a pass takes the second section tables (16000)")                   \
    X(ZKC_WITNESS_GROUP,        NUMBER,      1,   ANY,   PROCESS, "passes whose voters share one witness launch in a batch call (8)")                                             \
    X(ZKC_VW_BIG,               NUMBER,      ANY, ANY,   PROCESS, "buckets per reduction wave of the H jobs in passes of more than four proofs (0 or unset: 4096, 1024 below 32 proofs)") \
    X(ZKC_VW_SMALL,             NUMBER,      ANY, ANY,   PROCESS, "the same for the witness sections (0 or unset: 2048, 256 below 32 proofs)")                                    \
    X(ZKC_VW_G2,                NUMBER,      ANY, ANY,   PROCESS, "the same for the G2 jobs of passes of 32 proofs and more (0 or unset: as the witness sections)")              \
    X(ZKC_G2_ACC,               NUMBER,      ANY, ANY,   PROCESS, "form of the G2 accumulation: 0 registers hold the next row, 1 / 2 LDS-DMA prefetch at one / two waves per SIMD (0)") \
    X(ZKC_G2_BUCKET_WAVE,       OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: small G2 passes keep lane-per-segment accumulation instead of half a wave per bucket")                     \
    X(ZKC_G2_LATE,              SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): the G2 MSM of a pass starts after the G1 sort instead of with the pass")          \
    X(ZKC_G2_ACC_HOLD,          SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): the G2 accumulation always waits for the G1 stream to leave its transforms")      \
    X(ZKC_G2_ACC_EARLY,         SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): the G2 accumulation never waits for them (ZKC_G2_ACC_HOLD wins)")                 \
    X(ZKC_ACC_CHAIN,            OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: the G1 accumulations of a context's lanes are not chained one behind the other")                           \
    X(ZKC_REDUCE_STREAM,        ON_IF_ONE,   ANY, ANY,   PROCESS, "=1: the bucket reduction of a full pass runs on a stream of its own (the lanes then get that stream)")         \
    X(ZKC_MATVEC_UNITS,         OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: buildABC multiplies by its +-1 coefficients instead of adding the wire")                                   \
    X(ZKC_ABC_FOLD,             OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: buildABC of a folded pass computes every row instead of copying the voter-independent ones from the template") \
    X(ZKC_TOP_FOLD,             NUMBER,      0,   12,    LIVE,    "key load: census tree levels below the root whose MSM terms are summed once per subtree instead of per voter (8; 0: off)") \
    X(ZKC_C_ROWS,               NUMBER,      0,   2,     LIVE,    "key load: a folded pass leaves out the transform pair of C and adds its voter rows of C to the H job: 0 never, 2 wherever it is legal, 1 or unset by the rule k nw_H <= beta n log2 n") \
    X(ZKC_C_ROWS_BETA,          NUMBER,      0,   100000, LIVE,   "key load: beta of that rule in thousandths (120)")                                                             \
    X(ZKC_MATVEC_INLINE,        SET,        ANY, ANY,   PROCESS, "set (any value, 0 included): buildABC of the next pass is not prefetched on the blinding stream")              \
    X(ZKC_MV_PREFETCH_AT_NTT,   ON_IF_ONE,   ANY, ANY,   PROCESS, "=1: that prefetch starts beside the pass' bucketing instead of beside its accumulation")                       \
    X(ZKC_EARLY_LAYOUT,         OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: one-pass calls of more than two voters wait for their fold flags instead of reading the depths off the inputs") \
    X(ZKC_NOFOLD_LISTS,         OFF_IF_ZERO, ANY, ANY,   PROCESS, "=0: unfolded passes keep the wires whose bases are at infinity")                                               \
    X(ZKC_NTT_SEPARATE,         SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): two self-contained transforms instead of the fused pair")                         \
    X(ZKC_NTT_RADIX,            NUMBER,      ANY, ANY,   PROCESS, "below 4: the head transform kernel runs one stage at a time instead of two (4)")                               \
    X(ZKC_FINALIZE_WAVES,       SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): the one-wave-per-task blinding kernel for every pass")                            \
    X(ZKC_VERIFY_CHUNK,         NUMBER,      2,   16384, LIVE,    "per verify call: pairs per round of Miller-loop kernels (16384)")                                              \
    X(ZKC_SMT_WAVE_MAX,         NUMBER_U64,  ANY, ANY,   LIVE,    "per check call: census proof batches up to this size take the wave-per-proof form (64; 0: never)")            \
    X(ZKC_TRACE_HOST,           SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): prints where the enqueueing thread spends its time, per pass")                    \
    X(ZKC_VERIFY_TRACE,         SET,         ANY, ANY,   LIVE,    "per verify call: set (any value, 0 included): prints the stage times of zkc_verify_batch")                     \
    X(ZKC_DEBUG_SYNC,           SET,         ANY, ANY,   PROCESS, "set (any value, 0 included): synchronises after and logs every MSM launch; read when the library is loaded")   \
    /* ---- test hooks ---- */                                                                                                                                            \
    X(ZKC_TEST_FAIL_ALLOC,      NUMBER,      ANY, ANY,   LIVE,    "lane growth: the work-space allocation for this many proofs in flight or more fails")                          \
    X(ZKC_TEST_TOP_SLOTS,       NUMBER,      1,   16384, LIVE,    "key load: slots per tree of the top-of-tree table instead of 8 x 2^K (1: every subtree lands on one slot)")    \
    X(ZKC_TEST_FAIL_KEY_LOADS,  NUMBER,      ANY, ANY,   LIVE,    "service key load: fails as out of memory while the device holds this many keys or more")

enum Id {
#define X(name, kind, lo, hi, when, doc) name,
    ZKC_SWITCHES(X)
#undef X
    COUNT
};
struct Row { const char* name; Kind kind; long long lo, hi; When when; const char* doc; };
inline constexpr Row rows[COUNT] = {
#define X(name, kind, lo, hi, when, doc) {#name, kind, lo, (hi) == ANY ? LLONG_MAX : (hi), when, doc},
    ZKC_SWITCHES(X)
#undef X
};

struct Raw { bool set; long long num; const char* str; };      // one look at the environment
inline Raw read(const Row& r) {
    const char* e = getenv(r.name);
    if (!e) return {false, 0, nullptr};
    const long long v = r.kind == NUMBER_U64 ? (long long)strtoull(e, nullptr, 10) : r.kind == NUMBER_LONG ? (long long)atol(e) : (long long)atoi(e);
    return {true, v < r.lo ? r.lo : v > r.hi ? r.hi : v, e};
}
template <Id I> inline Raw get() {
    if constexpr (rows[I].when == PROCESS) { static const Raw cached = read(rows[I]); return cached; }
    else return read(rows[I]);
}
constexpr bool is_number(Kind k) { return k == NUMBER || k == NUMBER_LONG || k == NUMBER_U64; }

// the switch is on, by its row's kind and default
template <Id I> inline bool on() {
    static_assert(rows[I].kind == SET || rows[I].kind == OFF_IF_ZERO || rows[I].kind == ON_IF_ONE, "not an on/off switch");
    const Raw r = get<I>();
    return rows[I].kind == SET ? r.set : rows[I].kind == OFF_IF_ZERO ? !(r.set && r.num == 0) : (r.set && r.num == 1);
}
// the clamped number if the variable exists: for a default that depends on the caller
template <Id I> inline std::optional<long long> given() {
    static_assert(is_number(rows[I].kind), "not a number");
    const Raw r = get<I>();
    return r.set ? std::optional<long long>(r.num) : std::nullopt;
}
// the clamped number, or dflt (as it stands) if the variable does not exist
template <Id I> inline long long value(long long dflt) { return given<I>().value_or(dflt); }
template <Id I> inline const char* text() {
    static_assert(rows[I].kind == TEXT && rows[I].when == LIVE, "not a live text switch");
    return get<I>().str;
}

}}  // namespace zkc::sw
