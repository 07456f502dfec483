// zkc_host_util.h -- host-side helpers with no other home, once each: the roots of unity of Fr, the generators, points as files and the C ABI carry them, the order of 256-bit integers, an error text
// into a caller's buffer, a millisecond timer, a loop over host threads.  Host only (nothing here is ZKC_HD), internal to the library.
#pragma once
#include <chrono>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "zkc_curve.h"

#pragma GCC visibility push(hidden)
namespace zkc {

// 5^((r - 1) / 2^28) squared down to order 2^logn: ffjavascript's Fr.w[logn]
inline Fr fr_root_of_unity(int logn) {
    uint32_t e[8]; for (int i = 0; i < 8; i++) e[i] = FrParams::p[i]; e[0] -= 1;
    for (int i = 0; i < 8; i++) e[i] = (e[i] >> 28) | (i < 7 ? e[i + 1] << 4 : 0);
    Fr g = fp_from_u32<FrParams>(5), w = Fr::one();
    for (int i = 255; i >= 0; i--) { w = w * w; if ((e[i >> 5] >> (i & 31)) & 1) w = w * g; }
    for (int i = 28; i > logn; i--) w = w * w;
    return w;
}

inline G1Affine g1_generator() { return {Fq::one(), fp_from_u32<FqParams>(2)}; }
inline G2Affine g2_generator() {
    static const uint32_t X0[8] = {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu};
    static const uint32_t X1[8] = {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u};
    static const uint32_t Y0[8] = {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u};
    static const uint32_t Y1[8] = {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
    return {{fp_from_std<FqParams>(X0), fp_from_std<FqParams>(X1)}, {fp_from_std<FqParams>(Y0), fp_from_std<FqParams>(Y1)}};
}

// ---- points, 32 B little-endian per coordinate (G2: x.c0 x.c1 y.c0 y.c1).  rd_*: false for a coordinate >= q (the point is then not to be used) ----
// Montgomery form, as a .zkey stores its points.  Every coordinate is copied whatever the verdict (&, not &&): zkey_load_opts keeps the header points of a key unchecked
inline bool rd_fq_mont(Fq& o, const uint8_t* p) { memcpy(o.v, p, 32); return fp_std_lt_p<FqParams>(o.v); }
inline bool rd_g1_mont(G1Affine& o, const uint8_t* p) { return rd_fq_mont(o.x, p) & rd_fq_mont(o.y, p + 32); }
inline bool rd_g2_mont(G2Affine& o, const uint8_t* p) { return rd_fq_mont(o.x.c0, p) & rd_fq_mont(o.x.c1, p + 32) & rd_fq_mont(o.y.c0, p + 64) & rd_fq_mont(o.y.c1, p + 96); }
inline void wr_g1_mont(uint8_t* p, const G1Affine& a) { memcpy(p, a.x.v, 32); memcpy(p + 32, a.y.v, 32); }
inline void wr_g2_mont(uint8_t* p, const G2Affine& a) { memcpy(p, a.x.c0.v, 32); memcpy(p + 32, a.x.c1.v, 32); memcpy(p + 64, a.y.c0.v, 32); memcpy(p + 96, a.y.c1.v, 32); }
// standard form, as the C ABI and verification_key.json carry them
inline bool rd_fq_std(Fq& o, const uint8_t* p) { uint32_t s[8]; memcpy(s, p, 32); if (!fp_std_lt_p<FqParams>(s)) return false; o = fp_from_std<FqParams>(s); return true; }
inline bool rd_g1_std(G1Affine& o, const uint8_t* p) { return rd_fq_std(o.x, p) && rd_fq_std(o.y, p + 32); }
inline bool rd_g2_std(G2Affine& o, const uint8_t* p) { return rd_fq_std(o.x.c0, p) && rd_fq_std(o.x.c1, p + 32) && rd_fq_std(o.y.c0, p + 64) && rd_fq_std(o.y.c1, p + 96); }
inline void wr_fq_std(uint8_t* p, const Fq& a) { uint32_t s[8]; fp_to_std<FqParams>(s, a); memcpy(p, s, 32); }
inline void wr_g1_std(uint8_t* p, const G1Affine& a) { wr_fq_std(p, a.x); wr_fq_std(p + 32, a.y); }
inline void wr_g2_std(uint8_t* p, const G2Affine& a) { wr_fq_std(p, a.x.c0); wr_fq_std(p + 32, a.x.c1); wr_fq_std(p + 64, a.y.c0); wr_fq_std(p + 96, a.y.c1); }

// a coordinate as a hash takes it: big-endian standard form
inline void be_fq(uint8_t* o, const Fq& a) { uint32_t s[8]; fp_to_std<FqParams>(s, a); for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) o[4 * (7 - i) + (3 - b)] = (uint8_t)(s[i] >> (8 * b)); }
// the "uncompressed" form of a point: x || y, G2 components c1 before c0; infinity = zeros with bit 0x40 of the first byte set
inline void unc_g1(uint8_t o[64], const G1Affine& a) { if (a.is_inf()) { memset(o, 0, 64); o[0] = 0x40; return; } be_fq(o, a.x); be_fq(o + 32, a.y); }
inline void unc_g2(uint8_t o[128], const G2Affine& a) {
    if (a.is_inf()) { memset(o, 0, 128); o[0] = 0x40; return; }
    be_fq(o, a.x.c1); be_fq(o + 32, a.x.c0); be_fq(o + 64, a.y.c1); be_fq(o + 96, a.y.c0);
}

// a secret scalar (standard or Montgomery form): cleared on every way out of its scope, through a volatile pointer so that the stores are not dropped as dead.  wipe does
// the same for any other storage that held something derived from a secret
struct Secret {
    uint32_t v[8] = {0};
    ~Secret() { wipe(v, 32); }
    operator uint32_t*() { return v; }
    static void wipe(void* p, size_t n) { volatile uint8_t* q = (volatile uint8_t*)p; for (size_t i = 0; i < n; i++) q[i] = 0; }
};
struct SecretFr { Fr f = Fr::zero(); ~SecretFr() { Secret::wipe(&f, sizeof f); } };
inline bool std_is_zero(const uint32_t k[8]) { uint32_t o = 0; for (int i = 0; i < 8; i++) o |= k[i]; return o == 0; }

// a < b for two 256-bit integers of eight words, lowest first (standard form)
inline bool std_less(const uint32_t a[8], const uint32_t b[8]) { for (int i = 7; i >= 0; i--) if (a[i] != b[i]) return a[i] < b[i]; return false; }

// the text of an error into the caller's buffer (either may be absent); returns code
inline int err_out(char* err, size_t errlen, int code, const std::string& m) { if (err && errlen) snprintf(err, errlen, "%s", m.c_str()); return code; }

// milliseconds from t0 to t1 (now, when not given)
using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0, clk::time_point t1 = clk::now()) { return std::chrono::duration<double, std::milli>(t1 - t0).count(); }

constexpr unsigned HOST_THREADS = 16;            // of the ctx = NULL paths (zkc_setup_ptau.hip, zkc_ptau_prepare.hip)
// f over [0, n) in chunks of `grain`, handed out to at most HOST_THREADS threads as they come free (equal shares need not be equal work)
inline void par_chunks(size_t n, size_t grain, const std::function<void(size_t, size_t)>& f) {
    unsigned nt = std::thread::hardware_concurrency(); if (nt == 0) nt = 4; if (nt > HOST_THREADS) nt = HOST_THREADS;
    if (n <= grain || nt == 1) { if (n) f(0, n); return; }
    std::atomic<size_t> next{0};
    auto work = [&] { for (;;) { const size_t a = next.fetch_add(grain); if (a >= n) return; f(a, std::min(n, a + grain)); } };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

}  // namespace zkc
#pragma GCC visibility pop
