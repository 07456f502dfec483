// zkc_phase2_parse.h -- the host-only reader of section 10 of a Groth16 .zkey, the phase-2 ceremony log (product code), and BLAKE2b-512, the ceremony's hash.
//
// Plain C++17, no HIP, in the manner of zkc_r1cs_parse.h: compiled into libzkcensus.so by hipcc (zkc_phase2.hip) and, with -fsanitize=address,undefined, into
// tests/host/phase2_parse_asan.cc.  Every read is preceded by a bounds check that cannot wrap, every failure has a text, and nothing is allocated in proportion to a
// count the image merely claims: a record takes at least 392 bytes, so the section's own size bounds the count.
//
// Layout (snarkjs zkey_utils.js writeMPCParams / writeContribution, restated from memory: DESIGN.md section 7 says what has not been run against a snarkjs-written file):
//   csHash(64) nContributions(u32), then per contribution
//   deltaAfter(G1 64) g1_s(G1 64) g1_sx(G1 64) g2_spx(G2 128) transcript(64) type(u32) paramsLen(u32) params(paramsLen)
//   params: a list of items  0x01 len name[len]  |  0x02 iterExp  |  0x03 len beaconHash[len]   (0x02 and 0x03 in a type-1, beacon, record only)
// Points are affine with little-endian Montgomery coordinates, like the rest of the file.  The reader checks the framing only: whether a point is on its curve is the
// verifier's question (zkc_zkey_verify_contributions).
#pragma once
#include "zkc_hostparse.h"

namespace zkc { namespace parse {

// ---- BLAKE2b-512, unkeyed (RFC 7693) ----
struct Blake2b {
    uint64_t h[8]; uint64_t t0 = 0, t1 = 0; uint8_t buf[128]; size_t fill = 0;
    static uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
    static const uint64_t* iv() {
        static const uint64_t k[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                      0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
        return k;
    }
    Blake2b() { for (int i = 0; i < 8; i++) h[i] = iv()[i]; h[0] ^= 0x01010040ull; }       // digest length 64, no key, fanout 1, depth 1
    void compress(const uint8_t* block, bool last) {
        static const uint8_t sigma[12][16] = {
            {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}, {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
            {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8}, {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
            {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10}, {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
            {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
        uint64_t m[16], v[16];
        for (int i = 0; i < 16; i++) m[i] = rd64(block + 8 * i);
        for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = iv()[i]; }
        v[12] ^= t0; v[13] ^= t1; if (last) v[14] = ~v[14];
        auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
            v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 32); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 24);
            v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 63);
        };
        for (int r = 0; r < 12; r++) {
            const uint8_t* s = sigma[r];
            G(0, 4, 8, 12, m[s[0]], m[s[1]]); G(1, 5, 9, 13, m[s[2]], m[s[3]]); G(2, 6, 10, 14, m[s[4]], m[s[5]]); G(3, 7, 11, 15, m[s[6]], m[s[7]]);
            G(0, 5, 10, 15, m[s[8]], m[s[9]]); G(1, 6, 11, 12, m[s[10]], m[s[11]]); G(2, 7, 8, 13, m[s[12]], m[s[13]]); G(3, 4, 9, 14, m[s[14]], m[s[15]]);
        }
        for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
    }
    void count(uint64_t n) { t0 += n; if (t0 < n) t1++; }
    // a full buffer is compressed only once more input arrives: the last block, full or not, is the one that carries the final flag
    void update(const void* data, size_t n) {
        const uint8_t* p = (const uint8_t*)data;
        while (n) {
            if (fill == 128) { count(128); compress(buf, false); fill = 0; }
            const size_t k = n < 128 - fill ? n : 128 - fill;
            memcpy(buf + fill, p, k); fill += k; p += k; n -= k;
        }
    }
    void final(uint8_t out[64]) {
        count(fill); memset(buf + fill, 0, 128 - fill); compress(buf, true);
        for (int i = 0; i < 8; i++) memcpy(out + 8 * i, &h[i], 8);                           // little endian hosts only, as rd32 / rd64
    }
};
inline void blake2b512(const void* data, size_t n, uint8_t out[64]) { Blake2b b; b.update(data, n); b.final(out); }

// ---- section 10 ----
constexpr size_t P2_HEADER = 68;                        // csHash, nContributions
constexpr size_t P2_FIXED = 3 * 64 + 128 + 64 + 8;      // the fixed part of a record: four points, the transcript, type, paramsLen
constexpr uint32_t P2_TYPE_PLAIN = 0, P2_TYPE_BEACON = 1;
struct P2Record {
    const uint8_t* rec; size_t rec_len;                 // the whole record inside the image
    const uint8_t *deltaAfter, *g1_s, *g1_sx, *g2_spx, *transcript;
    uint32_t type, paramsLen;
    const uint8_t* name; uint32_t nameLen;              // name: NULL when the record has none
    bool hasIterExp; uint32_t iterExp; const uint8_t* beaconHash; uint32_t beaconLen;
};
struct P2Section { const uint8_t* csHash; uint32_t n; const uint8_t* records; size_t records_len; std::vector<P2Record> rec; };

inline bool phase2_section(const uint8_t* sec, uint64_t len, P2Section& out, std::string& err) {
    out.rec.clear(); out.n = 0; out.csHash = nullptr; out.records = nullptr; out.records_len = 0;
    if (!sec || len < P2_HEADER) { err = "phase2: section 10 is shorter than its header"; return false; }
    out.csHash = sec; out.n = rd32(sec + 64);
    const uint8_t* q = sec + P2_HEADER; const uint8_t* const end = sec + len;
    if ((uint64_t)out.n * P2_FIXED > (uint64_t)(end - q)) { err = "phase2: the contribution count does not fit the section"; return false; }
    out.records = q;
    for (uint32_t k = 0; k < out.n; k++) {
        const std::string at = " (record " + std::to_string(k) + ")";
        if ((size_t)(end - q) < P2_FIXED) { err = "phase2: truncated contribution record" + at; return false; }
        P2Record r{}; r.rec = q;
        r.deltaAfter = q; r.g1_s = q + 64; r.g1_sx = q + 128; r.g2_spx = q + 192; r.transcript = q + 320;
        r.type = rd32(q + 384); r.paramsLen = rd32(q + 388); q += P2_FIXED;
        if (r.type != P2_TYPE_PLAIN && r.type != P2_TYPE_BEACON) { err = "phase2: unknown contribution type " + std::to_string(r.type) + at; return false; }
        if (r.paramsLen > (uint64_t)(end - q)) { err = "phase2: paramsLen reaches beyond the section" + at; return false; }
        const uint8_t* const pend = q + r.paramsLen;
        while (q < pend) {
            const uint8_t tag = *q++;
            if (tag == 0x01 || tag == 0x03) {
                if (pend - q < 1 || (size_t)(pend - q - 1) < q[0]) { err = "phase2: truncated parameter" + at; return false; }
                const uint32_t l = q[0];
                if (tag == 0x01) { r.name = q + 1; r.nameLen = l; } else { r.beaconHash = q + 1; r.beaconLen = l; }
                q += 1 + l;
            } else if (tag == 0x02) {
                if (pend - q < 1) { err = "phase2: truncated parameter" + at; return false; }
                r.hasIterExp = true; r.iterExp = *q++;
            } else { err = "phase2: unknown parameter tag " + std::to_string(tag) + at; return false; }
            if (tag != 0x01 && r.type != P2_TYPE_BEACON) { err = "phase2: beacon parameter in a contribution that is no beacon" + at; return false; }
        }
        r.rec_len = (size_t)(q - r.rec);
        out.rec.push_back(r);
    }
    if (q != end) { err = "phase2: bytes after the last contribution record"; return false; }
    out.records_len = (size_t)(q - out.records);
    return true;
}

// a whole .zkey image -> its section table and section 10
inline bool phase2_of_zkey(const uint8_t* buf, size_t len, BinSections& bs, P2Section& out, std::string& err) {
    if (!binfile_sections(buf, len, "zkey", 1, bs, err)) return false;
    if (!bs.sec[10]) { err = "zkey: missing section 10"; return false; }
    return phase2_section(bs.sec[10], bs.ssz[10], out, err);
}

}}  // namespace zkc::parse
