// zkc_ptau_contrib_parse.h -- the host-only reader of section 7 of a powers-of-tau file, the phase-1 ceremony log as THIS library writes it (product code; the layout
// and its limits: include/zkcensus_ptau_contribute.h).
//
// Plain C++17, no HIP, in the manner of zkc_phase2_parse.h: compiled into libzkcensus.so by hipcc (zkc_scale_each.hip) and, with -fsanitize=address,undefined, into
// tests/host/ptau_contrib_parse_asan.cc.  Every read is preceded by a bounds check that cannot wrap, every failure has a text, and nothing is allocated in proportion to
// a count the section merely claims: a record takes at least 1288 bytes, so the section's own size bounds the count.
//
// Layout:  nContributions(u32), then per contribution
//   tauG1(G1 64) tauG2(G2 128) alphaG1(G1 64) betaG1(G1 64) betaG2(G2 128)          the five points AFTER the contribution: T_1, U_1, A_0, B_0, beta2
//   for tau, alpha, beta in this order: g1_s(G1 64) g1_sx(G1 64) g2_spx(G2 128)      the three proofs of knowledge
//   transcript(64) type(u32 = 0) paramsLen(u32) params(paramsLen)
//   params: a list of items  0x01 len name[len]
// Points are affine with little-endian Montgomery coordinates, like the rest of the file.  The reader checks the framing only: whether a point is on its curve is the
// verifier's question (zkc_ptau_verify_contributions).
#pragma once
#include "zkc_hostparse.h"

namespace zkc { namespace parse {

constexpr size_t PC_POINTS = 64 + 128 + 64 + 64 + 128;     // 448: the five points
constexpr size_t PC_POK = 64 + 64 + 128;                   // 256: one proof of knowledge
constexpr size_t PC_FIXED = PC_POINTS + 3 * PC_POK + 64 + 8;      // 1288: the fixed part of a record
constexpr uint32_t PC_TYPE_PLAIN = 0;
struct PcRecord {
    const uint8_t* rec; size_t rec_len;                    // the whole record inside the section
    const uint8_t *tauG1, *tauG2, *alphaG1, *betaG1, *betaG2;
    const uint8_t* pok[3];                                 // tau, alpha, beta: g1_s at +0, g1_sx at +64, g2_spx at +128
    const uint8_t* transcript;
    uint32_t type, paramsLen;
    const uint8_t* name; uint32_t nameLen;                 // name: NULL when the record has none
};
struct PcSection { uint32_t n = 0; const uint8_t* records = nullptr; size_t records_len = 0; std::vector<PcRecord> rec; };

inline bool ptau_contrib_section(const uint8_t* sec, uint64_t len, PcSection& out, std::string& err) {
    out.rec.clear(); out.n = 0; out.records = nullptr; out.records_len = 0;
    if (!sec || len < 4) { err = "ptau: section 7 is shorter than its count"; return false; }
    out.n = rd32(sec);
    const uint8_t* q = sec + 4; const uint8_t* const end = sec + len;
    if ((uint64_t)out.n * PC_FIXED > (uint64_t)(end - q)) { err = "ptau: the contribution count does not fit section 7"; return false; }
    out.records = q;
    for (uint32_t k = 0; k < out.n; k++) {
        const std::string at = " (record " + std::to_string(k) + ")";
        if ((size_t)(end - q) < PC_FIXED) { err = "ptau: truncated contribution record" + at; return false; }
        PcRecord r{}; r.rec = q;
        r.tauG1 = q; r.tauG2 = q + 64; r.alphaG1 = q + 192; r.betaG1 = q + 256; r.betaG2 = q + 320;
        for (int i = 0; i < 3; i++) r.pok[i] = q + PC_POINTS + PC_POK * (size_t)i;
        r.transcript = q + PC_POINTS + 3 * PC_POK;
        r.type = rd32(r.transcript + 64); r.paramsLen = rd32(r.transcript + 68); q += PC_FIXED;
        if (r.type != PC_TYPE_PLAIN) { err = "ptau: unknown contribution type " + std::to_string(r.type) + at; return false; }
        if (r.paramsLen > (uint64_t)(end - q)) { err = "ptau: truncated contribution record: paramsLen reaches beyond section 7" + at; return false; }
        const uint8_t* const pend = q + r.paramsLen;
        while (q < pend) {
            const uint8_t tag = *q++;
            if (tag != 0x01) { err = "ptau: unknown parameter tag " + std::to_string(tag) + at; return false; }
            if (pend - q < 1 || (size_t)(pend - q - 1) < q[0]) { err = "ptau: truncated parameter" + at; return false; }
            r.name = q + 1; r.nameLen = q[0];
            q += 1 + (size_t)r.nameLen;
        }
        r.rec_len = (size_t)(q - r.rec);
        out.rec.push_back(r);
    }
    if (q != end) { err = "ptau: bytes after the last contribution record"; return false; }
    out.records_len = (size_t)(q - out.records);
    return true;
}

}}  // namespace zkc::parse
