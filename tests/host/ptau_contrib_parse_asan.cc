// ptau_contrib_parse_asan.cc -- the host-only reader of a .ptau's section 7 as this library writes it (csrc/zkc_ptau_contrib_parse.h) under AddressSanitizer + UBSan, as
// a plain program with no arguments.  It builds a valid section (three records: no name item, a 64-byte name, a short name), parses it, then every prefix of the
// section and every single-byte mutation of the section's framing bytes plus a few thousand seeded ones anywhere.  Every section sits in a heap block of exactly its
// size, so a read past its end is reported; a parse that succeeds has every pointer of every record checked to lie inside the section and its bytes read.  Built and
// run by tests/test_ptau_contribute_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_ptau_contrib_parse.h"

using namespace zkc::parse;

static uint64_t g_sum = 0;
static void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
static void fill(std::vector<uint8_t>& o, size_t n, uint8_t seed) { for (size_t i = 0; i < n; i++) o.push_back((uint8_t)(seed + 7 * i)); }
static void record(std::vector<uint8_t>& o, uint32_t type, const std::vector<uint8_t>& params, uint8_t seed) {
    fill(o, PC_POINTS + 3 * PC_POK + 64, seed); put32(o, type); put32(o, (uint32_t)params.size()); o.insert(o.end(), params.begin(), params.end());
}
static std::vector<uint8_t> valid_section() {
    std::vector<uint8_t> s; put32(s, 3);
    record(s, 0, {}, 10);
    std::vector<uint8_t> p = {0x01, 64}; fill(p, 64, 'a'); record(s, 0, p, 20);
    std::vector<uint8_t> b = {0x01, 3, 'e', 'n', 'd'}; record(s, 0, b, 30);
    return s;
}
static bool inside(const uint8_t* p, size_t n, const uint8_t* base, size_t len) { return p >= base && p + n <= base + len; }
// the section at `exact` is a heap block of exactly len bytes.  1 parsed, 0 refused; aborts on a record that points outside it
static int run_exact(const uint8_t* exact, size_t len) {
    PcSection s; std::string err;
    if (!ptau_contrib_section(exact, len, s, err)) { if (err.empty()) { fprintf(stderr, "refused without a text\n"); abort(); } return 0; }
    if (s.rec.size() != s.n || !inside(s.records, s.records_len, exact, len)) { fprintf(stderr, "records outside the section\n"); abort(); }
    size_t total = 0;
    for (const PcRecord& r : s.rec) {
        if (!inside(r.rec, r.rec_len, exact, len) || r.rec_len != PC_FIXED + r.paramsLen) { fprintf(stderr, "a record outside the section\n"); abort(); }
        if (r.name && !inside(r.name, r.nameLen, r.rec, r.rec_len)) { fprintf(stderr, "a parameter outside its record\n"); abort(); }
        const uint8_t* const pts[5] = {r.tauG1, r.tauG2, r.alphaG1, r.betaG1, r.betaG2}; const size_t width[5] = {64, 128, 64, 64, 128};
        for (int i = 0; i < 5; i++) { if (!inside(pts[i], width[i], r.rec, r.rec_len)) { fprintf(stderr, "a point outside its record\n"); abort(); } for (size_t j = 0; j < width[i]; j++) g_sum += pts[i][j]; }
        for (int i = 0; i < 3; i++) { if (!inside(r.pok[i], PC_POK, r.rec, r.rec_len)) { fprintf(stderr, "a proof of knowledge outside its record\n"); abort(); } for (size_t j = 0; j < PC_POK; j++) g_sum += r.pok[i][j]; }
        if (!inside(r.transcript, 72, r.rec, r.rec_len)) { fprintf(stderr, "a transcript outside its record\n"); abort(); }
        for (size_t i = 0; i < r.rec_len; i++) g_sum += r.rec[i];
        for (uint32_t i = 0; r.name && i < r.nameLen; i++) g_sum += r.name[i];
        total += r.rec_len;
    }
    if (total != s.records_len || 4 + total != len) { fprintf(stderr, "the records do not cover the section\n"); abort(); }
    return 1;
}
static int run(const uint8_t* src, size_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) memcpy(exact.get(), src, len);
    return run_exact(exact.get(), len);
}

int main() {
    const std::vector<uint8_t> sec = valid_section();
    {
        PcSection s; std::string err;
        if (!ptau_contrib_section(sec.data(), sec.size(), s, err)) { fprintf(stderr, "valid section refused: %s\n", err.c_str()); return 1; }
        if (s.n != 3 || s.rec[0].name || s.rec[1].nameLen != 64 || s.rec[2].nameLen != 3 || memcmp(s.rec[2].name, "end", 3) || s.rec[1].rec_len != PC_FIXED + 66) {
            fprintf(stderr, "valid section misread\n"); return 1; }
        if (run(sec.data(), sec.size()) != 1) return 1;
        const uint8_t none[4] = {0, 0, 0, 0};
        if (run(none, 4) != 1 || run(nullptr, 0) != 0) { fprintf(stderr, "the empty sections misread\n"); return 1; }
        if (ptau_contrib_section(nullptr, 100, s, err)) { fprintf(stderr, "no section parsed\n"); return 1; }
    }
    size_t refused = 0, parsed = 0;
    for (size_t n = 0; n < sec.size(); n++) { if (run(sec.data(), n)) { fprintf(stderr, "prefix of %zu bytes parsed\n", n); return 1; } refused++; }
    { std::vector<uint8_t> more = sec; more.push_back(0); if (run(more.data(), more.size())) { fprintf(stderr, "trailing byte parsed\n"); return 1; } refused++; }
    // every value of every framing byte: the count, and each record's type, paramsLen and parameter bytes
    std::unique_ptr<uint8_t[]> m(new uint8_t[sec.size()]); memcpy(m.get(), sec.data(), sec.size());
    std::vector<size_t> framing; for (size_t i = 0; i < 4; i++) framing.push_back(i);
    { PcSection s; std::string err; ptau_contrib_section(sec.data(), sec.size(), s, err);
      for (const PcRecord& r : s.rec) for (size_t i = PC_FIXED - 8; i < r.rec_len; i++) framing.push_back((size_t)(r.rec - sec.data()) + i); }
    for (size_t at : framing) for (int v = 0; v < 256; v++) { const uint8_t old = m[at]; m[at] = (uint8_t)v; run_exact(m.get(), sec.size()) ? parsed++ : refused++; m[at] = old; }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int k = 0; k < 3000; k++) {
        const size_t at = next() % sec.size(); const uint8_t old = m[at]; uint8_t v = (uint8_t)next(); if (v == old) v ^= 0x80;
        m[at] = v; run_exact(m.get(), sec.size()) ? parsed++ : refused++; m[at] = old;
    }
    // ... and a few thousand truncations of mutated sections
    for (int k = 0; k < 3000; k++) {
        const size_t at = next() % sec.size(), len = next() % (sec.size() + 1); const uint8_t old = m[at]; m[at] = (uint8_t)next();
        run(m.get(), len) ? parsed++ : refused++; m[at] = old;
    }
    printf("ptau contribution parser: ok (%zu refused, %zu parsed within bounds, checksum %llu)\n", refused, parsed, (unsigned long long)g_sum);
    return 0;
}
