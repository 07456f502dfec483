// phase2_parse_asan.cc -- the host-only reader of a .zkey's section 10 (csrc/zkc_phase2_parse.h) under AddressSanitizer + UBSan, as a plain program with no arguments.
// It builds a valid section (three records: no name item, a 64-byte name, a beacon with all three items) inside a small binfile image, parses it, then every prefix
// of the section, every prefix of the image, and every single-byte mutation of the section's framing bytes plus a few thousand seeded ones anywhere.  Every image sits
// in a heap block of exactly its size, so a read past its end is reported; a parse that succeeds has every pointer of every record checked to lie inside the image and
// its bytes read.  BLAKE2b runs over every length up to 300 under the same sanitizers.  Built and run by tests/test_phase2_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_phase2_parse.h"

using namespace zkc::parse;

static uint64_t g_sum = 0;
static void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { uint8_t b[8]; memcpy(b, &v, 8); o.insert(o.end(), b, b + 8); }
static void fill(std::vector<uint8_t>& o, size_t n, uint8_t seed) { for (size_t i = 0; i < n; i++) o.push_back((uint8_t)(seed + 7 * i)); }
static void record(std::vector<uint8_t>& o, uint32_t type, const std::vector<uint8_t>& params, uint8_t seed) {
    fill(o, 3 * 64 + 128 + 64, seed); put32(o, type); put32(o, (uint32_t)params.size()); o.insert(o.end(), params.begin(), params.end());
}
static std::vector<uint8_t> valid_section() {
    std::vector<uint8_t> s; fill(s, 64, 1); put32(s, 3);
    record(s, 0, {}, 10);
    std::vector<uint8_t> p = {0x01, 64}; fill(p, 64, 'a'); record(s, 0, p, 20);
    std::vector<uint8_t> b = {0x01, 3, 'e', 'n', 'd', 0x02, 10, 0x03, 32}; fill(b, 32, 99); record(s, 1, b, 30);
    return s;
}
static bool inside(const uint8_t* p, size_t n, const uint8_t* base, size_t len) { return p >= base && p + n <= base + len; }
// the section at `exact` is a heap block of exactly len bytes.  1 parsed, 0 refused; aborts on a record that points outside it
static int run_exact(const uint8_t* exact, size_t len) {
    P2Section s; std::string err;
    if (!phase2_section(exact, len, s, err)) { if (err.empty()) { fprintf(stderr, "refused without a text\n"); abort(); } return 0; }
    if (s.rec.size() != s.n || !inside(s.records, s.records_len, exact, len)) { fprintf(stderr, "records outside the section\n"); abort(); }
    size_t total = 0;
    for (const P2Record& r : s.rec) {
        if (!inside(r.rec, r.rec_len, exact, len) || r.rec_len != P2_FIXED + r.paramsLen) { fprintf(stderr, "a record outside the section\n"); abort(); }
        if ((r.name && !inside(r.name, r.nameLen, r.rec, r.rec_len)) || (r.beaconHash && !inside(r.beaconHash, r.beaconLen, r.rec, r.rec_len))) { fprintf(stderr, "a parameter outside its record\n"); abort(); }
        for (size_t i = 0; i < r.rec_len; i++) g_sum += r.rec[i];
        for (uint32_t i = 0; r.name && i < r.nameLen; i++) g_sum += r.name[i];
        for (uint32_t i = 0; r.beaconHash && i < r.beaconLen; i++) g_sum += r.beaconHash[i];
        total += r.rec_len;
    }
    if (total != s.records_len) { fprintf(stderr, "the records do not cover the section\n"); abort(); }
    return 1;
}
static int run(const uint8_t* src, size_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) memcpy(exact.get(), src, len);
    return run_exact(exact.get(), len);
}
static int run_image(const uint8_t* src, size_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) memcpy(exact.get(), src, len);
    BinSections bs; P2Section s; std::string err;
    if (!phase2_of_zkey(exact.get(), len, bs, s, err)) { if (err.empty()) { fprintf(stderr, "refused without a text\n"); abort(); } return 0; }
    for (const P2Record& r : s.rec) for (size_t i = 0; i < r.rec_len; i++) g_sum += r.rec[i];
    return 1;
}

int main() {
    const std::vector<uint8_t> sec = valid_section();
    {
        P2Section s; std::string err;
        if (!phase2_section(sec.data(), sec.size(), s, err)) { fprintf(stderr, "valid section refused: %s\n", err.c_str()); return 1; }
        if (s.n != 3 || s.rec[0].name || s.rec[1].nameLen != 64 || s.rec[2].type != 1 || !s.rec[2].hasIterExp || s.rec[2].iterExp != 10 || s.rec[2].beaconLen != 32 || s.rec[2].nameLen != 3) {
            fprintf(stderr, "valid section misread\n"); return 1; }
        if (run(sec.data(), sec.size()) != 1) return 1;
    }
    size_t refused = 0, parsed = 0;
    for (size_t n = 0; n < sec.size(); n++) { if (run(sec.data(), n)) { fprintf(stderr, "prefix of %zu bytes parsed\n", n); return 1; } refused++; }
    // the section inside a binfile image, section 10 last or followed by another section; every prefix of the image
    for (int trailing = 0; trailing < 2; trailing++) {
        std::vector<uint8_t> img = {'z', 'k', 'e', 'y'}; put32(img, 1); put32(img, trailing ? 3 : 2);
        put32(img, 1); put64(img, 4); put32(img, 1);
        put32(img, 10); put64(img, sec.size()); img.insert(img.end(), sec.begin(), sec.end());
        if (trailing) { put32(img, 3); put64(img, 8); put64(img, 0); }
        if (run_image(img.data(), img.size()) != 1) { fprintf(stderr, "valid image refused\n"); return 1; }
        for (size_t n = 0; n < img.size(); n++) { if (run_image(img.data(), n) && !(trailing && n >= img.size() - 20)) { fprintf(stderr, "image prefix of %zu bytes parsed\n", n); return 1; } }
        std::vector<uint8_t> none(img.begin(), img.begin() + 12 + 12 + 4); memcpy(none.data() + 8, "\x01\0\0\0", 4);
        if (run_image(none.data(), none.size())) { fprintf(stderr, "an image without section 10 parsed\n"); return 1; }
    }
    // every value of every framing byte: the count, and each record's type, paramsLen and parameter bytes
    std::unique_ptr<uint8_t[]> m(new uint8_t[sec.size()]); memcpy(m.get(), sec.data(), sec.size());
    std::vector<size_t> framing; for (size_t i = 64; i < 68; i++) framing.push_back(i);
    { P2Section s; std::string err; phase2_section(sec.data(), sec.size(), s, err);
      for (const P2Record& r : s.rec) for (size_t i = 384; i < r.rec_len; i++) framing.push_back((size_t)(r.rec - sec.data()) + i); }
    for (size_t at : framing) for (int v = 0; v < 256; v++) { const uint8_t old = m[at]; m[at] = (uint8_t)v; run_exact(m.get(), sec.size()) ? parsed++ : refused++; m[at] = old; }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int k = 0; k < 3000; k++) {
        const size_t at = next() % sec.size(); const uint8_t old = m[at]; uint8_t v = (uint8_t)next(); if (v == old) v ^= 0x80;
        m[at] = v; run_exact(m.get(), sec.size()) ? parsed++ : refused++; m[at] = old;
    }
    // BLAKE2b over exactly-sized blocks of every length up to 300
    for (size_t n = 0; n <= 300; n++) {
        std::unique_ptr<uint8_t[]> d(new uint8_t[n ? n : 1]); for (size_t i = 0; i < n; i++) d[i] = (uint8_t)(i * 31 + n);
        uint8_t out[64]; blake2b512(d.get(), n, out); g_sum += out[0] + out[63];
    }
    printf("phase2 reader: ok (%zu refused, %zu parsed within bounds, checksum %llu)\n", refused, parsed, (unsigned long long)g_sum);
    return 0;
}
