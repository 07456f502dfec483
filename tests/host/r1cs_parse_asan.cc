// r1cs_parse_asan.cc -- the host-only .r1cs reader (csrc/zkc_r1cs_parse.h) under AddressSanitizer + UBSan, as a plain program:
//     r1cs_parse_asan <circuit.r1cs> <nWires> <nPublic> <nConstraints>
// It parses the valid image, every prefix of its first 4 KB, a cut at every section boundary and in mid-constraint, and a few thousand seeded single-byte
// mutations.  Every image sits in a heap block of exactly its size, so a read past its end is reported; a parse that succeeds has every term walked (wire index in
// range, the 32 coefficient bytes read).  Built and run by tests/test_r1cs_parse_asan_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_r1cs_parse.h"

using namespace zkc::parse;

static uint64_t g_sum = 0;
// the image at `exact` is a heap block of exactly len bytes.  returns 1 parsed, 0 refused; aborts on a parse that points outside the image
static int run_exact(const uint8_t* exact, size_t len) {
    R1cs cs; std::string err;
    if (!r1cs_parse(exact, len, cs, err)) { if (err.empty()) { fprintf(stderr, "refused without a text\n"); abort(); } return 0; }
    for (int m = 0; m < 3; m++) {
        if (cs.ptr[m].size() != (size_t)cs.h.nCons + 1 || cs.ptr[m].back() != cs.terms[m].size()) { fprintf(stderr, "row pointers do not cover the terms\n"); abort(); }
        for (const R1csTerm& t : cs.terms[m]) {
            if (t.wire >= cs.h.nWires || t.coef < exact || t.coef + 32 > exact + len) { fprintf(stderr, "a term outside the image\n"); abort(); }
            g_sum += t.coef[0] + t.coef[31];
        }
    }
    return 1;
}
static int run(const uint8_t* src, size_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) memcpy(exact.get(), src, len);
    return run_exact(exact.get(), len);
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: r1cs_parse_asan <circuit.r1cs> <nWires> <nPublic> <nConstraints>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> img; { uint8_t b[65536]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) img.insert(img.end(), b, b + n); } fclose(f);
    // the valid image
    {
        R1cs cs; std::string err;
        if (!r1cs_parse(img.data(), img.size(), cs, err)) { fprintf(stderr, "valid image refused: %s\n", err.c_str()); return 1; }
        if (cs.h.nWires != (uint32_t)atol(argv[2]) || cs.h.nPub != (uint32_t)atol(argv[3]) || cs.h.nCons != (uint32_t)atol(argv[4])) { fprintf(stderr, "header figures differ\n"); return 1; }
        R1csHeader h; std::string e2;
        if (!r1cs_header(img.data(), img.size(), h, nullptr, nullptr, e2) || h.nCons != cs.h.nCons) { fprintf(stderr, "r1cs_header disagrees\n"); return 1; }
        if (run(img.data(), img.size()) != 1) return 1;
    }
    size_t refused = 0, parsed = 0;
    // every prefix of the first 4 KB (none is a whole image)
    for (size_t n = 0; n <= 4096 && n < img.size(); n++) { if (run(img.data(), n)) { fprintf(stderr, "prefix of %zu bytes parsed\n", n); return 1; } refused++; }
    // a cut at every section boundary (before the section's header, inside it, right behind it) and in mid-constraint
    {
        size_t p = 12; const uint32_t ns = rd32(img.data() + 8);
        for (uint32_t i = 0; i < ns && p + 12 <= img.size(); i++) {
            const uint32_t id = rd32(img.data() + p); const uint64_t sz = rd64(img.data() + p + 4);
            const size_t cuts[] = {p, p + 5, p + 12, p + 12 + (size_t)sz / 2, p + 12 + (size_t)sz - 1};
            for (size_t c : cuts) if (c < img.size()) {
                const int ok = run(img.data(), c);
                if (ok && id != 3) { fprintf(stderr, "cut at %zu (section %u) parsed\n", c, id); return 1; }      // a cut inside the wire-to-label map loses nothing the reader needs
                ok ? parsed++ : refused++;
            }
            p += 12 + (size_t)sz;
        }
    }
    // seeded single-byte mutations: half of them in the first 256 bytes (magic, section table, header), the rest anywhere
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    std::unique_ptr<uint8_t[]> m(new uint8_t[img.size()]); memcpy(m.get(), img.data(), img.size());
    for (int k = 0; k < 3000; k++) {
        const size_t at = (k & 1) ? next() % 256 : next() % img.size();
        const uint8_t old = m[at]; uint8_t v = (uint8_t)next(); if (v == old) v ^= 0x80;
        m[at] = v;
        run_exact(m.get(), img.size()) ? parsed++ : refused++;
        m[at] = old;
    }
    printf("r1cs reader: ok (%zu refused, %zu parsed within bounds, checksum %llu)\n", refused, parsed, (unsigned long long)g_sum);
    return 0;
}
