// ptau_parse_asan.cc -- the host-only reader of a prepared powers-of-tau file (csrc/zkc_ptau_parse.h) under AddressSanitizer + UBSan, as a plain program.
// Argument: a directory to write its files into.  It builds a tiny valid file (power 1; the reader never looks inside a point, so the points are a byte pattern),
// opens it and reads every range a circuit can ask for into heap blocks of exactly the range's size; then every prefix of the file (each must be refused, with a
// text), every single-bit flip of the file header, of every section-table entry and of section 1, and the same file with its sections in another order.  A file that
// still opens after a flip is read in full the same way, so a length the reader took on trust shows as a read past a block.  Built and run by tests/test_ptau_setup_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_ptau_parse.h"

using namespace zkc::parse;

static uint64_t g_sum = 0;
static void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { uint8_t b[8]; memcpy(b, &v, 8); o.insert(o.end(), b, b + 8); }

struct Built { std::vector<uint8_t> img; std::vector<size_t> framing; };           // framing: offsets of the bytes whose every bit is flipped
static Built build(uint32_t power, const std::vector<int>& order) {
    Built b; std::vector<uint8_t>& o = b.img;
    o = {'p', 't', 'a', 'u'}; put32(o, 1); put32(o, (uint32_t)order.size());
    for (size_t i = 0; i < 12; i++) b.framing.push_back(i);
    for (int id : order) {
        for (size_t i = 0; i < 12; i++) b.framing.push_back(o.size() + i);
        put32(o, (uint32_t)id);
        if (id == 1) {
            put64(o, 44);
            for (size_t i = 0; i < 44; i++) b.framing.push_back(o.size() + i);
            put32(o, 32); o.insert(o.end(), (const uint8_t*)kFqP, (const uint8_t*)kFqP + 32); put32(o, power); put32(o, power);
        } else if (id == 7) { put64(o, 4); put32(o, 0); }
        else {
            const uint64_t n = ptau_section_points(id, power) * ptau_point_bytes(id);
            put64(o, n);
            for (uint64_t i = 0; i < n; i++) o.push_back((uint8_t)(id * 37 + i * 11));
        }
    }
    return b;
}
static void write_file(const std::string& path, const uint8_t* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb"); if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "short write\n"); exit(1); }
    fclose(f);
}
// 1: opened (and every range read inside exactly-sized blocks), 0: refused with a text
static int run(const std::string& path) {
    Ptau p; std::string err;
    if (!ptau_open(path.c_str(), p, err)) { if (err.empty()) { fprintf(stderr, "refused without a text\n"); abort(); } return 0; }
    if (p.power == 0 || p.power > PTAU_MAX_POWER) { fprintf(stderr, "power out of range after a successful open\n"); abort(); }
    if (p.power > 4) return 1;                                                    // cannot happen with files of this size: their lengths would not match
    for (uint32_t logn = 0; logn <= p.power + 1; logn++) {
        std::string why;
        if (ptau_fits(p, logn, why) != (logn <= p.power)) { fprintf(stderr, "ptau_fits wrong at %u\n", logn); abort(); }
        for (int id : {12, 13, 14, 15}) {
            if (logn == p.power + 1 && id != 12) continue;
            const size_t n = ((size_t)1 << logn) * ptau_point_bytes(id);
            std::unique_ptr<uint8_t[]> d(new uint8_t[n]);
            if (!ptau_read_lagrange(p, id, logn, d.get(), why)) { fprintf(stderr, "range refused: %s\n", why.c_str()); abort(); }
            for (size_t i = 0; i < n; i++) g_sum += d[i];
        }
    }
    for (int id : {4, 5, 6}) { std::string why; std::unique_ptr<uint8_t[]> d(new uint8_t[ptau_point_bytes(id)]); if (!ptau_read(p, id, 0, 1, d.get(), why)) abort(); g_sum += d[0]; }
    // ranges that reach beyond their section are refused, not read
    { std::string why; uint8_t one[128];
      if (ptau_read(p, 12, ptau_section_points(12, p.power), 1, one, why) || ptau_read(p, 13, 0, ~0ull, one, why) || ptau_read(p, 6, 1, 1, one, why) || ptau_read(p, 8, 0, 1, one, why) ||
          ptau_read_lagrange(p, 13, p.power + 1, one, why)) { fprintf(stderr, "a range beyond its section was read\n"); abort(); } }
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: ptau_parse_asan <dir>\n"); return 2; }
    const std::string path = std::string(argv[1]) + "/t.ptau";
    const std::vector<int> natural = {1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15}, shuffled = {15, 7, 12, 2, 1, 13, 6, 3, 14, 5, 4};
    size_t refused = 0, opened = 0;
    for (const std::vector<int>& order : {natural, shuffled}) {
        const Built b = build(1, order);
        write_file(path, b.img.data(), b.img.size());
        if (run(path) != 1) { fprintf(stderr, "valid file refused\n"); return 1; }
        { Ptau p; std::string e; if (!ptau_open(path.c_str(), p, e) || p.power != 1 || p.ceremonyPower != 1 || p.len[12] != 7 * 64 || p.len[13] != 3 * 128) { fprintf(stderr, "valid file misread\n"); return 1; } }
        for (size_t n = 0; n < b.img.size(); n++) { write_file(path, b.img.data(), n); if (run(path)) { fprintf(stderr, "prefix of %zu bytes opened\n", n); return 1; } refused++; }
        std::vector<uint8_t> m = b.img;
        for (size_t at : b.framing) for (int bit = 0; bit < 8; bit++) { m[at] ^= (uint8_t)(1 << bit); write_file(path, m.data(), m.size()); run(path) ? opened++ : refused++; m[at] ^= (uint8_t)(1 << bit); }
    }
    // a file of power 2 reads too, and one whose table claims 2^32 - 1 sections is refused without walking past the end
    { const Built b = build(2, natural); write_file(path, b.img.data(), b.img.size()); if (run(path) != 1) { fprintf(stderr, "power 2 refused\n"); return 1; }
      std::vector<uint8_t> m = b.img; memset(m.data() + 8, 0xff, 4); write_file(path, m.data(), m.size()); if (run(path)) { fprintf(stderr, "an endless table opened\n"); return 1; } }
    remove(path.c_str());
    printf("ptau reader: ok (%zu refused, %zu opened within bounds, checksum %llu)\n", refused, opened, (unsigned long long)g_sum);
    return 0;
}
