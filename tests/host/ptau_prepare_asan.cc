// ptau_prepare_asan.cc -- the host side of `powersoftau prepare phase2` under AddressSanitizer + UBSan, as a plain program: the open-unprepared path of the reader
// (csrc/zkc_ptau_parse.h, ptau_open with need_prepared = false) and the writer's section copy and block offsets (csrc/zkc_ptau_write.h).
// Arguments: an unprepared power-3 file written by the test, and a directory that holds sec12.bin .. sec15.bin (the bodies the test expects) and takes the outputs.
// A file that opens is read section by section into heap blocks of exactly the section's size and written out again with four Lagrange sections whose blocks are placed
// by the writer's own offsets into blocks of exactly the section's size, so a length or an offset taken on trust shows as an access past a block; the output must open
// as a prepared file.  Inputs: the file itself (its output, with the test's bodies, stays as out.ptau for the test to compare), every prefix of its first 2 KB, cuts at
// every section boundary, and 4000 seeded single-byte changes of the file header, the section table and section 1.  Built and run by tests/test_ptau_prepare_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_ptau_write.h"

using namespace zkc::parse;

static uint64_t g_sum = 0;
static std::vector<uint8_t> read_all(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(1); }
    std::vector<uint8_t> b; uint8_t buf[4096]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f); return b;
}
static void write_file(const std::string& path, const uint8_t* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb"); if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "short write\n"); exit(1); }
    fclose(f);
}
static bool exists(const std::string& path) { struct stat st; return stat(path.c_str(), &st) == 0; }

// 1: opened, read, written and read back; 0: refused with a text.  bodies: directory of sec%d.bin to write instead of a pattern (NULL: a pattern)
static int run(const std::string& in, const std::string& out, const std::string* bodies) {
    Ptau p; std::string err;
    if (!ptau_open(in.c_str(), p, err, false)) { if (err.empty()) { fprintf(stderr, "refused without a text\n"); abort(); } return 0; }
    if (p.power == 0 || p.power > PTAU_MAX_POWER || p.end > p.size || p.end < 12) { fprintf(stderr, "power or end out of range after a successful open\n"); abort(); }
    if (p.power > 4) return 1;                                                    // cannot happen with files of this size: their lengths would not match
    for (int id : {2, 3, 4, 5, 6}) {
        const uint64_t n = ptau_section_points(id, p.power); std::string why;
        std::unique_ptr<uint8_t[]> d(new uint8_t[n * ptau_point_bytes(id)]);
        if (!ptau_read(p, id, 0, n, d.get(), why)) { fprintf(stderr, "section refused: %s\n", why.c_str()); abort(); }
        for (uint64_t i = 0; i < n * ptau_point_bytes(id); i++) g_sum += d[i];
        uint8_t one[128];
        if (ptau_read(p, id, n, 1, one, why) || ptau_read(p, id, 1, n, one, why)) { fprintf(stderr, "a range beyond its section was read\n"); abort(); }
    }
    remove(out.c_str());                                                          // a previous input's
    bool prepared = false;
    for (int id = 12; id <= 15; id++) prepared |= p.have[id];
    std::string abandoned, abandoned2;
    {   // an output that is not committed leaves nothing behind
        PtauOut o;
        if (!ptau_out_begin(p, out.c_str(), o, err)) { fprintf(stderr, "begin refused: %s\n", err.c_str()); abort(); }
        if (!exists(o.tmp) || exists(out)) { fprintf(stderr, "the temporary file is not where it should be\n"); abort(); }
        abandoned = o.tmp;
        PtauOut o2;                                                               // a second writer to the same path at the same time has a name of its own
        if (!ptau_out_begin(p, out.c_str(), o2, err) || o2.tmp == o.tmp || !exists(o2.tmp)) { fprintf(stderr, "two writers share a temporary file\n"); abort(); }
        abandoned2 = o2.tmp;
    }
    if (exists(out) || exists(abandoned) || exists(abandoned2)) { fprintf(stderr, "an abandoned output left a file\n"); abort(); }
    PtauOut o;
    if (!ptau_out_begin(p, out.c_str(), o, err)) { fprintf(stderr, "begin refused: %s\n", err.c_str()); abort(); }
    for (int sec = 12; sec <= 15; sec++) {
        const size_t w = ptau_point_bytes(sec), total = (size_t)ptau_section_points(sec, p.power) * w;
        std::unique_ptr<uint8_t[]> body(new uint8_t[total]);
        if (ptau_monomial_of(sec) != sec - 10) abort();
        const uint32_t last = ptau_last_block(sec, p.power);
        uint64_t end = 0;
        for (uint32_t b = 0; b <= last; b++) {
            const uint64_t first = ptau_block_first(b), n = 1ull << b;
            if (first != end) { fprintf(stderr, "block %u of section %d does not start where block %u ends\n", b, sec, b - 1); abort(); }
            for (uint64_t i = 0; i < n * w; i++) body[first * w + i] = (uint8_t)(sec * 29 + b * 7 + i);
            end = first + n;
        }
        if (end * w != total) { fprintf(stderr, "the blocks of section %d do not fill it\n", sec); abort(); }
        if (bodies) {
            const std::vector<uint8_t> given = read_all(*bodies + "/sec" + std::to_string(sec) + ".bin");
            if (given.size() != total) { fprintf(stderr, "sec%d.bin has %zu bytes, the section %zu\n", sec, given.size(), total); abort(); }
            memcpy(body.get(), given.data(), total);
        }
        if (!ptau_out_section(o, sec, body.get(), total, err)) { fprintf(stderr, "section refused: %s\n", err.c_str()); abort(); }
    }
    if (!ptau_out_commit(o, err) || !exists(out)) { fprintf(stderr, "commit failed: %s\n", err.c_str()); abort(); }
    if (!prepared) {                                                              // the output opens as a prepared file with four more sections
        Ptau q; std::string e;
        if (!ptau_open(out.c_str(), q, e) || q.nsections != p.nsections + 4 || q.power != p.power || q.end != q.size) { fprintf(stderr, "the output does not open: %s\n", e.c_str()); abort(); }
        std::unique_ptr<uint8_t[]> d(new uint8_t[(size_t)(2ull << q.power) * 64]);
        if (!ptau_read_lagrange(q, 12, q.power + 1, d.get(), e)) { fprintf(stderr, "top block refused: %s\n", e.c_str()); abort(); }
        g_sum += d[0];
    }
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: ptau_prepare_asan <unprepared.ptau> <dir>\n"); return 2; }
    const std::string dir = argv[2], path = dir + "/t.ptau", scratch = dir + "/t_out.ptau", keep = dir + "/out.ptau";
    const std::vector<uint8_t> img = read_all(argv[1]);
    if (run(argv[1], keep, &dir) != 1) { fprintf(stderr, "the valid file was refused\n"); return 1; }
    { Ptau p; std::string e; if (!ptau_open(argv[1], p, e, false) || p.power != 3 || p.nsections != 7 || p.end != img.size()) { fprintf(stderr, "the valid file was misread\n"); return 1; }
      if (ptau_open(argv[1], p, e) || e.find("no section 12") == std::string::npos) { fprintf(stderr, "an unprepared file opened as prepared\n"); return 1; } }
    { Ptau p; std::string e; PtauOut o; if (!ptau_open(argv[1], p, e, false)) return 1;
      if (ptau_out_begin(p, (dir + "/no_such_dir/x.ptau").c_str(), o, e) || e.find("cannot write") == std::string::npos) { fprintf(stderr, "an unwritable path was taken\n"); return 1; } }
    size_t refused = 0, opened = 0;
    // every prefix of the first 2 KB, and cuts at (and one byte around) every section boundary
    std::vector<size_t> cuts, framing;
    for (size_t n = 0; n < img.size() && n < 2048; n++) cuts.push_back(n);
    for (size_t i = 0; i < 12; i++) framing.push_back(i);
    for (size_t at = 12; at + 12 <= img.size();) {
        uint32_t id; uint64_t len; memcpy(&id, &img[at], 4); memcpy(&len, &img[at + 4], 8);
        for (size_t i = 0; i < 12; i++) framing.push_back(at + i);
        if (id == 1) for (size_t i = 0; i < len; i++) framing.push_back(at + 12 + i);
        for (size_t c : {at - 1, at, at + 1, at + 11, at + 12, at + 13}) if (c < img.size()) cuts.push_back(c);
        at += 12 + (size_t)len;
    }
    cuts.push_back(img.size() - 1);
    for (size_t n : cuts) { write_file(path, img.data(), n); if (run(path, scratch, nullptr)) { fprintf(stderr, "a prefix of %zu bytes opened\n", n); return 1; } refused++; }
    // seeded single-byte changes of the framing
    std::vector<uint8_t> m = img; uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int it = 0; it < 4000; it++) {
        const size_t at = framing[next() % framing.size()]; const uint8_t old = m[at];
        m[at] = (uint8_t)next();
        write_file(path, m.data(), m.size());
        run(path, scratch, nullptr) ? opened++ : refused++;
        m[at] = old;
    }
    remove(path.c_str()); remove(scratch.c_str());
    printf("ptau prepare io: ok (%zu refused, %zu opened within bounds, checksum %llu)\n", refused, opened, (unsigned long long)g_sum);
    return 0;
}
