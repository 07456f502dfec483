// zkc_ptau_parse.h -- the host-only reader of a powers-of-tau file, `.ptau` (product code): what `snarkjs powersoftau prepare phase2` reads (circuit/circuit-compiler.sh:71;
// ptau_open with need_prepared = false) and what it leaves and `snarkjs groth16 setup` reads (circuit/circuit-compiler.sh:99-108).
//
// Plain C++17 and POSIX pread, no HIP, in the manner of zkc_phase2_parse.h: compiled into libzkcensus.so by hipcc (zkc_setup_ptau.hip) and, with
// -fsanitize=address,undefined, into tests/host/ptau_parse_asan.cc and tests/host/ptau_prepare_asan.cc.  A public file is hundreds of GB (power 28), so nothing here reads a section: ptau_open walks the
// section table, 12 bytes per section at 64-bit offsets, and reads section 1; ptau_read fetches a range of points of one section into the caller's buffer.  Every
// offset is checked against the file's size before it is used, in arithmetic that cannot wrap (power <= 28 bounds every product below 2^37), every failure has its
// own text, and nothing is allocated in proportion to a number the file merely claims.
//
// Layout (the iden3 binfile container and snarkjs' powersoftau sections, restated from the format's description: DESIGN.md section 7 says what has not been run against a
// snarkjs-written file):
//   "ptau" version(u32 = 1) nSections(u32), then per section id(u32) length(u64) body
//   1  n8(u32 = 32) q(32 B little endian) power(u32) ceremonyPower(u32)
//   2  tauG1        2^(power+1) - 1 points     tau^i G1
//   3  tauG2        2^power points             tau^i G2
//   4  alphaTauG1   2^power points             alpha tau^i G1
//   5  betaTauG1    2^power points             beta tau^i G1
//   6  betaG2       1 point
//   7  contributions (not read here)
//   12 .. 15  the same four families in Lagrange form (a *prepared* file): for p = 0 .. power the basis of the size-2^p domain, 2^p points at point offset 2^p - 1;
//             section 12 holds the p = power + 1 block as well.  12 tauG1: 2^(power+2) - 1 points; 13 tauG2, 14 alphaTauG1, 15 betaTauG1: 2^(power+1) - 1 points.
// Points are uncompressed affine with little-endian Montgomery coordinates, as in a .zkey: G1 64 B (x y), G2 128 B (x.c0 x.c1 y.c0 y.c1); all zero = infinity.
// Sections may come in any order; of a repeated id the first stands; ids above 15 are skipped.  Whether a point is on its curve is the generator's question.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "zkc_hostparse.h"

namespace zkc { namespace parse {

constexpr uint32_t PTAU_MAX_POWER = 28;
// Fr has no root of unity of order above 2^28, and preparing a file of power p transforms at size 2^(p+1) (section 12's last block): `prepare phase2` and the check of a
// prepared file stop one power below what the reader takes
constexpr uint32_t PTAU_MAX_PREPARE_POWER = 27;
struct Ptau {
    int fd = -1; uint64_t size = 0;
    uint32_t power = 0, ceremonyPower = 0;
    uint64_t off[16] = {0}, len[16] = {0}; bool have[16] = {false};
    uint32_t nsections = 0; uint64_t end = 12;      // the table's count, and where its last section ends: [12, end) is every section as it lies in the file
    Ptau() = default; Ptau(const Ptau&) = delete; Ptau& operator=(const Ptau&) = delete;
    ~Ptau() { if (fd >= 0) close(fd); }
};

// exactly n bytes at offset `at` (inside the file: the caller has checked), through short reads
inline bool ptau_pread(const Ptau& p, void* dst, size_t n, uint64_t at) {
    uint8_t* d = (uint8_t*)dst;
    while (n) { const ssize_t k = pread(p.fd, d, n, (off_t)at); if (k <= 0) return false; d += k; n -= (size_t)k; at += (uint64_t)k; }
    return true;
}
inline uint32_t ptau_point_bytes(int section) { return section == 3 || section == 13 || section == 6 ? 128u : 64u; }
// the points a section must hold for this power (sections 2..6 and 12..15)
inline uint64_t ptau_section_points(int section, uint32_t power) {
    const uint64_t n = 1ull << power;
    switch (section) {
        case 2: return 2 * n - 1; case 3: case 4: case 5: return n; case 6: return 1;
        case 12: return 4 * n - 1; case 13: case 14: case 15: return 2 * n - 1; default: return 0;
    }
}

// need_prepared = false: sections 12 .. 15 are not asked for (the input of `prepare phase2`, zkc_ptau_prepare.hip); which of them the file has is in p.have.
// max_power < PTAU_MAX_POWER: a file of a power above it is refused with a text of its own, before its section lengths are looked at (zkc_ptau_prepare.hip: 27)
inline bool ptau_open(const char* path, Ptau& p, std::string& err, bool need_prepared = true, uint32_t max_power = PTAU_MAX_POWER) {
    if (!path) { err = "ptau: no path"; return false; }
    p.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (p.fd < 0) { err = std::string("ptau: cannot open ") + path; return false; }
    struct stat st;
    if (fstat(p.fd, &st) != 0 || st.st_size < 0) { err = "ptau: cannot stat the file"; return false; }
    p.size = (uint64_t)st.st_size;
    uint8_t h[12];
    if (p.size < 12 || !ptau_pread(p, h, 12, 0)) { err = "ptau: shorter than a file header"; return false; }
    if (memcmp(h, "ptau", 4) != 0) { err = "ptau: bad magic (not a powers-of-tau file)"; return false; }
    if (rd32(h + 4) != 1) { err = "ptau: unsupported version " + std::to_string(rd32(h + 4)); return false; }
    const uint32_t nsec = rd32(h + 8);
    uint64_t at = 12;
    for (uint32_t i = 0; i < nsec; i++) {
        uint8_t s[12];
        if (p.size - at < 12 || !ptau_pread(p, s, 12, at)) { err = "ptau: the section table runs past the file (entry " + std::to_string(i) + ")"; return false; }       // no wrap: at <= size
        const uint32_t id = rd32(s); const uint64_t n = rd64(s + 4); at += 12;
        if (n > p.size - at) { err = "ptau: the section table runs past the file (section " + std::to_string(id) + ")"; return false; }
        if (id < 16 && !p.have[id]) { p.have[id] = true; p.off[id] = at; p.len[id] = n; }
        at += n;
    }
    p.nsections = nsec; p.end = at;
    if (!p.have[1]) { err = "ptau: no section 1 (header)"; return false; }
    if (p.len[1] != 44) { err = "ptau: section 1 is not 44 bytes"; return false; }
    uint8_t s1[44];
    if (!ptau_pread(p, s1, 44, p.off[1])) { err = "ptau: cannot read section 1"; return false; }
    if (rd32(s1) != 32) { err = "ptau: n8 is not 32"; return false; }
    if (memcmp(s1 + 4, kFqP, 32) != 0) { err = "ptau: q is not BN254's"; return false; }
    p.power = rd32(s1 + 36); p.ceremonyPower = rd32(s1 + 40);
    if (p.power == 0 || p.power > PTAU_MAX_POWER) { err = "ptau: power " + std::to_string(p.power) + " outside [1, 28]"; return false; }
    if (p.power > max_power) {
        err = "ptau: power " + std::to_string(p.power) + " cannot be prepared or checked here: section 12's last block is a transform of size 2^" + std::to_string(p.power + 1) +
              ", and Fr has no root of unity of order above 2^28 (the largest power is " + std::to_string(max_power) + ")";
        return false;
    }
    for (int id : {2, 3, 4, 5, 6}) {
        if (!p.have[id]) { err = "ptau: no section " + std::to_string(id); return false; }
        if (p.len[id] != ptau_section_points(id, p.power) * ptau_point_bytes(id)) { err = "ptau: the length of section " + std::to_string(id) + " does not match power " + std::to_string(p.power); return false; }
    }
    if (!need_prepared) return true;
    if (!p.have[12]) { err = "ptau: no section 12: run `powersoftau prepare phase2`"; return false; }
    for (int id : {12, 13, 14, 15}) {
        if (!p.have[id]) { err = "ptau: no section " + std::to_string(id) + ": the file is only partly prepared"; return false; }
        if (p.len[id] != ptau_section_points(id, p.power) * ptau_point_bytes(id)) { err = "ptau: the length of section " + std::to_string(id) + " does not match power " + std::to_string(p.power); return false; }
    }
    return true;
}

// can a circuit whose domain is 2^cirPower take its key from this file?  (section 12's p = power + 1 block is what lets cirPower == power work: H needs the size-2n basis)
inline bool ptau_fits(const Ptau& p, uint32_t cirPower, std::string& err) {
    if (cirPower > p.power) { err = "ptau: power " + std::to_string(p.power) + " is below the circuit's " + std::to_string(cirPower); return false; }
    return true;
}

// npoints points of `section` from point index `first` into dst (npoints x ptau_point_bytes(section) bytes)
inline bool ptau_read(const Ptau& p, int section, uint64_t first, uint64_t npoints, void* dst, std::string& err) {
    if (section < 2 || section > 15 || !p.have[section] || !ptau_section_points(section, p.power)) { err = "ptau: no section " + std::to_string(section); return false; }
    const uint64_t have = p.len[section] / ptau_point_bytes(section);
    if (first > have || npoints > have - first) { err = "ptau: points " + std::to_string(first) + " + " + std::to_string(npoints) + " reach beyond section " + std::to_string(section); return false; }
    if (!ptau_pread(p, dst, (size_t)(npoints * ptau_point_bytes(section)), p.off[section] + first * ptau_point_bytes(section))) { err = "ptau: short read in section " + std::to_string(section); return false; }
    return true;
}
// the Lagrange basis of the size-2^logn domain (logn <= power; section 12: logn <= power + 1)
inline bool ptau_read_lagrange(const Ptau& p, int section, uint32_t logn, void* dst, std::string& err) {
    return ptau_read(p, section, (1ull << logn) - 1, 1ull << logn, dst, err);
}

}}  // namespace zkc::parse
