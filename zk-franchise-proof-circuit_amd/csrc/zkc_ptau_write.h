// zkc_ptau_write.h -- the host-only writer of a prepared powers-of-tau file (product code): the output side of `snarkjs powersoftau prepare phase2`
// (zkc_ptau_prepare.hip), next to the reader zkc_ptau_parse.h and in its manner: plain C++17 and POSIX, no HIP, compiled into libzkcensus.so by hipcc and, with
// -fsanitize=address,undefined, into tests/host/ptau_prepare_asan.cc.
//
// The output is the input's header with four more sections counted, the input's sections [12, end) copied as they lie in the file (ids, lengths, order; section 7 and
// anything unknown are copied unread, in 1 MiB pieces), and then sections 12, 13, 14, 15.  It is written under a temporary name next to out_path (pid and a per-call serial), synced and renamed into place
// by ptau_out_commit; a PtauOut that goes out of scope uncommitted removes the temporary file, so a failure leaves nothing at out_path.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <vector>
#include "zkc_ptau_parse.h"

namespace zkc { namespace parse {

// the blocks of a Lagrange section of a file of this power: p = 0 .. ptau_last_block, block p = 2^p points at point offset 2^p - 1
inline uint32_t ptau_last_block(int section, uint32_t power) { return section == 12 ? power + 1 : power; }
inline uint64_t ptau_block_first(uint32_t p) { return (1ull << p) - 1; }
// the monomial section a Lagrange section is the transform of
inline int ptau_monomial_of(int section) { return section - 10; }

struct PtauOut {
    int fd = -1; std::string tmp, path; bool committed = false;
    PtauOut() = default; PtauOut(const PtauOut&) = delete; PtauOut& operator=(const PtauOut&) = delete;
    ~PtauOut() { if (fd >= 0) close(fd); if (!committed && !tmp.empty()) unlink(tmp.c_str()); }
};
inline bool ptau_out_bytes(PtauOut& o, const void* src, size_t n, std::string& err) {
    const uint8_t* s = (const uint8_t*)src;
    while (n) { const ssize_t k = write(o.fd, s, n); if (k <= 0) { err = "ptau: cannot write " + o.path; return false; } s += k; n -= (size_t)k; }
    return true;
}
// the temporary file and the file header of nsec sections (zkc_ptau_prepare.hip through ptau_out_begin; zkc_scale_each.hip, whose outputs take no section as it lies)
inline bool ptau_out_open(const char* out_path, uint32_t nsec, PtauOut& o, std::string& err) {
    if (!out_path) { err = "ptau: no output path"; return false; }
    static std::atomic<unsigned> serial{0};                     // two threads of one process writing to one out_path get two names
    o.path = out_path; o.tmp = o.path + ".tmp" + std::to_string((long)getpid()) + "." + std::to_string(serial.fetch_add(1));
    o.fd = open(o.tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0644);
    if (o.fd < 0) { o.tmp.clear(); err = "ptau: cannot write " + o.path; return false; }
    uint8_t h[12]; memcpy(h, "ptau", 4);
    const uint32_t ver = 1; memcpy(h + 4, &ver, 4); memcpy(h + 8, &nsec, 4);
    return ptau_out_bytes(o, h, 12, err);
}
// the head of a section whose body follows in pieces (ptau_out_bytes)
inline bool ptau_out_section_head(PtauOut& o, int id, uint64_t nbytes, std::string& err) {
    uint8_t h[12]; const uint32_t i = (uint32_t)id; memcpy(h, &i, 4); memcpy(h + 4, &nbytes, 8);
    return ptau_out_bytes(o, h, 12, err);
}
// the header and the input's sections
inline bool ptau_out_begin(const Ptau& in, const char* out_path, PtauOut& o, std::string& err) {
    if (!out_path) { err = "ptau: no output path"; return false; }
    if (in.nsections > 0xffffffffu - 4) { err = "ptau: too many sections"; return false; }
    if (!ptau_out_open(out_path, in.nsections + 4, o, err)) return false;
    std::vector<uint8_t> buf(1u << 20);
    for (uint64_t at = 12; at < in.end;) {                      // in.end <= the file's size: ptau_open has walked the table
        const size_t n = (size_t)std::min<uint64_t>(buf.size(), in.end - at);
        if (!ptau_pread(in, buf.data(), n, at)) { err = "ptau: short read while copying the input's sections"; return false; }
        if (!ptau_out_bytes(o, buf.data(), n, err)) return false;
        at += n;
    }
    return true;
}
// one new section whole: id, length, body (nbytes = ptau_section_points x ptau_point_bytes: the caller's buffer is that long)
inline bool ptau_out_section(PtauOut& o, int id, const void* body, uint64_t nbytes, std::string& err) {
    uint8_t h[12]; const uint32_t i = (uint32_t)id; memcpy(h, &i, 4); memcpy(h + 4, &nbytes, 8);
    return ptau_out_bytes(o, h, 12, err) && ptau_out_bytes(o, body, (size_t)nbytes, err);
}
inline bool ptau_out_commit(PtauOut& o, std::string& err) {
    const int rs = fsync(o.fd), rc = close(o.fd); o.fd = -1;   // on disk before the name changes
    if (rs != 0 || rc != 0 || rename(o.tmp.c_str(), o.path.c_str()) != 0) { err = "ptau: cannot write " + o.path; return false; }
    o.committed = true;
    return true;
}

}}  // namespace zkc::parse
