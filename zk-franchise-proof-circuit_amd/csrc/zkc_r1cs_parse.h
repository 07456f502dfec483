// zkc_r1cs_parse.h -- the host-only reader of iden3 .r1cs images (product code): what `circom --r1cs` writes (circuit/circuit-compiler.sh:91) and r1cs.py restates.
//
// Plain C++17, no HIP, in the manner of zkc_hostparse.h: compiled into libzkcensus.so by hipcc (zkc_setup.hip generates keys from it, zkc_r1cs.hip keeps the three
// matrices on the device) and, with -fsanitize=address,undefined, into tests/host/r1cs_parse_asan.cc.  Every read is preceded by a bounds check that cannot wrap, and
// nothing is allocated in proportion to a length the image merely claims: a constraint takes at least 12 bytes and a term 36, so the image's own size bounds both.
//
// Layout: "r1cs" version(u32) nSections(u32), then per section id(u32) size(u64) payload.  Section 1 (64 B): n8(u32) prime(n8 B) nWires nPubOut nPubIn nPrvIn(u32 each)
// nLabels(u64) nConstraints(u32).  Section 2: per constraint its A, B and C linear combinations, each nTerms(u32) then nTerms x (wire(u32) coefficient(32 B, little
// endian, standard form)).  Sections may come in any order; ids other than 1 and 2 (the wire-to-label map, custom gates) are skipped; of a repeated id the last stands.
// An image cut inside a section is read as far as it goes: the constraint walk says where it ends.
//
// What the reader does NOT normalise, because neither consumer needs it to:
//  - a wire that occurs twice in one linear combination stays two terms; both consumers sum over terms, so it contributes the sum of its coefficients;
//  - a coefficient >= r is not refused.  The terms point at the image's 32 bytes as they are, and both consumers take them through fp_from_std, a Montgomery product
//    by R^2 that is defined for any 256-bit operand and returns the canonical residue: such a coefficient MEANS its value mod r (as ffjavascript reads it).
#pragma once
#include "zkc_hostparse.h"

namespace zkc { namespace parse {

struct R1csHeader { uint32_t nWires, nPubOut, nPubIn, nPub, nCons; };
struct R1csTerm { uint32_t wire; const uint8_t* coef; };              // coef: 32 bytes inside the image (unaligned)
// constraint k's terms of matrix m (0 = A, 1 = B, 2 = C) are terms[m][ptr[m][k] .. ptr[m][k + 1]), in file order
struct R1cs { R1csHeader h; std::vector<uint64_t> ptr[3]; std::vector<R1csTerm> terms[3]; };

// magic, section table, header size, field size 32, prime = BN254 r, nPub < nWires.  *s2 / *s2sz: the constraint section, as much of it as the image holds.
inline bool r1cs_header(const uint8_t* buf, size_t len, R1csHeader& h, const uint8_t** s2_out, uint64_t* s2sz_out, std::string& err) {
    if (!buf || len < 12 || memcmp(buf, "r1cs", 4) != 0) { err = "not an r1cs file"; return false; }
    const uint32_t nsec = rd32(buf + 8); size_t p = 12; const uint8_t *s1 = nullptr, *s2 = nullptr; uint64_t s2sz = 0;
    for (uint32_t i = 0; i < nsec; i++) {
        if (len - p < 12) { err = "r1cs sections truncated"; return false; }                       // no wrap: p <= len
        const uint32_t id = rd32(buf + p); const uint64_t n = rd64(buf + p + 4); p += 12;
        const uint64_t have = std::min<uint64_t>(n, len - p);
        if (id == 1) { if (have < 64) { err = "bad r1cs header"; return false; } s1 = buf + p; }
        if (id == 2) { s2 = buf + p; s2sz = have; }
        if (have < n) break;
        p += (size_t)n;
    }
    if (!s1 || !s2 || rd32(s1) != 32) { err = "bad r1cs header"; return false; }
    for (int i = 0; i < 8; i++) if (rd32(s1 + 4 + 4 * i) != kFrP[i]) { err = "r1cs prime is not BN254 r"; return false; }
    h.nWires = rd32(s1 + 36); h.nPubOut = rd32(s1 + 40); h.nPubIn = rd32(s1 + 44); h.nCons = rd32(s1 + 60);
    h.nPub = h.nPubOut + h.nPubIn;
    if (h.nPub >= h.nWires) { err = "bad r1cs header"; return false; }
    if (s2_out) *s2_out = s2;
    if (s2sz_out) *s2sz_out = s2sz;
    return true;
}

// the whole image -> the three coefficient lists; on top of r1cs_header: truncated constraints, wire index out of range
inline bool r1cs_parse(const uint8_t* buf, size_t len, R1cs& out, std::string& err) {
    const uint8_t* q = nullptr; uint64_t s2sz = 0;
    if (!r1cs_header(buf, len, out.h, &q, &s2sz, err)) return false;
    const uint32_t nCons = out.h.nCons, nWires = out.h.nWires;
    if ((uint64_t)nCons * 12 > s2sz) { err = "r1cs constraints truncated"; return false; }        // three counts per constraint: the walk below would run out
    const uint8_t* const end = q + s2sz;
    for (int m = 0; m < 3; m++) { out.ptr[m].assign((size_t)nCons + 1, 0); out.terms[m].clear(); out.terms[m].reserve((size_t)(s2sz / 36 / 2)); }
    for (uint32_t k = 0; k < nCons; k++) {
        for (int m = 0; m < 3; m++) {
            if (end - q < 4) { err = "r1cs constraints truncated"; return false; }
            const uint32_t n = rd32(q); q += 4;
            if ((uint64_t)n * 36 > (uint64_t)(end - q)) { err = "r1cs constraints truncated"; return false; }
            for (uint32_t t = 0; t < n; t++, q += 36) {
                const uint32_t wire = rd32(q);
                if (wire >= nWires) { err = "r1cs wire index out of range"; return false; }
                out.terms[m].push_back(R1csTerm{wire, q + 4});
            }
            out.ptr[m][(size_t)k + 1] = out.terms[m].size();
        }
    }
    return true;
}

}}  // namespace zkc::parse
