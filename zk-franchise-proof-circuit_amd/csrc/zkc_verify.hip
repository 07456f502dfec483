// zkc_verify.hip -- a9: Groth16 verification on the CPU (constant work, no GPU), plus the JSON / .wtns codecs (a8) and the
// rapidsnark-shaped `groth16_prover` entry point (product host code).
//
// Mirrors go-rapidsnark/verifier VerifyGroth16 behind dvote's proof.Verify (zk_census_test.go:122) and snarkjs
// groth16.verify: vk_x = IC0 + sum s_i IC_{i+1};  e(-A, B) e(alpha, beta) e(vk_x, gamma) e(C, delta) == 1.
// The pairing lives in zkc_pairing.h (optimal ate, projective sparse lines, shared accumulator, prepared G2 points, cyclotomic final exponentiation).  The batch verifiers,
// which take a context and use the GPU, are zkc_verify_batch.hip; what they share with this file is declared in zkc_verify_host.h and defined here.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <random>
#include <algorithm>
#include "zkc_verify_host.h"
#include "zkc_hostparse.h"
#include <sys/random.h>
#include <cerrno>
#include <mutex>
#include <memory>
#include <array>

using namespace zkc;
using namespace zkc::pairing;
using parse::dec_of;

// e(P, Q) as snarkjs stores it in verification_key.json as vk_alphabeta_12 (artifacts/zkCensus/dev/160/verification_key.json:52): ffjavascript / wasmcurves follow
// libff's alt_bn128, whose final exponentiation ends in the Fuentes-Castaneda chunk and so yields the reduced pairing raised to 2x(6x^2 + 3x + 1) -- which is what
// pairing::final_exp returns.  Pinned by tests/test_oracle_pinning.py against the reference's own verification key (alpha, beta -> vk_alphabeta_12).
static Fq12 pairing_snarkjs(const G1Affine& P, const G2Affine& Q) { return final_exp(miller(P, Q)); }
static thread_local std::string g_err;

namespace zkc {
void fq12_to_std(const Fq12& e, uint8_t out[384]) {
    const Fq2* c[6] = {&e.a.a0, &e.a.a1, &e.a.a2, &e.b.a0, &e.b.a1, &e.b.a2};
    for (int i = 0; i < 6; i++) { wr_fq_std(out + 64 * i, c[i]->c0); wr_fq_std(out + 64 * i + 32, c[i]->c1); }
}
std::string& verify_error() { return g_err; }
int vfail(int code, const std::string& m) { g_err = m; return code; }
}  // namespace zkc

// the header of a key straight from the file image (no GPU, no load, no coefficient scan: that is the loader's)
static bool zkey_header(const void* zkey, size_t len, parse::ZkeyHeader& zh, std::string& why) {
    parse::BinSections bs;
    return parse::binfile_sections((const uint8_t*)zkey, len, "zkey", 1, bs, why) && parse::zkey_check(bs, zh, why, false);
}

extern "C" const char* zkc_verify_last_error(void) { return g_err.c_str(); }
// e(P, Q) as snarkjs / ffjavascript compute and print it: 12 x 32 B standard form, order c0.a0.(c0,c1) c0.a1 c0.a2 c1.a0 c1.a1 c1.a2
// (the nesting of vk_alphabeta_12 in verification_key.json).  Host only.
extern "C" int zkc_pairing_bin(const uint8_t g1[64], const uint8_t g2[128], uint8_t out[384]) {
    G1Affine P; G2Affine Q;
    if (!g1 || !g2 || !out || !rd_g1_std(P, g1) || !rd_g2_std(Q, g2) || !g1_on_curve(P) || !g2_on_curve(Q)) return ZKC_ERR_BAD_ARG;
    fq12_to_std(pairing_snarkjs(P, Q), out);
    return ZKC_OK;
}
extern "C" void zkc_sha256(const void* data, size_t len, uint8_t out[32]) { parse::sha256(data, len, out); }
extern "C" int zkc_zkey_sha256(const zkc_zkey* zk, uint8_t out[32]) { if (!zk || !out) return ZKC_ERR_BAD_ARG; memcpy(out, zk->sha256, 32); return ZKC_OK; }
extern "C" int zkc_zkey_fingerprint(const void* zkey_bytes, size_t len, uint8_t out[32]) {
    parse::BinSections bs; std::string perr;
    if (!zkey_bytes || !out || !parse::binfile_sections((const uint8_t*)zkey_bytes, len, "zkey", 1, bs, perr)) return ZKC_ERR_FORMAT;
    parse::zkey_fingerprint((const uint8_t*)zkey_bytes, len, bs, out);
    return ZKC_OK;
}
// The message of the Error snarkjs throws when the witness calculator hits an assert (witness_calculator.js exceptionHandler: "Assert Failed.\n" + the lines
// circom's runtime printed, innermost template first).  Pinned against the wasm's own output in tests/golden/witness_vectors.json.
extern "C" const char* zkc_witness_status_text(int nLevels, int32_t status) {
    struct Site { int32_t st; const char* frames[3][2]; };                        // {template, line}, innermost first
    static const Site sites[] = {
        {ZKC_W_ERR_WEIGHT,           {{"ZkFranchiseProofCircuit", "72"}}},
        {ZKC_W_ERR_SIK_LAST_SIBLING, {{"SMTLevIns", "93"}, {"SMTVerifier", "70"}, {"ZkFranchiseProofCircuit", "90"}}},
        {ZKC_W_ERR_SIK_ROOT,         {{"ForceEqualIfEnabled", "56"}, {"SMTVerifier", "134"}, {"ZkFranchiseProofCircuit", "90"}}},
        {ZKC_W_ERR_LAST_SIBLING,     {{"SMTLevIns", "93"}, {"SMTVerifier", "70"}, {"ZkFranchiseProofCircuit", "103"}}},
        {ZKC_W_ERR_CENSUS_ROOT,      {{"ForceEqualIfEnabled", "56"}, {"SMTVerifier", "134"}, {"ZkFranchiseProofCircuit", "103"}}},
        {ZKC_W_ERR_NULLIFIER,        {{"ForceEqualIfEnabled", "56"}, {"ZkFranchiseProofCircuit", "114"}}},
    };
    static const struct { const char* tmpl; const char* id; } ids160[] = {{"ForceEqualIfEnabled", "_159"}, {"SMTLevIns", "_80"}, {"SMTVerifier", "_160"}, {"ZkFranchiseProofCircuit", "_234"}};
    static const std::vector<std::string> text = [] {
        std::vector<std::string> t(2 * 8);
        for (int with_ids = 0; with_ids < 2; with_ids++) {
            for (const Site& s : sites) {
                std::string m = "Assert Failed.\n";
                for (const auto& f : s.frames) {
                    if (!f[0]) break;
                    m += std::string("Error in template ") + f[0];
                    if (with_ids) for (const auto& k : ids160) if (!strcmp(k.tmpl, f[0])) m += k.id;
                    m += std::string(" line: ") + f[1] + "\n";
                }
                t[with_ids * 8 + s.st] = m;
            }
            t[with_ids * 8 + ZKC_W_ERR_INPUT_RANGE] = "Input value is not below the field order r\n";
        }
        return t;
    }();
    if (status <= 0 || status >= 8) return nullptr;
    return text[(nLevels == 160 ? 8 : 0) + status].c_str();
}
// circuits this build has a native witness generator for, by the sha256 of their circom witness-calculator wasm
// the shape of a key straight from the file image (no GPU, no load): what a host needs to size its buffers before it submits a request
extern "C" int zkc_zkey_header_info(const void* zkey_bytes, size_t len, uint32_t* nVars, uint32_t* nPublic, uint32_t* domainSize) {
    parse::ZkeyHeader zh; std::string perr;
    if (!zkey_bytes || !zkey_header(zkey_bytes, len, zh, perr)) { g_err = perr; return ZKC_ERR_FORMAT; }
    if (nVars) *nVars = zh.nVars; if (nPublic) *nPublic = zh.nPub; if (domainSize) *domainSize = zh.n;
    return ZKC_OK;
}
extern "C" int zkc_circuit_nlevels_from_wasm(const void* wasm, size_t len, char sha256_hex[65]) {
    static const struct { const char* sha; int nLevels; } known[] = {
        {"80a73567f6a4655d4332301efcff4bc5711bb48176d1c71fdb1e48df222ac139", 160},      // artifacts/zkCensus/dev/circuits-info.md:7
    };
    if (!wasm) return -1;
    uint8_t d[32]; parse::sha256(wasm, len, d); const std::string hex = parse::hex_of(d, 32);
    if (sha256_hex) memcpy(sha256_hex, hex.c_str(), 65);
    for (const auto& k : known) if (hex == k.sha) return k.nLevels;
    return -1;
}

// the circuit a caller names by its witness-calculator image, per call and cheaply: the SHA-256 of a 3 MB wasm is ~2 ms, a proof's share of a GPU pass 0.3 ms, so the answer
// is remembered per (buffer, length) and re-checked against a sampled digest of the buffer (both ends and a 64-byte block of every 64 KB: a buffer re-used for another file
// is hashed again).  -1: unknown wasm
static int nlevels_of_wasm_cached(const void* wasm, size_t len) {
    struct Seen { const void* p; size_t len; uint8_t sample[32]; int nLevels; };
    static std::mutex mu; static std::vector<Seen> seen;
    uint8_t smp[32];
    { parse::Sha256 h; const uint8_t* b = (const uint8_t*)wasm; const uint64_t l64 = len; h.update(&l64, 8); const size_t edge = std::min<size_t>(len, 1024); h.update(b, edge); h.update(b + len - edge, edge);
      for (size_t off = 0; off + 64 <= len; off += 65536) h.update(b + off, 64); h.final(smp); }
    { std::lock_guard<std::mutex> g(mu); for (auto& e : seen) if (e.p == wasm && e.len == len && !memcmp(e.sample, smp, 32)) return e.nLevels; }
    const int nl = zkc_circuit_nlevels_from_wasm(wasm, len, nullptr);
    std::lock_guard<std::mutex> g(mu);
    if (seen.size() >= 16) seen.erase(seen.begin());
    Seen e; e.p = wasm; e.len = len; memcpy(e.sample, smp, 32); e.nLevels = nl; seen.push_back(e);
    return nl;
}
// nLevels of the call: from the wasm's hash when one is given (the reference's callers name the circuit that way: prover.Prove(zkey, wasm, inputs), zk_census_test.go:89),
// else from the key's own shape (wire count and 8 public signals).  < 0: err says why
static int nlevels_of_call(const void* zkey, size_t zkey_len, const void* wasm, size_t wasm_len, std::string& err) {
    if (wasm) {
        const int nl = nlevels_of_wasm_cached(wasm, wasm_len);
        if (nl < 0) err = "the witness calculator (wasm) is not one this build has a native circuit for; the C ABI has no wasm runtime (the N-API surface executes unknown circuits in Node): compute the witness elsewhere and call groth16_prover";
        return nl;
    }
    parse::ZkeyHeader zh;
    if (!zkey_header(zkey, zkey_len, zh, err)) return -1;
    if (zh.nPub == 8) for (int nl = 3; nl <= 253; nl++) if ((uint32_t)zkc_circuit_n_wires(nl) == zh.nVars) return nl;
    err = "no wasm given and the key is not a ZkFranchiseProofCircuit key"; return -1;
}
// inputs_example.json's text -> the flat input block (zkc_hostparse.h circuit_inputs_from_json: circom_runtime's reading and messages)
extern "C" int zkc_inputs_from_json(const char* json, size_t len, int nLevels, void* out, char* err, size_t errlen) {
    if (!json || !out || nLevels < 3 || nLevels > 253) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_inputs_from_json: bad argument");
    std::string why;
    const int rc = parse::circuit_inputs_from_json(json, len, nLevels, (uint8_t*)out, why);
    if (rc) return err_out(err, errlen, rc == 1 ? ZKC_ERR_FORMAT : ZKC_ERR_GENERIC, why);
    if (err && errlen) err[0] = 0;
    return ZKC_OK;
}
// prover.Prove(zkey, wasm, inputs) with the reference's three byte slices (zk_census_test.go:81-89), one voter, through the proving service: witness and proof on the GPU
extern "C" int zkc_service_fullprove_json(zkc_service* svc, const void* zkey, size_t zkey_len, const void* wasm, size_t wasm_len, const char* inputs_json, size_t inputs_len,
                                          const uint8_t* rs, uint8_t proof[256], uint8_t* publics, int32_t* status, char* err, size_t errlen) {
    if (status) *status = 0;
    if (!svc || !zkey || !inputs_json || !proof) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_service_fullprove_json: bad argument");
    std::string why;
    const int nl = nlevels_of_call(zkey, zkey_len, wasm, wasm_len, why);
    if (nl < 0) return err_out(err, errlen, ZKC_ERR_BAD_ARG, why);
    std::vector<uint8_t> flat(32 * (size_t)zkc_circuit_n_inputs(nl));
    const int rc = parse::circuit_inputs_from_json(inputs_json, inputs_len, nl, flat.data(), why);
    if (rc) return err_out(err, errlen, rc == 1 ? ZKC_ERR_FORMAT : ZKC_ERR_GENERIC, why);
    return zkc_service_fullprove(svc, zkey, zkey_len, nl, flat.data(), rs, proof, publics, status, err, errlen);
}
// What the two entry points of rapidsnark's shape (groth16_fullprove, groth16_prover) say about the caller's two buffers.  Before proving: is there room for ANY proof of
// this shape (77 decimal digits per coordinate)?  If not, the sizes needed are written back (they depend only on nPublic).  After proving: the two JSON texts into them.
static const char kShortJson[] = "Proof or public signals buffer is too short";
static bool proof_json_room(uint32_t nPub, const char* proof_buffer, unsigned long* proof_size, const char* public_buffer, unsigned long* public_size) {
    const unsigned long need_proof = 8 * 80 + 128, need_public = (unsigned long)nPub * 80 + 8;
    if (proof_buffer && public_buffer && *proof_size >= need_proof && *public_size >= need_public) return true;
    *proof_size = need_proof; *public_size = need_public;
    return false;
}
static int proof_json_out(const uint8_t proof[256], const uint8_t* pub, uint32_t nPub, char* proof_buffer, unsigned long* proof_size, char* public_buffer, unsigned long* public_size,
                          char* error_msg, unsigned long error_msg_maxsize) {
    const int rc = zkc_proof_to_json(proof, pub, (int)nPub, proof_buffer, proof_size, public_buffer, public_size);
    return rc == ZKC_ERR_SHORT_BUFFER ? err_out(error_msg, error_msg_maxsize, rc, kShortJson) : rc;
}
// ... and with rapidsnark's conventions for everything else (groth16_prover below): JSON texts out, 0 / 1 / 2, the process-wide service, random (r, s).  What a cgo
// prover.Prove calls instead of wasmer + groth16_prover.  A voter whose inputs fail a circuit assert: 1, error_msg = the wasm's message.
extern "C" int groth16_fullprove(const void* zkey_buffer, unsigned long zkey_size, const void* wasm_buffer, unsigned long wasm_size, const char* inputs_json, unsigned long inputs_size,
                                 char* proof_buffer, unsigned long* proof_size, char* public_buffer, unsigned long* public_size, char* error_msg, unsigned long error_msg_maxsize) {
    auto err = [&](int code, const std::string& m) { return err_out(error_msg, error_msg_maxsize, code, m); };
    if (!zkey_buffer || !inputs_json || !proof_size || !public_size) return err(ZKC_ERR_GENERIC, "groth16_fullprove: null argument");
    parse::ZkeyHeader zh; std::string perr;
    if (!zkey_header(zkey_buffer, zkey_size, zh, perr)) return err(ZKC_ERR_GENERIC, perr);
    if (!proof_json_room(zh.nPub, proof_buffer, proof_size, public_buffer, public_size)) return err(ZKC_ERR_SHORT_BUFFER, kShortJson);
    zkc_service* svc = zkc_service_default();
    if (!svc) return err(ZKC_ERR_GENERIC, zkc_service_last_error());
    uint8_t proof[256]; std::vector<uint8_t> pub(32 * (size_t)zh.nPub + 1); char etext[512] = {0}; int32_t st = 0;
    const int rc = zkc_service_fullprove_json(svc, zkey_buffer, zkey_size, wasm_buffer, wasm_size, inputs_json, inputs_size, nullptr, proof, pub.data(), &st, etext, sizeof etext);
    if (rc) return err(ZKC_ERR_GENERIC, etext);
    return proof_json_out(proof, pub.data(), zh.nPub, proof_buffer, proof_size, public_buffer, public_size, error_msg, error_msg_maxsize);
}

// ---- a verification key made ready once: points read and checked (on the curve, G2 points in the order-r subgroup), gamma and delta prepared into their line
// coefficients, the Miller value of (alpha, beta) computed.  A node verifies every ballot of an election under ONE key (zk_census_test.go:103-124 per vote), so the
// latest few keys are kept by their bytes; the three [r]Q checks and three preparations were a third of a verification. ----
static std::mutex g_vk_mu; static std::vector<std::shared_ptr<const VkReady>> g_vk_ready;      // most recent first, at most 8
std::shared_ptr<const VkReady> zkc::vk_ready(const uint8_t* vk, int nPublic, int* code) {
    const size_t len = 448 + 64 * ((size_t)nPublic + 1);
    {
        std::lock_guard<std::mutex> g(g_vk_mu);
        for (size_t i = 0; i < g_vk_ready.size(); i++)
            if (g_vk_ready[i]->bytes.size() == len && !memcmp(g_vk_ready[i]->bytes.data(), vk, len)) {
                auto hit = g_vk_ready[i];
                if (i) { g_vk_ready.erase(g_vk_ready.begin() + (long)i); g_vk_ready.insert(g_vk_ready.begin(), hit); }
                return hit;
            }
    }
    auto r = std::make_shared<VkReady>(); r->bytes.assign(vk, vk + len); r->nPublic = nPublic; r->ic.resize((size_t)nPublic + 1);
    if (!rd_g1_std(r->alpha, vk) || !rd_g2_std(r->beta, vk + 64) || !rd_g2_std(r->gamma, vk + 192) || !rd_g2_std(r->delta, vk + 320)) { *code = vfail(-ZKC_ERR_FORMAT, "verification key coordinate >= q"); return nullptr; }
    if (!g1_on_curve(r->alpha) || !g2_in_subgroup(r->beta) || !g2_in_subgroup(r->gamma) || !g2_in_subgroup(r->delta)) { *code = vfail(-ZKC_ERR_FORMAT, "verification key point not on the curve / not in the order-r subgroup"); return nullptr; }
    for (int j = 0; j <= nPublic; j++) if (!rd_g1_std(r->ic[j], vk + 448 + 64 * (size_t)j) || !g1_on_curve(r->ic[j])) { *code = vfail(-ZKC_ERR_FORMAT, "IC point invalid"); return nullptr; }
    r->pgamma = prepare_g2(r->gamma); r->pdelta = prepare_g2(r->delta); r->pbeta = prepare_g2(r->beta);
    const Pair ab{r->alpha, &r->pbeta}; r->m_alpha_beta = multi_miller(&ab, 1);
    if (nPublic <= 64) {
        r->ic_mult.resize(15 * (size_t)nPublic);
        for (int j = 0; j < nPublic; j++) {
            G1XYZZ m = G1XYZZ::from_affine(r->ic[j + 1]);
            for (int k = 0; k < 15; k++) { r->ic_mult[15 * (size_t)j + k] = xyzz_to_affine_gcd(m); m = xyzz_add_affine(m, r->ic[j + 1]); }
        }
    }
    std::lock_guard<std::mutex> g(g_vk_mu);
    g_vk_ready.insert(g_vk_ready.begin(), r); if (g_vk_ready.size() > 8) g_vk_ready.pop_back();
    return r;
}
G1XYZZ zkc::g1_sum_of_products(const G1Affine* pts, const uint32_t (*k)[8], int n) {
    int top = -1;
    for (int b = 255; b >= 0 && top < 0; b--) for (int j = 0; j < n; j++) if ((k[j][b >> 5] >> (b & 31)) & 1) { top = b; break; }
    G1XYZZ acc = G1XYZZ::inf();
    for (int b = top; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        for (int j = 0; j < n; j++) if ((k[j][b >> 5] >> (b & 31)) & 1) acc = xyzz_add_affine(acc, pts[j]);
    }
    return acc;
}

// vk: alpha1(64) beta2(128) gamma2(128) delta2(128) IC[nPublic+1](64 each); pub: nPublic x 32; proof: A(64) B(128) C(64); standard form
extern "C" int zkc_verify_bin(const uint8_t* vk, int nPublic, const uint8_t* pub, const uint8_t* proof) {
    g_err.clear();
    if (!vk || !pub || !proof || nPublic < 0 || nPublic > 4096) return vfail(-ZKC_ERR_BAD_ARG, "zkc_verify_bin: bad argument");
    int code = 0;
    const std::shared_ptr<const VkReady> V = vk_ready(vk, nPublic, &code);
    if (!V) return code;
    G1Affine A, C; G2Affine B;
    if (!rd_g1_std(A, proof) || !rd_g2_std(B, proof + 64) || !rd_g1_std(C, proof + 192)) return 0;
    // B must lie in the order-r subgroup of the twist (G2 has a cofactor): go-rapidsnark's bn256 unmarshalling and this library's batch verifier
    // reject such points too, so the two entry points agree on crafted proofs
    if (!g1_on_curve(A) || !g1_on_curve(C) || !g2_in_subgroup(B)) return 0;
    std::vector<std::array<uint32_t, 8>> k((size_t)nPublic);
    for (int i = 0; i < nPublic; i++) {
        memcpy(k[i].data(), pub + 32 * i, 32);
        if (!fp_std_lt_p<FrParams>(k[i].data())) return 0;                         // snarkjs: public input not in field -> invalid
    }
    G1XYZZ sum = G1XYZZ::inf();
    if (!V->ic_mult.empty()) {
        for (int w = 63; w >= 0; w--) {
            if (!sum.is_inf()) for (int d = 0; d < 4; d++) sum = xyzz_dbl(sum);
            for (int j = 0; j < nPublic; j++) { const uint32_t dg = (k[j][w >> 3] >> (4 * (w & 7))) & 15u; if (dg) sum = xyzz_add_affine(sum, V->ic_mult[15 * (size_t)j + dg - 1]); }
        }
    } else sum = g1_sum_of_products(V->ic.data() + 1, (const uint32_t (*)[8])k.data(), nPublic);
    const G1Affine vkx = xyzz_to_affine_gcd(xyzz_add_affine(sum, V->ic[0]));
    const G2Prepared pB = prepare_g2(B);
    const Pair pairs[3] = {{affine_neg(A), &pB}, {vkx, &V->pgamma}, {C, &V->pdelta}};
    return is_one12(final_exp(multi_miller(pairs, 3) * V->m_alpha_beta)) ? 1 : 0;
}

// JSON surface: the three artifact files of the reference (verification_key.json, signals.json, proof.json). 1 valid / 0 invalid / <0 error
extern "C" int zkc_verify(const char* vkey_json, const char* public_json, const char* proof_json) {
    g_err.clear();                                       // the text belongs to THIS call: a plain invalid proof (0) leaves it empty
    if (!vkey_json || !public_json || !proof_json) return vfail(-ZKC_ERR_BAD_ARG, "zkc_verify: bad argument");
    std::vector<uint8_t> vkb, pubb, prb; int np = 0; std::string perr;
    const int rc = parse::verify_inputs_from_json(vkey_json, public_json, proof_json, vkb, pubb, prb, np, perr);
    if (rc < 0) return vfail(-ZKC_ERR_FORMAT, perr);
    if (rc == 0) return 0;
    return zkc_verify_bin(vkb.data(), np, pubb.data(), prb.data());
}

// prover.ParseProof (zk_census_test.go:118) at the C ABI: proof.json + signals.json texts -> the binary forms every other entry point takes.  1 parsed / 0 well-formed
// documents with a value that is no encoding / <0 = -ZKC_ERR_* (text in zkc_verify_last_error)
extern "C" int zkc_proof_from_json(const char* proof_json, const char* public_json, uint8_t proof[256], uint8_t* pub, int* nPublic) {
    g_err.clear();
    if (!proof_json || !public_json || !nPublic) return vfail(-ZKC_ERR_BAD_ARG, "zkc_proof_from_json: bad argument");
    std::vector<uint8_t> pubb, prb; int np = 0; std::string perr;
    const int rc = parse::proof_from_json(public_json, proof_json, pubb, prb, np, perr);
    if (rc < 0) return vfail(-ZKC_ERR_FORMAT, perr);
    const int cap = *nPublic; *nPublic = np;
    if (rc == 0) return 0;
    if ((np && !pub) || cap < np) return vfail(-ZKC_ERR_SHORT_BUFFER, "zkc_proof_from_json: room for fewer public signals than the document holds");
    if (proof) memcpy(proof, prb.data(), 256);
    if (np) memcpy(pub, pubb.data(), 32ull * np);
    return 1;
}
// verification_key.json text -> the layout zkc_verify_bin / zkc_verify_batch take.  1 parsed / <0 = -ZKC_ERR_*; *vk_size: in = room, out = 448 + 64 (nPublic + 1)
extern "C" int zkc_vkey_from_json(const char* vkey_json, uint8_t* vk, unsigned long* vk_size, int* nPublic) {
    g_err.clear();
    if (!vkey_json || !vk_size) return vfail(-ZKC_ERR_BAD_ARG, "zkc_vkey_from_json: bad argument");
    std::vector<uint8_t> vkb; int nIC = 0; std::string perr;
    if (parse::vkey_from_json(vkey_json, vkb, nIC, perr) < 0) return vfail(-ZKC_ERR_FORMAT, perr);
    const unsigned long room = *vk_size; *vk_size = (unsigned long)vkb.size();
    if (nPublic) *nPublic = nIC - 1;
    if (!vk || room < vkb.size()) return vfail(-ZKC_ERR_SHORT_BUFFER, "zkc_vkey_from_json: buffer too small (size written back)");
    memcpy(vk, vkb.data(), vkb.size());
    return 1;
}

// proof 256 B + public signals -> the JSON texts snarkjs / rapidsnark emit (a8); returns needed size when the buffer is short
extern "C" int zkc_proof_to_json(const uint8_t proof[256], const uint8_t* pub, int nPublic, char* proof_buf, unsigned long* proof_size,
                                 char* public_buf, unsigned long* public_size) {
    if (!proof || (!pub && nPublic) || !proof_size || !public_size) return ZKC_ERR_BAD_ARG;
    auto d = [&](int off) { return "\"" + dec_of(proof + off) + "\""; };
    std::string pj = "{\"pi_a\":[" + d(0) + "," + d(32) + ",\"1\"],\"pi_b\":[[" + d(64) + "," + d(96) + "],[" + d(128) + "," + d(160) + "],[\"1\",\"0\"]],\"pi_c\":[" +
                     d(192) + "," + d(224) + ",\"1\"],\"protocol\":\"groth16\",\"curve\":\"bn128\"}";
    std::string sj = "[";
    for (int i = 0; i < nPublic; i++) sj += (i ? ",\"" : "\"") + dec_of(pub + 32 * i) + "\"";
    sj += "]";
    const bool shortbuf = !proof_buf || !public_buf || *proof_size < pj.size() + 1 || *public_size < sj.size() + 1;
    if (shortbuf) {      // report sizes that hold ANY proof of this shape (77 decimal digits per coordinate): r, s differ between calls
        *proof_size = 8 * 80 + 128; *public_size = (unsigned long)nPublic * 80 + 8;
        return ZKC_ERR_SHORT_BUFFER;
    }
    *proof_size = pj.size() + 1; *public_size = sj.size() + 1;
    memcpy(proof_buf, pj.c_str(), pj.size() + 1); memcpy(public_buf, sj.c_str(), sj.size() + 1);
    return ZKC_OK;
}

// .wtns (iden3 binfile) -> pointer to the nWitness x 32 B payload inside the buffer
extern "C" int zkc_wtns_parse(const void* wtns_bytes, unsigned long size, const uint8_t** payload, uint32_t* nWitness) {
    return parse::wtns_view((const uint8_t*)wtns_bytes, size, payload, nWitness) ? ZKC_OK : ZKC_ERR_FORMAT;
}
extern "C" unsigned long zkc_wtns_write(const void* payload, uint32_t nWitness, void* out, unsigned long out_size) {
    const unsigned long need = 12 + 12 + 40 + 12 + 32ul * nWitness;
    if (!out || out_size < need) return need;
    uint8_t* o = (uint8_t*)out; uint32_t v;
    memcpy(o, "wtns", 4); v = 2; memcpy(o + 4, &v, 4); memcpy(o + 8, &v, 4);
    uint64_t sz = 40; v = 1; memcpy(o + 12, &v, 4); memcpy(o + 16, &sz, 8);
    v = 32; memcpy(o + 24, &v, 4); memcpy(o + 28, FrParams::p, 32); memcpy(o + 60, &nWitness, 4);
    sz = 32ull * nWitness; v = 2; memcpy(o + 64, &v, 4); memcpy(o + 68, &sz, 8); memcpy(o + 76, payload, sz);
    return need;
}

// n scalars uniform in [0, r): 254 random bits from the OS generator, rejected when >= r (what snarkjs' Fr.random and rapidsnark do).  The bytes
// come from getrandom(2) in bulk: std::random_device costs a system call or an RDSEED per 32-bit word, 0.25 ms per scalar pair -- half a second
// for the 2048 scalars of a 1024-voter batch whose blinding the caller leaves to the library.
static void os_random(uint8_t* p, size_t n) {
    while (n) {
        const ssize_t got = getrandom(p, n < 4096 ? n : 4096, 0);
        if (got > 0) { p += got; n -= (size_t)got; continue; }
        if (got < 0 && errno == EINTR) continue;
        std::random_device rd;                                      // no getrandom (seccomp, ancient kernel): word by word
        for (size_t i = 0; i < n; i++) p[i] = (uint8_t)rd();
        return;
    }
}
extern "C" void zkc_random_scalars(uint8_t* out, size_t n) {
    std::vector<uint8_t> pool;
    size_t have = 0;
    for (size_t i = 0; i < n; i++) {
        uint32_t t[8];
        do {
            if (have == 0) { pool.resize(32 * std::min<size_t>(n - i + 8, 4096)); os_random(pool.data(), pool.size()); have = pool.size() / 32; }
            memcpy(t, pool.data() + 32 * (--have), 32); t[7] &= 0x3fffffffu;
        } while (!fp_std_lt_p<FrParams>(t));
        memcpy(out + 32 * i, t, 32);
    }
    if (!pool.empty()) memset(pool.data(), 0, pool.size());          // unused draws do not linger
}

// rapidsnark's entry point (prover.h), byte for byte: whole .zkey and .wtns buffers in, NUL-terminated JSON out.
// r and s are drawn from the OS generator like the reference provers do.  Re-entrant, and concurrent callers (goroutines over prover.Prove,
// zk_census_test.go:89) are coalesced: the call enqueues its witness with the process-wide proving service (zkc_service.hip; devices from
// $ZKC_DEVICE) and waits for its own proof.  The resident key is identified per call by the sampled fingerprint of the .zkey image and, once per
// (image, resident key), by the SHA-256 of the whole image (the identity the reference publishes for its keys,
// artifacts/zkCensus/dev/circuits-info.md:5).  When a buffer is too short the required sizes are written back WITHOUT proving (they depend only on nPublic).
extern "C" int groth16_prover(const void* zkey_buffer, unsigned long zkey_size, const void* wtns_buffer, unsigned long wtns_size,
                              char* proof_buffer, unsigned long* proof_size, char* public_buffer, unsigned long* public_size,
                              char* error_msg, unsigned long error_msg_maxsize) {
    auto err = [&](int code, const std::string& m) { return err_out(error_msg, error_msg_maxsize, code, m); };
    if (!zkey_buffer || !wtns_buffer || !proof_size || !public_size) return err(ZKC_ERR_GENERIC, "groth16_prover: null argument");
    // everything that does not need the GPU first: file shapes and buffer sizes
    parse::ZkeyHeader zh; std::string perr;
    if (!zkey_header(zkey_buffer, zkey_size, zh, perr)) return err(ZKC_ERR_GENERIC, perr);
    const uint8_t* payload; uint32_t nw;
    if (zkc_wtns_parse(wtns_buffer, wtns_size, &payload, &nw)) return err(ZKC_ERR_GENERIC, "Invalid witness file");
    if (nw != zh.nVars) return err(ZKC_ERR_INVALID_WITNESS_LENGTH, "Invalid witness length. Circuit: " + std::to_string(zh.nVars) + ", witness: " + std::to_string(nw));
    if (const long long bad = zkc::first_unreduced_wire(payload, nw); bad >= 0) return err(ZKC_ERR_GENERIC, zkc::unreduced_wire_msg(bad));
    if (!proof_json_room(zh.nPub, proof_buffer, proof_size, public_buffer, public_size)) return err(ZKC_ERR_SHORT_BUFFER, kShortJson);
    zkc_service* svc = zkc_service_default();
    if (!svc) return err(ZKC_ERR_GENERIC, zkc_service_last_error());
    uint8_t proof[256]; std::vector<uint8_t> pub(32 * (size_t)zh.nPub + 1); char etext[512] = {0};
    const int rc = zkc_service_prove(svc, zkey_buffer, zkey_size, payload, nw, nullptr, proof, pub.data(), etext, sizeof etext);
    if (rc) return err(rc == ZKC_ERR_INVALID_WITNESS_LENGTH ? rc : ZKC_ERR_GENERIC, etext);
    return proof_json_out(proof, pub.data(), zh.nPub, proof_buffer, proof_size, public_buffer, public_size, error_msg, error_msg_maxsize);
}
