// zkc_setup_write.h -- what a Groth16 key is made of on the host, and the ONE writer of its files (product host code): the circuit, scalars and points the two generators
// leave (zkc_setup.hip from a seed, zkc_setup_ptau.hip from a powers-of-tau file) and their way into a snarkjs-format .zkey and verification_key.json.
// Host only, internal to the library.  Both generators go through setup_image / setup_write, so they write the same layout by construction.
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "zkc_curve.h"
#include "zkc_hostparse.h"
#include "zkc_r1cs_parse.h"
#include "zkc_host_util.h"
#include "../../include/zkcensus.h"

#pragma GCC visibility push(hidden)
namespace zkc {

struct Term { uint32_t wire; Fr coef; };
struct Cons { std::vector<Term> a, b, c; };

inline void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
inline void put_raw(std::vector<uint8_t>& o, const void* p, size_t n) { o.insert(o.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
inline void put_g1(std::vector<uint8_t>& o, const G1Affine& p) { o.resize(o.size() + 64); wr_g1_mont(o.data() + o.size() - 64, p); }
inline void put_g2(std::vector<uint8_t>& o, const G2Affine& p) { o.resize(o.size() + 128); wr_g2_mont(o.data() + o.size() - 128, p); }

inline std::string dec_fq(const Fq& a) { uint8_t s[32]; wr_fq_std(s, a); return parse::dec_of(s); }
inline std::string json_g1(const G1Affine& p) { return "[\n  \"" + dec_fq(p.x) + "\",\n  \"" + dec_fq(p.y) + "\",\n  \"1\"\n ]"; }
inline std::string json_g2(const G2Affine& p) {
    return "[\n  [\n   \"" + dec_fq(p.x.c0) + "\",\n   \"" + dec_fq(p.x.c1) + "\"\n  ],\n  [\n   \"" + dec_fq(p.y.c0) + "\",\n   \"" + dec_fq(p.y.c1) +
           "\"\n  ],\n  [\n   \"1\",\n   \"0\"\n  ]\n ]";
}

inline int setup_fail(char* err, size_t errlen, const std::string& m) { return err_out(err, errlen, ZKC_ERR_FORMAT, m); }

// what stage 1 leaves: the circuit, and every scalar of the key (Montgomery form).  The powers-of-tau generator fills the circuit part only: it never sees a scalar.
struct SetupScalars {
    uint32_t nWires = 0, nPub = 0, nCons = 0, n = 0;             // n: the domain size
    std::vector<Cons> cons;
    std::vector<Fr> u, v, kc;                                    // per wire: A(tau), B(tau), (beta A + alpha B + C)(tau) / gamma (public wires) or / delta
    std::vector<Fr> h;                                           // per domain point: L'_i(tau) Z(tau) / (-2 delta)
    Fr alpha, beta, gamma, delta;
};
// what stage 2 leaves: the same, times the generators
struct SetupPoints {
    std::vector<G1Affine> pA, pB1, pC, pH; std::vector<G2Affine> pB2;
    G1Affine alpha1, beta1, delta1; G2Affine beta2, gamma2, delta2;
};

// a whole file into memory
inline int read_file(const char* path, std::vector<uint8_t>& buf, char* err, size_t errlen) {
    FILE* f = fopen(path, "rb"); if (!f) return setup_fail(err, errlen, std::string("cannot open ") + path);
    fseek(f, 0, SEEK_END); long sz = ftell(f); fseek(f, 0, SEEK_SET);
    buf.resize((size_t)sz); if (fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return setup_fail(err, errlen, "short read"); } fclose(f);
    return ZKC_OK;
}

// an .r1cs image (zkc_r1cs_parse.h: the host-only reader, with every check and its text) -> the circuit part of S: the constraints in Montgomery form, the counts, the domain
inline int setup_circuit(const std::vector<uint8_t>& buf, SetupScalars& S, char* err, size_t errlen) {
    parse::R1cs cs; std::string perr;
    if (!parse::r1cs_parse(buf.data(), buf.size(), cs, perr)) return setup_fail(err, errlen, perr);
    const uint32_t nCons = cs.h.nCons;
    std::vector<Cons>& cons = S.cons; cons.resize(nCons);
    for (uint32_t k = 0; k < nCons; k++) {
        std::vector<Term>* v[3] = {&cons[k].a, &cons[k].b, &cons[k].c};
        for (int m = 0; m < 3; m++) {
            const uint64_t t0 = cs.ptr[m][k], t1 = cs.ptr[m][k + 1];
            v[m]->resize((size_t)(t1 - t0));
            for (uint64_t t = t0; t < t1; t++) { uint32_t s[8]; memcpy(s, cs.terms[m][t].coef, 32); (*v[m])[t - t0] = Term{cs.terms[m][t].wire, fp_from_std<FrParams>(s)}; }
        }
    }
    uint32_t logn = 0; while ((1u << logn) < nCons + cs.h.nPub + 1) logn++;
    S.nWires = cs.h.nWires; S.nPub = cs.h.nPub; S.nCons = nCons; S.n = 1u << logn;
    return ZKC_OK;
}

// ---- stage 3: points -> the .zkey image.  cs_hash: the 64 bytes section 10 opens with (NULL: zeros, what a seeded key carries); no contributions ----
inline std::vector<uint8_t> setup_image(const SetupScalars& S, const SetupPoints& P, const uint8_t* cs_hash) {
    const uint32_t nWires = S.nWires, nPub = S.nPub, nCons = S.nCons, n = S.n;
    const std::vector<Cons>& cons = S.cons;
    const std::vector<G1Affine>&pA = P.pA, &pB1 = P.pB1, &pC = P.pC, &pH = P.pH; const std::vector<G2Affine>& pB2 = P.pB2;
    std::vector<std::vector<uint8_t>> sec(11);
    put32(sec[1], 1);
    put32(sec[2], 32); put_raw(sec[2], FqParams::p, 32); put32(sec[2], 32); put_raw(sec[2], FrParams::p, 32);
    put32(sec[2], nWires); put32(sec[2], nPub); put32(sec[2], n);
    put_g1(sec[2], P.alpha1); put_g1(sec[2], P.beta1); put_g2(sec[2], P.beta2); put_g2(sec[2], P.gamma2); put_g1(sec[2], P.delta1); put_g2(sec[2], P.delta2);
    for (uint32_t i = 0; i <= nPub; i++) put_g1(sec[3], pC[i]);
    {
        uint32_t ncoef = nPub + 1; for (auto& c : cons) ncoef += (uint32_t)(c.a.size() + c.b.size());
        put32(sec[4], ncoef);
        Fr r2; for (int i = 0; i < 8; i++) r2.v[i] = FrParams::r2[i];
        auto put_coef = [&](uint32_t m, uint32_t c, uint32_t s, const Fr& val) { put32(sec[4], m); put32(sec[4], c); put32(sec[4], s); Fr dm = val * r2; put_raw(sec[4], dm.v, 32); };
        for (uint32_t k = 0; k < nCons; k++) { for (auto& t : cons[k].a) put_coef(0, k, t.wire, t.coef); for (auto& t : cons[k].b) put_coef(1, k, t.wire, t.coef); }
        for (uint32_t i = 0; i <= nPub; i++) put_coef(0, nCons + i, i, Fr::one());
    }
    for (uint32_t i = 0; i < nWires; i++) { put_g1(sec[5], pA[i]); put_g1(sec[6], pB1[i]); put_g2(sec[7], pB2[i]); }
    for (uint32_t i = nPub + 1; i < nWires; i++) put_g1(sec[8], pC[i]);
    for (uint32_t i = 0; i < n; i++) put_g1(sec[9], pH[i]);
    if (cs_hash) put_raw(sec[10], cs_hash, 64); else sec[10].assign(64, 0);
    put32(sec[10], 0);                                                     // circuit hash, 0 contributions
    std::vector<uint8_t> o;
    size_t total = 12; for (uint32_t id = 1; id <= 10; id++) total += 12 + sec[id].size();
    o.reserve(total);
    put_raw(o, "zkey", 4); put32(o, 1); put32(o, 10);
    for (uint32_t id = 1; id <= 10; id++) { const uint64_t len = sec[id].size(); put32(o, id); put_raw(o, &len, 8); put_raw(o, sec[id].data(), sec[id].size()); }
    return o;
}

// ---- the image into zkey_path, and verification_key.json (members and order of artifacts/zkCensus/dev/160/verification_key.json, vk_alphabeta_12 = e(alpha1, beta2)
//      as snarkjs' `zkey export verificationkey` prints it, circuit/circuit-compiler.sh:133-134) ----
inline int setup_write(const SetupScalars& S, const SetupPoints& P, const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen, const uint8_t* cs_hash = nullptr) {
    const uint32_t nPub = S.nPub;
    const std::vector<G1Affine>& pC = P.pC;
    const G1Affine& alpha1 = P.alpha1; const G2Affine &beta2 = P.beta2, &gamma2 = P.gamma2, &delta2 = P.delta2;
    // the JSON first: nothing is written when the pairing fails
    std::string j;
    if (vkey_json_path) {
        j = "{\n \"protocol\": \"groth16\",\n \"curve\": \"bn128\",\n \"nPublic\": " + std::to_string(nPub) + ",\n";
        j += " \"vk_alpha_1\": " + json_g1(alpha1) + ",\n \"vk_beta_2\": " + json_g2(beta2) + ",\n \"vk_gamma_2\": " + json_g2(gamma2) + ",\n \"vk_delta_2\": " + json_g2(delta2) + ",\n";
        {
            uint8_t a[64], b[128], e[384];
            wr_g1_std(a, alpha1); wr_g2_std(b, beta2);
            if (zkc_pairing_bin(a, b, e) != ZKC_OK) return setup_fail(err, errlen, "pairing e(alpha, beta) failed");
            j += " \"vk_alphabeta_12\": [\n";
            for (int h = 0; h < 2; h++) {
                j += "  [\n";
                for (int k = 0; k < 3; k++) j += "   [\"" + zkc::parse::dec_of(e + 64 * (3 * h + k)) + "\", \"" + zkc::parse::dec_of(e + 64 * (3 * h + k) + 32) + "\"]" + (k < 2 ? ",\n" : "\n");
                j += h == 0 ? "  ],\n" : "  ]\n";
            }
            j += " ],\n";
        }
        j += " \"IC\": [\n";
        for (uint32_t i = 0; i <= nPub; i++) j += "  " + json_g1(pC[i]) + (i < nPub ? ",\n" : "\n");
        j += " ]\n}\n";
    }
    const std::vector<uint8_t> img = setup_image(S, P, cs_hash);
    FILE* o = fopen(zkey_path, "wb"); if (!o) return setup_fail(err, errlen, std::string("cannot write ") + zkey_path);
    const bool okw = fwrite(img.data(), 1, img.size(), o) == img.size();
    if (fclose(o) != 0 || !okw) return setup_fail(err, errlen, std::string("cannot write ") + zkey_path);
    if (vkey_json_path) {
        FILE* v = fopen(vkey_json_path, "wb"); if (!v) return setup_fail(err, errlen, std::string("cannot write ") + vkey_json_path);
        fwrite(j.data(), 1, j.size(), v); fclose(v);
    }
    return ZKC_OK;
}

}  // namespace zkc
#pragma GCC visibility pop
