// zkc_setup.hip -- TEST-ONLY Groth16 trusted setup with KNOWN toxic waste (product host code; the device entry point hands its points to zkc_fixedbase_dev.hip).
//
// Stand-in for the reference's ceremony `snarkjs groth16 setup / zkey contribute / beacon`
// (circuit/circuit-compiler.sh:99-136), needed because proving_key.zkey is a missing blob and unreproducible.
// Reads an iden3 .r1cs (written by r1cs.py), derives tau, alpha, beta, gamma, delta from a seed and writes a
// snarkjs-format Groth16 .zkey plus verification_key.json.  NOT for production keys: whoever knows
// the seed can forge proofs.  Knowing the waste also gives tests an exponent-space closed form for every MSM.
//
// Three stages.  1 (host): read the file, derive the waste, compute every scalar the key needs -- linear in the constraint matrix.  2: scalars -> points, fixed-base
// products of the two generators, on host threads (zkc_setup_from_r1cs: zkc_fixedbase.h) or on the GPU (zkc_setup_from_r1cs_dev: zkc_fixedbase_dev.hip).  3 (host):
// write the .zkey and the JSON.  Field elements are canonical and the affine form of a point is unique, so the two entry points write the same bytes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <functional>
#include "zkc_curve.h"
#include "zkc_fixedbase.h"
#include "zkc_fixedbase_dev.h"
#include "../../include/zkcensus.h"
#include "../../include/zkcensus_setup.h"

#include "zkc_hostparse.h"
#include "zkc_r1cs_parse.h"
#include "zkc_host_util.h"
using namespace zkc;

namespace {

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    Fr fr() {      // uniform-ish non-zero element: 253 random bits (< r)
        uint32_t v[8];
        for (int i = 0; i < 4; i++) { uint64_t x = next(); v[2 * i] = (uint32_t)x; v[2 * i + 1] = (uint32_t)(x >> 32); }
        v[7] &= 0x1fffffffu; if (!(v[0] | v[1])) v[0] = 1;
        return fp_from_std<FrParams>(v);
    }
};

Fr fr_pow(Fr a, uint64_t e) { Fr r = Fr::one(); while (e) { if (e & 1) r = r * a; a = a * a; e >>= 1; } return r; }
void batch_inverse(std::vector<Fr>& v) {  // in place; zeros stay zero
    std::vector<Fr> pre(v.size()); Fr acc = Fr::one();
    for (size_t i = 0; i < v.size(); i++) { pre[i] = acc; if (!v[i].is_zero()) acc = acc * v[i]; }
    Fr ai = fp_inv<FrParams>(acc);
    for (size_t i = v.size(); i-- > 0;) { if (v[i].is_zero()) continue; Fr t = ai * pre[i]; ai = ai * v[i]; v[i] = t; }
}

struct Term { uint32_t wire; Fr coef; };
struct Cons { std::vector<Term> a, b, c; };

void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
void put_raw(std::vector<uint8_t>& o, const void* p, size_t n) { o.insert(o.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
void put_g1(std::vector<uint8_t>& o, const G1Affine& p) { o.resize(o.size() + 64); wr_g1_mont(o.data() + o.size() - 64, p); }
void put_g2(std::vector<uint8_t>& o, const G2Affine& p) { o.resize(o.size() + 128); wr_g2_mont(o.data() + o.size() - 128, p); }

std::string dec_fq(const Fq& a) { uint8_t s[32]; wr_fq_std(s, a); return parse::dec_of(s); }
std::string json_g1(const G1Affine& p) { return "[\n  \"" + dec_fq(p.x) + "\",\n  \"" + dec_fq(p.y) + "\",\n  \"1\"\n ]"; }
std::string json_g2(const G2Affine& p) {
    return "[\n  [\n   \"" + dec_fq(p.x.c0) + "\",\n   \"" + dec_fq(p.x.c1) + "\"\n  ],\n  [\n   \"" + dec_fq(p.y.c0) + "\",\n   \"" + dec_fq(p.y.c1) +
           "\"\n  ],\n  [\n   \"1\",\n   \"0\"\n  ]\n ]";
}

int fail(char* err, size_t errlen, const std::string& m) { return err_out(err, errlen, ZKC_ERR_FORMAT, m); }

}  // namespace


namespace {

// what stage 1 leaves: the circuit, and every scalar of the key (Montgomery form)
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

thread_local double g_setup_ms[4] = {0, 0, 0, 0};

// ---- stage 1: .r1cs -> scalars ----
int setup_scalars(const char* r1cs_path, uint64_t seed, SetupScalars& S, char* err, size_t errlen) {
    // ---- read .r1cs ----
    FILE* f = fopen(r1cs_path, "rb"); if (!f) return fail(err, errlen, std::string("cannot open ") + r1cs_path);
    fseek(f, 0, SEEK_END); long sz = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf((size_t)sz); if (fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return fail(err, errlen, "short read"); } fclose(f);
    // ---- parse it (zkc_r1cs_parse.h: the host-only reader, with every check and its text) ----
    parse::R1cs cs; std::string perr;
    if (!parse::r1cs_parse(buf.data(), buf.size(), cs, perr)) return fail(err, errlen, perr);
    const uint32_t nWires = cs.h.nWires, nPub = cs.h.nPub, nCons = cs.h.nCons;
    std::vector<Cons>& cons = S.cons; cons.resize(nCons);
    for (uint32_t k = 0; k < nCons; k++) {
        std::vector<Term>* v[3] = {&cons[k].a, &cons[k].b, &cons[k].c};
        for (int m = 0; m < 3; m++) {
            const uint64_t t0 = cs.ptr[m][k], t1 = cs.ptr[m][k + 1];
            v[m]->resize((size_t)(t1 - t0));
            for (uint64_t t = t0; t < t1; t++) { uint32_t s[8]; memcpy(s, cs.terms[m][t].coef, 32); (*v[m])[t - t0] = Term{cs.terms[m][t].wire, fp_from_std<FrParams>(s)}; }
        }
    }
    uint32_t logn = 0; while ((1u << logn) < nCons + nPub + 1) logn++;
    const uint32_t n = 1u << logn;
    S.nWires = nWires; S.nPub = nPub; S.nCons = nCons; S.n = n;
    // ---- toxic waste ----
    Rng rng{seed};
    const Fr tau = rng.fr(), alpha = rng.fr(), beta = rng.fr(), gamma = rng.fr(), delta = rng.fr();
    S.alpha = alpha; S.beta = beta; S.gamma = gamma; S.delta = delta;
    const Fr w = fr_root_of_unity((int)logn), g = fr_root_of_unity((int)logn + 1);
    const Fr ninv = fp_inv<FrParams>(fp_from_u32<FrParams>(n));
    const Fr tn = fr_pow(tau, n), zt = tn - Fr::one();                     // Z(tau) = tau^n - 1
    // Lagrange basis at tau over H: L_c = Z(tau) w^c / (n (tau - w^c));  over the odd coset gH: L'_c = (-tau^n - 1) w^c / (n (tau/g - w^c))
    std::vector<Fr> wp(n), lag(n), lagc(n);
    wp[0] = Fr::one(); for (uint32_t i = 1; i < n; i++) wp[i] = wp[i - 1] * w;
    const Fr tg = tau * fp_inv<FrParams>(g);
    for (uint32_t i = 0; i < n; i++) { lag[i] = tau - wp[i]; lagc[i] = tg - wp[i]; }
    batch_inverse(lag); batch_inverse(lagc);
    const Fr zc = Fr::zero() - tn - Fr::one();
    for (uint32_t i = 0; i < n; i++) { lag[i] = lag[i] * wp[i] * zt * ninv; lagc[i] = lagc[i] * wp[i] * zc * ninv; }
    // ---- QAP polynomials at tau ----
    std::vector<Fr>& u = S.u; std::vector<Fr>& v = S.v; std::vector<Fr> ww(nWires, Fr::zero());
    u.assign(nWires, Fr::zero()); v.assign(nWires, Fr::zero());
    for (uint32_t k = 0; k < nCons; k++) {
        for (auto& t : cons[k].a) u[t.wire] = u[t.wire] + t.coef * lag[k];
        for (auto& t : cons[k].b) v[t.wire] = v[t.wire] + t.coef * lag[k];
        for (auto& t : cons[k].c) ww[t.wire] = ww[t.wire] + t.coef * lag[k];
    }
    for (uint32_t i = 0; i <= nPub; i++) u[i] = u[i] + lag[nCons + i];     // snarkjs' extra rows A[nCons+i][i] = 1
    // ---- the scalars of the C and H points ----
    const Fr dinv = fp_inv<FrParams>(delta), ginv = fp_inv<FrParams>(gamma);
    S.kc.resize(nWires); S.h.resize(n);
    parallel_for(nWires, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) S.kc[i] = (beta * u[i] + alpha * v[i] + ww[i]) * (i <= nPub ? ginv : dinv); });
    const Fr hk = zt * dinv * fp_inv<FrParams>(Fr::zero() - fp_from_u32<FrParams>(2));   // Z(tau) / (-2 delta)
    parallel_for(n, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) S.h[i] = lagc[i] * hk; });
    return ZKC_OK;
}

// ---- stage 2 on the host: fixed-base products on host threads ----
void setup_points_host(const SetupScalars& S, SetupPoints& P) {
    const clk::time_point t0 = clk::now();
    FixedBase<Fq> fb1(g1_generator()); FixedBase<Fq2> fb2(g2_generator());
    const clk::time_point t1 = clk::now();
    const uint32_t nWires = S.nWires, n = S.n;
    P.pA.resize(nWires); P.pB1.resize(nWires); P.pC.resize(nWires); P.pH.resize(n); P.pB2.resize(nWires);
    parallel_for(nWires, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) { P.pA[i] = fb1.mul(S.u[i]); P.pB1[i] = fb1.mul(S.v[i]); P.pB2[i] = fb2.mul(S.v[i]); P.pC[i] = fb1.mul(S.kc[i]); }
    });
    parallel_for(n, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) P.pH[i] = fb1.mul(S.h[i]); });
    P.alpha1 = fb1.mul(S.alpha); P.beta1 = fb1.mul(S.beta); P.delta1 = fb1.mul(S.delta);
    P.beta2 = fb2.mul(S.beta); P.gamma2 = fb2.mul(S.gamma); P.delta2 = fb2.mul(S.delta);
    g_setup_ms[1] = ms_since(t0, t1); g_setup_ms[2] = ms_since(t1);
}

// ---- stage 2 on the device: one batch per group.  G1: u | v | kc | h | alpha, beta, delta; G2: v | beta, gamma, delta.  The scalars go up as they are (Montgomery form)
// and the points come back in Montgomery form, which is what the vectors hold. ----
int setup_points_dev(zkc_ctx* ctx, const SetupScalars& S, SetupPoints& P) {
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t nWires = S.nWires, n = S.n, N1 = 3 * nWires + n + 3, N2 = nWires + 3;
    if (N1 > 0xffffffffull) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_setup_from_r1cs_dev: circuit too large");
    P.pA.resize(nWires); P.pB1.resize(nWires); P.pC.resize(nWires); P.pH.resize(n); P.pB2.resize(nWires);
    DevBuf k, out, t1, t2; int rc;
    const clk::time_point t0 = clk::now();
    if ((rc = fixed_table_g1(ctx, g1_generator(), (G1Affine**)&t1.p, nullptr)) || (rc = fixed_table_g2(ctx, g2_generator(), (uint32_t**)&t2.p, nullptr))) return rc;
    const clk::time_point t1e = clk::now();
    if ((rc = k.alloc(ctx, N1 * sizeof(Fr))) || (rc = out.alloc(ctx, std::max(N1 * sizeof(G1Affine), N2 * sizeof(G2Affine))))) return rc;
    Fr* dk = (Fr*)k.p;
    const Fr tail1[3] = {S.alpha, S.beta, S.delta}, tail2[3] = {S.beta, S.gamma, S.delta};
    ZKC_HIP_CHECK(ctx, hipMemcpy(dk, S.u.data(), nWires * sizeof(Fr), hipMemcpyHostToDevice));
    ZKC_HIP_CHECK(ctx, hipMemcpy(dk + nWires, S.v.data(), nWires * sizeof(Fr), hipMemcpyHostToDevice));
    ZKC_HIP_CHECK(ctx, hipMemcpy(dk + 2 * nWires, S.kc.data(), nWires * sizeof(Fr), hipMemcpyHostToDevice));
    ZKC_HIP_CHECK(ctx, hipMemcpy(dk + 3 * nWires, S.h.data(), n * sizeof(Fr), hipMemcpyHostToDevice));
    ZKC_HIP_CHECK(ctx, hipMemcpy(dk + 3 * nWires + n, tail1, sizeof(tail1), hipMemcpyHostToDevice));
    if ((rc = fixed_mul_g1(ctx, (const G1Affine*)t1.p, dk, true, (uint32_t)N1, out.p, true))) return rc;
    const G1Affine* o1 = (const G1Affine*)out.p; G1Affine got1[3];
    ZKC_HIP_CHECK(ctx, hipMemcpy(P.pA.data(), o1, nWires * sizeof(G1Affine), hipMemcpyDeviceToHost));
    ZKC_HIP_CHECK(ctx, hipMemcpy(P.pB1.data(), o1 + nWires, nWires * sizeof(G1Affine), hipMemcpyDeviceToHost));
    ZKC_HIP_CHECK(ctx, hipMemcpy(P.pC.data(), o1 + 2 * nWires, nWires * sizeof(G1Affine), hipMemcpyDeviceToHost));
    ZKC_HIP_CHECK(ctx, hipMemcpy(P.pH.data(), o1 + 3 * nWires, n * sizeof(G1Affine), hipMemcpyDeviceToHost));
    ZKC_HIP_CHECK(ctx, hipMemcpy(got1, o1 + 3 * nWires + n, sizeof(got1), hipMemcpyDeviceToHost));
    P.alpha1 = got1[0]; P.beta1 = got1[1]; P.delta1 = got1[2];
    // G2: v is on the device already; its three key scalars follow it in place of kc's first three
    ZKC_HIP_CHECK(ctx, hipMemcpy(dk + 2 * nWires, tail2, sizeof(tail2), hipMemcpyHostToDevice));
    if ((rc = fixed_mul_g2(ctx, (const uint32_t*)t2.p, dk + nWires, true, (uint32_t)N2, out.p, true))) return rc;
    const G2Affine* o2 = (const G2Affine*)out.p; G2Affine got2[3];
    ZKC_HIP_CHECK(ctx, hipMemcpy(P.pB2.data(), o2, nWires * sizeof(G2Affine), hipMemcpyDeviceToHost));
    ZKC_HIP_CHECK(ctx, hipMemcpy(got2, o2 + nWires, sizeof(got2), hipMemcpyDeviceToHost));
    P.beta2 = got2[0]; P.gamma2 = got2[1]; P.delta2 = got2[2];
    g_setup_ms[1] = ms_since(t0, t1e); g_setup_ms[2] = ms_since(t1e);
    return ZKC_OK;
}

// ---- stage 3: points -> .zkey and verification_key.json ----
int setup_write(const SetupScalars& S, const SetupPoints& P, const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen) {
    const uint32_t nWires = S.nWires, nPub = S.nPub, nCons = S.nCons, n = S.n;
    const std::vector<Cons>& cons = S.cons;
    const std::vector<G1Affine>&pA = P.pA, &pB1 = P.pB1, &pC = P.pC, &pH = P.pH; const std::vector<G2Affine>& pB2 = P.pB2;
    const G1Affine &alpha1 = P.alpha1, &beta1 = P.beta1, &delta1 = P.delta1; const G2Affine &beta2 = P.beta2, &gamma2 = P.gamma2, &delta2 = P.delta2;
    // ---- .zkey ----
    std::vector<std::vector<uint8_t>> sec(11);
    put32(sec[1], 1);
    put32(sec[2], 32); put_raw(sec[2], FqParams::p, 32); put32(sec[2], 32); put_raw(sec[2], FrParams::p, 32);
    put32(sec[2], nWires); put32(sec[2], nPub); put32(sec[2], n);
    put_g1(sec[2], alpha1); put_g1(sec[2], beta1); put_g2(sec[2], beta2); put_g2(sec[2], gamma2); put_g1(sec[2], delta1); put_g2(sec[2], delta2);
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
    sec[10].assign(64, 0); put32(sec[10], 0);                              // circuit hash (unused here), 0 contributions
    FILE* o = fopen(zkey_path, "wb"); if (!o) return fail(err, errlen, std::string("cannot write ") + zkey_path);
    fwrite("zkey", 1, 4, o); uint32_t ver = 1, ns = 10; fwrite(&ver, 4, 1, o); fwrite(&ns, 4, 1, o);
    for (uint32_t id = 1; id <= 10; id++) { uint64_t len = sec[id].size(); fwrite(&id, 4, 1, o); fwrite(&len, 8, 1, o); fwrite(sec[id].data(), 1, len, o); }
    fclose(o);
    // ---- verification_key.json (members and order of artifacts/zkCensus/dev/160/verification_key.json, vk_alphabeta_12 = e(alpha1, beta2)
    //      as snarkjs' `zkey export verificationkey` prints it, circuit/circuit-compiler.sh:133-134) ----
    if (vkey_json_path) {
        std::string j = "{\n \"protocol\": \"groth16\",\n \"curve\": \"bn128\",\n \"nPublic\": " + std::to_string(nPub) + ",\n";
        j += " \"vk_alpha_1\": " + json_g1(alpha1) + ",\n \"vk_beta_2\": " + json_g2(beta2) + ",\n \"vk_gamma_2\": " + json_g2(gamma2) + ",\n \"vk_delta_2\": " + json_g2(delta2) + ",\n";
        {
            uint8_t a[64], b[128], e[384];
            wr_g1_std(a, alpha1); wr_g2_std(b, beta2);
            if (zkc_pairing_bin(a, b, e) != ZKC_OK) return fail(err, errlen, "pairing e(alpha, beta) failed");
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
        FILE* v = fopen(vkey_json_path, "wb"); if (!v) return fail(err, errlen, std::string("cannot write ") + vkey_json_path);
        fwrite(j.data(), 1, j.size(), v); fclose(v);
    }
    return ZKC_OK;
}

}  // namespace

extern "C" int zkc_setup_from_r1cs(const char* r1cs_path, uint64_t seed, const char* zkey_path, const char* vkey_json_path,
                                   char* err, size_t errlen) {
    SetupScalars S; SetupPoints P;
    const clk::time_point t0 = clk::now();
    int rc = setup_scalars(r1cs_path, seed, S, err, errlen); if (rc) return rc;
    const clk::time_point t1 = clk::now(); g_setup_ms[0] = ms_since(t0, t1);
    setup_points_host(S, P);
    const clk::time_point t2 = clk::now();
    rc = setup_write(S, P, zkey_path, vkey_json_path, err, errlen);
    g_setup_ms[3] = ms_since(t2);
    return rc;
}

// The same key with stage 2 on ctx's GPU (zkcensus_setup.h).
extern "C" int zkc_setup_from_r1cs_dev(zkc_ctx* ctx, const char* r1cs_path, uint64_t seed, const char* zkey_path, const char* vkey_json_path,
                                       char* err, size_t errlen) {
    if (!ctx) { if (err && errlen) snprintf(err, errlen, "zkc_setup_from_r1cs_dev: no context"); return ZKC_ERR_BAD_ARG; }
    SetupScalars S; SetupPoints P;
    const clk::time_point t0 = clk::now();
    int rc = setup_scalars(r1cs_path, seed, S, err, errlen); if (rc) return rc;
    const clk::time_point t1 = clk::now(); g_setup_ms[0] = ms_since(t0, t1);
    if ((rc = setup_points_dev(ctx, S, P))) { if (err && errlen) snprintf(err, errlen, "%s", zkc_last_error(ctx)); return rc; }
    const clk::time_point t2 = clk::now();
    rc = setup_write(S, P, zkey_path, vkey_json_path, err, errlen);
    g_setup_ms[3] = ms_since(t2);
    return rc;
}

extern "C" int zkc_setup_stats(double ms[4]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    for (int i = 0; i < 4; i++) ms[i] = g_setup_ms[i];
    return ZKC_OK;
}
