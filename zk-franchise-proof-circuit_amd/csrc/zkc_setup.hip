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
#include "zkc_setup_write.h"
#include "../../include/zkcensus_ptau.h"
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

}  // namespace


namespace {

thread_local double g_setup_ms[4] = {0, 0, 0, 0};

// ---- stage 1: .r1cs -> scalars ----
// the five values a seed stands for: tau, alpha, beta, gamma, delta
void draw_waste(uint64_t seed, Fr w[5]) { Rng rng{seed}; for (int i = 0; i < 5; i++) w[i] = rng.fr(); }

int setup_scalars(const char* r1cs_path, const Fr waste[5], SetupScalars& S, char* err, size_t errlen) {
    std::vector<uint8_t> buf; int rc;
    if ((rc = read_file(r1cs_path, buf, err, errlen)) || (rc = setup_circuit(buf, S, err, errlen))) return rc;
    const uint32_t nWires = S.nWires, nPub = S.nPub, nCons = S.nCons, n = S.n;
    const std::vector<Cons>& cons = S.cons;
    uint32_t logn = 0; while ((1u << logn) < n) logn++;
    // ---- toxic waste ----
    const Fr tau = waste[0], alpha = waste[1], beta = waste[2], gamma = waste[3], delta = waste[4];
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

// ---- stage 3: points -> .zkey and verification_key.json: setup_write (zkc_setup_write.h), shared with zkc_setup_ptau.hip ----

}  // namespace

extern "C" int zkc_setup_from_r1cs(const char* r1cs_path, uint64_t seed, const char* zkey_path, const char* vkey_json_path,
                                   char* err, size_t errlen) {
    SetupScalars S; SetupPoints P;
    const clk::time_point t0 = clk::now();
    Fr waste[5]; draw_waste(seed, waste);
    int rc = setup_scalars(r1cs_path, waste, S, err, errlen); if (rc) return rc;
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
    Fr waste[5]; draw_waste(seed, waste);
    int rc = setup_scalars(r1cs_path, waste, S, err, errlen); if (rc) return rc;
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

// Test hook (zkcensus_ptau.h): the host generator with the waste given instead of drawn.  What a key from a powers-of-tau file of that (tau, alpha, beta) must equal at
// gamma = delta = 1 (tests/test_ptau_setup_cpu.py).  Every value is 32 bytes, little endian, standard form, in [1, r).
extern "C" int zkc_debug_setup_from_waste(const char* r1cs_path, const uint8_t tau[32], const uint8_t alpha[32], const uint8_t beta[32], const uint8_t gamma[32],
                                          const uint8_t delta[32], const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen) {
    if (!r1cs_path || !tau || !alpha || !beta || !gamma || !delta || !zkey_path) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_debug_setup_from_waste: bad argument");
    const uint8_t* in[5] = {tau, alpha, beta, gamma, delta}; Fr waste[5];
    for (int i = 0; i < 5; i++) {
        uint32_t s[8]; memcpy(s, in[i], 32);
        if (!fp_std_lt_p<FrParams>(s) || !(s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7])) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_debug_setup_from_waste: a value outside [1, r)");
        waste[i] = fp_from_std<FrParams>(s);
    }
    SetupScalars S; SetupPoints P;
    int rc = setup_scalars(r1cs_path, waste, S, err, errlen); if (rc) return rc;
    setup_points_host(S, P);
    return setup_write(S, P, zkey_path, vkey_json_path, err, errlen);
}
