// host check of the addition chain of zkc_p2_scale_g1 (csrc/zkc_phase2.hip, through G1Ops::dbl and add_point of zkc_point_ops.h): f29_acc_dbl and f29_madd alternating on one accumulator along the non-adjacent form of a
// scalar, against xyzz_mul of zkc_curve.h on points of the curve.  Also records the largest top limb each accumulator coordinate reaches, against the invariant the two
// formulas state (X, Y < 10.5 p; ZZ, ZZZ < 4 p).  The recoding below restates the library's (digit = 2 - (k mod 4) for odd k).
#include <array>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "zkc_curve.h"
#include "zkc_f29_g1.h"
using namespace zkc;

static uint32_t worst[4] = {0, 0, 0, 0};
static void track(const Acc29& a) {
    const uint32_t* all[4] = {a.X, a.Y, a.ZZ, a.ZZZ};
    for (int q = 0; q < 4; q++) if (all[q][8] > worst[q]) worst[q] = all[q][8];
}
static G1Affine scale(const G1Affine& p, const uint32_t k_in[8], int* exceptional) {
    int8_t dig[260] = {0}; int top = -1;
    uint32_t k[9]; memcpy(k, k_in, 32); k[8] = 0;
    for (int j = 0; j < 258; j++) {
        if (k[0] & 1) {
            if ((k[0] & 3) == 1) { dig[j] = 1; k[0] -= 1; }
            else { dig[j] = -1; uint64_t c = 1; for (int i = 0; i < 9 && c; i++) { c += k[i]; k[i] = (uint32_t)c; c >>= 32; } }
            top = j;
        }
        for (int i = 0; i < 8; i++) k[i] = (k[i] >> 1) | (k[i + 1] << 31);
        k[8] >>= 1;
    }
    if (top < 0) return G1Affine::inf();
    const Fq ny = fp_neg(p.y);
    uint32_t px[9], py[9], pny[9];
    f29_enter_fq(px, p.x.v); f29_enter_fq(py, p.y.v); f29_enter_fq(pny, ny.v);
    Acc29 acc; memcpy(acc.X, px, 36); memcpy(acc.Y, py, 36); memcpy(acc.ZZ, F29K<FqParams>::one.l, 36); memcpy(acc.ZZZ, F29K<FqParams>::one.l, 36);
    for (int j = top - 1; j >= 0; j--) {
        f29_acc_dbl(acc); track(acc);
        if (dig[j]) {
            bool same_y = false;
            if (!f29_madd(acc, px, dig[j] < 0 ? pny : py, same_y)) { (*exceptional)++; if (same_y) f29_acc_dbl(acc); else return G1Affine::inf(); }
            track(acc);
        }
    }
    return xyzz_to_affine(f29_pt_to_xyzz(acc));
}

int main() {
    std::mt19937_64 rng(77);
    int bad = 0, exceptional = 0, exc_r2 = 0;
    const G1Affine G{Fq::one(), fp_from_u32<FqParams>(2)};
    auto rnd_scalar = [&](uint32_t k[8]) { for (int i = 0; i < 8; i++) k[i] = (uint32_t)rng(); k[7] &= 0x1fffffffu; };
    std::vector<std::array<uint32_t, 8>> ks;
    auto push = [&](const uint32_t k[8]) { std::array<uint32_t, 8> a; memcpy(a.data(), k, 32); ks.push_back(a); };
    uint32_t r[8]; memcpy(r, FrParams::p, 32);
    auto sub_small = [&](const uint32_t a[8], uint32_t s, uint32_t o[8]) { int64_t br = s; for (int i = 0; i < 8; i++) { int64_t v = (int64_t)a[i] - br; br = v < 0; o[i] = (uint32_t)v; } };
    uint32_t t[8] = {0};
    t[0] = 1; push(t); t[0] = 2; push(t); t[0] = 3; push(t);
    sub_small(r, 1, t); push(t);
    const size_t idx_r2 = ks.size(); sub_small(r, 2, t); push(t);
    sub_small(r, 1, t); for (int i = 0; i < 8; i++) t[i] = (t[i] >> 1) | (i < 7 ? t[i + 1] << 31 : 0); push(t);                           // (r - 1) / 2
    { uint64_t c = 1; for (int i = 0; i < 8; i++) { c += t[i]; t[i] = (uint32_t)c; c >>= 32; } push(t); }                                   // (r + 1) / 2
    memset(t, 0, 32); t[7] = 1u << 29; push(t);                                                                                             // 2^253
    for (int i = 0; i < 8; i++) t[i] = 0xffffffffu; t[7] = (1u << 29) - 1; push(t);                                                        // 2^253 - 1
    for (int i = 0; i < 8; i++) t[i] = 0x55555555u; t[7] &= 0x1fffffffu; push(t);
    for (int i = 0; i < 8; i++) t[i] = 0xaaaaaaaau; t[7] &= 0x1fffffffu; push(t);
    for (int i = 0; i < 40; i++) { rnd_scalar(t); push(t); }
    for (int b = 0; b < 4; b++) {
        uint32_t a[8]; rnd_scalar(a);
        const G1Affine P = b == 0 ? G : xyzz_to_affine(xyzz_mul(G1XYZZ::from_affine(G), a));
        for (size_t i = 0; i < ks.size(); i++) {
            int exc = 0;
            const G1Affine got = scale(P, ks[i].data(), &exc), ref = xyzz_to_affine(xyzz_mul(G1XYZZ::from_affine(P), ks[i].data()));
            if (!(got.x == ref.x && got.y == ref.y)) { if (bad < 5) printf("mismatch base %d scalar %zu\n", b, i); bad++; }
            if (i == idx_r2) exc_r2 += exc; else exceptional += exc;
        }
    }
    if (exceptional) { printf("exceptional case met for a scalar other than r - 2\n"); bad++; }
    if (exc_r2 != 4) { printf("r - 2 did not meet the exceptional case once per base (%d)\n", exc_r2); bad++; }
    const uint32_t ptop = FqParams::p[7] >> 8;
    const double lim[4] = {10.5, 10.5, 4.0, 4.0};
    for (int q = 0; q < 4; q++) if ((double)worst[q] > lim[q] * ptop) { printf("coordinate %d leaves the accumulator invariant\n", q); bad++; }
    printf("G1 scale chain: %d mismatches; largest top limbs in units of p: X %.2f Y %.2f ZZ %.2f ZZZ %.2f\n", bad, (double)worst[0] / ptop, (double)worst[1] / ptop,
           (double)worst[2] / ptop, (double)worst[3] / ptop);
    return bad != 0;
}
