// Canonical operands for the radix-2^29 host checks (f29_*_host_test.hip): the whole range [0, p), not just below 2^252.
// Half the draws are uniform over [0, p) (rejection from the bit length of p); the other half sit at the top of the range, where
// the lazy bounds ("value < 32 p", limbs of 2^30.6) are tightest: p - 1 - small, p - 2^k, and values whose eight low 29-bit limbs
// are all 2^29 - 1 (the top limb below p's, so the value stays below p).
#pragma once
#include <cstdint>
#include <random>
#include "zkc_field.h"

template <class P> zkc::Fp<P> f29_operand(std::mt19937_64& rng) {
    zkc::Fp<P> r;
    uint32_t topmask = 1; while (topmask <= P::p[7]) topmask = (topmask << 1) | 1;      // bits of p's top word
    const uint32_t kind = (uint32_t)(rng() % 8);
    if (kind < 4) {
        do { for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)rng(); r.v[7] &= topmask; } while (!zkc::fp_std_lt_p<P>(r.v));
        return r;
    }
    if (kind < 7) {                                     // p - t with t = 1 + small (kinds 4, 5) or t = 2^k, k < 254 (kind 6)
        uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kind < 6) t[0] = 1 + (uint32_t)(rng() & 0xffff);
        else { const uint32_t k = (uint32_t)(rng() % 254); t[k >> 5] = 1u << (k & 31); }
        uint64_t br = 0;
        for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)P::p[i] - t[i] - br; r.v[i] = (uint32_t)d; br = (d >> 63) & 1; }
        return r;
    }
    // limbs 0..7 (bits 0..231) all ones, limb 8 (bits 232..) below p's
    const uint32_t ptop = P::p[7] >> 8;
    const uint32_t top = (uint32_t)(rng() % ptop);
    for (int i = 0; i < 7; i++) r.v[i] = 0xffffffffu;
    r.v[7] = (top << 8) | 0xffu;
    return r;
}
