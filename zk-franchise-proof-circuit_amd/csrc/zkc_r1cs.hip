// zkc_r1cs.hip -- f5: witnesses checked against a constraint system (include/zkcensus_r1cs.h; `snarkjs wtns check`, snarkjs.wtns.check).
//
// zkc_r1cs_load   parses an iden3 .r1cs image with the host-only reader (zkc_r1cs_parse.h) and keeps A, B and C on the device as ONE jagged-diagonal matrix of merged rows:
//                 row k = the terms of A_k, then of B_k, then of C_k.
// zkc_r1cs_check  per witness of a batch: wire 0 == 1 and every wire < r (zkc_r1cs_range), then <A_k, w> * <B_k, w> == <C_k, w> for every k (zkc_r1cs_check_rows); the
//                 verdict is the lowest violated k in file order and the number of violated constraints.
//
// Layout.  One lane evaluates the three rows of one constraint, does the one product and compares: nothing but two words per witness ever goes back to HBM (the prover's
// buildABC writes 3 n field elements per proof because the transforms need them; a check does not).  The constraints are sorted by the length of their merged row, longest
// first (stable), and stored in the jagged-diagonal order of zkc_zkey_load: slot jdptr[j] + s holds the j-th term of the s-th longest row, so the loads of a wave's lanes
// are contiguous and neighbouring lanes have (nearly) equal work.  rows[s] = (end of A, end of B, end of C, index in the file) for the s-th longest: the verdict is a
// FILE index, the sort is only the device's.  Coefficients are stored as zkc_zkey_load stores the key's: val R^2, so that one Montgomery product with the standard-form
// wire is the term in Montgomery form, with +1 / -1 marked in the two top bits of the wire word (MV_UNIT / MV_NEG, zkc_jds.h) and served by the wire's Montgomery form
// from zkc_wtns_mont.  The three sums are then Montgomery forms, and so are their product and the comparison.
//
// Long rows.  The first `nlong` rows (more than R1CS_LONG terms) get a wave each: lane l takes terms l, l + 64, ... and the three sums are reduced by shuffles.  The
// threshold follows MATVEC_LONG (zkc_prove.hip: a row of more than 16 coefficients is summed by a wave, because above it a lane's chain of dependent gathers costs more
// than one round of gathers and a six-step shuffle reduction).  A merged row is three such rows and its wave reduces three sums, three times that fixed cost:
// R1CS_LONG = 3 x 16 = 48.  At nLevels 160 the census circuit has 82 435 merged rows of 1 142 528 terms; 6 997 of them are long, the longest has 521 terms.
//
// Verdicts.  Per witness three words: `first` (preset to 0xffffffff), `count` and `flag` (zeroed).  zkc_r1cs_range ORs bit 0 (a wire >= r) or bit 1 (wire 0 != 1) into
// flag; zkc_r1cs_check_rows, launched behind it on the same stream, returns at once for a witness whose flag is set -- the two negative verdicts are decided before any
// constraint is looked at.  A wave that found violations takes the minimum of their file indices by shuffles and their number from the ballot, and its first lane issues
// one atomicMin and one atomicAdd.  A satisfied witness costs no atomic at all.
#include "zkc_census_host.h"
#include "zkc_r1cs_parse.h"
#include "zkc_kernels.h"
#include "../../include/zkcensus_r1cs.h"
#include <algorithm>
#include <vector>

using namespace zkc;

static constexpr uint32_t R1CS_LONG = 48;              // merged rows with more terms are summed by a whole wave (see above)

namespace zkc {

// flag[witness] |= 1 if a wire is >= r, |= 2 if wire 0 is not 1.  grid (ceil(nWires / 256), witnesses)
extern "C" __global__ void __launch_bounds__(256)
zkc_r1cs_range(const Fr* __restrict__ wtns_std, size_t wtns_stride, uint32_t nWires, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t f = 0;
    if (i < nWires) {
        const Fr x = ld_fr(wtns_std + (size_t)blockIdx.y * wtns_stride + i);
        if (!fp_std_lt_p<FrParams>(x.v)) f |= 1u;
        if (i == 0) { uint32_t o = x.v[0] ^ 1u; for (int k = 1; k < 8; k++) o |= x.v[k]; if (o) f |= 2u; }
    }
    for (int d = 32; d > 0; d >>= 1) f |= (uint32_t)__shfl_xor((int)f, d, 64);
    if ((threadIdx.x & 63u) == 0 && f) atomicOr(flag + blockIdx.y, f);
}

// grid (ceil((nCons + 63 nlong) / 256), witnesses): waves [0, nlong) take the long rows, every later lane one row
extern "C" __global__ void __launch_bounds__(256)
zkc_r1cs_check_rows(const uint4* __restrict__ rows, const uint32_t* __restrict__ jdptr, const uint32_t* __restrict__ col, const Fr* __restrict__ val,
                    const Fr* __restrict__ wtns_std, size_t wtns_stride, const Fr* __restrict__ wm_all, size_t wm_stride, uint32_t nCons, uint32_t nlong,
                    uint32_t* __restrict__ first, uint32_t* __restrict__ count, const uint32_t* __restrict__ flag) {
    if (flag[blockIdx.y]) return;                   // block-uniform: NOT_ONE / WIRE_RANGE, decided by the launch before this one
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const Fr* __restrict__ w = wtns_std + (size_t)blockIdx.y * wtns_stride;
    const Fr* __restrict__ wm = wm_all ? wm_all + (size_t)blockIdx.y * wm_stride : nullptr;
    Fr a = Fr::zero(), b = Fr::zero(), c = Fr::zero();
    bool decide = false; uint32_t file = 0xffffffffu;
    if ((t >> 6) < nlong) {                         // wave-uniform
        const uint32_t s = t >> 6; const uint4 row = rows[s];
        for (uint32_t j = lane; j < row.z; j += 64) {
            const uint32_t idx = jdptr[j] + s; const Fr x = mv_term(val, w, wm, idx, col[idx]);
            if (j < row.x) a = a + x; else if (j < row.y) b = b + x; else c = c + x;
        }
        for (int d = 32; d > 0; d >>= 1) {
            Fr oa, ob, oc;
#pragma unroll
            for (int i = 0; i < 8; i++) { oa.v[i] = (uint32_t)__shfl_down((int)a.v[i], d, 64); ob.v[i] = (uint32_t)__shfl_down((int)b.v[i], d, 64); oc.v[i] = (uint32_t)__shfl_down((int)c.v[i], d, 64); }
            a = a + oa; b = b + ob; c = c + oc;
        }
        decide = lane == 0; file = row.w;
    } else {
        const uint32_t s = t - nlong * 63u;         // = nlong + (t - 64 nlong)
        if (s < nCons) {
            const uint4 row = rows[s]; uint32_t j = 0;
            for (; j < row.x; j++) { const uint32_t idx = jdptr[j] + s; a = a + mv_term(val, w, wm, idx, col[idx]); }
            for (; j < row.y; j++) { const uint32_t idx = jdptr[j] + s; b = b + mv_term(val, w, wm, idx, col[idx]); }
            for (; j < row.z; j++) { const uint32_t idx = jdptr[j] + s; c = c + mv_term(val, w, wm, idx, col[idx]); }
            decide = true; file = row.w;
        }
    }
    bool bad = false;
    if (decide) bad = a * b != c;
    const unsigned long long m = __ballot(bad);     // every lane of the wave is here: nothing above returns past the flag test
    if (m == 0) return;
    uint32_t lo = bad ? file : 0xffffffffu;
    for (int d = 32; d > 0; d >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
    if (lane == 0) { atomicMin(first + blockIdx.y, lo); atomicAdd(count + blockIdx.y, (uint32_t)__popcll(m)); }
}

}  // namespace zkc

struct zkc_r1cs {
    zkc_ctx* ctx = nullptr;
    uint32_t nWires = 0, nPub = 0, nCons = 0, nlong = 0;
    uint64_t nTerms = 0, nUnit = 0;
    uint4* d_rows = nullptr; uint32_t* d_jdptr = nullptr; uint32_t* d_col = nullptr; Fr* d_val = nullptr;
    // work space of the checks, made on first use and kept: a chunk of uploaded witnesses (host-pointer form only), their Montgomery forms (when the system has unit
    // coefficients), the verdict words of a whole call
    void* d_w = nullptr; size_t w_sz = 0; void* d_wm = nullptr; size_t wm_sz = 0; void* d_verdict = nullptr; size_t verdict_sz = 0;
};

namespace {
constexpr size_t CHUNK_BYTES = (size_t)128 << 20;      // witnesses of one chunk (and as much again for their Montgomery forms)
constexpr size_t CHUNK_MAX = 16384;                    // and at most this many: the witness is the grid's y

struct Events {                                        // timing events of one call, destroyed with it
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

int check_batch(zkc_r1cs* cs, const void* wtns, bool on_device, int B, int64_t* first_bad, uint32_t* n_bad) {
    zkc_ctx* ctx = cs->ctx;
    ctx->r1cs_ms[0] = ctx->r1cs_ms[1] = ctx->r1cs_ms[2] = 0;
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t nW = cs->nWires, wbytes = nW * sizeof(Fr), nB = (size_t)B;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>({nB, CHUNK_MAX, CHUNK_BYTES / wbytes}));
    const bool units = cs->nUnit > 0;
    int rc;
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));            // zkc_ensure may free a buffer the stream still reads
    if (!on_device && (rc = zkc_ensure(ctx, &cs->d_w, &cs->w_sz, chunk * wbytes))) return rc;
    if (units && (rc = zkc_ensure(ctx, &cs->d_wm, &cs->wm_sz, chunk * wbytes))) return rc;
    if ((rc = zkc_ensure(ctx, &cs->d_verdict, &cs->verdict_sz, 3 * nB * sizeof(uint32_t)))) return rc;
    uint32_t *d_first = (uint32_t*)cs->d_verdict, *d_count = d_first + nB, *d_flag = d_count + nB;
    const size_t nchunks = (nB + chunk - 1) / chunk;
    Events tev; tev.ev.assign(3 * nchunks, nullptr);
    for (hipEvent_t& e : tev.ev) ZKC_HIP_CHECK(ctx, hipEventCreate(&e));
    hipStream_t st = ctx->stream;
    ZKC_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)d_first, (int)0xffffffffu, nB, st));
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, 2 * nB * sizeof(uint32_t), st));
    const unsigned gx_rows = (unsigned)(((uint64_t)cs->nCons + 63ull * cs->nlong + 255) / 256), gx_wires = (unsigned)((nW + 255) / 256);
    for (size_t k = 0; k < nchunks; k++) {
        const size_t b0 = k * chunk, nb = std::min(chunk, nB - b0);
        const Fr* d_w = on_device ? (const Fr*)wtns + b0 * nW : (const Fr*)cs->d_w;
        ZKC_HIP_CHECK(ctx, hipEventRecord(tev.ev[3 * k], st));
        if (!on_device) ZKC_HIP_CHECK(ctx, hipMemcpyAsync(cs->d_w, (const uint8_t*)wtns + b0 * wbytes, nb * wbytes, hipMemcpyHostToDevice, st));
        ZKC_HIP_CHECK(ctx, hipEventRecord(tev.ev[3 * k + 1], st));
        hipLaunchKernelGGL(zkc_r1cs_range, dim3(gx_wires, (unsigned)nb), dim3(256), 0, st, d_w, nW, (uint32_t)nW, d_flag + b0);
        if (cs->nCons) {
            if (units) hipLaunchKernelGGL(zkc_wtns_mont, dim3(gx_wires, (unsigned)nb), dim3(256), 0, st, d_w, nW, (Fr*)cs->d_wm, nW, (uint32_t)nW);
            hipLaunchKernelGGL(zkc_r1cs_check_rows, dim3(gx_rows, (unsigned)nb), dim3(256), 0, st, cs->d_rows, cs->d_jdptr, cs->d_col, cs->d_val, d_w, nW,
                               units ? (const Fr*)cs->d_wm : (const Fr*)nullptr, nW, cs->nCons, cs->nlong, d_first + b0, d_count + b0, d_flag + b0);
        }
        ZKC_HIP_CHECK(ctx, hipGetLastError());
        ZKC_HIP_CHECK(ctx, hipEventRecord(tev.ev[3 * k + 2], st));
    }
    std::vector<uint32_t> v(3 * nB);
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(v.data(), cs->d_verdict, v.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const clk::time_point t0 = clk::now();
    for (size_t i = 0; i < nB; i++) {
        const uint32_t first = v[i], count = v[nB + i], flag = v[2 * nB + i];
        const bool neg = flag != 0;
        first_bad[i] = (flag & 2u) ? ZKC_R1CS_NOT_ONE : (flag & 1u) ? ZKC_R1CS_WIRE_RANGE : first == 0xffffffffu ? ZKC_R1CS_SATISFIED : (int64_t)first;
        if (n_bad) n_bad[i] = neg ? 0 : count;
    }
    double up = 0, kern = 0;
    for (size_t k = 0; k < nchunks; k++) {
        float x = 0, y = 0;
        ZKC_HIP_CHECK(ctx, hipEventElapsedTime(&x, tev.ev[3 * k], tev.ev[3 * k + 1]));
        ZKC_HIP_CHECK(ctx, hipEventElapsedTime(&y, tev.ev[3 * k + 1], tev.ev[3 * k + 2]));
        up += x; kern += y;
    }
    ctx->r1cs_ms[0] = ms_since(t0); ctx->r1cs_ms[1] = up; ctx->r1cs_ms[2] = kern;
    return ZKC_OK;
}
}  // namespace

extern "C" int zkc_r1cs_header_info(const void* r1cs, size_t len, uint32_t* nWires, uint32_t* nPublic, uint32_t* nConstraints) {
    if (!r1cs) return zkc_fail(nullptr, ZKC_ERR_BAD_ARG, "zkc_r1cs_header_info: bad argument");
    parse::R1csHeader h; std::string perr;
    if (!parse::r1cs_header((const uint8_t*)r1cs, len, h, nullptr, nullptr, perr)) return zkc_fail(nullptr, ZKC_ERR_FORMAT, perr);
    if (nWires) *nWires = h.nWires; if (nPublic) *nPublic = h.nPub; if (nConstraints) *nConstraints = h.nCons;
    return ZKC_OK;
}

extern "C" void zkc_r1cs_free(zkc_r1cs* cs) {
    if (!cs) return;
    {
        ZKC_LOCK(cs->ctx);
        (void)hipSetDevice(cs->ctx->device);
        (void)hipStreamSynchronize(cs->ctx->stream);
        void* all[] = {cs->d_rows, cs->d_jdptr, cs->d_col, cs->d_val, cs->d_w, cs->d_wm, cs->d_verdict};
        for (void* p : all) if (p) (void)hipFree(p);
    }
    delete cs;
}

extern "C" int zkc_r1cs_load(zkc_ctx* ctx, const void* r1cs, size_t len, zkc_r1cs** out) {
    if (!ctx || !r1cs || !out) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_r1cs_load: bad argument");
    ZKC_LOCK(ctx);
    ctx->r1cs_ms[0] = ctx->r1cs_ms[1] = ctx->r1cs_ms[2] = 0;
    const clk::time_point t0 = clk::now();
    parse::R1cs P; std::string perr;
    if (!parse::r1cs_parse((const uint8_t*)r1cs, len, P, perr)) return zkc_fail(ctx, ZKC_ERR_FORMAT, perr);
    const uint32_t nCons = P.h.nCons;
    const uint64_t nTerms = P.terms[0].size() + P.terms[1].size() + P.terms[2].size();
    if (P.h.nWires >= (1u << 30) || nCons >= (1u << 31)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_r1cs_load: more than 2^30 - 1 wires or 2^31 - 1 constraints");
    if (nTerms >= (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_r1cs_load: more than 2^32 - 1 coefficients");
    // merged rows, longest first; jagged-diagonal slots (zkc_jds.h)
    auto len_of = [&](uint32_t k, int m) { return (uint32_t)(P.ptr[m][(size_t)k + 1] - P.ptr[m][k]); };
    const JdsLayout J = jds_layout(nCons, [&](uint32_t k) { return len_of(k, 0) + len_of(k, 1) + len_of(k, 2); }, R1CS_LONG);
    const uint32_t nlong = J.nlong; const std::vector<uint32_t>& jdptr = J.jdptr;
    std::vector<uint4> rows(nCons);
    for (uint32_t s = 0; s < nCons; s++) {
        const uint32_t k = J.perm[s], la = len_of(k, 0), lb = len_of(k, 1), lc = len_of(k, 2);
        rows[s] = make_uint4(la, la + lb, la + lb + lc, k);
    }
    if ((uint64_t)nCons + 63ull * nlong + 255 >= (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_r1cs_load: too many long constraints");
    std::vector<uint32_t> jcol((size_t)nTerms + 1, 0); std::vector<Fr> jval((size_t)nTerms + 1, Fr::zero());
    Fr r2, one_r2, neg_r2; for (int i = 0; i < 8; i++) r2.v[i] = FrParams::r2[i];
    one_r2 = r2; neg_r2 = Fr::zero() - one_r2;
    const uint64_t nUnit = jds_fill(J, [&](uint32_t k, uint32_t j) {      // term j of merged row k: A's terms, then B's, then C's
        int m = 0; while (j >= len_of(k, m)) j -= len_of(k, m++);
        const parse::R1csTerm& T = P.terms[m][(size_t)(P.ptr[m][k] + j)];
        uint32_t sv[8]; memcpy(sv, T.coef, 32);
        return std::pair<uint32_t, Fr>(T.wire, fp_from_std<FrParams>(sv) * r2);        // val R^2: a coefficient >= r enters as its residue
    }, one_r2, neg_r2, jcol.data(), jval.data());
    const double host_ms = ms_since(t0);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    zkc_r1cs* cs = new zkc_r1cs(); cs->ctx = ctx;
    cs->nWires = P.h.nWires; cs->nPub = P.h.nPub; cs->nCons = nCons; cs->nlong = nlong; cs->nTerms = nTerms; cs->nUnit = nUnit;
    const clk::time_point t1 = clk::now();
    auto up = [&](void** d, const void* h, size_t bytes) {
        hipError_t e = hipMalloc(d, std::max<size_t>(bytes, 16));
        if (e == hipSuccess && bytes) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e;
    if ((e = up((void**)&cs->d_rows, rows.data(), rows.size() * sizeof(uint4))) != hipSuccess || (e = up((void**)&cs->d_jdptr, jdptr.data(), jdptr.size() * 4)) != hipSuccess ||
        (e = up((void**)&cs->d_col, jcol.data(), jcol.size() * 4)) != hipSuccess || (e = up((void**)&cs->d_val, jval.data(), jval.size() * sizeof(Fr))) != hipSuccess) {
        zkc_r1cs_free(cs);
        return zkc_fail(ctx, ZKC_ERR_HIP, std::string("zkc_r1cs_load: ") + hipGetErrorString(e));
    }
    ctx->r1cs_ms[0] = host_ms; ctx->r1cs_ms[1] = ms_since(t1);
    *out = cs;
    return ZKC_OK;
}

extern "C" int zkc_r1cs_info(const zkc_r1cs* cs, uint32_t* nWires, uint32_t* nPublic, uint32_t* nConstraints) {
    if (!cs) return ZKC_ERR_BAD_ARG;
    if (nWires) *nWires = cs->nWires; if (nPublic) *nPublic = cs->nPub; if (nConstraints) *nConstraints = cs->nCons;
    return ZKC_OK;
}

static int check_args(zkc_r1cs* cs, const void* wtns, uint32_t nWitness, int B, int64_t* first_bad, const char* who) {
    if (!wtns || !first_bad || B <= 0) return zkc_fail(cs->ctx, ZKC_ERR_BAD_ARG, std::string(who) + ": bad argument");
    if (nWitness != cs->nWires)
        return zkc_fail(cs->ctx, ZKC_ERR_BAD_ARG, std::string(who) + ": the witnesses have " + std::to_string(nWitness) + " wires, the constraint system " + std::to_string(cs->nWires));
    return ZKC_OK;
}
extern "C" int zkc_r1cs_check(zkc_r1cs* cs, const void* wtns, uint32_t nWitness, int B, int64_t* first_bad, uint32_t* n_bad) {
    if (!cs) return ZKC_ERR_BAD_ARG;
    ZKC_LOCK(cs->ctx);
    const int rc = check_args(cs, wtns, nWitness, B, first_bad, "zkc_r1cs_check");
    return rc ? rc : check_batch(cs, wtns, false, B, first_bad, n_bad);
}
extern "C" int zkc_r1cs_check_dev(zkc_r1cs* cs, const void* d_wtns, uint32_t nWitness, int B, int64_t* first_bad, uint32_t* n_bad) {
    if (!cs) return ZKC_ERR_BAD_ARG;
    ZKC_LOCK(cs->ctx);
    const int rc = check_args(cs, d_wtns, nWitness, B, first_bad, "zkc_r1cs_check_dev");
    return rc ? rc : check_batch(cs, d_wtns, true, B, first_bad, n_bad);
}

extern "C" int zkc_r1cs_check_stats(zkc_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_r1cs_check_stats: bad argument");
    ZKC_LOCK(ctx);
    for (int k = 0; k < 3; k++) ms[k] = ctx->r1cs_ms[k];
    return ZKC_OK;
}
