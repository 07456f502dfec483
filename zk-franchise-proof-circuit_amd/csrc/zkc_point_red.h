// zkc_point_red.h -- partial sums of points to one sum per row, for the kernels that leave one XYZZ partial sum per segment of a row (zkc_setup_ptau.hip: the rows of a
// sparse matrix times a vector of points; zkc_ptau_verify.hip: the two weighted sums of a chunk of a section).  One kernel, instantiated with G1Ops / G2Ops
// (zkc_point_ops.h), the host's plan of its steps and the loop that launches them.  Needs hipcc.  Product code.
#pragma once
#include <algorithm>
#include <vector>
#include "zkc_internal.h"
#include "zkc_point_ops.h"

namespace zkc {

constexpr uint32_t POINT_RED = 32;               // partial sums per lane of a reduction step

// ---- reduce: out[j] = sum of in[job_start[j] .. job_start[j + 1]) (at most POINT_RED of them; none: infinity), complete additions ----
template <class G> __global__ void __launch_bounds__(64)
zkc_ptau_red(const XYZZ<typename G::F>* __restrict__ in, const uint32_t* __restrict__ job_start, uint32_t njobs, XYZZ<typename G::F>* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const uint32_t a = job_start[j]; uint32_t b = job_start[j + 1];
    if (b - a > POINT_RED) b = a + POINT_RED;
    if (a == b) { out[j] = XYZZ<typename G::F>::inf(); return; }
    if (b - a == 1) { out[j] = in[a]; return; }
    typename G::Acc acc = G::from_xyzz(in[a]);
    for (uint32_t i = a + 1; i < b; i++) { const typename G::Acc o = G::from_xyzz(in[i]); typename G::Acc r; G::add(r, acc, o); acc = r; }
    out[j] = G::is_inf(acc) ? XYZZ<typename G::F>::inf() : G::leave(acc);
}

// the reduction steps of rows that hold cnt[p] partial sums each, back to back: step i sums, per job j, the partial sums [start[j], start[j + 1]) of step i - 1's
// output; the last step has one job per row
inline std::vector<std::vector<uint32_t>> reduction_steps(std::vector<uint32_t> cnt) {
    std::vector<std::vector<uint32_t>> steps;
    const size_t nrows = cnt.size();
    for (;;) {
        const uint32_t maxc = nrows ? *std::max_element(cnt.begin(), cnt.end()) : 0;
        std::vector<uint32_t> start; start.push_back(0);
        if (maxc <= POINT_RED) { for (size_t p = 0; p < nrows; p++) start.push_back(start.back() + cnt[p]); steps.push_back(std::move(start)); return steps; }
        for (size_t p = 0; p < nrows; p++) {
            for (uint32_t c = 0; c < cnt[p]; c += POINT_RED) start.push_back(start.back() + std::min(POINT_RED, cnt[p] - c));
            cnt[p] = (cnt[p] + POINT_RED - 1) / POINT_RED;
        }
        steps.push_back(std::move(start));
    }
}

// cur (the partial sums of every row, cnt[p] of row p, back to back) -> cur = one sum per row, through the steps above on ctx->stream.  The context's lock is held
// and the device is set; has synchronised on return.
template <class F>
int point_reduce(zkc_ctx* ctx, DevBuf& cur, const std::vector<uint32_t>& cnt) {
    typedef typename GroupOf<F>::Ops G;
    int rc;
    for (const std::vector<uint32_t>& start : reduction_steps(cnt)) {
        const uint32_t njobs = (uint32_t)start.size() - 1;
        DevBuf st, nxt;
        if ((rc = st.alloc(ctx, start.size() * 4)) || (rc = nxt.alloc(ctx, (size_t)njobs * sizeof(XYZZ<F>)))) return rc;
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(st.p, start.data(), start.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (njobs) {
            hipLaunchKernelGGL(zkc_ptau_red<G>, dim3((njobs + 63) / 64), dim3(64), 0, ctx->stream, cur.as<XYZZ<F>>(), st.as<uint32_t>(), njobs, nxt.as<XYZZ<F>>());
            ZKC_HIP_CHECK(ctx, hipGetLastError());
        }
        ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));                                                  // `start` and `st` end with this turn of the loop
        (void)hipFree(cur.p); cur.p = nxt.release();
    }
    return ZKC_OK;
}

}  // namespace zkc
