// Sumcheck prover rounds over 5..8 MLEs (CCS with 4..7 matrices: the plain Plonk gate is t = 6, seven tables with eq()).
//
// Reference loops replaced: the same as kernels_sumcheck.cuh (IPForMLSumcheck::prove_round, src/sumcheck/prover.rs:62-180,
// with the fold of DenseMultilinearExtension::fix_variables, src/poly_f/mle/dense.rs:142-168, fused in).
//
// The one-thread-per-point kernel does not stretch this far: sumcheck_round_kernel<4, 4, 3> is at 210 VGPRs already, and
// eight MLEs with five lazy accumulators would spill.  This is sumcheck_round_quad_kernel with EIGHT lanes per hypercube
// point instead of four: lane e of the group keeps the K values at t = e (v0, v1, v1 + (e - 1)(v1 - v0): the same canonical
// residues as the reference's running sum, prover.rs:128-150) and ONE lazy accumulator; the lanes e > degree compute a
// value nobody reads.  In a folding round lane k < K folds MLE k and the group shares the folded pairs through
// ds_swizzle (the LDS crossbar, no LDS memory: gfx9 DPP has no broadcast wider than a quad), so no fold multiplication is
// done twice; the first round has no fold and every lane reads all pairs (one cache line, one request per group).
// K is a template parameter (the folded pairs live in registers and lane numbers are immediates); the degree and the
// lane's e are run-time values, applied with lane predicates and wave-uniform branches: twelve instances (FL = 2, 3, 4 x
// K = 5..8) instead of forty-eight.  A lane does NOT keep all K values of its point: with eight of them next to the
// accumulator <4, 8> needed 130 VGPRs.  It keeps the pair IT folded (p0, p1) and fetches the value of MLE k where the
// combination function multiplies by it -- a ds_swizzle and at most four modular additions, against the multiplication
// that follows; an MLE that two terms share is fetched twice (no CCS whose S lists 0..t-1 in order has one).
// Same partials layout, last-block fold and sumcheck_reduce_kernel as the kernels for K <= 4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "kernels_sumcheck.cuh"

namespace zipk {

constexpr int kSumcheckWideLanes = 8;  // lanes per hypercube point: the evaluation points 0..7, of which 0..degree count

// lane SRC of every group of eight: bit-mask mode, lane' = (lane & 0x18) | SRC inside each half wave
template <int SRC>
__device__ __forceinline__ uint64_t group8_bcast(uint64_t x) {
    constexpr int PATTERN = 0x18 | (SRC << 5);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)x, PATTERN);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(x >> 32), PATTERN);
    return ((uint64_t)hi << 32) | lo;
}

// sumcheck_comb (kernels_sumcheck.cuh) with the values fetched where they are used: value(k_tag, out) gives the value of
// MLE k at this lane's point
template <int FL, int K, class V>
__device__ __forceinline__ void sumcheck_comb_fetch(const SumcheckRoundArgs<FL> &a, const FieldDev<FL> &f, V &&value,
                                                    uint64_t (&c)[FL]) {
    if (a.n_terms == 0) {
        value(std::integral_constant<int, 0>{}, c);
        sc_static_for<1, K - 2>([&](auto k_tag) {
            uint64_t v[FL], t[FL];
            value(k_tag, v);
            mont_mul<FL>(c, v, f, t);
#pragma unroll
            for (int i = 0; i < FL; i++) c[i] = t[i];
        });
    } else {
#pragma unroll
        for (int i = 0; i < FL; i++) c[i] = 0;
        for (uint32_t tt = 0; tt < a.n_terms; tt++) {
            uint64_t term[FL];
            const uint32_t kind = a.coeff_kind[tt];  // wave-uniform
            bool have = kind == 0;
            if (have) {
#pragma unroll
                for (int i = 0; i < FL; i++) term[i] = a.coeff[tt][i];
            }
            const uint32_t m = a.term_mask[tt];
            sc_static_for<0, K - 1>([&](auto k_tag) {
                constexpr int k = decltype(k_tag)::value;
                if ((m >> k) & 1u) {  // wave-uniform
                    if (have) {
                        uint64_t v[FL], t[FL];
                        value(k_tag, v);
                        mont_mul<FL>(term, v, f, t);
#pragma unroll
                        for (int i = 0; i < FL; i++) term[i] = t[i];
                    } else {
                        value(k_tag, term);
                        have = true;
                    }
                }
            });
            if (!have) {
#pragma unroll
                for (int i = 0; i < FL; i++) term[i] = a.one[i];
            }
            if (kind == 2) fe_sub<FL>(c, term, f);
            else fe_add<FL>(c, term, f);
        }
    }
}

template <int FL, int K>
__global__ void __launch_bounds__(256, 4) sumcheck_round_wide_kernel(SumcheckRoundArgs<FL> a, FieldDev<FL> f) {
    static_assert(K > 4 && K <= kSumcheckWideLanes && K <= kSumcheckMaxMles, "lane k of a group folds MLE k");
    static_assert(kSumcheckMaxDegree < kSumcheckWideLanes, "a group holds the points 0..degree");
    extern __shared__ __align__(16) unsigned char sc_smem[];
    uint64_t *red = reinterpret_cast<uint64_t *>(sc_smem);  // [256][FL]
    const uint32_t tid = threadIdx.x, e = tid & 7u, ne = a.degree + 1;
    uint64_t wacc[2 * FL + 1];
#pragma unroll
    for (int i = 0; i <= 2 * FL; i++) wacc[i] = 0;
    uint64_t rr[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) rr[i] = a.r[i];
    const bool is0 = e == 0u, ge2 = e >= 2u, ge3 = e >= 3u, ge4 = e >= 4u;  // lane predicates: no vector registers
    const bool deg3 = a.degree >= 3, deg4 = a.degree >= 4;  // wave-uniform
    // the MLE this lane folds (lane k of a group: MLE k)
    const uint64_t *my_src = a.src[0];
    uint64_t *my_dst = a.dst[0];
#pragma unroll
    for (int k = 1; k < K; k++) {
        if (e == (uint32_t)k) {
            my_src = a.src[k];
            my_dst = a.dst[k];
        }
    }
    // the value at this lane's point from the entries at t = 0 and t = 1 (lanes above the degree stop at the last point)
    auto at_point = [&](const uint64_t (&v0)[FL], const uint64_t (&v1)[FL], uint64_t (&out)[FL]) {
        uint64_t step[FL], s[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) {
            step[i] = v1[i];
            out[i] = is0 ? v0[i] : v1[i];
        }
        fe_sub<FL>(step, v0, f);
#pragma unroll
        for (int i = 0; i < FL; i++) s[i] = ge2 ? step[i] : 0;  // (adding 0 leaves a canonical residue as it is)
        fe_add<FL>(out, s, f);
        if (deg3) {
#pragma unroll
            for (int i = 0; i < FL; i++) s[i] = ge3 ? step[i] : 0;
            fe_add<FL>(out, s, f);
        }
        if (deg4) {
#pragma unroll
            for (int i = 0; i < FL; i++) s[i] = ge4 ? step[i] : 0;
            fe_add<FL>(out, s, f);
        }
    };
    const uint64_t per_pass = (uint64_t)gridDim.x * 32u;
    for (uint64_t b = (uint64_t)blockIdx.x * 32u + (tid >> 3); b < a.half; b += per_pass) {  // (uniform in a group)
        uint64_t p0[FL], p1[FL];  // a folding round: the pair this lane folded
#pragma unroll
        for (int i = 0; i < FL; i++) p0[i] = p1[i] = 0;
        if (a.fold && e < (uint32_t)K) {  // p'[j] = p[2j] + r (p[2j+1] - p[2j])
            uint64_t d[FL], t[FL];
            const uint64_t *s = my_src + (size_t)(4 * b) * FL;
            fe_load<FL>(p0, s);
            fe_load<FL>(d, s + FL);
            fe_sub<FL>(d, p0, f);
            mont_mul<FL>(d, rr, f, t);
            fe_add<FL>(p0, t, f);
            fe_load<FL>(p1, s + 2 * FL);
            fe_load<FL>(d, s + 3 * FL);
            fe_sub<FL>(d, p1, f);
            mont_mul<FL>(d, rr, f, t);
            fe_add<FL>(p1, t, f);
            fe_store<FL>(my_dst + (size_t)(2 * b) * FL, p0);
            fe_store<FL>(my_dst + (size_t)(2 * b + 1) * FL, p1);
        }
        // MLE k at this lane's point: from the group's lane k, or (first round) from the table -- the lanes of a group
        // read the same entries: one cache line, one request
        auto value = [&](auto k_tag, uint64_t (&out)[FL]) {
            constexpr int k = decltype(k_tag)::value;
            uint64_t v0[FL], v1[FL];
            if (a.fold) {
#pragma unroll
                for (int i = 0; i < FL; i++) {
                    v0[i] = group8_bcast<k>(p0[i]);
                    v1[i] = group8_bcast<k>(p1[i]);
                }
            } else {
                const uint64_t *s = a.src[k] + (size_t)(2 * b) * FL;
                fe_load<FL>(v0, s);
                fe_load<FL>(v1, s + FL);
            }
            at_point(v0, v1, out);
        };
        uint64_t c[FL], last[FL], w[2 * FL];
        sumcheck_comb_fetch<FL, K>(a, f, value, c);
        value(std::integral_constant<int, K - 1>{}, last);
        mul_wide<FL>(c, last, w);
        acc_wide_add<FL>(wacc, w);
    }
    uint64_t acc[FL];
    acc_wide_reduce<FL>(wacc, f, acc);
    fe_store<FL>(red + (size_t)tid * FL, acc);
    __syncthreads();
    for (uint32_t s = 128; s >= 8; s >>= 1) {  // lanes with the same point: tid mod 8 survives every halving
        if (tid < s) {
            uint64_t p[FL], q[FL];
            fe_load<FL>(p, red + (size_t)tid * FL);
            fe_load<FL>(q, red + (size_t)(tid + s) * FL);
            fe_add<FL>(p, q, f);
            fe_store<FL>(red + (size_t)tid * FL, p);
        }
        __syncthreads();
    }
    if (tid < ne * FL) a.partials[(size_t)blockIdx.x * ne * FL + tid] = red[tid];  // red[e][FL], e = 0..degree
    sumcheck_last_block_folds<FL>(a, f, red, ne, tid);
}

}  // namespace zipk
