// Sumcheck prover rounds for a SUM OF PRODUCTS over up to 32 MLEs in one pass per round:
//   comb_fn(vals) = sum_p coeff[p] * prod_{j in S_p} vals[j]        (no trailing factor)
// the polynomial of rand_poly / rand_poly_comb_fn (src/sumcheck/utils.rs:27-78), which the reference's own sumcheck
// benchmark and tests prove (benches/sumcheck_benches.rs, src/sumcheck/tests.rs): 7 products of 2..4 multiplicands.
//
// Reference loops replaced: the same as kernels_sumcheck.cuh (IPForMLSumcheck::prove_round, src/sumcheck/prover.rs:62-180,
// with the fold of DenseMultilinearExtension::fix_variables, src/poly_f/mle/dense.rs:142-168, fused in).
//
// Work layout: EIGHT lanes per hypercube point b, as in sumcheck_round_wide_kernel, and the group walks the products.
//   * evaluation: lane e of the group keeps ONE lazy accumulator for the point t = e (the lanes e > degree compute a
//     value nobody reads) and multiplies its way through every product: coefficient and factors by mont_mul, the last
//     factor by the unreduced mul_wide into the accumulator.  One accumulator serves all products of the point.
//   * fold: a product has at most four factors with two folded entries each, eight values: lane (j, h) = (e & 3, e >> 2)
//     of the group computes entry 2b + h of factor j's folded table -- ONE fold multiplication per lane and product --
//     and the group shares the eight values through ds_swizzle (group8_bcast).  In the first round the same lane loads
//     entry 2b + h instead.
//   * ownership: the folded table of an MLE is written once per round, by the lowest-numbered product that contains it
//     (own[p], computed by the host).  A product that shares the MLE folds its pair again FROM THE ROUND'S INPUT: the
//     folded output is never read in the round that writes it.
// A thread per hypercube point was the alternative: sumcheck_round_kernel<4, 4, 3> needs 210 VGPRs for four pairs and
// four accumulators and is bound by the latency of its dependent multiply chains at two waves per SIMD
// (kernels_sumcheck.cuh); five accumulators for degree 4 would push it further.  Here a lane holds one accumulator, one
// folded value and one running term.
// Factor lists, ownership, coefficient kinds and table pointers are wave-uniform run-time values read from the kernel
// arguments (scalar loads): one instance per limb count.
// Same partials layout, last-block fold and sumcheck_reduce_kernel as the other round kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "kernels_sumcheck_wide.cuh"

namespace zipk {

constexpr int kSumcheckProductsMaxMles = 32;
constexpr int kSumcheckProductsMaxFactors = 4;  // per product: the eight lanes of a group hold 4 folded pairs

template <int FL>
struct SumcheckProductsArgs {
    const uint64_t *src[kSumcheckProductsMaxMles];  // tables of this round's input (2*half entries, or 4*half when fold)
    uint64_t *dst[kSumcheckProductsMaxMles];        // folded tables (2*half entries) when fold; null for an unused MLE
    uint64_t r[FL];                                 // previous round's challenge (Montgomery), when fold
    uint32_t degree, fold;
    uint64_t half;                                  // number of hypercube points b of this round: 2^(nv - round)
    uint64_t *partials;                             // [gridDim.x][degree + 1][FL]
    uint32_t *done;                                 // as SumcheckRoundArgs::done
    uint64_t *evals_out;                            // [degree + 1][FL], device memory or host-mapped pinned memory
    uint32_t *host_flag;                            // host-mapped word set to `seq` after the message, or null
    uint32_t seq;
    uint32_t n_products;                            // 1..8
    uint32_t n_factors[kSumcheckMaxTerms];          // 1..4
    uint32_t factors[kSumcheckMaxTerms];            // byte j: the MLE that is factor j (bytes at and above n_factors
                                                    // repeat factor 0: a valid table, never read)
    uint32_t own[kSumcheckMaxTerms];                // bit j: this product writes the folded table of its factor j
    uint64_t coeff[kSumcheckMaxTerms][FL];
    // 0 = general (the coefficient is the first multiplicand), 1 = one, 2 = minus one: no multiplication.  The host
    // sets 1 / 2 only for products of two or more factors (a single factor times 1 is `general` with coeff = R).
    uint32_t coeff_kind[kSumcheckMaxTerms];
};

template <int FL>
__global__ void __launch_bounds__(256, 4) sumcheck_round_products_kernel(SumcheckProductsArgs<FL> a, FieldDev<FL> f) {
    static_assert(2 * kSumcheckProductsMaxFactors == kSumcheckWideLanes, "lane (j, h) of a group folds entry h of factor j");
    static_assert(kSumcheckMaxDegree < kSumcheckWideLanes, "a group holds the points 0..degree");
    extern __shared__ __align__(16) unsigned char sc_smem[];
    uint64_t *red = reinterpret_cast<uint64_t *>(sc_smem);  // [256][FL]
    const uint32_t tid = threadIdx.x, e = tid & 7u, ne = a.degree + 1;
    const uint32_t fj = e & 3u, fh = e >> 2;  // the factor and the entry of its pair this lane loads / folds
    uint64_t wacc[2 * FL + 1];
#pragma unroll
    for (int i = 0; i <= 2 * FL; i++) wacc[i] = 0;
    uint64_t rr[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) rr[i] = a.r[i];
    const bool is0 = e == 0u, ge2 = e >= 2u, ge3 = e >= 3u, ge4 = e >= 4u;  // lane predicates: no vector registers
    const bool deg3 = a.degree >= 3, deg4 = a.degree >= 4;                  // wave-uniform
    // the value at this lane's point from the entries at t = 0 and t = 1 (as in sumcheck_round_wide_kernel)
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
        for (uint32_t p = 0; p < a.n_products; p++) {  // everything read from `a` in here is wave-uniform
            const uint32_t nf = a.n_factors[p], fidx = a.factors[p], kind = a.coeff_kind[p];
            // the table this lane loads from: factor fj of the product
            const uint64_t *my_src = a.src[fidx & 0xffu];
            uint64_t *my_dst = a.dst[fidx & 0xffu];
#pragma unroll
            for (int j = 1; j < kSumcheckProductsMaxFactors; j++) {
                const uint32_t k = (fidx >> (8 * j)) & 0xffu;
                const uint64_t *sj = a.src[k];
                uint64_t *dj = a.dst[k];
                if (fj == (uint32_t)j) {
                    my_src = sj;
                    my_dst = dj;
                }
            }
            uint64_t pv[FL];  // entry 2b + fh of factor fj's table AFTER the fold with the previous challenge
#pragma unroll
            for (int i = 0; i < FL; i++) pv[i] = 0;
            if (fj < nf) {
                if (a.fold) {  // p'[2b + h] = p[4b + 2h] + r (p[4b + 2h + 1] - p[4b + 2h])
                    uint64_t d[FL], t[FL];
                    const uint64_t *s = my_src + (size_t)(4 * b + 2 * fh) * FL;
                    fe_load<FL>(pv, s);
                    fe_load<FL>(d, s + FL);
                    fe_sub<FL>(d, pv, f);
                    mont_mul<FL>(d, rr, f, t);
                    fe_add<FL>(pv, t, f);
                    if ((a.own[p] >> fj) & 1u) fe_store<FL>(my_dst + (size_t)(2 * b + fh) * FL, pv);
                } else {
                    fe_load<FL>(pv, my_src + (size_t)(2 * b + fh) * FL);
                }
            }
            uint64_t term[FL], last[FL];
            bool have = kind == 0;  // wave-uniform
#pragma unroll
            for (int i = 0; i < FL; i++) {
                term[i] = a.coeff[p][i];
                last[i] = 0;
            }
            sc_static_for<0, kSumcheckProductsMaxFactors - 1>([&](auto j_tag) {
                constexpr int j = decltype(j_tag)::value;
                if ((uint32_t)j < nf) {  // wave-uniform
                    uint64_t v0[FL], v1[FL], val[FL];
#pragma unroll
                    for (int i = 0; i < FL; i++) {
                        v0[i] = group8_bcast<j>(pv[i]);
                        v1[i] = group8_bcast<j + 4>(pv[i]);
                    }
                    at_point(v0, v1, val);
                    if ((uint32_t)j + 1 < nf) {
                        if (have) {
                            uint64_t t[FL];
                            mont_mul<FL>(term, val, f, t);
#pragma unroll
                            for (int i = 0; i < FL; i++) term[i] = t[i];
                        } else {
#pragma unroll
                            for (int i = 0; i < FL; i++) term[i] = val[i];
                            have = true;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < FL; i++) last[i] = val[i];
                    }
                }
            });
            if (kind == 2) {  // coefficient -1: negate the running term (nf >= 2: there is one)
                uint64_t z[FL];
#pragma unroll
                for (int i = 0; i < FL; i++) z[i] = 0;
                fe_sub<FL>(z, term, f);
#pragma unroll
                for (int i = 0; i < FL; i++) term[i] = z[i];
            }
            uint64_t w[2 * FL];
            mul_wide<FL>(term, last, w);
            acc_wide_add<FL>(wacc, w);
        }
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
    // the shared last-block fold reads five fields of the other kernels' argument struct
    SumcheckRoundArgs<FL> la{};
    la.partials = a.partials;
    la.done = a.done;
    la.evals_out = a.evals_out;
    la.host_flag = a.host_flag;
    la.seq = a.seq;
    sumcheck_last_block_folds<FL>(la, f, red, ne, tid);
}

}  // namespace zipk
