// MANY small sumchecks in ONE launch (zip_sumcheck_prove_batch): workgroup i of 1024 threads plays EVERY round of
// instance i -- MLSumcheck::prove_as_subprotocol (src/sumcheck.rs:56-112) from the absorption of nvars and degree to the
// last challenge -- with its own tables, its own field and its own Keccak sponge.  The instances are independent, so
// the workgroups never talk to each other or to the host: no flags, no atomics, no spin loops; every loop has a trip
// count known at launch.  The serial Keccak chains of the instances run side by side on as many CUs.
//
// The last n rounds (tables of at most 2^n entries, n = the tail kernel's LDS bound cut by ZIP_HIP_SUMCHECK_TAIL) are
// the rounds of sumcheck_tail_kernel, step for step: tables in LDS, folded on the way in, in-place fold with one barrier
// per pass and table, ne_pad lanes per point, wave shuffles plus 16 wave sums, the sponge in LDS.  The rounds before
// ("streamed") are the same two steps with the tables in HBM: fold pass, __syncthreads(), evaluation pass.  Round 1
// reads the caller's tables (never written); round 2 folds them into the instance's scratch block [K][2^(nv-1)][FL];
// rounds 3.. fold that block in place with the pass scheme of the tail kernel (kernels_sumcheck_tail.cuh: pass p reads
// [2pN, 2pN + 2N), barrier, writes [pN, pN + N)).  Only this workgroup reads what it stored, and a workgroup lives on one
// CU with one vector L1: __syncthreads() (workgroup-scope release, barrier, acquire) is all the ordering there is.
// The two passes are not fused and the scratch is not double-buffered: the simplest correct form.
//
// Static LDS is that of the tail kernel (<= kTailFixedLds), so tail_lds_bound() holds for this kernel too: the
// per-instance arguments stay in device memory and are read through uniform addresses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keccak_dev.cuh"
#include "kernels_sumcheck.cuh"
#include "kernels_sumcheck_tail.cuh"

namespace zipk {

constexpr uint32_t kBatchSumcheckMaxVars = 16;

// one instance of a batch: an array of these lives in device memory, uploaded once per call
template <int FL>
struct SumcheckBatchInst {
    const uint64_t *src[kSumcheckMaxMles];  // the instance's tables, 2^num_vars entries each: read, never written
    uint64_t *scratch;                      // [n_mles][2^(num_vars - 1)][FL]; null when fewer than two rounds are streamed
    FieldDev<FL> f;
    TrField<FL> tf;
    uint32_t n_terms;  // 0: the product of all tables
    uint32_t term_mask[kSumcheckMaxTerms];
    uint64_t coeff[kSumcheckMaxTerms][FL];
    uint64_t st[25], blk[kKeccakRateWords];  // the sponge BEFORE the sumcheck (nvars and degree not yet absorbed)
    uint32_t buflen;
    // [num_vars][degree + 1][FL] messages | [num_vars][FL] challenges | 25 state words | 17 rate words | buflen
    uint64_t *out;
};

// words of SumcheckBatchInst::out
constexpr size_t sumcheck_batch_out_words(uint32_t num_vars, uint32_t degree, uint32_t fl) {
    return (size_t)num_vars * (degree + 2) * fl + 25 + kKeccakRateWords + 1;
}

// where table k of a round lives: K tables at a fixed stride (LDS, or the scratch block) ...
struct BatchTabsStrided {
    uint64_t *base;
    size_t stride;
    __device__ __forceinline__ uint64_t *operator()(uint32_t k) const { return base + k * stride; }
};
// ... or the caller's K pointers (uniform loads from the instance)
struct BatchTabsCaller {
    const uint64_t *const *src;
    __device__ __forceinline__ const uint64_t *operator()(uint32_t k) const { return src[k]; }
};

// dst[k][j] = src[k][2j] + r (src[k][2j+1] - src[k][2j]) for j < len, by N threads (fix_variables, dense.rs:142-168).
// IN_PLACE (dst == src): the pass scheme of the tail kernel, one barrier per pass and table between the reads and the
// writes.  Uniform trip counts: every thread reaches every barrier.
template <int FL, bool IN_PLACE, class Src, class Dst>
__device__ __forceinline__ void batch_fold(const Src &src, const Dst &dst, uint32_t K, uint32_t len, const uint64_t (&rr)[FL],
                                           const FieldDev<FL> &f, uint32_t tid) {
    constexpr uint32_t N = kTailThreads;
    for (uint32_t base = 0; base < len; base += N) {
        const uint32_t j = base + tid;
        for (uint32_t k = 0; k < K; k++) {  // (one table at a time, as in the tail kernel)
            uint64_t p[FL];
            if (j < len) {
                uint64_t d[FL], t[FL];
                const uint64_t *s = src(k) + (size_t)(2 * j) * FL;
                fe_load<FL>(p, s);
                fe_load<FL>(d, s + FL);
                fe_sub<FL>(d, p, f);
                mont_mul<FL>(d, rr, f, t);
                fe_add<FL>(p, t, f);
            }
            if (IN_PLACE) __syncthreads();
            if (j < len) fe_store<FL>(dst(k) + (size_t)j * FL, p);
        }
    }
}

// This lane's share of the round polynomial at t = e: the sum of the combination function over its points b < half
// (ne_pad lanes per point; the tail kernel's evaluation with the tables behind `tabs`).
template <int FL, class Tabs>
__device__ __forceinline__ void batch_eval(const Tabs &tabs, const SumcheckBatchInst<FL> &a, uint32_t K, uint32_t half, uint32_t ne,
                                           uint32_t ne_pad, uint32_t ne_shift, const FieldDev<FL> &f, uint32_t tid, uint64_t (&acc)[FL]) {
    constexpr uint32_t N = kTailThreads;
    const uint32_t e = tid & (ne_pad - 1), n_terms = a.n_terms;
#pragma unroll
    for (int i = 0; i < FL; i++) acc[i] = 0;
    auto at_point = [&](uint32_t k, uint32_t b, uint64_t (&out)[FL]) {
        const uint64_t *s = tabs(k) + (size_t)(2 * b) * FL;
        uint64_t v0[FL], step[FL];
        fe_load<FL>(v0, s);
        fe_load<FL>(out, s + FL);
        if (e == 0) {
#pragma unroll
            for (int i = 0; i < FL; i++) out[i] = v0[i];
        } else if (e > 1) {
#pragma unroll
            for (int i = 0; i < FL; i++) step[i] = out[i];
            fe_sub<FL>(step, v0, f);
            for (uint32_t t = 1; t < e; t++) fe_add<FL>(out, step, f);
        }
    };
    if (e >= ne) return;
    for (uint32_t b = tid >> ne_shift; b < half; b += N >> ne_shift) {
        uint64_t c[FL], v[FL], t[FL];
        if (n_terms == 0) {  // the product of all MLE values
            at_point(0, b, c);
            for (uint32_t k = 1; k < K; k++) {
                at_point(k, b, v);
                mont_mul<FL>(c, v, f, t);
#pragma unroll
                for (int i = 0; i < FL; i++) c[i] = t[i];
            }
        } else {  // (sum_t coeff[t] * prod_{j in term_mask[t]} v_j) * v_last   (zinc/utils.rs:77-94)
            uint64_t sum[FL];
#pragma unroll
            for (int i = 0; i < FL; i++) sum[i] = 0;
            for (uint32_t tt = 0; tt < n_terms; tt++) {
                uint64_t term[FL];
#pragma unroll
                for (int i = 0; i < FL; i++) term[i] = a.coeff[tt][i];
                const uint32_t m = a.term_mask[tt];
                for (uint32_t k = 0; k < K; k++) {
                    if ((m >> k) & 1u) {
                        at_point(k, b, v);
                        mont_mul<FL>(term, v, f, t);
#pragma unroll
                        for (int i = 0; i < FL; i++) term[i] = t[i];
                    }
                }
                fe_add<FL>(sum, term, f);
            }
            at_point(K - 1, b, v);
            mont_mul<FL>(sum, v, f, c);
        }
        fe_add<FL>(acc, c, f);
    }
}

// grid = the instances; n_lds = the rounds played from LDS (<= num_vars, <= tail_lds_bound(n_mles, FL)); dynamic LDS =
// n_mles * 2^n_lds * FL * 8 bytes (none when n_lds == 0)
template <int FL>
__global__ void __launch_bounds__(kTailThreads) sumcheck_batch_kernel(const SumcheckBatchInst<FL> *__restrict__ insts, uint32_t n_mles,
                                                                      uint32_t degree, uint32_t num_vars, uint32_t n_lds) {
    extern __shared__ __align__(16) unsigned char scb_smem[];
    uint64_t *tab = reinterpret_cast<uint64_t *>(scb_smem);  // [K][2^n_lds][FL]
    __shared__ uint64_t wred[kTailWaves][8][FL];
    __shared__ uint64_t msg[kSumcheckMaxDegree + 1][FL];
    __shared__ uint64_t r_lds[FL], mod_lds[FL];
    __shared__ uint64_t st[25], blk[kKeccakRateWords], tmp[25];
    constexpr uint32_t P = 16 * FL + 4;
    const SumcheckBatchInst<FL> &a = insts[blockIdx.x];
    const FieldDev<FL> f = a.f;
    const uint32_t tid = threadIdx.x, K = n_mles, ne = degree + 1;
    const uint32_t ne_pad = ne <= 2 ? 2u : ne <= 4 ? 4u : 8u, ne_shift = ne <= 2 ? 1u : ne <= 4 ? 2u : 3u;
    const uint32_t n_streamed = num_vars - n_lds;
    const BatchTabsStrided lds_tabs{tab, ((size_t)1 << n_lds) * FL};
    const BatchTabsStrided scr_tabs{a.scratch, ((size_t)1 << (num_vars - 1)) * FL};
    const BatchTabsCaller src_tabs{a.src};
    uint32_t buflen = a.buflen;  // every thread keeps the same copy

    if (tid < 25) st[tid] = a.st[tid];
    if (tid < (uint32_t)FL) mod_lds[tid] = a.tf.modulus[tid];
    if (tid < kKeccakRateWords) blk[tid] = a.blk[tid];
    if (tid == 0) {  // nvars and degree as field elements (sumcheck.rs:64-76)
        uint64_t v[FL];
        tr_map_u128<FL>(a.tf, num_vars, 0, v);
        fe_store<FL>(&msg[0][0], v);
        tr_map_u128<FL>(a.tf, degree, 0, v);
        fe_store<FL>(&msg[1][0], v);
    }
    __syncthreads();

    // all threads run the same control flow here: gen(i) = byte i of the stream, n = its length
    auto absorb = [&](auto gen, uint32_t n) {
        uint32_t done = 0;
        while (done < n) {
            const uint32_t room = kKeccakRate - buflen, take = room < n - done ? room : n - done;
            if (tid < kKeccakRateWords) blk[tid] |= tr_gather_word(gen, tid, buflen, take, done);
            buflen += take;
            done += take;
            if (buflen == kKeccakRate) {
                if (tid < kKeccakRateWords) {  // (blk[tid] is this thread's own; st was last written before a barrier)
                    st[tid] ^= blk[tid];
                    blk[tid] = 0;
                }
                __syncthreads();
                if (tid == 0) tail_permute(st);
                buflen = 0;
                __syncthreads();
            }
        }
    };
    absorb([&](uint32_t i) { return tr_field_stream_byte<FL>(mod_lds, &msg[0][0], i); }, 2 * P);
    __syncthreads();

    uint64_t rr[FL];
    for (uint32_t round = 0; round < num_vars; round++) {
        const uint32_t len = 1u << (num_vars - round), half = len >> 1;  // this round's tables: len entries, half points
        const bool in_lds = round >= n_streamed;
        if (round > 0) {
#pragma unroll
            for (int i = 0; i < FL; i++) rr[i] = r_lds[i];
        }
        // ---- this round's tables: fold those of the round before with its challenge (round 1: the caller's, as they are)
        if (round == n_streamed) {  // the first LDS round: HBM -> LDS
            if (round == 0) {
                for (uint32_t k = 0; k < K; k++)
                    for (uint32_t j = tid; j < len; j += kTailThreads) {
                        uint64_t l[FL];
                        fe_load<FL>(l, src_tabs(k) + (size_t)j * FL);
                        fe_store<FL>(lds_tabs(k) + (size_t)j * FL, l);
                    }
            } else if (round == 1) {
                batch_fold<FL, false>(src_tabs, lds_tabs, K, len, rr, f, tid);
            } else {
                batch_fold<FL, false>(scr_tabs, lds_tabs, K, len, rr, f, tid);
            }
        } else if (round > 0) {
            if (in_lds) batch_fold<FL, true>(lds_tabs, lds_tabs, K, len, rr, f, tid);
            else if (round == 1) batch_fold<FL, false>(src_tabs, scr_tabs, K, len, rr, f, tid);
            else batch_fold<FL, true>(scr_tabs, scr_tabs, K, len, rr, f, tid);
        }
        __syncthreads();
        // ---- the round polynomial at t = e for this lane's points
        uint64_t acc[FL];
        if (in_lds) batch_eval<FL>(lds_tabs, a, K, half, ne, ne_pad, ne_shift, f, tid, acc);
        else if (round == 0) batch_eval<FL>(src_tabs, a, K, half, ne, ne_pad, ne_shift, f, tid, acc);
        else batch_eval<FL>(scr_tabs, a, K, half, ne, ne_pad, ne_shift, f, tid, acc);
        // ---- sum over the lanes with the same e: inside the wave by shuffles, across the waves through LDS
        for (uint32_t s = 32; s >= ne_pad; s >>= 1) {
            uint64_t o[FL];
#pragma unroll
            for (int i = 0; i < FL; i++) o[i] = tail_shfl_xor(acc[i], s);
            fe_add<FL>(acc, o, f);
        }
        if ((tid & 63u) < ne_pad) fe_store<FL>(&wred[tid >> 6][tid & 63u][0], acc);
        __syncthreads();
        if (tid < ne) {
            uint64_t sum[FL];
            fe_load<FL>(sum, &wred[0][tid][0]);
            for (uint32_t w = 1; w < kTailWaves; w++) {
                uint64_t o[FL];
                fe_load<FL>(o, &wred[w][tid][0]);
                fe_add<FL>(sum, o, f);
            }
            fe_store<FL>(&msg[tid][0], sum);
            fe_store<FL>(a.out + ((size_t)round * ne + tid) * FL, sum);
        }
        __syncthreads();
        // ---- the transcript: absorb_slice(message), get_challenge, absorb(challenge)   (sumcheck.rs:100-103)
        absorb([&](uint32_t i) { return tr_field_stream_byte<FL>(mod_lds, &msg[0][0], i); }, ne * P);
        // finalize a COPY: pad 0x01 .. 0x80 over the pending bytes, one more permutation
        if (tid < 25) tmp[tid] = tr_finalize_word(st, blk, buflen, tid);
        __syncthreads();
        if (tid == 0) {
            tail_permute(tmp);
            uint64_t ch[FL];
            tr_challenge<FL>(a.tf, tmp, ch);
            fe_store<FL>(r_lds, ch);
            fe_store<FL>(a.out + (size_t)num_vars * ne * FL + (size_t)round * FL, ch);
        }
        __syncthreads();
        // 0x00 | digest | 0x01 (get_challenge_limbs, transcript.rs:72-86), then the challenge as a field element
        absorb([&](uint32_t i) { return tr_challenge_stream_byte<FL>(mod_lds, tmp, r_lds, i); }, 34 + P);
        __syncthreads();
    }
    uint64_t *so = a.out + (size_t)num_vars * (ne + 1) * FL;
    if (tid < 25) so[tid] = st[tid];
    if (tid < kKeccakRateWords) so[25 + tid] = blk[tid];
    if (tid == 0) so[25 + kKeccakRateWords] = buflen;
}

}  // namespace zipk
