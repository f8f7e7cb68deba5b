// The tail of a sumcheck in ONE launch (zip_sumcheck_prove): from the first round whose tables fit the LDS of one
// workgroup, a single workgroup of 1024 threads plays every remaining round of IPForMLSumcheck::prove_round
// (src/sumcheck/prover.rs:62-180) AND the verifier's side of MLSumcheck::prove_as_subprotocol (src/sumcheck.rs:97-106):
// absorb the round message, squeeze the challenge, absorb it, fold with it.  The Keccak sponge lives in LDS; nothing
// waits for the host or for another launch.  Messages, challenges and the final sponge are written out once.
//
// LDS budget (160 KiB per CU, one workgroup): the first tail round works on tables of 2^n entries per MLE (it reads
// the 2^(n+1)-entry tables of the round before from HBM and folds them on the way in; n = num_vars: it copies the
// caller's tables).  Later rounds fold IN PLACE (below), so the tables take K * 2^n * FL * 8 bytes and nothing more;
// the reduction scratch, the message, the challenge and the sponge take kTailFixedLds bytes.  Hence
//   n <= floor(log2((160 KiB - kTailFixedLds) / (8 K FL)))  :  K = 4, FL = 4 -> 2^10 entries (128 KiB),
//   K = 2, FL = 4 -> 2^11, K = 1, FL = 2 -> 2^13 (the cap).
//
// In-place fold of a table of `len` entries, p'[j] = p[2j] + r (p[2j+1] - p[2j]) (fix_variables, dense.rs:142-168),
// by N = 1024 threads in passes: pass p reads the entries [2pN, 2pN + 2N) into registers, BARRIER, writes [pN, pN + N).
// A later pass q > p reads from 2qN >= (p + 1) N on: nothing an earlier pass wrote; and it writes only after its own
// barrier, when every read of the passes before is long done.  One barrier per pass and table, no second buffer.
//
// Evaluation: ne_pad = the power of two >= degree + 1 lanes per hypercube point b, lane e computes the combination
// function at t = e from the entries at t = 0, 1 (v1 + (e - 1)(v1 - v0): the same canonical residue as the reference's
// running sum).  Everything is exact arithmetic on canonical Montgomery residues, so the sums are bit for bit those of
// the round kernels in any order.  K, degree and the terms are run-time values (loops over LDS reads, no per-thread
// arrays indexed by them): three instances (FL = 2, 3, 4) instead of forty-eight, and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keccak_dev.cuh"
#include "kernels_sumcheck.cuh"

namespace zipk {

constexpr uint32_t kTailThreads = 1024, kTailWaves = kTailThreads / 64;
constexpr uint32_t kTailMaxLog = 13;  // tables of at most 2^13 entries (K = 1, FL = 2: 128 KiB)
// static LDS of sumcheck_tail_kernel: wred + msg + r + modulus + st + blk + tmp, rounded up
constexpr uint32_t kTailFixedLds = (kTailWaves * 8 * 4 + 5 * 4 + 4 + 4 + 25 + 17 + 25) * 8 + 64;
constexpr uint32_t kTailLdsTotal = 160 * 1024;

template <int FL>
struct SumcheckTailArgs {
    const uint64_t *src[kSumcheckMaxMles];  // what the first tail round reads: 2^(n+1) entries when fold_first, else 2^n
    uint64_t r[FL];                         // the challenge of the round before (fold_first)
    uint32_t n_mles, degree, fold_first;
    uint32_t log_len;                       // n: the first tail round's tables have 2^n entries; it plays n rounds
    uint32_t n_terms;
    uint32_t term_mask[kSumcheckMaxTerms];
    uint64_t coeff[kSumcheckMaxTerms][FL];
    uint64_t st[25], blk[kKeccakRateWords];  // the sponge before the first tail round's message
    uint32_t buflen;
    TrField<FL> tf;
    // [n][degree + 1][FL] messages | [n][FL] challenges | 25 state words | 17 rate words | buflen
    uint64_t *out;
};

// Keccak-f on 25 words in LDS, by the calling lane alone (the caller branches on tid == 0): the 25 lanes of the state in
// 50 VGPRs.  The forms tried beside it (wave-uniform values on the scalar ALU; 25 lanes of one wave trading words through
// LDS) live in tools/ubench_keccak.hip; profiles/sumcheck_onecall.md has the figures.
__device__ __forceinline__ void tail_permute(uint64_t *w) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = w[i];
    keccak_f1600(a);
#pragma unroll
    for (int i = 0; i < 25; i++) w[i] = a[i];
}

__device__ __forceinline__ uint64_t tail_shfl_xor(uint64_t v, uint32_t mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)mask, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)mask, 64);
    return ((uint64_t)hi << 32) | lo;
}

template <int FL>
__global__ void __launch_bounds__(kTailThreads) sumcheck_tail_kernel(SumcheckTailArgs<FL> a, FieldDev<FL> f) {
    extern __shared__ __align__(16) unsigned char sct_smem[];
    uint64_t *tab = reinterpret_cast<uint64_t *>(sct_smem);  // [K][2^n][FL]
    __shared__ uint64_t wred[kTailWaves][8][FL];
    __shared__ uint64_t msg[kSumcheckMaxDegree + 1][FL];
    __shared__ uint64_t r_lds[FL], mod_lds[FL];  // (the modulus: the byte streams index it at run time)
    __shared__ uint64_t st[25], blk[kKeccakRateWords], tmp[25];
    constexpr uint32_t N = kTailThreads, P = 16 * FL + 4;
    const uint32_t tid = threadIdx.x, K = a.n_mles, ne = a.degree + 1;
    const uint32_t ne_pad = ne <= 2 ? 2u : ne <= 4 ? 4u : 8u, ne_shift = ne <= 2 ? 1u : ne <= 4 ? 2u : 3u;
    const uint32_t len0 = 1u << a.log_len;
    const size_t tab_stride = (size_t)len0 * FL;
    uint32_t buflen = a.buflen;  // every thread keeps the same copy

    if (tid < 25) st[tid] = a.st[tid];
    if (tid < (uint32_t)FL) mod_lds[tid] = a.tf.modulus[tid];
    if (tid < kKeccakRateWords) blk[tid] = a.blk[tid];
    uint64_t rr[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) rr[i] = a.r[i];

    // the first tail round's tables: HBM -> LDS, folded on the way when there is a round before
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t *s = a.src[k];
        for (uint32_t j = tid; j < len0; j += N) {
            uint64_t l[FL];
            if (a.fold_first) {
                uint64_t d[FL], t[FL];
                fe_load<FL>(l, s + (size_t)(2 * j) * FL);
                fe_load<FL>(d, s + (size_t)(2 * j + 1) * FL);
                fe_sub<FL>(d, l, f);
                mont_mul<FL>(d, rr, f, t);
                fe_add<FL>(l, t, f);
            } else {
                fe_load<FL>(l, s + (size_t)j * FL);
            }
            fe_store<FL>(tab + k * tab_stride + (size_t)j * FL, l);
        }
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

    for (uint32_t round = 0; round < a.log_len; round++) {
        const uint32_t len = len0 >> round, half = len >> 1;  // this round's tables: len entries, half points
        if (round > 0) {
            // ---- fold in place with the challenge of the round before: 2 len entries -> len
#pragma unroll
            for (int i = 0; i < FL; i++) rr[i] = r_lds[i];
            for (uint32_t base = 0; base < len; base += N) {  // uniform trip counts: the barrier is inside
                const uint32_t j = base + tid;
                for (uint32_t k = 0; k < K; k++) {  // (one table at a time: all K folded pairs at once spill at FL = 4)
                    uint64_t p[FL];
                    if (j < len) {
                        uint64_t d[FL], t[FL];
                        const uint64_t *s = tab + k * tab_stride + (size_t)(2 * j) * FL;
                        fe_load<FL>(p, s);
                        fe_load<FL>(d, s + FL);
                        fe_sub<FL>(d, p, f);
                        mont_mul<FL>(d, rr, f, t);
                        fe_add<FL>(p, t, f);
                    }
                    __syncthreads();
                    if (j < len) fe_store<FL>(tab + k * tab_stride + (size_t)j * FL, p);
                }
            }
            __syncthreads();
        }
        // ---- the round polynomial at t = e for this lane's points
        const uint32_t e = tid & (ne_pad - 1);
        uint64_t acc[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) acc[i] = 0;
        auto at_point = [&](uint32_t k, uint32_t b, uint64_t (&out)[FL]) {
            const uint64_t *s = tab + k * tab_stride + (size_t)(2 * b) * FL;
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
        if (e < ne) {
            for (uint32_t b = tid >> ne_shift; b < half; b += N >> ne_shift) {
                uint64_t c[FL], v[FL], t[FL];
                if (a.n_terms == 0) {  // the product of all MLE values
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
                    for (uint32_t tt = 0; tt < a.n_terms; tt++) {
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
            fe_store<FL>(a.out + (size_t)a.log_len * ne * FL + (size_t)round * FL, ch);
        }
        __syncthreads();
        // 0x00 | digest | 0x01 (get_challenge_limbs, transcript.rs:72-86), then the challenge as a field element
        absorb([&](uint32_t i) { return tr_challenge_stream_byte<FL>(mod_lds, tmp, r_lds, i); }, 34 + P);
        __syncthreads();
    }
    uint64_t *so = a.out + (size_t)a.log_len * (ne + 1) * FL;
    if (tid < 25) so[tid] = st[tid];
    if (tid < kKeccakRateWords) so[25 + tid] = blk[tid];
    if (tid == 0) so[25 + kKeccakRateWords] = buflen;
}

}  // namespace zipk
