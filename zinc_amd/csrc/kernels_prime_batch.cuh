// The kernels of zip_get_prime_batch: get_prime on n independent transcripts, one MEMBER per lane.
//
// One Keccak-f[1600] by one lane is pure latency (profiles/sumcheck_onecall.md), so 64 chains per wave cost what one
// costs.  A call runs in rounds of w candidates per member; a round is four launches whatever the number of members:
//   prime_chain_batch_kernel   every live member's sponge advances by w candidates (prime_next_candidate_words,
//                              prime_dev.cuh); the candidates go out candidate-major for (live index, k)
//   prime_test_base2_kernel    (kernels_prime.cuh, unchanged) tests the round's n_live * w candidates
//   prime_reduce_batch_kernel  per live member the first accepted candidate, or none: prime and position out, the
//                              list of the members still live for the next round
//   prime_chain_batch_kernel   again, as the REPLAY: the members that finished walk first + 1 steps from the sponge
//                              the round started with, into the result -- the winner's sponge, with nothing of the
//                              candidates beyond it; no snapshot per candidate is kept
// Sponges on the device are word-major, [kPrimeSpongeWords][n]: st[25], blk[17], buflen -- lane m reads word i at
// i * n + m, so the loads of a wave coalesce.  Workgroups of ONE wave, as prime_test_base2_kernel has them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_prime.cuh"

namespace zipk {

constexpr uint32_t kPrimeSpongeWords = 25 + kKeccakRateWords + 1;

// src, dst: [kPrimeSpongeWords][n], indexed by MEMBER; live: n_live member numbers (nullptr: member j is lane j);
// steps: per live index, how many candidates to walk (nullptr: w for every one; 0: the lane does nothing and writes
// nothing); cands: [n_live * w][FL] (nullptr: none are written).
template <int FL>
__global__ __launch_bounds__(kPrimeThreads) void prime_chain_batch_kernel(const uint64_t *__restrict__ src,
                                                                         uint64_t *__restrict__ dst, uint32_t n,
                                                                         const uint32_t *__restrict__ live, uint32_t n_live,
                                                                         const uint32_t *__restrict__ steps, uint32_t w,
                                                                         uint64_t *__restrict__ cands) {
    const uint32_t j = blockIdx.x * kPrimeThreads + threadIdx.x;
    if (j >= n_live) return;
    const uint32_t m = live ? live[j] : j;
    const uint32_t count = steps ? steps[j] : w;
    if (m >= n || count == 0 || count > w) return;
    TrSponge sp;
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) sp.st[i] = src[(size_t)i * n + m];
#pragma unroll
    for (uint32_t i = 0; i < kKeccakRateWords; i++) sp.blk[i] = src[(size_t)(25 + i) * n + m];
    sp.buflen = (uint32_t)src[(size_t)(kPrimeSpongeWords - 1) * n + m];
#pragma unroll 1
    for (uint32_t k = 0; k < count; k++) {
        uint64_t c[FL];
        prime_next_candidate_words<FL>(sp, c);
        if (cands) {
#pragma unroll
            for (int i = 0; i < FL; i++) cands[((size_t)j * w + k) * FL + i] = c[i];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 25; i++) dst[(size_t)i * n + m] = sp.st[i];
#pragma unroll
    for (uint32_t i = 0; i < kKeccakRateWords; i++) dst[(size_t)(25 + i) * n + m] = sp.blk[i];
    dst[(size_t)(kPrimeSpongeWords - 1) * n + m] = sp.buflen;
}

// One live member per lane: the first accepted of its w candidates of this round.  Found: primes[m], tried[m] =
// done + first + 1, steps[j] = first + 1 (the replay's count).  Not found: steps[j] = 0 and m joins live_next -- the
// wave counts its survivors by ballot, lane 0 takes a range of the list with one atomic on *n_next (zeroed before the
// launch), every survivor stores its member number at its rank within the wave.  The ORDER of live_next depends on
// which wave comes first; nothing of the results does.
template <int FL>
__global__ __launch_bounds__(kPrimeThreads) void prime_reduce_batch_kernel(const uint64_t *__restrict__ cands,
                                                                          const uint8_t *__restrict__ verdicts, uint32_t n,
                                                                          const uint32_t *__restrict__ live, uint32_t n_live,
                                                                          uint32_t w, uint32_t done, uint64_t *__restrict__ primes,
                                                                          uint32_t *__restrict__ tried, uint32_t *__restrict__ steps,
                                                                          uint32_t *__restrict__ live_next,
                                                                          uint32_t *__restrict__ n_next) {
    const uint32_t j = blockIdx.x * kPrimeThreads + threadIdx.x;
    const bool valid = j < n_live;
    uint32_t m = 0;
    bool survives = false;
    if (valid) {
        m = live ? live[j] : j;
        uint32_t first = w;
        for (uint32_t k = 0; k < w && first == w; k++)
            if (verdicts[(size_t)j * w + k]) first = k;
        if (m < n) {
            if (first < w) {
#pragma unroll
                for (int i = 0; i < FL; i++) primes[(size_t)m * FL + i] = cands[((size_t)j * w + first) * FL + i];
                tried[m] = done + first + 1;
                steps[j] = first + 1;
            } else {
                steps[j] = 0;
                survives = true;
            }
        }
    }
    const uint64_t mask = __ballot(survives);
    uint32_t base = 0;
    if (threadIdx.x == 0 && mask) base = atomicAdd(n_next, (uint32_t)__popcll(mask));
    base = __shfl(base, 0);
    if (survives) live_next[base + (uint32_t)__popcll(mask & (((uint64_t)1 << threadIdx.x) - 1))] = m;
}

}  // namespace zipk
