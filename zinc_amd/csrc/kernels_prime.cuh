// The primality tests of zip_get_prime / zip_prime_test_base2: prime_test_base2 (prime_dev.cuh) on one candidate per
// lane.  The tests of a batch are independent modular exponentiations of 64 FL squarings each -- pure VALU work in
// registers: no LDS, no atomics, no cross-lane traffic.  Workgroups of ONE wave, so that a batch of a few hundred
// candidates spreads over as many CUs as it has waves instead of queueing on one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prime_dev.cuh"

namespace zipk {

constexpr uint32_t kPrimeThreads = 64;

// candidates: n * FL limbs, little-endian, candidate-major; verdicts: n bytes, 1 = probably prime
template <int FL>
__global__ __launch_bounds__(kPrimeThreads) void prime_test_base2_kernel(const uint64_t *__restrict__ candidates, uint32_t n,
                                                                        uint8_t *__restrict__ verdicts) {
    const uint32_t i = blockIdx.x * kPrimeThreads + threadIdx.x;
    if (i >= n) return;  // tail lanes of the last wave
    uint64_t c[FL];
#pragma unroll
    for (int k = 0; k < FL; k++) c[k] = candidates[(size_t)i * FL + k];
    verdicts[i] = prime_test_base2<FL>(c) ? 1 : 0;
}

}  // namespace zipk
