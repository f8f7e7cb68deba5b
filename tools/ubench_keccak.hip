// What does ONE Keccak-f[1600] permutation by ONE wave cost on this chip, and what a whole round's transcript step of
// the sumcheck tail kernel (absorb the message, finalize a copy, absorb the challenge)?  zip_sumcheck_prove's tail
// kernel has 3-4 permutations on the critical path of every round.
//   form A  one lane, VALU: the 25 lanes of the state in 50 VGPRs of lane 0 (tail_permute, what the library ships)
//   form B  scalar ALU: the same code on wave-uniform values, the state in SGPRs (permute_scalar, here)
//   form C  25 lanes of one wave, one state lane each, two exchanges through LDS per round (permute_25_lanes, here)
// Each form as a chain of dependent permutations inside one kernel (100 MHz wall clock around the chain), checked
// against the host's keccak_f1600 first; then sumcheck_tail_kernel itself with tables so small that the arithmetic is
// one pass: the time per tail round is the slope over the number of rounds.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -Izinc_amd/csrc -Iinclude tools/ubench_keccak.hip -o ubench_keccak
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kernels_sumcheck_tail.cuh"
using namespace zipk;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__device__ __forceinline__ uint64_t tail_uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// Form B: the library's tail_permute on wave-uniform values, so that the compiler keeps the whole permutation in SGPRs
// (native 64-bit logic on the scalar ALU); the results are stored with ordinary vector stores.
__device__ __forceinline__ void permute_scalar(uint64_t *w) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = tail_uniform64(w[i]);
    keccak_f1600(a);
#pragma unroll
    for (int i = 0; i < 25; i++) w[i] = a[i];
}
// Form C: Keccak-f on 25 words in LDS by 25 LANES of one wave (every lane of the wave calls it; lanes >= 25 idle): lane
// x + 5 y keeps lane (x, y) of the state.  Two exchanges through LDS per round -- theta reads the two neighbour columns
// (10 words), rho + pi + chi write the rotated lane to its pi position and read the three words of a row -- instead of
// ~300 dependent VALU instructions of one lane.  LDS operations of one wave execute in order, so a wave-level fence
// (compiler ordering only) is all the synchronisation there is.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void permute_25_lanes(uint64_t *w, uint64_t *xch, uint32_t lane) {
    constexpr uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
        0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
        0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
        0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
        0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    constexpr uint32_t ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    const bool on = lane < 25;
    const uint32_t l = on ? lane : 0, x = l % 5, y = l / 5;
    const uint32_t rot = ROT[l], dest = y + 5 * ((2 * x + 3 * y) % 5);
    const uint32_t cm = (x + 4) % 5, cp = (x + 1) % 5, r1 = (x + 1) % 5 + 5 * y, r2 = (x + 2) % 5 + 5 * y;
    uint64_t a = w[l];
#pragma unroll 1
    for (int round = 0; round < 24; round++) {
        if (on) w[l] = a;
        wave_sync();
        const uint64_t c_m = w[cm] ^ w[cm + 5] ^ w[cm + 10] ^ w[cm + 15] ^ w[cm + 20];
        const uint64_t c_p = w[cp] ^ w[cp + 5] ^ w[cp + 10] ^ w[cp + 15] ^ w[cp + 20];
        a ^= c_m ^ ((c_p << 1) | (c_p >> 63));       // theta
        a = (a << rot) | (a >> ((64 - rot) & 63));   // rho (rot = 0: a | a)
        wave_sync();
        if (on) xch[dest] = a;                        // pi
        wave_sync();
        a = xch[l] ^ (~xch[r1] & xch[r2]);            // chi
        if (l == 0) a ^= RC[round];                   // iota
        wave_sync();
    }
    if (on) w[l] = a;
    wave_sync();
}


template <bool SCALAR>
__global__ void __launch_bounds__(64) perm_chain(uint64_t *state, int n, unsigned long long *stamps) {
    __shared__ uint64_t st[25];
    if (threadIdx.x < 25) st[threadIdx.x] = state[threadIdx.x];
    __syncthreads();
    const unsigned long long w0 = wall_clock64();
    if (threadIdx.x == 0)
        for (int i = 0; i < n; i++) {  // LDS -> registers -> LDS, as in the tail kernel
            if (SCALAR) permute_scalar(st);
            else tail_permute(st);
        }
    __syncthreads();
    const unsigned long long w1 = wall_clock64();
    if (threadIdx.x < 25) state[threadIdx.x] = st[threadIdx.x];
    if (threadIdx.x == 0) stamps[0] = w1 - w0;
}

__global__ void __launch_bounds__(64) perm_chain25(uint64_t *state, int n, unsigned long long *stamps) {
    __shared__ uint64_t st[25], xch[25];
    if (threadIdx.x < 25) st[threadIdx.x] = state[threadIdx.x];
    __syncthreads();
    const unsigned long long w0 = wall_clock64();
    for (int i = 0; i < n; i++) permute_25_lanes(st, xch, threadIdx.x);
    __syncthreads();
    const unsigned long long w1 = wall_clock64();
    if (threadIdx.x < 25) state[threadIdx.x] = st[threadIdx.x];
    if (threadIdx.x == 0) stamps[0] = w1 - w0;
}
// the three forms must agree
static void check_forms(uint64_t *state, unsigned long long *st, hipStream_t s) {
    uint64_t h[3][25];
    for (int form = 0; form < 3; form++) {
        CK(hipMemset(state, 0x5a, 200));
        if (form == 0) hipLaunchKernelGGL(perm_chain<false>, dim3(1), dim3(64), 0, s, state, 3, st);
        else if (form == 1) hipLaunchKernelGGL(perm_chain<true>, dim3(1), dim3(64), 0, s, state, 3, st);
        else hipLaunchKernelGGL(perm_chain25, dim3(1), dim3(64), 0, s, state, 3, st);
        CK(hipStreamSynchronize(s));
        CK(hipMemcpy(h[form], state, 200, hipMemcpyDeviceToHost));
    }
    uint64_t ref[25];
    memset(ref, 0x5a, sizeof ref);
    for (int i = 0; i < 3; i++) keccak_f1600(ref);
    for (int form = 0; form < 3; form++)
        printf("form %d %s the host permutation\n", form, memcmp(h[form], ref, 200) ? "DIFFERS FROM" : "equals");
}

static double tail_us(uint32_t n_rounds, uint32_t degree, const uint64_t *tab_d, uint64_t *out_d, hipStream_t s) {
    constexpr int FL = 4;
    SumcheckTailArgs<FL> a{};
    FieldDev<FL> f{};
    // 2^255 - 19 (any odd modulus does: the arithmetic is not what is measured)
    const uint64_t q[4] = {0xffffffffffffffedULL, ~0ULL, ~0ULL, 0x7fffffffffffffffULL};
    for (int i = 0; i < FL; i++) { f.modulus[i] = a.tf.modulus[i] = a.tf.red_mod[i] = q[i]; f.r2[i] = a.tf.r2[i] = i == 0 ? 1444 : 0; }
    f.inv = a.tf.inv = 0x86bca1af286bca1bULL;
    a.tf.cbits = 254;
    a.n_mles = 1;
    a.degree = degree;
    a.log_len = n_rounds;
    a.src[0] = tab_d;
    a.out = out_d;
    std::vector<float> ms;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int rep = 0; rep < 21; rep++) {
        CK(hipEventRecord(e0, s));
        hipLaunchKernelGGL((sumcheck_tail_kernel<FL>), dim3(1), dim3(kTailThreads), ((size_t)1 << n_rounds) * FL * 8, s, a, f);
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2] * 1e3;
}

int main() {
    uint64_t *state, *tab, *out;
    unsigned long long *st;
    CK(hipMalloc(&state, 256));
    CK(hipMemset(state, 0x5a, 256));
    CK(hipMalloc(&tab, 64 * 32));
    CK(hipMemset(tab, 0, 64 * 32));
    CK(hipMalloc(&out, 8192));
    CK(hipHostMalloc(&st, 256));
    hipStream_t s;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    check_forms(state, st, s);
    const int n = 200;
    for (int form = 0; form < 3; form++) {
        double best = 1e30;
        for (int rep = 0; rep < 5; rep++) {
            if (form == 0) hipLaunchKernelGGL(perm_chain<false>, dim3(1), dim3(64), 0, s, state, n, st);
            else if (form == 1) hipLaunchKernelGGL(perm_chain<true>, dim3(1), dim3(64), 0, s, state, n, st);
            else hipLaunchKernelGGL(perm_chain25, dim3(1), dim3(64), 0, s, state, n, st);
            CK(hipStreamSynchronize(s));
            best = std::min(best, (double)st[0] * 10.0 / n);  // 100 MHz ticks -> ns per permutation
        }
        printf("permutation, %-22s %8.0f ns each (chain of %d, best of 5)\n", form == 0 ? "one lane VALU:" : form == 1 ? "scalar ALU:" : "25 lanes, LDS exchange:", best, n);
    }
    for (uint32_t degree = 2; degree <= 3; degree++) {
        const double a1 = tail_us(1, degree, tab, out, s), a6 = tail_us(6, degree, tab, out, s);
        printf("tail kernel, degree %u, 4 limbs: 1 round %.1f us, 6 rounds %.1f us -> %.1f us per round\n", degree, a1, a6, (a6 - a1) / 5);
    }
    return 0;
}
