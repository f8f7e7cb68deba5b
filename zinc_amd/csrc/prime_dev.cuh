// The primality test of prime_gen::get_prime (src/prime_gen.rs:15-28) -- MillerRabin::test_base_two (src/field/uint.rs:66-76):
// a strong probable-prime test to base 2 -- as code that runs on the device and on the host alike, one candidate per
// thread (prime_test_base2_kernel, kernels_prime.cuh; the CPU restatement of tools/prime_times.py and the host-side
// checks compile the same lines with g++).  Written from the definition of the test:
//   n - 1 = 2^s d, d odd; z = 2^d mod n; accept if z == 1 or z == n - 1; otherwise square up to s - 1 times, accepting on
//   n - 1 and rejecting on 1; reject when the squarings run out.
//
// The CANDIDATE is the modulus, so every Montgomery constant is per thread: -n^-1 mod 2^64 by Newton iteration and
// R mod n by 64 FL modular doublings of 1.  The base is 2: "multiply by the base" is a modular doubling, only the
// squarings need the Montgomery product.  n is any odd value of FL limbs -- no spare top bit, top limbs possibly zero.
// Every loop below has a trip count of at most 64 FL whatever n is.
#pragma once
#include <stdint.h>
#include <string.h>

#include "keccak_dev.cuh"  // ZK_HD, tr_geq, tr_sub

namespace zipk {

// -n^-1 mod 2^64 for odd n0: x = n0 is the inverse modulo 8 (n0^2 = 1 mod 8), every Newton step doubles the bits
ZK_HD uint64_t prime_neg_inv64(uint64_t n0) {
    uint64_t x = n0;
#pragma unroll
    for (int i = 0; i < 5; i++) x *= 2 - n0 * x;  // 3 -> 6 -> 12 -> 24 -> 48 -> 96 bits
    return 0 - x;
}

// a = 2 a mod n for a < n (2 a < 2^(64 FL + 1): the bit shifted out counts)
template <int FL>
ZK_HD void prime_dbl_mod(uint64_t (&a)[FL], const uint64_t (&n)[FL]) {
    const uint64_t top = a[FL - 1] >> 63;
#pragma unroll
    for (int i = FL - 1; i > 0; i--) a[i] = (a[i] << 1) | (a[i - 1] >> 63);
    a[0] <<= 1;
    if (top || tr_geq<FL>(a, n)) tr_sub<FL>(a, n);
}

// a * b / 2^(64 FL) mod n, canonical, for a, b < n: the interleaved Montgomery product of tr_mont_mul (keccak_dev.cuh)
// and mont_mul / mont_redc (kernels_open.cuh), which keep the carry limb a modulus without a spare bit needs, over a
// bare modulus instead of a field structure
template <int FL>
ZK_HD void prime_mont_mul(const uint64_t (&a)[FL], const uint64_t (&b)[FL], const uint64_t (&n)[FL], uint64_t inv,
                          uint64_t (&out)[FL]) {
    typedef unsigned __int128 u128_t;
    uint64_t t[FL + 2];
#pragma unroll
    for (int i = 0; i < FL + 2; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < FL; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < FL; j++) {
            const u128_t x = (u128_t)a[j] * b[i] + t[j] + carry;
            t[j] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        u128_t x = (u128_t)t[FL] + carry;
        t[FL] = (uint64_t)x;
        t[FL + 1] = (uint64_t)(x >> 64);
        const uint64_t m = t[0] * inv;
        x = (u128_t)m * n[0] + t[0];
        carry = (uint64_t)(x >> 64);
#pragma unroll
        for (int j = 1; j < FL; j++) {
            x = (u128_t)m * n[j] + t[j] + carry;
            t[j - 1] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        x = (u128_t)t[FL] + carry;
        t[FL - 1] = (uint64_t)x;
        t[FL] = t[FL + 1] + (uint64_t)(x >> 64);
    }
#pragma unroll
    for (int i = 0; i < FL; i++) out[i] = t[i];
    if (t[FL] || tr_geq<FL>(out, n)) tr_sub<FL>(out, n);
}

template <int FL>
ZK_HD bool prime_eq(const uint64_t (&a)[FL], const uint64_t (&b)[FL]) {
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < FL; i++) d |= a[i] ^ b[i];
    return d == 0;
}

// bit `idx` of a (0 at and beyond 64 FL); the limb is picked by comparison, not by a variable index into registers
template <int FL>
ZK_HD uint32_t prime_bit(const uint64_t (&a)[FL], uint32_t idx) {
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < FL; k++)
        if ((uint32_t)k == idx / 64) w = a[k];
    return (uint32_t)(w >> (idx % 64)) & 1u;
}

// MillerRabin::new(n).test_base_two().is_probably_prime() for odd n >= 3; false for what is outside that contract
// (even n, n < 3).  A strong pseudoprime to base 2 (2047, 2^64 + 1, 2^67 - 1, ...) is accepted, as by the reference.
template <int FL>
ZK_HD bool prime_test_base2(const uint64_t (&n)[FL]) {
    uint64_t hi = 0;
#pragma unroll
    for (int i = 1; i < FL; i++) hi |= n[i];
    if (!(n[0] & 1) || (hi == 0 && n[0] < 3)) return false;

    // n - 1 = 2^s d: s = the trailing zeros of n - 1, 1 <= s <= 64 FL - 1
    uint64_t nm1[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) nm1[i] = n[i];
    nm1[0] &= ~(uint64_t)1;
    uint32_t s = 0;
    bool counting = true;
#pragma unroll
    for (int i = 0; i < FL; i++) {
        if (counting && nm1[i]) {
            s += (uint32_t)__builtin_ctzll(nm1[i]);
            counting = false;
        } else if (counting) {
            s += 64;
        }
    }

    // Montgomery forms of 1 and of n - 1: R mod n by 64 FL doublings of 1 (1 < n), and n - (R mod n)
    const uint64_t inv = prime_neg_inv64(n[0]);
    uint64_t one[FL], minus_one[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) one[i] = i == 0 ? 1 : 0;
#pragma unroll 1
    for (int i = 0; i < 64 * FL; i++) prime_dbl_mod<FL>(one, n);
#pragma unroll
    for (int i = 0; i < FL; i++) minus_one[i] = n[i];
    tr_sub<FL>(minus_one, one);

    // z = 2^d, d = (n - 1) >> s, left to right over all 64 FL bit positions (the leading zeros square 1)
    uint64_t z[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) z[i] = one[i];
#pragma unroll 1
    for (int i = 64 * FL - 1; i >= 0; i--) {
        prime_mont_mul<FL>(z, z, n, inv, z);
        if (prime_bit<FL>(nm1, (uint32_t)i + s)) prime_dbl_mod<FL>(z, n);
    }
    if (prime_eq<FL>(z, one) || prime_eq<FL>(z, minus_one)) return true;
#pragma unroll 1
    for (uint32_t r = 1; r < s; r++) {  // s - 1 <= 64 FL - 2 squarings
        prime_mont_mul<FL>(z, z, n, inv, z);
        if (prime_eq<FL>(z, minus_one)) return true;
        if (prime_eq<FL>(z, one)) return false;
    }
    return false;
}

// ---- the candidate chain of get_prime (prime_gen.rs:8-26) on one thread --------------------------------------------------
// hash_int: get_random_bytes(8 FL) -- 8 FL <= 32, so ONE squeeze of a clone that absorbed the counter 0 as four
// big-endian bytes (transcript.rs:40-55), truncated --, the bytes absorbed, then read big-endian; get_prime subtracts 1
// from an even candidate (0 wraps to 2^(64 FL) - 1).  The chain never looks at a verdict: candidates can be produced
// ahead of their tests, and `sp` after candidate k is what the reference's loop holds when it tests candidate k.
// (host only, little-endian: the pending bytes of TrSponge::blk are addressed as bytes)
inline void prime_sponge_absorb_bytes(TrSponge &sp, const uint8_t *bytes, uint32_t n) {
    while (n) {
        const uint32_t room = kKeccakRate - sp.buflen, take = room < n ? room : n;
        if (bytes) {
            memcpy(reinterpret_cast<uint8_t *>(sp.blk) + sp.buflen, bytes, take);
            bytes += take;
        }  // (bytes == nullptr: n zero bytes -- blk is zero beyond buflen)
        sp.buflen += take;
        n -= take;
        if (sp.buflen == kKeccakRate) {
            for (uint32_t w = 0; w < kKeccakRateWords; w++) {
                sp.st[w] ^= sp.blk[w];
                sp.blk[w] = 0;
            }
            keccak_f1600(sp.st);
            sp.buflen = 0;
        }
    }
}
template <int FL>
inline void prime_next_candidate(TrSponge &sp, uint64_t (&cand)[FL]) {
    TrSponge clone = sp;
    prime_sponge_absorb_bytes(clone, nullptr, 4);  // the counter 0
    uint64_t d[25];
    for (uint32_t w = 0; w < 25; w++) d[w] = tr_finalize_word(clone.st, clone.blk, clone.buflen, w);
    keccak_f1600(d);
    prime_sponge_absorb_bytes(sp, reinterpret_cast<const uint8_t *>(d), 8 * FL);  // the digest's first 8 FL bytes
    for (int k = 0; k < FL; k++) cand[FL - 1 - k] = keccak_bswap64(d[k]);
    if (!(cand[0] & 1)) {
        uint64_t one[FL] = {1};
        tr_sub<FL>(cand, one);
    }
}

// The same step word-wise, for the device and the host alike (prime_chain_batch_kernel, kernels_prime_batch.cuh: one
// member of a batch per lane, `buflen` differs per lane).  No byte addressing and no variable index into st / blk: the
// rate words a step touches are picked by comparison over the 17 words, as prime_bit picks a limb.
//   1. the clone absorbs the counter 0: four zero bytes change no pending word, they only move buflen -- across the
//      rate boundary from 132 on, where the clone's block is absorbed first;
//   2./3. finalize (tr_finalize_word) and one permutation: d;
//   4. the first 8 FL digest bytes go to byte offset buflen: with q = buflen / 8 and s = 8 (buflen % 8), word q + k of
//      the (two-block) rate gets d[k] << s | d[k - 1] >> (64 - s), k = 0 .. FL; words 17 .. 17 + FL are words 0 .. FL
//      of the next block (136 = 17 * 8: the block boundary is a word boundary);
//   5./6. the candidate big-endian, minus 1 if even.
template <int FL>
ZK_HD void prime_next_candidate_words(TrSponge &sp, uint64_t (&cand)[FL]) {
    uint64_t d[25];
    uint32_t cl = sp.buflen + 4;
    if (cl >= kKeccakRate) {  // the clone's block fills: st ^ blk permuted, nothing pending but zero bytes
#pragma unroll
        for (uint32_t w = 0; w < 25; w++) d[w] = w < kKeccakRateWords ? sp.st[w] ^ sp.blk[w] : sp.st[w];
        keccak_f1600(d);
        cl -= kKeccakRate;
        d[0] ^= (uint64_t)0x01 << (8 * cl);  // cl <= 3: the pad's first byte is in word 0
        d[kKeccakRateWords - 1] ^= (uint64_t)0x80 << 56;
    } else {
#pragma unroll
        for (uint32_t w = 0; w < 25; w++) d[w] = tr_finalize_word(sp.st, sp.blk, cl, w);
    }
    keccak_f1600(d);

    const uint32_t q = sp.buflen / 8, s = 8 * (sp.buflen % 8);
    uint64_t piece[FL + 1];  // piece[k] belongs to word q + k
#pragma unroll
    for (int k = 0; k <= FL; k++) {
        const uint64_t lo = k < FL ? d[k] << s : 0;
        const uint64_t hi = k > 0 ? (d[k - 1] >> 1) >> (63 - s) : 0;  // d[k - 1] >> (64 - s), 0 for s == 0
        piece[k] = lo | hi;
    }
    uint64_t next[FL + 1];  // words 0 .. FL of the block after this one
#pragma unroll
    for (int i = 0; i <= FL; i++) next[i] = 0;
#pragma unroll
    for (int k = 0; k <= FL; k++) {
#pragma unroll
        for (uint32_t w = 0; w < kKeccakRateWords; w++)
            if (w == q + (uint32_t)k) sp.blk[w] |= piece[k];
#pragma unroll
        for (int i = 0; i <= FL; i++)
            if (kKeccakRateWords + (uint32_t)i == q + (uint32_t)k) next[i] |= piece[k];
    }
    sp.buflen += 8 * FL;
    if (sp.buflen >= kKeccakRate) {
#pragma unroll
        for (uint32_t w = 0; w < kKeccakRateWords; w++) {
            sp.st[w] ^= sp.blk[w];
            sp.blk[w] = w <= (uint32_t)FL ? next[w] : 0;
        }
        keccak_f1600(sp.st);
        sp.buflen -= kKeccakRate;
    }

#pragma unroll
    for (int k = 0; k < FL; k++) cand[FL - 1 - k] = keccak_bswap64(d[k]);
    if (!(cand[0] & 1)) {
        uint64_t one[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) one[i] = i == 0 ? 1 : 0;
        tr_sub<FL>(cand, one);
    }
}

// ZIP_HIP_PRIME_BATCH: candidates per launch, 1 .. max.  Anything else -- unset, empty, not all digits, out of range --
// leaves the default.
inline uint32_t prime_batch_knob(const char *text, uint32_t def, uint32_t max) {
    if (!text || !*text) return def;
    uint64_t v = 0;
    for (const char *p = text; *p; p++) {
        if (*p < '0' || *p > '9' || p - text >= 9) return def;
        v = 10 * v + (uint64_t)(*p - '0');
    }
    return v >= 1 && v <= max ? (uint32_t)v : def;
}

}  // namespace zipk
