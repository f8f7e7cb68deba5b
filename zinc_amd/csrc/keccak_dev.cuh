// The Keccak Fiat-Shamir transcript of ONE loop -- MLSumcheck::prove_as_subprotocol (src/sumcheck.rs:56-112) -- as code
// that runs on the device and on the host alike (zip_sumcheck_prove: the tail kernel steps the sponge itself, the
// library's host thread steps it for the rounds above the tail).  Written from the definitions: Keccak-f[1600]
// (FIPS 202, 3.2-3.4), the Keccak-256 sponge the transcript uses (rate 136, domain byte 0x01, src/transcript.rs:2)
// and this project's host mirror of KeccakTranscript (zinc_amd/host/zinc_zip.cpp).
//
// Sponge in transit (zip_keccak_state, include/zip_hip.h): st = the state after every full block, and the bytes
// absorbed since.  Here the pending bytes are kept as the 17 little-endian words of the rate (`blk`, zero beyond
// buflen), so that a block is absorbed with 17 word xors and the padding of finalize is two word xors.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZK_HD __host__ __device__ __forceinline__
#else
#define ZK_HD inline
#endif

namespace zipk {

constexpr uint32_t kKeccakRate = 136, kKeccakRateWords = 17;

ZK_HD uint64_t keccak_rol(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// Keccak-f[1600]: lane (x, y) = a[x + 5 y].  The 25 lanes stay in registers: every index below is a compile-time
// constant once the x / y loops are unrolled; only the loop over the 24 rounds is kept (code size).
ZK_HD void keccak_f1600(uint64_t (&a)[25]) {
    constexpr uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
        0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
        0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
        0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
        0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    // rho offsets, [x + 5 y]
    constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll 1
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];  // theta
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ keccak_rol(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
        }
#pragma unroll
        for (int x = 0; x < 5; x++)  // rho and pi: B[y, 2x + 3y] = rot(A[x, y])
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rol(a[x + 5 * y], ROT[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; y++)  // chi
#pragma unroll
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= RC[round];  // iota
    }
}

ZK_HD uint64_t keccak_bswap64(uint64_t v) {
    v = ((v & 0x00ff00ff00ff00ffULL) << 8) | ((v >> 8) & 0x00ff00ff00ff00ffULL);
    v = ((v & 0x0000ffff0000ffffULL) << 16) | ((v >> 16) & 0x0000ffff0000ffffULL);
    return (v << 32) | (v >> 32);
}

// ---- the byte streams the sumcheck loop absorbs ---------------------------------------------------------------------
// absorb_random_field (field.rs:360-378, the host mirror's KeccakTranscript::absorb_random_field): per element
//   0x3 | modulus, big-endian | 0x5 | 0x1 | value, big-endian | 0x3            = 16 FL + 4 bytes
// Byte `idx` of the framing of `n` consecutive elements vals[e][FL] (limbs little-endian, as everywhere).
template <int FL>
ZK_HD uint32_t tr_field_stream_byte(const uint64_t *modulus, const uint64_t *vals, uint32_t idx) {
    constexpr uint32_t P = 16 * FL + 4;
    const uint32_t e = idx / P, off = idx % P;
    if (off == 0 || off == P - 1) return 0x3;
    if (off == 8 * FL + 1) return 0x5;
    if (off == 8 * FL + 2) return 0x1;
    const bool is_val = off > 8 * FL + 2;
    const uint32_t k = is_val ? off - (8 * FL + 3) : off - 1;  // big-endian byte number, 0 = most significant
    const uint64_t *src = is_val ? vals + (size_t)e * FL : modulus;
    return (uint32_t)(src[FL - 1 - k / 8] >> (8 * (7 - k % 8))) & 0xffu;
}

// The contribution of `take` stream bytes, the first of which lands at sponge offset `buflen`, to word `w` of the
// rate: byte p of the block is bits 8 (p mod 8) of word p / 8.  gen(i) = stream byte i; the block's first new byte
// is stream byte `done`.
template <class Gen>
ZK_HD uint64_t tr_gather_word(Gen &&gen, uint32_t w, uint32_t buflen, uint32_t take, uint32_t done) {
    uint64_t word = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t p = 8 * w + j;
        if (p >= buflen && p < buflen + take) word |= (uint64_t)(gen(done + p - buflen) & 0xffu) << (8 * j);
    }
    return word;
}

// ---- get_challenge (transcript.rs:88-133): digest -> field element, Montgomery -----------------------------------------
// The reference maps the lo / hi u128 halves through FieldMap, which reads value AND modulus as signed integers of
// FL limbs: a modulus with its top bit set acts as 2^(64 FL) - q inside the `%` (the host mirror's from_signed_words).
// red_mod is that |modulus|; when the top bit is clear no reduction ever happens here (lo masked to num_bits - 1 bits
// is below q; with 129 bits or more, lo, hi and 2^128 are).  two128 = Montgomery form of 2^128 mod red_mod (FL >= 3).
template <int FL>
struct TrField {
    uint64_t modulus[FL], r2[FL], red_mod[FL], two128[FL];
    uint64_t inv;
    uint32_t cbits;      // num_bits - 1: the bits a challenge keeps
    uint32_t needs_mod;  // the modulus has no spare bit: values are reduced modulo red_mod first
};

template <int FL>
ZK_HD bool tr_geq(const uint64_t (&a)[FL], const uint64_t (&b)[FL]) {
#pragma unroll
    for (int i = FL - 1; i >= 0; i--)
        if (a[i] != b[i]) return a[i] > b[i];
    return true;
}
template <int FL>
ZK_HD uint64_t tr_sub(uint64_t (&a)[FL], const uint64_t (&b)[FL]) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < FL; i++) {
        const unsigned __int128 d = (unsigned __int128)a[i] - b[i] - borrow;
        a[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
    return borrow;
}
// a * b / R mod q, canonical, for a, b < q (any odd q of FL limbs, spare bit or not)
template <int FL>
ZK_HD void tr_mont_mul(const uint64_t (&a)[FL], const uint64_t (&b)[FL], const TrField<FL> &f, uint64_t (&out)[FL]) {
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
        const uint64_t m = t[0] * f.inv;
        x = (u128_t)m * f.modulus[0] + t[0];
        carry = (uint64_t)(x >> 64);
#pragma unroll
        for (int j = 1; j < FL; j++) {
            x = (u128_t)m * f.modulus[j] + t[j] + carry;
            t[j - 1] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        x = (u128_t)t[FL] + carry;
        t[FL - 1] = (uint64_t)x;
        t[FL] = t[FL + 1] + (uint64_t)(x >> 64);
    }
#pragma unroll
    for (int i = 0; i < FL; i++) out[i] = t[i];
    if (t[FL] || tr_geq<FL>(out, f.modulus)) tr_sub<FL>(out, f.modulus);
}
// the u128 (w0, w1) -> field, Montgomery (map_to_field for u128: conversion.rs:9-46)
template <int FL>
ZK_HD void tr_map_u128(const TrField<FL> &f, uint64_t w0, uint64_t w1, uint64_t (&out)[FL]) {
    uint64_t v[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) v[i] = i == 0 ? w0 : i == 1 ? w1 : 0;
    if (f.needs_mod) {  // v mod red_mod by binary long division over the 128 bits (red_mod < 2^(64 FL - 1): no overflow)
        uint64_t rem[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) rem[i] = 0;
#pragma unroll 1
        for (int bit = 0; bit < 128; bit++) {
            const uint64_t top = w1 >> 63;
            w1 = (w1 << 1) | (w0 >> 63);
            w0 <<= 1;
#pragma unroll
            for (int i = FL - 1; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
            rem[0] = (rem[0] << 1) | top;
            if (tr_geq<FL>(rem, f.red_mod)) tr_sub<FL>(rem, f.red_mod);
        }
#pragma unroll
        for (int i = 0; i < FL; i++) v[i] = rem[i];
    }
    tr_mont_mul<FL>(v, f.r2, f, out);
}
ZK_HD void tr_mask128(uint64_t &w0, uint64_t &w1, uint32_t keep) {
    if (keep < 64) {
        w0 &= ((uint64_t)1 << keep) - 1;
        w1 = 0;
    } else if (keep == 64) {
        w1 = 0;
    } else if (keep < 128) {
        w1 &= ((uint64_t)1 << (keep - 64)) - 1;
    }
}
// d[0..4): the first four state words after finalize (the 32 digest bytes, little-endian words)
template <int FL>
ZK_HD void tr_challenge(const TrField<FL> &f, const uint64_t *d, uint64_t (&out)[FL]) {
    // lo = u128::from_be_bytes(digest[0..16]), hi = u128::from_be_bytes(digest[16..32])   (transcript.rs:72-86)
    uint64_t lo0 = keccak_bswap64(d[1]), lo1 = keccak_bswap64(d[0]), hi0 = keccak_bswap64(d[3]), hi1 = keccak_bswap64(d[2]);
    if (f.cbits < 128) {
        tr_mask128(lo0, lo1, f.cbits);
        tr_map_u128<FL>(f, lo0, lo1, out);
        return;
    }
    if (f.cbits < 256) tr_mask128(hi0, hi1, f.cbits - 128);  // (exactly 128: the hi mask keeps nothing)
    uint64_t b[FL], t[FL];
    tr_map_u128<FL>(f, lo0, lo1, out);
    tr_map_u128<FL>(f, hi0, hi1, b);
    tr_mont_mul<FL>(f.two128, b, f, t);
    // out += t (mod q)
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < FL; i++) {
        const unsigned __int128 x = (unsigned __int128)out[i] + t[i] + carry;
        out[i] = (uint64_t)x;
        carry = (uint64_t)(x >> 64);
    }
    if (carry || tr_geq<FL>(out, f.modulus)) tr_sub<FL>(out, f.modulus);
}

// ---- the sponge on one thread (the library's host thread, for the rounds above the tail) --------------------------------
// The same representation and the same steps as sumcheck_tail_kernel: st after every full block, the pending bytes as
// the 17 words of the rate, tr_gather_word to place stream bytes -- the kernel spreads the 17 words over 17 lanes and
// puts barriers between the steps, this is its serial form.
struct TrSponge {
    uint64_t st[25];
    uint64_t blk[kKeccakRateWords];
    uint32_t buflen;
};
template <class Gen>
inline void tr_sponge_absorb(TrSponge &sp, Gen &&gen, uint32_t n) {
    uint32_t done = 0;
    while (done < n) {
        const uint32_t room = kKeccakRate - sp.buflen, take = room < n - done ? room : n - done;
        for (uint32_t w = 0; w < kKeccakRateWords; w++) sp.blk[w] |= tr_gather_word(gen, w, sp.buflen, take, done);
        sp.buflen += take;
        done += take;
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
// word `w` of the state a finalize of a COPY permutes: pad 0x01 .. 0x80 over the pending bytes (domain byte 0x01)
ZK_HD uint64_t tr_finalize_word(const uint64_t *st, const uint64_t *blk, uint32_t buflen, uint32_t w) {
    uint64_t v = st[w];
    if (w < kKeccakRateWords) v ^= blk[w];
    if (w == buflen / 8) v ^= (uint64_t)0x01 << (8 * (buflen % 8));
    if (w == kKeccakRateWords - 1) v ^= (uint64_t)0x80 << 56;
    return v;
}
// byte i of what get_challenge absorbs: 0x00 | digest | 0x01 (transcript.rs:72-86), then the challenge as a field element
template <int FL>
ZK_HD uint32_t tr_challenge_stream_byte(const uint64_t *modulus, const uint64_t *digest_words, const uint64_t *challenge, uint32_t i) {
    if (i == 0) return 0x00;
    if (i <= 32) return (uint32_t)(digest_words[(i - 1) / 8] >> (8 * ((i - 1) % 8))) & 0xffu;
    if (i == 33) return 0x01;
    return tr_field_stream_byte<FL>(modulus, challenge, i - 34);
}
template <int FL>
inline void tr_sponge_absorb_fields(TrSponge &sp, const TrField<FL> &f, const uint64_t *vals, uint32_t n) {
    tr_sponge_absorb(sp, [&](uint32_t i) { return tr_field_stream_byte<FL>(f.modulus, vals, i); }, n * (16 * FL + 4));
}
// one round of the verifier's side (sumcheck.rs:100-103): absorb_slice(message), get_challenge, absorb the challenge
template <int FL>
inline void tr_sponge_round(TrSponge &sp, const TrField<FL> &f, const uint64_t *msg, uint32_t ne, uint64_t (&r)[FL]) {
    tr_sponge_absorb_fields<FL>(sp, f, msg, ne);
    uint64_t tmp[25];
    for (uint32_t w = 0; w < 25; w++) tmp[w] = tr_finalize_word(sp.st, sp.blk, sp.buflen, w);
    keccak_f1600(tmp);
    tr_challenge<FL>(f, tmp, r);
    tr_sponge_absorb(sp, [&](uint32_t i) { return tr_challenge_stream_byte<FL>(f.modulus, tmp, r, i); }, 34 + 16 * FL + 4);
}

// TrField from the Montgomery constants of the modulus (r2 = R^2 mod q, inv = -q^-1 mod 2^64)
template <int FL>
inline TrField<FL> tr_make_field(const uint64_t *modulus, const uint64_t *r2, uint64_t inv) {
    TrField<FL> tf{};
    uint32_t bits = 0;
    for (int i = FL - 1; i >= 0 && !bits; i--)
        if (modulus[i]) bits = 64u * (uint32_t)i + 64u - (uint32_t)__builtin_clzll(modulus[i]);
    tf.cbits = bits - 1;
    tf.needs_mod = (uint32_t)(modulus[FL - 1] >> 63);
    tf.inv = inv;
    for (int i = 0; i < FL; i++) {
        tf.modulus[i] = tf.red_mod[i] = modulus[i];
        tf.r2[i] = r2[i];
    }
    if (tf.needs_mod) {  // 2^(64 FL) - q
        uint64_t zero[FL] = {};
        tr_sub<FL>(zero, tf.modulus);
        for (int i = 0; i < FL; i++) tf.red_mod[i] = zero[i];
    }
    if constexpr (FL >= 3) {  // 2^128 (mod red_mod when the modulus has no spare bit), Montgomery
        uint64_t w[FL] = {};
        if (tf.needs_mod) {
            bool is_one = tf.red_mod[0] == 1;
            for (int i = 1; i < FL; i++) is_one &= tf.red_mod[i] == 0;
            w[0] = is_one ? 0 : 1;
            for (int d = 0; d < 128; d++) {  // doubling modulo red_mod (< 2^(64 FL - 1): no overflow)
                for (int i = FL - 1; i > 0; i--) w[i] = (w[i] << 1) | (w[i - 1] >> 63);
                w[0] <<= 1;
                if (tr_geq<FL>(w, tf.red_mod)) tr_sub<FL>(w, tf.red_mod);
            }
        } else {
            w[2] = 1;
        }
        tr_mont_mul<FL>(w, tf.r2, tf, tf.two128);
    }
    return tf;
}

}  // namespace zipk
