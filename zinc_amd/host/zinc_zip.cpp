// Host side of the Zip commit/open path (see zinc_zip.hpp).  Only sequential, tiny work lives
// here; MultilinearZip::commit / open forward every O(n) loop to libzip_hip.so.
#include "zinc_zip.hpp"

#include <chrono>
#include <cstdio>

#include <algorithm>
#include <list>
#include <map>
#include <set>
#include <mutex>

#include <sys/mman.h>

namespace zinc {

namespace {
// Freed proof- / witness-sized blocks are kept (exact sizes recur from proof to proof; at most 4 GiB) instead of
// going back to the kernel: a fresh 383 MiB block costs as much in first-touch page faults as its PCIe transfer.
struct BigBlockCache {
    std::mutex mu;
    std::multimap<size_t, void *> blocks;
    size_t bytes = 0;
    std::set<void *> pinned;  // blocks registered with the HIP runtime (unregistered before they are freed)
};
BigBlockCache g_big;
void big_block_free(void *p) {  // g_big.mu held
    if (g_big.pinned.erase(p)) zip_host_unregister(p);
    std::free(p);
}
constexpr size_t kBigBlock = (size_t)16 << 20, kBigCacheCap = (size_t)4 << 30;
}  // namespace

void *byte_stream_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes >= kBigBlock) {
        {
            std::lock_guard<std::mutex> g(g_big.mu);
            auto it = g_big.blocks.find(bytes);
            if (it != g_big.blocks.end()) {
                p = it->second;
                g_big.blocks.erase(it);
                g_big.bytes -= bytes;
                return p;
            }
        }
        if (posix_memalign(&p, (size_t)2 << 20, bytes) != 0) throw std::bad_alloc();
#ifdef MADV_HUGEPAGE
        (void)madvise(p, bytes, MADV_HUGEPAGE);
#endif
        // pinned once, reused for every later proof of this size: the device then writes the proof straight into
        // it (ZINC_HOST_NO_PIN=1 keeps the blocks pageable)
        static const bool pin = std::getenv("ZINC_HOST_NO_PIN") == nullptr;
        if (pin && zip_host_register(p, bytes) == ZIP_OK) {
            std::lock_guard<std::mutex> g(g_big.mu);
            g_big.pinned.insert(p);
        }
        return p;
    }
    p = std::malloc(bytes ? bytes : 1);
    if (!p) throw std::bad_alloc();
    return p;
}

void byte_stream_free(void *p, size_t bytes) {
    if (p && bytes >= kBigBlock) {
        std::lock_guard<std::mutex> g(g_big.mu);
        if (g_big.bytes + bytes <= kBigCacheCap) {
            g_big.blocks.emplace(bytes, p);
            g_big.bytes += bytes;
            return;
        }
        big_block_free(p);
        return;
    }
    std::free(p);
}

void byte_stream_release_cache() {
    std::lock_guard<std::mutex> g(g_big.mu);
    for (auto &kv : g_big.blocks) big_block_free(kv.second);
    g_big.blocks.clear();
    g_big.bytes = 0;
}

using u128 = unsigned __int128;

// ============================================================================ Keccak-256
// sha3 crate `Keccak256` (src/transcript.rs:2): Keccak-f[1600], rate 136, domain byte 0x01.
static inline uint64_t rol64(uint64_t v, int n) { return (v << n) | (v >> (64 - n)); }

void Keccak256::permute(uint64_t a[25]) {
    static const uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
        0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
        0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
        0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
        0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    // theta, rho + pi, chi, iota with the 25 lanes in registers (lane (x, y) = a[x + 5y]; unrolled by a script from the
    // rotation table 0 1 62 28 27 / 36 44 6 55 20 / 3 10 43 25 39 / 41 45 15 21 8 / 18 2 61 56 14): four times the speed
    // of the loop form, and the transcript is on the critical path of every sumcheck round and every opening
    uint64_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8], a9 = a[9], a10 = a[10], a11 = a[11], a12 = a[12], a13 = a[13], a14 = a[14], a15 = a[15], a16 = a[16], a17 = a[17], a18 = a[18], a19 = a[19], a20 = a[20], a21 = a[21], a22 = a[22], a23 = a[23], a24 = a[24];
    for (int round = 0; round < 24; round++) {
        const uint64_t c0 = a0 ^ a5 ^ a10 ^ a15 ^ a20;
        const uint64_t c1 = a1 ^ a6 ^ a11 ^ a16 ^ a21;
        const uint64_t c2 = a2 ^ a7 ^ a12 ^ a17 ^ a22;
        const uint64_t c3 = a3 ^ a8 ^ a13 ^ a18 ^ a23;
        const uint64_t c4 = a4 ^ a9 ^ a14 ^ a19 ^ a24;
        const uint64_t d0 = c4 ^ rol64(c1, 1);
        const uint64_t d1 = c0 ^ rol64(c2, 1);
        const uint64_t d2 = c1 ^ rol64(c3, 1);
        const uint64_t d3 = c2 ^ rol64(c4, 1);
        const uint64_t d4 = c3 ^ rol64(c0, 1);
        const uint64_t b0 = (a0 ^ d0);
        const uint64_t b1 = rol64((a6 ^ d1), 44);
        const uint64_t b2 = rol64((a12 ^ d2), 43);
        const uint64_t b3 = rol64((a18 ^ d3), 21);
        const uint64_t b4 = rol64((a24 ^ d4), 14);
        const uint64_t b5 = rol64((a3 ^ d3), 28);
        const uint64_t b6 = rol64((a9 ^ d4), 20);
        const uint64_t b7 = rol64((a10 ^ d0), 3);
        const uint64_t b8 = rol64((a16 ^ d1), 45);
        const uint64_t b9 = rol64((a22 ^ d2), 61);
        const uint64_t b10 = rol64((a1 ^ d1), 1);
        const uint64_t b11 = rol64((a7 ^ d2), 6);
        const uint64_t b12 = rol64((a13 ^ d3), 25);
        const uint64_t b13 = rol64((a19 ^ d4), 8);
        const uint64_t b14 = rol64((a20 ^ d0), 18);
        const uint64_t b15 = rol64((a4 ^ d4), 27);
        const uint64_t b16 = rol64((a5 ^ d0), 36);
        const uint64_t b17 = rol64((a11 ^ d1), 10);
        const uint64_t b18 = rol64((a17 ^ d2), 15);
        const uint64_t b19 = rol64((a23 ^ d3), 56);
        const uint64_t b20 = rol64((a2 ^ d2), 62);
        const uint64_t b21 = rol64((a8 ^ d3), 55);
        const uint64_t b22 = rol64((a14 ^ d4), 39);
        const uint64_t b23 = rol64((a15 ^ d0), 41);
        const uint64_t b24 = rol64((a21 ^ d1), 2);
        a0 = b0 ^ (~b1 & b2);
        a1 = b1 ^ (~b2 & b3);
        a2 = b2 ^ (~b3 & b4);
        a3 = b3 ^ (~b4 & b0);
        a4 = b4 ^ (~b0 & b1);
        a5 = b5 ^ (~b6 & b7);
        a6 = b6 ^ (~b7 & b8);
        a7 = b7 ^ (~b8 & b9);
        a8 = b8 ^ (~b9 & b5);
        a9 = b9 ^ (~b5 & b6);
        a10 = b10 ^ (~b11 & b12);
        a11 = b11 ^ (~b12 & b13);
        a12 = b12 ^ (~b13 & b14);
        a13 = b13 ^ (~b14 & b10);
        a14 = b14 ^ (~b10 & b11);
        a15 = b15 ^ (~b16 & b17);
        a16 = b16 ^ (~b17 & b18);
        a17 = b17 ^ (~b18 & b19);
        a18 = b18 ^ (~b19 & b15);
        a19 = b19 ^ (~b15 & b16);
        a20 = b20 ^ (~b21 & b22);
        a21 = b21 ^ (~b22 & b23);
        a22 = b22 ^ (~b23 & b24);
        a23 = b23 ^ (~b24 & b20);
        a24 = b24 ^ (~b20 & b21);
        a0 ^= RC[round];
    }
    a[0] = a0;
    a[1] = a1;
    a[2] = a2;
    a[3] = a3;
    a[4] = a4;
    a[5] = a5;
    a[6] = a6;
    a[7] = a7;
    a[8] = a8;
    a[9] = a9;
    a[10] = a10;
    a[11] = a11;
    a[12] = a12;
    a[13] = a13;
    a[14] = a14;
    a[15] = a15;
    a[16] = a16;
    a[17] = a17;
    a[18] = a18;
    a[19] = a19;
    a[20] = a20;
    a[21] = a21;
    a[22] = a22;
    a[23] = a23;
    a[24] = a24;
}

void Keccak256::absorb_block(const uint8_t *blk) {
    for (int i = 0; i < 17; i++) {
        uint64_t w;
        std::memcpy(&w, blk + 8 * i, 8);  // little-endian host
        st_[i] ^= w;
    }
    permute(st_);
}

void Keccak256::update(const uint8_t *data, size_t len) {
    while (len) {
        const size_t take = std::min<size_t>(136 - buflen_, len);
        std::memcpy(buf_ + buflen_, data, take);
        buflen_ += (uint32_t)take;
        data += take;
        len -= take;
        if (buflen_ == 136) {
            absorb_block(buf_);
            buflen_ = 0;
        }
    }
}

std::array<uint8_t, 32> Keccak256::finalize() const {
    Keccak256 c = *this;
    std::memset(c.buf_ + c.buflen_, 0, 136 - c.buflen_);
    c.buf_[c.buflen_] ^= 0x01;
    c.buf_[135] ^= 0x80;
    c.absorb_block(c.buf_);
    std::array<uint8_t, 32> out;
    std::memcpy(out.data(), c.st_, 32);
    return out;
}

void Keccak256::export_state(zip_keccak_state *out) const {
    std::memcpy(out->st, st_, sizeof st_);
    std::memset(out->buf, 0, sizeof out->buf);
    std::memcpy(out->buf, buf_, buflen_);
    out->buflen = buflen_;
}

void Keccak256::import_state(const zip_keccak_state &in) {
    if (in.buflen >= 136) throw std::logic_error("Keccak256::import_state: buflen is not below the rate (136)");
    std::memcpy(st_, in.st, sizeof st_);
    std::memcpy(buf_, in.buf, in.buflen);
    buflen_ = in.buflen;
}

// ============================================================================ multi-limb helpers
namespace {

int cmp(const Limbs &a, const Limbs &b, uint32_t n) {
    for (uint32_t i = n; i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
bool add_in_place(Limbs &a, const Limbs &b, uint32_t n) {
    u128 c = 0;
    for (uint32_t i = 0; i < n; i++) {
        c += (u128)a[i] + b[i];
        a[i] = (uint64_t)c;
        c >>= 64;
    }
    return c != 0;
}
void sub_in_place(Limbs &a, const Limbs &b, uint32_t n) {
    uint64_t borrow = 0;
    for (uint32_t i = 0; i < n; i++) {
        const u128 d = (u128)a[i] - b[i] - borrow;
        a[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
}
bool is_zero(const Limbs &a, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (a[i]) return false;
    return true;
}
void negate(Limbs &a, uint32_t n) {  // two's complement
    uint64_t carry = 1;
    for (uint32_t i = 0; i < n; i++) {
        a[i] = ~a[i] + carry;
        carry = (carry && a[i] == 0) ? 1 : 0;
    }
}
uint32_t bit_length(const Limbs &a, uint32_t n) {
    for (uint32_t i = n; i-- > 0;)
        if (a[i]) return 64 * i + 64 - (uint32_t)__builtin_clzll(a[i]);
    return 0;
}
// a mod m for n-limb unsigned values (schoolbook shift-subtract; only used off the hot path)
Limbs umod(const Limbs &a, const Limbs &m, uint32_t n) {
    if (cmp(a, m, n) < 0) return a;
    Limbs r{};
    for (uint32_t b = bit_length(a, n); b-- > 0;) {
        const bool top = r[n - 1] >> 63;
        for (uint32_t i = n; i-- > 1;) r[i] = (r[i] << 1) | (r[i - 1] >> 63);
        r[0] = (r[0] << 1) | ((a[b / 64] >> (b % 64)) & 1);
        if (top || cmp(r, m, n) >= 0) sub_in_place(r, m, n);
    }
    return r;
}

// Tail shared by every FieldMap impl: the value and the MODULUS are read as signed Int<W>
// (F::I = Int<N>, src/field.rs:280), `%=` is crypto-bigint's Int::rem (|lhs| mod |rhs|, sign of
// lhs) and BigInt::from(Int) takes the magnitude (biginteger.rs:805-816); then times R^2.
Limbs from_signed_words(const FieldConfig &f, Limbs words) {
    const uint32_t n = f.limbs;
    if (words[n - 1] >> 63) negate(words, n);
    Limbs mod = f.modulus;
    if (mod[n - 1] >> 63) negate(mod, n);
    Limbs v = umod(words, mod, n);
    f.mul_assign(v, f.r2);
    return v;
}

}  // namespace

// ============================================================================ FieldConfig
FieldConfig FieldConfig::make(const uint64_t *modulus, uint32_t limbs) {
    if (limbs == 0 || limbs > kMaxLimbs || !(modulus[0] & 1)) throw std::logic_error("FieldConfig: bad modulus");
    FieldConfig f;
    f.limbs = limbs;
    for (uint32_t i = 0; i < limbs; i++) f.modulus[i] = modulus[i];
    f.modulus_has_spare_bit = (modulus[limbs - 1] >> 63) == 0;
    uint64_t inv = 1;  // config.rs:196-214
    for (int i = 0; i < 63; i++) {
        inv *= inv;
        inv *= modulus[0];
    }
    f.inv = 0 - inv;
    Limbs x{};
    x[0] = 1;
    auto dbl = [&](Limbs &v) {
        const bool top = v[limbs - 1] >> 63;
        for (uint32_t i = limbs; i-- > 1;) v[i] = (v[i] << 1) | (v[i - 1] >> 63);
        v[0] <<= 1;
        if (top || cmp(v, f.modulus, limbs) >= 0) sub_in_place(v, f.modulus, limbs);
    };
    for (uint32_t i = 0; i < 64 * limbs; i++) dbl(x);
    f.r = x;
    for (uint32_t i = 0; i < 64 * limbs; i++) dbl(x);
    f.r2 = x;
    return f;
}

void FieldConfig::reduce_modulus(Limbs &a, bool carry) const {
    if (modulus_has_spare_bit) {
        if (cmp(a, modulus, limbs) >= 0) sub_in_place(a, modulus, limbs);
    } else if (carry || cmp(a, modulus, limbs) >= 0) {
        sub_in_place(a, modulus, limbs);
    }
}

// mul_naive (biginteger.rs:448-464) then montgomery_reduction (:532-560)
void FieldConfig::mul_assign(Limbs &a, const Limbs &b) const {
    const uint32_t N = limbs;
    uint64_t t[2 * kMaxLimbs] = {0};
    for (uint32_t i = 0; i < N; i++) {
        uint64_t carry = 0;
        for (uint32_t j = 0; j < N; j++) {
            const u128 x = (u128)a[i] * b[j] + t[i + j] + carry;
            t[i + j] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        t[i + N] = carry;
    }
    uint64_t carry2 = 0;
    for (uint32_t i = 0; i < N; i++) {
        const uint64_t k = t[i] * inv;
        uint64_t carry = 0;
        for (uint32_t j = 0; j < N; j++) {
            const u128 x = (u128)k * modulus[j] + t[i + j] + carry;
            t[i + j] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        const u128 y = (u128)t[i + N] + carry + carry2;
        t[i + N] = (uint64_t)y;
        carry2 = (uint64_t)(y >> 64);
    }
    for (uint32_t i = 0; i < N; i++) a[i] = t[N + i];
    reduce_modulus(a, carry2 != 0);
}

void FieldConfig::add_assign(Limbs &a, const Limbs &b) const { reduce_modulus(a, add_in_place(a, b, limbs)); }

void FieldConfig::sub_assign(Limbs &a, const Limbs &b) const {
    if (cmp(b, a, limbs) > 0) add_in_place(a, modulus, limbs);
    sub_in_place(a, b, limbs);
}

void FieldConfig::neg(Limbs &a) const {
    if (is_zero(a, limbs)) return;
    Limbs t = modulus;
    sub_in_place(t, a, limbs);
    a = t;
}

Limbs FieldConfig::inverse(const Limbs &a) const {
    Limbs e = modulus, two{};
    two[0] = 2;
    sub_in_place(e, two, limbs);  // q - 2
    Limbs acc = r, base = a;
    for (uint32_t i = 0; i < 64 * limbs; i++) {
        if ((e[i / 64] >> (i % 64)) & 1) mul_assign(acc, base);
        const Limbs sq = base;
        mul_assign(base, sq);
    }
    return acc;
}

uint32_t FieldConfig::num_bits() const { return bit_length(modulus, limbs); }

zip_field FieldConfig::to_abi() const {
    zip_field z{};
    z.limbs = limbs;
    for (uint32_t i = 0; i < kMaxLimbs; i++) z.modulus[i] = i < limbs ? modulus[i] : 0;
    return z;
}

Limbs map_to_field(const FieldConfig &f, int64_t v) {
    Limbs w{};
    w[0] = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;  // Integer::abs
    Limbs r = from_signed_words(f, w);
    if (v < 0) f.neg(r);
    return r;
}

Limbs map_to_field_u128(const FieldConfig &f, uint64_t lo, uint64_t hi) {
    Limbs w{};
    w[0] = lo;
    if (f.limbs > 1) w[1] = hi;
    return from_signed_words(f, w);
}

std::vector<Limbs> build_eq_x_r(const FieldConfig &f, const Limbs *r, uint32_t nvars) {
    if (nvars == 0) throw std::logic_error("r length is 0");  // ArithErrors::InvalidParameters
    std::vector<Limbs> buf(2);
    buf[0] = f.r;  // F::one()
    f.sub_assign(buf[0], r[nvars - 1]);
    buf[1] = r[nvars - 1];
    for (uint32_t t = nvars - 1; t-- > 0;) {
        std::vector<Limbs> res(buf.size() * 2);
        for (size_t i = 0; i < res.size(); i++) {
            Limbs tmp = r[t];
            f.mul_assign(tmp, buf[i >> 1]);
            if (i & 1) {
                res[i] = tmp;
            } else {
                res[i] = buf[i >> 1];
                f.sub_assign(res[i], tmp);
            }
        }
        buf.swap(res);
    }
    return buf;
}

// ============================================================================ KeccakTranscript
std::vector<uint8_t> KeccakTranscript::get_random_bytes(size_t length) {
    std::vector<uint8_t> out;
    out.reserve(length + 32);
    for (int32_t counter = 0; out.size() < length; counter++) {
        Keccak256 tmp = hasher_;
        tmp.update({(uint8_t)(counter >> 24), (uint8_t)(counter >> 16), (uint8_t)(counter >> 8), (uint8_t)counter});
        const auto h = tmp.finalize();
        out.insert(out.end(), h.begin(), h.end());
    }
    out.resize(length);
    return out;
}

void KeccakTranscript::get_integer_challenge(uint32_t n_limbs, uint64_t *out) {
    for (uint32_t i = 0; i < n_limbs; i++) {
        const auto ch = get_random_bytes(8);
        hasher_.update({0x12});
        hasher_.update(ch.data(), 8);
        hasher_.update({0x34});
        uint64_t w;
        std::memcpy(&w, ch.data(), 8);  // u64::from_le_bytes
        out[i] = w;
    }
}

std::vector<int64_t> KeccakTranscript::get_integer_challenges_i64(size_t n) {
    std::vector<int64_t> v(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t w;
        get_integer_challenge(1, &w);
        v[i] = (int64_t)w;
    }
    return v;
}

static void to_be_bytes(const Limbs &v, uint32_t n, uint8_t *out) {
    for (uint32_t i = 0; i < n; i++)
        for (int b = 0; b < 8; b++) out[8 * (n - 1 - i) + (7 - b)] = (uint8_t)(v[i] >> (8 * b));
}

void KeccakTranscript::absorb_random_field(const FieldConfig &f, const Limbs &v) {
    uint8_t buf[8 * kMaxLimbs];
    hasher_.update({0x3});
    to_be_bytes(f.modulus, f.limbs, buf);
    hasher_.update(buf, 8 * f.limbs);
    hasher_.update({0x5});
    hasher_.update({0x1});
    to_be_bytes(v, f.limbs, buf);
    hasher_.update(buf, 8 * f.limbs);
    hasher_.update({0x3});
}

Limbs KeccakTranscript::get_challenge(const FieldConfig &f) {
    const auto ch = hasher_.finalize();  // get_challenge_limbs, transcript.rs:72-86
    auto be64 = [&](int off) {
        uint64_t w = 0;
        for (int b = 0; b < 8; b++) w = (w << 8) | ch[off + b];
        return w;
    };
    uint64_t lo0 = be64(8), lo1 = be64(0), hi0 = be64(24), hi1 = be64(16);
    hasher_.update({0x00});
    hasher_.update(ch.data(), 32);
    hasher_.update({0x01});

    const uint32_t cbits = f.num_bits() - 1;
    auto mask128 = [](uint64_t &w0, uint64_t &w1, uint32_t keep) {
        if (keep < 64) {
            w0 &= (1ULL << keep) - 1;
            w1 = 0;
        } else if (keep == 64) {
            w1 = 0;
        } else if (keep < 128) {
            w1 &= (1ULL << (keep - 64)) - 1;
        }
    };
    if (f.limbs == 1) return map_to_field_u128(f, lo0 & ((1ULL << cbits) - 1), 0);
    if (cbits < 128) {
        mask128(lo0, lo1, cbits);
        return map_to_field_u128(f, lo0, lo1);
    }
    if (cbits < 256) mask128(hi0, hi1, cbits - 128);
    Limbs w{};
    if (f.limbs > 2) w[2] = 1;  // BigInt::from_bits_le(bit 128)
    Limbs two128 = from_signed_words(f, w);
    Limbs a = map_to_field_u128(f, lo0, lo1);
    const Limbs b = map_to_field_u128(f, hi0, hi1);
    f.mul_assign(two128, b);
    f.add_assign(a, two128);
    return a;
}

namespace zip {

// ============================================================================ shuffle_seeded
// rand 0.9.2: StdRng = ChaCha12, seed_from_u64 = PCG32 expansion, SliceRandom::shuffle =
// IncreasingUniform Fisher-Yates with Canon's-method random_range.  Every piece pinned by published vectors
// (tests/golden/rand_vectors.json; the seed expansion directly through zinc_kat_seed_from_u64).
namespace {
struct ChaCha12 {
    uint32_t key[8];
    uint64_t counter = 0;
    uint32_t buf[16];
    int idx = 16;
    // rand_core::SeedableRng::seed_from_u64: PCG32 steps, the state advanced before each output
    static void seed_words(uint64_t state, uint32_t *out, int n) {
        for (int i = 0; i < n; i++) {
            state = state * 6364136223846793005ULL + 11634580027462260723ULL;
            const uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27), rot = (uint32_t)(state >> 59);
            out[i] = (xs >> rot) | (xs << ((32 - rot) & 31));
        }
    }
    explicit ChaCha12(uint64_t state) { seed_words(state, key, 8); }
    static inline uint32_t rotl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }
    void refill() {
        uint32_t s[16] = {0x61707865, 0x3320646e, 0x79622d32, 0x6b206574}, x[16];
        for (int i = 0; i < 8; i++) s[4 + i] = key[i];
        s[12] = (uint32_t)counter;
        s[13] = (uint32_t)(counter >> 32);
        s[14] = s[15] = 0;
        std::memcpy(x, s, sizeof x);
        auto qr = [&](int a, int b, int c, int d) {
            x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
            x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
            x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
            x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
        };
        for (int r = 0; r < 6; r++) {
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
        }
        for (int i = 0; i < 16; i++) buf[i] = x[i] + s[i];
        counter++;
        idx = 0;
    }
    uint32_t next_u32() {
        if (idx >= 16) refill();
        return buf[idx++];
    }
    uint32_t random_range(uint32_t bound) {
        const uint64_t m = (uint64_t)next_u32() * bound;
        uint32_t result = (uint32_t)(m >> 32);
        const uint32_t lo = (uint32_t)m;
        if (lo > (uint32_t)(0u - bound)) {
            const uint32_t hi2 = (uint32_t)(((uint64_t)next_u32() * bound) >> 32);
            result += (uint32_t)(lo + hi2 < lo);
        }
        return result;
    }
};
}  // namespace

void kat_seed_from_u64(uint64_t seed, uint32_t *words, uint32_t n_words) { ChaCha12::seed_words(seed, words, (int)n_words); }

std::vector<uint32_t> shuffle_seeded_perm(uint64_t seed, uint32_t len) {
    std::vector<uint32_t> perm(len);
    for (uint32_t i = 0; i < len; i++) perm[i] = i;
    if (len <= 1) return perm;
    ChaCha12 rng(seed);
    uint32_t n = 0, chunk = 0;
    uint8_t remaining = 1;  // IncreasingUniform::new(rng, 0)
    for (uint32_t i = 0; i < len; i++) {
        const uint32_t next_n = n + 1;
        uint8_t next_rem;
        if (remaining > 0) {
            next_rem = remaining - 1;
        } else {
            uint32_t product = next_n, current = next_n + 1;
            while (((uint64_t)product * current) >> 32 == 0) product *= current++;
            chunk = rng.random_range(product);
            next_rem = (uint8_t)(current - next_n - 1);
        }
        uint32_t j;
        if (next_rem == 0) {
            j = chunk;
        } else {
            j = chunk % next_n;
            chunk /= next_n;
        }
        remaining = next_rem;
        n = next_n;
        std::swap(perm[i], perm[j]);
    }
    return perm;
}

// ============================================================================ RaaCode
static uint64_t isqrt(uint64_t x) {
    uint64_t r = 0;
    for (int b = 31; b >= 0; b--) {
        const uint64_t t = r | (1ULL << b);
        if (t * t <= x) r = t;
    }
    return r;
}
static uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
static uint32_t ilog2(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }

RaaCode RaaCode::make(const LinearCodeSpec &spec, uint64_t poly_size, SeedSource &transcript) {
    RaaCode c;
    const uint32_t num_vars = ilog2(poly_size);
    c.row_len = (uint32_t)next_pow2(isqrt(1ULL << num_vars));  // code_raa.rs:43
    c.repetition_factor = spec.repetition_factor;
    c.num_column_opening = spec.num_column_opening;
    c.num_proximity_testing = spec.num_proximity_testing;
    // width assertion, code_raa.rs:53-72 (N = Int<1>: 64 bits, K = Int<4>: 256 bits)
    const uint32_t rep_log = ilog2(next_pow2(spec.repetition_factor));
    const uint32_t nv_even = (num_vars & 1) ? num_vars + 1 : num_vars;
    const uint32_t width = 64 + nv_even + 2 * rep_log;
    if (256 < width)
        throw std::logic_error("Cannot fit " + std::to_string(width) + "-bit wide codeword entries in 256 bits integers");
    c.perm_1_seed = transcript.get_u64();
    c.perm_2_seed = transcript.get_u64();
    return c;
}

// ============================================================================ PcsTranscript
void PcsTranscript::write_field_elements(const FieldConfig &f, const Limbs *elems, size_t n) {
    uint8_t be[8 * kMaxLimbs];
    for (size_t i = 0; i < n; i++) {
        fs_transcript.absorb_random_field(f, elems[i]);  // common_field_element
        to_be_bytes(elems[i], f.limbs, be);
        append(be, 8 * f.limbs);
    }
}

size_t PcsTranscript::squeeze_challenge_idx(const FieldConfig &f, size_t cap) {
    const Limbs ch = fs_transcript.get_challenge(f);
    return (size_t)(uint32_t)ch[0] % cap;  // first 4 little-endian bytes of the Montgomery value
}

// ============================================================================ MultilinearZip
static void check(zip_ctx *ctx, int32_t rc, const char *what) {
    if (rc == ZIP_OK) return;
    const std::string detail = ctx ? zip_ctx_last_error(ctx) : "";
    const std::string msg = std::string(what) + ": " + zip_strerror(rc) + (detail.empty() ? "" : " (" + detail + ")");
    if (rc == ZIP_ERR_SHAPE) throw std::logic_error(msg);  // the reference panics (assert_eq!)
    if (rc == ZIP_ERR_INVALID_PARAM) throw ZipError(ZipError::InvalidPcsParam, msg);
    throw ZipError(ZipError::Device, msg);
}

namespace {
struct CtxKey {
    int device;
    uint32_t num_vars, row_len, rep;
    uint64_t seed1, seed2;
    uint32_t tests;  // zip_ctx_set_proximity_tests of the ctx: two specs never share one
    bool operator==(const CtxKey &o) const {
        return device == o.device && num_vars == o.num_vars && row_len == o.row_len && rep == o.rep &&
               seed1 == o.seed1 && seed2 == o.seed2 && tests == o.tests;
    }
};
constexpr size_t kCtxCacheSize = 4;
constexpr uint32_t kMaxProximityTests = 8;  // zip_ctx_set_proximity_tests accepts 1 .. 8
std::mutex &ctx_cache_mu() {
    static std::mutex m;
    return m;
}
std::list<std::pair<CtxKey, std::shared_ptr<zip_ctx>>> &ctx_cache() {
    static std::list<std::pair<CtxKey, std::shared_ptr<zip_ctx>>> c;
    return c;
}

}  // namespace

MultilinearZipParams MultilinearZip::setup(uint64_t poly_size, const RaaCode &code, int device) {
    if (poly_size == 0 || (poly_size & (poly_size - 1))) throw std::logic_error("assertion failed: poly_size.is_power_of_two()");
    MultilinearZipParams pp;
    pp.num_vars = ilog2(poly_size);
    pp.num_rows = (uint32_t)next_pow2((1ULL << pp.num_vars) / code.row_len);  // structs.rs:82
    pp.linear_code = code;
    // The shim's job: expand the two seeds once (the reference re-runs the shuffle for every row).
    pp.perm1 = shuffle_seeded_perm(code.perm_1_seed, code.codeword_len());
    pp.perm2 = shuffle_seeded_perm(code.perm_2_seed, code.codeword_len());
    // cached device context for this (device, geometry, seeds)
    // (a count the device does not serve is open's and verify's to refuse, as the reference's errors are: the ctx of
    // such a spec, and of a one-row matrix, which has no test at all, is a one-test ctx)
    const uint32_t tests = pp.num_rows > 1 && code.num_proximity_testing >= 1 && code.num_proximity_testing <= kMaxProximityTests
                               ? code.num_proximity_testing : 1;
    const CtxKey key{device, pp.num_vars, code.row_len, code.repetition_factor, code.perm_1_seed, code.perm_2_seed, tests};
    {
        std::lock_guard<std::mutex> g(ctx_cache_mu());
        auto &cache = ctx_cache();
        for (auto it = cache.begin(); it != cache.end(); ++it) {
            if (it->first == key) {
                pp.ctx = it->second;
                cache.splice(cache.begin(), cache, it);  // most recently used first
                return pp;
            }
        }
    }
    zip_params zp{};
    zp.num_vars = pp.num_vars;
    zp.row_len = code.row_len;
    zp.num_rows = pp.num_rows;
    zp.codeword_len = code.codeword_len();
    zp.rep = code.repetition_factor;
    zp.n_limbs = 1;
    zp.k_limbs = 4;
    zp.m_limbs = 8;
    zp.perm1 = pp.perm1.data();
    zp.perm2 = pp.perm2.data();
    zp.device = device;
    zip_ctx *ctx = nullptr;
    check(nullptr, zip_ctx_create(&zp, &ctx), "zip_ctx_create");
    pp.ctx = std::shared_ptr<zip_ctx>(ctx, zip_ctx_destroy);
    if (tests != 1) check(ctx, zip_ctx_set_proximity_tests(ctx, tests), "zip_ctx_set_proximity_tests");
    {
        std::lock_guard<std::mutex> g(ctx_cache_mu());
        auto &cache = ctx_cache();
        cache.emplace_front(key, pp.ctx);
        while (cache.size() > kCtxCacheSize) cache.pop_back();
    }
    return pp;
}

void MultilinearZip::release_cached_contexts() {
    {
        std::lock_guard<std::mutex> g(ctx_cache_mu());
        ctx_cache().clear();
    }
    byte_stream_release_cache();   // and the host blocks kept for the next proof
    zip_release_cached_memory();   // and the device / pinned blocks of the per-proof handles
}

// validate_input (pcs/utils.rs:24-58)
static void validate_input(const char *function, uint32_t param_num_vars, uint32_t poly_num_vars, const size_t *point_len) {
    if (param_num_vars < poly_num_vars)
        throw ZipError(ZipError::InvalidPcsParam, std::string("Too many variates of poly to ") + function +
                                                      " (param supports variates up to " + std::to_string(param_num_vars) +
                                                      " but got " + std::to_string(poly_num_vars) + ")");
    if (point_len && *point_len != poly_num_vars)
        throw ZipError(ZipError::InvalidPcsParam, "Invalid point (expect point to have " + std::to_string(poly_num_vars) +
                                                      " variates but got " + std::to_string(*point_len) + ")");
}

static std::pair<MultilinearZipData, MultilinearZipCommitment> commit_impl(const MultilinearZipParams &pp,
                                                                          const int64_t *evals, size_t n_evals,
                                                                          uint32_t poly_num_vars, bool merkle) {
    validate_input("commit", pp.num_vars, poly_num_vars, nullptr);
    MultilinearZipCommitment comm;
    if (merkle) comm.roots.resize(pp.num_rows);
    zip_commitment *h = nullptr;
    check(pp.ctx.get(),
          zip_commit(pp.ctx.get(), evals, n_evals, ZIP_MEM_HOST, merkle ? 1 : 0,
                     merkle ? reinterpret_cast<uint8_t *>(comm.roots.data()) : nullptr, &h),
          "zip_commit");
    MultilinearZipData data;
    data.ctx = pp.ctx;
    data.handle = std::shared_ptr<zip_commitment>(h, zip_commitment_free);
    return {std::move(data), std::move(comm)};
}

std::pair<MultilinearZipData, MultilinearZipCommitment> MultilinearZip::commit(const MultilinearZipParams &pp,
                                                                               const int64_t *evals, size_t n_evals,
                                                                               uint32_t poly_num_vars) {
    return commit_impl(pp, evals, n_evals, poly_num_vars, true);
}

MultilinearZipData MultilinearZip::commit_no_merkle(const MultilinearZipParams &pp, const int64_t *evals, size_t n_evals,
                                                    uint32_t poly_num_vars) {
    return commit_impl(pp, evals, n_evals, poly_num_vars, false).first;
}

std::pair<std::vector<int64_t>, std::vector<uint32_t>> MultilinearZip::open_challenges(uint32_t num_rows, uint32_t codeword_len,
                                                                                      uint32_t num_column_opening,
                                                                                      uint32_t num_proximity_testing,
                                                                                      const FieldConfig &field,
                                                                                      PcsTranscript &transcript) {
    std::pair<std::vector<int64_t>, std::vector<uint32_t>> out;
    if (num_rows > 1) {  // prove_testing_phase, open_z.rs:100-113; verify_testing, verify_z.rs:66-77
        if (num_proximity_testing < 1 || num_proximity_testing > kMaxProximityTests)
            throw ZipError(ZipError::InvalidPcsParam, "num_proximity_testing " + std::to_string(num_proximity_testing) +
                                                          " is outside the supported range 1 .. " +
                                                          std::to_string(kMaxProximityTests) + " of the device path");
        out.first.reserve((size_t)num_proximity_testing * num_rows);
        for (uint32_t t = 0; t < num_proximity_testing; t++) {
            const auto c = transcript.fs_transcript.get_integer_challenges_i64(num_rows);
            out.first.insert(out.first.end(), c.begin(), c.end());
        }
    }
    out.second.resize(num_column_opening);
    for (auto &c : out.second) c = (uint32_t)transcript.squeeze_challenge_idx(field, codeword_len);  // open_z.rs:116-120
    return out;
}

void MultilinearZip::open(const MultilinearZipParams &pp, const int64_t *evals, size_t n_evals, uint32_t poly_num_vars,
                          const MultilinearZipData &commit_data, const Limbs *point, size_t point_len,
                          const FieldConfig &field, PcsTranscript &transcript) {
    validate_input("open", pp.num_vars, poly_num_vars, &point_len);
    const uint32_t row_len = pp.linear_code.row_len, num_rows = pp.num_rows, cw = pp.linear_code.codeword_len();
    if (n_evals != (size_t)row_len * num_rows) throw std::logic_error("evaluations do not fill the matrix");
    zip_ctx *ctx = pp.ctx.get();

    // ---- everything the transcript yields BEFORE the first absorb (write_integers and
    // write_merkle_proof never absorb: pcs_transcript.rs:115-135,198-211), in the reference's order
    // (the ctx of setup() carries the spec's count of proximity tests: the stream gets one u' per test)
    auto challenges = open_challenges(num_rows, cw, pp.linear_code.num_column_opening, pp.linear_code.num_proximity_testing,
                                      field, transcript);
    const std::vector<int64_t> &coeffs = challenges.first;   // [tests][num_rows]
    const std::vector<uint32_t> &cols = challenges.second;
    // left_point_to_tensor (pcs/utils.rs:279-292): eq over the LAST log2(num_rows) coordinates
    std::vector<uint64_t> q0;
    if (num_rows > 1) {
        const uint32_t lr = ilog2(num_rows);
        const auto eq = build_eq_x_r(field, point + (point_len - lr), lr);
        q0.resize((size_t)num_rows * field.limbs);
        for (uint32_t r = 0; r < num_rows; r++)
            for (uint32_t k = 0; k < field.limbs; k++) q0[(size_t)r * field.limbs + k] = eq[r][k];
    }
    // ---- one device call produces the whole stream of open() ----
    const zip_field zf = field.to_abi();
    const size_t len = zip_proof_len(ctx, (uint32_t)cols.size(), field.limbs);
    const size_t at = transcript.stream.size();
    transcript.stream.resize(at + len);  // uninitialised (ByteStream); the library's copy threads touch the pages
    check(ctx,
          zip_open(commit_data.handle.get(), evals, ZIP_MEM_HOST, coeffs.empty() ? nullptr : coeffs.data(), cols.data(),
                   (uint32_t)cols.size(), q0.empty() ? nullptr : q0.data(), &zf, transcript.stream.data() + at,
                   ZIP_MEM_HOST),
          "zip_open");
    // ---- write_field_elements absorbs each element of the evaluation row (pcs_transcript.rs:107-113);
    // the bytes are already in the stream, only the Fiat-Shamir state still has to follow
    const uint8_t *row_be = transcript.stream.data() + at + len - (size_t)row_len * field.limbs * 8;
    for (uint32_t c = 0; c < row_len; c++) {
        Limbs v{};
        const uint8_t *b = row_be + (size_t)c * field.limbs * 8;
        for (uint32_t i = 0; i < field.limbs; i++) {
            uint64_t w = 0;
            for (int k = 0; k < 8; k++) w = (w << 8) | b[8 * (field.limbs - 1 - i) + k];
            v[i] = w;
        }
        transcript.fs_transcript.absorb_random_field(field, v);
    }
}

static bool batch_path_enabled() {
    const char *e = std::getenv("ZIP_HIP_BATCH");  // (read per call: the tests flip it)
    return !(e && e[0] == '0' && !e[1]);
}

std::vector<std::pair<MultilinearZipData, MultilinearZipCommitment>> MultilinearZip::batch_commit(const MultilinearZipParams &pp,
                                                                                                 const PolyRef *polys,
                                                                                                 size_t n_polys) {
    std::vector<std::pair<MultilinearZipData, MultilinearZipCommitment>> out;
    if (!n_polys) return out;
    const uint32_t row_len = pp.linear_code.row_len, num_rows = pp.num_rows, cw = pp.linear_code.codeword_len();
    const size_t per = (size_t)row_len * num_rows;
    bool batched = batch_path_enabled() && cw <= 16384 && n_polys <= 65535 && (uint64_t)n_polys * num_rows <= 0xFFFFFFFFull;
    for (size_t i = 0; i < n_polys && batched; i++) batched = polys[i].n_evals == per && polys[i].num_vars <= pp.num_vars;
    if (!batched) {  // (also where the loop's own checks produce the reference's errors)
        for (size_t i = 0; i < n_polys; i++) out.push_back(commit(pp, polys[i].evals, polys[i].n_evals, polys[i].num_vars));
        return out;
    }
    // polynomial-major and contiguous is what the device call wants; the reference's callers hold separate Vecs
    bool contiguous = true;
    for (size_t i = 1; i < n_polys && contiguous; i++) contiguous = polys[i].evals == polys[i - 1].evals + per;
    IntVec packed;
    const int64_t *evals = polys[0].evals;
    if (!contiguous) {
        packed.resize(n_polys * per);
        for (size_t i = 0; i < n_polys; i++) std::memcpy(packed.data() + i * per, polys[i].evals, per * 8);
        evals = packed.data();
    }
    std::vector<uint8_t> roots(n_polys * (size_t)num_rows * 32);
    zip_batch *b = nullptr;
    check(pp.ctx.get(), zip_batch_commit(pp.ctx.get(), evals, n_polys * per, (uint32_t)n_polys, ZIP_MEM_HOST, roots.data(), &b),
          "zip_batch_commit");
    std::shared_ptr<zip_batch> batch(b, zip_batch_free);
    out.reserve(n_polys);
    for (size_t i = 0; i < n_polys; i++) {
        zip_commitment *h = nullptr;
        check(pp.ctx.get(), zip_batch_member(b, (uint32_t)i, &h), "zip_batch_member");
        MultilinearZipData data;
        data.ctx = pp.ctx;
        data.handle = std::shared_ptr<zip_commitment>(h, zip_commitment_free);
        data.batch = batch;
        data.batch_index = (uint32_t)i;
        MultilinearZipCommitment comm;
        comm.roots.resize(num_rows);
        std::memcpy(comm.roots.data(), roots.data() + i * (size_t)num_rows * 32, (size_t)num_rows * 32);
        out.emplace_back(std::move(data), std::move(comm));
    }
    return out;
}

void MultilinearZip::batch_open_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                           const FieldConfig &field, PcsTranscript &transcript, const uint64_t *eval_rows,
                                           size_t n_polys, int64_t *coeffs_out, uint32_t *cols_out) {
    for (size_t i = 0; i < n_polys; i++) {
        if (num_rows > 1) {  // prove_testing_phase, open_z.rs:100-113
            const auto coeffs = transcript.fs_transcript.get_integer_challenges_i64(num_rows);
            std::memcpy(coeffs_out + i * num_rows, coeffs.data(), (size_t)num_rows * 8);
        }
        for (uint32_t k = 0; k < n_cols; k++)  // open_z.rs:116-120
            cols_out[i * n_cols + k] = (uint32_t)transcript.squeeze_challenge_idx(field, codeword_len);
        const uint64_t *row = eval_rows + i * (size_t)row_len * field.limbs;
        for (uint32_t c = 0; c < row_len; c++) {  // write_field_elements' absorption, pcs_transcript.rs:107-113
            Limbs v{};
            for (uint32_t k = 0; k < field.limbs; k++) v[k] = row[(size_t)c * field.limbs + k];
            transcript.fs_transcript.absorb_random_field(field, v);
        }
    }
}

void MultilinearZip::batch_open(const MultilinearZipParams &pp, const PolyRef *polys, const MultilinearZipData *const *datas,
                                const Limbs *const *points, size_t n_polys, const FieldConfig &field, PcsTranscript &transcript) {
    if (!n_polys) return;
    const uint32_t row_len = pp.linear_code.row_len, num_rows = pp.num_rows, cw = pp.linear_code.codeword_len();
    zip_batch *b = datas[0]->batch.get();
    bool batched = batch_path_enabled() && b && zip_batch_size(b) == n_polys && pp.linear_code.num_proximity_testing == 1;
    for (size_t i = 0; i < n_polys && batched; i++)
        batched = datas[i]->batch.get() == b && datas[i]->batch_index == i && polys[i].num_vars == pp.num_vars &&
                  polys[i].n_evals == (size_t)row_len * num_rows;
    if (!batched) {
        for (size_t i = 0; i < n_polys; i++)
            open(pp, polys[i].evals, polys[i].n_evals, polys[i].num_vars, *datas[i], points[i], polys[i].num_vars, field, transcript);
        return;
    }
    zip_ctx *ctx = pp.ctx.get();
    const uint32_t fl = field.limbs, n_cols = pp.linear_code.num_column_opening;
    // left_point_to_tensor (pcs/utils.rs:279-292) per polynomial: the points differ
    std::vector<uint64_t> q0;
    if (num_rows > 1) {
        const uint32_t lr = ilog2(num_rows);
        q0.resize(n_polys * (size_t)num_rows * fl);
        for (size_t i = 0; i < n_polys; i++) {
            const auto eq = build_eq_x_r(field, points[i] + (pp.num_vars - lr), lr);
            for (uint32_t r = 0; r < num_rows; r++)
                for (uint32_t k = 0; k < fl; k++) q0[(i * num_rows + r) * fl + k] = eq[r][k];
        }
    }
    const zip_field zf = field.to_abi();
    // 1. every evaluation row: they depend on the witness and the point alone
    std::vector<uint64_t> rows(n_polys * (size_t)row_len * fl);
    check(ctx, zip_batch_open_eval(b, q0.empty() ? nullptr : q0.data(), &zf, rows.data(), ZIP_MEM_HOST), "zip_batch_open_eval");
    // 2. the shared transcript, in the reference's order
    std::vector<int64_t> coeffs(num_rows > 1 ? n_polys * (size_t)num_rows : 0);
    std::vector<uint32_t> cols(n_polys * (size_t)n_cols);
    batch_open_challenges(num_rows, row_len, cw, n_cols, field, transcript, rows.data(), n_polys, coeffs.data(), cols.data());
    // 3. every proof stream, straight into the transcript's stream
    const size_t len = zip_proof_len(ctx, n_cols, fl), at = transcript.stream.size();
    transcript.stream.resize(at + n_polys * len);
    check(ctx,
          zip_batch_open(b, coeffs.empty() ? nullptr : coeffs.data(), cols.data(), n_cols, q0.empty() ? nullptr : q0.data(), &zf,
                         transcript.stream.data() + at, ZIP_MEM_HOST),
          "zip_batch_open");
}

// point_to_tensor (pcs/utils.rs:252-276): q_0 over the last log2(num_rows) coordinates, q_1 over the rest;
// an empty half gives an EMPTY vector (MLE::zero()).
static void point_to_tensor(const FieldConfig &field, uint32_t num_rows, const Limbs *point, size_t point_len,
                            std::vector<uint64_t> &q0, std::vector<uint64_t> &q1) {
    const uint32_t lr = ilog2(num_rows);
    const size_t lc = point_len - lr;
    auto flat = [&](const std::vector<Limbs> &eq, std::vector<uint64_t> &out) {
        out.resize(eq.size() * field.limbs);
        for (size_t i = 0; i < eq.size(); i++)
            for (uint32_t k = 0; k < field.limbs; k++) out[i * field.limbs + k] = eq[i][k];
    };
    q0.clear();
    q1.clear();
    if (lr) flat(build_eq_x_r(field, point + lc, lr), q0);
    if (lc) flat(build_eq_x_r(field, point, (uint32_t)lc), q1);
}

// what MultilinearZip::verify returns for a verdict of the device (zip_verify_verdict): Ok(()), the reference's errors,
// a panic where it panics
static void throw_unless_accepted(int32_t verdict) {
    switch (verdict) {
        case ZIP_VERIFY_ACCEPT: return;
        case ZIP_VERIFY_PROXIMITY_TESTING:
        case ZIP_VERIFY_PROXIMITY_Q0: throw ZipError(ZipError::InvalidPcsOpen, "Proximity failure");
        case ZIP_VERIFY_EVAL_CONSISTENCY: throw ZipError(ZipError::InvalidPcsOpen, "Evaluation consistency failure");
        case ZIP_VERIFY_MERKLE: throw ZipError(ZipError::InvalidPcsOpen, "Merkle proof verification failed");
        case ZIP_VERIFY_OVERFLOW: throw std::logic_error("attempt to add with overflow (encode_wide of the combined row)");
        default: throw ZipError(ZipError::Transcript, "Failed to read the proof stream");
    }
}

// read_field_elements' absorption (pcs_transcript.rs:138-160): row_len big-endian elements, not range-checked
static void absorb_row_be(const FieldConfig &field, PcsTranscript &transcript, const uint8_t *row_be, uint32_t row_len) {
    for (uint32_t c = 0; c < row_len; c++) {
        Limbs v{};
        const uint8_t *b = row_be + (size_t)c * field.limbs * 8;
        for (uint32_t i = 0; i < field.limbs; i++) {
            uint64_t w = 0;
            for (int k = 0; k < 8; k++) w = (w << 8) | b[8 * (field.limbs - 1 - i) + k];
            v[i] = w;
        }
        transcript.fs_transcript.absorb_random_field(field, v);
    }
}

void MultilinearZip::verify(const MultilinearZipParams &vp, const MultilinearZipCommitment &comm, const Limbs *point,
                            size_t point_len, const Limbs &eval, PcsTranscript &transcript, const FieldConfig &field) {
    validate_input("verify", vp.num_vars, vp.num_vars, &point_len);
    const uint32_t row_len = vp.linear_code.row_len, num_rows = vp.num_rows, cw = vp.linear_code.codeword_len();
    if (comm.roots.size() != num_rows) throw ZipError(ZipError::InvalidPcsOpen, "commitment has the wrong number of roots");
    zip_ctx *ctx = vp.ctx.get();
    // the challenges in the order verify_testing draws them (verify_z.rs:69-90); reads never absorb
    auto challenges = open_challenges(num_rows, cw, vp.linear_code.num_column_opening, vp.linear_code.num_proximity_testing,
                                      field, transcript);
    const std::vector<int64_t> &coeffs = challenges.first;   // [tests][num_rows]
    const std::vector<uint32_t> &cols = challenges.second;
    std::vector<uint64_t> q0, q1;
    point_to_tensor(field, num_rows, point, point_len, q0, q1);
    const zip_field zf = field.to_abi();
    const size_t len = zip_proof_len(ctx, (uint32_t)cols.size(), field.limbs);
    const size_t avail = transcript.read_size() - transcript.read_pos;
    zip_verify_report rep{};
    check(ctx,
          zip_verify(ctx, comm.roots.empty() ? nullptr : comm.roots[0].data(), transcript.read_data() + transcript.read_pos,
                     ZIP_MEM_HOST, avail, coeffs.empty() ? nullptr : coeffs.data(), cols.data(), (uint32_t)cols.size(),
                     q0.empty() ? nullptr : q0.data(), q1.empty() ? nullptr : q1.data(), eval.data(), &zf, &rep),
          "zip_verify");
    throw_unless_accepted(rep.verdict);
    // read_field_elements absorbed every element of the evaluation row (pcs_transcript.rs:138-160)
    absorb_row_be(field, transcript, transcript.read_data() + transcript.read_pos + len - (size_t)row_len * field.limbs * 8, row_len);
    transcript.read_pos += len;
}

// One polynomial of the verifier's Fiat-Shamir walk: the squeezes of verify_testing (verify_z.rs:69-90), then -- `absorb`
// -- what read_field_elements absorbs, the evaluation row at the end of its stream.
static void verify_walk_one(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols, const FieldConfig &field,
                            PcsTranscript &transcript, const uint8_t *stream, size_t stream_len, bool absorb, int64_t *coeffs_out,
                            uint32_t *cols_out) {
    if (num_rows > 1) {
        const auto coeffs = transcript.fs_transcript.get_integer_challenges_i64(num_rows);
        if (coeffs_out) std::memcpy(coeffs_out, coeffs.data(), (size_t)num_rows * 8);
    }
    for (uint32_t k = 0; k < n_cols; k++) {
        const uint32_t c = (uint32_t)transcript.squeeze_challenge_idx(field, codeword_len);
        if (cols_out) cols_out[k] = c;
    }
    if (absorb) absorb_row_be(field, transcript, stream + stream_len - (size_t)row_len * field.limbs * 8, row_len);
}

void MultilinearZip::batch_verify_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                             const FieldConfig &field, PcsTranscript &transcript, const uint8_t *proofs,
                                             size_t stream_len, size_t n_polys, int64_t *coeffs_out, uint32_t *cols_out) {
    for (size_t i = 0; i < n_polys; i++)
        verify_walk_one(num_rows, row_len, codeword_len, n_cols, field, transcript, proofs + i * stream_len, stream_len, true,
                        num_rows > 1 ? coeffs_out + i * num_rows : nullptr, cols_out + i * n_cols);
}

void MultilinearZip::batch_verify_z(const MultilinearZipParams &vp, const MultilinearZipCommitment *const *comms,
                                    const Limbs *const *points, const size_t *point_lens, const Limbs *evals, size_t n_polys,
                                    PcsTranscript &transcript, const FieldConfig &field) {
    const uint32_t row_len = vp.linear_code.row_len, num_rows = vp.num_rows, cw = vp.linear_code.codeword_len();
    const uint32_t n_cols = vp.linear_code.num_column_opening, fl = field.limbs;
    bool batched = batch_path_enabled() && n_polys >= 2 && n_polys <= 65535 && cw <= 16384 &&
                   vp.linear_code.num_proximity_testing == 1 && (uint64_t)n_polys * n_cols <= 0xFFFFFFFFull;
    for (size_t i = 0; i < n_polys && batched; i++) batched = point_lens[i] == vp.num_vars && comms[i]->roots.size() == num_rows;
    if (!batched) {  // (also where the loop's own checks produce the reference's errors)
        for (size_t i = 0; i < n_polys; i++) verify(vp, *comms[i], points[i], point_lens[i], evals[i], transcript, field);
        return;
    }
    zip_ctx *ctx = vp.ctx.get();
    const size_t len = zip_proof_len(ctx, n_cols, fl);
    const uint8_t *proofs = transcript.read_data() + transcript.read_pos;
    // the polynomials whose streams are all there; the first one after them fails on a short stream, as in the loop
    const size_t k = std::min(n_polys, (transcript.read_size() - transcript.read_pos) / len);
    if (k) {
        // 1. the shared transcript, in the reference's order: needs no verdict (zip_hip.h, zip_batch_verify)
        const KeccakTranscript before = transcript.fs_transcript;
        std::vector<int64_t> coeffs(num_rows > 1 ? k * (size_t)num_rows : 0);
        std::vector<uint32_t> cols(k * (size_t)n_cols);
        batch_verify_challenges(num_rows, row_len, cw, n_cols, field, transcript, proofs, len, k, coeffs.data(), cols.data());
        // 2. point_to_tensor per polynomial (the points differ), roots and claimed evaluations polynomial-major
        std::vector<uint64_t> q0, q1, one0, one1, ev(k * (size_t)fl);
        std::vector<uint8_t> roots(k * (size_t)num_rows * 32);
        for (size_t i = 0; i < k; i++) {
            point_to_tensor(field, num_rows, points[i], point_lens[i], one0, one1);
            q0.insert(q0.end(), one0.begin(), one0.end());
            q1.insert(q1.end(), one1.begin(), one1.end());
            std::memcpy(roots.data() + i * (size_t)num_rows * 32, comms[i]->roots.data(), (size_t)num_rows * 32);
            for (uint32_t l = 0; l < fl; l++) ev[i * fl + l] = evals[i][l];
        }
        // 3. every proof in one launch set
        const zip_field zf = field.to_abi();
        std::vector<zip_verify_report> reps(k);
        check(ctx,
              zip_batch_verify(ctx, (uint32_t)k, roots.data(), proofs, ZIP_MEM_HOST, k * len, coeffs.empty() ? nullptr : coeffs.data(),
                               cols.data(), n_cols, q0.empty() ? nullptr : q0.data(), q1.empty() ? nullptr : q1.data(), ev.data(), &zf,
                               reps.data()),
              "zip_batch_verify");
        for (size_t i = 0; i < k; i++) {
            if (reps[i].verdict == ZIP_VERIFY_ACCEPT) continue;
            // the reference stops here: leave what the loop leaves -- polynomials 0 .. i-1 walked in full, the squeezes of
            // polynomial i, the cursor at the start of its stream -- and throw what verify throws
            transcript.fs_transcript = before;
            batch_verify_challenges(num_rows, row_len, cw, n_cols, field, transcript, proofs, len, i, coeffs.data(), cols.data());
            verify_walk_one(num_rows, row_len, cw, n_cols, field, transcript, proofs + i * len, len, false, nullptr, nullptr);
            transcript.read_pos += i * len;
            throw_unless_accepted(reps[i].verdict);
        }
        transcript.read_pos += k * len;
    }
    for (size_t i = k; i < n_polys; i++) verify(vp, *comms[i], points[i], point_lens[i], evals[i], transcript, field);
}

Limbs MultilinearZip::evaluate(const MultilinearZipParams &pp, const int64_t *evals, size_t n_evals, const Limbs *point,
                               size_t point_len, const FieldConfig &field) {
    if (point_len != pp.num_vars)
        throw ZipError(ZipError::InvalidPcsParam, "IncorrectLength: the point does not have num_vars coordinates");
    if (n_evals != (size_t)pp.linear_code.row_len * pp.num_rows) throw std::logic_error("evaluations do not fill the matrix");
    std::vector<uint64_t> q0, q1;
    point_to_tensor(field, pp.num_rows, point, point_len, q0, q1);
    const zip_field zf = field.to_abi();
    Limbs v{};
    check(pp.ctx.get(),
          zip_mle_eval(pp.ctx.get(), evals, ZIP_MEM_HOST, q0.empty() ? nullptr : q0.data(), q1.empty() ? nullptr : q1.data(),
                       &zf, v.data()),
          "zip_mle_eval");
    return v;
}

}  // namespace zip

namespace {
// ZINC_HOST_TIMING=1: stage times on stderr (tools/zinc_prover_times.py, tools/prover_pcs_step.py)
struct PcsStageTimer {
    bool on = std::getenv("ZINC_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[zinc]   pcs %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};
}  // namespace

zip::ZipProof zip::commit_z_mle_and_prove_evaluation(const LinearCodeSpec &lc_spec, const int64_t *z_evals, size_t m,
                                                     const Limbs *r_y, size_t r_y_len, KeccakTranscript &transcript,
                                                     const FieldConfig &config, int device) {
    PcsStageTimer timer;
    KeccakSeedSource seeds(transcript);
    const RaaCode linear_code = RaaCode::make(lc_spec, m, seeds);               // prover.rs:313
    const MultilinearZipParams param = MultilinearZip::setup(m, linear_code, device);  // :314
    timer.lap("RaaCode::new + setup");
    auto committed = MultilinearZip::commit(param, z_evals, m, param.num_vars);  // :315
    timer.lap("commit");
    PcsTranscript pcs_transcript;                                                // :316 (fresh)
    ZipProof out;
    {   // :317-319, z_mle.map_to_field(config).evaluate(r_y): over the witness the commit left on the device
        if (r_y_len != param.num_vars)
            throw ZipError(ZipError::InvalidPcsParam, "IncorrectLength: the point does not have num_vars coordinates");
        std::vector<uint64_t> q0, q1;
        point_to_tensor(config, param.num_rows, r_y, r_y_len, q0, q1);
        const zip_field zf = config.to_abi();
        check(param.ctx.get(),
              zip_commitment_mle_eval(committed.first.handle.get(), q0.empty() ? nullptr : q0.data(),
                                      q1.empty() ? nullptr : q1.data(), &zf, out.v.data()),
              "zip_commitment_mle_eval");
    }
    timer.lap("evaluate");
    MultilinearZip::open(param, z_evals, m, param.num_vars, committed.first, r_y, r_y_len, config, pcs_transcript);  // :320
    timer.lap("open");
    out.z_comm = std::move(committed.second);
    out.pcs_proof = pcs_transcript.into_proof();
    return out;
}

// The same for B proofs whose z fill one geometry, each with its own main transcript (hence its own RAA code: :313)
// and its own field: ONE zip_batch_commit_codes, ONE zip_batch_open_eval_fields, the walk of B fresh PcsTranscripts and
// v_i = <row_i, q1_i> on the host, ONE zip_batch_open_each that writes every stream into its ZipProof.  What is shared is the geometry, and with it the ctx
// (streams, pools) and the witness block; per member are the permutations (read by the commit alone), the field, the
// point, the challenges.  The caller has made sure of what the batch serves (one proximity test, codewords up to 8192,
// one limb count); everything a member's own step would throw is thrown here at the same member, in the same order.
std::vector<zip::ZipProof> zip::commit_z_mle_and_prove_evaluation_batch(const LinearCodeSpec &lc_spec, size_t m,
                                                                        const std::vector<PcsBatchMember> &members, int device) {
    const size_t B = members.size();
    std::vector<ZipProof> out(B);
    if (!B) return out;
    PcsStageTimer timer;
    // 1. per proof, in the reference's order: the code from its transcript, the two permutations, the point's tensors
    MultilinearZipParams param;
    std::vector<uint32_t> perms1, perms2;
    std::vector<uint64_t> q0_all;
    std::vector<std::vector<uint64_t>> q1(B);
    uint32_t cw = 0, fl = members[0].config->limbs;
    for (size_t i = 0; i < B; i++) {
        const PcsBatchMember &mb = members[i];
        KeccakSeedSource seeds(*mb.transcript);
        const RaaCode code = RaaCode::make(lc_spec, m, seeds);  // prover.rs:313
        if (i == 0) {
            param = MultilinearZip::setup(m, code, device);     // :314; the ctx of the geometry, cached like any other
            cw = code.codeword_len();
            perms1.resize(B * (size_t)cw);
            perms2.resize(B * (size_t)cw);
            std::memcpy(perms1.data(), param.perm1.data(), (size_t)cw * 4);
            std::memcpy(perms2.data(), param.perm2.data(), (size_t)cw * 4);
        } else {
            const auto p1 = shuffle_seeded_perm(code.perm_1_seed, cw), p2 = shuffle_seeded_perm(code.perm_2_seed, cw);
            std::memcpy(perms1.data() + i * cw, p1.data(), (size_t)cw * 4);
            std::memcpy(perms2.data() + i * cw, p2.data(), (size_t)cw * 4);
        }
        if (mb.r_y_len != param.num_vars)
            throw ZipError(ZipError::InvalidPcsParam, "IncorrectLength: the point does not have num_vars coordinates");
        std::vector<uint64_t> q0;
        point_to_tensor(*mb.config, param.num_rows, mb.r_y, mb.r_y_len, q0, q1[i]);
        q0_all.insert(q0_all.end(), q0.begin(), q0.end());
    }
    timer.lap("batch: codes + tensors");
    zip_ctx *ctx = param.ctx.get();
    const uint32_t num_rows = param.num_rows, row_len = param.linear_code.row_len, n_cols = param.linear_code.num_column_opening;
    // 2. one commit: the members' z, polynomial-major
    IntVec packed(B * m);
    for (size_t i = 0; i < B; i++) std::memcpy(packed.data() + i * m, members[i].z_evals, m * 8);
    std::vector<uint8_t> roots(B * (size_t)num_rows * 32);
    zip_batch *raw = nullptr;
    check(ctx, zip_batch_commit_codes(ctx, packed.data(), B * m, (uint32_t)B, ZIP_MEM_HOST, perms1.data(), perms2.data(), roots.data(), &raw),
          "zip_batch_commit_codes");
    std::shared_ptr<zip_batch> batch(raw, zip_batch_free);
    timer.lap("batch: commit");
    // 3. every evaluation row, each in its member's field
    std::vector<zip_field> zf(B);
    std::vector<const zip_field *> zfp(B);
    for (size_t i = 0; i < B; i++) {
        zf[i] = members[i].config->to_abi();
        zfp[i] = &zf[i];
    }
    const uint64_t *q0p = q0_all.empty() ? nullptr : q0_all.data();
    std::vector<uint64_t> rows(B * (size_t)row_len * fl);
    check(ctx, zip_batch_open_eval_fields(raw, q0p, zfp.data(), rows.data(), ZIP_MEM_HOST), "zip_batch_open_eval_fields");
    timer.lap("batch: evaluation rows");
    // 4. per proof: v = <row, q1> (:317-319; what zip_commitment_mle_eval computes -- a one-column matrix evaluates to its
    // entry), then the walk of a FRESH PcsTranscript (:316): coefficients, columns, the row's absorption
    std::vector<int64_t> coeffs(num_rows > 1 ? B * (size_t)num_rows : 0);
    std::vector<uint32_t> cols(B * (size_t)n_cols);
    std::vector<PcsTranscript> walks(B);
    for (size_t i = 0; i < B; i++) {
        const FieldConfig &f = *members[i].config;
        const uint64_t *row = rows.data() + i * (size_t)row_len * fl;
        Limbs v{};
        for (uint32_t c = 0; c < row_len; c++) {
            Limbs t{}, q = f.r;
            for (uint32_t k = 0; k < fl; k++) t[k] = row[(size_t)c * fl + k];
            if (row_len > 1)
                for (uint32_t k = 0; k < fl; k++) q[k] = q1[i][(size_t)c * fl + k];
            f.mul_assign(t, q);
            f.add_assign(v, t);
        }
        out[i].v = v;
        MultilinearZip::batch_open_challenges(num_rows, row_len, cw, n_cols, f, walks[i], row, 1,
                                              coeffs.empty() ? nullptr : coeffs.data() + i * num_rows, cols.data() + i * n_cols);
    }
    timer.lap("batch: v + transcripts");
    // 5. every proof stream in one call, each straight into its ZipProof (window by window: no block of B streams)
    const size_t len = zip_proof_len(ctx, n_cols, fl);
    std::vector<uint8_t *> dsts(B);
    for (size_t i = 0; i < B; i++) {
        out[i].z_comm.roots.resize(num_rows);
        std::memcpy(out[i].z_comm.roots.data(), roots.data() + i * (size_t)num_rows * 32, (size_t)num_rows * 32);
        out[i].pcs_proof.resize(len);
        dsts[i] = out[i].pcs_proof.data();
    }
    check(ctx, zip_batch_open_each(raw, coeffs.empty() ? nullptr : coeffs.data(), cols.data(), n_cols, q0p, zfp.data(), dsts.data(),
                                   ZIP_MEM_HOST, 0),
          "zip_batch_open_each");
    timer.lap("batch: open");
    return out;
}

namespace {
sumcheck::ProverOutput prove_as_subprotocol_impl(KeccakTranscript &transcript, const std::vector<const uint64_t *> &mles,
                                                 uint32_t nvars, uint32_t degree, const zip_sumcheck_comb *comb,
                                                 const FieldConfig &config, int device,
                                                 zip_mem_kind kind = ZIP_MEM_HOST, bool products = false) {
    sumcheck::ProverOutput out;
    // ZIP_HIP_SUMCHECK_ONECALL=1 (read per call: the tests flip it): the whole loop is ONE zip_sumcheck_prove call --
    // the library borrows the sponge, the tail of the rounds runs in one kernel (zip_hip.h).  Default (and =0): the
    // per-round loop with the transcript here, until the end-to-end legs say otherwise (profiles/sumcheck_onecall.md).
    const char *onecall_env = std::getenv("ZIP_HIP_SUMCHECK_ONECALL");
    const bool per_round = nvars == 0 || !(onecall_env && onecall_env[0] == '1' && !onecall_env[1]);
    if (per_round) {  // sumcheck.rs:64-76 (FIELD_LIMBS > 1: the u128 map); zip_sumcheck_prove absorbs them itself
        transcript.absorb_random_field(config, map_to_field_u128(config, nvars, 0));
        transcript.absorb_random_field(config, map_to_field_u128(config, degree, 0));
    }
    if (nvars == 0) return out;  // :77-92: empty proof
    const zip_field zf = config.to_abi();
    zip_sumcheck *raw = nullptr;
    // products: `comb` is a sum of products with no trailing factor, all of it in one handle (zip_hip.h)
    int32_t rc = (products ? zip_sumcheck_init_products : zip_sumcheck_init)(device, mles.data(), kind, (uint32_t)mles.size(), nvars,
                                                                             degree, comb, &zf, &raw);
    if (rc) throw ZipError(rc == ZIP_ERR_INVALID_PARAM ? ZipError::InvalidPcsParam : ZipError::Device,
                           std::string(products ? "zip_sumcheck_init_products: " : "zip_sumcheck_init: ") + zip_strerror(rc));
    std::unique_ptr<zip_sumcheck, void (*)(zip_sumcheck *)> s(raw, zip_sumcheck_free);
    if (!per_round) {
        zip_keccak_state st;
        transcript.export_state(&st);
        const size_t ne = degree + 1, fl = config.limbs;
        std::vector<uint64_t> msgs((size_t)nvars * ne * fl), rand((size_t)nvars * fl);
        rc = zip_sumcheck_prove(s.get(), &st, msgs.data(), rand.data());
        if (rc) throw ZipError(ZipError::Device, std::string("zip_sumcheck_prove: ") + zip_sumcheck_last_error(s.get()));
        transcript.import_state(st);
        for (uint32_t round = 0; round < nvars; round++) {
            std::vector<Limbs> msg(ne);
            for (size_t e = 0; e < ne; e++)
                for (size_t i = 0; i < fl; i++) msg[e][i] = msgs[((size_t)round * ne + e) * fl + i];
            out.proof.msgs.push_back(std::move(msg));
            Limbs r{};
            for (size_t i = 0; i < fl; i++) r[i] = rand[(size_t)round * fl + i];
            out.randomness.push_back(r);
        }
        return out;
    }
    std::vector<uint64_t> evals((size_t)(degree + 1) * config.limbs);
    Limbs r{};
    for (uint32_t round = 0; round < nvars; round++) {  // :97-106
        rc = zip_sumcheck_round(s.get(), round ? r.data() : nullptr, evals.data());
        if (rc) throw ZipError(ZipError::Device, std::string("zip_sumcheck_round: ") + zip_sumcheck_last_error(s.get()));
        std::vector<Limbs> msg(degree + 1);
        for (uint32_t e = 0; e <= degree; e++) {
            for (uint32_t i = 0; i < config.limbs; i++) msg[e][i] = evals[(size_t)e * config.limbs + i];
            transcript.absorb_random_field(config, msg[e]);  // absorb_slice
        }
        out.proof.msgs.push_back(std::move(msg));
        r = transcript.get_challenge(config);   // sample_round
        transcript.absorb_random_field(config, r);
        out.randomness.push_back(r);
    }
    return out;
}
}  // namespace

sumcheck::ProverOutput sumcheck::prove_as_subprotocol_product(KeccakTranscript &transcript,
                                                              const std::vector<const uint64_t *> &mles, uint32_t nvars,
                                                              uint32_t degree, const FieldConfig &config, int device) {
    return prove_as_subprotocol_impl(transcript, mles, nvars, degree, nullptr, config, device);
}

namespace {
zip_sumcheck_comb make_comb(size_t n_mles, const std::vector<Limbs> &c, const std::vector<std::vector<uint32_t>> &S,
                            const FieldConfig &config) {
    if (c.size() != S.size()) throw std::logic_error("ccs.c and ccs.S differ in length");
    zip_sumcheck_comb comb{};
    for (size_t t = 0; t < c.size(); t++) {
        bool zero = true;  // terms with a zero coefficient are skipped (zinc/utils.rs:80-82)
        for (uint32_t i = 0; i < config.limbs; i++) zero &= c[t][i] == 0;
        if (zero) continue;
        if (comb.n_terms == 8) throw ZipError(ZipError::InvalidPcsParam, "more than 8 non-zero CCS terms");
        for (uint32_t j : S[t]) {
            if (j >= n_mles) throw std::logic_error("index out of bounds: ccs.S refers to a missing MLE");
            comb.term_mask[comb.n_terms] |= 1u << j;
        }
        for (uint32_t i = 0; i < config.limbs; i++) comb.coeff[comb.n_terms][i] = c[t][i];
        comb.n_terms++;
    }
    if (comb.n_terms == 0) throw ZipError(ZipError::InvalidPcsParam, "no non-zero CCS term");
    return comb;
}
}  // namespace

sumcheck::ProverOutput sumcheck::prove_as_subprotocol_ccs(KeccakTranscript &transcript,
                                                          const std::vector<const uint64_t *> &mles, uint32_t nvars,
                                                          uint32_t degree, const std::vector<Limbs> &c,
                                                          const std::vector<std::vector<uint32_t>> &S,
                                                          const FieldConfig &config, int device) {
    const zip_sumcheck_comb comb = make_comb(mles.size(), c, S, config);
    return prove_as_subprotocol_impl(transcript, mles, nvars, degree, &comb, config, device);
}

namespace {
// ZIP_HIP_SUMCHECK_FUSED (read per call: the tests flip it): 1 = a sum of products that one handle can hold goes through
// zip_sumcheck_init_products, 0 = always the loop of one handle per product.  Unset: kSumcheckFusedDefault
// (profiles/sumcheck_products.md).
constexpr bool kSumcheckFusedDefault = true;
bool env_flag(const char *e, bool def) {
    if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
    return def;
}
}  // namespace

sumcheck::ProverOutput sumcheck::prove_as_subprotocol_products(
    KeccakTranscript &transcript, const std::vector<const uint64_t *> &mles, uint32_t nvars, uint32_t degree,
    const std::vector<std::pair<Limbs, std::vector<uint32_t>>> &products, const FieldConfig &config, int device) {
    const bool fused = env_flag(std::getenv("ZIP_HIP_SUMCHECK_FUSED"), kSumcheckFusedDefault);
    auto absorb_header = [&] {  // sumcheck.rs:64-76 (the one-handle path leaves it to prove_as_subprotocol_impl)
        transcript.absorb_random_field(config, map_to_field_u128(config, nvars, 0));
        transcript.absorb_random_field(config, map_to_field_u128(config, degree, 0));
    };
    if (nvars == 0 || products.empty()) absorb_header();
    ProverOutput out;
    if (nvars == 0) return out;
    if (products.empty()) {  // comb_fn == 0 (sumcheck/tests.rs:525-557): every round polynomial is the zero constant
        for (uint32_t round = 0; round < nvars; round++) {
            std::vector<Limbs> msg(degree + 1);
            for (const Limbs &e : msg) transcript.absorb_random_field(config, e);
            out.proof.msgs.push_back(std::move(msg));
            const Limbs r = transcript.get_challenge(config);
            transcript.absorb_random_field(config, r);
            out.randomness.push_back(r);
        }
        return out;
    }
    // the shape is checked before a path is chosen: both paths refuse the same polynomials in the same way.  One handle
    // holds <= 32 MLEs and <= 8 products of 1..4 DIFFERENT multiplicands (a mask cannot say "v0 * v0").
    bool admissible = mles.size() <= 32 && products.size() <= 8;
    for (const auto &[coeff, indices] : products) {
        if (indices.empty() || indices.size() > 4) {
            absorb_header();
            throw ZipError(ZipError::InvalidPcsParam, "a product needs 1..4 multiplicands");
        }
        uint32_t mask = 0;
        for (uint32_t j : indices) {
            if (j >= mles.size()) {
                absorb_header();
                throw std::logic_error("index out of bounds: a product refers to a missing MLE");
            }
            if (j < 32) {
                if ((mask >> j) & 1u) admissible = false;
                mask |= 1u << j;
            }
        }
    }
    if (fused && admissible) {
        zip_sumcheck_comb comb{};
        comb.n_terms = (uint32_t)products.size();
        for (size_t t = 0; t < products.size(); t++) {
            for (uint32_t j : products[t].second) comb.term_mask[t] |= 1u << j;
            for (uint32_t i = 0; i < config.limbs; i++) comb.coeff[t][i] = products[t].first[i];
        }
        return prove_as_subprotocol_impl(transcript, mles, nvars, degree, &comb, config, device, ZIP_MEM_HOST, true);
    }
    const zip_field zf = config.to_abi();
    absorb_header();  // the loop: one handle per product, each on its own stream; the round messages add up here
    struct Free {
        void operator()(zip_sumcheck *p) const { zip_sumcheck_free(p); }
    };
    std::vector<std::unique_ptr<zip_sumcheck, Free>> provers;
    for (const auto &[coeff, indices] : products) {
        std::vector<const uint64_t *> tables;  // (1..4 of them, all present: checked above)
        for (uint32_t j : indices) tables.push_back(mles[j]);
        zip_sumcheck_comb comb{};  // coeff * prod_{j < K-1} vals[j] * vals[K-1]
        comb.n_terms = 1;
        comb.term_mask[0] = (1u << (tables.size() - 1)) - 1u;
        for (uint32_t i = 0; i < config.limbs; i++) comb.coeff[0][i] = coeff[i];
        zip_sumcheck *raw = nullptr;
        const int32_t rc = zip_sumcheck_init(device, tables.data(), ZIP_MEM_HOST, (uint32_t)tables.size(), nvars, degree, &comb, &zf, &raw);
        if (rc) throw ZipError(rc == ZIP_ERR_INVALID_PARAM ? ZipError::InvalidPcsParam : ZipError::Device,
                               std::string("zip_sumcheck_init: ") + zip_strerror(rc));
        provers.emplace_back(raw);
    }
    std::vector<uint64_t> evals((size_t)(degree + 1) * config.limbs);
    Limbs r{};
    for (uint32_t round = 0; round < nvars; round++) {
        for (auto &p : provers)
            if (zip_sumcheck_round_begin(p.get(), round ? r.data() : nullptr))
                throw ZipError(ZipError::Device, std::string("zip_sumcheck_round_begin: ") + zip_sumcheck_last_error(p.get()));
        std::vector<Limbs> msg(degree + 1);
        for (auto &p : provers) {
            if (zip_sumcheck_round_end(p.get(), evals.data()))
                throw ZipError(ZipError::Device, std::string("zip_sumcheck_round_end: ") + zip_sumcheck_last_error(p.get()));
            for (uint32_t e = 0; e <= degree; e++) {
                Limbs t{};
                for (uint32_t i = 0; i < config.limbs; i++) t[i] = evals[(size_t)e * config.limbs + i];
                config.add_assign(msg[e], t);
            }
        }
        for (uint32_t e = 0; e <= degree; e++) transcript.absorb_random_field(config, msg[e]);
        out.proof.msgs.push_back(std::move(msg));
        r = transcript.get_challenge(config);
        transcript.absorb_random_field(config, r);
        out.randomness.push_back(r);
    }
    return out;
}

std::vector<sumcheck::ProverOutput> sumcheck::prove_as_subprotocol_batch(std::vector<BatchInstance> &instances, uint32_t nvars,
                                                                         uint32_t degree, int device) {
    std::vector<ProverOutput> out;
    auto one = [&](BatchInstance &b) {
        return b.ccs ? prove_as_subprotocol_ccs(*b.transcript, b.mles, nvars, degree, b.c, b.S, b.config, device)
                     : prove_as_subprotocol_product(*b.transcript, b.mles, nvars, degree, b.config, device);
    };
    // What zip_sumcheck_prove_batch serves: up to 65535 instances of one shape (the same number of tables and of limbs),
    // 1..16 variables.  Everything else, and ZIP_HIP_BATCH=0, is the loop.  So is a batch too small to beat the loop by
    // more than the loop's own spread (profiles/sumcheck_batch.md, host tables): one workgroup plays the streamed rounds
    // of an instance more slowly than the whole device plays them for the loop, so the line moves with num_vars -- from
    // 2 instances on up to 2^12, from 3 up to 2^14, from 6 up to 2^16 (the sizes between the measured ones take the
    // rule of the next larger one).
    const size_t B = instances.size();
    const size_t min_batch = nvars <= 12 ? 2 : nvars <= 14 ? 3 : 6;
    bool batched = zip::batch_path_enabled() && B >= min_batch && B <= 65535 && nvars >= 1 && nvars <= 16;
    for (size_t i = 0; i < B && batched; i++)
        batched = instances[i].mles.size() == instances[0].mles.size() && !instances[i].mles.empty() && instances[i].mles.size() <= 8 &&
                  instances[i].config.limbs == instances[0].config.limbs;
    if (batched) {
        const size_t ne = degree + 1, fl = instances[0].config.limbs;
        std::vector<zip_sumcheck_comb> combs(B);
        std::vector<zip_field> fields(B);
        std::vector<zip_keccak_state> states(B);
        std::vector<zip_sumcheck_instance> abi(B);
        for (size_t i = 0; i < B; i++) {
            BatchInstance &b = instances[i];
            if (b.ccs) combs[i] = make_comb(b.mles.size(), b.c, b.S, b.config);
            fields[i] = b.config.to_abi();
            b.transcript->export_state(&states[i]);
            abi[i] = {b.mles.data(), b.ccs ? &combs[i] : nullptr, &fields[i], &states[i]};
        }
        std::vector<uint64_t> msgs(B * nvars * ne * fl), rand(B * nvars * fl);
        const int32_t rc = zip_sumcheck_prove_batch(device, abi.data(), (uint32_t)B, ZIP_MEM_HOST, (uint32_t)instances[0].mles.size(), nvars,
                                                    degree, msgs.data(), rand.data());
        if (rc == ZIP_OK) {
            for (size_t i = 0; i < B; i++) {
                instances[i].transcript->import_state(states[i]);
                ProverOutput o;
                for (uint32_t round = 0; round < nvars; round++) {
                    std::vector<Limbs> msg(ne);
                    for (size_t e = 0; e < ne; e++)
                        for (size_t l = 0; l < fl; l++) msg[e][l] = msgs[((i * nvars + round) * ne + e) * fl + l];
                    o.proof.msgs.push_back(std::move(msg));
                    Limbs r{};
                    for (size_t l = 0; l < fl; l++) r[l] = rand[(i * nvars + round) * fl + l];
                    o.randomness.push_back(r);
                }
                out.push_back(std::move(o));
            }
            return out;
        }
        // a refusal leaves every transcript as it was: the loop then reports what is wrong the way it always did
        if (rc != ZIP_ERR_INVALID_PARAM && rc != ZIP_ERR_UNSUPPORTED)
            throw ZipError(ZipError::Device, std::string("zip_sumcheck_prove_batch: ") + zip_strerror(rc));
    }
    for (BatchInstance &b : instances) out.push_back(one(b));
    return out;
}

// ---------------------------------------------------------------------------- CCS
ccs::SparseMatrix ccs::SparseMatrix::from_coeffs(uint32_t n_rows, uint32_t n_cols,
                                                 const std::vector<std::vector<std::pair<int64_t, uint32_t>>> &coeffs) {
    if (coeffs.size() > n_rows) throw std::logic_error("more coefficient rows than n_rows");
    SparseMatrix M;
    M.n_rows = n_rows;
    M.n_cols = n_cols;
    M.row_ptr.assign(1, 0);
    for (uint32_t r = 0; r < n_rows; r++) {
        if (r < coeffs.size())
            for (const auto &[v, col] : coeffs[r]) {
                M.values.push_back(v);
                M.col_idx.push_back(col);
            }
        M.row_ptr.push_back((uint32_t)M.col_idx.size());
    }
    return M;
}

std::vector<int64_t> ccs::Statement_Z::get_z_vector(const std::vector<int64_t> &w) const {
    std::vector<int64_t> z;
    z.reserve(public_input.size() + w.size() + 1);
    z.insert(z.end(), public_input.begin(), public_input.end());
    z.push_back(1);
    z.insert(z.end(), w.begin(), w.end());
    return z;
}

// ---------------------------------------------------------------------------- ZincProver
IntVec ZincProver::get_z_ccs(const int64_t *x, size_t l, const int64_t *w, size_t w_len, size_t m) {
    const size_t len = l + 1 + w_len;
    IntVec z(len <= m ? m : len);  // prover.rs:230-232: resize(ccs.m) only when not longer
    if (l) std::memcpy(z.data(), x, l * 8);
    z[l] = 1;
    if (w_len) std::memcpy(z.data() + l + 1, w, w_len * 8);
    if (z.size() > len) std::memset(z.data() + len, 0, (z.size() - len) * 8);
    return z;
}

namespace {
// ZINC_HOST_TIMING=1: stage times of the prover on stderr (tools/zinc_prover_times.py)
struct StageTimer {
    bool on = std::getenv("ZINC_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[zinc] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};
void ccs_check(zip_ccs *h, int32_t rc, const char *what) {
    if (rc == ZIP_OK) return;
    const std::string msg = std::string(what) + ": " + (h ? zip_ccs_last_error(h) : zip_strerror(rc));
    if (rc == ZIP_ERR_SHAPE) throw std::logic_error(msg);  // the reference panics / LengthsNotEqual
    throw ZipError(rc == ZIP_ERR_INVALID_PARAM ? ZipError::InvalidPcsParam : ZipError::Device, msg);
}
const uint64_t *ccs_table(zip_ccs *h, zip_ccs_table_kind which, uint32_t index) {
    const uint64_t *p = nullptr;
    ccs_check(h, zip_ccs_table(h, which, index, &p), "zip_ccs_table");
    return p;
}
}  // namespace

namespace {
// the shape the reference's prover supports (see the header), checked before anything else of a proof; -> ccs.S
std::vector<std::vector<uint32_t>> spartan_shape(size_t n_matrices, const ccs::CCS_Z &ccs, size_t z_len) {
    if (ccs.s == 0 || ccs.s > 28 || ccs.m != ((size_t)1 << ccs.s) || ccs.n != ccs.m || ccs.s_prime != ccs.s)
        throw std::logic_error("assertion failed: rx.len() == num_rows (compute_eval_table_sparse): m == n == 2^s is required");
    if (n_matrices != ccs.t || ccs.S.size() != ccs.q || ccs.c.size() != ccs.q)
        throw std::logic_error("CCS sizes and the statement disagree");
    if (z_len > ccs.m) throw std::logic_error("LengthsNotEqual: M.n_cols != z.len()");
    std::vector<std::vector<uint32_t>> S(ccs.q);
    size_t pos = 0;
    for (size_t i = 0; i < ccs.q; i++) {
        if (ccs.c[i] == 0) throw ZipError(ZipError::InvalidPcsParam, "a zero CCS coefficient shifts the MLE list the combination function indexes");
        for (size_t j : ccs.S[i]) {
            if (j != pos++) throw ZipError(ZipError::InvalidPcsParam, "ccs.S must list the matrices 0..t-1 in order");
            S[i].push_back((uint32_t)j);
        }
    }
    if (pos != ccs.t) throw ZipError(ZipError::InvalidPcsParam, "ccs.S must list the matrices 0..t-1 in order");
    return S;
}
}  // namespace

PreparedCcs::PreparedCcs(const ccs::Statement_Z &statement, const ccs::CCS_Z &ccs, const FieldConfig &config, int device)
    : t_((uint32_t)ccs.t), s_((uint32_t)ccs.s), limbs_(config.limbs), modulus_(config.modulus), device_(device) {
    if (ccs.s == 0 || ccs.s > 28 || ccs.m != ((size_t)1 << ccs.s) || ccs.n != ccs.m || ccs.s_prime != ccs.s)
        throw std::logic_error("assertion failed: rx.len() == num_rows (compute_eval_table_sparse): m == n == 2^s is required");
    if (statement.constraints.size() != ccs.t) throw std::logic_error("CCS sizes and the statement disagree");
    const zip_field zf = config.to_abi();
    std::vector<zip_sparse_matrix> mats;
    for (const auto &M : statement.constraints) mats.push_back(M.to_abi());
    ccs_check(nullptr, zip_ccs_create(device, mats.data(), t_, s_, &zf, &h_), "zip_ccs_create");
}
PreparedCcs::PreparedCcs(const zip_sparse_matrix *matrices, uint32_t t, uint32_t s, const FieldConfig &config, int device)
    : t_(t), s_(s), limbs_(config.limbs), modulus_(config.modulus), device_(device) {
    const zip_field zf = config.to_abi();
    ccs_check(nullptr, zip_ccs_create(device, matrices, t, s, &zf, &h_), "zip_ccs_create");
}
PreparedCcs::~PreparedCcs() { zip_ccs_free(h_); }

std::pair<SpartanProof, std::vector<Limbs>> ZincProver::spartan_prove(const ccs::Statement_Z &statement,
                                                                      const int64_t *z_ccs, size_t z_len,
                                                                      KeccakTranscript &transcript, const ccs::CCS_Z &ccs,
                                                                      const FieldConfig &config, PreparedCcs *prepared) const {
    const std::vector<std::vector<uint32_t>> S = spartan_shape(statement.constraints.size(), ccs, z_len);
    const uint32_t s = (uint32_t)ccs.s, t = (uint32_t)ccs.t;
    StageTimer timer;
    std::unique_ptr<PreparedCcs> own;
    if (!prepared) {  // prepare_for_random_field_piop: ccs.map_to_field / statement.map_to_field
        own = std::make_unique<PreparedCcs>(statement, ccs, config, device_);
        prepared = own.get();
        timer.lap("PreparedCcs (zip_ccs_create)");
    } else if (prepared->t_ != t || prepared->s_ != s || prepared->limbs_ != config.limbs ||
               prepared->modulus_ != config.modulus || prepared->device_ != device_) {
        throw std::logic_error("the prepared CCS belongs to another circuit, field or device");
    }
    std::lock_guard<std::mutex> one_proof(prepared->mu_);
    zip_ccs *dev = prepared->h_;
    // z_ccs -> F_q (prover.rs:236); calculate_Mz_mles
    ccs_check(dev, zip_ccs_set_z(dev, z_ccs, z_len, ZIP_MEM_HOST), "zip_ccs_set_z");
    timer.lap("zip_ccs_set_z");

    SpartanProof proof;
    // ---- sumcheck_1 (prover.rs:242-259)
    transcript.absorb(reinterpret_cast<const uint8_t *>("beta_s"), 6);  // squeeze_beta_challenges, zinc/utils.rs:100-106
    std::vector<uint64_t> flat((size_t)s * config.limbs);
    for (uint32_t i = 0; i < s; i++) {
        const Limbs b = transcript.get_challenge(config);
        std::copy(b.begin(), b.begin() + config.limbs, flat.begin() + (size_t)i * config.limbs);
    }
    ccs_check(dev, zip_ccs_eq_table(dev, flat.data(), 0), "zip_ccs_eq_table");
    std::vector<const uint64_t *> g;  // prepare_lin_sumcheck_polynomial: [Mz_0 .. Mz_{t-1}, eq(beta)], degree d + 1
    for (uint32_t k = 0; k < t; k++) g.push_back(ccs_table(dev, ZIP_CCS_MZ, k));
    g.push_back(ccs_table(dev, ZIP_CCS_EQ, 0));
    std::vector<Limbs> c_f;
    for (int64_t c : ccs.c) c_f.push_back(map_to_field(config, c));  // CCS_Z::map_to_field, ccs_z.rs:147
    const zip_sumcheck_comb comb = make_comb(g.size(), c_f, S, config);
    auto sc1 = prove_as_subprotocol_impl(transcript, g, s, (uint32_t)ccs.d + 1, &comb, config, device_, ZIP_MEM_DEVICE);
    proof.linearization_sumcheck = std::move(sc1.proof);
    timer.lap("sumcheck_1");
    const std::vector<Limbs> &r_x = sc1.randomness;

    // ---- sumcheck_2 (prover.rs:261-303)
    transcript.absorb(reinterpret_cast<const uint8_t *>("gamma"), 5);  // squeeze_gamma_challenge, zinc/utils.rs:112-118
    const Limbs gamma = transcript.get_challenge(config);
    for (uint32_t i = 0; i < s; i++) std::copy(r_x[i].begin(), r_x[i].begin() + config.limbs, flat.begin() + (size_t)i * config.limbs);
    std::vector<uint64_t> vs((size_t)t * config.limbs);
    ccs_check(dev, zip_ccs_second_table(dev, flat.data(), gamma.data(), vs.data()), "zip_ccs_second_table");
    timer.lap("zip_ccs_second_table");
    const std::vector<const uint64_t *> two{ccs_table(dev, ZIP_CCS_SECOND, 0), ccs_table(dev, ZIP_CCS_Z_FIELD, 0)};
    auto sc2 = prove_as_subprotocol_impl(transcript, two, s, 2, nullptr, config, device_, ZIP_MEM_DEVICE);
    proof.second_sumcheck = std::move(sc2.proof);
    timer.lap("sumcheck_2");

    // ---- calculate_V_s (prover.rs:330-347), computed with the second table
    for (uint32_t k = 0; k < t; k++) {
        Limbs v{};
        for (uint32_t i = 0; i < config.limbs; i++) v[i] = vs[(size_t)k * config.limbs + i];
        proof.V_s.push_back(v);
    }
    return {std::move(proof), std::move(sc2.randomness)};
}

ZincProof ZincProver::prove(const ccs::Statement_Z &statement, const ccs::Witness_Z &wit, KeccakTranscript &transcript,
                            const ccs::CCS_Z &ccs, const FieldConfig &config, std::vector<Limbs> *r_y_out,
                            PreparedCcs *prepared) const {
    const IntVec z_ccs = get_z_ccs(statement, wit, ccs);
    return prove_z(statement, z_ccs.data(), z_ccs.size(), transcript, ccs, config, r_y_out, prepared);
}

ZincProof ZincProver::prove_z(const ccs::Statement_Z &statement, const int64_t *z_ccs, size_t z_len, KeccakTranscript &transcript,
                              const ccs::CCS_Z &ccs, const FieldConfig &config, std::vector<Limbs> *r_y_out,
                              PreparedCcs *prepared) const {
    auto [spartan_proof, r_y] = spartan_prove(statement, z_ccs, z_len, transcript, ccs, config, prepared);
    ZincProof out;
    out.spartan_proof = std::move(spartan_proof);
    StageTimer timer;
    out.zip_proof = pcs_step(z_ccs, z_len, ccs, r_y, transcript, config);
    timer.lap("commit_z_mle_and_prove_eval");
    if (r_y_out) *r_y_out = std::move(r_y);
    return out;
}

zip::ZipProof ZincProver::pcs_step(const int64_t *z_ccs, size_t z_len, const ccs::CCS_Z &ccs, const std::vector<Limbs> &r_y,
                                   KeccakTranscript &transcript, const FieldConfig &config) const {
    // commit_z_mle_and_prove_evaluation (prover.rs:305-327); z_mle = from_evaluations_slice(s_prime, z_ccs)
    const size_t n_mle = (size_t)1 << ccs.s_prime;
    IntVec padded;
    const int64_t *z_mle = z_ccs;
    if (z_len != n_mle) {
        padded.resize(n_mle);
        std::memcpy(padded.data(), z_ccs, std::min(z_len, n_mle) * 8);
        if (z_len < n_mle) std::memset(padded.data() + z_len, 0, (n_mle - z_len) * 8);
        z_mle = padded.data();
    }
    return zip::commit_z_mle_and_prove_evaluation(lc_spec_, z_mle, ccs.m, r_y.data(), r_y.size(), transcript, config, device_);
}

// ---- B proofs of one circuit (zip_ccs_batch + zip_sumcheck_prove_batch) -------------------------------------------------
namespace {
void ccs_batch_check(zip_ccs_batch *h, int32_t rc, const char *what) {
    if (rc == ZIP_OK) return;
    const std::string detail = h ? zip_ccs_batch_last_error(h) : "";
    const std::string msg = std::string(what) + ": " + (detail.empty() ? zip_strerror(rc) : detail);
    if (rc == ZIP_ERR_SHAPE) throw std::logic_error(msg);  // the reference panics / LengthsNotEqual
    throw ZipError(rc == ZIP_ERR_INVALID_PARAM ? ZipError::InvalidPcsParam : ZipError::Device, msg);
}
struct CcsBatchHandle {
    zip_ccs_batch *h = nullptr;
    ~CcsBatchHandle() { zip_ccs_batch_free(h); }
};
// From how many instances on the batch is taken: where it beat the loop over spartan_prove by more than the loop's own
// spread (profiles/spartan_batch.md, t = 3, 4 limbs).  2 proofs win at 2^10 and 2^12 (1.31x, 1.12x) and lose at 2^14 and
// 2^16 (0.84x, 0.47x); 3 win at 2^14 (1.34x); at 2^16 3 and 4 lose (0.76x, 0.98x) and 6 win (1.48x).  The batch costs what
// its two batch sumchecks cost -- one workgroup plays an instance's streamed rounds more slowly than the whole device
// plays them for the loop -- so the line is prove_as_subprotocol_batch's; a size between the measured ones takes the rule
// of the next larger one.
// ZIP_HIP_SPARTAN_MIN_BATCH=n (n >= 2, read per call) puts the line at n for every size: how tools/spartan_batch_times.py
// measures the batch below the line.
size_t min_spartan_batch(size_t s) {
    if (const char *e = std::getenv("ZIP_HIP_SPARTAN_MIN_BATCH")) {
        const long n = std::atol(e);
        if (n >= 2) return (size_t)n;
    }
    return s <= 12 ? 2 : s <= 14 ? 3 : 6;
}
}  // namespace

std::vector<ZincProver::SpartanOutput> ZincProver::spartan_prove_batch(const ccs::Statement_Z &statement, const ccs::CCS_Z &ccs,
                                                                       const std::vector<ZVector> &zs,
                                                                       const std::vector<KeccakTranscript *> &transcripts,
                                                                       const std::vector<FieldConfig> &configs) const {
    if (statement.constraints.size() != ccs.t) throw std::logic_error("CCS sizes and the statement disagree");
    std::vector<zip_sparse_matrix> mats;
    for (const auto &M : statement.constraints) mats.push_back(M.to_abi());
    return spartan_prove_batch(mats.data(), ccs, zs, transcripts, configs);
}

std::vector<ZincProver::SpartanOutput> ZincProver::spartan_prove_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs,
                                                                       const std::vector<ZVector> &zs,
                                                                       const std::vector<KeccakTranscript *> &transcripts,
                                                                       const std::vector<FieldConfig> &configs) const {
    const size_t B = zs.size();
    if (transcripts.size() != B || configs.size() != B) throw std::logic_error("spartan_prove_batch: one transcript and one field per z");
    if (!matrices && B) throw std::logic_error("spartan_prove_batch: no matrices");
    // every shape check of spartan_prove on every instance, before any transcript is touched
    std::vector<std::vector<uint32_t>> S;
    for (size_t i = 0; i < B; i++) {
        if (!transcripts[i] || (!zs[i].z && zs[i].len)) throw std::logic_error("spartan_prove_batch: a NULL transcript or z");
        S = spartan_shape(ccs.t, ccs, zs[i].len);
    }
    const uint32_t s = (uint32_t)ccs.s, t = (uint32_t)ccs.t;
    bool batched = zip::batch_path_enabled() && B >= 2 && B >= min_spartan_batch(s) && B <= 65535 && s <= 16;
    for (size_t i = 1; i < B && batched; i++) batched = configs[i].limbs == configs[0].limbs;
    std::vector<SpartanOutput> out;
    if (!batched) {
        ccs::Statement_Z st;
        st.constraints.resize(t);  // the matrices go to the device straight from the caller's arrays
        for (size_t i = 0; i < B; i++) {  // per proof, as the reference maps the matrices per proof
            PreparedCcs prep(matrices, t, s, configs[i], device_);
            out.push_back(spartan_prove(st, zs[i].z, zs[i].len, *transcripts[i], ccs, configs[i], &prep));
        }
        return out;
    }
    const uint32_t fl = configs[0].limbs;
    StageTimer timer;
    CcsBatchHandle dev;
    ccs_batch_check(nullptr, zip_ccs_batch_create(device_, matrices, t, s, fl, (uint32_t)B, &dev.h), "zip_ccs_batch_create");
    timer.lap("zip_ccs_batch_create");
    std::vector<zip_field> fields(B);
    std::vector<const zip_field *> field_ptrs(B);
    std::vector<const int64_t *> z_ptrs(B);
    std::vector<size_t> z_lens(B);
    for (size_t i = 0; i < B; i++) {
        fields[i] = configs[i].to_abi();
        field_ptrs[i] = &fields[i];
        z_ptrs[i] = zs[i].z;
        z_lens[i] = zs[i].len;
    }
    // z_ccs -> F_q (prover.rs:236); calculate_Mz_mles -- of every proof
    ccs_batch_check(dev.h, zip_ccs_batch_set_z(dev.h, field_ptrs.data(), z_ptrs.data(), z_lens.data(), (uint32_t)B, ZIP_MEM_HOST),
                    "zip_ccs_batch_set_z");
    timer.lap("zip_ccs_batch_set_z");
    auto table = [&](size_t i, zip_ccs_table_kind which, uint32_t index) {
        const uint64_t *p = nullptr;
        ccs_batch_check(dev.h, zip_ccs_batch_table(dev.h, (uint32_t)i, which, index, &p), "zip_ccs_batch_table");
        return p;
    };
    // one zip_sumcheck_prove_batch over device tables; the transcripts travel as sponge states and come back
    auto sumcheck = [&](const std::vector<std::vector<const uint64_t *>> &tables, uint32_t degree, const std::vector<zip_sumcheck_comb> *combs) {
        const size_t ne = degree + 1;
        std::vector<zip_keccak_state> states(B);
        std::vector<zip_sumcheck_instance> abi(B);
        for (size_t i = 0; i < B; i++) {
            transcripts[i]->export_state(&states[i]);
            abi[i] = {tables[i].data(), combs ? &(*combs)[i] : nullptr, &fields[i], &states[i]};
        }
        std::vector<uint64_t> msgs(B * s * ne * fl), rand(B * s * fl);
        const int32_t rc = zip_sumcheck_prove_batch(device_, abi.data(), (uint32_t)B, ZIP_MEM_DEVICE, (uint32_t)tables[0].size(), s, degree,
                                                    msgs.data(), rand.data());
        if (rc != ZIP_OK) throw ZipError(rc == ZIP_ERR_INVALID_PARAM ? ZipError::InvalidPcsParam : ZipError::Device,
                                         std::string("zip_sumcheck_prove_batch: ") + zip_strerror(rc));
        std::vector<sumcheck::ProverOutput> res(B);
        for (size_t i = 0; i < B; i++) {
            transcripts[i]->import_state(states[i]);
            for (uint32_t round = 0; round < s; round++) {
                std::vector<Limbs> msg(ne);
                for (size_t e = 0; e < ne; e++)
                    for (size_t l = 0; l < fl; l++) msg[e][l] = msgs[((i * s + round) * ne + e) * fl + l];
                res[i].proof.msgs.push_back(std::move(msg));
                Limbs r{};
                for (size_t l = 0; l < fl; l++) r[l] = rand[(i * s + round) * fl + l];
                res[i].randomness.push_back(r);
            }
        }
        return res;
    };

    // ---- sumcheck_1 (prover.rs:242-259)
    std::vector<uint64_t> flat(B * s * fl);
    for (size_t i = 0; i < B; i++) {
        transcripts[i]->absorb(reinterpret_cast<const uint8_t *>("beta_s"), 6);  // squeeze_beta_challenges
        for (uint32_t j = 0; j < s; j++) {
            const Limbs b = transcripts[i]->get_challenge(configs[i]);
            std::copy(b.begin(), b.begin() + fl, flat.begin() + (i * s + j) * fl);
        }
    }
    ccs_batch_check(dev.h, zip_ccs_batch_eq_tables(dev.h, flat.data(), 0), "zip_ccs_batch_eq_tables");
    std::vector<std::vector<const uint64_t *>> g(B);  // prepare_lin_sumcheck_polynomial: [Mz_0 .. Mz_{t-1}, eq(beta)], degree d + 1
    std::vector<zip_sumcheck_comb> combs(B);
    for (size_t i = 0; i < B; i++) {
        for (uint32_t k = 0; k < t; k++) g[i].push_back(table(i, ZIP_CCS_MZ, k));
        g[i].push_back(table(i, ZIP_CCS_EQ, 0));
        std::vector<Limbs> c_f;
        for (int64_t c : ccs.c) c_f.push_back(map_to_field(configs[i], c));  // CCS_Z::map_to_field, ccs_z.rs:147
        combs[i] = make_comb(g[i].size(), c_f, S, configs[i]);
    }
    timer.lap("beta, zip_ccs_batch_eq_tables");
    auto sc1 = sumcheck(g, (uint32_t)ccs.d + 1, &combs);
    timer.lap("sumcheck_1 (batch)");

    // ---- sumcheck_2 (prover.rs:261-303)
    std::vector<uint64_t> gammas(B * fl), vs(B * t * fl);
    for (size_t i = 0; i < B; i++) {
        transcripts[i]->absorb(reinterpret_cast<const uint8_t *>("gamma"), 5);  // squeeze_gamma_challenge
        const Limbs gamma = transcripts[i]->get_challenge(configs[i]);
        std::copy(gamma.begin(), gamma.begin() + fl, gammas.begin() + i * fl);
        for (uint32_t j = 0; j < s; j++)
            std::copy(sc1[i].randomness[j].begin(), sc1[i].randomness[j].begin() + fl, flat.begin() + (i * s + j) * fl);
    }
    ccs_batch_check(dev.h, zip_ccs_batch_second_tables(dev.h, flat.data(), gammas.data(), vs.data()), "zip_ccs_batch_second_tables");
    timer.lap("gamma, zip_ccs_batch_second_tables");
    std::vector<std::vector<const uint64_t *>> two(B);
    for (size_t i = 0; i < B; i++) two[i] = {table(i, ZIP_CCS_SECOND, 0), table(i, ZIP_CCS_Z_FIELD, 0)};
    auto sc2 = sumcheck(two, 2, nullptr);
    timer.lap("sumcheck_2 (batch)");

    for (size_t i = 0; i < B; i++) {
        SpartanProof proof;
        proof.linearization_sumcheck = std::move(sc1[i].proof);
        proof.second_sumcheck = std::move(sc2[i].proof);
        for (uint32_t k = 0; k < t; k++) {  // calculate_V_s (prover.rs:330-347), computed with the second table
            Limbs v{};
            for (uint32_t l = 0; l < fl; l++) v[l] = vs[(i * t + k) * fl + l];
            proof.V_s.push_back(v);
        }
        out.emplace_back(std::move(proof), std::move(sc2[i].randomness));
    }
    return out;
}

std::vector<ZincProof> ZincProver::prove_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs, const std::vector<ZVector> &zs,
                                               const std::vector<KeccakTranscript *> &transcripts,
                                               const std::vector<FieldConfig> &configs, std::vector<std::vector<Limbs>> *r_y_out) const {
    auto spartan = spartan_prove_batch(matrices, ccs, zs, transcripts, configs);
    std::vector<std::vector<Limbs>> r_y(zs.size());
    for (size_t i = 0; i < zs.size(); i++) r_y[i] = std::move(spartan[i].second);
    StageTimer timer;
    auto zip_proofs = pcs_step_batch(ccs, zs, r_y, transcripts, configs);
    timer.lap("pcs_step_batch");
    std::vector<ZincProof> out(zs.size());
    for (size_t i = 0; i < zs.size(); i++) {
        out[i].spartan_proof = std::move(spartan[i].first);
        out[i].zip_proof = std::move(zip_proofs[i]);
    }
    if (r_y_out) *r_y_out = std::move(r_y);
    return out;
}

namespace {
// From how many proofs on the PCS step is taken as one batch.  The rule is the profile's: where the batch beats the loop
// over pcs_step by more than the loop's own spread.  profiles/pcs_step_batch.md measured the batch with the ONE-BLOCK
// delivery (zip_batch_open_fields into a block of B streams, cut afterwards): it won once, 256 proofs at 2^10 rows
// (1.41x), and lost everywhere else.  Step 5 now delivers per member (zip_batch_open_each), and that table no longer
// describes what would run; a table of the new delivery has not been measured.  Until
// one exists there is NO line: the default is the loop at every size, so no default path runs on an unmeasured number.
// ZIP_HIP_PCS_MIN_BATCH=n (n >= 2, read per call) puts the line at n for every size: how tools/pcs_batch_times.py measures
// the batch, and how the tests run it.
size_t min_pcs_batch(size_t s_prime) {
    if (const char *e = std::getenv("ZIP_HIP_PCS_MIN_BATCH")) {
        const long n = std::atol(e);
        if (n >= 2) return (size_t)n;
    }
    (void)s_prime;
    return SIZE_MAX;
}
}  // namespace

std::vector<zip::ZipProof> ZincProver::pcs_step_batch(const ccs::CCS_Z &ccs, const std::vector<ZVector> &zs,
                                                      const std::vector<std::vector<Limbs>> &r_y,
                                                      const std::vector<KeccakTranscript *> &transcripts,
                                                      const std::vector<FieldConfig> &configs) const {
    const size_t B = zs.size();
    if (r_y.size() != B || transcripts.size() != B || configs.size() != B)
        throw std::logic_error("pcs_step_batch: one point, one transcript and one field per z");
    // the geometry RaaCode::make will give every member (code_raa.rs:43), known before a transcript is touched
    const uint64_t cw = ccs.m && !(ccs.m & (ccs.m - 1)) ? zip::next_pow2(zip::isqrt(ccs.m)) * lc_spec_.repetition_factor : UINT64_MAX;
    bool batched = zip::batch_path_enabled() && B >= 2 && B <= 65535 && lc_spec_.num_proximity_testing <= 1 && cw <= 8192 &&
                   B >= min_pcs_batch(ccs.s_prime);
    for (size_t i = 1; i < B && batched; i++) batched = configs[i].limbs == configs[0].limbs;
    std::vector<zip::ZipProof> out(B);
    if (!batched) {
        for (size_t i = 0; i < B; i++) out[i] = pcs_step(zs[i].z, zs[i].len, ccs, r_y[i], *transcripts[i], configs[i]);
        return out;
    }
    // z_mle = from_evaluations_slice(s_prime, z_ccs), as pcs_step pads it
    const size_t n_mle = (size_t)1 << ccs.s_prime;
    std::vector<IntVec> padded(B);
    std::vector<zip::PcsBatchMember> members(B);
    for (size_t i = 0; i < B; i++) {
        members[i].z_evals = zs[i].z;
        if (zs[i].len != n_mle) {
            padded[i].assign(n_mle, 0);
            std::memcpy(padded[i].data(), zs[i].z, std::min(zs[i].len, n_mle) * 8);
            members[i].z_evals = padded[i].data();
        }
        members[i].r_y = r_y[i].data();
        members[i].r_y_len = r_y[i].size();
        members[i].transcript = transcripts[i];
        members[i].config = &configs[i];
    }
    return zip::commit_z_mle_and_prove_evaluation_batch(lc_spec_, ccs.m, members, device_);
}

// ---------------------------------------------------------------------------- sumcheck verifier
Limbs sumcheck::interpolate_uni_poly(const FieldConfig &config, const std::vector<Limbs> &p_i, const Limbs &x) {
    const size_t len = p_i.size();
    std::vector<Limbs> evals{x};
    Limbs prod = x, j{};
    for (size_t i = 1; i < len; i++) {  // verifier.rs:176-185: early return when x is one of the nodes
        if (x == j) return p_i[i - 1];
        config.add_assign(j, config.r);
        Limbs tmp = x;
        config.sub_assign(tmp, j);
        evals.push_back(tmp);
        config.mul_assign(prod, tmp);
    }
    if (x == j) return p_i[len - 1];
    // sum_i p_i[i] * prod / ((x - i) * prod_{k != i} (i - k)): the reference only organises the denominators
    // so that it needs fewer divisions (:217-300); the value is that of the unique interpolant either way
    Limbs res{};
    for (size_t i = 0; i < len; i++) {
        Limbs den = config.r;
        for (size_t k = 0; k < len; k++)
            if (k != i) config.mul_assign(den, map_to_field(config, (int64_t)i - (int64_t)k));
        config.mul_assign(den, evals[i]);
        Limbs term = config.inverse(den);
        config.mul_assign(term, prod);
        config.mul_assign(term, p_i[i]);
        config.add_assign(res, term);
    }
    return res;
}

sumcheck::SubClaim sumcheck::verify_as_subprotocol(KeccakTranscript &transcript, uint32_t num_vars, uint32_t degree,
                                                   const Limbs &claimed_sum, const SumcheckProof &proof,
                                                   const FieldConfig &config) {
    transcript.absorb_random_field(config, map_to_field_u128(config, num_vars, 0));  // sumcheck.rs:124-136
    transcript.absorb_random_field(config, map_to_field_u128(config, degree, 0));
    SubClaim claim;
    if (num_vars == 0) {  // :138-144
        transcript.absorb_random_field(config, claimed_sum);
        claim.expected_evaluation = claimed_sum;
        return claim;
    }
    if (proof.msgs.size() != num_vars)
        throw SpartanError(SpartanError::InvalidProofLength, "sumcheck proof has " + std::to_string(proof.msgs.size()) +
                                                                 " rounds, expected " + std::to_string(num_vars));
    for (uint32_t i = 0; i < num_vars; i++) {  // :155-160, verify_round (verifier.rs:61-90)
        for (const Limbs &e : proof.msgs[i]) transcript.absorb_random_field(config, e);
        const Limbs r = transcript.get_challenge(config);
        transcript.absorb_random_field(config, r);
        claim.point.push_back(r);
    }
    Limbs expected = claimed_sum;  // check_and_generate_subclaim (verifier.rs:97-143)
    for (uint32_t i = 0; i < num_vars; i++) {
        const std::vector<Limbs> &ev = proof.msgs[i];
        if (ev.size() != (size_t)degree + 1) throw SpartanError(SpartanError::MaxDegreeExceeded, "MaxDegreeExceeded");
        Limbs sum = ev[0];
        if (degree > 0) config.add_assign(sum, ev[1]);
        if (sum != expected) throw SpartanError(SpartanError::SumCheckFailed, "sumcheck round " + std::to_string(i) + ": p(0) + p(1) != expected");
        expected = interpolate_uni_poly(config, ev, claim.point[i]);
    }
    claim.expected_evaluation = expected;
    return claim;
}

// ---------------------------------------------------------------------------- ZincVerifier
namespace {
Limbs lin_comb_V_s(const FieldConfig &config, const Limbs &gamma, const std::vector<Limbs> &V) {  // verifier.rs:212-219
    Limbs res{};
    for (size_t i = V.size(); i-- > 0;) {
        config.mul_assign(res, gamma);
        config.add_assign(res, V[i]);
    }
    return res;
}
}  // namespace

VerificationPoints ZincVerifier::spartan_verify(const SpartanProof &proof, const ccs::CCS_Z &ccs, KeccakTranscript &transcript,
                                                const FieldConfig &config) const {
    if (proof.V_s.size() != ccs.t || ccs.S.size() != ccs.q || ccs.c.size() != ccs.q)
        throw std::logic_error("index out of bounds: V_s / ccs.S / ccs.c sizes");  // the reference indexes V_s[j]
    transcript.absorb(reinterpret_cast<const uint8_t *>("beta_s"), 6);
    std::vector<Limbs> beta_s;
    for (size_t i = 0; i < ccs.s; i++) beta_s.push_back(transcript.get_challenge(config));
    // verify_linearization_proof (:142-162): degree d + 1, claimed sum 0
    const sumcheck::SubClaim first = sumcheck::verify_as_subprotocol(transcript, (uint32_t)ccs.s, (uint32_t)ccs.d + 1, Limbs{},
                                                                    proof.linearization_sumcheck, config);
    // verify_linearization_claim (:164-187)
    Limbs e = config.r;
    for (size_t i = 0; i < ccs.s; i++) {  // eq_eval, sumcheck/utils.rs:81-95
        Limbs xy = first.point[i];
        config.mul_assign(xy, beta_s[i]);
        Limbs term = xy;
        config.add_assign(term, xy);
        config.sub_assign(term, first.point[i]);
        config.sub_assign(term, beta_s[i]);
        config.add_assign(term, config.r);
        config.mul_assign(e, term);
    }
    Limbs sum{};
    for (size_t i = 0; i < ccs.q; i++) {
        Limbs term = map_to_field(config, ccs.c[i]);
        for (size_t j : ccs.S[i]) {
            if (j >= proof.V_s.size()) throw std::logic_error("index out of bounds: ccs.S refers to a missing V_s");
            config.mul_assign(term, proof.V_s[j]);
        }
        config.add_assign(sum, term);
    }
    config.mul_assign(e, sum);
    if (e != first.expected_evaluation) throw SpartanError(SpartanError::SumCheckFailed, "linearization claim: e * sum c_i prod V_s != s");
    VerificationPoints out;
    transcript.absorb(reinterpret_cast<const uint8_t *>("gamma"), 5);
    out.gamma = transcript.get_challenge(config);
    const Limbs claimed = lin_comb_V_s(config, out.gamma, proof.V_s);
    const sumcheck::SubClaim second = sumcheck::verify_as_subprotocol(transcript, (uint32_t)ccs.s_prime, 2, claimed,
                                                                     proof.second_sumcheck, config);  // :189-210
    out.rx_ry = first.point;
    out.rx_ry.insert(out.rx_ry.end(), second.point.begin(), second.point.end());
    out.e_y = second.expected_evaluation;
    return out;
}

void ZincVerifier::verify_pcs_proof(const ccs::Statement_Z &statement, const zip::MultilinearZipCommitment &z_comm,
                                    const Limbs &v, const uint8_t *pcs_proof, size_t pcs_proof_len,
                                    const VerificationPoints &points, const ccs::CCS_Z &ccs, KeccakTranscript &transcript,
                                    const FieldConfig &config, PreparedCcs *prepared) const {
    if (points.rx_ry.size() != ccs.s + ccs.s_prime) throw std::logic_error("range end index out of range for rx_ry");
    zip::KeccakSeedSource seeds(transcript);
    const zip::RaaCode linear_code = zip::RaaCode::make(lc_spec_, ccs.m, seeds);                  // :234
    const zip::MultilinearZipParams param = zip::MultilinearZip::setup(ccs.m, linear_code, device_);  // :235
    zip::PcsTranscript pcs_transcript = zip::PcsTranscript::from_proof_view(pcs_proof, pcs_proof_len);  // :236
    const Limbs *r_y = points.rx_ry.data() + ccs.s;
    zip::MultilinearZip::verify(param, z_comm, r_y, ccs.s_prime, v, pcs_transcript, config);  // :239-246
    // V_xy (:248-261) on the device
    std::unique_ptr<PreparedCcs> own;
    if (!prepared) {
        own = std::make_unique<PreparedCcs>(statement, ccs, config, device_);
        prepared = own.get();
    }
    std::vector<uint64_t> rx((size_t)ccs.s * config.limbs), ry((size_t)ccs.s_prime * config.limbs), vxy((size_t)ccs.t * config.limbs);
    for (size_t i = 0; i < ccs.s; i++) std::copy(points.rx_ry[i].begin(), points.rx_ry[i].begin() + config.limbs, rx.begin() + i * config.limbs);
    for (size_t i = 0; i < ccs.s_prime; i++) std::copy(r_y[i].begin(), r_y[i].begin() + config.limbs, ry.begin() + i * config.limbs);
    {
        std::lock_guard<std::mutex> one(prepared->mu_);
        ccs_check(prepared->h_, zip_ccs_eval_matrices(prepared->h_, rx.data(), ry.data(), vxy.data()), "zip_ccs_eval_matrices");
    }
    std::vector<Limbs> V_xy(ccs.t);
    for (size_t k = 0; k < ccs.t; k++)
        for (uint32_t i = 0; i < config.limbs; i++) V_xy[k][i] = vxy[k * config.limbs + i];
    Limbs lhs = lin_comb_V_s(config, points.gamma, V_xy);  // :264
    config.mul_assign(lhs, v);
    if (lhs != points.e_y)
        throw SpartanError(SpartanError::PcsVerification, "linear combination of powers of gamma and V_x != e_y");
}

// ---------------------------------------------------------------------------- the random field
Limbs prime_gen::get_prime(KeccakTranscript &transcript, uint32_t limbs, int device, uint32_t *candidates_tried) {
    if (limbs < 2 || limbs > 4) throw ZipError(ZipError::InvalidPcsParam, "get_prime: FIELD_LIMBS must be 2, 3 or 4");
    zip_keccak_state k;
    transcript.export_state(&k);
    Limbs prime{};
    const int32_t rc = zip_get_prime(device, &k, limbs, prime.data(), candidates_tried);
    if (rc) throw ZipError(ZipError::Device, std::string("zip_get_prime: ") + zip_strerror(rc));
    transcript.import_state(k);
    return prime;
}

FieldConfig draw_random_field(const int64_t *public_input, size_t l, KeccakTranscript &transcript, uint32_t limbs, int device) {
    for (size_t i = 0; i < l; i++) {  // cast_slice(input.as_words()): the one word of an Int<1>, little-endian
        uint8_t b[8];
        const uint64_t w = (uint64_t)public_input[i];
        for (int j = 0; j < 8; j++) b[j] = (uint8_t)(w >> (8 * j));
        transcript.absorb(b, 8);
    }
    const Limbs prime = prime_gen::get_prime(transcript, limbs, device);
    return FieldConfig::make(prime.data(), limbs);
}

namespace {
// From how many members on get_prime_batch makes ONE zip_get_prime_batch call instead of the loop over zip_get_prime: per
// limb count the smallest measured n at which the batch beat the loop by more than the loop's own run-to-run spread
// (tools/prime_batch_times.py, profiles/prime_batch.md: n = 2, 4, 16, 64, 256).  At 2, 4 and 16 members the loop is
// faster at every limb count (a batch call costs its longest chain, 4 .. 13 ms, however few the members); 64 members win
// 1.6x / 1.7x / 2.9x at 2 / 3 / 4 limbs and 256 win 4.6x / 6.0x / 7.7x.  Counts between 16 and 64 were not measured and
// loop.  ZIP_HIP_PRIME_MIN_BATCH=n (n >= 2, read per call) puts the line at n for every limb count: how the tests reach
// the batch below the line.
size_t min_prime_batch(uint32_t limbs) {
    if (const char *e = std::getenv("ZIP_HIP_PRIME_MIN_BATCH")) {
        const long n = std::atol(e);
        if (n >= 2) return (size_t)n;
    }
    (void)limbs;  // the same line at 2, 3 and 4 limbs
    return 64;
}
void absorb_public_input(KeccakTranscript &transcript, const int64_t *public_input, size_t l) {
    for (size_t i = 0; i < l; i++) {  // cast_slice(input.as_words()): the one word of an Int<1>, little-endian
        uint8_t b[8];
        const uint64_t w = (uint64_t)public_input[i];
        for (int j = 0; j < 8; j++) b[j] = (uint8_t)(w >> (8 * j));
        transcript.absorb(b, 8);
    }
}
}  // namespace

std::vector<Limbs> prime_gen::get_prime_batch(const std::vector<KeccakTranscript *> &transcripts, uint32_t limbs, int device,
                                              uint32_t *candidates_tried) {
    if (limbs < 2 || limbs > 4) throw ZipError(ZipError::InvalidPcsParam, "get_prime: FIELD_LIMBS must be 2, 3 or 4");
    const size_t B = transcripts.size();
    for (KeccakTranscript *t : transcripts)
        if (!t) throw std::logic_error("get_prime_batch: a NULL transcript");
    std::vector<Limbs> primes(B, Limbs{});
    if (!zip::batch_path_enabled() || B < 2 || B > 65535 || B < min_prime_batch(limbs)) {
        for (size_t i = 0; i < B; i++) primes[i] = get_prime(*transcripts[i], limbs, device, candidates_tried ? candidates_tried + i : nullptr);
        return primes;
    }
    std::vector<zip_keccak_state> k(B);
    for (size_t i = 0; i < B; i++) transcripts[i]->export_state(&k[i]);
    std::vector<uint64_t> words(B * limbs);
    const int32_t rc = zip_get_prime_batch(device, k.data(), (uint32_t)B, limbs, words.data(), candidates_tried);
    if (rc) throw ZipError(ZipError::Device, std::string("zip_get_prime_batch: ") + zip_strerror(rc));
    for (size_t i = 0; i < B; i++) {
        transcripts[i]->import_state(k[i]);
        std::copy(words.begin() + i * limbs, words.begin() + (i + 1) * limbs, primes[i].begin());
    }
    return primes;
}

std::vector<FieldConfig> draw_random_field_batch(const std::vector<const int64_t *> &public_inputs, const std::vector<size_t> &lens,
                                                 const std::vector<KeccakTranscript *> &transcripts, uint32_t limbs, int device) {
    const size_t B = transcripts.size();
    if (public_inputs.size() != B || lens.size() != B)
        throw std::logic_error("draw_random_field_batch: one public input and one transcript per member");
    if (limbs < 2 || limbs > 4) throw ZipError(ZipError::InvalidPcsParam, "get_prime: FIELD_LIMBS must be 2, 3 or 4");
    for (size_t i = 0; i < B; i++)
        if (!transcripts[i] || (lens[i] && !public_inputs[i])) throw std::logic_error("draw_random_field_batch: a NULL transcript or public input");
    for (size_t i = 0; i < B; i++) absorb_public_input(*transcripts[i], public_inputs[i], lens[i]);
    const std::vector<Limbs> primes = prime_gen::get_prime_batch(transcripts, limbs, device);
    std::vector<FieldConfig> out;
    out.reserve(B);
    for (size_t i = 0; i < B; i++) out.push_back(FieldConfig::make(primes[i].data(), limbs));
    return out;
}

std::vector<bool> ZincVerifier::check_field_batch(const std::vector<const int64_t *> &public_inputs, const std::vector<size_t> &lens,
                                                  const std::vector<KeccakTranscript *> &transcripts,
                                                  const std::vector<FieldConfig> &configs) const {
    const size_t B = transcripts.size();
    if (public_inputs.size() != B || lens.size() != B || configs.size() != B)
        throw std::logic_error("check_field_batch: one public input, one transcript and one field per member");
    for (size_t i = 0; i < B; i++)  // before any transcript is touched
        if (configs[i].limbs < 2 || configs[i].limbs > 4) throw ZipError(ZipError::InvalidPcsParam, "get_prime: FIELD_LIMBS must be 2, 3 or 4");
    std::vector<bool> same(B, false);
    for (uint32_t limbs = 2; limbs <= 4; limbs++) {  // the members of one limb count are one draw
        std::vector<size_t> who;
        std::vector<const int64_t *> x;
        std::vector<size_t> l;
        std::vector<KeccakTranscript *> tr;
        for (size_t i = 0; i < B; i++)
            if (configs[i].limbs == limbs) {
                who.push_back(i);
                x.push_back(public_inputs[i]);
                l.push_back(lens[i]);
                tr.push_back(transcripts[i]);
            }
        if (who.empty()) continue;
        const std::vector<FieldConfig> drawn = draw_random_field_batch(x, l, tr, limbs, device_);  // :53-57
        for (size_t j = 0; j < who.size(); j++) same[who[j]] = drawn[j].modulus == configs[who[j]].modulus;
    }
    return same;
}

std::vector<ZincVerifier::BatchOutcome> ZincVerifier::verify_batch_checked(
    const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs, const std::vector<const int64_t *> &public_inputs,
    const std::vector<size_t> &lens, const std::vector<const ZincProof *> &proofs, const std::vector<KeccakTranscript *> &transcripts,
    const std::vector<FieldConfig> &configs) const {
    std::vector<BatchProof> views(proofs.size());
    for (size_t i = 0; i < proofs.size(); i++) {
        if (!proofs[i]) throw std::logic_error("verify_batch: a NULL proof");
        const zip::ZipProof &zp = proofs[i]->zip_proof;
        views[i] = {&proofs[i]->spartan_proof, &zp.z_comm, &zp.v, zp.pcs_proof.data(), zp.pcs_proof.size()};
    }
    return verify_batch_checked(matrices, ccs, public_inputs, lens, views, transcripts, configs);
}

std::vector<ZincVerifier::BatchOutcome> ZincVerifier::verify_batch_checked(
    const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs, const std::vector<const int64_t *> &public_inputs,
    const std::vector<size_t> &lens, const std::vector<BatchProof> &proofs, const std::vector<KeccakTranscript *> &transcripts,
    const std::vector<FieldConfig> &configs) const {
    const size_t B = proofs.size();
    if (transcripts.size() != B) throw std::logic_error("verify_batch: one transcript and one field per proof");
    const std::vector<bool> same = check_field_batch(public_inputs, lens, transcripts, configs);
    std::vector<BatchProof> p;
    std::vector<KeccakTranscript *> tr;
    std::vector<FieldConfig> f;
    std::vector<size_t> who;
    for (size_t i = 0; i < B; i++)
        if (same[i]) {
            who.push_back(i);
            p.push_back(proofs[i]);
            tr.push_back(transcripts[i]);
            f.push_back(configs[i]);
        }
    std::vector<BatchOutcome> out(B);
    for (size_t i = 0; i < B; i++)
        if (!same[i]) {
            out[i].kind = BatchOutcome::FieldConfig;
            out[i].message = "the field drawn from the public input and the transcript is not the given field configuration";
        }
    const std::vector<BatchOutcome> passed = verify_batch(matrices, ccs, p, tr, f);
    for (size_t j = 0; j < who.size(); j++) out[who[j]] = passed[j];
    return out;
}

void ZincVerifier::check_field(const int64_t *public_input, size_t l, KeccakTranscript &transcript,
                               const FieldConfig &config) const {
    const FieldConfig drawn = draw_random_field(public_input, l, transcript, config.limbs, device_);  // :53-57
    if (drawn.limbs != config.limbs || drawn.modulus != config.modulus)
        throw FieldConfigError("the field drawn from the public input and the transcript is not the given field configuration");
}

void ZincVerifier::verify_checked(const ccs::Statement_Z &statement, const ZincProof &proof, KeccakTranscript &transcript,
                                  const ccs::CCS_Z &ccs, const FieldConfig &config, PreparedCcs *prepared) const {
    check_field(statement.public_input.data(), statement.public_input.size(), transcript, config);
    verify(statement, proof, transcript, ccs, config, prepared);
}

void ZincVerifier::verify(const ccs::Statement_Z &statement, const ZincProof &proof, KeccakTranscript &transcript,
                          const ccs::CCS_Z &ccs, const FieldConfig &config, PreparedCcs *prepared) const {
    if (ccs.s == 0 || ccs.s > 28 || ccs.m != ((size_t)1 << ccs.s) || ccs.n != ccs.m || ccs.s_prime != ccs.s)
        throw std::logic_error("m == n == 2^s is required (see ZincProver)");
    const VerificationPoints points = spartan_verify(proof.spartan_proof, ccs, transcript, config);  // :62-64
    verify_pcs_proof(statement, proof.zip_proof, points, ccs, transcript, config, prepared);          // :66-73
}

// ---- B proofs of one circuit (zip_batch_verify_codes + zip_ccs_batch_eval_matrices) -------------------------------------
namespace {
// From how many proofs on verify_batch takes the batched path: per size the smallest B at which it beat the loop over
// verify by more than the loop's own spread (tools/verify_batch_times.py, profiles/verify_batch.md: 1000 openings, 4
// limbs, B = 2, 16 and, at 2^10 rows, 256).  2 proofs win at 2^10 and 2^14 rows (1.21x, 1.10x) and stay inside the loop's
// spread at 2^12 and 2^16 (1.11x, 1.06x); 16 proofs win at every size (2.4x .. 3.7x).  Counts between 2 and 16 were not
// measured and loop where 2 did not win; a size between the measured ones takes the rule of the next larger one.
// ZIP_HIP_VERIFY_MIN_BATCH=n (n >= 2, read per call) puts the line at n for every size: how the tests and
// tools/verify_batch_times.py reach the batched path below the line.
size_t min_verify_batch(size_t s_prime) {
    if (const char *e = std::getenv("ZIP_HIP_VERIFY_MIN_BATCH")) {
        const long n = std::atol(e);
        if (n >= 2) return (size_t)n;
    }
    return s_prime <= 10 ? 2 : s_prime <= 12 ? 16 : s_prime <= 14 ? 2 : 16;
}

// f(): true when it returned; false with the outcome `verify` would have ended in when it threw one of the verifier's own
// errors.  Device failures and panics pass through: they are no verdict on a proof.
template <class F>
bool attempt(ZincVerifier::BatchOutcome &o, F &&f) {
    try {
        f();
        return true;
    } catch (const SpartanError &e) {
        o.kind = ZincVerifier::BatchOutcome::Spartan;
        o.message = e.what();
    } catch (const ZipError &e) {
        if (e.kind == ZipError::Device) throw;
        o.kind = ZincVerifier::BatchOutcome::Zip;
        o.zip_kind = e.kind;
        o.message = e.what();
    }
    return false;
}
}  // namespace

std::vector<ZincVerifier::BatchOutcome> ZincVerifier::verify_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs,
                                                                   const std::vector<const ZincProof *> &proofs,
                                                                   const std::vector<KeccakTranscript *> &transcripts,
                                                                   const std::vector<FieldConfig> &configs) const {
    std::vector<BatchProof> views(proofs.size());
    for (size_t i = 0; i < proofs.size(); i++) {
        if (!proofs[i]) throw std::logic_error("verify_batch: a NULL proof");
        const zip::ZipProof &zp = proofs[i]->zip_proof;
        views[i] = {&proofs[i]->spartan_proof, &zp.z_comm, &zp.v, zp.pcs_proof.data(), zp.pcs_proof.size()};
    }
    return verify_batch(matrices, ccs, views, transcripts, configs);
}

std::vector<ZincVerifier::BatchOutcome> ZincVerifier::verify_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs,
                                                                   const std::vector<BatchProof> &proofs,
                                                                   const std::vector<KeccakTranscript *> &transcripts,
                                                                   const std::vector<FieldConfig> &configs) const {
    const size_t B = proofs.size();
    if (transcripts.size() != B || configs.size() != B) throw std::logic_error("verify_batch: one transcript and one field per proof");
    if (!matrices && B) throw std::logic_error("verify_batch: no matrices");
    // the shapes verify and spartan_verify panic on, on every member, before any transcript is touched
    if (ccs.s == 0 || ccs.s > 28 || ccs.m != ((size_t)1 << ccs.s) || ccs.n != ccs.m || ccs.s_prime != ccs.s)
        throw std::logic_error("m == n == 2^s is required (see ZincProver)");
    for (size_t i = 0; i < B; i++) {
        const BatchProof &p = proofs[i];
        if (!transcripts[i] || !p.spartan_proof || !p.z_comm || !p.v || (!p.pcs_proof && p.pcs_proof_len))
            throw std::logic_error("verify_batch: a NULL transcript or proof part");
        if (p.spartan_proof->V_s.size() != ccs.t || ccs.S.size() != ccs.q || ccs.c.size() != ccs.q)
            throw std::logic_error("index out of bounds: V_s / ccs.S / ccs.c sizes");
        for (const auto &Si : ccs.S)
            for (size_t j : Si)
                if (j >= ccs.t) throw std::logic_error("index out of bounds: ccs.S refers to a missing V_s");
    }
    std::vector<BatchOutcome> out(B);
    const uint32_t s = (uint32_t)ccs.s, t = (uint32_t)ccs.t;
    // the geometry RaaCode::make will give every member (code_raa.rs:43), known before a transcript is touched
    const uint64_t cw_all = zip::next_pow2(zip::isqrt(ccs.m)) * lc_spec_.repetition_factor;
    bool batched = zip::batch_path_enabled() && B >= 2 && B <= 65535 && lc_spec_.num_proximity_testing <= 1 && cw_all <= 16384 &&
                   s <= 16 && B >= min_verify_batch(ccs.s_prime);
    for (size_t i = 1; i < B && batched; i++) batched = configs[i].limbs == configs[0].limbs;
    if (!batched) {
        ccs::Statement_Z st;
        st.constraints.resize(t);  // the matrices go to the device straight from the caller's arrays
        for (size_t i = 0; i < B; i++)
            attempt(out[i], [&] {
                const VerificationPoints points = spartan_verify(*proofs[i].spartan_proof, ccs, *transcripts[i], configs[i]);
                PreparedCcs prep(matrices, t, s, configs[i], device_);  // per proof: every proof has its own field
                verify_pcs_proof(st, *proofs[i].z_comm, *proofs[i].v, proofs[i].pcs_proof, proofs[i].pcs_proof_len, points, ccs,
                                 *transcripts[i], configs[i], &prep);
            });
        return out;
    }
    const uint32_t fl = configs[0].limbs;
    // 1. SpartanVerifier::verify per member: host work
    std::vector<VerificationPoints> points(B);
    std::vector<size_t> live;
    for (size_t i = 0; i < B; i++)
        if (attempt(out[i], [&] { points[i] = spartan_verify(*proofs[i].spartan_proof, ccs, *transcripts[i], configs[i]); })) live.push_back(i);
    if (live.empty()) return out;
    // 2. per survivor, in verify_pcs_proof's order: the code from its transcript (:234), then what MultilinearZip::verify
    // does in front of the device call on a FRESH PcsTranscript over the proof bytes (:236)
    zip::MultilinearZipParams param;
    bool have_param = false;
    uint32_t cw = 0, num_rows = 0, n_cols = 0;
    std::vector<size_t> pcs;  // the members that reach zip_batch_verify_codes
    std::vector<uint32_t> perms1, perms2, cols;
    std::vector<int64_t> coeffs;
    std::vector<uint64_t> q0, q1, evals;
    std::vector<uint8_t> roots;
    std::vector<const uint8_t *> streams;
    std::vector<size_t> stream_lens;
    for (size_t i : live) {
        const BatchProof &p = proofs[i];
        const FieldConfig &f = configs[i];
        zip::KeccakSeedSource seeds(*transcripts[i]);
        const zip::RaaCode code = zip::RaaCode::make(lc_spec_, ccs.m, seeds);
        if (!have_param) {
            param = zip::MultilinearZip::setup(ccs.m, code, device_);  // the ctx of the geometry, cached like any other
            have_param = true;
            cw = code.codeword_len();
            num_rows = param.num_rows;
            n_cols = param.linear_code.num_column_opening;
        }
        std::pair<std::vector<int64_t>, std::vector<uint32_t>> ch;
        std::vector<uint64_t> q0_i, q1_i;
        const bool reaches = attempt(out[i], [&] {
            size_t point_len = ccs.s_prime;
            zip::validate_input("verify", param.num_vars, param.num_vars, &point_len);
            if (p.z_comm->roots.size() != num_rows) throw ZipError(ZipError::InvalidPcsOpen, "commitment has the wrong number of roots");
            zip::PcsTranscript walk = zip::PcsTranscript::from_proof_view(p.pcs_proof, p.pcs_proof_len);
            ch = zip::MultilinearZip::open_challenges(num_rows, cw, n_cols, param.linear_code.num_proximity_testing, f, walk);
            zip::point_to_tensor(f, num_rows, points[i].rx_ry.data() + ccs.s, ccs.s_prime, q0_i, q1_i);
        });
        if (!reaches) continue;
        pcs.push_back(i);
        const auto p1 = zip::shuffle_seeded_perm(code.perm_1_seed, cw), p2 = zip::shuffle_seeded_perm(code.perm_2_seed, cw);
        perms1.insert(perms1.end(), p1.begin(), p1.end());
        perms2.insert(perms2.end(), p2.begin(), p2.end());
        coeffs.insert(coeffs.end(), ch.first.begin(), ch.first.end());
        cols.insert(cols.end(), ch.second.begin(), ch.second.end());
        q0.insert(q0.end(), q0_i.begin(), q0_i.end());
        q1.insert(q1.end(), q1_i.begin(), q1_i.end());
        evals.insert(evals.end(), p.v->begin(), p.v->begin() + fl);
        for (const auto &r : p.z_comm->roots) roots.insert(roots.end(), r.begin(), r.end());
        streams.push_back(p.pcs_proof);
        stream_lens.push_back(p.pcs_proof_len);
    }
    // 3. every proof stream in one call, read where it lies
    std::vector<zip_verify_report> reports(pcs.size());
    std::vector<zip_field> zf(pcs.size());
    std::vector<const zip_field *> zfp(pcs.size());
    for (size_t j = 0; j < pcs.size(); j++) {
        zf[j] = configs[pcs[j]].to_abi();
        zfp[j] = &zf[j];
    }
    if (!pcs.empty()) {
        zip_ctx *ctx = param.ctx.get();
        zip::check(ctx,
                   zip_batch_verify_codes(ctx, (uint32_t)pcs.size(), perms1.data(), perms2.data(), roots.data(), streams.data(),
                                          stream_lens.data(), ZIP_MEM_HOST, coeffs.empty() ? nullptr : coeffs.data(), cols.data(), n_cols,
                                          q0.empty() ? nullptr : q0.data(), q1.empty() ? nullptr : q1.data(), evals.data(), zfp.data(),
                                          reports.data()),
                   "zip_batch_verify_codes");
    }
    // 4. V_xy (:248-261) of the same members over the circuit as integers
    std::vector<uint64_t> vxy(pcs.size() * (size_t)t * fl);
    if (!pcs.empty()) {
        std::vector<uint64_t> rx(pcs.size() * (size_t)s * fl), ry(pcs.size() * (size_t)s * fl);
        for (size_t j = 0; j < pcs.size(); j++)
            for (size_t k = 0; k < s; k++) {
                const std::vector<Limbs> &pt = points[pcs[j]].rx_ry;
                std::copy(pt[k].begin(), pt[k].begin() + fl, rx.begin() + (j * s + k) * fl);
                std::copy(pt[s + k].begin(), pt[s + k].begin() + fl, ry.begin() + (j * s + k) * fl);
            }
        CcsBatchHandle dev;
        ccs_batch_check(nullptr, zip_ccs_batch_create(device_, matrices, t, s, fl, (uint32_t)pcs.size(), &dev.h), "zip_ccs_batch_create");
        ccs_batch_check(dev.h, zip_ccs_batch_eval_matrices(dev.h, zfp.data(), (uint32_t)pcs.size(), rx.data(), ry.data(), vxy.data()),
                        "zip_ccs_batch_eval_matrices");
    }
    // 5. per member, in the loop's order: the PCS verdict, then the last check (:264-271)
    for (size_t j = 0; j < pcs.size(); j++) {
        const size_t i = pcs[j];
        const FieldConfig &f = configs[i];
        attempt(out[i], [&] {
            zip::throw_unless_accepted(reports[j].verdict);
            std::vector<Limbs> V_xy(t);
            for (size_t k = 0; k < t; k++)
                for (uint32_t l = 0; l < fl; l++) V_xy[k][l] = vxy[(j * t + k) * fl + l];
            Limbs lhs = lin_comb_V_s(f, points[i].gamma, V_xy);
            f.mul_assign(lhs, *proofs[i].v);
            if (lhs != points[i].e_y)
                throw SpartanError(SpartanError::PcsVerification, "linear combination of powers of gamma and V_x != e_y");
        });
    }
    return out;
}

}  // namespace zinc
