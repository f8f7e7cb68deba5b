// Host build of the word-wise chain step of zinc_amd/csrc/prime_dev.cuh (prime_next_candidate_words: what every lane of
// prime_chain_batch_kernel runs) for tests/test_prime_chain_host.py: run beside the byte-addressed prime_next_candidate,
// candidate by candidate.  With PRIME_CHAIN_CHECK_MAIN it is a program of its own: every starting buflen 0 .. 135, 300
// consecutive candidates, 2 / 3 / 4 limbs, on sponges it makes up -- what the sanitizer build runs.
#include <cstdio>
#include <cstring>

#include "prime_dev.cuh"

using namespace zipk;

namespace {
void load(TrSponge &sp, const uint64_t *st, const uint8_t *buf, uint32_t buflen) {
    std::memcpy(sp.st, st, sizeof sp.st);
    uint8_t pending[kKeccakRate] = {0};
    std::memcpy(pending, buf, buflen);
    std::memcpy(sp.blk, pending, kKeccakRate);  // little-endian host
    sp.buflen = buflen;
}
bool same(const TrSponge &a, const TrSponge &b) {
    return !std::memcmp(a.st, b.st, sizeof a.st) && !std::memcmp(a.blk, b.blk, sizeof a.blk) && a.buflen == b.buflen;
}

// `count` candidates by both steps from the same sponge; the word-wise step's candidates and sponges go out.
// Returns the number of candidates at which the two differ in the candidate or in the sponge afterwards.
template <int FL>
uint32_t chain_fl(const TrSponge &start, uint32_t count, uint64_t *cands, uint64_t *st_out, uint8_t *buf_out, uint32_t *buflen_out) {
    TrSponge words = start, bytes = start;
    uint32_t differ = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t cw[FL], cb[FL];
        prime_next_candidate_words<FL>(words, cw);
        prime_next_candidate<FL>(bytes, cb);
        if (std::memcmp(cw, cb, sizeof cw) || !same(words, bytes)) differ++;
        if (cands) std::memcpy(cands + (size_t)i * FL, cw, sizeof cw);
        if (st_out) std::memcpy(st_out + (size_t)i * 25, words.st, sizeof words.st);
        if (buf_out) std::memcpy(buf_out + (size_t)i * kKeccakRate, words.blk, kKeccakRate);
        if (buflen_out) buflen_out[i] = words.buflen;
    }
    return differ;
}
uint32_t chain(uint32_t fl, const TrSponge &sp, uint32_t count, uint64_t *cands, uint64_t *st_out, uint8_t *buf_out,
               uint32_t *buflen_out) {
    switch (fl) {
        case 2: return chain_fl<2>(sp, count, cands, st_out, buf_out, buflen_out);
        case 3: return chain_fl<3>(sp, count, cands, st_out, buf_out, buflen_out);
        case 4: return chain_fl<4>(sp, count, cands, st_out, buf_out, buflen_out);
    }
    return ~0u;
}
}  // namespace

extern "C" {

// the first `count` candidates of the word-wise chain from the sponge (st, buf, buflen) and the sponge after each;
// returns how many of them differ from prime_next_candidate's (~0 for a limb count outside 2 .. 4)
uint32_t pc_chain_words(uint32_t fl, const uint64_t *st, const uint8_t *buf, uint32_t buflen, uint32_t count, uint64_t *cands,
                        uint64_t *st_out, uint8_t *buf_out, uint32_t *buflen_out) {
    TrSponge sp;
    load(sp, st, buf, buflen);
    return chain(fl, sp, count, cands, st_out, buf_out, buflen_out);
}

}  // extern "C"

#ifdef PRIME_CHAIN_CHECK_MAIN
int main() {
    uint64_t x = 0x9E3779B97F4A7C15ULL;
    auto next = [&x] {  // splitmix64
        uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    uint64_t differ = 0, steps = 0;
    for (uint32_t fl = 2; fl <= 4; fl++)
        for (uint32_t buflen = 0; buflen < kKeccakRate; buflen++) {
            uint64_t st[25];
            uint8_t buf[kKeccakRate];
            for (uint64_t &w : st) w = next();
            for (uint8_t &b : buf) b = (uint8_t)next();  // bytes at and beyond buflen are ignored on input
            TrSponge sp;
            load(sp, st, buf, buflen);
            differ += chain(fl, sp, 300, nullptr, nullptr, nullptr, nullptr);
            steps += 300;
        }
    std::printf("prime_chain_check: %llu steps, %llu differ\n", (unsigned long long)steps, (unsigned long long)differ);
    return differ ? 1 : 0;
}
#endif
