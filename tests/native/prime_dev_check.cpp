// Host build of zinc_amd/csrc/prime_dev.cuh for tests/test_prime_dev_host.py and tools/prime_times.py: the lane
// function of prime_test_base2_kernel, the candidate chain of zip_get_prime and the knob parser, compiled with g++.
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
void store(const TrSponge &sp, uint64_t *st, uint8_t *buf, uint32_t *buflen) {
    std::memcpy(st, sp.st, sizeof sp.st);
    std::memcpy(buf, sp.blk, kKeccakRate);
    *buflen = sp.buflen;
}

template <int FL>
void test_fl(const uint64_t *cands, uint32_t n, uint8_t *out) {
    for (uint32_t i = 0; i < n; i++) {
        uint64_t c[FL];
        for (int k = 0; k < FL; k++) c[k] = cands[(size_t)i * FL + k];
        out[i] = prime_test_base2<FL>(c) ? 1 : 0;
    }
}
template <int FL>
void chain_fl(TrSponge &sp, uint32_t count, uint64_t *cands, uint64_t *st_out, uint8_t *buf_out, uint32_t *buflen_out) {
    for (uint32_t i = 0; i < count; i++) {
        uint64_t c[FL];
        prime_next_candidate<FL>(sp, c);
        for (int k = 0; k < FL; k++) cands[(size_t)i * FL + k] = c[k];
        store(sp, st_out + (size_t)i * 25, buf_out + (size_t)i * kKeccakRate, buflen_out + i);
    }
}
// the reference's loop, one candidate after the other on this thread
template <int FL>
uint32_t get_prime_fl(TrSponge &sp, uint64_t *prime_out, uint32_t max_tries) {
    for (uint32_t tried = 1; tried <= max_tries; tried++) {
        uint64_t c[FL];
        prime_next_candidate<FL>(sp, c);
        if (prime_test_base2<FL>(c)) {
            for (int k = 0; k < FL; k++) prime_out[k] = c[k];
            return tried;
        }
    }
    return 0;
}
}  // namespace

extern "C" {

int pd_test_base2(uint32_t fl, const uint64_t *cands, uint32_t n, uint8_t *out) {
    switch (fl) {
        case 2: test_fl<2>(cands, n, out); return 0;
        case 3: test_fl<3>(cands, n, out); return 0;
        case 4: test_fl<4>(cands, n, out); return 0;
    }
    return -1;
}

// the first `count` candidates of the chain from the sponge (st, buf, buflen) and the sponge after each of them
int pd_chain(uint32_t fl, const uint64_t *st, const uint8_t *buf, uint32_t buflen, uint32_t count, uint64_t *cands,
             uint64_t *st_out, uint8_t *buf_out, uint32_t *buflen_out) {
    TrSponge sp;
    load(sp, st, buf, buflen);
    switch (fl) {
        case 2: chain_fl<2>(sp, count, cands, st_out, buf_out, buflen_out); return 0;
        case 3: chain_fl<3>(sp, count, cands, st_out, buf_out, buflen_out); return 0;
        case 4: chain_fl<4>(sp, count, cands, st_out, buf_out, buflen_out); return 0;
    }
    return -1;
}

// get_prime sequentially on one core; the sponge in place.  Returns the candidates tried, 0 if max_tries ran out.
uint32_t pd_get_prime(uint32_t fl, uint64_t *st, uint8_t *buf, uint32_t *buflen, uint64_t *prime_out, uint32_t max_tries) {
    TrSponge sp;
    load(sp, st, buf, *buflen);
    uint32_t tried = 0;
    switch (fl) {
        case 2: tried = get_prime_fl<2>(sp, prime_out, max_tries); break;
        case 3: tried = get_prime_fl<3>(sp, prime_out, max_tries); break;
        case 4: tried = get_prime_fl<4>(sp, prime_out, max_tries); break;
    }
    store(sp, st, buf, buflen);
    return tried;
}

uint32_t pd_batch_knob(const char *text, uint32_t def, uint32_t max) { return prime_batch_knob(text, def, max); }

}  // extern "C"
