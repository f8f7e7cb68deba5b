// Host build of zinc_amd/csrc/keccak_dev.cuh for tests/test_keccak_dev_host.py: the transcript code the sumcheck tail
// kernel and the library's host thread share, driven from Python against the oracle's KeccakTranscript.
#include <cstring>

#include "keccak_dev.cuh"

using namespace zipk;

template <int FL>
static void rounds(const uint64_t *modulus, const uint64_t *r2, uint64_t inv, TrSponge &sp, const uint64_t *msgs, uint32_t ne,
                   uint32_t n_rounds, uint64_t *r_out) {
    const TrField<FL> tf = tr_make_field<FL>(modulus, r2, inv);
    for (uint32_t i = 0; i < n_rounds; i++) {
        uint64_t r[FL];
        tr_sponge_round<FL>(sp, tf, msgs + (size_t)i * ne * FL, ne, r);
        std::memcpy(r_out + (size_t)i * FL, r, sizeof r);
    }
}

extern "C" {
// n_rounds times: absorb ne field elements, get_challenge, absorb the challenge.  st / buf / buflen: zip_keccak_state.
int kd_rounds(uint32_t fl, const uint64_t *modulus, const uint64_t *r2, uint64_t inv, uint64_t *st, uint8_t *buf, uint32_t *buflen,
              const uint64_t *msgs, uint32_t ne, uint32_t n_rounds, uint64_t *r_out) {
    TrSponge sp;
    std::memcpy(sp.st, st, sizeof sp.st);
    uint8_t b[kKeccakRate] = {0};
    std::memcpy(b, buf, *buflen);
    std::memcpy(sp.blk, b, kKeccakRate);
    sp.buflen = *buflen;
    switch (fl) {
        case 2: rounds<2>(modulus, r2, inv, sp, msgs, ne, n_rounds, r_out); break;
        case 3: rounds<3>(modulus, r2, inv, sp, msgs, ne, n_rounds, r_out); break;
        case 4: rounds<4>(modulus, r2, inv, sp, msgs, ne, n_rounds, r_out); break;
        default: return -1;
    }
    std::memcpy(st, sp.st, sizeof sp.st);
    std::memcpy(buf, sp.blk, kKeccakRate);
    *buflen = sp.buflen;
    return 0;
}
// map_to_field of a u128 (the nvars / degree absorbed in front of a sumcheck)
int kd_map_u128(uint32_t fl, const uint64_t *modulus, const uint64_t *r2, uint64_t inv, uint64_t lo, uint64_t hi, uint64_t *out) {
    if (fl == 2) { uint64_t o[2]; tr_map_u128<2>(tr_make_field<2>(modulus, r2, inv), lo, hi, o); std::memcpy(out, o, sizeof o); }
    else if (fl == 3) { uint64_t o[3]; tr_map_u128<3>(tr_make_field<3>(modulus, r2, inv), lo, hi, o); std::memcpy(out, o, sizeof o); }
    else if (fl == 4) { uint64_t o[4]; tr_map_u128<4>(tr_make_field<4>(modulus, r2, inv), lo, hi, o); std::memcpy(out, o, sizeof o); }
    else return -1;
    return 0;
}
}
