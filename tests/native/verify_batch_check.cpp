// Stand-alone: the entry points of the batched Zinc verifier (zip_batch_verify_codes, zip_batch_verify_codes_counts,
// zip_ccs_batch_eval_matrices in include/zip_hip.h; zinc_verifier_verify_batch in include/zinc_zip_host.h), called as a C
// caller on a machine that may have no device.  A zip_ctx and a zip_ccs_batch cannot exist without one, so what can be
// asked of the first two here is what each answers before it looks at a handle: ZIP_ERR_NULL, first, whatever else is
// wrong with the arguments, with every output left alone and the counters standing still.  The facade is asked what it
// decides on the host: its own NULL checks, the shape the reference panics on, and two proofs whose first sumcheck
// message is wrong -- both rejected by the Spartan part, on the loop and on the batched path, before any device work.
// (The errors behind a live handle, and their order, are in tests/test_gpu_batch_verify_codes.py and
// tests/test_gpu_ccs_batch_eval.py.)  Built by tests/test_verify_batch_host.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zinc_zip_host.h"
#include "zip_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

int main() {
    EXPECT(zip_abi_version() == 3);
    uint64_t calls0 = 1, members0 = 2;
    zip_batch_verify_codes_counts(&calls0, &members0);
    zip_batch_verify_codes_counts(nullptr, nullptr);  // either pointer may be NULL
    uint64_t only = 77;
    zip_batch_verify_codes_counts(nullptr, &only);
    EXPECT(only == members0);

    // ---- zip_batch_verify_codes: no ctx -- before n_polys, the fields, the streams and the permutations are looked at
    const uint32_t cw = 8, n_polys = 2, n_cols = 3;
    std::vector<uint32_t> p1(n_polys * cw), p2(n_polys * cw);
    for (uint32_t i = 0; i < n_polys * cw; i++) p1[i] = p2[i] = i % cw;
    std::vector<uint8_t> roots(n_polys * 4 * 32, 1), stream(512, 0xAB);
    const uint8_t *proofs[2] = {stream.data(), stream.data() + 1};  // (the second would be misaligned as a device stream)
    const size_t lens[2] = {stream.size(), 0};
    std::vector<int64_t> coeffs(n_polys * 4, 1);
    uint32_t cols[n_polys * n_cols] = {0, 1, 2, 3, 4, 99};
    std::vector<uint64_t> q(n_polys * 4 * 4, 1), ev(n_polys * 4, 1);
    zip_field f{};
    f.limbs = 4;
    f.modulus[0] = 4;  // even: still NULL first
    const zip_field *fields[2] = {&f, nullptr};
    zip_verify_report reps[2];
    std::memset(reps, 0x5A, sizeof reps);
    EXPECT(zip_batch_verify_codes(nullptr, n_polys, p1.data(), p2.data(), roots.data(), proofs, lens, ZIP_MEM_HOST, coeffs.data(), cols,
                                  n_cols, q.data(), q.data(), ev.data(), fields, reps) == ZIP_ERR_NULL);
    EXPECT(zip_batch_verify_codes(nullptr, 0, p1.data(), p2.data(), roots.data(), proofs, lens, ZIP_MEM_DEVICE, coeffs.data(), cols, n_cols,
                                  q.data(), q.data(), ev.data(), fields, reps) == ZIP_ERR_NULL);
    p1[3] = p1[4];  // not a permutation: still NULL first
    EXPECT(zip_batch_verify_codes(nullptr, 70000, p1.data(), p2.data(), roots.data(), proofs, lens, ZIP_MEM_HOST, coeffs.data(), cols, n_cols,
                                  q.data(), q.data(), ev.data(), fields, reps) == ZIP_ERR_NULL);
    EXPECT(zip_batch_verify_codes(nullptr, n_polys, nullptr, nullptr, nullptr, nullptr, nullptr, ZIP_MEM_HOST, nullptr, nullptr, 0, nullptr,
                                  nullptr, nullptr, nullptr, nullptr) == ZIP_ERR_NULL);
    for (size_t i = 0; i < sizeof reps; i++) EXPECT(reinterpret_cast<const uint8_t *>(reps)[i] == 0x5A);  // nothing is written

    // ---- zip_ccs_batch_eval_matrices: no handle
    std::vector<uint64_t> r(n_polys * 3 * 4, 1), vxy(n_polys * 3 * 4, 9);
    EXPECT(zip_ccs_batch_eval_matrices(nullptr, fields, n_polys, r.data(), r.data(), vxy.data()) == ZIP_ERR_NULL);
    EXPECT(zip_ccs_batch_eval_matrices(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == ZIP_ERR_NULL);
    for (uint64_t v : vxy) EXPECT(v == 9);
    uint64_t launches0 = 0, instances0 = 0, launches1 = 1, instances1 = 1;
    zip_ccs_batch_counts(&launches0, &instances0);

    // ---- zinc_verifier_verify_batch: the 3-matrix boolean circuit at s = 2 (A = B = C = I, S = [[0, 1], [2]], c = [1, -1])
    const uint32_t t = 3, s = 2, d = 2, nq = 2, B = 2, fl = 2;
    const uint32_t row_ptr[5] = {0, 1, 2, 3, 4}, col_idx[4] = {0, 1, 2, 3};
    const int64_t ones[4] = {1, 1, 1, 1};
    zip_sparse_matrix mats[3];
    for (auto &m : mats) m = {4, 4, row_ptr, col_idx, ones};
    const uint32_t masks[2] = {3, 4};
    const int64_t c[2] = {1, -1};
    zinc_transcript *tr[2] = {zinc_transcript_new(), zinc_transcript_new()};
    const uint64_t moduli[8] = {0x7fffffffffffffffull, 0x7fffffffffffffffull, 0, 0,   // 2^127 - 1
                                0xffffffffffffff61ull, 0xffffffffffffffffull, 0, 0};  // 2^128 - 159
    const uint32_t limbs[2] = {fl, fl};
    std::vector<uint64_t> msgs1(B * s * (d + 2) * fl, 0), msgs2(B * s * 3 * fl, 0), v_s(B * t * fl, 0), v(B * fl, 0);
    for (uint32_t i = 0; i < B; i++) msgs1[i * s * (d + 2) * fl] = 1;  // round 0: p(0) + p(1) = 1, the claimed sum is 0
    std::vector<uint8_t> comm(2 * 32, 7), pcs(64, 3);
    const uint8_t *root_ptrs[2] = {comm.data(), comm.data()};
    const size_t n_roots[2] = {2, 2};
    const uint8_t *pcs_ptrs[2] = {pcs.data(), pcs.data()};
    const size_t pcs_lens[2] = {pcs.size(), pcs.size()};
    int32_t results[2] = {99, 99};
    const size_t cap = 64;
    std::vector<char> messages(B * cap, 'x');
    auto call = [&](const zip_sparse_matrix *m, uint32_t s_, zinc_transcript *const *trs, int32_t *res) {
        return zinc_verifier_verify_batch(nullptr, m, t, s_, d, nq, masks, c, B, trs, moduli, limbs, 0, msgs1.data(), msgs2.data(),
                                          v_s.data(), root_ptrs, n_roots, v.data(), pcs_ptrs, pcs_lens, res, messages.data(), cap);
    };
    EXPECT(call(nullptr, s, tr, results) == ZINC_ERR_NULL);
    EXPECT(call(mats, s, tr, nullptr) == ZINC_ERR_NULL);
    zinc_transcript *hole[2] = {tr[0], nullptr};
    EXPECT(call(mats, s, hole, results) == ZINC_ERR_NULL);
    EXPECT(results[0] == 99 && results[1] == 99 && messages[0] == 'x');
    const uint64_t before0 = zinc_transcript_get_u64(tr[0]);  // (moves the transcript: both legs below start from the same place)
    (void)before0;
    EXPECT(call(mats, 0, tr, results) == ZINC_ERR_PANIC);  // m == n == 2^s with s >= 1: found before any transcript is touched
    EXPECT(results[0] == 99 && results[1] == 99);
    for (int leg = 0; leg < 2; leg++) {  // the loop, then the batched path: the Spartan part rejects both on the host
        setenv("ZIP_HIP_BATCH", leg ? "1" : "0", 1);
        setenv("ZIP_HIP_VERIFY_MIN_BATCH", "2", 1);
        results[0] = results[1] = 99;
        EXPECT(call(mats, s, tr, results) == ZINC_OK);
        EXPECT(results[0] == ZINC_ERR_SPARTAN && results[1] == ZINC_ERR_SPARTAN);
        for (uint32_t i = 0; i < B; i++) {
            const char *msg = messages.data() + i * cap;
            EXPECT(std::memchr(msg, 0, cap) != nullptr && msg[0] != 0);
        }
    }
    unsetenv("ZIP_HIP_VERIFY_MIN_BATCH");
    unsetenv("ZIP_HIP_BATCH");
    zinc_transcript_free(tr[0]);
    zinc_transcript_free(tr[1]);

    uint64_t calls1, members1;
    zip_batch_verify_codes_counts(&calls1, &members1);
    zip_ccs_batch_counts(&launches1, &instances1);
    EXPECT(calls1 == calls0 && members1 == members0 && launches1 == launches0 && instances1 == instances0);
    if (failures) return 1;
    std::puts("verify_batch_check ok");
    return 0;
}
