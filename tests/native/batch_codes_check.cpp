// Stand-alone: every entry point of the batch family with a code and a field per member (include/zip_hip.h), called as a
// C caller on a machine that may have no device.  A zip_ctx cannot exist without one, so what can be asked here is what
// each call answers before it looks at a handle: ZIP_ERR_NULL, first, whatever else is wrong with the arguments, with
// every output left as documented, and the counters standing still.  (The errors behind a live handle, and their order,
// are in tests/test_gpu_batch_codes.py.)  Built by tests/test_pcs_step_batch_host.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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
    uint64_t c0 = 1, m0 = 2, f0 = 3;
    zip_batch_codes_counts(&c0, &m0, &f0);
    zip_batch_codes_counts(nullptr, nullptr, nullptr);  // any pointer may be NULL
    uint64_t only = 77;
    zip_batch_codes_counts(nullptr, &only, nullptr);
    EXPECT(only == m0);

    const uint32_t cw = 8, n_polys = 2;
    std::vector<int64_t> evals(n_polys * 4, 5);
    std::vector<uint32_t> p1(n_polys * cw), p2(n_polys * cw);
    for (uint32_t i = 0; i < n_polys * cw; i++) p1[i] = p2[i] = i % cw;
    uint8_t roots[64];
    zip_batch *out = reinterpret_cast<zip_batch *>(0x1);

    // zip_batch_commit_codes: no ctx -- before n_polys (0), the shape (n_evals) and the permutations are looked at
    EXPECT(zip_batch_commit_codes(nullptr, evals.data(), evals.size(), n_polys, ZIP_MEM_HOST, p1.data(), p2.data(), roots, &out) == ZIP_ERR_NULL);
    EXPECT(zip_batch_commit_codes(nullptr, evals.data(), 3, 0, ZIP_MEM_HOST, p1.data(), p2.data(), roots, &out) == ZIP_ERR_NULL);
    p1[3] = p1[4];  // not a permutation: still NULL first
    EXPECT(zip_batch_commit_codes(nullptr, evals.data(), evals.size(), n_polys, ZIP_MEM_HOST, p1.data(), p2.data(), roots, &out) == ZIP_ERR_NULL);
    EXPECT(zip_batch_commit_codes(nullptr, nullptr, 0, 70000, ZIP_MEM_HOST, nullptr, nullptr, nullptr, nullptr) == ZIP_ERR_NULL);
    EXPECT(out == reinterpret_cast<zip_batch *>(0x1));  // without a ctx nothing is written

    // the two opens: no batch
    zip_field f{};
    f.limbs = 4;
    f.modulus[0] = 4;  // even: still NULL first
    const zip_field *fields[2] = {&f, nullptr};
    std::vector<uint64_t> q0(2 * 4 * 4, 1), rows(2 * 4 * 4, 9);
    std::vector<int64_t> coeffs(8, 1);
    uint32_t cols[4] = {0, 1, 2, 99};
    std::vector<uint8_t> proofs(256, 0xAB);
    EXPECT(zip_batch_open_eval_fields(nullptr, q0.data(), fields, rows.data(), ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_eval_fields(nullptr, nullptr, nullptr, nullptr, ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_fields(nullptr, coeffs.data(), cols, 2, q0.data(), fields, proofs.data(), ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_fields(nullptr, nullptr, nullptr, 2, nullptr, nullptr, nullptr, ZIP_MEM_DEVICE) == ZIP_ERR_NULL);
    for (uint64_t v : rows) EXPECT(v == 9);
    for (uint8_t v : proofs) EXPECT(v == 0xAB);
    // the calls a batch of either commit entry point shares
    EXPECT(zip_batch_size(nullptr) == 0);
    zip_batch_free(nullptr);
    zip_commitment *member = nullptr;
    EXPECT(zip_batch_member(nullptr, 0, &member) == ZIP_ERR_NULL);

    uint64_t c1, m1, f1;
    zip_batch_codes_counts(&c1, &m1, &f1);
    EXPECT(c1 == c0 && m1 == m0 && f1 == f0);
    if (failures) return 1;
    std::puts("batch_codes_check ok");
    return 0;
}
