// Stand-alone: what the two-limb entry points (include/zip_hip.h, "Two-limb witnesses") answer a C caller before a device
// is looked for.  A zip_ctx cannot exist without a GPU, so this covers zip_ctx_create's admission of the limb triples, the
// refusals that need no ctx (row shards, zip_mctx_create, codewords above 65536), the parameter and NULL errors of a
// two-limb geometry, and ZIP_ERR_NULL from every call that would refuse a live two-limb ctx.  (The refusals behind a live
// ctx are in tests/test_gpu_two_limb_refusals.py.)  The program never makes a ctx: where a device is visible the one call
// that would is left out.  Built by tests/test_two_limb_host.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
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
    // num_vars 8: 16 x 16, codeword 32
    std::vector<uint32_t> p1(32), p2(32);
    std::iota(p1.begin(), p1.end(), 0u);
    for (uint32_t i = 0; i < 32; i++) p2[i] = 31 - i;
    zip_params p{};
    p.num_vars = 8;
    p.row_len = 16;
    p.num_rows = 16;
    p.codeword_len = 32;
    p.rep = 2;
    p.n_limbs = 2;
    p.k_limbs = 8;
    p.m_limbs = 16;
    p.perm1 = p1.data();
    p.perm2 = p2.data();
    zip_ctx *const untouched = reinterpret_cast<zip_ctx *>(0x1);
    zip_ctx *ctx = untouched;

    // ---- admission: every triple but (1, 4, 8) and (2, 8, 16) is unsupported, before anything else is looked at
    const uint32_t bad[][3] = {{2, 4, 8}, {2, 8, 8}, {1, 8, 16}, {3, 12, 24}, {0, 0, 0}, {2, 16, 8}};
    for (const auto &t : bad) {
        zip_params q = p;
        q.n_limbs = t[0];
        q.k_limbs = t[1];
        q.m_limbs = t[2];
        q.row_len = 3;  // (not a power of two: the triple is refused first)
        ctx = untouched;
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_UNSUPPORTED);
        EXPECT(ctx == nullptr);
    }
    // ---- a two-limb ctx has no row shards
    const uint32_t shards[][2] = {{0, 8}, {8, 8}, {1, 0}};  // (row_begin, row_count)
    for (const auto &s : shards) {
        zip_params q = p;
        q.row_begin = s[0];
        q.row_count = s[1];
        ctx = untouched;
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_UNSUPPORTED);
        EXPECT(ctx == nullptr);
    }
    {
        const int32_t devices[2] = {0, 1};
        zip_mctx *m = reinterpret_cast<zip_mctx *>(0x1);
        EXPECT(zip_mctx_create(&p, 2, devices, &m) == ZIP_ERR_UNSUPPORTED);
        EXPECT(m == nullptr);
        EXPECT(zip_mctx_create(&p, 2, nullptr, &m) == ZIP_ERR_NULL);
    }
    // ---- shape and parameter errors of a two-limb geometry
    {
        zip_params q = p;
        q.num_rows = 32;  // 16 x 32 != 2^8
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_INVALID_PARAM);
        q = p;
        q.codeword_len = 64;  // != row_len * rep
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_INVALID_PARAM);
        q = p;
        q.perm1 = nullptr;
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_NULL);
        std::vector<uint32_t> twice = p1;
        twice[3] = twice[4];
        q = p;
        q.perm2 = twice.data();
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_INVALID_PARAM);
        // codewords above 65536: unsupported, as for one limb (2^16 = 32768 x 2, rep 4; the permutations are not read)
        q = p;
        q.num_vars = 16;
        q.row_len = 32768;
        q.num_rows = 2;
        q.rep = 4;
        q.codeword_len = 131072;
        EXPECT(zip_ctx_create(&q, &ctx) == ZIP_ERR_UNSUPPORTED);
        EXPECT(zip_ctx_create(nullptr, &ctx) == ZIP_ERR_NULL);
        EXPECT(zip_ctx_create(&p, nullptr) == ZIP_ERR_NULL);
    }
    // ---- the admitted triple: without a device the answer is "no device", never "unsupported"
    if (zip_device_count() == 0) {
        ctx = untouched;
        EXPECT(zip_ctx_create(&p, &ctx) == ZIP_ERR_NO_DEVICE);
        EXPECT(ctx == nullptr);
    }

    // ---- every call that refuses a live two-limb ctx: no ctx, no handle -> ZIP_ERR_NULL, nothing written
    std::vector<int64_t> evals(2 * 256, 7), coeffs(2 * 16, 1);
    std::vector<uint64_t> q0(16 * 4, 1), out64(16 * 16, 9);
    std::vector<uint8_t> proof(4096, 0xAB);
    uint32_t cols[2] = {0, 31};
    zip_field f{};
    f.limbs = 4;
    f.modulus[0] = 5;
    f.modulus[3] = 1;
    EXPECT(zip_ctx_set_proximity_tests(nullptr, 2) == ZIP_ERR_NULL);
    EXPECT(zip_ctx_set_speculation(nullptr, 1) == ZIP_ERR_NULL);
    EXPECT(zip_open_shard(nullptr, evals.data(), coeffs.data(), cols, 2, q0.data(), &f, out64.data(), out64.data(), proof.data()) == ZIP_ERR_NULL);
    zip_job *job = reinterpret_cast<zip_job *>(0x1);
    EXPECT(zip_commit_open_begin(nullptr, evals.data(), 256, coeffs.data(), cols, 2, q0.data(), &f, proof.data(), &job) == ZIP_ERR_NULL);
    EXPECT(job == reinterpret_cast<zip_job *>(0x1));
    EXPECT(zip_open_stream(nullptr, evals.data(), ZIP_MEM_HOST, coeffs.data(), cols, 2, q0.data(), &f,
                           [](void *, const uint8_t *, size_t) -> int32_t { return 0; }, nullptr, 0) == ZIP_ERR_NULL);
    zip_batch *batch = reinterpret_cast<zip_batch *>(0x1);
    EXPECT(zip_batch_commit(nullptr, evals.data(), 256, 1, ZIP_MEM_HOST, nullptr, &batch) == ZIP_ERR_NULL);
    EXPECT(zip_batch_commit_codes(nullptr, evals.data(), 256, 1, ZIP_MEM_HOST, p1.data(), p2.data(), nullptr, &batch) == ZIP_ERR_NULL);
    EXPECT(batch == reinterpret_cast<zip_batch *>(0x1));
    zip_verify_report rep;
    std::memset(&rep, 0x5A, sizeof rep);
    uint8_t roots[16 * 32] = {0};
    EXPECT(zip_batch_verify(nullptr, 1, roots, proof.data(), ZIP_MEM_HOST, proof.size(), coeffs.data(), cols, 2, q0.data(), q0.data(),
                            q0.data(), &f, &rep) == ZIP_ERR_NULL);
    EXPECT(zip_sum_partials(nullptr, out64.data(), nullptr, 2, &f, out64.data(), nullptr) == ZIP_ERR_NULL);

    // ---- the served two-limb calls: NULL first
    zip_commitment *com = reinterpret_cast<zip_commitment *>(0x1);
    EXPECT(zip_commit(nullptr, evals.data(), 256, ZIP_MEM_HOST, 1, nullptr, &com) == ZIP_ERR_NULL);
    EXPECT(zip_commit_hinted(nullptr, evals.data(), 256, ZIP_MEM_HOST, cols, 2, nullptr, &com) == ZIP_ERR_NULL);
    EXPECT(com == reinterpret_cast<zip_commitment *>(0x1));
    EXPECT(zip_commit_open(nullptr, evals.data(), 256, ZIP_MEM_HOST, coeffs.data(), cols, 2, q0.data(), &f, nullptr, proof.data(),
                           ZIP_MEM_HOST, nullptr) == ZIP_ERR_NULL);
    EXPECT(zip_open_testing(nullptr, evals.data(), ZIP_MEM_HOST, coeffs.data(), out64.data(), ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_open_eval(nullptr, evals.data(), ZIP_MEM_HOST, q0.data(), &f, out64.data(), ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_open_columns(nullptr, cols, 2, proof.data(), ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_open(nullptr, evals.data(), ZIP_MEM_HOST, coeffs.data(), cols, 2, q0.data(), &f, proof.data(), ZIP_MEM_HOST) == ZIP_ERR_NULL);
    EXPECT(zip_mle_eval(nullptr, evals.data(), ZIP_MEM_HOST, q0.data(), q0.data(), &f, out64.data()) == ZIP_ERR_NULL);
    EXPECT(zip_verify(nullptr, roots, proof.data(), ZIP_MEM_HOST, proof.size(), coeffs.data(), cols, 2, q0.data(), q0.data(), q0.data(),
                      &f, &rep) == ZIP_ERR_NULL);
    EXPECT(zip_commitment_upload(nullptr, out64.data(), nullptr, nullptr, &com) == ZIP_ERR_NULL);
    EXPECT(zip_field_map_int(nullptr, out64.data(), 4, 2, &f, out64.data()) == ZIP_ERR_NULL);
    EXPECT(zip_field_map_int(nullptr, nullptr, 4, 8, &f, nullptr) == ZIP_ERR_NULL);
    EXPECT(zip_proof_len(nullptr, 12, 4) == 0);
    EXPECT(std::strcmp(zip_ctx_last_error(nullptr), "") == 0);
    for (uint64_t v : out64) EXPECT(v == 9);
    for (uint8_t v : proof) EXPECT(v == 0xAB);
    {
        zip_verify_report same;
        std::memset(&same, 0x5A, sizeof same);
        EXPECT(std::memcmp(&rep, &same, sizeof rep) == 0);
    }
    if (failures) return 1;
    std::puts("two_limb_check ok");
    return 0;
}
