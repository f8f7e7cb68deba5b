// Stand-alone: zip_batch_open_each and zip_batch_open_each_counts (include/zip_hip.h), called as a C caller on a machine
// that may have no device.  A zip_batch cannot exist without one, so what can be asked here is what the open answers
// before it looks at a handle -- ZIP_ERR_NULL, first, whatever else is wrong with the arguments, nothing written and the
// counters standing still -- and the counts call with every combination of NULL pointers.  (The errors behind a live
// handle are in tests/test_gpu_batch_open_each.py.)  Built by tests/test_batch_open_each_host.py with
// -fsanitize=address,undefined.
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
    uint64_t base[4] = {11, 12, 13, 14};
    zip_batch_open_each_counts(&base[0], &base[1], &base[2], &base[3]);
    EXPECT(base[0] == 0 && base[1] == 0 && base[2] == 0 && base[3] == 0);  // nothing has reached a device
    // every combination of NULL pointers: a pointer that is given receives its count, the others are left alone
    for (unsigned mask = 0; mask < 16; mask++) {
        uint64_t v[4] = {71, 72, 73, 74};
        zip_batch_open_each_counts(mask & 1 ? &v[0] : nullptr, mask & 2 ? &v[1] : nullptr, mask & 4 ? &v[2] : nullptr,
                                   mask & 8 ? &v[3] : nullptr);
        for (unsigned k = 0; k < 4; k++) EXPECT(v[k] == ((mask >> k) & 1 ? base[k] : 71 + k));
    }

    // the open: no batch
    zip_field f{};
    f.limbs = 4;
    f.modulus[0] = 4;  // even: still NULL first
    const zip_field *fields[2] = {&f, nullptr};
    std::vector<uint64_t> q0(2 * 4 * 4, 1);
    std::vector<int64_t> coeffs(8, 1);
    uint32_t cols[4] = {0, 1, 2, 99};
    std::vector<uint8_t> proofs(256, 0xAB);
    uint8_t *table[2] = {proofs.data(), proofs.data() + 128};
    EXPECT(zip_batch_open_each(nullptr, coeffs.data(), cols, 2, q0.data(), fields, table, ZIP_MEM_HOST, 0) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_each(nullptr, coeffs.data(), cols, 2, q0.data(), fields, table, ZIP_MEM_DEVICE, 1) == ZIP_ERR_NULL);
    // inconsistent arguments: destinations that overlap, a NULL entry, an odd device address, no table, no columns
    uint8_t *overlap[2] = {proofs.data(), proofs.data() + 1};
    EXPECT(zip_batch_open_each(nullptr, coeffs.data(), cols, 2, q0.data(), fields, overlap, ZIP_MEM_HOST, 64) == ZIP_ERR_NULL);
    uint8_t *hole[2] = {proofs.data(), nullptr};
    EXPECT(zip_batch_open_each(nullptr, coeffs.data(), cols, 2, q0.data(), fields, hole, ZIP_MEM_HOST, 0) == ZIP_ERR_NULL);
    uint8_t *odd[2] = {proofs.data() + 4, proofs.data() + 132};
    EXPECT(zip_batch_open_each(nullptr, coeffs.data(), cols, 2, q0.data(), fields, odd, ZIP_MEM_DEVICE, 0) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_each(nullptr, coeffs.data(), cols, 2, q0.data(), fields, nullptr, ZIP_MEM_HOST, 0) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_each(nullptr, nullptr, nullptr, 2, nullptr, nullptr, nullptr, ZIP_MEM_DEVICE, ~(size_t)0) == ZIP_ERR_NULL);
    EXPECT(zip_batch_open_each(nullptr, nullptr, nullptr, 0, nullptr, nullptr, table, ZIP_MEM_HOST, 0) == ZIP_ERR_NULL);
    for (uint8_t v : proofs) EXPECT(v == 0xAB);

    uint64_t now[4];
    zip_batch_open_each_counts(&now[0], &now[1], &now[2], &now[3]);
    EXPECT(!std::memcmp(now, base, sizeof now));
    uint64_t c = 1, m = 2, fo = 3;
    zip_batch_codes_counts(&c, &m, &fo);
    EXPECT(c == 0 && m == 0 && fo == 0);
    if (failures) return 1;
    std::puts("batch_open_each_check ok");
    return 0;
}
