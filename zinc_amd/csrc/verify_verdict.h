// The order in which MultilinearZip::verify's checks turn into a verdict (src/zip/pcs/verify_z.rs:60-188), written once
// for zip_verify's host code and batch_verify_report_kernel's device code alike:
//   encode_wide(u') overflows                                              verify_z.rs:75-77, int.rs:122-134
//   per opening, in transcript order: the proximity test over Z, then its
//   Merkle records (a wrong length prefix, then a path that misses its root) verify_z.rs:88-127
//   <row, q1> differs from the claimed evaluation                          verify_z.rs:139-149
//   an evaluation-row element >= q (zip_verify's documented deviation: after the consistency check, which is
//   representation independent)
//   per opening: the proximity test over F_q                               verify_z.rs:165-188
// The callers reduce their flags and counts to the facts below; no HIP header is needed here.
#pragma once
#include <stdint.h>

#include "../../include/zip_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZV_HD __host__ __device__ __forceinline__
#else
#define ZV_HD inline
#endif

namespace zipk {

constexpr uint32_t kNoOpening = 0xFFFFFFFFu;
// what an opening fails (VerifyFacts::first_why), in the order the reference meets them
constexpr uint32_t kFailsProximity = 1u, kFailsMalformed = 2u, kFailsMerkle = 4u;

// flags: bit 0 = the opening's proximity test over Z failed; the counts of its wrong prefixes and wrong paths
ZV_HD uint32_t opening_fails(uint32_t flags, uint32_t malformed, uint32_t bad_merkle) {
    return ((flags & 1u) ? kFailsProximity : 0u) | (malformed ? kFailsMalformed : 0u) | (bad_merkle ? kFailsMerkle : 0u);
}

struct VerifyFacts {
    bool overflow;       // encode_wide(u') left Int<M>
    uint32_t first;      // first opening that fails the proximity test over Z, a length prefix or a path; kNoOpening
    uint32_t first_why;  // kFails* bits of that opening
    bool eval_differs;   // <row, q1> != the claimed evaluation
    bool noncanonical;   // an evaluation-row element >= q
    uint32_t first_q0;   // first opening that fails the proximity test over F_q; kNoOpening
};

// sets rep.verdict and rep.column (0 unless the verdict names an opening); the counts are the caller's
ZV_HD void verify_verdict(const VerifyFacts &x, zip_verify_report &rep) {
    rep.verdict = ZIP_VERIFY_ACCEPT;
    rep.column = 0;
    if (x.overflow) {
        rep.verdict = ZIP_VERIFY_OVERFLOW;
    } else if (x.first != kNoOpening) {
        rep.column = x.first;
        rep.verdict = (x.first_why & kFailsProximity) ? ZIP_VERIFY_PROXIMITY_TESTING
                      : (x.first_why & kFailsMalformed) ? ZIP_VERIFY_MALFORMED
                                                        : ZIP_VERIFY_MERKLE;
    } else if (x.eval_differs) {
        rep.verdict = ZIP_VERIFY_EVAL_CONSISTENCY;
    } else if (x.noncanonical) {
        rep.verdict = ZIP_VERIFY_MALFORMED;
    } else if (x.first_q0 != kNoOpening) {
        rep.verdict = ZIP_VERIFY_PROXIMITY_Q0;
        rep.column = x.first_q0;
    }
}

}  // namespace zipk
