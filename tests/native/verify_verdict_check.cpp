// Host build of zinc_amd/csrc/verify_verdict.h for tests/test_verify_verdict_host.py: the order of checks zip_verify's
// host code and batch_verify_report_kernel share, driven from Python against the model of tests/_verify_cases.py.
#include "verify_verdict.h"

using namespace zipk;

extern "C" {
// first / first_q0: an opening index, or -1 for none.  why: bit 0 proximity, bit 1 malformed, bit 2 Merkle.
void vv_verdict(int overflow, int64_t first, uint32_t why, int eval_differs, int noncanonical, int64_t first_q0, int32_t *verdict,
                uint32_t *column) {
    static_assert(kFailsProximity == 1u && kFailsMalformed == 2u && kFailsMerkle == 4u, "the bits the test passes");
    VerifyFacts x;
    x.overflow = overflow != 0;
    x.first = first < 0 ? kNoOpening : (uint32_t)first;
    x.first_why = why;
    x.eval_differs = eval_differs != 0;
    x.noncanonical = noncanonical != 0;
    x.first_q0 = first_q0 < 0 ? kNoOpening : (uint32_t)first_q0;
    zip_verify_report rep = {-1, 0xFFFFFFFFu, 7u, 9u};
    verify_verdict(x, rep);
    *verdict = rep.verdict;
    *column = rep.column;
    if (rep.bad_merkle_paths != 7u || rep.malformed_paths != 9u) *verdict = -2;  // the counts are the caller's
}
}
