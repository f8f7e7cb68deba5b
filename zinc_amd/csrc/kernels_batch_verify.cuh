// Batched verifier kernels: MultilinearZip::verify of MANY small proofs that share one zip_ctx (zip_batch_verify).
// The polynomial is a grid dimension, so the number of launches does not depend on how many there are, and the verdict
// is folded on the device: n_polys reports come back, not 3 * n_cols words per proof.
//
// Reference loops replaced (per polynomial, as in kernels_verify.cuh):
//   encode_wide / encode_f (one row)             src/zip/code_raa.rs:107-138
//   read_field_elements + <row, q1>              src/zip/pcs_transcript.rs:138-160, src/zip/pcs/verify_z.rs:139-149
//   verify_column_testing / verify_proximity_q_0 src/zip/pcs/verify_z.rs:88-127,165-188
//   MerkleProof::verify                          src/zip/pcs/utils.rs:178-210
// and the loop over the polynomials itself, src/zip/pcs/verify_z.rs:40-58.
//
// Proof stream b starts at proofs + b * stream_bytes, a multiple of 8 bytes and not of 16: every wire load is 8 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake3.cuh"
#include "kernels_open.cuh"
#include "kernels_verify.cuh"
#include "verify_verdict.h"

namespace zipk {

// ---------------------------------------------------------------------------------------
// encode_row_kernel with the polynomial as blockIdx.x and the input row read where it lies in proof stream b:
//   FIELD = false: u', L-limb little-endian integers at the start of the stream; head[b].overflow
//   FIELD = true : the evaluation row, big-endian Montgomery values at in_at; head[b].noncanonical counts
//                  elements >= q (not range-checked by the reference: see zip_verify in zip_hip.h) and
//                  head[b].dot = <row, q1[b]> -- decode_field_row_kernel and field_dot_kernel in the same workgroup.
// Grid (n_polys), blockDim.x = T threads sized to cw by the host, dynamic LDS T * sizeof(EncElem<L, FIELD>).
// ---------------------------------------------------------------------------------------
struct BatchEncodeArgs {
    const uint8_t *proofs;
    size_t stream_bytes, in_at;
    uint32_t row_len, cw;
    const uint32_t *perm1, *perm2;
    uint64_t *tmp, *out;     // [n_polys][cw][L]
    const uint64_t *q1;      // FIELD: [n_polys][row_len][L], or null (row_len == 1)
    uint32_t clear_overflow; // FIELD: no encode_wide runs (num_rows == 1); this kernel zeroes head[b].overflow
    VerifyHead *head;        // [n_polys]
};

template <int L, bool FIELD>
__device__ __forceinline__ void batch_enc_load_wire(EncElem<L, FIELD> &x, const uint64_t *p) {
    if constexpr (FIELD) {
#pragma unroll
        for (int i = 0; i < L; i++) x.v[i] = __builtin_bswap64(p[L - 1 - i]);
    } else {
        enc_load<L, FIELD>(x, p);
    }
}

// polynomial blockIdx.x: its stream starts at `stream`, its code is (perm1, perm2), its field f
template <int L, bool FIELD>
__device__ __forceinline__ void batch_encode_body(const BatchEncodeArgs &a, const FieldDev<L> &f, const uint8_t *stream,
                                                  const uint32_t *perm1, const uint32_t *perm2) {
    extern __shared__ __align__(16) unsigned char benc_smem[];
    using El = EncElem<L, FIELD>;
    El *tot = reinterpret_cast<El *>(benc_smem);  // [blockDim.x]
    const uint32_t T = blockDim.x, tid = threadIdx.x, b = blockIdx.x, cw = a.cw;
    const uint64_t *in = reinterpret_cast<const uint64_t *>(stream + a.in_at);
    const bool ovf = raa_encode_row<L, FIELD>([&](uint32_t c, El &x) { batch_enc_load_wire<L, FIELD>(x, in + (size_t)c * L); },
                                              a.row_len, cw, perm1, perm2, a.tmp + (size_t)b * cw * L,
                                              a.out + (size_t)b * cw * L, f, tot);
    if constexpr (!FIELD) {
        const int any = __syncthreads_or(ovf ? 1 : 0);
        if (tid == 0) a.head[b].overflow = any ? 1u : 0u;
    } else {
        // the row once more: range check and <row, q1>
        uint32_t nc = 0;
        uint64_t acc[L];
#pragma unroll
        for (int i = 0; i < L; i++) acc[i] = 0;
        const uint64_t *q1 = a.q1 ? a.q1 + (size_t)b * a.row_len * L : nullptr;
        for (uint32_t c = tid; c < a.row_len; c += T) {
            El x;
            batch_enc_load_wire<L, FIELD>(x, in + (size_t)c * L);
            if (geq_n<L>(x.v, f.modulus)) nc++;
            if (q1) {
                uint64_t y[L], t[L];
                fe_load<L>(y, q1 + (size_t)c * L);
                mont_mul<L>(x.v, y, f, t);
                fe_add<L>(acc, t, f);
            }
        }
        const int any_nc = __syncthreads_or(nc ? 1 : 0);
#pragma unroll
        for (int i = 0; i < L; i++) tot[tid].v[i] = acc[i];
        __syncthreads();
        for (uint32_t s = T / 2; s > 0; s >>= 1) {  // (T is a power of two)
            if (tid < s) {
                El p = tot[tid];
                enc_add<L, FIELD>(p, tot[tid + s], f);
                tot[tid] = p;
            }
            __syncthreads();
        }
        if (tid == 0) {
            VerifyHead &h = a.head[b];
            if (a.clear_overflow) h.overflow = 0;
            h.noncanonical = any_nc ? 1u : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) h.dot[i] = i < L ? tot[0].v[i < L ? i : 0] : 0;
        }
    }
}

template <int L, bool FIELD>
__global__ void __launch_bounds__(1024) batch_encode_kernel(BatchEncodeArgs a, FieldDev<L> f) {
    batch_encode_body<L, FIELD>(a, f, a.proofs + (size_t)blockIdx.x * a.stream_bytes, a.perm1, a.perm2);
}

// ---------------------------------------------------------------------------------------
// One code and one field per polynomial (zip_batch_verify_codes): what differs between the members of a batch of Zinc
// proofs is entry b of a device array.  The entry sits at a wave-uniform address (blockIdx.x here, blockIdx.y in the
// column kernel), so its field constants and pointers are read through the scalar cache, as batch_combine_fields_kernel
// and kernels_spartan_batch.cuh read theirs.  The args' proofs / stream_bytes / perm1 / perm2 / quirk are not read.
// ---------------------------------------------------------------------------------------
template <int FL>
struct BatchVerifyMember {
    FieldDev<FL> f, fq;            // the member's field, and that of 2^256 - q (= f unless quirk)
    const uint8_t *stream;         // where its proof stream starts (8-byte aligned)
    const uint32_t *perm1, *perm2; // its RAA code: codeword_len entries each
    uint32_t quirk;                // 1: the modulus is a negative Int<4> in the reference (see opening_terms)
};

// FIELD: L == FL and the member's field encodes; else encode_wide, which reads no field (L = 8 for every FL)
template <int L, bool FIELD, int FL>
__global__ void __launch_bounds__(1024) batch_encode_codes_kernel(BatchEncodeArgs a, const BatchVerifyMember<FL> *__restrict__ inst) {
    const BatchVerifyMember<FL> &m = inst[blockIdx.x];
    if constexpr (FIELD) {
        static_assert(L == FL, "encode_f runs in the member's field");
        batch_encode_body<L, true>(a, m.f, m.stream, m.perm1, m.perm2);
    } else {
        const FieldDev<L> unused{};
        batch_encode_body<L, false>(a, unused, m.stream, m.perm1, m.perm2);
    }
}

// ---------------------------------------------------------------------------------------
// Every (polynomial, opening): hash the paths, form the two column inner products, compare them with the encoded
// combined rows.  A 256-thread workgroup serves ONE polynomial (blockIdx.y) and
//   num_rows <  256: 256 / num_rows consecutive openings, one thread per opened entry -- every lane hashes a path;
//   num_rows >= 256: one opening, thread t walks rows t, t + 256, ... (the polynomials supply the parallelism, as in
//                    batch_combine_kernel): no row-block partials, no finalize pass.
// The sums of an opening are reduced by a butterfly of wave shuffles over its min(num_rows, 64) lanes (384-bit
// wrap-around adds and modular adds: both commute), then over its waves through 4 LDS slots.
// flags[b][ci]: bit 0 = proximity test over Z failed (verify_z.rs:122-125), bit 1 = over F_q (:184-186).
// Grid (ceil(n_cols / openings per workgroup), n_polys).
// ---------------------------------------------------------------------------------------
struct BatchVerifyColsArgs {
    const uint8_t *proofs;
    size_t stream_bytes, openings_at;  // length of one stream; where its column openings start (behind u')
    const uint32_t *cols;    // [n_polys][n_cols]
    const int64_t *coeffs;   // [n_polys][num_rows] or null (num_rows == 1)
    const uint64_t *q0;      // [n_polys][num_rows][FL] Montgomery, or null (num_rows == 1)
    const uint32_t *roots;   // [n_polys][num_rows][8]
    const uint64_t *enc_u;   // [n_polys][cw][8] or null (num_rows == 1)
    const uint64_t *enc_f;   // [n_polys][cw][FL]
    uint32_t num_rows, depth, n_cols, cw, quirk;
    uint32_t *flags, *bad_merkle, *malformed;  // [n_polys][n_cols]
};

// polynomial blockIdx.y: its stream starts at `stream`; f, fq and quirk are its field's
template <int FL>
__device__ __forceinline__ void batch_verify_columns_body(const BatchVerifyColsArgs &a, const FieldDev<FL> &f, const FieldDev<FL> &fq,
                                                          bool quirk, const uint8_t *stream) {
    constexpr int W = 6 + FL;
    __shared__ uint64_t wave_sum[4][W];
    __shared__ uint32_t s_bad[256], s_mal[256];
    const uint32_t tid = threadIdx.x, b = blockIdx.y, R = a.num_rows;
    const uint32_t lgS = R < 256 ? (uint32_t)__ffs((int)R) - 1 : 8;  // (num_rows is a power of two)
    const uint32_t S = 1u << lgS;                                    // threads per opening
    const uint32_t o = tid >> lgS, r0 = tid & (S - 1);
    const uint32_t ci = (blockIdx.x << (8 - lgS)) + o;
    const bool live = ci < a.n_cols;
    s_bad[tid] = 0;
    s_mal[tid] = 0;
    __syncthreads();

    uint64_t si[6] = {0, 0, 0, 0, 0, 0}, sf[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) sf[i] = 0;
    uint32_t col = 0;
    if (live) {
        col = a.cols[(size_t)b * a.n_cols + ci];
        const uint32_t d = a.depth, rec_bytes = 8 + 32 * d;
        const size_t col_bytes = (size_t)R * (32 + rec_bytes);
        const uint8_t *base = stream + a.openings_at + (size_t)ci * col_bytes;
        const int64_t *coeffs = a.coeffs ? a.coeffs + (size_t)b * R : nullptr;
        const uint64_t *q0 = a.q0 ? a.q0 + (size_t)b * R * FL : nullptr;
        const uint32_t *roots = a.roots + (size_t)b * R * 8;
        uint32_t n_bad = 0, n_mal = 0;
        for (uint32_t r = r0; r < R; r += 256) {
            uint64_t v[4];
            fe_load<4>(v, reinterpret_cast<const uint64_t *>(base + (size_t)r * 32));
            opening_terms<FL, true>(v, coeffs ? coeffs + r : nullptr, q0 ? q0 + (size_t)r * FL : nullptr, f, fq, quirk, si, sf);
            const uint64_t *rec = reinterpret_cast<const uint64_t *>(base + (size_t)R * 32 + (size_t)r * rec_bytes);
            const MerkleRecord m = check_merkle_record(v, rec, d, col, roots + (size_t)r * 8);
            n_mal += m == kMerkleMalformed;
            n_bad += m == kMerkleBadPath;
        }
        if (n_bad) atomicAdd(&s_bad[o], n_bad);
        if (n_mal) atomicAdd(&s_mal[o], n_mal);
    }
    // ---- the sums of one opening: butterfly over its lanes of this wave (dead lanes hold zeros) ----
    const uint32_t span = S < 64 ? S : 64;
    for (uint32_t off = 1; off < span; off <<= 1) {
        uint64_t y[6], q[FL];
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] = __shfl_xor(si[i], (int)off);
#pragma unroll
        for (int i = 0; i < FL; i++) q[i] = __shfl_xor(sf[i], (int)off);
        column_sums_add<FL>(si, sf, y, q, f);
    }
    // ---- ... and over its waves (S = 128 or 256) ----
    if (S > 64 && (tid & 63) == 0) {
        fe_store<6>(wave_sum[tid >> 6], si);
        fe_store<FL>(wave_sum[tid >> 6] + 6, sf);
    }
    __syncthreads();
    if (!live || r0 != 0) return;
    if (S > 64) {
        const uint32_t w0 = tid >> 6, nw = S >> 6;
        for (uint32_t w = w0 + 1; w < w0 + nw; w++) {
            uint64_t y[6], q[FL];
            fe_load<6>(y, wave_sum[w]);
            fe_load<FL>(q, wave_sum[w] + 6);
            column_sums_add<FL>(si, sf, y, q, f);
        }
    }
    // ---- the opening's leader holds the complete column sums: compare, as verify_finalize_kernel does ----
    const size_t slot = (size_t)b * a.n_cols + ci, at = (size_t)b * a.cw + col;
    a.flags[slot] = column_flags<FL>(si, sf, a.enc_u ? a.enc_u + at * 8 : nullptr, 8, a.enc_f + at * FL);
    a.bad_merkle[slot] = s_bad[o];
    a.malformed[slot] = s_mal[o];
}

template <int FL>
__global__ void __launch_bounds__(256) batch_verify_columns_kernel(BatchVerifyColsArgs a, FieldDev<FL> f, FieldDev<FL> fq) {
    batch_verify_columns_body<FL>(a, f, fq, a.quirk != 0, a.proofs + (size_t)blockIdx.y * a.stream_bytes);
}

// zip_batch_verify_codes: the quirk is the member's, decided at run time as kQuirkPerMember is in batch_combine_body
template <int FL>
__global__ void __launch_bounds__(256) batch_verify_columns_codes_kernel(BatchVerifyColsArgs a,
                                                                          const BatchVerifyMember<FL> *__restrict__ inst) {
    const BatchVerifyMember<FL> &m = inst[blockIdx.y];
    batch_verify_columns_body<FL>(a, m.f, m.fq, m.quirk != 0, m.stream);
}

// ---------------------------------------------------------------------------------------
// One workgroup per polynomial folds its n_cols entries into a zip_verify_report: the two counts, and the first
// failing check in the order zip_verify applies (the reference's, verify_z.rs:60-163, with zip_verify's documented
// deviations).  evals: the claimed evaluations [n_polys][FL]; for a one-column matrix <row, q1> is 0.
// ---------------------------------------------------------------------------------------
struct BatchVerifyReportArgs {
    const uint32_t *flags, *bad_merkle, *malformed;  // [n_polys][n_cols]
    const VerifyHead *head;                          // [n_polys]
    const uint64_t *evals;                           // [n_polys][FL]
    uint32_t n_cols, row_len;
    zip_verify_report *reports;                      // [n_polys]
};

template <int FL>
__global__ void __launch_bounds__(256) batch_verify_report_kernel(BatchVerifyReportArgs a) {
    __shared__ uint32_t s_first_a, s_first_b, s_bad, s_mal;
    const uint32_t tid = threadIdx.x, b = blockIdx.x, n = a.n_cols;
    const uint32_t *flags = a.flags + (size_t)b * n, *bad = a.bad_merkle + (size_t)b * n, *mal = a.malformed + (size_t)b * n;
    if (tid == 0) {
        s_first_a = s_first_b = kNoOpening;
        s_bad = s_mal = 0;
    }
    __syncthreads();
    uint32_t first_a = kNoOpening, first_b = kNoOpening, n_bad = 0, n_mal = 0;
    for (uint32_t ci = tid; ci < n; ci += 256) {
        const uint32_t fl = flags[ci], nb = bad[ci], nm = mal[ci];
        n_bad += nb;
        n_mal += nm;
        if (opening_fails(fl, nm, nb) && first_a == kNoOpening) first_a = ci;
        if ((fl & 2u) && first_b == kNoOpening) first_b = ci;
    }
    if (n_bad) atomicAdd(&s_bad, n_bad);
    if (n_mal) atomicAdd(&s_mal, n_mal);
    if (first_a != kNoOpening) atomicMin(&s_first_a, first_a);
    if (first_b != kNoOpening) atomicMin(&s_first_b, first_b);
    __syncthreads();
    if (tid != 0) return;
    const VerifyHead &h = a.head[b];
    VerifyFacts x;
    x.overflow = h.overflow != 0;
    x.first = s_first_a;
    x.first_why = x.first != kNoOpening ? opening_fails(flags[x.first], mal[x.first], bad[x.first]) : 0u;
    x.eval_differs = false;
#pragma unroll
    for (int i = 0; i < FL; i++) x.eval_differs |= a.evals[(size_t)b * FL + i] != (a.row_len > 1 ? h.dot[i] : 0);
    x.noncanonical = h.noncanonical != 0;
    x.first_q0 = s_first_b;
    zip_verify_report rep;
    verify_verdict(x, rep);
    rep.bad_merkle_paths = s_bad;
    rep.malformed_paths = s_mal;
    a.reports[b] = rep;
}

}  // namespace zipk
