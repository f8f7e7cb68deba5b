// Batch kernels: the open of MANY small polynomials that share one zip_ctx (zip_batch_open_eval, zip_batch_open).
// The polynomial is a grid dimension, so the number of launches does not depend on how many there are.
//
// Reference loops replaced (per polynomial, as in kernels_open.cuh):
//   combine_rows over Int<M>           src/zip/utils.rs:94-127 via src/zip/pcs/open_z.rs:103-112
//   map_to_field + combine_rows over F src/zip/pcs/open_z.rs:76-90
//   open_merkle_trees_for_column       src/zip/pcs/open_z.rs:124-143
// and the loop over the polynomials itself, src/zip/pcs/open_z.rs:43-58.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_open.cuh"

namespace zipk {

// ---------------------------------------------------------------------------
// Batched row combinations.  Grid (column blocks, polynomials), one thread per witness column.  The sums are the
// ones of combine_rows_kernel (unsigned operands, bias terms applied at the end: see there), but ONE thread walks
// ALL rows of its column and finishes it: at the sizes a batch is for (<= 256 rows) the polynomials supply the
// parallelism that the row chunks of the single-polynomial kernel are there to create, and without partial sums
// there is no second kernel.  Row r's coefficient and q0 entry come from polynomial b's slice by scalar loads.
// ---------------------------------------------------------------------------
struct BatchCombineArgs {
    const int64_t *evals;   // [n_polys][num_rows][row_len]
    const int64_t *coeffs;  // [n_polys][num_rows]       (device; DO_INT)
    const uint64_t *q0;     // [n_polys][num_rows][FL]   (device, Montgomery limbs), or ONE slice for all: q0_shared
    uint32_t q0_shared;     // num_rows == 1: every polynomial multiplies by 1_mont (open_z.rs:84-88)
    uint32_t num_rows, row_len, m_limbs;
    uint64_t quirk_mod;
    // where polynomial b's results go: u' [row_len][m_limbs] little-endian limbs at uprime + b * out_stride, the
    // big-endian evaluation row [row_len][8 FL] at row_be + b * out_stride (both inside proof stream b), the
    // evaluation row as Montgomery limbs at row_limbs + b * row_len * FL.  Any of them may be null.
    uint8_t *uprime, *row_be;
    size_t out_stride;
    uint64_t *row_limbs;
};

constexpr uint32_t kBatchCombineThreads = 64;

// The signed-modulus quirk (make_field, combine_rows_kernel) of the members of one launch: none of them, all of them
// (one modulus: zip_batch_open), or decided per member at run time, quirk_mod == 0 meaning none (batch_combine_fields_kernel)
enum BatchQuirk { kQuirkNone = 0, kQuirkAlways = 1, kQuirkPerMember = 2 };

// A launch over the members [first, first + grid) of a batch (zip_batch_open_each): block position p reads the inputs of
// member first + p.  Its stream goes to slot position p (dst == nullptr: base + p * stride, as in the launches over the
// whole batch) or to dst[first + p], a device table with one stream base per member of the batch; the evaluation row
// then sits row_be_at bytes into the stream, u' at its start.  Everything here is wave-uniform.
struct BatchEachArgs {
    uint32_t first;
    uint8_t *const *dst;
    size_t row_be_at;
};

// member m's entry of the table, through the scalar cache (the table was uploaded before the launch)
__device__ __forceinline__ uint8_t *batch_each_stream(const BatchEachArgs &e, uint32_t m) {
    const auto *tab = (const __attribute__((address_space(4))) uint64_t *)(uintptr_t)e.dst;
    return reinterpret_cast<uint8_t *>((uintptr_t)tab[m]);
}

// polynomial blockIdx.y in the field f (quirk_mod: its 2^(64 FL) - q where that fits 64 bits, see BatchQuirk).
// EACH: polynomial e.first + blockIdx.y, written where BatchEachArgs says
template <int FL, bool DO_INT, int QUIRK, bool EACH = false>
__device__ __forceinline__ void batch_combine_body(const BatchCombineArgs &a, const FieldDev<FL> &f, uint64_t quirk_mod,
                                                   const BatchEachArgs &e = BatchEachArgs{}) {
    const uint32_t col = blockIdx.x * kBatchCombineThreads + threadIdx.x;
    const uint32_t ob = blockIdx.y;                    // the position among this launch's outputs
    const uint32_t b = EACH ? e.first + ob : ob;       // the polynomial
    const bool to_table = EACH && e.dst != nullptr;
    const uint32_t R = a.num_rows;
    constexpr uint64_t kBias = 1ull << 63;

    WideAcc<3> P;           // sum c' w'
    WideAcc<1> W;           // sum w'
    WideAcc<2 * FL + 1> A;  // sum q0 w'
    P.clear();
    W.clear();
    A.clear();
    // the column-independent sums (wave-uniform: they stay in scalar registers)
    uint64_t Kq[FL + 1], Kc[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < FL + 1; i++) Kq[i] = 0;

    const bool live = col < a.row_len;
    const int64_t *p = a.evals + (size_t)b * R * a.row_len + (live ? col : 0);
    const auto *coeffs_k = (const __attribute__((address_space(4))) int64_t *)(uintptr_t)(a.coeffs + (DO_INT ? (size_t)b * R : 0));
    const auto *q0_k = (const __attribute__((address_space(4))) uint64_t *)(uintptr_t)(a.q0 + (a.q0_shared ? 0 : (size_t)b * R * FL));
    auto one_row = [&](int64_t w, uint32_t r) {
        const uint64_t wb = (uint64_t)w ^ kBias;
        uint32_t w0 = (uint32_t)wb, w1 = (uint32_t)(wb >> 32);
        if (DO_INT) {
            const uint64_t cb = (uint64_t)coeffs_k[r] ^ kBias;
            const uint32_t c[2] = {(uint32_t)cb, (uint32_t)(cb >> 32)};
            mad_words<2>(P, c, w0, w1);
            W.template add<0>(wb);
            const uint64_t t[2] = {cb, 0};
            add_n<2>(Kc, t);
        }
        if (QUIRK == kQuirkAlways || (QUIRK == kQuirkPerMember && quirk_mod)) {  // (the field half only: see combine_rows_kernel)
            const uint64_t mag = (w < 0 ? (uint64_t)0 - (uint64_t)w : (uint64_t)w) % quirk_mod;
            const uint64_t qb = (uint64_t)((w < 0) ? -(int64_t)mag : (int64_t)mag) ^ kBias;
            w0 = (uint32_t)qb;
            w1 = (uint32_t)(qb >> 32);
        }
        const auto *q = q0_k + (size_t)r * FL;
        uint32_t qw[2 * FL];
        uint64_t t[FL + 1];
#pragma unroll
        for (int i = 0; i < FL; i++) {
            const uint64_t qi = q[i];
            qw[2 * i] = (uint32_t)qi;
            qw[2 * i + 1] = (uint32_t)(qi >> 32);
            t[i] = qi;
        }
        t[FL] = 0;
        add_n<FL + 1>(Kq, t);
        mad_words<2 * FL>(A, qw, w0, w1);
    };
    uint32_t r = 0;
    for (; r + kCombineUnroll <= R; r += kCombineUnroll, p += (size_t)kCombineUnroll * a.row_len) {
        int64_t w[kCombineUnroll];
#pragma unroll
        for (int k = 0; k < kCombineUnroll; k++) w[k] = p[(size_t)k * a.row_len];
#pragma unroll
        for (int k = 0; k < kCombineUnroll; k++) one_row(w[k], r + k);
    }
    for (; r < R; r++, p += a.row_len) one_row(*p, r);
    if (!live) return;

    if (DO_INT && (a.uprime || to_table)) {
        // sum c w = P - 2^63 (W + sum c') + rows 2^126   (mod 2^192: the value fits)
        uint64_t s[3], ws[2], t[3];
        P.template pack<3>(s);
        W.template pack<2>(ws);
        t[0] = ws[0] << 63;
        t[1] = (ws[0] >> 1) | (ws[1] << 63);
        t[2] = ws[1] >> 1;
        sub_n<3>(s, t);
        uint64_t k[3] = {Kc[0] << 63, (Kc[0] >> 1) | (Kc[1] << 63), Kc[1] >> 1};
        sub_n<3>(s, k);
        uint64_t u[3] = {0, (uint64_t)(R & 3u) << 62, (uint64_t)(R >> 2)};
        add_n<3>(s, u);
        const uint64_t sign = (uint64_t)((int64_t)s[2] >> 63);
        uint8_t *stream = to_table ? batch_each_stream(e, b) : a.uprime + (size_t)ob * a.out_stride;
        uint64_t *dst = reinterpret_cast<uint64_t *>(stream) + (size_t)col * a.m_limbs;
        for (uint32_t i = 0; i < a.m_limbs; i++) dst[i] = i < 3 ? s[i] : sign;  // write_integer, pcs_transcript.rs:115-123
    }
    {
        // sum q0 w = A - 2^63 sum q0, both reduced mod q
        uint64_t Al[FL + 2], Bs[FL + 2];
        A.template pack<FL + 2>(Al);
        Bs[0] = Kq[0] << 63;
#pragma unroll
        for (int i = 1; i < FL + 1; i++) Bs[i] = (Kq[i - 1] >> 1) | (Kq[i] << 63);
        Bs[FL + 1] = Kq[FL] >> 1;
        uint64_t ra[FL], rb[FL];
        reduce_wide<FL>(Al, f, ra);
        reduce_wide<FL>(Bs, f, rb);
        if (!geq_n<FL>(ra, rb)) add_n<FL>(ra, f.modulus);  // (wraps mod 2^(64 FL) when q has no spare bit; fine)
        sub_n<FL>(ra, rb);
        if (a.row_limbs) {
            uint64_t *dst = a.row_limbs + ((size_t)ob * a.row_len + col) * FL;
#pragma unroll
            for (int i = 0; i < FL; i++) dst[i] = ra[i];
        }
        if (a.row_be || to_table) {  // BigInt::to_bytes_be of the Montgomery value, pcs_transcript.rs:107-113
            uint8_t *stream = to_table ? batch_each_stream(e, b) + e.row_be_at : a.row_be + (size_t)ob * a.out_stride;
            uint64_t *dst = reinterpret_cast<uint64_t *>(stream) + (size_t)col * FL;
#pragma unroll
            for (int i = 0; i < FL; i++) dst[i] = __builtin_bswap64(ra[FL - 1 - i]);
        }
    }
}

template <int FL, bool DO_INT, bool QUIRK>
__global__ void __launch_bounds__(kBatchCombineThreads) batch_combine_kernel(BatchCombineArgs a, FieldDev<FL> f) {
    batch_combine_body<FL, DO_INT, QUIRK ? kQuirkAlways : kQuirkNone>(a, f, a.quirk_mod);
}

// One field per polynomial (zip_batch_open_eval_fields, zip_batch_open_fields): polynomial b's field constants and
// quirk_mod are entry b of a device array.  The entry sits at a wave-uniform address, so it is read through the scalar
// cache (as kernels_spartan_batch.cuh reads its per-instance arguments); BatchCombineArgs.quirk_mod is not read, and
// q0 is never shared: with one row, polynomial b multiplies by ITS 1_mont.
template <int FL>
struct BatchFieldInst {
    FieldDev<FL> f;
    uint64_t quirk_mod;  // 0: this member's modulus has no quirk
};

template <int FL, bool DO_INT>
__global__ void __launch_bounds__(kBatchCombineThreads)
batch_combine_fields_kernel(BatchCombineArgs a, const BatchFieldInst<FL> *__restrict__ inst) {
    const BatchFieldInst<FL> &m = inst[blockIdx.y];
    batch_combine_body<FL, DO_INT, kQuirkPerMember>(a, m.f, m.quirk_mod);
}

// batch_combine_fields_kernel over the members [e.first, e.first + gridDim.y) (zip_batch_open_each)
template <int FL, bool DO_INT>
__global__ void __launch_bounds__(kBatchCombineThreads)
batch_combine_each_kernel(BatchCombineArgs a, const BatchFieldInst<FL> *__restrict__ inst, BatchEachArgs e) {
    const BatchFieldInst<FL> &m = inst[e.first + blockIdx.y];
    batch_combine_body<FL, DO_INT, kQuirkPerMember, true>(a, m.f, m.quirk_mod, e);
}

// ---------------------------------------------------------------------------
// Batched column openings: open_columns_kernel (natural layout, LDS image of the path records) with the polynomial
// as blockIdx.z.  Polynomial b owns rows [b num_rows, (b + 1) num_rows) of the batch's row entries and trees, reads
// cols[b][.] and writes into proof stream b.  A stream starts at a multiple of 8 bytes, not of 16: the values go out
// as 16-byte stores to 8-byte-aligned addresses and the records take the 8-byte path where they must.
// Grid (n_cols, row blocks, n_polys); dynamic LDS rows_per_block * (8 + 32 depth) bytes.
// (batch_open_columns_each_kernel below is a copy of this kernel with another member index and stream base: a fix to
// the gather here is a fix there too.)
// ---------------------------------------------------------------------------
struct BatchOpenColsArgs {
    const uint64_t *rows;    // [n_polys * num_rows][cw][2]   16-byte entries (w0, w1, w2, sign)
    const uint64_t *layers;  // [n_polys * num_rows][2 cw][4]
    const uint32_t *cols;    // [n_polys][n_cols] (device)
    uint8_t *out;            // proof stream 0; stream b at out + b * stream_bytes
    size_t stream_bytes, openings_at;  // length of one stream; where its column openings start (behind u')
    uint32_t n_cols, num_rows, cw, depth;
    uint32_t rows_per_block;  // <= 128
};

template <int SLOTS>
__global__ void __launch_bounds__(256) batch_open_columns_kernel(BatchOpenColsArgs a) {
    extern __shared__ __align__(16) unsigned char img[];
    constexpr uint32_t K = 4;
    constexpr uint32_t RPP = 256 / SLOTS;
    const uint32_t ci = blockIdx.x, b = blockIdx.z;
    const uint32_t col = a.cols[(size_t)b * a.n_cols + ci];
    const uint32_t d = a.depth, cw2 = 2u * a.cw;
    const uint32_t rec_bytes = 8 + 32 * d;
    const size_t col_bytes = (size_t)a.num_rows * (8 * K + rec_bytes);
    uint8_t *base = a.out + (size_t)b * a.stream_bytes + a.openings_at + (size_t)ci * col_bytes;
    const uint32_t r0 = blockIdx.y * a.rows_per_block;
    const uint32_t r1 = min(r0 + a.rows_per_block, a.num_rows);
    const uint32_t nrows = r1 - r0;
    const size_t g0 = (size_t)b * a.num_rows + r0;  // the block's first row among the batch's rows

    // ---- phase 1: sibling hashes into the LDS image (lane roles as in open_columns_kernel) ----
    {
        const uint32_t h = threadIdx.x & (SLOTS - 1), rsub = threadIdx.x / SLOTS;
        const uint32_t lvl = h >> 1;
        const uint32_t node = cw2 - (cw2 >> lvl) + ((col >> lvl) ^ 1u);
        const uint64_t *src = a.layers + ((g0 + rsub) * cw2 + node) * 4 + (h & 1) * 2;
        const size_t src_step = (size_t)RPP * cw2 * 4;
        unsigned char *dst = img + (size_t)rsub * rec_bytes + 8 + (size_t)h * 16;
        const uint32_t dst_step = RPP * rec_bytes;
        if (h < 2 * d) {
#pragma unroll 4
            for (uint32_t rr = rsub; rr < nrows; rr += RPP, src += src_step, dst += dst_step) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(src);
                reinterpret_cast<uint64_t *>(dst)[0] = v.x;
                reinterpret_cast<uint64_t *>(dst)[1] = v.y;
            }
        } else if (h == 2 * d) {
            const uint64_t hdr = __builtin_bswap64((uint64_t)d);
            for (uint32_t rr = rsub; rr < nrows; rr += RPP)
                *reinterpret_cast<uint64_t *>(img + (size_t)rr * rec_bytes) = hdr;
        }
    }
    // ---- column values: the Int<4> of a 16-byte entry is (w0, w1 | w2, sign | sign x 4) ----
    {
        const uint32_t half = threadIdx.x & 1, rsub = threadIdx.x >> 1;
        if (rsub < nrows) {
            const uint4 e = *reinterpret_cast<const uint4 *>(a.rows + ((g0 + rsub) * a.cw + col) * 2);
            const uint64_t ss = ((uint64_t)e.w << 32) | e.w;
            oc_u128_a8 v;
            v.x = half ? ss : ((uint64_t)e.y << 32) | e.x;
            v.y = half ? ss : ((uint64_t)e.w << 32) | e.z;
            *reinterpret_cast<oc_u128_a8 *>(base + (size_t)(r0 + rsub) * 8 * K + half * 16) = v;
        }
    }
    __syncthreads();
    // ---- phase 2: stream the image out ----
    unsigned char *recs = base + (size_t)a.num_rows * 8 * K + (size_t)r0 * rec_bytes;
    const uint32_t total = nrows * rec_bytes;
    if ((reinterpret_cast<uintptr_t>(recs) & 15) == 0) {
        const uint32_t n16 = total / 16;
        for (uint32_t i = threadIdx.x; i < n16; i += 256)
            reinterpret_cast<uint4 *>(recs)[i] = reinterpret_cast<const uint4 *>(img)[i];
        if (threadIdx.x == 0 && (total & 15))
            reinterpret_cast<uint64_t *>(recs)[n16 * 2] = reinterpret_cast<const uint64_t *>(img)[n16 * 2];
    } else {
        for (uint32_t i = threadIdx.x; i < total / 8; i += 256)
            reinterpret_cast<uint64_t *>(recs)[i] = reinterpret_cast<const uint64_t *>(img)[i];
    }
}

// batch_open_columns_kernel over the members [e.first, e.first + gridDim.z) (zip_batch_open_each): polynomial
// e.first + blockIdx.z, its stream at slot position blockIdx.z or at its entry of e.dst (BatchEachArgs).  The LDS image
// and the stores are the ones above; only where the polynomial's inputs and its stream are found differs -- a sibling
// and not a shared body, because the kernel above keeps its code to the instruction.
template <int SLOTS>
__global__ void __launch_bounds__(256) batch_open_columns_each_kernel(BatchOpenColsArgs a, BatchEachArgs e) {
    extern __shared__ __align__(16) unsigned char img[];
    constexpr uint32_t K = 4;
    constexpr uint32_t RPP = 256 / SLOTS;
    const uint32_t ci = blockIdx.x, ob = blockIdx.z;
    const uint32_t b = e.first + ob;
    const uint32_t col = a.cols[(size_t)b * a.n_cols + ci];
    const uint32_t d = a.depth, cw2 = 2u * a.cw;
    const uint32_t rec_bytes = 8 + 32 * d;
    const size_t col_bytes = (size_t)a.num_rows * (8 * K + rec_bytes);
    uint8_t *stream = e.dst ? batch_each_stream(e, b) : a.out + (size_t)ob * a.stream_bytes;
    uint8_t *base = stream + a.openings_at + (size_t)ci * col_bytes;
    const uint32_t r0 = blockIdx.y * a.rows_per_block;
    const uint32_t r1 = min(r0 + a.rows_per_block, a.num_rows);
    const uint32_t nrows = r1 - r0;
    const size_t g0 = (size_t)b * a.num_rows + r0;  // the block's first row among the batch's rows

    // ---- phase 1: sibling hashes into the LDS image (lane roles as in open_columns_kernel) ----
    {
        const uint32_t h = threadIdx.x & (SLOTS - 1), rsub = threadIdx.x / SLOTS;
        const uint32_t lvl = h >> 1;
        const uint32_t node = cw2 - (cw2 >> lvl) + ((col >> lvl) ^ 1u);
        const uint64_t *src = a.layers + ((g0 + rsub) * cw2 + node) * 4 + (h & 1) * 2;
        const size_t src_step = (size_t)RPP * cw2 * 4;
        unsigned char *dst = img + (size_t)rsub * rec_bytes + 8 + (size_t)h * 16;
        const uint32_t dst_step = RPP * rec_bytes;
        if (h < 2 * d) {
#pragma unroll 4
            for (uint32_t rr = rsub; rr < nrows; rr += RPP, src += src_step, dst += dst_step) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(src);
                reinterpret_cast<uint64_t *>(dst)[0] = v.x;
                reinterpret_cast<uint64_t *>(dst)[1] = v.y;
            }
        } else if (h == 2 * d) {
            const uint64_t hdr = __builtin_bswap64((uint64_t)d);
            for (uint32_t rr = rsub; rr < nrows; rr += RPP)
                *reinterpret_cast<uint64_t *>(img + (size_t)rr * rec_bytes) = hdr;
        }
    }
    // ---- column values: the Int<4> of a 16-byte entry is (w0, w1 | w2, sign | sign x 4) ----
    {
        const uint32_t half = threadIdx.x & 1, rsub = threadIdx.x >> 1;
        if (rsub < nrows) {
            const uint4 ent = *reinterpret_cast<const uint4 *>(a.rows + ((g0 + rsub) * a.cw + col) * 2);
            const uint64_t ss = ((uint64_t)ent.w << 32) | ent.w;
            oc_u128_a8 v;
            v.x = half ? ss : ((uint64_t)ent.y << 32) | ent.x;
            v.y = half ? ss : ((uint64_t)ent.w << 32) | ent.z;
            *reinterpret_cast<oc_u128_a8 *>(base + (size_t)(r0 + rsub) * 8 * K + half * 16) = v;
        }
    }
    __syncthreads();
    // ---- phase 2: stream the image out ----
    unsigned char *recs = base + (size_t)a.num_rows * 8 * K + (size_t)r0 * rec_bytes;
    const uint32_t total = nrows * rec_bytes;
    if ((reinterpret_cast<uintptr_t>(recs) & 15) == 0) {
        const uint32_t n16 = total / 16;
        for (uint32_t i = threadIdx.x; i < n16; i += 256)
            reinterpret_cast<uint4 *>(recs)[i] = reinterpret_cast<const uint4 *>(img)[i];
        if (threadIdx.x == 0 && (total & 15))
            reinterpret_cast<uint64_t *>(recs)[n16 * 2] = reinterpret_cast<const uint64_t *>(img)[n16 * 2];
    } else {
        for (uint32_t i = threadIdx.x; i < total / 8; i += 256)
            reinterpret_cast<uint64_t *>(recs)[i] = reinterpret_cast<const uint64_t *>(img)[i];
    }
}

}  // namespace zipk
