// INT_LIMBS = 2: the Zip PCS path for Int<2> witnesses (N = Int<2>, K = Int<8>, M = Int<16>; src/field/int.rs:276-288).
//
// Reference loops replaced, all at two limbs:
//   RaaCode::encode_inner + MerkleTree leaves     src/zip/code_raa.rs:89-171, src/zip/pcs/utils.rs:74-93
//   combine_rows over Int<16> and over F_q         src/zip/utils.rs:94-127 via open_z.rs:76-112
//   open_merkle_trees_for_column                   src/zip/pcs/open_z.rs:124-143
//   verify_column_testing / verify_proximity_q_0   src/zip/pcs/verify_z.rs:107-127, 165-188
//   FieldMap for Int<2> and Int<8>                 src/conversion.rs:86-100 over src/field.rs:536-568
//
// Widths.  A witness entry is 128-bit two's complement.  After the two accumulate passes an honest row entry needs
// 128 + 2 log2(cw) signed bits; the scan lanes here are THREE 64-bit limbs (192 bits), which holds for every codeword
// the ctx admits (cw <= 65536: 160 bits) with room to spare -- 64-bit limbs because every other multi-limb helper of
// this library (add_n, mont_mul) is written for them.  Row entries are stored as the reference stores them, Int<8>,
// 64 bytes: one BLAKE3 block per leaf, the same compression count as the one-limb path.
//
// phi (the FieldMap), as oracle/zip_oracle.c orc_field_from_int restates it: over W = max(value limbs, FL) words
//   Int<2> witness:  W = FL, so a modulus whose top bit is set is read as the NEGATIVE Int<FL> 2^(64 FL) - q inside `%=`:
//                    |w| is reduced modulo m = 2^(64 FL) - q whenever m <= |w| (m up to 2^127 bites), then mapped;
//                    otherwise |w| mod q (a real reduction for FL = 2 and q < 2^127), Montgomery form, sign last.
//   Int<8> entry:    W = 8 > FL, the modulus is never negative there: |v| mod q of a 512-bit magnitude, sign last.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake3.cuh"
#include "kernels_commit.cuh"
#include "kernels_open.cuh"
#include "kernels_verify.cuh"

namespace zipk {

constexpr int kTlLane = 3;    // 64-bit limbs of a scan lane (192 bits >= 128 + 2 log2 cw + 1)
constexpr int kTlAcc = 5;     // limbs of the integer row combination: 256-bit products, up to 2^32 rows
constexpr int kTlVerAcc = 11; // limbs of the verifier's column sum: 128 x 512-bit products, up to 2^32 rows

// out (M limbs) = the N-limb two's-complement x, sign-extended
template <int N, int M>
__device__ __forceinline__ void sign_extend(const uint64_t (&x)[N], uint64_t (&out)[M]) {
    static_assert(M >= N, "sign_extend widens");
    const uint64_t s = (uint64_t)((int64_t)x[N - 1] >> 63);
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = x[i];
#pragma unroll
    for (int i = N; i < M; i++) out[i] = s;
}

// ---------------------------------------------------------------------------------------
// phi for the two widths
// ---------------------------------------------------------------------------------------
// |w| mod m for m <= |w| < 2^128, m < 2^127 (only then can m <= |w| hold: |w| <= 2^127 and m is odd): shift-subtract
__device__ __forceinline__ u128 tl_mod128(u128 x, u128 m) {
    u128 r = 0;
    for (int b = 0; b < 128; b++) {
        r = (r << 1) | (x >> 127);
        x <<= 1;
        if (r >= m) r -= m;
    }
    return r;
}

template <int FL>
__device__ __forceinline__ void tl_negate_mod(uint64_t (&x)[FL], const FieldDev<FL> &f) {
    bool zero = true;
#pragma unroll
    for (int i = 0; i < FL; i++) zero &= x[i] == 0;
    if (!zero) {
        uint64_t q[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) q[i] = f.modulus[i];
        sub_n<FL>(q, x);
#pragma unroll
        for (int i = 0; i < FL; i++) x[i] = q[i];
    }
}

// qm: 2^(64 FL) - q when the modulus has its top bit set and that value is below 2^128, else 0 (no reduction can bite)
template <int FL>
__device__ __forceinline__ void field_from_int128(uint64_t lo, uint64_t hi, const FieldDev<FL> &f, u128 qm, uint64_t (&out)[FL]) {
    const bool neg = (int64_t)hi < 0;
    u128 mag = ((u128)hi << 64) | lo;
    if (neg) mag = (u128)0 - mag;
    if (qm != 0 && mag >= qm) mag = tl_mod128(mag, qm);
    uint64_t a[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) a[i] = i == 0 ? (uint64_t)mag : i == 1 ? (uint64_t)(mag >> 64) : 0;
    // a < 2^128 <= R and r2 < q: the product is below q R, REDC returns a R mod q, canonical -- the reduction of |w|
    // modulo a q below 2^128 included
    mont_mul<FL>(a, f.r2, f, out);
    if (neg) tl_negate_mod<FL>(out, f);
}

// R^(i+2) mod q for chunk i of FL limbs of a 512-bit magnitude (host: tl_phi8_consts)
template <int FL>
struct Phi8Consts {
    static constexpr int N = (8 + FL - 1) / FL;
    uint64_t p[N][FL];
};

template <int FL>
__device__ __forceinline__ void field_from_int512(const uint64_t (&v)[8], const FieldDev<FL> &f, const Phi8Consts<FL> &pc,
                                                  uint64_t (&out)[FL]) {
    const bool neg = (int64_t)v[7] < 0;
    uint64_t mag[Phi8Consts<FL>::N * FL];  // |v|, zero-padded to whole chunks (FL = 3: nine limbs)
    {
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u128 t = (u128)0 - v[i] - borrow;
            mag[i] = neg ? (uint64_t)t : v[i];
            borrow = (uint64_t)(t >> 64) & 1;
        }
#pragma unroll
        for (int i = 8; i < Phi8Consts<FL>::N * FL; i++) mag[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < FL; i++) out[i] = 0;
#pragma unroll
    for (int c = 0; c < Phi8Consts<FL>::N; c++) {
        uint64_t chunk[FL], p[FL], t[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) {
            chunk[i] = mag[c * FL + i];
            p[i] = pc.p[c][i];
        }
        mont_mul<FL>(chunk, p, f, t);  // chunk * 2^(64 FL c) * R mod q
        fe_add<FL>(out, t, f);
    }
    if (neg) tl_negate_mod<FL>(out, f);
}

// ---------------------------------------------------------------------------------------
// Commit: both permute-and-accumulate passes of a row by ONE workgroup, rows strided over the grid.
// Each thread owns ceil(cw / 256) consecutive codeword positions: it sums them, the 256 sums are scanned (wave
// shuffles, then one LDS step over the four wave totals), and it walks its positions again from its exclusive prefix.
// Pass 1 writes t1 to the workgroup's own scratch row in global memory (cw * 24 bytes, only ever read by the workgroup
// that wrote it, behind a barrier; the rows of all workgroups of the launch together are sized by the host to stay
// inside the Infinity Cache; a thread's stores are 24-byte pieces of its own run, not coalesced across the wave),
// pass 2 gathers it through perm2, writes the Int<8> entry and, when HASH, its leaf hash to level 0 of the row's tree.
// ---------------------------------------------------------------------------------------
struct TlEncodeArgs {
    const uint64_t *evals;   // [num_rows][row_len][2]
    const uint32_t *perm1, *perm2;
    uint64_t *t1;            // [gridDim.x][cw][3]
    uint64_t *rows;          // [num_rows][cw][8]
    uint32_t *layers;        // [num_rows][2 cw][8], level 0 written here (HASH)
    uint32_t num_rows, row_len, cw;
};

template <bool HASH>
__global__ void __launch_bounds__(256) tl_encode_rows_kernel(TlEncodeArgs a) {
    __shared__ uint64_t wave_tot[4][kTlLane];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (a.cw + 255u) / 256u;
    const uint32_t j0 = min(tid * per, a.cw), j1 = min(j0 + per, a.cw);
    uint64_t *t1 = a.t1 + (size_t)blockIdx.x * a.cw * kTlLane;
    for (uint32_t row = blockIdx.x; row < a.num_rows; row += gridDim.x) {
        const uint64_t *w = a.evals + (size_t)row * a.row_len * 2;
        for (int pass = 0; pass < 2; pass++) {
            auto fetch = [&](uint32_t j, uint64_t (&x)[kTlLane]) {
                if (pass == 0) {
                    const uint64_t *p = w + (size_t)(a.perm1[j] & (a.row_len - 1u)) * 2;
                    x[0] = p[0];
                    x[1] = p[1];
                    x[2] = (uint64_t)((int64_t)x[1] >> 63);
                } else {
                    const uint64_t *p = t1 + (size_t)a.perm2[j] * kTlLane;
#pragma unroll
                    for (int i = 0; i < kTlLane; i++) x[i] = p[i];
                }
            };
            uint64_t sum[kTlLane] = {0, 0, 0};
            for (uint32_t j = j0; j < j1; j++) {
                uint64_t x[kTlLane];
                fetch(j, x);
                add_n<kTlLane>(sum, x);
            }
            // inclusive scan of the thread sums inside the wave
            uint64_t inc[kTlLane] = {sum[0], sum[1], sum[2]};
            for (uint32_t off = 1; off < 64; off <<= 1) {
                uint64_t y[kTlLane];
#pragma unroll
                for (int i = 0; i < kTlLane; i++) y[i] = __shfl_up(inc[i], off);
                if (lane >= off) add_n<kTlLane>(inc, y);
            }
            if (lane == 63) {
#pragma unroll
                for (int i = 0; i < kTlLane; i++) wave_tot[wave][i] = inc[i];
            }
            __syncthreads();
            // exclusive prefix of this thread: the waves before its own, then the lanes before it
            uint64_t run[kTlLane];
#pragma unroll
            for (int i = 0; i < kTlLane; i++) run[i] = __shfl_up(inc[i], 1u);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < kTlLane; i++) run[i] = 0;
            }
            for (uint32_t k = 0; k < wave; k++) {
                uint64_t y[kTlLane];
#pragma unroll
                for (int i = 0; i < kTlLane; i++) y[i] = wave_tot[k][i];
                add_n<kTlLane>(run, y);
            }
            for (uint32_t j = j0; j < j1; j++) {
                uint64_t x[kTlLane];
                fetch(j, x);
                add_n<kTlLane>(run, x);
                if (pass == 0) {
#pragma unroll
                    for (int i = 0; i < kTlLane; i++) t1[(size_t)j * kTlLane + i] = run[i];
                } else {
                    uint64_t v[8];
                    sign_extend<kTlLane, 8>(run, v);
                    uint64_t *dst = a.rows + ((size_t)row * a.cw + j) * 8;
#pragma unroll
                    for (int i = 0; i < 8; i++) dst[i] = v[i];
                    if constexpr (HASH) {
                        uint32_t h[8];
                        blake3_leaf_limbs<8>(v, h);
                        store_hash(a.layers + ((size_t)row * 2u * a.cw + j) * 8, h);
                    }
                }
            }
            // pass 0: t1 is complete before anybody gathers from it; pass 1: everybody has finished reading t1 (and
            // wave_tot) before the next row overwrites them
            __threadfence_block();
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------
// Row combinations, one pass over the witness for both:
//   u'[c]  = sum_r coeffs[r] * w[r][c]       signed 128 x 128-bit products in a 320-bit accumulator
//   row[c] = sum_r q0[r] (x) phi(w[r][c])    Montgomery products, modular sums
// Block = 64 columns x 4 row lanes; grid.y = row blocks: thread (cx, ry) of block (bx, by) takes column 64 bx + cx and
// rows 4 by + ry, 4 (by + gridDim.y) + ry, ...  The four row lanes are folded through LDS, the row blocks by
// tl_combine_finalize_kernel.
// ---------------------------------------------------------------------------------------
struct TlCombineArgs {
    const uint64_t *evals;   // [num_rows][row_len][2]
    const uint64_t *coeffs;  // [num_rows][2] (device), DO_INT
    const uint64_t *q0;      // [num_rows][FL] Montgomery (device), DO_FIELD
    uint32_t num_rows, row_len;
    uint64_t qm_lo, qm_hi;   // field_from_int128's qm
    uint64_t *part_int;      // [gridDim.y][row_len][kTlAcc]
    uint64_t *part_f;        // [gridDim.y][row_len][FL]
};

// acc += c * w, both 128-bit two's complement, acc kTlAcc limbs
__device__ __forceinline__ void tl_mac_128x128(uint64_t (&acc)[kTlAcc], uint64_t c0, uint64_t c1, uint64_t w0, uint64_t w1) {
    uint64_t t[kTlAcc];
    {
        const u128 p00 = (u128)c0 * w0, p01 = (u128)c0 * w1, p10 = (u128)c1 * w0, p11 = (u128)c1 * w1;
        t[0] = (uint64_t)p00;
        u128 s = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
        t[1] = (uint64_t)s;
        s = (s >> 64) + (p01 >> 64) + (p10 >> 64) + (uint64_t)p11;
        t[2] = (uint64_t)s;
        t[3] = (uint64_t)((s >> 64) + (p11 >> 64));
    }
    // c = c_u - 2^128 [c < 0], w = w_u - 2^128 [w < 0]: the signed product modulo 2^256
    if ((int64_t)c1 < 0) {
        const u128 d = (u128)t[2] - w0;
        t[2] = (uint64_t)d;
        t[3] = t[3] - w1 - ((uint64_t)(d >> 64) & 1);
    }
    if ((int64_t)w1 < 0) {
        const u128 d = (u128)t[2] - c0;
        t[2] = (uint64_t)d;
        t[3] = t[3] - c1 - ((uint64_t)(d >> 64) & 1);
    }
    t[4] = (uint64_t)((int64_t)t[3] >> 63);  // |c w| <= 2^254: the 256-bit value is the product
    add_n<kTlAcc>(acc, t);
}

template <int FL, bool DO_INT, bool DO_FIELD>
__global__ void __launch_bounds__(256) tl_combine_kernel(TlCombineArgs a, FieldDev<FL> f) {
    constexpr int S = kTlAcc + FL;
    __shared__ uint64_t red[3][64][S];
    const uint32_t cx = threadIdx.x & 63u, ry = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 64u + cx;
    const u128 qm = ((u128)a.qm_hi << 64) | a.qm_lo;
    uint64_t ai[kTlAcc], af[FL];
#pragma unroll
    for (int i = 0; i < kTlAcc; i++) ai[i] = 0;
#pragma unroll
    for (int i = 0; i < FL; i++) af[i] = 0;
    if (c < a.row_len) {
        for (uint32_t r = blockIdx.y * 4u + ry; r < a.num_rows; r += gridDim.y * 4u) {
            const uint64_t *p = a.evals + ((size_t)r * a.row_len + c) * 2;
            const uint64_t w0 = p[0], w1 = p[1];
            if constexpr (DO_INT) tl_mac_128x128(ai, a.coeffs[2 * (size_t)r], a.coeffs[2 * (size_t)r + 1], w0, w1);
            if constexpr (DO_FIELD) {
                uint64_t e[FL], q[FL], t[FL];
                field_from_int128<FL>(w0, w1, f, qm, e);
                fe_load<FL>(q, a.q0 + (size_t)r * FL);
                mont_mul<FL>(q, e, f, t);
                fe_add<FL>(af, t, f);
            }
        }
    }
    if (ry) {
#pragma unroll
        for (int i = 0; i < kTlAcc; i++) red[ry - 1][cx][i] = ai[i];
#pragma unroll
        for (int i = 0; i < FL; i++) red[ry - 1][cx][kTlAcc + i] = af[i];
    }
    __syncthreads();
    if (ry == 0 && c < a.row_len) {
        for (int k = 0; k < 3; k++) {
            uint64_t y[kTlAcc], q[FL];
#pragma unroll
            for (int i = 0; i < kTlAcc; i++) y[i] = red[k][cx][i];
#pragma unroll
            for (int i = 0; i < FL; i++) q[i] = red[k][cx][kTlAcc + i];
            if constexpr (DO_INT) add_n<kTlAcc>(ai, y);
            if constexpr (DO_FIELD) fe_add<FL>(af, q, f);
        }
        const size_t slot = (size_t)blockIdx.y * a.row_len + c;
        if constexpr (DO_INT) {
#pragma unroll
            for (int i = 0; i < kTlAcc; i++) a.part_int[slot * kTlAcc + i] = ai[i];
        }
        if constexpr (DO_FIELD) fe_store<FL>(a.part_f + slot * FL, af);
    }
}

// One thread per column: folds the row blocks; u' leaves as Int<16> (sign-extended), the evaluation row as Montgomery
// limbs (row_limbs) and / or as the stream's big-endian bytes (row_be).  Any output may be null.
template <int FL>
__global__ void __launch_bounds__(256) tl_combine_finalize_kernel(const uint64_t *part_int, const uint64_t *part_f, uint32_t blocks,
                                                                  uint32_t row_len, uint64_t *uprime, uint64_t *row_limbs,
                                                                  uint8_t *row_be, FieldDev<FL> f) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= row_len) return;
    if (uprime) {
        uint64_t s[kTlAcc];
#pragma unroll
        for (int i = 0; i < kTlAcc; i++) s[i] = 0;
        for (uint32_t b = 0; b < blocks; b++) {
            uint64_t y[kTlAcc];
            fe_load<kTlAcc>(y, part_int + ((size_t)b * row_len + c) * kTlAcc);
            add_n<kTlAcc>(s, y);
        }
        uint64_t u[16];
        sign_extend<kTlAcc, 16>(s, u);
        fe_store<16>(uprime + (size_t)c * 16, u);
    }
    if (row_limbs || row_be) {
        uint64_t p[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) p[i] = 0;
        for (uint32_t b = 0; b < blocks; b++) {
            uint64_t q[FL];
            fe_load<FL>(q, part_f + ((size_t)b * row_len + c) * FL);
            fe_add<FL>(p, q, f);
        }
        if (row_limbs) fe_store<FL>(row_limbs + (size_t)c * FL, p);
        if (row_be) {  // write_field_element: big-endian bytes of the Montgomery value (the stream is 8-byte aligned)
            uint64_t *dst = reinterpret_cast<uint64_t *>(row_be + (size_t)c * 8 * FL);
#pragma unroll
            for (int i = 0; i < FL; i++) dst[i] = __builtin_bswap64(p[FL - 1 - i]);
        }
    }
}

// ---------------------------------------------------------------------------------------
// Column gather, natural layout.  Per opened column: num_rows x 64-byte values, then num_rows records
// { be64(depth), depth x 32-byte siblings }.  One thread per (opening, row, piece): piece l < depth copies the sibling
// of level l, piece depth writes the length prefix, piece depth + 1 copies the value.  Every offset is a multiple of 8.
// ---------------------------------------------------------------------------------------
struct TlOpenColsArgs {
    const uint64_t *rows;    // [num_rows][cw][8]
    const uint32_t *layers;  // [num_rows][2 cw][8]
    const uint32_t *cols;    // [n_cols]
    uint8_t *out;
    uint32_t num_rows, cw, depth, n_cols;
};

__global__ void __launch_bounds__(256) tl_open_columns_kernel(TlOpenColsArgs a) {
    const uint32_t pieces = a.depth + 2u;
    const uint64_t total = (uint64_t)a.n_cols * a.num_rows * pieces;
    const uint32_t rec = 8u + 32u * a.depth;
    const size_t col_bytes = (size_t)a.num_rows * (64u + rec);
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = (uint32_t)(g % pieces);
        const uint64_t cr = g / pieces;
        const uint32_t r = (uint32_t)(cr % a.num_rows), ci = (uint32_t)(cr / a.num_rows);
        const uint32_t col = a.cols[ci];
        uint8_t *blk = a.out + (size_t)ci * col_bytes;
        uint64_t *record = reinterpret_cast<uint64_t *>(blk + (size_t)a.num_rows * 64u + (size_t)r * rec);
        if (l < a.depth) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(
                a.layers + ((size_t)r * 2u * a.cw + level_off(a.cw, l) + ((col >> l) ^ 1u)) * 8);
#pragma unroll
            for (int i = 0; i < 4; i++) record[1 + 4 * (size_t)l + i] = src[i];
        } else if (l == a.depth) {
            record[0] = __builtin_bswap64((uint64_t)a.depth);
        } else {
            const uint64_t *src = a.rows + ((size_t)r * a.cw + col) * 8;
            uint64_t *dst = reinterpret_cast<uint64_t *>(blk + (size_t)r * 64u);
#pragma unroll
            for (int i = 0; i < 8; i++) dst[i] = src[i];
        }
    }
}

// ---------------------------------------------------------------------------------------
// Verifier: one workgroup per opening.  Thread t walks rows t, t + 256, ...: hashes the 64-byte entry and its path,
// adds coeffs[r] * v (128 x 512-bit, two's complement in 704 bits) and q0[r] (x) phi_8(v) to its sums; the sums are
// folded through LDS and thread 0 compares them with encode_wide(u') and encode_f(row) at the column
// (flags: bit 0 = over Z, bit 1 = over F_q, as column_flags).
// ---------------------------------------------------------------------------------------
struct TlVerifyColsArgs {
    const uint8_t *wire;     // column section of the proof (device)
    const uint32_t *cols;    // [n_cols]
    const uint64_t *coeffs;  // [num_rows][2] or null (num_rows == 1)
    const uint64_t *q0;      // [num_rows][FL] Montgomery, or null (num_rows == 1)
    const uint32_t *roots;   // [num_rows][8]
    const uint64_t *enc_int; // [cw][16] or null (num_rows == 1)
    const uint64_t *enc_f;   // [cw][FL]
    uint32_t num_rows, depth, n_cols;
    uint32_t *flags, *bad_merkle, *malformed;  // [n_cols] each
};

// acc += c * v: c 128-bit, v 512-bit, both two's complement; acc kTlVerAcc limbs (the value needs 641 bits)
__device__ __forceinline__ void tl_mac_128x512(uint64_t (&acc)[kTlVerAcc], uint64_t c0, uint64_t c1, const uint64_t (&v)[8]) {
    uint64_t t[kTlVerAcc];
#pragma unroll
    for (int i = 0; i < kTlVerAcc; i++) t[i] = 0;
    {
        uint64_t carry = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u128 x = (u128)v[i] * c0 + carry;
            t[i] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        t[8] = carry;
        carry = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u128 x = (u128)v[i] * c1 + t[i + 1] + carry;
            t[i + 1] = (uint64_t)x;
            carry = (uint64_t)(x >> 64);
        }
        t[9] = carry;
    }
    const bool cneg = (int64_t)c1 < 0, vneg = (int64_t)v[7] < 0;
    // (c_u - 2^128 [c < 0]) (v_u - 2^512 [v < 0]) modulo 2^704
    if (vneg) {
        const u128 d0 = (u128)t[8] - c0;
        t[8] = (uint64_t)d0;
        const u128 d1 = (u128)t[9] - c1 - ((uint64_t)(d0 >> 64) & 1);
        t[9] = (uint64_t)d1;
        t[10] -= (uint64_t)(d1 >> 64) & 1;
    }
    if (cneg) {
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u128 d = (u128)t[i + 2] - v[i] - borrow;
            t[i + 2] = (uint64_t)d;
            borrow = (uint64_t)(d >> 64) & 1;
        }
        t[10] -= borrow;
    }
    if (cneg && vneg) t[10] += 1;  // + 2^640
    add_n<kTlVerAcc>(acc, t);
}

// MerkleProof::verify of one record with a 64-byte leaf (check_merkle_record at Int<8>)
__device__ __forceinline__ MerkleRecord tl_check_merkle_record(const uint64_t (&v)[8], const uint64_t *rec, uint32_t depth,
                                                               uint32_t col, const uint32_t *root) {
    if (rec[0] != __builtin_bswap64((uint64_t)depth)) return kMerkleMalformed;
    uint32_t cur[8];
    blake3_leaf_limbs<8>(v, cur);
    uint32_t index = col;
    for (uint32_t l = 0; l < depth; l++) {
        uint32_t sib[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t w = rec[1 + 4 * l + i];
            sib[2 * i] = (uint32_t)w;
            sib[2 * i + 1] = (uint32_t)(w >> 32);
        }
        uint32_t m[16], h[8];
        const bool right = index & 1u;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            m[i] = right ? sib[i] : cur[i];
            m[8 + i] = right ? cur[i] : sib[i];
        }
        blake3_block64(m, h);
#pragma unroll
        for (int i = 0; i < 8; i++) cur[i] = h[i];
        index >>= 1;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; i++) ok &= cur[i] == root[i];
    return ok ? kMerkleOk : kMerkleBadPath;
}

template <int FL>
__global__ void __launch_bounds__(256) tl_verify_columns_kernel(TlVerifyColsArgs a, FieldDev<FL> f, Phi8Consts<FL> pc) {
    constexpr int S = kTlVerAcc + FL;
    __shared__ uint64_t red[256 * S];
    __shared__ uint32_t counts[2];
    const uint32_t ci = blockIdx.x, tid = threadIdx.x;
    const uint32_t rec_bytes = 8u + 32u * a.depth;
    const size_t col_bytes = (size_t)a.num_rows * (64u + rec_bytes);
    const uint8_t *base = a.wire + (size_t)ci * col_bytes;
    const uint32_t col = a.cols[ci];
    if (tid < 2) counts[tid] = 0;
    __syncthreads();
    uint64_t si[kTlVerAcc], sf[FL];
#pragma unroll
    for (int i = 0; i < kTlVerAcc; i++) si[i] = 0;
#pragma unroll
    for (int i = 0; i < FL; i++) sf[i] = 0;
    for (uint32_t r = tid; r < a.num_rows; r += 256u) {
        uint64_t v[8];
        fe_load<8>(v, reinterpret_cast<const uint64_t *>(base + (size_t)r * 64u));
        if (a.coeffs) tl_mac_128x512(si, a.coeffs[2 * (size_t)r], a.coeffs[2 * (size_t)r + 1], v);
        uint64_t e[FL], t[FL];
        field_from_int512<FL>(v, f, pc, e);
        if (a.q0) {
            uint64_t q[FL];
            fe_load<FL>(q, a.q0 + (size_t)r * FL);
            mont_mul<FL>(q, e, f, t);
        } else {
            fe_store<FL>(t, e);
        }
        fe_add<FL>(sf, t, f);
        const uint64_t *rec = reinterpret_cast<const uint64_t *>(base + (size_t)a.num_rows * 64u + (size_t)r * rec_bytes);
        const MerkleRecord m = tl_check_merkle_record(v, rec, a.depth, col, a.roots + (size_t)r * 8);
        if (m == kMerkleMalformed) atomicAdd(&counts[1], 1u);
        if (m == kMerkleBadPath) atomicAdd(&counts[0], 1u);
    }
    fe_store<kTlVerAcc>(red + tid * S, si);
    fe_store<FL>(red + tid * S + kTlVerAcc, sf);
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            uint64_t x[kTlVerAcc], y[kTlVerAcc], p[FL], q[FL];
            fe_load<kTlVerAcc>(x, red + tid * S);
            fe_load<kTlVerAcc>(y, red + (tid + s) * S);
            fe_load<FL>(p, red + tid * S + kTlVerAcc);
            fe_load<FL>(q, red + (tid + s) * S + kTlVerAcc);
            add_n<kTlVerAcc>(x, y);
            fe_add<FL>(p, q, f);
            fe_store<kTlVerAcc>(red + tid * S, x);
            fe_store<FL>(red + tid * S + kTlVerAcc, p);
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t fl = 0;
        if (a.enc_int) {
            uint64_t sum[kTlVerAcc], wide[16];
            fe_load<kTlVerAcc>(sum, red);
            sign_extend<kTlVerAcc, 16>(sum, wide);
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (a.enc_int[(size_t)col * 16 + i] != wide[i]) fl |= 1u;
        }
        for (uint32_t i = 0; i < (uint32_t)FL; i++)
            if (a.enc_f[(size_t)col * FL + i] != red[kTlVerAcc + i]) fl |= 2u;
        a.flags[ci] = fl;
        a.bad_merkle[ci] = counts[0];
        a.malformed[ci] = counts[1];
    }
}

// ---------------------------------------------------------------------------------------
// Diagnostic (zip_field_map_int): phi of arbitrary Int<2> / Int<8> values, checked against the oracle in tests.
// ---------------------------------------------------------------------------------------
template <int FL>
__global__ void __launch_bounds__(256) tl_field_map_int2_kernel(const uint64_t *vals, uint32_t n, uint64_t *out, FieldDev<FL> f,
                                                                uint64_t qm_lo, uint64_t qm_hi) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t e[FL];
    field_from_int128<FL>(vals[2 * (size_t)i], vals[2 * (size_t)i + 1], f, ((u128)qm_hi << 64) | qm_lo, e);
    fe_store<FL>(out + (size_t)i * FL, e);
}

template <int FL>
__global__ void __launch_bounds__(256) tl_field_map_int8_kernel(const uint64_t *vals, uint32_t n, uint64_t *out, FieldDev<FL> f,
                                                                Phi8Consts<FL> pc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t v[8], e[FL];
    fe_load<8>(v, vals + (size_t)i * 8);
    field_from_int512<FL>(v, f, pc, e);
    fe_store<FL>(out + (size_t)i * FL, e);
}

}  // namespace zipk
