// The field loops of SpartanProver::prove (kernels_spartan.cuh) for MANY small proofs of ONE circuit, each proof with its
// own field and its own z (zip_ccs_batch): every kernel takes the instance from blockIdx.y or blockIdx.z, so the number
// of launches of a call does not depend on the number of proofs.
//
//   ccs_batch_map_z_kernel    z_f[i] = phi_i(z_i[j]), zero beyond z_len[i]            prover.rs:230-236
//   ccs_batch_spmv_kernel     M_k z_i for every (row, matrix, instance)               zinc/utils.rs:121-135
//   ccs_batch_eq_kernel       build_eq_x_r from two half tables built in LDS          sumcheck/utils.rs:102-177
//   ccs_batch_second_kernel   sum_k gamma_i^k * compute_eval_table_sparse(M_k, eq)    sparse_matrix.rs:165-182 + prover.rs:279-290
//   ccs_batch_vs_kernel       V_s[k] = <M_k z_i, eq(r_x)>, one workgroup each         prover.rs:330-347
//   ccs_batch_eval_matrices_kernel  the verifier's V_xy[k] = mle[M_k](r_x_i, r_y_i)   verifier.rs (zip_ccs_eval_matrices)
//
// The matrices are held ONCE, as the int64 values the caller gave (CSR, and the CSC form csc_fill_kernel<1> makes of
// them): a kernel maps a value into the instance's field where it uses it (field_from_i64 with the instance's FieldDev
// and quirk_mod), so no copy of the matrices depends on a field.  The per-instance arguments are one device array; an
// instance's entry sits at a wave-uniform address, so its field constants and pointers are read through the scalar
// cache.  Exact arithmetic on canonical residues throughout: summation order is free, the bits are the reference's.
// No kernel waits on another workgroup, no atomics, every loop's trip count is fixed at launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_spartan.cuh"

namespace zipk {

template <int FL>
struct CcsBatchInst {
    FieldDev<FL> f;
    uint64_t quirk_mod;
    const int64_t *z;  // z_len entries
    uint64_t z_len;
    uint64_t *z_f, *mz[kCcsMaxMatrices], *eq[2], *second;  // tables of m elements
};

struct CcsBatchMats {
    const uint32_t *row_ptr[kCcsMaxMatrices], *col_idx[kCcsMaxMatrices];  // CSR
    const int64_t *vals[kCcsMaxMatrices];
    const uint32_t *col_ptr[kCcsMaxMatrices], *row_idx[kCcsMaxMatrices];  // CSC
    const int64_t *vals_t[kCcsMaxMatrices];
    uint32_t n_rows[kCcsMaxMatrices];
    uint32_t t, m;
};

// grid (ceil(m / 256), n)
template <int FL>
__global__ void __launch_bounds__(256) ccs_batch_map_z_kernel(const CcsBatchInst<FL> *__restrict__ inst, uint32_t m) {
    const CcsBatchInst<FL> &a = inst[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint64_t e[FL];
    if (i < a.z_len) {
        field_from_i64<FL>(a.z[i], a.f, a.quirk_mod, e);
    } else {
#pragma unroll
        for (int k = 0; k < FL; k++) e[k] = 0;
    }
    fe_store<FL>(a.z_f + (size_t)i * FL, e);
}

// grid (ceil(m / 256), t, n): mz[k][row] = sum_e phi(vals[k][e]) (x) z_f[col[e]]  (row < n_rows[k]), 0 up to m
template <int FL>
__global__ void __launch_bounds__(256) ccs_batch_spmv_kernel(CcsBatchMats M, const CcsBatchInst<FL> *__restrict__ inst) {
    const CcsBatchInst<FL> &a = inst[blockIdx.z];
    const uint32_t k = blockIdx.y, row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M.m) return;
    const FieldDev<FL> f = a.f;
    const uint64_t quirk_mod = a.quirk_mod;
    const uint64_t *z_f = a.z_f;
    uint64_t acc[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) acc[i] = 0;
    if (row < M.n_rows[k]) {
        const uint32_t *col_idx = M.col_idx[k];
        const int64_t *vals = M.vals[k];
        for (uint32_t e = M.row_ptr[k][row]; e < M.row_ptr[k][row + 1]; e++) {
            uint64_t v[FL], x[FL], t[FL];
            field_from_i64<FL>(vals[e], f, quirk_mod, v);
            fe_load<FL>(x, z_f + (size_t)col_idx[e] * FL);
            mont_mul<FL>(x, v, f, t);
            fe_add<FL>(acc, t, f);
        }
    }
    fe_store<FL>(a.mz[k] + (size_t)row * FL, acc);
}

constexpr uint32_t kCcsBatchMaxVars = 16;
constexpr uint32_t kCcsBatchEqPerBlock = 4096;  // entries of eq a workgroup writes: 16 per thread beside the <= 2 half-table entries it builds

// grid (ceil(2^s / kCcsBatchEqPerBlock), n): eq(x, r_i) into slot `slot` of instance i, r = n * s Montgomery elements.
// eq(x, r) = eq(x_lo, r_lo) (x) eq(x_hi, r_hi) over the low s/2 and the remaining variables: at s <= 16 both half tables
// are at most 256 entries, every workgroup builds them in LDS (up to 8 multiplications for each of its <= 2 entries per
// thread) and then writes its entries of the table with one multiplication each.
template <int FL>
__global__ void __launch_bounds__(256) ccs_batch_eq_kernel(const CcsBatchInst<FL> *__restrict__ inst, const uint64_t *__restrict__ r,
                                                           uint32_t s, uint32_t slot) {
    __shared__ uint64_t fac[2][kCcsBatchMaxVars][FL];                     // [bit][j]
    __shared__ uint64_t half[(2u << (kCcsBatchMaxVars / 2)) * FL];        // lo table, then hi table
    const CcsBatchInst<FL> &a = inst[blockIdx.y];
    const FieldDev<FL> f = a.f;
    const uint32_t tid = threadIdx.x;
    uint64_t one[FL];
    {
        uint64_t unit[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) unit[i] = 0;
        unit[0] = 1;
        mont_mul<FL>(unit, f.r2, f, one);  // R mod q
    }
    if (tid < s) {
        uint64_t rj[FL], c[FL];
        fe_load<FL>(rj, r + ((size_t)blockIdx.y * s + tid) * FL);
#pragma unroll
        for (int i = 0; i < FL; i++) c[i] = one[i];
        fe_sub<FL>(c, rj, f);
#pragma unroll
        for (int i = 0; i < FL; i++) { fac[0][tid][i] = c[i]; fac[1][tid][i] = rj[i]; }
    }
    __syncthreads();
    const uint32_t nv_lo = s / 2, nv_hi = s - nv_lo, n_lo = 1u << nv_lo, n_hi = 1u << nv_hi;
    for (uint32_t h = tid; h < n_lo + n_hi; h += blockDim.x) {
        const bool hi = h >= n_lo;
        const uint32_t idx = hi ? h - n_lo : h, first = hi ? nv_lo : 0, nv = hi ? nv_hi : nv_lo;
        uint64_t acc[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) acc[i] = one[i];
        for (uint32_t j = 0; j < nv; j++) {
            uint64_t x[FL], t[FL];
            fe_load<FL>(x, fac[(idx >> j) & 1][first + j]);
            mont_mul<FL>(acc, x, f, t);
#pragma unroll
            for (int i = 0; i < FL; i++) acc[i] = t[i];
        }
        fe_store<FL>(half + (size_t)h * FL, acc);
    }
    __syncthreads();
    const uint32_t m = 1u << s;
    uint64_t *out = a.eq[slot];
    for (uint32_t p = 0; p < kCcsBatchEqPerBlock; p += blockDim.x) {
        const uint32_t i = blockIdx.x * kCcsBatchEqPerBlock + p + tid;
        if (i < m) {
            uint64_t x[FL], y[FL], t[FL];
            fe_load<FL>(x, half + (size_t)(i & (n_lo - 1)) * FL);
            fe_load<FL>(y, half + (size_t)(n_lo + (i >> nv_lo)) * FL);
            mont_mul<FL>(x, y, f, t);
            fe_store<FL>(out + (size_t)i * FL, t);
        }
    }
}

// grid (ceil(m / 256), n): second[col] = sum_k gamma^k * sum_{rows of column col} eq1[row] (x) phi(M_k[row][col]), folded as
// second_table_kernel does (highest k first: lin = lin * gamma + table_k[col]); gamma = n Montgomery elements.
template <int FL>
__global__ void __launch_bounds__(256) ccs_batch_second_kernel(CcsBatchMats M, const CcsBatchInst<FL> *__restrict__ inst,
                                                               const uint64_t *__restrict__ gamma_d) {
    const CcsBatchInst<FL> &a = inst[blockIdx.y];
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= M.m) return;
    const FieldDev<FL> f = a.f;
    const uint64_t quirk_mod = a.quirk_mod;
    const uint64_t *eq = a.eq[1];
    uint64_t gamma[FL], lin[FL];
    fe_load<FL>(gamma, gamma_d + (size_t)blockIdx.y * FL);
#pragma unroll
    for (int i = 0; i < FL; i++) lin[i] = 0;
    for (int k = (int)M.t - 1; k >= 0; k--) {
        const uint32_t *row_idx = M.row_idx[k];
        const int64_t *vals_t = M.vals_t[k];
        uint64_t acc[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) acc[i] = 0;
        for (uint32_t e = M.col_ptr[k][col]; e < M.col_ptr[k][col + 1]; e++) {
            uint64_t v[FL], x[FL], t[FL];
            field_from_i64<FL>(vals_t[e], f, quirk_mod, v);
            fe_load<FL>(x, eq + (size_t)row_idx[e] * FL);
            mont_mul<FL>(x, v, f, t);
            fe_add<FL>(acc, t, f);
        }
        uint64_t t[FL];
        mont_mul<FL>(lin, gamma, f, t);
        fe_add<FL>(t, acc, f);
#pragma unroll
        for (int i = 0; i < FL; i++) lin[i] = t[i];
    }
    fe_store<FL>(a.second + (size_t)col * FL, lin);
}

constexpr uint32_t kCcsBatchVsThreads = 512;

// grid (t, n): vs[(i * t + k)] = <mz[k], eq1> of instance i -- one workgroup walks the m entries, folds its threads'
// sums in LDS down to the element and writes it.
template <int FL>
__global__ void __launch_bounds__(kCcsBatchVsThreads) ccs_batch_vs_kernel(const CcsBatchInst<FL> *__restrict__ inst, uint32_t m,
                                                                          uint64_t *__restrict__ vs) {
    __shared__ uint64_t red[kCcsBatchVsThreads * FL];
    const CcsBatchInst<FL> &a = inst[blockIdx.y];
    const FieldDev<FL> f = a.f;
    const uint32_t tid = threadIdx.x, k = blockIdx.x;
    const uint64_t *mz = a.mz[k], *eq = a.eq[1];
    uint64_t acc[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) acc[i] = 0;
    for (uint32_t i = tid; i < m; i += kCcsBatchVsThreads) {
        uint64_t x[FL], y[FL], t[FL];
        fe_load<FL>(x, mz + (size_t)i * FL);
        fe_load<FL>(y, eq + (size_t)i * FL);
        mont_mul<FL>(x, y, f, t);
        fe_add<FL>(acc, t, f);
    }
    fe_store<FL>(red + (size_t)tid * FL, acc);
    __syncthreads();
    for (uint32_t w = kCcsBatchVsThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            uint64_t p[FL], q[FL];
            fe_load<FL>(p, red + (size_t)tid * FL);
            fe_load<FL>(q, red + (size_t)(tid + w) * FL);
            fe_add<FL>(p, q, f);
            fe_store<FL>(red + (size_t)tid * FL, p);
        }
        __syncthreads();
    }
    if (tid < FL) vs[((size_t)blockIdx.y * gridDim.x + k) * FL + tid] = red[tid];
}

// grid (t, n): out[(i * t + k)] = mle[M_k](r_x_i, r_y_i) = sum_rows eq0[row] (x) sum_e phi_i(vals[k][e]) (x) eq1[col[e]], the
// verifier's V_xy (zinc/verifier.rs: evaluate the matrices' MLEs at the two sumcheck points; matrix_eval_partials_kernel
// for one field).  eq slot 0 holds eq(r_x_i), slot 1 eq(r_y_i).  One workgroup walks the n_rows[k] rows of the integer CSR,
// a thread per row, and folds its threads' sums in LDS as ccs_batch_vs_kernel does; field additions commute, so the
// value does not depend on the order.
template <int FL>
__global__ void __launch_bounds__(kCcsBatchVsThreads) ccs_batch_eval_matrices_kernel(CcsBatchMats M,
                                                                                     const CcsBatchInst<FL> *__restrict__ inst,
                                                                                     uint64_t *__restrict__ out) {
    __shared__ uint64_t red[kCcsBatchVsThreads * FL];
    const CcsBatchInst<FL> &a = inst[blockIdx.y];
    const FieldDev<FL> f = a.f;
    const uint64_t quirk_mod = a.quirk_mod;
    const uint32_t tid = threadIdx.x, k = blockIdx.x;
    const uint64_t *eq_x = a.eq[0], *eq_y = a.eq[1];
    const uint32_t *row_ptr = M.row_ptr[k], *col_idx = M.col_idx[k];
    const int64_t *vals = M.vals[k];
    const uint32_t n_rows = M.n_rows[k] < M.m ? M.n_rows[k] : M.m;
    uint64_t acc[FL];
#pragma unroll
    for (int i = 0; i < FL; i++) acc[i] = 0;
    for (uint32_t row = tid; row < n_rows; row += kCcsBatchVsThreads) {
        uint64_t in[FL];
#pragma unroll
        for (int i = 0; i < FL; i++) in[i] = 0;
        for (uint32_t e = row_ptr[row]; e < row_ptr[row + 1]; e++) {
            uint64_t v[FL], y[FL], t[FL];
            field_from_i64<FL>(vals[e], f, quirk_mod, v);
            fe_load<FL>(y, eq_y + (size_t)col_idx[e] * FL);
            mont_mul<FL>(y, v, f, t);
            fe_add<FL>(in, t, f);
        }
        uint64_t x[FL], t[FL];
        fe_load<FL>(x, eq_x + (size_t)row * FL);
        mont_mul<FL>(x, in, f, t);
        fe_add<FL>(acc, t, f);
    }
    fe_store<FL>(red + (size_t)tid * FL, acc);
    __syncthreads();
    for (uint32_t w = kCcsBatchVsThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            uint64_t p[FL], q[FL];
            fe_load<FL>(p, red + (size_t)tid * FL);
            fe_load<FL>(q, red + (size_t)(tid + w) * FL);
            fe_add<FL>(p, q, f);
            fe_store<FL>(red + (size_t)tid * FL, p);
        }
        __syncthreads();
    }
    if (tid < FL) out[((size_t)blockIdx.y * gridDim.x + k) * FL + tid] = red[tid];
}

}  // namespace zipk
