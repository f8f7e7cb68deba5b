/*
 * zip_hip.h -- C ABI of libzip_hip.so: the MI355X (gfx950) implementation of the
 * Zip PCS commit/open hot path of NethermindEth/zinc.
 *
 * This is the drop-in boundary.  A thin Rust shim inside
 *   zinc::zip::pcs::MultilinearZip::{commit, commit_no_merkle, encode_rows, open}
 *   (src/zip/pcs/commit.rs:50,104,158; src/zip/pcs/open_z.rs:22)
 * binds these symbols (see INTEGRATION.md for the `extern "C"` block) and keeps
 * ZincProver / ZincVerifier unchanged.  Everything that is sequential and tiny
 * stays on the host side of the boundary: the Keccak Fiat-Shamir transcript
 * (src/transcript.rs), the rand-based permutation expansion
 * (src/zip/utils.rs:139-142), the eq-tensor q_0 (src/zip/pcs/utils.rs:279-292) and
 * the absorption of the evaluation row (src/zip/pcs_transcript.rs:107-113).
 *
 * Conventions
 *  - plain C types only; every call returns int32 (ZIP_OK == 0, negative = error)
 *  - no exceptions / unwinding cross the boundary; zip_strerror() names a code and
 *    zip_ctx_last_error() returns the detailed message of the last failing call
 *  - one zip_ctx per GPU and per geometry.  Several GPUs: either ONE process drives them all through the
 *    multi-device context below -- row shards behind one call, the roots gathered with in-process RCCL --, or one process
 *    per GPU gives every rank its own ctx with a row shard and exchanges roots / partial rows with RCCL above
 *    this ABI (zinc_amd/dist.py)
 *  - all work is enqueued on the ctx's HIP stream; calls that write HOST memory
 *    return after the data has landed, calls that only touch DEVICE memory return
 *    asynchronously (use zip_ctx_synchronize)
 *  - integers are little-endian arrays of 64-bit limbs in two's complement
 *    (src/field/int.rs:23-25); field elements are little-endian limb arrays of the
 *    Montgomery representation (src/field.rs:24-32)
 *  - a pointer argument with a zip_mem_kind may be host or device memory
 */
#ifndef ZIP_HIP_H
#define ZIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZIP_HIP_ABI_VERSION 3 /* 3: zip_ctx_set_speculation, zip_open_shard, zip_mctx_roots, zip_mctx_roots_path */
/* (zip_keccak_state and zip_sumcheck_prove came later and are purely additive: no existing entry point or structure
 * changed, so the version stays 3; a caller that needs them looks the symbol up.  Likewise zip_sumcheck_init taking
 * up to 8 tables instead of 4: a widening, every call that was valid means what it meant.  The batch entry points,
 * zip_batch_commit and the five beside it, are additive in the same way, and so are zip_batch_verify and
 * zip_batch_verify_calls.  So are zip_prime_test_base2, zip_get_prime and zip_prime_launch_counts, and
 * zip_ctx_set_proximity_tests / zip_ctx_proximity_tests: a ctx that never calls the setter behaves as before.  So is
 * zip_sumcheck_init_products, and so is zip_sumcheck_grid_counts.  So are zip_sumcheck_prove_batch and
 * zip_sumcheck_batch_counts: many small sumchecks in one launch, beside the one-at-a-time form that is unchanged.  So are the
 * zip_ccs_batch_* entry points: the Spartan tables of many proofs of one circuit, beside zip_ccs.  So are
 * zip_batch_commit_codes, zip_batch_open_eval_fields, zip_batch_open_fields and zip_batch_codes_counts: a batch whose
 * members have their own code and field, beside the shared-code batch that is unchanged.  So are zip_batch_verify_codes,
 * zip_batch_verify_codes_counts and zip_ccs_batch_eval_matrices: the verifier's side of such a batch.  So is
 * zip_field_map_int, and so is the admission of (n_limbs, k_limbs, m_limbs) = (2, 8, 16) by zip_ctx_create: a triple that
 * was refused is now served, every call on a (1, 4, 8) ctx means what it meant.  So are zip_get_prime_batch and
 * zip_prime_batch_counts: the fields of a whole batch in one launch set, beside zip_get_prime that is unchanged.  So are
 * zip_batch_open_each and zip_batch_open_each_counts: the streams of a batch open delivered one by one, beside
 * zip_batch_open and zip_batch_open_fields that are unchanged.) */

/* status codes */
#define ZIP_OK 0
#define ZIP_ERR_INVALID_PARAM (-1) /* zip::Error::InvalidPcsParam (src/zip/pcs/utils.rs:17-39) and the
                                      RaaCode width assertion (src/zip/code_raa.rs:68-72) */
#define ZIP_ERR_SHAPE (-2)         /* where the reference panics on a shape mismatch (commit.rs:56-63) */
#define ZIP_ERR_HIP (-3)           /* a HIP runtime call failed */
#define ZIP_ERR_NO_DEVICE (-4)     /* no usable gfx950 device: there is NO CPU fallback */
#define ZIP_ERR_UNSUPPORTED (-5)   /* geometry outside what the kernels implement */
#define ZIP_ERR_ALLOC (-6)
#define ZIP_ERR_NULL (-7)

typedef enum { ZIP_MEM_HOST = 0, ZIP_MEM_DEVICE = 1 } zip_mem_kind;

typedef struct zip_ctx zip_ctx;
typedef struct zip_commitment zip_commitment;

/* Geometry of one polynomial size: what RaaCode::new (src/zip/code_raa.rs:35-86) and
 * MultilinearZip::setup (src/zip/pcs/structs.rs:79-91) compute, plus the two
 * permutations that shuffle_seeded(perm_k_seed) applies (out[j] = in[perm[j]]). */
typedef struct {
    uint32_t num_vars;     /* log2(poly_size) */
    uint32_t row_len;      /* next_pow2(isqrt(poly_size))            code_raa.rs:43  */
    uint32_t num_rows;     /* next_pow2(poly_size / row_len)         structs.rs:82   */
    uint32_t codeword_len; /* row_len * rep                          code_raa.rs:113
                            * supported: codeword_len <= 65536 (num_vars <= 30 at rep 2, <= 28 at rep 4);
                            * larger codewords exceed the 96-bit lanes: ZIP_ERR_UNSUPPORTED */
    uint32_t rep;          /* repetition factor (power of two)       code.rs:235-237 */
    uint32_t n_limbs;      /* ZipTypes::N limbs, must be 1 or 2      traits/types.rs:225-240 */
    uint32_t k_limbs;      /* ZipTypes::K limbs, must be 4 (8 with n_limbs 2) */
    uint32_t m_limbs;      /* ZipTypes::M limbs, must be 8 (16 with n_limbs 2); any other triple: ZIP_ERR_UNSUPPORTED */
    const uint32_t *perm1; /* HOST, codeword_len entries, a permutation of [0, codeword_len) */
    const uint32_t *perm2; /* HOST, codeword_len entries */
    int32_t device;        /* HIP device ordinal */
    uint32_t row_begin;    /* first row of this ctx's shard (0 for a whole polynomial) */
    uint32_t row_count;    /* rows in the shard; 0 means num_rows */
} zip_params;

/* Field configuration (src/field/config.rs:30-50).  Only the modulus crosses the
 * boundary; R^2 and -q^-1 mod 2^64 are recomputed (config.rs:174-214). */
typedef struct {
    uint32_t limbs;      /* FIELD_LIMBS: 2, 3 or 4 */
    uint64_t modulus[8]; /* little-endian limbs, odd */
} zip_field;

/* ---- Two-limb witnesses: INT_LIMBS = 2 (src/field/int.rs:276-288: N = Int<2>, K = Int<8>, M = Int<16>) ------------------
 * A ctx created with (n_limbs, k_limbs, m_limbs) = (2, 8, 16) commits, opens and verifies polynomials whose coefficients
 * are 128-bit two's complement: two little-endian u64 limbs per value.  Every `const int64_t *evals` / `coeffs` argument
 * of the calls below then points at 2 limbs per value (n_evals still COUNTS coefficients, ZIP_ERR_SHAPE as before; coeffs
 * are full-range Int<2> challenges, get_integer_challenge(2)), and every size in this header that names k_limbs / m_limbs
 * holds with 8 / 16:
 *   rows        row_count * cw * 8 u64 (zip_commitment_device_ptrs, zip_commit_download, zip_commitment_upload); a leaf is
 *               BLAKE3 of the 64-byte entry (int.rs:201-210), one compression as for Int<4>
 *   u'          row_len * 16 u64 (zip_open_testing; row_len * 128 bytes at the head of the stream when num_rows > 1)
 *   stream      [u' : row_len * 128 B, only if num_rows > 1] [n_cols x (num_rows x 64 B values, num_rows x {be64(depth),
 *               depth x 32 B})] [row_len field elements]: zip_proof_len with k_limbs 8, m_limbs 16
 * Served: zip_commit (with_merkle 0 and 1), zip_commit_hinted and zip_commit_open (same roots and bytes as zip_commit then
 * zip_open; the hint is ignored, such a commit always stores every entry and every tree node, and the ctx never hints
 * itself whatever zip_ctx_set_speculation or ZIP_HIP_SPECULATE say), zip_commitment_device_ptrs / zip_commit_download /
 * zip_commitment_upload, zip_open_testing, zip_open_eval, zip_open_columns, zip_open, zip_mle_eval,
 * zip_commitment_mle_eval, zip_verify (the same verdict order and the same two deliberate deviations), zip_proof_len.
 * Codewords: every power of two up to 65536, the bound of the one-limb ctx (the scan lanes are 192 bits; honest entries
 * need 128 + 2 log2(codeword_len) <= 160).
 * The FieldMap of such a ctx (src/conversion.rs:86-100 over src/field.rs:536-568; zip_field_map_int pins both):
 *   witness, Int<2>   W = FIELD_LIMBS words: for a modulus with its top bit set the signed-modulus reading (see
 *                     zip_open_eval) reduces |w| modulo 2^(64 limbs) - q first, whenever that is <= |w| -- up to 2^127,
 *                     so moduli that no 64-bit witness touches are touched here (q = 2^256 - 2^100 - 1); a two-limb
 *                     modulus below 2^127 is a real reduction of |w|
 *   entries, Int<8>   W = 8 > FIELD_LIMBS in the verifier: |v| mod q of the 512-bit magnitude, then the sign; never the quirk
 * REFUSED with ZIP_ERR_UNSUPPORTED, a zip_ctx_last_error text that says "two-limb", and no launch: row shards
 * (row_begin / row_count in zip_ctx_create, which has no ctx to leave a text in; zip_open_shard; zip_sum_partials),
 * zip_ctx_set_proximity_tests above 1, zip_commit_open_begin, zip_open_stream, zip_batch_commit, zip_batch_commit_codes,
 * zip_batch_verify, zip_batch_verify_codes (the other zip_batch_* calls take a batch, which such a ctx cannot make), and
 * zip_mctx_create with such params.  The ctx stays usable after a refusal. */

int32_t zip_abi_version(void);
const char *zip_strerror(int32_t code);
/* number of visible HIP devices (0 when there is no GPU); never initialises a context */
int32_t zip_device_count(void);
/* zip_sumcheck / zip_ccs handles live for one proof; their device blocks are kept (per device, at most 4 GiB)
 * for the next handle instead of going back to hipFree / hipMalloc.  This returns them to the driver. */
void zip_release_cached_memory(void);
/* Host buffers the caller pins once (a reused proof or witness buffer) are reached by the DMA engines directly:
 * every host transfer of this library first looks whether its buffer is pinned and only otherwise goes through the
 * library's pinned bounce buffers and a host-side copy (~33 GB/s instead of PCIe's ~55).  ZIP_ERR_ALLOC when the
 * range cannot be pinned (locked-memory limit); nothing else changes then. */
int32_t zip_host_register(void *p, size_t bytes);
void zip_host_unregister(void *p);

/* Threading: calls on one ctx (and on its commitments) are serialised inside the library -- they
 * share one pinned staging buffer and one set of streams; distinct contexts run concurrently. */
int32_t zip_ctx_create(const zip_params *params, zip_ctx **out);
void zip_ctx_destroy(zip_ctx *ctx);
const char *zip_ctx_last_error(const zip_ctx *ctx);
int32_t zip_ctx_synchronize(zip_ctx *ctx);
/* the ctx's hipStream_t, for callers that order their own device work against it */
void *zip_ctx_stream(zip_ctx *ctx);

/* ---- commit ------------------------------------------------------------------
 * MultilinearZip::commit (commit.rs:50-87) when with_merkle != 0,
 * commit_no_merkle / encode_rows (commit.rs:104-119,158-183) when with_merkle == 0.
 * evals: the shard's row_count * row_len witness values (Int<1>), row-major.
 * n_evals must equal row_count * row_len (ZIP_ERR_SHAPE otherwise, commit.rs:56-63).
 * roots_out: HOST, row_count * 32 bytes, may be NULL.
 * The returned handle owns the device-resident MultilinearZipData. */
int32_t zip_commit(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind,
                   int32_t with_merkle, uint8_t *roots_out, zip_commitment **out);
void zip_commitment_free(zip_commitment *c);

/* zip_commit (with Merkle trees) for a caller that already knows which columns it is going to open.  In the
 * prover flow it does: ZincProver::commit_z_mle_and_prove_evaluation (src/zinc/prover.rs:305-328) opens with a
 * FRESH PcsTranscript (prover.rs:316) and write_integers / write_merkle_proof never absorb
 * (src/zip/pcs_transcript.rs:115-135,198-211), so the column indices of open (src/zip/pcs/open_z.rs:116-120) are
 * a function of the field configuration alone and the shim can squeeze them before it commits.
 * cols: HOST, n_cols indices < codeword_len (duplicates allowed).
 * Same roots and the same handle semantics as zip_commit; the hint only lets the commit kernel skip the HBM
 * stores no opening of those columns can read (about three quarters of the encoded rows and tree nodes at 1000
 * of 8192 columns) and put what they do read of the entries and of tree levels 0..2 into one dense block per row.
 * Whatever else is later asked of the handle -- an opening of any other column list (codeword_len >= 512: of
 * anything but exactly `cols`, in that order), zip_commit_download, the rows / layers device pointers -- first
 * re-runs the commit in full from the witness, transparently; for that a DEVICE
 * `evals` must stay valid and unchanged until the handle is freed.  Geometries below codeword_len 512 and above
 * 16384 ignore the hint (a hinted or packed commit above 16384 is not built): they store everything. */
/* zip_commit and the opening hint: a ctx whose zip_open / zip_open_stream has named a column list hints its NEXT plain
 * zip_commit calls (with_merkle != 0) with that list on its own -- in the prover's flow (commit, then open on a fresh
 * PcsTranscript: src/zinc/prover.rs:315-320) the columns never change, so the two unchanged calls run at the hinted
 * commit's speed and produce the same bytes.  The handle's semantics stay zip_commit's: whatever it is asked for that
 * the hint did not keep completes it first (a transparent re-run of the commit from the witness).
 *   default      only commits of a HOST witness speculate (the Rust binding's case: poly.evaluations): the re-run reads
 *                the library's own device copy, nothing changes for the caller's buffers;
 *   on != 0      commits of a DEVICE witness speculate too.  LIFETIME RULE the caller accepts with this call: the device
 *                witness of such a commit must stay valid and unchanged until its handle is freed -- a re-run reads it
 *                again (from the witness zip_open is handed, or from `evals` of the commit, whose digest, taken beside
 *                the commit kernel, must then still match: ZIP_ERR_INVALID_PARAM otherwise);
 *   on == 0      no speculation on this ctx.
 * ZIP_HIP_SPECULATE=0 / 1 makes "off" / "device witnesses too" the process-wide default. */
int32_t zip_ctx_set_speculation(zip_ctx *ctx, int32_t on);

int32_t zip_commit_hinted(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind,
                          const uint32_t *cols, uint32_t n_cols, uint8_t *roots_out, zip_commitment **out);

/* ---- proximity tests beyond one: LinearCodeSpec::num_proximity_testing (src/zip/code.rs:217-242) --------------------
 * The proximity coefficients are 64-bit challenges; repeating the test is how a spec buys more proximity soundness
 * (open_z.rs:103 and verify_z.rs:71 loop over the tests).  T = n_tests, default 1, accepted 1 .. 8; 0 or above 8 is
 * ZIP_ERR_UNSUPPORTED, and so is T > 1 on a row-sharded ctx.  With T set, and num_rows > 1 (a one-row matrix has no
 * test at all, whatever T is):
 *   stream     u'_0 | ... | u'_{T-1} | columns | evaluation row (commit.rs:726): the column section and the row do not
 *              depend on T, they only start (T - 1) * row_len * m_limbs * 8 bytes later
 *   coeffs     T * num_rows values, test-major, in the order they are squeezed: test 0 .. test T-1, then the columns
 *              (nothing between the first squeeze and the evaluation row absorbs)
 * honoured by zip_proof_len, zip_open_testing (uprime_out: T * row_len * m_limbs), zip_open, zip_commit_open,
 * zip_commit_open_begin / zip_job_wait, zip_open_stream (the first piece carries all T rows) and zip_verify, on every
 * kind of handle.  The prover computes tests 1 .. T-1 in ONE extra pass over the witness; the verifier checks them
 * from the column values alone, nothing is hashed again.  In zip_verify ZIP_VERIFY_PROXIMITY_TESTING at opening i
 * means that ANY test failed there (verify_z.rs:92-97 checks every test of a column before its Merkle records), and
 * ZIP_VERIFY_OVERFLOW that encode_wide overflowed for ANY u'_t.
 * These stay ONE-test paths and return ZIP_ERR_UNSUPPORTED on a ctx with T > 1, before anything reaches the device:
 * zip_batch_open, zip_batch_verify, zip_open_shard, zip_mctx_commit_open. */
int32_t zip_ctx_set_proximity_tests(zip_ctx *ctx, uint32_t n_tests);
uint32_t zip_ctx_proximity_tests(const zip_ctx *ctx); /* 0 for NULL */

/* Device views of the handle (zero-copy interop).  rows: row_count*cw*4 u64 -- asking for them expands the
 * 16-byte entries a commitment keeps internally into this array once (a copy of row_count*cw*32 bytes on the
 * device); pass rows == NULL if only the layers / roots are wanted.
 * layers: per row 2*cw hashes of 32 B (level k at hash offset 2cw-(2cw>>k), root at
 * 2cw-2, last slot padding).  roots: row_count*32 B.  Any out pointer may be NULL. */
int32_t zip_commitment_device_ptrs(zip_commitment *c, uint64_t **rows, uint8_t **layers, uint8_t **roots);
/* Host copies in the reference's layout: rows_out row_count*cw*k_limbs u64
 * (MultilinearZipData.rows), layers_out row_count * ((2<<depth)-2) * 32 B
 * (MerkleTree.layers of every row, root popped), roots_out row_count*32 B. */
int32_t zip_commit_download(zip_commitment *c, uint64_t *rows_out, uint8_t *layers_out, uint8_t *roots_out);
/* Build a handle from host data in the layout above (the reference's tests mutate
 * MultilinearZipData before opening: commit.rs:389, open_z.rs:230-241). */
int32_t zip_commitment_upload(zip_ctx *ctx, const uint64_t *rows, const uint8_t *layers, const uint8_t *roots,
                              zip_commitment **out);

/* ---- open ----------------------------------------------------------------------
 * The three parts of MultilinearZip::open (open_z.rs:22-40) with the transcript
 * outputs as inputs: coeffs = get_integer_challenges(num_rows) (open_z.rs:104),
 * cols = the squeezed column indices (open_z.rs:118), q0_mont = the eq tensor of the
 * last log2(num_rows) point coordinates (pcs/utils.rs:279-292).  Shard-local slices
 * (row_count entries) when the ctx is a row shard. */

/* prove_testing_phase, proximity rows (open_z.rs:103-112): coeffs T * num_rows, uprime_out T * row_len * m_limbs u64
 * (T = zip_ctx_proximity_tests, 1 unless set). */
int32_t zip_open_testing(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                         uint64_t *uprime_out, zip_mem_kind out_kind);
/* open_merkle_trees_for_column for n_cols columns (open_z.rs:116-120,124-143): wire_out gets
 * n_cols * row_count * (8*k_limbs + 8 + 32*depth) bytes in proof-stream format. */
int32_t zip_open_columns(zip_commitment *c, const uint32_t *cols, uint32_t n_cols, uint8_t *wire_out,
                         zip_mem_kind out_kind);
/* prove_evaluation_phase (open_z.rs:62-91): row_out row_len * field->limbs u64 (Montgomery limbs).
 * When num_rows == 1 q0_mont is ignored and row_out = map_to_field(evals).
 *
 * PARITY UNPINNED -- the signed-modulus quirk.  For a modulus q whose top bit is set in its limb width with
 * 2^(64 limbs) - q < 2^64 (e.g. q = 2^256 - 189, benches/spartan_benches.rs:134-137) the kernels first reduce |w|
 * modulo 2^(64 limbs) - q (`quirk_mod`), because the builder READS src/field.rs:550-557 as doing so: `F::I = Int<N>`
 * makes the modulus a NEGATIVE Int inside map_to_field's `%=`.  That reading of crypto-bigint 0.6's `Int::rem`
 * sign semantics has no published vector and could not be run here (no cargo); it changes results only for such
 * moduli (never for the 256-bit modulus of benches/zip_benches.rs:253: its top bit is set too, but 2^256 - q there
 * is far above 2^64, so a 64-bit |w| is never touched), it is applied
 * identically in zip_open_eval, zip_open, zip_verify, zip_mle_eval and zip_field_map_int256, and
 * integration/rust/fixture_dump.rs + tests/test_rust_fixtures.py pin it the first time a maintainer runs
 * `cargo test fixture_dump`. */
int32_t zip_open_eval(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const uint64_t *q0_mont,
                      const zip_field *field, uint64_t *row_out, zip_mem_kind out_kind);
/* proof length in bytes for n_cols openings (commit.rs:712-737) */
size_t zip_proof_len(const zip_ctx *ctx, uint32_t n_cols, uint32_t field_limbs);
/* Whole proof stream of open() in one call, witness read once:
 *   [u'_0 .. u'_{T-1} : row_len*m_limbs*8 B each, only if num_rows > 1] [n_cols column openings] [row_len field
 *   elements, big-endian bytes of the Montgomery value (pcs_transcript.rs:107-113)].
 * The caller still absorbs the field elements into its transcript afterwards.
 * Only valid on an unsharded ctx. */
int32_t zip_open(zip_commitment *c, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                 const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                 uint8_t *proof_out, zip_mem_kind out_kind);

/* The open of ONE ROW SHARD in one call (ctx created with row_begin / row_count; SURVEY.md 8e, one process per GPU):
 * one pass over the shard's rows of the witness for BOTH partial row combinations -- partial u' (row_len * m_limbs
 * u64) and partial evaluation row (row_len * limbs u64, Montgomery limbs) over the shard's rows, to be all-gathered
 * and added with zip_sum_partials -- and the shard's rows of every opened column in wire order
 * ([n_cols][row_count * 32 B values | row_count records]), pipelined behind the shard's commit kernel.
 * coeffs / q0_mont: the shard's slices (row_count entries), HOST; everything else DEVICE.  Returns when the device work
 * has finished. */
int32_t zip_open_shard(zip_commitment *c, const int64_t *evals_d, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                       const uint64_t *q0_mont, const zip_field *field, uint64_t *uprime_part_d, uint64_t *row_part_d,
                       uint8_t *wire_d);

/* commit + open in ONE call: what ZincProver::commit_z_mle_and_prove_evaluation (src/zinc/prover.rs:305-328) does with
 * its two calls, commit (commit.rs:50-87) and open (open_z.rs:22-40) on a fresh PcsTranscript -- the binding for that
 * function body.  Same roots and byte-identical proof stream as zip_commit followed by zip_open; internally
 * zip_commit_hinted + the pipelined open.
 *   roots_out  HOST, num_rows * 32 bytes, may be NULL
 *   proof_out  zip_proof_len() bytes, HOST or DEVICE per out_kind
 *   out        may be NULL (the handle is then freed); otherwise a handle like zip_commit_hinted's: anything later
 *              asked of it that is not in it first re-runs the commit in full, transparently -- a DEVICE `evals` must
 *              stay valid and unchanged until the handle is freed.
 * Unsharded ctx only. */
int32_t zip_commit_open(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                        const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                        uint8_t *roots_out, uint8_t *proof_out, zip_mem_kind out_kind, zip_commitment **out);

/* zip_commit_open as a JOB, for a caller that proves several polynomials in a row (the reference's batch paths are
 * loops over polynomials, commit.rs:134-142, open_z.rs:43-58): _begin enqueues the whole commit + open and returns,
 * zip_job_wait collects it.  With a second _begin made before the first job is waited for, the commit kernel of the
 * second polynomial starts the moment the first one's ends and runs beside the tail of the first one's openings
 * (the last chunk's gather, which has the GPU to itself otherwise) -- about 10 % more proofs per second at 2^24.
 * At most TWO jobs per ctx are in flight; a third _begin returns ZIP_ERR_INVALID_PARAM.
 *   evals_d, proof_out_d   DEVICE memory, valid and untouched until the job has been waited for
 *   coeffs, cols, q0_mont  HOST, consumed before _begin returns
 *   roots_out              HOST, num_rows * 32 bytes, or NULL
 * zip_job_wait frees the job whatever it returns.  Unsharded ctx only. */
typedef struct zip_job zip_job;
int32_t zip_commit_open_begin(zip_ctx *ctx, const int64_t *evals_d, size_t n_evals, const int64_t *coeffs,
                              const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                              uint8_t *proof_out_d, zip_job **job);
int32_t zip_job_wait(zip_job *job, uint8_t *roots_out);

/* ---- batches: many small polynomials in one launch ----------------------------------
 * The reference's batch_commit / batch_open (commit.rs:134-142, open_z.rs:43-58) for polynomials that do not fill the
 * machine one at a time (2^12: 64 one-wave workgroups): all polynomials of a batch share the ctx's geometry and
 * permutations, every row has its own Merkle tree, so B polynomials of R rows are B * R rows to ONE commit launch, and
 * the open is one launch set with the polynomial as a grid dimension.  The number of launches does not depend on B.
 * The verifier's side of the family, zip_batch_verify, is declared with zip_verify below.
 * Unsharded ctx, codeword_len <= 16384, 1 <= n_polys <= 65535, n_polys * num_rows < 2^32.
 *
 * zip_batch_commit: MultilinearZip::commit (with Merkle trees) of n_polys polynomials.
 *   evals      polynomial-major, n_polys * num_rows * row_len values, contiguous.  A HOST witness is copied and the
 *              batch keeps the device copy; a DEVICE witness is read in place and must outlive the handle and its
 *              members (the rule of zip_sumcheck_init's tables).  The later calls take no witness argument.
 *   roots_out  HOST, n_polys * num_rows * 32 bytes, may be NULL
 * Roots, rows and layers of polynomial i are byte-identical to those of a plain zip_commit of polynomial i.
 * Errors, before anything reaches the device: ZIP_ERR_NULL (ctx, evals, out), ZIP_ERR_INVALID_PARAM (n_polys 0 or
 * above 65535, row-sharded ctx), ZIP_ERR_UNSUPPORTED (codeword_len above 16384 -- not launch-bound, the jobs above
 * serve them --, n_polys * num_rows beyond 32 bits), ZIP_ERR_SHAPE (n_evals).
 *
 * zip_batch_member: a zip_commitment for polynomial `index` that borrows the batch's storage -- a plain, complete,
 * unhinted handle like an uploaded one, good for zip_open, zip_open_columns, zip_open_stream, zip_commit_download,
 * zip_commitment_device_ptrs, zip_commitment_mle_eval and zip_commitment_free.  Members and the batch are freed in any
 * order; the storage lives until the last of them is.  index >= size: ZIP_ERR_INVALID_PARAM.
 *
 * zip_batch_open_eval: prove_evaluation_phase (open_z.rs:62-91) of every polynomial.
 *   q0_mont    HOST, n_polys * num_rows * limbs: one eq tensor per polynomial (the points differ); NULL when num_rows == 1
 *   rows_out   n_polys * row_len * limbs Montgomery limbs; polynomial i's part equals zip_open_eval of polynomial i
 *
 * zip_batch_open: n_polys proof streams; stream i starts at byte i * zip_proof_len (a multiple of 8, not of 16) of
 * proofs_out and is byte-identical to zip_open of polynomial i with coeffs[i], cols[i], q0[i] -- the concatenation is what
 * batch_open leaves in a shared PcsTranscript stream.  In `open` only write_field_elements absorbs
 * (pcs_transcript.rs:107-113), and the evaluation row depends on the witness and the point alone: a caller first takes
 * all rows (zip_batch_open_eval), walks its transcript on the host -- per polynomial: squeeze the coefficients, squeeze
 * the columns, absorb the row --, then makes this one call.
 *   coeffs     HOST, n_polys * num_rows (NULL when num_rows == 1)
 *   cols       HOST, n_polys * n_cols, duplicates allowed; an index >= codeword_len is ZIP_ERR_INVALID_PARAM */
typedef struct zip_batch zip_batch;
int32_t zip_batch_commit(zip_ctx *ctx, const int64_t *evals, size_t n_evals, uint32_t n_polys, zip_mem_kind evals_kind,
                         uint8_t *roots_out, zip_batch **out);
uint32_t zip_batch_size(const zip_batch *b); /* 0 for NULL */
void zip_batch_free(zip_batch *b);           /* NULL is a no-op */
int32_t zip_batch_member(zip_batch *b, uint32_t index, zip_commitment **out);
int32_t zip_batch_open_eval(zip_batch *b, const uint64_t *q0_mont, const zip_field *field, uint64_t *rows_out,
                            zip_mem_kind out_kind);
int32_t zip_batch_open(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                       const zip_field *field, uint8_t *proofs_out, zip_mem_kind out_kind);

/* ---- batches whose members have their own code and their own field ----------------------
 * A batch of Zinc proofs of one circuit (ZincProver::prove_batch): every proof draws the two seeds of its RAA code and
 * its field from its own transcript (prover.rs:313), so the members of its PCS step share the geometry and nothing else.
 * Only the commit reads a code -- the row combinations read the witness, the column openings read row entries and trees
 * -- so ONE entry point takes the permutations per member, and the two open calls take the fields per member.
 *
 * zip_batch_commit_codes: zip_batch_commit with one RAA code per member.
 *   perms1, perms2   HOST, n_polys * codeword_len entries each, member-major: member i's slices are what
 *                    zip_params.perm1 / perm2 would be for it.  They are uploaded once, into the batch's storage.
 * The ctx supplies geometry, streams and pools; its own permutations are not read.  Roots, rows and layers of member i
 * are byte-identical to a plain zip_commit on a ctx created with member i's permutations.  The result is an ordinary
 * zip_batch: zip_batch_size / _member / _free, zip_batch_open_eval / _open (which never read a permutation) and
 * everything a member handle serves work on it unchanged; members are complete and unhinted, nothing re-runs a commit.
 * Errors, before anything reaches the device, in zip_batch_commit's order with two additions: ZIP_ERR_NULL also for
 * perms1 / perms2; ZIP_ERR_INVALID_PARAM (n_polys, row-sharded ctx); ZIP_ERR_UNSUPPORTED (codeword_len above 8192: the
 * geometry is not built -- a Zinc batch has at most 2^16 rows, codewords of 1024 --, n_polys * num_rows beyond 32 bits);
 * ZIP_ERR_SHAPE (n_evals); last, ZIP_ERR_INVALID_PARAM for a slice that is not a permutation of [0, codeword_len)
 * (zip_ctx_create's test, per member).
 *
 * zip_batch_open_eval_fields, zip_batch_open_fields: the two open calls with one field per member.
 *   fields     HOST, n_polys pointers; fields[i] is member i's field.  All share one `limbs` (as in zip_ccs_batch_set_z),
 *              each has its own modulus; q0_mont's slice i holds Montgomery limbs of fields[i]
 * Layouts, the stream stride (zip_proof_len depends on limbs only) and everything else are those of the one-field calls;
 * stream i is byte-identical to zip_open of member i with fields[i].  Both work on a batch from either commit entry point.
 * Errors in the one-field calls' order, where those look at their field: ZIP_ERR_NULL (fields, a fields[i]), then
 * ZIP_ERR_INVALID_PARAM (limbs outside {2, 3, 4}, differing limb counts, a modulus that is even or 1) -- all before
 * anything reaches the device.
 *
 * zip_batch_codes_counts: process-wide, monotonic, kept like zip_batch_verify_calls: zip_batch_commit_codes calls that
 * reached the device, the members they committed, and calls of the two _fields entry points that reached the device
 * (zip_batch_open_each is zip_batch_open_fields with another delivery and counts as one).  Any pointer may be NULL.
 *
 * The verifier's side of this family, zip_batch_verify_codes, is declared with zip_batch_verify below.
 *
 * Not part of this family: codewords above 8192 in the commit (the verifier serves them up to 16384); more than one
 * proximity test in a batch; row-sharded contexts. */
int32_t zip_batch_commit_codes(zip_ctx *ctx, const int64_t *evals, size_t n_evals, uint32_t n_polys, zip_mem_kind evals_kind,
                               const uint32_t *perms1, const uint32_t *perms2, uint8_t *roots_out, zip_batch **out);
int32_t zip_batch_open_eval_fields(zip_batch *b, const uint64_t *q0_mont, const zip_field *const *fields, uint64_t *rows_out,
                                   zip_mem_kind out_kind);
int32_t zip_batch_open_fields(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                              const uint64_t *q0_mont, const zip_field *const *fields, uint8_t *proofs_out,
                              zip_mem_kind out_kind);
void zip_batch_codes_counts(uint64_t *commits, uint64_t *members, uint64_t *field_opens);

/* ---- a batch open that delivers every stream to a buffer of its own ---------------------
 * zip_batch_open_fields writes n_polys streams into ONE block of n_polys * zip_proof_len bytes, on the device and (HOST
 * output) on the host.  zip_batch_open_each writes stream i to proofs_out[i] and never holds more than two windows of
 * streams at once: no device or host block grows with n_polys, and the first streams leave the device while later
 * members are still being gathered.
 *   coeffs, cols, n_cols, q0_mont, fields   exactly as for zip_batch_open_fields (a caller with one field passes the
 *                same pointer n_polys times); the batch may come from either commit entry point
 *   proofs_out   HOST array of n_polys pointers; proofs_out[i] receives zip_proof_len bytes, byte-identical to stream i
 *                of zip_batch_open_fields with the same arguments (and so to zip_open of member i).  The destinations
 *                need not be contiguous or in order; their ranges must not overlap
 *   out_kind     of every destination.  HOST: any alignment, pageable or pinned (zip_host_register).  DEVICE: 8-byte
 *                aligned, the alignment a stream has inside zip_batch_open_fields' block
 *   window_bytes HOST output only: members leave in windows of W = max(1, window_bytes / zip_proof_len) consecutive
 *                members (0 = 64 MiB, zip_open_stream's default).  The library stages at most two windows on the device
 *                (two slots from the ctx's pool, reused): while window w is copied out on the ctx's second stream, window
 *                w + 1 is combined and gathered.  Each stream goes from its slot straight to proofs_out[i]: a pinned
 *                destination by one asynchronous copy, a pageable one through the library's bounce buffers.
 * DEVICE output has no staging and no windows (window_bytes is ignored): the kernels write through a device table of
 * the destinations.  The call returns when every byte has landed (DEVICE: as zip_batch_open_fields does).
 * Errors, all before anything reaches the device, in zip_batch_open_fields' order with these additions: ZIP_ERR_NULL
 * also for proofs_out and any proofs_out[i]; after the column indices, ZIP_ERR_INVALID_PARAM for a DEVICE destination that
 * is not 8-byte aligned and for two destinations whose zip_proof_len-byte ranges overlap.  A ctx set to more than one
 * proximity test is refused (ZIP_ERR_UNSUPPORTED) as by the other batch opens.  Batch and ctx stay usable after any error.
 *
 * zip_batch_open_each_counts: process-wide, kept like zip_batch_codes_counts: calls that reached the device, the members
 * and the windows of those calls (monotonic; a DEVICE call is one window), and the bytes of device staging the most
 * recent such call asked its pool for (0 for DEVICE output).  Any pointer may be NULL. */
int32_t zip_batch_open_each(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                            const uint64_t *q0_mont, const zip_field *const *fields, uint8_t *const *proofs_out,
                            zip_mem_kind out_kind, size_t window_bytes);
void zip_batch_open_each_counts(uint64_t *calls, uint64_t *members, uint64_t *windows, uint64_t *last_staging_bytes);

/* ---- streaming proof writer -------------------------------
 * zip_open with the stream delivered to `sink` in order, piece by piece (u', then groups of opened
 * columns, then the evaluation row), instead of into one contiguous buffer: the 1.74 GiB proof of a
 * 2^24 witness never needs a single host allocation, and the PCIe copy of one group overlaps the
 * gather of the next.  `bytes` points into pinned memory owned by the library and is valid only
 * during the call; a non-zero return from the sink aborts (ZIP_ERR_INVALID_PARAM).
 * chunk_bytes: target size of a column group (0 = 64 MiB).  The concatenation of all pieces is
 * byte-identical to what zip_open writes. */
typedef int32_t (*zip_proof_sink)(void *user, const uint8_t *bytes, size_t len);
int32_t zip_open_stream(zip_commitment *c, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                        const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                        zip_proof_sink sink, void *user, size_t chunk_bytes);

/* ---- verifier side ---------------------------------------------
 * MultilinearZip::verify (src/zip/pcs/verify_z.rs:19-188) on the device.  The caller (the Rust
 * shim / zinc_amd/host) keeps the Fiat-Shamir work: it squeezes `coeffs` (T * num_rows, test-major, only when
 * num_rows > 1; T = zip_ctx_proximity_tests) and the `cols`, builds (q0, q1) = point_to_tensor (pcs/utils.rs:252-276) and, after
 * the call, absorbs the row_len field elements at the end of the stream
 * (read_field_elements, pcs_transcript.rs:138-160).
 *   roots      HOST, num_rows * 32 bytes (MultilinearZipCommitment.roots)
 *   proof      the stream `open` wrote, zip_proof_len() bytes (longer is allowed, shorter is malformed)
 *   q1_mont    row_len field elements (may be NULL when row_len == 1: q_1 is empty there)
 *   eval_mont  the claimed evaluation, Montgomery limbs
 * report->verdict is the first check that fails in the reference's order, ZIP_VERIFY_ACCEPT if none.
 * Deliberate differences from the reference, both on the rejecting side:
 *  - Merkle paths ARE checked (the reference computes the check and drops the result,
 *    verify_z.rs:99, but then loses its place in the stream at the first bad path);
 *  - evaluation-row elements >= q that survive the evaluation-consistency check (which is
 *    representation independent and comes first, as in the reference) are rejected as malformed; the
 *    reference does not range-check them and its sequential modular additions in encode_f then
 *    depend on the representation.
 * The function result is only non-zero for usage / device errors. */
typedef enum {
    ZIP_VERIFY_ACCEPT = 0,
    ZIP_VERIFY_PROXIMITY_TESTING = 1, /* "Proximity failure", verify_z.rs:122-125 */
    ZIP_VERIFY_EVAL_CONSISTENCY = 2,  /* "Evaluation consistency failure", verify_z.rs:145-149 */
    ZIP_VERIFY_PROXIMITY_Q0 = 3,      /* "Proximity failure", verify_z.rs:184-186 */
    ZIP_VERIFY_MERKLE = 4,            /* a path does not hash to its row root */
    ZIP_VERIFY_MALFORMED = 5,         /* short stream, wrong path length prefix, non-canonical field element */
    ZIP_VERIFY_OVERFLOW = 6           /* encode_wide overflows Int<M>: the reference panics (int.rs:122-134) */
} zip_verify_verdict;
typedef struct {
    int32_t verdict;
    uint32_t column;           /* index into cols[] of the failing opening, when the verdict names one */
    uint32_t bad_merkle_paths; /* over all openings */
    uint32_t malformed_paths;
} zip_verify_report;
int32_t zip_verify(zip_ctx *ctx, const uint8_t *roots, const uint8_t *proof, zip_mem_kind proof_kind, size_t proof_len,
                   const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                   const uint64_t *q1_mont, const uint64_t *eval_mont, const zip_field *field,
                   zip_verify_report *report);

/* zip_batch_verify: MultilinearZip::batch_verify_z (verify_z.rs:40-58) for n_polys proofs of the ctx's geometry in one
 * launch set -- the third member of the batch family above, with the same constraints (unsharded ctx, codeword_len
 * <= 16384, 1 <= n_polys <= 65535).  batch_verify_z runs verify per polynomial on ONE PcsTranscript, so the challenges
 * of polynomial i depend on what polynomials 0 .. i-1 absorbed; but in `verify` only read_field_elements absorbs
 * (pcs_transcript.rs:91-103; read_integers and read_merkle_proof do not, :137-155, :181-196), and what it absorbs are
 * bytes of the stream itself at a known offset, the last row_len * 8 * limbs bytes of stream i.  The whole transcript
 * walk -- per polynomial: squeeze the coefficients (num_rows > 1), squeeze the columns, absorb the row read from the
 * stream -- is therefore host work that needs no verdict; the caller does it first and then makes this one call.
 *   proofs      HOST or DEVICE per proofs_kind; stream i starts at byte i * zip_proof_len(ctx, n_cols, field->limbs)
 *               (a multiple of 8, not of 16): the layout zip_batch_open writes
 *   proofs_len  bytes available at `proofs`.  A polynomial whose stream does not lie wholly inside gets
 *               ZIP_VERIFY_MALFORMED with zero counts (what zip_verify gives a short stream) and never reaches the
 *               device; the polynomials before it are verified.
 *   HOST, polynomial-major: roots n_polys * num_rows * 32 bytes; coeffs n_polys * num_rows (NULL when num_rows == 1);
 *               cols n_polys * n_cols; q0_mont n_polys * num_rows * limbs (NULL when num_rows == 1); q1_mont
 *               n_polys * row_len * limbs (may be NULL when row_len == 1); evals_mont n_polys * limbs
 *   reports     HOST, n_polys entries.  reports[i] equals, field by field, what zip_verify returns for polynomial i's
 *               slices, for every input, with every deliberate deviation documented there.
 * Five kernel launches whatever n_polys is, one device-to-host copy (of the n_polys reports), one synchronisation.
 * Errors, before anything reaches the device: ZIP_ERR_NULL (ctx, roots, proofs, reports, evals_mont; cols when
 * n_cols != 0; a needed coeffs / q0_mont / q1_mont), ZIP_ERR_INVALID_PARAM (n_polys 0 or above 65535, row-sharded ctx,
 * a column index >= codeword_len), ZIP_ERR_UNSUPPORTED (codeword_len above 16384, n_polys * n_cols beyond 32 bits,
 * field limbs outside {2, 3, 4}).
 * zip_batch_verify_calls: process-wide, monotonic count of zip_batch_verify calls that reached the device (tests and
 * tools read from it which path a caller took; kept like zip_sumcheck_launch_counts). */
int32_t zip_batch_verify(zip_ctx *ctx, uint32_t n_polys, const uint8_t *roots, const uint8_t *proofs,
                         zip_mem_kind proofs_kind, size_t proofs_len, const int64_t *coeffs, const uint32_t *cols,
                         uint32_t n_cols, const uint64_t *q0_mont, const uint64_t *q1_mont, const uint64_t *evals_mont,
                         const zip_field *field, zip_verify_report *reports);
uint64_t zip_batch_verify_calls(void);

/* zip_batch_verify_codes: zip_batch_verify for the proofs of a Zinc batch (ZincVerifier::verify_batch): member i has its
 * own RAA code, its own field and its own stream buffer, and shares the ctx's geometry with the others and nothing else.
 *   ctx         geometry, stream and pools; its own permutations are not read (as in zip_batch_commit_codes)
 *   perms1, perms2   HOST, n_polys * codeword_len entries each, member-major, as for zip_batch_commit_codes.  Every slice
 *               is tested as zip_ctx_create tests a permutation -- the encode kernel indexes with these values
 *   fields      HOST, n_polys pointers, one `limbs` shared, each its own modulus (the rules of zip_batch_open_fields);
 *               slice i of q0_mont, q1_mont and evals_mont holds Montgomery limbs of fields[i]
 *   proofs, proof_lens   HOST arrays of n_polys entries: ONE pointer and ONE length per member -- the members are
 *               independent proofs with their own buffers.  proofs_kind HOST: stream i is copied into its slot of one
 *               pooled device block.  DEVICE: it is read in place and must be 8-byte aligned.
 *               A member with proof_lens[i] < zip_proof_len gets ZIP_VERIFY_MALFORMED with zero counts and never reaches
 *               the device (its pointer is not looked at); every other member is still verified: the members share no
 *               transcript, so none comes "after" another.
 *   roots, coeffs, cols, q0_mont, q1_mont, evals_mont   HOST, polynomial-major, as in zip_batch_verify
 *   reports     HOST, n_polys entries.  reports[i] equals, field by field, what zip_verify returns for member i's slices on
 *               a ctx created with member i's permutations and fields[i], for every input, both documented deviations
 *               included.  A batch may mix moduli with and without the signed-modulus quirk.
 * The same five kernel launches as zip_batch_verify whatever n_polys is (the member is a grid dimension; what differs
 * between members is one entry of a device array read through the scalar cache), one device-to-host copy of the
 * reports, one synchronisation.
 * Constraints: zip_batch_verify's (unsharded ctx, one proximity test, codeword_len <= 16384 -- not the 8192 of
 * zip_batch_commit_codes: the encode kernel reads its permutations from memory --, 1 <= n_polys <= 65535,
 * n_polys * n_cols within 32 bits).
 * Errors, all before anything reaches the device, in this order: ZIP_ERR_NULL (ctx, roots, proofs, proof_lens, reports,
 * evals_mont, cols when n_cols != 0, perms1, perms2); ZIP_ERR_INVALID_PARAM (n_polys, row-sharded ctx);
 * ZIP_ERR_UNSUPPORTED (more than one proximity test, codeword_len above 16384, n_polys * n_cols beyond 32 bits);
 * ZIP_ERR_NULL (fields, a fields[i]); ZIP_ERR_INVALID_PARAM (limbs outside {2, 3, 4}, differing limb counts, a modulus
 * that is even or 1); ZIP_ERR_NULL (a needed coeffs / q0_mont / q1_mont); ZIP_ERR_INVALID_PARAM (a column index >=
 * codeword_len); ZIP_ERR_NULL (the proofs[i] of a member that is long enough); ZIP_ERR_INVALID_PARAM (a misaligned DEVICE
 * stream); last, ZIP_ERR_INVALID_PARAM for a slice that is not a permutation of [0, codeword_len).
 * zip_batch_verify_codes_counts: process-wide, monotonic, kept like zip_batch_codes_counts: calls that reached the
 * device, and the members they verified (short members are not among them).  Either pointer may be NULL.
 * Not part of this: more than one proximity test in a batch; batches on zip_mctx. */
int32_t zip_batch_verify_codes(zip_ctx *ctx, uint32_t n_polys, const uint32_t *perms1, const uint32_t *perms2,
                               const uint8_t *roots, const uint8_t *const *proofs, const size_t *proof_lens,
                               zip_mem_kind proofs_kind, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                               const uint64_t *q0_mont, const uint64_t *q1_mont, const uint64_t *evals_mont,
                               const zip_field *const *fields, zip_verify_report *reports);
void zip_batch_verify_codes_counts(uint64_t *calls, uint64_t *members);

/* ---- sumcheck prover --------------------------------------------
 * IPForMLSumcheck::prove_round (src/sumcheck/prover.rs:62-180) for the two combination functions
 * ZincProver uses -- comb == NULL: comb_fn(vals) = vals[0] * vals[1] * ... (second sumcheck,
 * src/zinc/prover.rs:297-302); comb != NULL: sumcheck_polynomial_comb_fn_1 (src/zinc/utils.rs:77-94),
 *   (sum_t coeff[t] * prod_{j in term_mask[t]} vals[j]) * vals[n_mles - 1]
 * with coeff = ccs.c (Montgomery limbs), term_mask[t] = the bits of ccs.S[t] (positions in the MLE list of
 * prepare_lin_sumcheck_polynomial, zinc/utils.rs:49-75) and the eq() MLE last -- one call per round; the
 * caller keeps the
 * transcript (MLSumcheck::prove_as_subprotocol, src/sumcheck.rs:56-112: absorb the evaluations, squeeze
 * the challenge, absorb it, hand it to the next round).
 *   mles      n_mles (1..8) tables of 2^num_vars field elements, Montgomery limbs, variable 0 = least
 *             significant index bit; HOST tables are copied, DEVICE tables are read in place (never
 *             written) and must outlive the handle.  (A CCS with t matrices needs t + 1: t <= 7.)
 *   comb      a term_mask with a bit at or above n_mles is ZIP_ERR_INVALID_PARAM
 *   degree    1..4: the round polynomial is returned as its values at 0..degree (ProverMsg.evaluations)
 *   r_prev    the verifier's challenge for the previous round (NULL in round 1): the tables are folded
 *             with it (fix_variables, src/poly_f/mle/dense.rs:142-168) in the same pass
 *   evaluations_out  HOST, (degree + 1) * field->limbs limbs */
typedef struct zip_sumcheck zip_sumcheck;
typedef struct {
    uint32_t n_terms;      /* 1..8 */
    uint32_t term_mask[8]; /* bit j: MLE j is a factor of the term */
    uint64_t coeff[8][8];  /* Montgomery limbs, little-endian, unused limbs zero */
} zip_sumcheck_comb;
int32_t zip_sumcheck_init(int32_t device, const uint64_t *const *mles, zip_mem_kind kind, uint32_t n_mles,
                          uint32_t num_vars, uint32_t degree, const zip_sumcheck_comb *comb, const zip_field *field,
                          zip_sumcheck **out);
int32_t zip_sumcheck_round(zip_sumcheck *s, const uint64_t *r_prev, uint64_t *evaluations_out);
/* The same round in two halves -- enqueue, then collect -- so that several handles (the products of a
 * sum-of-products polynomial, src/sumcheck/utils.rs:27-78: each product folds its own MLEs, the round messages
 * add up) work at the same time on their own streams. */
int32_t zip_sumcheck_round_begin(zip_sumcheck *s, const uint64_t *r_prev);
int32_t zip_sumcheck_round_end(zip_sumcheck *s, uint64_t *evaluations_out);
const char *zip_sumcheck_last_error(const zip_sumcheck *s);
void zip_sumcheck_free(zip_sumcheck *s);

/* A KeccakTranscript (src/transcript.rs) in transit: Keccak-256 sponge, rate 136.
 * st: the state after every full block absorbed so far; buf[0 .. buflen): the bytes absorbed since, buflen < 136.
 * On input bytes at and beyond buflen are ignored; on output they are zero. */
typedef struct {
    uint64_t st[25];
    uint8_t buf[136];
    uint32_t buflen;
} zip_keccak_state;

/* MLSumcheck::prove_as_subprotocol (src/sumcheck.rs:56-112) in ONE call on a fresh handle (no round played yet):
 * absorbs nvars and degree (:64-76), then for every round computes the message, absorbs it (absorb_slice),
 * squeezes the challenge (get_challenge, transcript.rs:88-133), absorbs it and folds with it.  For this loop, and
 * only for it, the library owns the transcript.  The last rounds -- from tables of 2^n entries on, n =
 * ZIP_HIP_SUMCHECK_TAIL or as many as fit the LDS of one workgroup -- run in ONE kernel with the sponge on the
 * device; the rounds before use the kernels of zip_sumcheck_round and the library steps the sponge on the host.
 *   transcript      HOST, in/out: the caller's transcript before / after the sumcheck
 *   msgs_out        HOST, num_vars * (degree + 1) * field->limbs limbs (ProverMsg.evaluations per round)
 *   randomness_out  HOST, num_vars * field->limbs limbs (ProverState.randomness), Montgomery
 * ZIP_ERR_INVALID_PARAM (nothing reaches the device): a round already played or in flight on the handle, a second
 * zip_sumcheck_prove, buflen >= 136.  Afterwards the handle is finished: zip_sumcheck_round* return
 * "Prover is not active". */
int32_t zip_sumcheck_prove(zip_sumcheck *s, zip_keccak_state *transcript, uint64_t *msgs_out, uint64_t *randomness_out);
/* Process-wide, monotonic: rounds played through the round kernels (zip_sumcheck_round_begin, from whichever entry
 * point) and launches of the tail kernel.  Every path gives the same bytes; tests and tools read the path taken here.
 * Either pointer may be NULL. */
void zip_sumcheck_launch_counts(uint64_t *round_kernel_rounds, uint64_t *tail_kernel_launches);
/* Process-wide, monotonic, kept like zip_sumcheck_launch_counts -- of the round-kernel launches so far: those whose
 * grid-stride loop ran more than one pass (points of the round > workgroups launched * points per workgroup), those
 * among them whose last pass was not taken by every workgroup, and those that left their partials to
 * sumcheck_reduce_kernel (grid above 64).  Computed on the host at launch.  ZIP_HIP_SUMCHECK_GRID=n (test hook,
 * 1 .. 8 * CUs, read per round) caps the workgroups of a round-kernel launch, after every other cap: with it the tests
 * reach these regimes at small sizes.  Any pointer may be NULL. */
void zip_sumcheck_grid_counts(uint64_t *multi_pass, uint64_t *uneven_last_pass, uint64_t *reduce_kernel);

/* A sum of products in ONE handle: the polynomial of rand_poly / rand_poly_comb_fn (src/sumcheck/utils.rs:27-78, what
 * benches/sumcheck_benches.rs and src/sumcheck/tests.rs prove),
 *   comb_fn(vals) = sum_t coeff[t] * prod_{j in term_mask[t]} vals[j]
 * with NO trailing factor; `products` is a zip_sumcheck_comb whose n_terms is the number of products.  One kernel per
 * round reads every table once and folds it once, whatever the number of products that share it.
 *   n_mles    1..32 tables; products->n_terms 1..8; every term_mask has 1..4 bits set, none at or above n_mles.
 *             Masks may overlap and may repeat.  A table that belongs to no product is neither read nor folded (its
 *             pointer must still not be NULL).
 *   degree    1..4; it may exceed the largest product (rand_poly hands over the maximum it could have drawn)
 *   num_vars  1..30
 * Usage errors are those of zip_sumcheck_init, with the same codes and in the same order, before the device is touched:
 * ZIP_ERR_NULL for mles, out, field or products; then ZIP_ERR_INVALID_PARAM for n_terms, for n_mles / degree /
 * num_vars, for a mask.  HOST tables are copied, DEVICE tables are read in place and never written.
 * The handle is an ordinary zip_sumcheck: zip_sumcheck_round, zip_sumcheck_round_begin / _end, zip_sumcheck_prove,
 * zip_sumcheck_last_error and zip_sumcheck_free work on it as documented above.  zip_sumcheck_prove plays EVERY round
 * of such a handle through the round kernel and steps the sponge on the host (what ZIP_HIP_SUMCHECK_TAIL=0 does for the
 * other handles): the tail kernel does not know this combination function, so tail_kernel_launches does not move and
 * round_kernel_rounds grows by num_vars.  Not built: the tail kernel for this form, more than 8 products or 32 tables
 * in one handle (the host mirror keeps its loop of one handle per product for those).
 * Additive: the ABI version stays 3. */
int32_t zip_sumcheck_init_products(int32_t device, const uint64_t *const *mles, zip_mem_kind kind, uint32_t n_mles,
                                   uint32_t num_vars, uint32_t degree, const zip_sumcheck_comb *products,
                                   const zip_field *field, zip_sumcheck **out);

/* MANY small sumchecks of one shape in ONE launch: for instance i exactly what
 *   zip_sumcheck_init(device, inst[i].mles, tables_kind, n_mles, num_vars, degree, inst[i].comb, inst[i].field, &h)
 * followed by zip_sumcheck_prove on h and inst[i].transcript does, bit for bit (MLSumcheck::prove_as_subprotocol with the
 * absorption of nvars and degree) -- but workgroup i of one kernel plays every round of instance i with the sponge on
 * the device: one launch, one upload of the arguments, one device-to-host copy of the results and one synchronisation,
 * whatever n_instances is.  For callers of the batch family (zip_batch_commit ...) that hold many small proofs.
 *   inst            HOST, n_instances (1..65535) entries; every instance has its own tables, transcript, combination
 *                   (NULL: the product; the forms may differ between instances) and field (the same `limbs` for all)
 *   n_mles 1..8, degree 1..4, num_vars 1..16 (above: ZIP_ERR_UNSUPPORTED -- one sumcheck of that size fills the device
 *                   through the round kernels; loop over zip_sumcheck_prove)
 *   msgs_out        HOST, instance-major: n_instances * num_vars * (degree + 1) * limbs limbs
 *   randomness_out  HOST, n_instances * num_vars * limbs limbs
 * HOST tables are copied, DEVICE tables are read in place and never written.  The last n rounds are played from LDS, n =
 * ZIP_HIP_SUMCHECK_TAIL cut to what fits one workgroup (the bound of zip_sumcheck_prove's tail kernel) and to num_vars;
 * the rounds before stream the tables from HBM (round 1: the caller's; later: a per-instance scratch block).  Here
 * ZIP_HIP_SUMCHECK_TAIL=0 means that every round is streamed.
 * Errors, before anything reaches the device and in this order: ZIP_ERR_NULL (inst, msgs_out, randomness_out, any
 * instance's mles / field / transcript / a table pointer); ZIP_ERR_INVALID_PARAM (n_instances; n_mles, degree, num_vars;
 * limbs not in {2, 3, 4} or differing between instances; a comb with n_terms outside 1..8 or a mask bit at or above
 * n_mles; buflen >= 136; a modulus that is even or 1); ZIP_ERR_UNSUPPORTED (num_vars above 16).  ZIP_ERR_ALLOC when scratch
 * or staging cannot be had.  On ANY non-zero return no transcript has been modified and the outputs are unspecified.
 * Not part of this: the sum-of-products form of zip_sumcheck_init_products.  The caller's current device is restored.
 * Additive: the ABI version stays 3. */
typedef struct {
    const uint64_t *const *mles;   /* n_mles tables of 2^num_vars elements, Montgomery limbs */
    const zip_sumcheck_comb *comb; /* NULL: the product of all tables; else as in zip_sumcheck_init */
    const zip_field *field;        /* each instance its own (each proof draws its own field); same `limbs` for all */
    zip_keccak_state *transcript;  /* in/out, as in zip_sumcheck_prove */
} zip_sumcheck_instance;
int32_t zip_sumcheck_prove_batch(int32_t device, const zip_sumcheck_instance *inst, uint32_t n_instances,
                                 zip_mem_kind tables_kind, uint32_t n_mles, uint32_t num_vars, uint32_t degree,
                                 uint64_t *msgs_out, uint64_t *randomness_out);
/* Process-wide, monotonic, kept like zip_sumcheck_launch_counts: launches of the batch kernel, the instances they played,
 * and the rounds played from HBM (max(0, num_vars - n) per instance, computed on the host at launch).  A batch call
 * moves neither zip_sumcheck_launch_counts nor zip_sumcheck_grid_counts.  Any pointer may be NULL. */
void zip_sumcheck_batch_counts(uint64_t *launches, uint64_t *instances, uint64_t *streamed_rounds);

/* ---- the random field: prime_gen::get_prime (src/prime_gen.rs:15-28) ---------------------------------------------
 * draw_random_field (src/zinc/utils.rs:161-171) absorbs the public inputs and calls get_prime: hash a candidate of
 * 8 * limbs bytes out of the transcript (get_random_bytes: one squeeze with the 4-byte big-endian counter 0,
 * truncated), absorb those bytes, read them big-endian, subtract 1 if even, and repeat until
 * MillerRabin::test_base_two (src/field/uint.rs:66-76) accepts one.  The hash chain does not depend on the tests, and
 * the tests are independent modular exponentiations: the host hashes candidates in batches, the device tests a batch in
 * ONE launch with one candidate per lane, and the next batch is hashed while the current one is on the device.
 *
 * zip_prime_test_base2: the strong probable-prime test to base 2 of n candidates of `limbs` limbs each (HOST,
 * candidate-major, little-endian limbs; any odd value >= 3 up to 2^(64 limbs) - 1) -> verdicts_out (HOST, n bytes,
 * 1 = probably prime).  What the reference's test accepts is accepted: strong pseudoprimes to base 2 included.
 *   ZIP_ERR_NULL           candidates or verdicts_out is NULL
 *   ZIP_ERR_INVALID_PARAM  limbs not in {2, 3, 4}, n == 0, an even candidate or one below 3 -- nothing reaches the device
 *
 * zip_get_prime: get_prime::<RandomField<limbs>> on the caller's transcript.  For this call the library owns the
 * transcript (as zip_sumcheck_prove does for a sumcheck): on return *transcript is exactly what the reference's loop
 * leaves -- the sponge after absorbing the winner's bytes, nothing of the candidates hashed ahead beyond it.
 *   prime_out             HOST, `limbs` little-endian limbs: the first candidate the test accepts
 *   candidates_tried_out  the winner's 1-based position in the chain; may be NULL
 *   ZIP_ERR_NULL           transcript or prime_out is NULL
 *   ZIP_ERR_INVALID_PARAM  limbs not in {2, 3, 4}, buflen >= 136 -- before the device is touched
 *   ZIP_ERR_UNSUPPORTED    no candidate among the first 65536 was accepted (one line on stderr says so).  The reference
 *                          would loop for ever; the primes of 128 .. 256 bits are dense enough that this is a defect
 *                          of the device, not of the input.  *transcript is then unchanged.
 * ZIP_HIP_PRIME_BATCH=n (1 .. 4096) sets the candidates per launch; read per call.
 *
 * zip_prime_launch_counts: process-wide, monotonic -- launches of the test kernel (from either entry point) and the
 * candidates they tested, kept like zip_batch_verify_calls.  Either pointer may be NULL. */
int32_t zip_prime_test_base2(int32_t device, const uint64_t *candidates, uint32_t n, uint32_t limbs, uint8_t *verdicts_out);
int32_t zip_get_prime(int32_t device, zip_keccak_state *transcript, uint32_t limbs, uint64_t *prime_out,
                      uint32_t *candidates_tried_out);
void zip_prime_launch_counts(uint64_t *launches, uint64_t *candidates_tested);

/* zip_get_prime_batch: get_prime::<RandomField<limbs>> on n INDEPENDENT transcripts -- the fields of a whole batch of
 * proofs (zip_ccs_batch_*, zip_sumcheck_prove_batch, zip_batch_commit_codes, zip_batch_verify_codes: each member lives in
 * the field drawn from its own transcript).  Member i gets exactly what zip_get_prime(device, &transcripts[i], limbs, ...)
 * gives on its own: the same prime, the same 1-based winner position, the same sponge afterwards (the winner's state,
 * pending bytes and buflen; nothing of the candidates hashed beyond the winner).
 * Here the candidate chains run on the device too, one member per lane: a call proceeds in rounds of w candidates per
 * member still without a prime -- chain, test (the kernel of zip_prime_test_base2), a per-member reduction, and a replay
 * that walks each finished member's sponge to its winner.  The kernel launches of a call depend on the rounds its LONGEST
 * chain needs, not on n; one host synchronisation per round; one copy of the sponges up and one copy of primes, positions
 * and sponges back.
 *   transcripts           HOST, n entries, in/out
 *   primes_out            HOST, n * limbs little-endian limbs, member-major
 *   candidates_tried_out  HOST, n entries; may be NULL
 * Errors, answered before any device is looked for and in this order:
 *   ZIP_ERR_NULL           transcripts or primes_out is NULL
 *   ZIP_ERR_INVALID_PARAM  limbs not in {2, 3, 4}
 *   ZIP_ERR_INVALID_PARAM  n == 0 or n > 65535
 *   ZIP_ERR_INVALID_PARAM  a member with buflen >= 136
 * ZIP_ERR_UNSUPPORTED: some member has no probable prime among its first 65536 candidates (one line on stderr).
 * On EVERY non-zero return all n transcripts are byte-for-byte unchanged and zip_prime_batch_counts has not moved.
 * ZIP_HIP_PRIME_BATCH_WINDOW=w (1 .. 1024, default 64) sets the candidates per member and round; read per call, anything
 * else keeps the default.  zip_get_prime, zip_prime_test_base2, zip_prime_launch_counts and ZIP_HIP_PRIME_BATCH are
 * untouched: a batch call moves its own counters only.
 * Not part of this: members of differing limb counts in one call, more than one device per call.
 *
 * zip_prime_batch_counts: process-wide, monotonic -- successful zip_get_prime_batch calls, the members they served and
 * the kernel launches they made (four per round).  Any pointer may be NULL.
 * Additive: the ABI version stays 3. */
int32_t zip_get_prime_batch(int32_t device, zip_keccak_state *transcripts, uint32_t n, uint32_t limbs, uint64_t *primes_out,
                            uint32_t *candidates_tried_out);
void zip_prime_batch_counts(uint64_t *calls, uint64_t *members, uint64_t *kernel_launches);

/* ---- the field loops of SpartanProver::prove around its sumchecks (BASELINE configs[4]) ---------
 * A zip_ccs holds the constraint matrices of a CCS (Statement_Z.constraints, src/ccs/ccs_z.rs:155-158,
 * mapped to F_q as SparseMatrix::map_to_field does, src/sparse_matrix.rs:38-58) and the per-proof
 * tables in HBM.  With zip_sumcheck_* (tables handed over as ZIP_MEM_DEVICE) this is everything
 * src/zinc/prover.rs:130-161 computes; the caller keeps the transcript.
 *   zip_sparse_matrix   SparseMatrix<Int<1>> as CSR: row_ptr[n_rows + 1], col_idx / values[row_ptr[n_rows]].
 *                       n_cols must be 2^s and n_rows <= 2^s (missing rows are zero: pad_rows,
 *                       src/sparse_matrix.rs:104-108); else ZIP_ERR_SHAPE, where the reference panics
 *                       or returns LengthsNotEqual (src/ccs/utils.rs:52-59).
 *   zip_ccs_set_z       z = x || 1 || w (Statement_Z::get_z_vector), z_len <= 2^s, zero-extended
 *                       (prover.rs:230-232): builds z_ccs in F_q (:236) and the t tables M_k z
 *                       (calculate_Mz_mles, src/zinc/utils.rs:121-135)
 *   zip_ccs_eq_table    build_eq_x_r(r) (src/sumcheck/utils.rs:102-177), r = s Montgomery elements on
 *                       the HOST; slot 0 is for eq(beta) (prepare_lin_sumcheck_polynomial,
 *                       zinc/utils.rs:72), slot 1 for eq(r_x)
 *   zip_ccs_second_table  what sumcheck_2 needs (prover.rs:261-296): eq(r_x) into slot 1, the table
 *                       sum_k gamma^k * compute_eval_table_sparse(M_k, eq(r_x)) (src/sparse_matrix.rs:165-182),
 *                       and V_s[k] = (M_k z)(r_x) (calculate_V_s, prover.rs:330-347) to v_s_out (HOST, t elements)
 *   zip_ccs_eval_matrices  the verifier's V_xy (src/zinc/verifier.rs:248-261): mle[M_k](r_x, r_y) for every matrix,
 *                       DenseMultilinearExtension::from_matrix (src/poly_f/mle/dense.rs:69-87) evaluated without
 *                       building the dense 2^(2s) table; r_x, r_y: s elements each on the HOST; overwrites both eq slots
 *   zip_ccs_table       device pointer of a table of 2^s elements, valid until the next call that
 *                       rebuilds it or zip_ccs_free; index = matrix for ZIP_CCS_MZ, slot for ZIP_CCS_EQ
 *   zip_ccs_download    the same table copied to the HOST (tests) */
typedef struct zip_ccs zip_ccs;
typedef struct {
    uint32_t n_rows, n_cols;
    const uint32_t *row_ptr, *col_idx;
    const int64_t *values;
} zip_sparse_matrix;
typedef enum { ZIP_CCS_Z_FIELD = 0, ZIP_CCS_MZ = 1, ZIP_CCS_EQ = 2, ZIP_CCS_SECOND = 3 } zip_ccs_table_kind;
int32_t zip_ccs_create(int32_t device, const zip_sparse_matrix *matrices, uint32_t t, uint32_t s, const zip_field *field,
                       zip_ccs **out);
void zip_ccs_free(zip_ccs *c);
const char *zip_ccs_last_error(const zip_ccs *c);
int32_t zip_ccs_set_z(zip_ccs *c, const int64_t *z, size_t z_len, zip_mem_kind kind);
int32_t zip_ccs_eq_table(zip_ccs *c, const uint64_t *r, uint32_t slot);
int32_t zip_ccs_second_table(zip_ccs *c, const uint64_t *r_x, const uint64_t *gamma, uint64_t *v_s_out);
int32_t zip_ccs_eval_matrices(zip_ccs *c, const uint64_t *r_x, const uint64_t *r_y, uint64_t *v_xy_out);
int32_t zip_ccs_table(zip_ccs *c, zip_ccs_table_kind which, uint32_t index, const uint64_t **table_dev);
int32_t zip_ccs_download(zip_ccs *c, zip_ccs_table_kind which, uint32_t index, uint64_t *out);

/* ---- the same tables for MANY small proofs of ONE circuit, each proof in its own field ----------------------------
 * A zip_ccs is one circuit mapped into one field.  In the protocol every proof draws its own field from its public input
 * (draw_random_field), so a caller of the batch family that holds n proofs of one circuit cannot share a zip_ccs between
 * them.  A zip_ccs_batch holds the matrices ONCE, as the integers they are -- CSR as given and the CSC form, built at
 * creation, both with int64 values; no Montgomery copy of them exists, a kernel maps a value into the instance's field
 * where it uses it -- and the tables of up to `capacity` proofs.  Every call below launches a number of kernels that does
 * not depend on n (the instance is a grid dimension): set_z 2, eq_tables 1, second_tables 3, eval_matrices 3.
 *   zip_ccs_batch_create   t 1..7, s 1..16 (the bound of zip_sumcheck_prove_batch, which these tables feed), limbs 2..4,
 *                          capacity 1..65535.  Device memory: capacity * (t + 4) tables of 2^s * limbs * 8 bytes, and
 *                          capacity * 2^s * 8 bytes for the z of a HOST set_z; ZIP_ERR_ALLOC when that cannot be had.
 *                          Errors before a device is looked for, in this order: ZIP_ERR_NULL (matrices, out);
 *                          ZIP_ERR_INVALID_PARAM (t; s outside 1..28; limbs; capacity); the matrices one after the other
 *                          with the rules and codes of zip_ccs_create (ZIP_ERR_NULL an array, ZIP_ERR_SHAPE n_cols != 2^s
 *                          or n_rows > 2^s, ZIP_ERR_INVALID_PARAM a row_ptr that does not start at 0 or decreases,
 *                          ZIP_ERR_SHAPE a column index >= 2^s); ZIP_ERR_UNSUPPORTED (s above 16).
 *   zip_ccs_batch_set_z    n <= capacity proofs: fields[i] (all of the handle's `limbs`, each its own modulus) and z[i]
 *                          of z_len[i] <= 2^s entries, zero-extended (HOST: gathered into one copy; DEVICE: read in place,
 *                          and must stay until the call's work is done -- the next call that waits).  Builds z_i in
 *                          F_{q_i} and the t tables M_k z_i of every instance.  Replaces everything a previous set_z and
 *                          the calls after it left: the handle is reusable with another n and other fields.
 *                          Errors before anything reaches the device, in this order: ZIP_ERR_NULL (b, fields, z, z_len, a
 *                          fields[i], a z[i] with z_len[i] > 0); ZIP_ERR_INVALID_PARAM (n outside 1..capacity; a field
 *                          whose limbs differ from the handle's; a modulus that is even or 1); ZIP_ERR_SHAPE (a z_len[i]
 *                          above 2^s).  A refused call leaves the handle as it was.
 *   zip_ccs_batch_eq_tables      build_eq_x_r(r_i) of every instance into `slot`; r: HOST, n * s * limbs limbs, instance-major
 *   zip_ccs_batch_second_tables  per instance what zip_ccs_second_table does: eq(r_x_i) into slot 1, the second
 *                          sumcheck's table with gamma_i, and V_s (v_s_out: HOST, n * t * limbs limbs, instance-major);
 *                          r_x: n * s * limbs, gamma: n * limbs, both HOST.  One upload, three launches, one copy back,
 *                          one synchronisation.
 *                          Both: ZIP_ERR_NULL for a NULL argument, then ZIP_ERR_INVALID_PARAM for slot > 1 and for a
 *                          handle on which set_z has not run.
 *   zip_ccs_batch_eval_matrices  the verifier's V_xy: per instance i, in fields[i], mle[M_k](r_x_i, r_y_i) for every matrix
 *                          k -- what zip_ccs_eval_matrices gives on a zip_ccs of that field.  r_x, r_y: HOST, n * s * limbs
 *                          each, instance-major; v_xy_out: HOST, n * t * limbs.  The verifier has no z: the call takes
 *                          the fields itself and does not need set_z to have run.  It builds eq(r_x_i) and eq(r_y_i) in
 *                          the two eq slots and sums over the integer CSR, every value mapped into the instance's field
 *                          where it is used.  One upload, three launches whatever n is, one copy back, one
 *                          synchronisation.  It REPLACES what a previous set_z and the calls after it left, as set_z
 *                          does: afterwards the table calls (eq_tables, second_tables, table, download) answer
 *                          ZIP_ERR_INVALID_PARAM until the next set_z.
 *                          Errors before anything reaches the device, in set_z's order: ZIP_ERR_NULL (b, fields, r_x,
 *                          r_y, v_xy_out, a fields[i]); ZIP_ERR_INVALID_PARAM (n outside 1..capacity; a field whose limbs
 *                          differ from the handle's; a modulus that is even or 1).
 *   zip_ccs_batch_table    device pointer of a table of 2^s elements of `instance` (< n), which / index as for
 *                          zip_ccs_table; valid until the next call that rebuilds it or zip_ccs_batch_free.  set_z and
 *                          eq_tables only enqueue their work; this call (and download, and second_tables) waits for what
 *                          is still enqueued, so a pointer it returns may be handed to any stream.
 *                          ZIP_ERR_INVALID_PARAM: set_z has not run, instance >= n, a table that has not been built.
 *   zip_ccs_batch_download the same table copied to the HOST (tests)
 *   zip_ccs_batch_counts   process-wide, monotonic, kept like zip_sumcheck_batch_counts: kernel launches of set_z /
 *                          eq_tables / second_tables / eval_matrices so far, and the instances handed to set_z.  Any
 *                          pointer may be NULL.
 * Calls on one handle are serialised inside the library.  Not part of this: a circuit per instance, s above 16.
 * Additive: the ABI version stays 3. */
typedef struct zip_ccs_batch zip_ccs_batch;
int32_t zip_ccs_batch_create(int32_t device, const zip_sparse_matrix *matrices, uint32_t t, uint32_t s, uint32_t limbs,
                             uint32_t capacity, zip_ccs_batch **out);
void zip_ccs_batch_free(zip_ccs_batch *b); /* NULL is a no-op */
const char *zip_ccs_batch_last_error(const zip_ccs_batch *b);
int32_t zip_ccs_batch_set_z(zip_ccs_batch *b, const zip_field *const *fields, const int64_t *const *z, const size_t *z_len,
                            uint32_t n, zip_mem_kind kind);
int32_t zip_ccs_batch_eq_tables(zip_ccs_batch *b, const uint64_t *r, uint32_t slot);
int32_t zip_ccs_batch_second_tables(zip_ccs_batch *b, const uint64_t *r_x, const uint64_t *gamma, uint64_t *v_s_out);
int32_t zip_ccs_batch_table(zip_ccs_batch *b, uint32_t instance, zip_ccs_table_kind which, uint32_t index,
                            const uint64_t **table_dev);
int32_t zip_ccs_batch_download(zip_ccs_batch *b, uint32_t instance, zip_ccs_table_kind which, uint32_t index, uint64_t *out);
int32_t zip_ccs_batch_eval_matrices(zip_ccs_batch *b, const zip_field *const *fields, uint32_t n, const uint64_t *r_x,
                                    const uint64_t *r_y, uint64_t *v_xy_out);
void zip_ccs_batch_counts(uint64_t *kernel_launches, uint64_t *instances);

/* Diagnostic: FieldMap for Int<4> (src/conversion.rs:86-100) of n arbitrary 256-bit values, as the
 * verifier applies it to column entries.  values: HOST n*4 limbs; out: HOST n*limbs Montgomery limbs. */
int32_t zip_field_map_int256(zip_ctx *ctx, const uint64_t *values, uint32_t n, const zip_field *field, uint64_t *out);
/* The same diagnostic for the two maps of a two-limb ctx (see "Two-limb witnesses" above): value_limbs == 2, the Int<2>
 * witness map (W = FIELD_LIMBS: the signed-modulus reading applies when the modulus has its top bit set, for
 * 2^(64 limbs) - q up to 2^127); value_limbs == 8, the verifier's map of Int<8> column entries (W = 8: |v| mod q of a
 * 512-bit magnitude, then the sign, never the quirk).  values: HOST n * value_limbs limbs; out: HOST n * limbs Montgomery
 * limbs.  Works on any ctx; another value_limbs is ZIP_ERR_UNSUPPORTED.  Additive: the ABI version stays 3. */
int32_t zip_field_map_int(zip_ctx *ctx, const uint64_t *values, uint32_t n, uint32_t value_limbs, const zip_field *field,
                          uint64_t *out);

/* z_mle.map_to_field(config).evaluate(r_y) (src/zinc/prover.rs:317-319, poly_f/mle/dense.rs:35-41),
 * the step ZincProver runs between commit and open: <q0-combination of the rows, q1>.
 * q0_mont: num_rows elements (NULL when num_rows == 1), q1_mont: row_len elements (NULL when
 * row_len == 1).  value_out: HOST, field->limbs Montgomery limbs. */
int32_t zip_mle_eval(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const uint64_t *q0_mont,
                     const uint64_t *q1_mont, const zip_field *field, uint64_t *value_out);
/* The same over the witness a host-side zip_commit left on the device with the commitment: the prover's
 * z_mle.evaluate(r_y) between commit and open (src/zinc/prover.rs:315-320) without a second upload. */
int32_t zip_commitment_mle_eval(zip_commitment *c, const uint64_t *q0_mont, const uint64_t *q1_mont,
                                const zip_field *field, uint64_t *value_out);

/* Row-sharded open: exact sum of n_parts partial results (after an all-gather).
 * uparts: n_parts * row_len * m_limbs u64 or NULL; fparts: n_parts * row_len * limbs u64 or NULL.
 * All pointers DEVICE memory. */
int32_t zip_sum_partials(zip_ctx *ctx, const uint64_t *uparts, const uint64_t *fparts, uint32_t n_parts,
                         const zip_field *field, uint64_t *uprime_out, uint64_t *row_out);

/* ---- several GPUs behind one call ---------------------------------------
 * The reference's callers are one process making one call (src/zinc/prover.rs:305-328): a zip_mctx gives that
 * process all the GPUs of the node.  It owns one row-shard context per entry of `devices` (contiguous blocks of
 * rows; an ordinal may repeat -- several shards on one GPU).  `params->device / row_begin / row_count` are ignored.
 *
 * zip_mctx_commit_open = zip_commit_open on the whole polynomial, the same roots and the same proof bytes:
 *   - every shard commits its rows (hinted persistent kernel) and opens THEM for every column, pipelined as on
 *     one GPU; no shard waits for another;
 *   - the row combinations are computed per shard and added on the lead device (the first of `devices`): the
 *     only exchange besides the roots, 96 bytes per witness column and shard, peer copies -- exact, the sums are
 *     integer / modular;
 *   - proof_out != NULL (HOST): u', then every shard's rows of every column straight from that shard's memory
 *     over its own PCIe link (two pitched copies per shard), then the evaluation row.  Pin the buffer
 *     (zip_host_register) for full link speed;
 *   - proof_out == NULL: the pieces stay on the devices (zip_mctx_shard_openings, zip_mctx_ends).
 *   evals      HOST, the whole witness, or NULL to use the slices zip_mctx_set_witness left on the devices
 *   coeffs, q0_mont, cols   the WHOLE challenge vectors, as for zip_open
 *   roots_out  HOST, num_rows * 32 bytes, may be NULL */
typedef struct zip_mctx zip_mctx;
int32_t zip_mctx_create(const zip_params *params, int32_t n_devices, const int32_t *devices, zip_mctx **out);
void zip_mctx_destroy(zip_mctx *m);
const char *zip_mctx_last_error(const zip_mctx *m);
uint32_t zip_mctx_shards(const zip_mctx *m);
zip_ctx *zip_mctx_shard_ctx(zip_mctx *m, uint32_t shard); /* the shard's context (profiling hooks, geometry); owned by m */
int32_t zip_mctx_set_witness(zip_mctx *m, const int64_t *evals, size_t n_evals);
int32_t zip_mctx_commit_open(zip_mctx *m, const int64_t *evals, const int64_t *coeffs, const uint32_t *cols,
                             uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field, uint8_t *roots_out,
                             uint8_t *proof_out);
/* after zip_mctx_commit_open: shard's openings on ITS device, [n_cols][row_count * 32 B values | row_count records] */
int32_t zip_mctx_shard_openings(zip_mctx *m, uint32_t shard, uint8_t **ptr, size_t *bytes, uint32_t *row_begin,
                                uint32_t *row_count);
/* after zip_mctx_commit_open: u' (u_bytes) followed by the evaluation row (row_bytes) on the lead device */
int32_t zip_mctx_ends(zip_mctx *m, uint8_t **ptr, size_t *u_bytes, size_t *row_bytes);
/* after zip_mctx_commit_open: the commitment -- the roots of ALL rows, [num_rows][32] -- as shard's device holds it.
 * The concatenation of the per-row roots (src/zip/pcs/commit.rs:78-81) is the one exchange of a row-sharded commit:
 * over distinct devices it is one grouped ncclAllGather (ncclBroadcast per owner for uneven blocks) on in-process
 * RCCL communicators (ncclCommInitAll; librccl is bound with dlopen when such a zip_mctx is created), over repeated
 * ordinals -- or when RCCL is missing or refuses -- device copies.  zip_mctx_roots_path: "rccl" | "copies" | "none". */
int32_t zip_mctx_roots(zip_mctx *m, uint32_t shard, uint8_t **ptr);
const char *zip_mctx_roots_path(const zip_mctx *m);

/* ---- standalone Merkle tree --------------------------------------------------------
 * MerkleTree::new (pcs/utils.rs:74-85) over num_trees * 2^depth leaves of leaf_limbs
 * (1..8) limbs each.  layers_out: num_trees * ((2<<depth)-1) * 32 B, root last
 * (the reference pops it into .root).  Buffers HOST or DEVICE per kind. */
int32_t zip_merkle_trees(int32_t device, const uint64_t *leaves, uint32_t leaf_limbs, uint32_t depth,
                         uint32_t num_trees, zip_mem_kind kind, uint8_t *layers_out);

/* ---- measurement hooks ---------------------------------------------------------------
 * With profiling on (1), every kernel launch is bracketed by HIP events on the stream it is launched on; with on = 2
 * only the commit / encode kernel is (it has its stream to itself: between the kernels of ONE stream the events cost
 * every dependent launch about 12 us, which a timed region need not pay).
 * zip_ctx_profile_read synchronises, then fills up to cap entries (kernel name, launch
 * count, total ms) and resets the counters; returns the number of distinct kernels. */
typedef struct {
    const char *name;
    uint32_t launches;
    float total_ms;
} zip_kernel_time;
int32_t zip_ctx_set_profiling(zip_ctx *ctx, int32_t on);
/* Shader clock (MHz) the chip held during the most recent commit kernel launched with profiling on: the kernel's
 * first workgroup stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) at its start and end.  0 if none.
 * bench.py prices the VALU roofline of the commit kernel at this clock. */
int32_t zip_ctx_commit_clock(zip_ctx *ctx, double *mhz_out);
int32_t zip_ctx_profile_read(zip_ctx *ctx, zip_kernel_time *out, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZIP_HIP_H */
