/*
 * zinc_zip_host.h -- C facade of libzinc_zip.so, the C++ mirror (zinc_amd/host/zinc_zip.hpp) of
 * the HOST side of zinc::zip: what stays in the Rust crate in the real integration (Fiat-Shamir
 * transcript, permutation-seed expansion, the eq tensor, parameter checks) driving the HIP
 * library through include/zip_hip.h.  The facade exists so that tests and tools can exercise
 * that layer through ctypes; it adds no behaviour of its own.
 *
 * Return codes: 0 ok; ZINC_ERR_INVALID_PARAM = zip::Error::InvalidPcsParam; ZINC_ERR_PANIC = a
 * place where the reference panics (assert!/expect); ZINC_ERR_DEVICE = HIP library failure.
 * zinc_last_error() returns the message of the calling thread's last failure.
 */
#ifndef ZINC_ZIP_HOST_H
#define ZINC_ZIP_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "zip_hip.h" /* zip_sparse_matrix */
#ifdef __cplusplus
extern "C" {
#endif

#define ZINC_OK 0
#define ZINC_ERR_INVALID_PARAM (-1)
#define ZINC_ERR_PANIC (-2)
#define ZINC_ERR_DEVICE (-3)
#define ZINC_ERR_NULL (-4)

const char *zinc_last_error(void);

/* KeccakTranscript (src/transcript.rs) */
typedef struct zinc_transcript zinc_transcript;
zinc_transcript *zinc_transcript_new(void);
void zinc_transcript_free(zinc_transcript *t);
void zinc_transcript_absorb(zinc_transcript *t, const uint8_t *bytes, size_t len);
uint64_t zinc_transcript_get_u64(zinc_transcript *t);
void zinc_transcript_get_integer_challenges(zinc_transcript *t, size_t n, int64_t *out);
/* get_challenge::<RandomField<limbs>>: Montgomery limbs of the challenge */
int32_t zinc_transcript_get_challenge(zinc_transcript *t, const uint64_t *modulus, uint32_t limbs, uint64_t *out);
/* The Keccak-256 sponge in transit (the fields of zip_keccak_state, zip_hip.h): st = the 25 state words after every
 * full block, buf[0 .. *buflen) = the bytes absorbed since (136 bytes of room; zero beyond *buflen on export).
 * ZINC_ERR_NULL for a NULL argument; import: ZINC_ERR_INVALID_PARAM when buflen >= 136. */
int32_t zinc_transcript_export(const zinc_transcript *t, uint64_t *st, uint8_t *buf, uint32_t *buflen);
int32_t zinc_transcript_import(zinc_transcript *t, const uint64_t *st, const uint8_t *buf, uint32_t buflen);

/* The random field.  zinc_get_prime: prime_gen::get_prime::<RandomField<limbs>> (src/prime_gen.rs:15-28), limbs in
 * {2, 3, 4}: the candidate chain on the host, the primality tests of a batch of candidates in one launch on the device
 * (zip_hip.h); the transcript ends where the reference's loop leaves it.  prime_out: limbs little-endian limbs;
 * candidates_tried_out (may be NULL): the winner's 1-based position in the chain.
 * zinc_draw_random_field: draw_random_field (src/zinc/utils.rs:161-171) with I = Int<1> -- every public input absorbed
 * as its 8 little-endian bytes, then get_prime -> modulus_out, the modulus of the FieldConfig (limbs limbs).
 * ZINC_ERR_INVALID_PARAM for other limb counts, ZINC_ERR_DEVICE when the device call fails (there is no host path).
 * ZINC_ERR_FIELD_CONFIG is ZincError::FieldConfigError: what Verifier::verify returns (src/zinc/verifier.rs:53-57) when
 * the field it draws this way is not the configuration it was handed. */
#define ZINC_ERR_FIELD_CONFIG (-7)
int32_t zinc_get_prime(zinc_transcript *t, uint32_t limbs, int32_t device, uint64_t *prime_out, uint32_t *candidates_tried_out);
int32_t zinc_draw_random_field(const int64_t *public_input, size_t l, zinc_transcript *t, uint32_t limbs, int32_t device,
                               uint64_t *modulus_out);
/* The same for the n members of a batch of proofs, each on its own transcript.  From the line profiles/prime_batch.md sets
 * on (per limb count; ZIP_HIP_PRIME_MIN_BATCH=n, n >= 2, moves it) the draws are ONE zip_get_prime_batch call, chains and
 * tests on the device; below it, for one member and with ZIP_HIP_BATCH=0 they are the loop over zinc_get_prime.  Both give
 * the same bytes and the same errors.
 *   zinc_get_prime_batch              primes_out n * limbs limbs, member-major; candidates_tried_out n entries or NULL
 *   zinc_draw_random_field_batch      member i absorbs public_inputs[i][0 .. lens[i]) first; moduli_out n * limbs limbs
 *   zinc_verifier_check_field_batch   the check of Verifier::verify (:53-57) per member: same_out[i] = 1 when the field
 *                                     drawn at limbs[i] limbs is moduli[4 i ..]; every transcript is left where
 *                                     zinc_verifier_verify_checked's check leaves it.  The members of one limb count are
 *                                     one zinc_draw_random_field_batch. */
int32_t zinc_get_prime_batch(zinc_transcript *const *transcripts, uint32_t n, uint32_t limbs, int32_t device, uint64_t *primes_out,
                             uint32_t *candidates_tried_out);
int32_t zinc_draw_random_field_batch(const int64_t *const *public_inputs, const size_t *lens, zinc_transcript *const *transcripts,
                                     uint32_t n, uint32_t limbs, int32_t device, uint64_t *moduli_out);
int32_t zinc_verifier_check_field_batch(const int64_t *const *public_inputs, const size_t *lens, zinc_transcript *const *transcripts,
                                        uint32_t n, const uint64_t *moduli, const uint32_t *limbs, int32_t device, uint8_t *same_out);

/* field helpers (src/field/config.rs, src/conversion.rs, src/sumcheck/utils.rs) */
int32_t zinc_field_constants(const uint64_t *modulus, uint32_t limbs, uint64_t *r, uint64_t *r2, uint64_t *inv);
int32_t zinc_field_mul(const uint64_t *modulus, uint32_t limbs, const uint64_t *a, const uint64_t *b, uint64_t *out);
int32_t zinc_map_to_field_i64(const uint64_t *modulus, uint32_t limbs, const int64_t *v, size_t n, uint64_t *out);
int32_t zinc_build_eq_x_r(const uint64_t *modulus, uint32_t limbs, const uint64_t *r, uint32_t nvars, uint64_t *out);

/* shuffle_seeded on the identity (src/zip/utils.rs:139-142; rand 0.9 restated, every piece held to a published
 * vector: tests/golden/rand_vectors.json) */
void zinc_shuffle_seeded_perm(uint64_t seed, uint32_t len, uint32_t *perm);
/* known-answer hook: the first n_words little-endian words rand_core::SeedableRng::seed_from_u64 expands `seed` to */
void zinc_kat_seed_from_u64(uint64_t seed, uint32_t *words, uint32_t n_words);

/* RaaCode::new (src/zip/code_raa.rs:35-86).  transcript == NULL uses MockTranscript (seeds 1, 2). */
typedef struct {
    uint32_t row_len, repetition_factor, num_column_opening, num_proximity_testing;
    uint64_t perm_1_seed, perm_2_seed;
} zinc_raa_code;
int32_t zinc_raa_code_new(uint64_t poly_size, zinc_transcript *transcript, zinc_raa_code *out);
/* LinearCodeSpec (src/zip/code.rs:217-242).  The functions without _spec pass DefaultLinearCodeSpec {1000, 2, 1}, and so
 * does a NULL spec.  num_proximity_testing = T in 1 .. 8 reaches the device (zip_ctx_set_proximity_tests, zip_hip.h): the
 * proof carries T proximity rows and the verifier checks every one; another T is ZINC_ERR_INVALID_PARAM from open and
 * verify when the matrix has more than one row (a one-row matrix has no test at all). */
typedef struct {
    uint32_t num_column_opening, repetition_factor, num_proximity_testing;
} zinc_linear_code_spec;
int32_t zinc_raa_code_new_spec(const zinc_linear_code_spec *spec, uint64_t poly_size, zinc_transcript *transcript,
                               zinc_raa_code *out);

/* MultilinearZip::setup / commit / open (src/zip/pcs/structs.rs:79-91, commit.rs:50-119, open_z.rs:22-40) */
typedef struct zinc_zip_params zinc_zip_params;
typedef struct zinc_zip_data zinc_zip_data;
int32_t zinc_zip_setup(uint64_t poly_size, const zinc_raa_code *code, int32_t device, zinc_zip_params **out);
void zinc_zip_params_free(zinc_zip_params *pp);
/* setup() caches device contexts per (device, geometry, seeds); this drops the cache and its device memory */
void zinc_zip_release_cached_contexts(void);
void zinc_zip_params_geometry(const zinc_zip_params *pp, uint32_t *num_vars, uint32_t *num_rows, uint32_t *row_len,
                              uint32_t *codeword_len);
/* roots_out: num_rows * 32 bytes (ignored when with_merkle == 0) */
int32_t zinc_zip_commit(const zinc_zip_params *pp, const int64_t *evals, size_t n_evals, uint32_t poly_num_vars,
                        int32_t with_merkle, uint8_t *roots_out, zinc_zip_data **out);
void zinc_zip_data_free(zinc_zip_data *d);
/* MultilinearZipData is `pub rows` / `pub rows_merkle_trees` in the reference (structs.rs:33-38) and its
 * tests read and mutate both: these move them between the host and the device handle.
 *   rows    num_rows * codeword_len Int<4>  (4 u64 each)
 *   layers  per row (2 * codeword_len - 2) hashes = MerkleTree.layers (pcs/utils.rs:67-71)
 *   roots   per row one hash.  Any pointer may be NULL on download; layers / roots NULL on upload = no trees. */
int32_t zinc_zip_data_download(const zinc_zip_data *d, uint64_t *rows_out, uint8_t *layers_out, uint8_t *roots_out);
int32_t zinc_zip_data_upload(const zinc_zip_params *pp, const uint64_t *rows, const uint8_t *layers,
                             const uint8_t *roots, zinc_zip_data **out);
/* MerkleTree::new(depth, leaves) (pcs/utils.rs:74-85) for n_leaves Int<leaf_limbs>; layers_out: (2 << depth) - 1
 * hashes, the root last.  ZINC_ERR_PANIC when n_leaves != 2^depth ("leaves.len().is_power_of_two()" / depth assert). */
int32_t zinc_merkle_tree_new(uint32_t depth, const uint64_t *leaves, size_t n_leaves, uint32_t leaf_limbs,
                             int32_t device, uint8_t *layers_out);

/* PcsTranscript (src/zip/pcs_transcript.rs) */
typedef struct zinc_pcs_transcript zinc_pcs_transcript;
zinc_pcs_transcript *zinc_pcs_transcript_new(void);
void zinc_pcs_transcript_free(zinc_pcs_transcript *t);
size_t zinc_pcs_transcript_len(const zinc_pcs_transcript *t);
void zinc_pcs_transcript_copy(const zinc_pcs_transcript *t, uint8_t *out); /* into_proof() */
/* the Fiat-Shamir state after the calls so far, as one more u64 squeeze (for equality checks) */
uint64_t zinc_pcs_transcript_probe(const zinc_pcs_transcript *t);

/* point: point_len field elements, Montgomery limbs */
int32_t zinc_zip_open(const zinc_zip_params *pp, const int64_t *evals, size_t n_evals, uint32_t poly_num_vars,
                      const zinc_zip_data *data, const uint64_t *point, size_t point_len, const uint64_t *modulus,
                      uint32_t limbs, zinc_pcs_transcript *transcript);

/* The squeezes of prove_testing_phase / verify_testing and nothing else (open_z.rs:100-120, verify_z.rs:66-90) -- host
 * only, the Fiat-Shamir work a shim does in front of zip_open / zip_verify: per proximity test, in order,
 * get_integer_challenges over num_rows (only if num_rows > 1), then num_column_opening times squeeze_challenge_idx over
 * codeword_len.
 *   coeffs_out  num_proximity_testing * num_rows, test-major (untouched when num_rows == 1; may then be NULL)
 *   cols_out    num_column_opening
 * ZINC_ERR_INVALID_PARAM: num_proximity_testing outside 1 .. 8 with num_rows > 1 (nothing is squeezed). */
int32_t zinc_zip_open_challenges(uint32_t num_rows, uint32_t codeword_len, uint32_t num_column_opening,
                                 uint32_t num_proximity_testing, const uint64_t *modulus, uint32_t limbs,
                                 zinc_pcs_transcript *transcript, int64_t *coeffs_out, uint32_t *cols_out);

/* ---- batch_commit / batch_open (commit.rs:134-142, open_z.rs:43-58) -------------------------
 * polys[i]: n_evals[i] evaluations with poly_num_vars[i] variables.
 * zinc_zip_batch_commit: one device batch, one commit launch for all polynomials (libzip_hip's zip_batch_commit);
 * out[i] is polynomial i's MultilinearZipData (a member of the batch; free each with zinc_zip_data_free, in any order),
 * roots_out n_polys * num_rows * 32 bytes (may be NULL).  Geometries the device batch does not serve, and
 * ZIP_HIP_BATCH=0, take the loop over zinc_zip_commit: same results.
 * zinc_zip_batch_open: points[i] = poly_num_vars[i] field elements (Montgomery limbs).  When datas[] are the members
 * 0 .. n_polys-1 of one batch, in order: all evaluation rows in one device call, the transcript walk below, all proof
 * streams in one device call; otherwise (or with ZIP_HIP_BATCH=0) the loop over zinc_zip_open.  Stream and
 * Fiat-Shamir state end up the same. */
int32_t zinc_zip_batch_commit(const zinc_zip_params *pp, const int64_t *const *polys, const size_t *n_evals,
                              const uint32_t *poly_num_vars, size_t n_polys, uint8_t *roots_out, zinc_zip_data **out);
int32_t zinc_zip_batch_open(const zinc_zip_params *pp, const int64_t *const *polys, const size_t *n_evals,
                            const uint32_t *poly_num_vars, const zinc_zip_data *const *datas, const uint64_t *const *points,
                            size_t n_polys, const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript);
/* The Fiat-Shamir walk of batch_open once the evaluation rows are known -- host only, what a Rust shim runs between
 * zip_batch_open_eval and zip_batch_open.  Per polynomial, in the reference's order: get_integer_challenges over
 * num_rows (only if num_rows > 1, open_z.rs:104), n_cols times squeeze_challenge_idx over codeword_len (:116-120),
 * then the absorption of its evaluation row (pcs_transcript.rs:107-113).
 *   eval_rows   n_polys * row_len * limbs Montgomery limbs (zip_batch_open_eval's output)
 *   coeffs_out  n_polys * num_rows (untouched when num_rows == 1; may then be NULL)
 *   cols_out    n_polys * n_cols */
int32_t zinc_zip_batch_open_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                       const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript,
                                       const uint64_t *eval_rows, size_t n_polys, int64_t *coeffs_out, uint32_t *cols_out);

/* PcsTranscript::from_proof (src/zip/pcs_transcript.rs:28-35): the reading side */
zinc_pcs_transcript *zinc_pcs_transcript_from_proof(const uint8_t *proof, size_t len);
size_t zinc_pcs_transcript_position(const zinc_pcs_transcript *t);

/* MultilinearZip::verify (src/zip/pcs/verify_z.rs:19-38).  roots: num_rows * 32 bytes; eval: Montgomery limbs.
 * ZINC_OK = accepted; ZINC_ERR_INVALID_OPEN = rejected (zinc_last_error() carries the reference's message);
 * ZINC_ERR_PANIC where the reference panics. */
#define ZINC_ERR_INVALID_OPEN (-5)
int32_t zinc_zip_verify(const zinc_zip_params *vp, const uint8_t *roots, const uint64_t *point, size_t point_len,
                        const uint64_t *eval, const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript);

/* MultilinearZip::batch_verify_z (src/zip/pcs/verify_z.rs:40-58): verify per polynomial on ONE transcript.  With at
 * least two polynomials, codewords up to 16384, one proximity test and every point of num_vars coordinates, the host
 * walks the shared transcript over the streams that are all there and makes ONE device call for all of them (zip_hip.h,
 * the batched verifier); otherwise, or with ZIP_HIP_BATCH=0, it is the loop over verify.  Result, error message,
 * transcript and cursor are the loop's either way: after a rejected polynomial i the cursor is at the start of its stream.
 *   roots       n_polys * num_rows * 32 bytes, polynomial-major
 *   points      n_polys pointers to point_lens[i] * limbs Montgomery limbs
 *   evals       n_polys * limbs Montgomery limbs */
int32_t zinc_zip_batch_verify(const zinc_zip_params *vp, const uint8_t *roots, const uint64_t *const *points,
                              const size_t *point_lens, const uint64_t *evals, size_t n_polys, const uint64_t *modulus,
                              uint32_t limbs, zinc_pcs_transcript *transcript);
/* The Fiat-Shamir walk of batch_verify_z -- host only, what a Rust shim runs in front of the one device call.  In
 * `verify` only read_field_elements absorbs (pcs_transcript.rs:91-103), and what it absorbs are the last
 * row_len * 8 * limbs bytes of the stream itself.  Per polynomial, in the reference's order: get_integer_challenges over
 * num_rows (only if num_rows > 1, verify_z.rs:69-72), n_cols times squeeze_challenge_idx over codeword_len (:88-90),
 * then the absorption of the evaluation row at the end of its stream.  The transcript's cursor is not moved.
 *   proofs      n_polys whole streams of stream_len bytes each
 *   coeffs_out  n_polys * num_rows (untouched when num_rows == 1; may then be NULL)
 *   cols_out    n_polys * n_cols */
int32_t zinc_zip_batch_verify_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                         const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript,
                                         const uint8_t *proofs, size_t stream_len, size_t n_polys, int64_t *coeffs_out,
                                         uint32_t *cols_out);

/* z_mle.map_to_field(config).evaluate(r_y) (src/zinc/prover.rs:317-319): out = limbs Montgomery limbs */
int32_t zinc_zip_evaluate(const zinc_zip_params *pp, const int64_t *evals, size_t n_evals, const uint64_t *point,
                          size_t point_len, const uint64_t *modulus, uint32_t limbs, uint64_t *out);

/* ZincProver::commit_z_mle_and_prove_evaluation (src/zinc/prover.rs:305-327) -> ZipProof {z_comm, v, pcs_proof}.
 * transcript: the prover's main KeccakTranscript (two permutation seeds are drawn from it).
 * Call once with proof_out == NULL to learn *proof_len and *n_roots; the result is kept in the handle. */
typedef struct zinc_zip_proof zinc_zip_proof;
int32_t zinc_commit_z_mle_and_prove_evaluation(const int64_t *z_evals, size_t m, const uint64_t *r_y, size_t r_y_len,
                                               zinc_transcript *transcript, const uint64_t *modulus, uint32_t limbs,
                                               int32_t device, zinc_zip_proof **out);
int32_t zinc_commit_z_mle_and_prove_evaluation_spec(const zinc_linear_code_spec *spec, const int64_t *z_evals, size_t m,
                                                    const uint64_t *r_y, size_t r_y_len, zinc_transcript *transcript,
                                                    const uint64_t *modulus, uint32_t limbs, int32_t device,
                                                    zinc_zip_proof **out);
size_t zinc_zip_proof_len(const zinc_zip_proof *p);
size_t zinc_zip_proof_num_roots(const zinc_zip_proof *p);
void zinc_zip_proof_read(const zinc_zip_proof *p, uint8_t *roots_out, uint64_t *v_out, uint8_t *pcs_proof_out);
void zinc_zip_proof_free(zinc_zip_proof *p);

/* MLSumcheck::prove_as_subprotocol with comb_fn = product (src/sumcheck.rs:56-112, zinc/prover.rs:297-302).
 * mles: n_mles host tables of 2^nvars elements (Montgomery limbs).  msgs_out: nvars * (degree+1) * limbs;
 * randomness_out: nvars * limbs. */
int32_t zinc_sumcheck_prove_product(zinc_transcript *transcript, const uint64_t *const *mles, uint32_t n_mles,
                                    uint32_t nvars, uint32_t degree, const uint64_t *modulus, uint32_t limbs,
                                    int32_t device, uint64_t *msgs_out, uint64_t *randomness_out);

/* MLSumcheck::prove_as_subprotocol with sumcheck_polynomial_comb_fn_1 (src/zinc/utils.rs:77-94):
 * (sum_t c[t] * prod_{j in S[t]} vals[j]) * vals[n_mles - 1].  c: n_terms field elements (Montgomery);
 * s_masks[t]: the bits of ccs.S[t] as positions in `mles` (the eq() MLE is the last one). */
int32_t zinc_sumcheck_prove_ccs(zinc_transcript *transcript, const uint64_t *const *mles, uint32_t n_mles,
                                uint32_t nvars, uint32_t degree, uint32_t n_terms, const uint64_t *c,
                                const uint32_t *s_masks, const uint64_t *modulus, uint32_t limbs, int32_t device,
                                uint64_t *msgs_out, uint64_t *randomness_out);

/* n_instances sumchecks of one shape, each with its own transcript, tables and field: on instance i what
 * zinc_sumcheck_prove_product (n_terms == NULL or n_terms[i] == 0) or zinc_sumcheck_prove_ccs (n_terms[i] = 1..8) does, with
 * the same transcript, messages and challenges afterwards.  With nvars 1..16, the same number of limbs in every instance
 * and from 2 / 3 / 6 instances on for nvars up to 12 / 14 / 16, it is ONE device call (zip_sumcheck_prove_batch: one
 * workgroup per instance); with ZIP_HIP_BATCH=0, fewer instances or any other shape it is the loop over those two
 * functions.
 *   mles     n_instances * n_mles host tables, instance-major
 *   c        instance i's coefficients at c + (i * 8 + t) * 4, limbs[i] limbs each; s_masks[i * 8 + t] as in zinc_sumcheck_prove_ccs
 *   moduli   instance i's modulus at moduli + i * 4; limbs[i] its limbs
 *   msgs_out / randomness_out   instance-major, instance i with nvars * (degree + 1) * limbs[i] / nvars * limbs[i] limbs */
int32_t zinc_sumcheck_prove_batch(zinc_transcript *const *transcripts, uint32_t n_instances, const uint64_t *const *mles,
                                  uint32_t n_mles, uint32_t nvars, uint32_t degree, const uint32_t *n_terms, const uint64_t *c,
                                  const uint32_t *s_masks, const uint64_t *moduli, const uint32_t *limbs, int32_t device,
                                  uint64_t *msgs_out, uint64_t *randomness_out);

/* MLSumcheck::prove_as_subprotocol with rand_poly_comb_fn (src/sumcheck/utils.rs:67-78), the workload of
 * benches/sumcheck_benches.rs: sum_p coeffs[p] * prod_{j in masks[p]} vals[j] (bit j of masks[p]: MLE j is a factor;
 * 1..4 factors per product, up to 32 MLEs).  coeffs: n_products field elements (Montgomery). */
int32_t zinc_sumcheck_prove_products(zinc_transcript *transcript, const uint64_t *const *mles, uint32_t n_mles,
                                     uint32_t nvars, uint32_t degree, uint32_t n_products, const uint64_t *coeffs,
                                     const uint32_t *masks, const uint64_t *modulus, uint32_t limbs, int32_t device,
                                     uint64_t *msgs_out, uint64_t *randomness_out);

/* MLSumcheck::verify_as_subprotocol (src/sumcheck.rs:116-160) with check_and_generate_subclaim
 * (src/sumcheck/verifier.rs:97-143), on the host (O(nvars * degree) field operations).  msgs: n_rounds messages of
 * evals_per_round elements each.  point_out: nvars elements, expected_out: one (either may be NULL).
 * ZINC_ERR_SPARTAN: SumCheckFailed / MaxDegreeExceeded / InvalidProofLength (zinc_last_error() says which). */
#define ZINC_ERR_SPARTAN (-6)
int32_t zinc_sumcheck_verify(zinc_transcript *transcript, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum,
                             const uint64_t *msgs, uint32_t n_rounds, uint32_t evals_per_round, const uint64_t *modulus,
                             uint32_t limbs, uint64_t *point_out, uint64_t *expected_out);

/* ZincProver (src/zinc/prover.rs): Prover::prove (:50-88) when with_pcs != 0, else
 * prepare_for_random_field_piop + SpartanProver::prove (:130-161, what benches/spartan_benches.rs times).
 *   constraints   Statement_Z.constraints as CSR (zip_sparse_matrix, include/zip_hip.h), t matrices of
 *                 2^s columns; CCS_Z {m = n = 2^s, s = s_prime = s, d, S = s_masks (bit j: matrix j), c}
 *   public_input / w_ccs   Statement_Z.public_input (l entries), Witness_Z.w_ccs: z = x || 1 || w
 *   outputs       SpartanProof.linearization_sumcheck: s * (d + 2) elements; .second_sumcheck: s * 3;
 *                 .V_s: t; r_y: s elements (all Montgomery limbs); ZipProof through the last argument when with_pcs != 0
 * ZINC_ERR_PANIC where the reference panics (shapes the prover's own assertions reject).
 *
 * zinc_prover_prepare: the circuit's matrices mapped to F_q and resident in HBM (what
 * prepare_for_random_field_piop recomputes per proof, prover.rs:188-189, depends only on circuit and field).
 * Pass the handle as `prepared` (then `constraints` may be NULL) to every proof of that circuit; NULL = build
 * and drop it inside the call, as the reference does. */
typedef struct zinc_prepared_ccs zinc_prepared_ccs;
int32_t zinc_prover_prepare(const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, const uint64_t *modulus,
                            uint32_t limbs, int32_t device, zinc_prepared_ccs **out);
void zinc_prepared_ccs_free(zinc_prepared_ccs *p);
int32_t zinc_prover_prove(const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, uint32_t d, uint32_t q,
                          const uint32_t *s_masks, const int64_t *c, const int64_t *public_input, size_t l,
                          const int64_t *w_ccs, size_t w_len, zinc_transcript *transcript, const uint64_t *modulus,
                          uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared, int32_t with_pcs,
                          uint64_t *msgs1_out, uint64_t *msgs2_out, uint64_t *v_s_out, uint64_t *r_y_out,
                          zinc_zip_proof **zip_proof_out);
int32_t zinc_prover_prove_spec(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                               uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, const int64_t *public_input,
                               size_t l, const int64_t *w_ccs, size_t w_len, zinc_transcript *transcript,
                               const uint64_t *modulus, uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared,
                               int32_t with_pcs, uint64_t *msgs1_out, uint64_t *msgs2_out, uint64_t *v_s_out,
                               uint64_t *r_y_out, zinc_zip_proof **zip_proof_out);

/* zinc_prover_prove for n_instances proofs of ONE circuit, each with its own statement (public_inputs[i] of l[i] entries),
 * witness (w_ccs[i] of w_len[i]), transcript and field (moduli: n_instances * 4 limbs, limbs[i] each): for every instance
 * the same proof, r_y and transcript afterwards as zinc_prover_prove gives.  From 2 instances on (6 above 2^14 rows, 3
 * above 2^12), with s <= 16 and one limb count in all fields, the circuit goes to the device once, as integers
 * (zip_ccs_batch), the tables of all proofs are built with a launch count that does not depend on n_instances, and each of
 * the two sumchecks is one zip_sumcheck_prove_batch; ZIP_HIP_BATCH=0, one instance and every other shape take the loop.
 * Every shape check runs on every instance before any transcript is touched.  with_pcs != 0 adds the PCS step of every
 * proof (zinc_prover_pcs_step_batch below).
 *   spec          NULL: the default LinearCodeSpec
 *   outputs       instance-major, each instance with its own number of limbs, per instance as zinc_prover_prove;
 *                 zip_proofs_out: n_instances handles when with_pcs != 0 (each freed with zinc_zip_proof_free) */
int32_t zinc_prover_prove_batch(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, uint32_t n_instances,
                                const int64_t *const *public_inputs, const size_t *l, const int64_t *const *w_ccs,
                                const size_t *w_len, zinc_transcript *const *transcripts, const uint64_t *moduli,
                                const uint32_t *limbs, int32_t device, int32_t with_pcs, uint64_t *msgs1_out, uint64_t *msgs2_out,
                                uint64_t *v_s_out, uint64_t *r_y_out, zinc_zip_proof **zip_proofs_out);

/* The PCS step of zinc_prover_prove_batch alone (ZincProver::pcs_step_batch; tools/pcs_batch_times.py times it): for
 * n_instances proofs of one circuit of 2^s columns, z[i] (z_len[i] entries, zero-extended), the point r_y[i] (s elements
 * of limbs[i] limbs, instance-major) and the transcript as the Spartan part left them.  Every proof draws the two seeds of
 * its RAA code from its own transcript (prover.rs:313); from the line profiles/pcs_step_batch.md sets on, all proofs are
 * committed by one zip_batch_commit_codes and opened by one zip_batch_open_eval_fields + zip_batch_open_fields.  The loop
 * over the one-proof step runs instead when ZIP_HIP_BATCH=0 is set, there is one instance, the spec asks for more than
 * one proximity test, the codeword is above 8192, the limb counts differ, or n_instances is below that line
 * (ZIP_HIP_PCS_MIN_BATCH=n moves it).  Same ZipProofs, transcripts and errors either way.
 *   zip_proofs_out  n_instances handles (each freed with zinc_zip_proof_free) */
int32_t zinc_prover_pcs_step_batch(const zinc_linear_code_spec *spec, uint32_t s, uint32_t n_instances, const int64_t *const *z,
                                   const size_t *z_len, const uint64_t *r_y, zinc_transcript *const *transcripts,
                                   const uint64_t *moduli, const uint32_t *limbs, int32_t device, zinc_zip_proof **zip_proofs_out);

/* zinc_verifier_verify_spec (with_pcs != 0) for n_instances proofs of ONE circuit, each with its own transcript and field
 * (ZincVerifier::verify_batch): results_out[i] and transcripts[i] afterwards are what the loop over zinc_verifier_verify
 * leaves, for rejected proofs as well, and the call does not stop at the first reject.  From the line
 * profiles/verify_batch.md sets on (2 instances up to 2^10 rows and at 2^14, 16 at 2^12 and 2^16;
 * ZIP_HIP_VERIFY_MIN_BATCH=n moves it to n at every size), with one limb count, s <= 16, one
 * proximity test and codewords up to 16384, the PCS part of all proofs is ONE zip_batch_verify_codes call -- a code and a
 * field per proof, the streams read where they lie -- and the matrix MLEs are ONE zip_ccs_batch_eval_matrices; ZIP_HIP_BATCH=0,
 * one instance and every other shape take the loop.
 *   per-instance arrays, as zinc_prover_prove_batch writes them: msgs1 / msgs2 / v_s instance-major, instance i with
 *   limbs[i] limbs per element; moduli n_instances * 4 limbs; roots[i] (n_roots[i] hashes), v instance-major (limbs[i]
 *   each), pcs_proofs[i] (pcs_proof_lens[i] bytes, read in place)
 *   results_out   n_instances codes: ZINC_OK, ZINC_ERR_SPARTAN (a sumcheck or the final equation failed) or
 *                 ZINC_ERR_INVALID_OPEN (the Zip verifier rejected) -- ZINC_ERR_INVALID_PARAM where verify gives that
 *   messages_out  may be NULL; else n_instances slots of message_cap bytes: the NUL-terminated (cut if need be) message
 *                 of what zinc_verifier_verify would have reported for that proof alone, empty for an accepted one
 * The function result is ZINC_OK when every proof has its outcome; ZINC_ERR_NULL, ZINC_ERR_PANIC (a shape the reference
 * panics on, found on the first member that has it before any device work) and ZINC_ERR_DEVICE are the call's own. */
int32_t zinc_verifier_verify_batch(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                   uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, uint32_t n_instances,
                                   zinc_transcript *const *transcripts, const uint64_t *moduli, const uint32_t *limbs,
                                   int32_t device, const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s,
                                   const uint8_t *const *roots, const size_t *n_roots, const uint64_t *v,
                                   const uint8_t *const *pcs_proofs, const size_t *pcs_proof_lens, int32_t *results_out,
                                   char *messages_out, size_t message_cap);
/* The same with the field check of Verifier::verify first (ZincVerifier::verify_batch_checked):
 * zinc_verifier_check_field_batch over all members, then zinc_verifier_verify_batch over those that passed.  A member
 * that failed the check has ZINC_ERR_FIELD_CONFIG in results_out and its transcript where the check left it. */
int32_t zinc_verifier_verify_batch_checked(const int64_t *const *public_inputs, const size_t *public_input_lens,
                                           const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t,
                                           uint32_t s, uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c,
                                           uint32_t n_instances, zinc_transcript *const *transcripts, const uint64_t *moduli,
                                           const uint32_t *limbs, int32_t device, const uint64_t *msgs1, const uint64_t *msgs2,
                                           const uint64_t *v_s, const uint8_t *const *roots, const size_t *n_roots, const uint64_t *v,
                                           const uint8_t *const *pcs_proofs, const size_t *pcs_proof_lens, int32_t *results_out,
                                           char *messages_out, size_t message_cap);

/* ZincVerifier (src/zinc/verifier.rs): SpartanVerifier::verify (:105-139), and with with_pcs != 0 also
 * verify_pcs_proof (:221-273: RaaCode::new from the transcript, MultilinearZip::verify, the matrix MLEs at
 * (r_x, r_y) on the device, the final equation) -- Verifier::verify without its draw_random_field check (with it:
 * the _checked entry below).
 * Proof fields as zinc_prover_prove returns them.  rx_ry_out: 2 s elements; e_y_out, gamma_out: one element (any
 * may be NULL).  ZINC_ERR_SPARTAN: a sumcheck or the final equation failed; ZINC_ERR_INVALID_OPEN: the Zip
 * verifier rejected; zinc_last_error() has the message. */
int32_t zinc_verifier_verify(const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, uint32_t d, uint32_t q,
                             const uint32_t *s_masks, const int64_t *c, zinc_transcript *transcript, const uint64_t *modulus,
                             uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared, const uint64_t *msgs1,
                             const uint64_t *msgs2, const uint64_t *v_s, int32_t with_pcs, const uint8_t *roots,
                             size_t n_roots, const uint64_t *v, const uint8_t *pcs_proof, size_t pcs_proof_len,
                             uint64_t *rx_ry_out, uint64_t *e_y_out, uint64_t *gamma_out);
/* The same with the check Verifier::verify starts with (src/zinc/verifier.rs:53-57) when check_field != 0: the field
 * is drawn from the l public inputs on `transcript` (zinc_draw_random_field above) and must be `modulus`, else
 * ZINC_ERR_FIELD_CONFIG before any other work; the verification then continues on that transcript.  check_field == 0:
 * zinc_verifier_verify, the public input is not read. */
int32_t zinc_verifier_verify_checked(const int64_t *public_input, size_t l, int32_t check_field,
                                     const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, uint32_t d, uint32_t q,
                                     const uint32_t *s_masks, const int64_t *c, zinc_transcript *transcript,
                                     const uint64_t *modulus, uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared,
                                     const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s, int32_t with_pcs,
                                     const uint8_t *roots, size_t n_roots, const uint64_t *v, const uint8_t *pcs_proof,
                                     size_t pcs_proof_len, uint64_t *rx_ry_out, uint64_t *e_y_out, uint64_t *gamma_out);
/* Both with the verifier's LinearCodeSpec (the spec argument first, everything else as above) */
int32_t zinc_verifier_verify_spec(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                  uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, zinc_transcript *transcript,
                                  const uint64_t *modulus, uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared,
                                  const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s, int32_t with_pcs,
                                  const uint8_t *roots, size_t n_roots, const uint64_t *v, const uint8_t *pcs_proof,
                                  size_t pcs_proof_len, uint64_t *rx_ry_out, uint64_t *e_y_out, uint64_t *gamma_out);
int32_t zinc_verifier_verify_checked_spec(const zinc_linear_code_spec *spec, const int64_t *public_input, size_t l,
                                          int32_t check_field, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                          uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c,
                                          zinc_transcript *transcript, const uint64_t *modulus, uint32_t limbs, int32_t device,
                                          zinc_prepared_ccs *prepared, const uint64_t *msgs1, const uint64_t *msgs2,
                                          const uint64_t *v_s, int32_t with_pcs, const uint8_t *roots, size_t n_roots,
                                          const uint64_t *v, const uint8_t *pcs_proof, size_t pcs_proof_len, uint64_t *rx_ry_out,
                                          uint64_t *e_y_out, uint64_t *gamma_out);

#ifdef __cplusplus
}
#endif
#endif
