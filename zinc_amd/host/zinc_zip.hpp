// zinc_zip.hpp -- C++ mirror of the host side of zinc::zip for the commit/open path.
//
// In the real integration this layer is the Rust crate itself: `ZincProver` keeps calling
// `MultilinearZip::{setup, commit, open}` and a shim inside those functions calls the C ABI of
// libzip_hip.so.  This image has no Rust toolchain, so the same host logic is
// restated here in C++ with the reference's names, argument meaning and error behaviour:
//
//   zinc::KeccakTranscript          src/transcript.rs
//   zinc::FieldConfig / FieldElem   src/field/config.rs, src/field.rs (RandomField::Initialized)
//   zinc::map_to_field              src/conversion.rs:86-100, src/field.rs:536-568
//   zinc::build_eq_x_r              src/sumcheck/utils.rs:117-177
//   zinc::zip::shuffle_seeded       src/zip/utils.rs:139-142 (rand 0.9 restated, PARITY UNPINNED)
//   zinc::zip::RaaCode              src/zip/code_raa.rs:16-140
//   zinc::zip::PcsTranscript        src/zip/pcs_transcript.rs
//   zinc::zip::MultilinearZip       src/zip/pcs/structs.rs, commit.rs, open_z.rs
//
// Everything sequential and tiny stays here on the host (Fiat-Shamir, permutation expansion,
// the eq tensor, absorbing the evaluation row); every O(n) loop is a call into the HIP library.
// There is no CPU implementation of commit/open in this layer.
#pragma once
#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <utility>
#include <stdexcept>
#include <string>
#include <vector>

#include "zip_hip.h"

namespace zinc {

// Byte vector whose resize() leaves new bytes uninitialised: the proof stream of a 2^24 witness is
// 1.74 GiB that the device overwrites entirely, and value-initialising it first costs a full extra
// pass over fresh pages on the host.
template <class T>
struct default_init_allocator {
    using value_type = T;
    template <class U> struct rebind { using other = default_init_allocator<U>; };
    default_init_allocator() = default;
    template <class U> default_init_allocator(const default_init_allocator<U> &) {}
    // Large blocks are 2 MiB aligned and marked for transparent huge pages: first-touch faults
    // (the kernel zero-filling fresh pages) are what bounds the arrival of a proof in host memory.
    T *allocate(size_t n) { return static_cast<T *>(big_alloc(n * sizeof(T))); }
    void deallocate(T *p, size_t n) { byte_stream_free_dispatch(p, n * sizeof(T)); }
    static void byte_stream_free_dispatch(void *p, size_t bytes);
    template <class U> void construct(U *p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void *>(p)) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
    bool operator==(const default_init_allocator &) const { return true; }
    bool operator!=(const default_init_allocator &) const { return false; }
    static void *big_alloc(size_t bytes);
};
void *byte_stream_alloc(size_t bytes);
void byte_stream_free(void *p, size_t bytes);   // big blocks go to a small process-wide cache
void byte_stream_release_cache();               // returns that cache to the system
template <class T>
void *default_init_allocator<T>::big_alloc(size_t bytes) { return byte_stream_alloc(bytes); }
template <class T>
void default_init_allocator<T>::byte_stream_free_dispatch(void *p, size_t bytes) { byte_stream_free(p, bytes); }
using ByteStream = std::vector<uint8_t, default_init_allocator<uint8_t>>;
using IntVec = std::vector<int64_t, default_init_allocator<int64_t>>;  // witness-sized: huge pages, no zero fill

constexpr uint32_t kMaxLimbs = 8;
using Limbs = std::array<uint64_t, kMaxLimbs>;  // little-endian, unused limbs zero

// ---------------------------------------------------------------------------- errors
// zip::Error (src/zip.rs:29-41).  Where the reference panics, this layer throws std::logic_error.
struct ZipError : std::runtime_error {
    enum Kind { InvalidPcsParam, InvalidPcsOpen, Transcript, Device } kind;
    ZipError(Kind k, const std::string &what) : std::runtime_error(what), kind(k) {}
};

// ---------------------------------------------------------------------------- Keccak-256
class Keccak256 {
  public:
    Keccak256() { std::memset(st_, 0, sizeof st_); }
    void update(const uint8_t *data, size_t len);
    void update(std::initializer_list<uint8_t> bytes) { update(bytes.begin(), bytes.size()); }
    std::array<uint8_t, 32> finalize() const;  // of a clone: the hasher keeps absorbing
    // the sponge in transit (zip_keccak_state): the state after every full block, and the bytes absorbed since
    void export_state(zip_keccak_state *out) const;
    void import_state(const zip_keccak_state &in);  // throws std::logic_error when buflen >= 136

  private:
    static void permute(uint64_t st[25]);
    void absorb_block(const uint8_t *blk);
    uint64_t st_[25];
    uint8_t buf_[136];
    uint32_t buflen_ = 0;
};

// ---------------------------------------------------------------------------- field
// FieldConfig (src/field/config.rs:30-50): Montgomery constants for an odd modulus of `limbs` limbs.
struct FieldConfig {
    uint32_t limbs = 0;
    Limbs modulus{}, r{}, r2{};
    uint64_t inv = 0;
    bool modulus_has_spare_bit = false;

    static FieldConfig make(const uint64_t *modulus, uint32_t limbs);  // Config::new, config.rs:174-186
    void mul_assign(Limbs &a, const Limbs &b) const;                   // config.rs:163-170
    void add_assign(Limbs &a, const Limbs &b) const;                   // config.rs:53-58
    void sub_assign(Limbs &a, const Limbs &b) const;                   // config.rs:60-66
    void neg(Limbs &a) const;                                          // arithmetic.rs:130-149
    Limbs inverse(const Limbs &a) const;                               // a^(q-2): the unique inverse (q prime)
    uint32_t num_bits() const;
    zip_field to_abi() const;

  private:
    void reduce_modulus(Limbs &a, bool carry) const;  // config.rs:68-76
};

// FieldMap for i64 / u128 (conversion.rs:9-46,86-100; field.rs:536-568): Montgomery form.
Limbs map_to_field(const FieldConfig &f, int64_t v);
Limbs map_to_field_u128(const FieldConfig &f, uint64_t lo, uint64_t hi);
// build_eq_x_r_vec (sumcheck/utils.rs:117-177); r: nvars field elements, result 2^nvars.
std::vector<Limbs> build_eq_x_r(const FieldConfig &f, const Limbs *r, uint32_t nvars);

// ---------------------------------------------------------------------------- Fiat-Shamir
class KeccakTranscript {
  public:
    void absorb(const uint8_t *v, size_t len) { hasher_.update(v, len); }
    std::vector<uint8_t> get_random_bytes(size_t length);          // transcript.rs:40-55
    void absorb_random_field(const FieldConfig &f, const Limbs &v);  // field.rs:360-378 (Initialized)
    Limbs get_challenge(const FieldConfig &f);                     // transcript.rs:88-133
    void get_integer_challenge(uint32_t n_limbs, uint64_t *out);   // transcript.rs:142-155
    std::vector<int64_t> get_integer_challenges_i64(size_t n);     // transcript.rs:158-160 with I = Int<1>
    uint64_t get_u64() {                                           // ZipTranscript::get_u64, transcript.rs:183-185
        uint64_t w;
        get_integer_challenge(1, &w);
        return w;
    }
    // zip_sumcheck_prove borrows the transcript for one sumcheck: hand the sponge over, take it back
    void export_state(zip_keccak_state *out) const { hasher_.export_state(out); }
    void import_state(const zip_keccak_state &in) { hasher_.import_state(in); }

  private:
    Keccak256 hasher_;
};

// ---------------------------------------------------------------------------- the random field
// prime_gen::get_prime (src/prime_gen.rs:15-28) with F = RandomField<limbs>, limbs in {2, 3, 4}: candidates are hashed
// out of the transcript (hash_int, :8-13) until MillerRabin::test_base_two accepts one.  The chain is hashed on the
// host, in batches ahead of the tests; the tests of a batch are one launch on the device (zip_get_prime, zip_hip.h).
// The transcript ends where the reference's loop leaves it.  Returns the prime's words; candidates_tried (may be
// null): the winner's 1-based position.  Throws ZipError{InvalidPcsParam} for other limb counts, ZipError{Device} when
// the device call fails -- there is no host path for the tests.
namespace prime_gen {
Limbs get_prime(KeccakTranscript &transcript, uint32_t limbs, int device = 0, uint32_t *candidates_tried = nullptr);
// get_prime on every transcript of a batch (the fields of many small proofs): ONE zip_get_prime_batch call, chains and
// tests on the device, from min_prime_batch(limbs) members on (zinc_zip.cpp, from profiles/prime_batch.md;
// ZIP_HIP_PRIME_MIN_BATCH=n, n >= 2, read per call, moves the line).  Below it, with ZIP_HIP_BATCH=0 and for one
// member: the loop over get_prime.  Both paths give the same primes, positions, transcripts and errors.
// candidates_tried (may be null): one entry per member.
std::vector<Limbs> get_prime_batch(const std::vector<KeccakTranscript *> &transcripts, uint32_t limbs, int device = 0,
                                   uint32_t *candidates_tried = nullptr);
}
// draw_random_field (src/zinc/utils.rs:161-171) with I = Int<1>: every public input is absorbed as its 8 little-endian
// bytes (:165-167), then FieldConfig::new(get_prime(transcript)).
FieldConfig draw_random_field(const int64_t *public_input, size_t l, KeccakTranscript &transcript, uint32_t limbs,
                              int device = 0);
// draw_random_field for every member of a batch: member i absorbs public_inputs[i][0 .. lens[i]) on transcripts[i] as
// draw_random_field does, then ONE prime_gen::get_prime_batch over all of them.
std::vector<FieldConfig> draw_random_field_batch(const std::vector<const int64_t *> &public_inputs, const std::vector<size_t> &lens,
                                                 const std::vector<KeccakTranscript *> &transcripts, uint32_t limbs,
                                                 int device = 0);
// ZincError::FieldConfigError (src/zinc/errors.rs): the field the verifier draws is not the one it was handed
struct FieldConfigError : std::runtime_error {
    explicit FieldConfigError(const std::string &what) : std::runtime_error(what) {}
};

namespace zip {

// shuffle_seeded applied to the identity: shuffle_seeded(x, seed)[j] == x[perm[j]].
std::vector<uint32_t> shuffle_seeded_perm(uint64_t seed, uint32_t len);
// the seed bytes rand_core's seed_from_u64 expands `seed` to, as little-endian words (known-answer hook)
void kat_seed_from_u64(uint64_t seed, uint32_t *words, uint32_t n_words);

// LinearCodeSpec / DefaultLinearCodeSpec (src/zip/code.rs:217-242)
struct LinearCodeSpec {
    uint32_t num_column_opening = 1000;
    uint32_t repetition_factor = 2;
    uint32_t num_proximity_testing = 1;
};

// A source of permutation seeds: ZipTranscript::get_u64 (structs.rs:67-76).
struct SeedSource {
    virtual ~SeedSource() = default;
    virtual uint64_t get_u64() = 0;
};
struct KeccakSeedSource : SeedSource {
    explicit KeccakSeedSource(KeccakTranscript &t) : t_(t) {}
    uint64_t get_u64() override { return t_.get_u64(); }
    KeccakTranscript &t_;
};
struct MockTranscript : SeedSource {  // src/zip/pcs/tests.rs:24-37
    int64_t counter = 0;
    uint64_t get_u64() override { return (uint64_t)++counter; }
};

// RaaCode (src/zip/code_raa.rs:16-86), ZipTypes fixed to INT_LIMBS = 1 (N = Int<1>, K = Int<4>, M = Int<8>).
struct RaaCode {
    uint32_t row_len = 0, repetition_factor = 0, num_column_opening = 0, num_proximity_testing = 0;
    uint64_t perm_1_seed = 0, perm_2_seed = 0;

    // RaaCode::new: geometry, width assertion (throws std::logic_error like the reference's assert!),
    // then two seeds from the transcript.
    static RaaCode make(const LinearCodeSpec &spec, uint64_t poly_size, SeedSource &transcript);
    uint32_t codeword_len() const { return row_len * repetition_factor; }
};

// PcsTranscript (src/zip/pcs_transcript.rs:19-48): Fiat-Shamir state + the proof byte stream.
struct PcsTranscript {
    KeccakTranscript fs_transcript;
    ByteStream stream;
    size_t read_pos = 0;  // Cursor position of the reading side (PcsTranscript::from_proof, :28-35)

    const uint8_t *borrowed = nullptr;  // reading side over the caller's bytes (from_proof_view): nothing is copied
    size_t borrowed_len = 0;

    static PcsTranscript from_proof(const uint8_t *proof, size_t len) {
        PcsTranscript t;
        t.stream.assign(proof, proof + len);
        return t;
    }
    // the same without taking a copy of a proof that may be GiBs; the bytes must outlive the transcript
    static PcsTranscript from_proof_view(const uint8_t *proof, size_t len) {
        PcsTranscript t;
        t.borrowed = proof;
        t.borrowed_len = len;
        return t;
    }
    const uint8_t *read_data() const { return borrowed ? borrowed : stream.data(); }
    size_t read_size() const { return borrowed ? borrowed_len : stream.size(); }

    void write_field_elements(const FieldConfig &f, const Limbs *elems, size_t n);  // :76-113
    void append(const uint8_t *bytes, size_t n) { stream.insert(stream.end(), bytes, bytes + n); }
    size_t squeeze_challenge_idx(const FieldConfig &f, size_t cap);                // :174-179
    ByteStream into_proof() { return std::move(stream); }
};

// MultilinearZipParams (structs.rs:13-18) + the device context that serves this geometry.
struct MultilinearZipParams {
    uint32_t num_vars = 0, num_rows = 0;
    RaaCode linear_code;
    std::vector<uint32_t> perm1, perm2;
    std::shared_ptr<zip_ctx> ctx;  // created by setup()
};

// MultilinearZipData (structs.rs:33-38): rows + Merkle trees, device resident behind the handle.
struct MultilinearZipData {
    std::shared_ptr<zip_ctx> ctx;             // keeps the device context alive (declared first: destroyed last)
    std::shared_ptr<zip_commitment> handle;
    // what batch_commit returns: `handle` is member `batch_index` of `batch` (zip_batch_member) and every member shares
    // the reference to it; batch_open recognises the members 0 .. B-1 of one batch by these
    std::shared_ptr<zip_batch> batch;
    uint32_t batch_index = 0;
};
// one polynomial of a batch call: DenseMultilinearExtension {evaluations, num_vars}
struct PolyRef {
    const int64_t *evals = nullptr;
    size_t n_evals = 0;
    uint32_t num_vars = 0;
};
// MultilinearZipCommitment (structs.rs:42-45)
struct MultilinearZipCommitment {
    std::vector<std::array<uint8_t, 32>> roots;
};

struct MultilinearZip {
    // structs.rs:79-91.  Device contexts (streams, pinned staging, the device memory pool, the
    // uploaded permutation tables) are cached per (device, geometry, seeds): ZincProver calls setup
    // for every proof, and a cold context costs more than a 2^20 commit.  The most recent few stay
    // alive; release_cached_contexts() drops them (and their device memory).
    static MultilinearZipParams setup(uint64_t poly_size, const RaaCode &code, int device = 0);
    static void release_cached_contexts();
    // commit.rs:50-87.  poly_num_vars is DenseMultilinearExtension::num_vars of the caller's polynomial.
    static std::pair<MultilinearZipData, MultilinearZipCommitment> commit(const MultilinearZipParams &pp,
                                                                          const int64_t *evals, size_t n_evals,
                                                                          uint32_t poly_num_vars);
    // commit.rs:104-119
    static MultilinearZipData commit_no_merkle(const MultilinearZipParams &pp, const int64_t *evals, size_t n_evals,
                                               uint32_t poly_num_vars);
    // The squeezes of prove_testing_phase / verify_testing and nothing else (open_z.rs:100-120, verify_z.rs:66-90): per
    // proximity test, in order, get_integer_challenges(num_rows) -- only if num_rows > 1: a one-row matrix has no test
    // whatever the spec says --, then num_column_opening times squeeze_challenge_idx(codeword_len).  Nothing between the
    // first squeeze and the evaluation row absorbs, so this is all the Fiat-Shamir work in front of the device call.
    // Returns (coeffs [tests][num_rows], cols).  Throws ZipError{InvalidPcsParam} for num_proximity_testing outside
    // 1 .. 8 when num_rows > 1 (what the device path serves).  Host only; open and verify call it.
    static std::pair<std::vector<int64_t>, std::vector<uint32_t>> open_challenges(uint32_t num_rows, uint32_t codeword_len,
                                                                                 uint32_t num_column_opening,
                                                                                 uint32_t num_proximity_testing,
                                                                                 const FieldConfig &field,
                                                                                 PcsTranscript &transcript);
    // open_z.rs:22-40.  point: num_vars field elements in Montgomery form.  A spec with num_proximity_testing = T > 1
    // writes T proximity rows (the ctx of setup() is set to T: zip_ctx_set_proximity_tests).
    static void open(const MultilinearZipParams &pp, const int64_t *evals, size_t n_evals, uint32_t poly_num_vars,
                     const MultilinearZipData &commit_data, const Limbs *point, size_t point_len,
                     const FieldConfig &field, PcsTranscript &transcript);
    // commit.rs:134-142.  ONE zip_batch for all polynomials (one commit launch); the returned data are its members.
    // Geometries a batch does not serve (codewords above 16384) and ZIP_HIP_BATCH=0 fall back to the loop over commit.
    static std::vector<std::pair<MultilinearZipData, MultilinearZipCommitment>> batch_commit(const MultilinearZipParams &pp,
                                                                                           const PolyRef *polys, size_t n_polys);
    // open_z.rs:43-58.  points[i]: polys[i].num_vars field elements.  When `datas` are the members 0 .. B-1 of one
    // batch, in order, the whole loop is three device steps (all evaluation rows, the transcript walk of
    // batch_open_challenges on the host, all proof streams in one call); otherwise, or with ZIP_HIP_BATCH=0, the
    // loop over open.  The transcript and the stream end up the same either way.
    static void batch_open(const MultilinearZipParams &pp, const PolyRef *polys, const MultilinearZipData *const *datas,
                           const Limbs *const *points, size_t n_polys, const FieldConfig &field, PcsTranscript &transcript);
    // The Fiat-Shamir walk of batch_open with the evaluation rows already known (in `open` only write_field_elements
    // absorbs, pcs_transcript.rs:107-113, and the row does not depend on anything squeezed before it): per polynomial,
    // in the reference's order, get_integer_challenges(num_rows) if num_rows > 1 (open_z.rs:104), n_cols times
    // squeeze_challenge_idx(codeword_len) (:116-120), then the absorption of its row_len evaluation-row elements.
    // eval_rows: [n_polys][row_len][limbs] Montgomery limbs; coeffs_out: [n_polys][num_rows] (untouched when
    // num_rows == 1); cols_out: [n_polys][n_cols].  Host only.
    static void batch_open_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                      const FieldConfig &field, PcsTranscript &transcript, const uint64_t *eval_rows,
                                      size_t n_polys, int64_t *coeffs_out, uint32_t *cols_out);
    // verify_z.rs:19-38.  Throws ZipError{InvalidPcsOpen} with the reference's message when a check
    // fails ("Proximity failure", "Evaluation consistency failure"), std::logic_error where the
    // reference panics (encode_wide overflow).  Merkle paths are checked (zip_hip.h, zip_verify).
    static void verify(const MultilinearZipParams &vp, const MultilinearZipCommitment &comm, const Limbs *point,
                       size_t point_len, const Limbs &eval, PcsTranscript &transcript, const FieldConfig &field);
    // verify_z.rs:40-58: verify per polynomial on ONE transcript.  With at least two polynomials, codewords up to 16384,
    // one proximity test, every point of num_vars coordinates and every commitment of num_rows roots (and ZIP_HIP_BATCH
    // not 0) the whole loop is the host walk of batch_verify_challenges over the streams that are all there and ONE
    // zip_batch_verify call; otherwise the loop over verify, which raises the reference's own errors.  Either way the
    // transcript, the cursor and the exception are what the loop leaves: after a rejected polynomial i, polynomials
    // 0 .. i-1 absorbed, the squeezes of polynomial i drawn, read_pos at the start of stream i.
    static void batch_verify_z(const MultilinearZipParams &vp, const MultilinearZipCommitment *const *comms,
                               const Limbs *const *points, const size_t *point_lens, const Limbs *evals, size_t n_polys,
                               PcsTranscript &transcript, const FieldConfig &field);
    // The Fiat-Shamir walk of batch_verify_z over n_polys whole streams of stream_len bytes at `proofs`: in `verify` only
    // read_field_elements absorbs (pcs_transcript.rs:91-103), and what it absorbs are the last row_len * 8 * limbs bytes
    // of the stream itself.  Per polynomial: get_integer_challenges(num_rows) if num_rows > 1, n_cols times
    // squeeze_challenge_idx(codeword_len), then the absorption of the evaluation row read from the stream.  read_pos is
    // not touched.  coeffs_out: [n_polys][num_rows] (untouched when num_rows == 1); cols_out: [n_polys][n_cols].  Host only.
    static void batch_verify_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                        const FieldConfig &field, PcsTranscript &transcript, const uint8_t *proofs,
                                        size_t stream_len, size_t n_polys, int64_t *coeffs_out, uint32_t *cols_out);
    // z_mle.map_to_field(config).evaluate(r_y, config) (zinc/prover.rs:317-319; poly_f/mle/dense.rs:35-41):
    // nullopt-like failure (wrong point length) throws ZipError{InvalidPcsParam}.
    static Limbs evaluate(const MultilinearZipParams &pp, const int64_t *evals, size_t n_evals, const Limbs *point,
                          size_t point_len, const FieldConfig &field);
};

// ZipProof (src/zinc/structs.rs:26-30) and the PCS step of the prover,
// ZincProver::commit_z_mle_and_prove_evaluation (src/zinc/prover.rs:305-327): code from the main
// transcript, setup, commit, v = z_mle(r_y), open on a FRESH PcsTranscript.
struct ZipProof {
    MultilinearZipCommitment z_comm;
    Limbs v{};
    ByteStream pcs_proof;
};
ZipProof commit_z_mle_and_prove_evaluation(const LinearCodeSpec &lc_spec, const int64_t *z_evals, size_t m,
                                           const Limbs *r_y, size_t r_y_len, KeccakTranscript &transcript,
                                           const FieldConfig &config, int device = 0);
// The PCS step of B proofs whose z fill ONE geometry (m evaluations each) in one commit and one open: each proof's code
// comes from its own main transcript, so the members share the geometry and nothing else -- zip_batch_commit_codes takes
// the permutations per member, zip_batch_open_eval_fields / zip_batch_open_each the fields.  Per proof the result, the
// main transcript afterwards and whatever is thrown are those of commit_z_mle_and_prove_evaluation called member after
// member.  The caller sees to what the device batch serves: one proximity test, codeword_len <= 8192, one limb count.
struct PcsBatchMember {
    const int64_t *z_evals = nullptr;  // m evaluations
    const Limbs *r_y = nullptr;
    size_t r_y_len = 0;
    KeccakTranscript *transcript = nullptr;
    const FieldConfig *config = nullptr;
};
std::vector<ZipProof> commit_z_mle_and_prove_evaluation_batch(const LinearCodeSpec &lc_spec, size_t m,
                                                              const std::vector<PcsBatchMember> &members, int device = 0);

}  // namespace zip

// ---------------------------------------------------------------------------- sumcheck
// MLSumcheck::prove_as_subprotocol (src/sumcheck.rs:56-112) for comb_fn = product of the MLE values
// (ZincProver::sumcheck_2, src/zinc/prover.rs:297-302): the rounds run on the device
// (zip_sumcheck_round), the transcript stays here.
namespace sumcheck {
struct SumcheckProof {                       // SumcheckProof(Vec<ProverMsg>) (src/sumcheck.rs:24-26)
    std::vector<std::vector<Limbs>> msgs;    // per round: evaluations at 0..degree
};
struct ProverOutput {
    SumcheckProof proof;
    std::vector<Limbs> randomness;           // ProverState.randomness
};
// mles[k]: 2^nvars field elements as flat little-endian Montgomery limbs (config.limbs each), host memory.
ProverOutput prove_as_subprotocol_product(KeccakTranscript &transcript, const std::vector<const uint64_t *> &mles,
                                          uint32_t nvars, uint32_t degree, const FieldConfig &config, int device = 0);
// The same with sumcheck_polynomial_comb_fn_1 (src/zinc/utils.rs:77-94; ZincProver::sumcheck_1,
// zinc/prover.rs:241-259): (sum_t c[t] * prod_{j in S[t]} vals[j]) * vals.last().  c: ccs.c (Montgomery),
// S: ccs.S as positions in `mles`, whose last entry is the eq() MLE (prepare_lin_sumcheck_polynomial).
ProverOutput prove_as_subprotocol_ccs(KeccakTranscript &transcript, const std::vector<const uint64_t *> &mles,
                                      uint32_t nvars, uint32_t degree, const std::vector<Limbs> &c,
                                      const std::vector<std::vector<uint32_t>> &S, const FieldConfig &config,
                                      int device = 0);
// The same for a sum of products, comb(vals) = sum_p coeff_p * prod_{j in indices_p} vals[j] (rand_poly_comb_fn,
// src/sumcheck/utils.rs:67-78; the workload of benches/sumcheck_benches.rs: 7 products of 2-4 fresh MLEs), at most
// 4 multiplicands per product.  Up to 32 MLEs and 8 products with no multiplicand twice in a product: ONE device
// prover for the whole sum (zip_sumcheck_init_products; ZIP_HIP_SUMCHECK_FUSED=0 turns it off, and with
// ZIP_HIP_SUMCHECK_ONECALL=1 it is one zip_sumcheck_prove call).  Otherwise each product runs as its own device
// prover, all of them enqueued before any is collected, and the round message is the field sum of theirs.  Same
// bytes and transcript either way.
ProverOutput prove_as_subprotocol_products(KeccakTranscript &transcript, const std::vector<const uint64_t *> &mles,
                                           uint32_t nvars, uint32_t degree,
                                           const std::vector<std::pair<Limbs, std::vector<uint32_t>>> &products,
                                           const FieldConfig &config, int device = 0);
// MANY small sumchecks of one shape, each with its own transcript, tables and field: prove_as_subprotocol_product (ccs
// false) or prove_as_subprotocol_ccs (ccs true: c and S as there) on every instance.  Up to 16 variables, with the same
// number of tables and limbs in every instance and from 2 / 3 / 6 instances on up to 2^12 / 2^14 / 2^16 points
// (profiles/sumcheck_batch.md), it is ONE zip_sumcheck_prove_batch call (one workgroup per instance, the sponges on the
// device); ZIP_HIP_BATCH=0, fewer instances and every shape the batch does not serve take the loop.  Transcripts,
// messages and challenges are the same either way.
struct BatchInstance {
    KeccakTranscript *transcript = nullptr;
    std::vector<const uint64_t *> mles;  // host tables, as above
    FieldConfig config;
    bool ccs = false;
    std::vector<Limbs> c;
    std::vector<std::vector<uint32_t>> S;
};
std::vector<ProverOutput> prove_as_subprotocol_batch(std::vector<BatchInstance> &instances, uint32_t nvars, uint32_t degree,
                                                     int device = 0);
// SumCheckError / SpartanError (src/sumcheck.rs:28-38, src/zinc/errors.rs): what the verifier returns as Err
struct SpartanError : std::runtime_error {
    enum Kind { SumCheckFailed, InvalidProofLength, MaxDegreeExceeded, PcsVerification } kind;
    SpartanError(Kind k, const std::string &what) : std::runtime_error(what), kind(k) {}
};
struct SubClaim {  // src/sumcheck/verifier.rs:33-40
    std::vector<Limbs> point;
    Limbs expected_evaluation{};
};
// interpolate_uni_poly (src/sumcheck/verifier.rs:161-303)
Limbs interpolate_uni_poly(const FieldConfig &config, const std::vector<Limbs> &p_i, const Limbs &x);
// MLSumcheck::verify_as_subprotocol (src/sumcheck.rs:116-160); throws SpartanError
SubClaim verify_as_subprotocol(KeccakTranscript &transcript, uint32_t num_vars, uint32_t degree, const Limbs &claimed_sum,
                               const SumcheckProof &proof, const FieldConfig &config);
}  // namespace sumcheck
using sumcheck::SpartanError;

// ---------------------------------------------------------------------------- CCS (src/ccs/ccs_z.rs)
namespace ccs {
// SparseMatrix<Int<1>> (src/sparse_matrix.rs:12-17) as CSR; `coeffs` may hold fewer than n_rows rows
// (pad_rows only bumps n_rows, :104-108): from_coeffs() leaves the missing rows empty.
struct SparseMatrix {
    uint32_t n_rows = 0, n_cols = 0;
    std::vector<uint32_t> row_ptr{0}, col_idx;
    std::vector<int64_t> values;
    static SparseMatrix from_coeffs(uint32_t n_rows, uint32_t n_cols,
                                    const std::vector<std::vector<std::pair<int64_t, uint32_t>>> &coeffs);
    zip_sparse_matrix to_abi() const { return {n_rows, n_cols, row_ptr.data(), col_idx.data(), values.data()}; }
};
struct CCS_Z {  // src/ccs/ccs_z.rs:30-52
    size_t m = 0, n = 0, l = 0, t = 0, q = 0, d = 0, s = 0, s_prime = 0;
    std::vector<std::vector<size_t>> S;
    std::vector<int64_t> c;
};
struct Statement_Z {  // :155-158
    std::vector<SparseMatrix> constraints;
    std::vector<int64_t> public_input;
    std::vector<int64_t> get_z_vector(const std::vector<int64_t> &w) const;  // x || 1 || w, :219-229
};
struct Witness_Z {  // :178-182
    std::vector<int64_t> w_ccs;
};
}  // namespace ccs

// ---------------------------------------------------------------------------- ZincProver (src/zinc/prover.rs)
// SpartanProof / ZincProof (src/zinc/structs.rs:13-30)
struct SpartanProof {
    sumcheck::SumcheckProof linearization_sumcheck, second_sumcheck;
    std::vector<Limbs> V_s;
};
struct ZincProof {
    SpartanProof spartan_proof;
    zip::ZipProof zip_proof;
};
// The transcript, the challenges and the proof objects live here; every O(n) loop runs on the device
// (zip_ccs_* for the matrix / eq tables, zip_sumcheck_* for the rounds, the Zip PCS for the last step).
// Shape: m == n == 2^s == 2^s_prime, every c[i] != 0, the S[i] concatenated == 0..t-1 -- what the
// reference's own code supports (compute_eval_table_sparse asserts rx.len() == ccs.n, ccs_f.rs:133;
// sumcheck_polynomial_comb_fn_1 indexes the MLE list by matrix number, zinc/utils.rs:84-88);
// anything else throws std::logic_error where the reference panics.
// The constraint matrices of one circuit in HBM (F_q values in CSR and CSC order) with the proof-time tables
// beside them.  What prepare_for_random_field_piop recomputes per proof in the reference
// (ccs.map_to_field / statement.map_to_field, prover.rs:188-189) depends only on the circuit and the field:
// build it once, hand it to every proof.  One proof at a time per object (internally locked).
class PreparedCcs {
  public:
    PreparedCcs(const ccs::Statement_Z &statement, const ccs::CCS_Z &ccs, const FieldConfig &config, int device = 0);
    // the same from borrowed CSR arrays (t matrices of 2^s columns): nothing is copied on the host
    PreparedCcs(const zip_sparse_matrix *matrices, uint32_t t, uint32_t s, const FieldConfig &config, int device = 0);
    ~PreparedCcs();
    PreparedCcs(const PreparedCcs &) = delete;
    PreparedCcs &operator=(const PreparedCcs &) = delete;

  private:
    friend class ZincProver;
    friend class ZincVerifier;
    zip_ccs *h_ = nullptr;
    std::mutex mu_;
    uint32_t t_ = 0, s_ = 0, limbs_ = 0;
    Limbs modulus_{};
    int device_ = 0;
};

class ZincProver {
  public:
    explicit ZincProver(zip::LinearCodeSpec spec = {}, int device = 0) : lc_spec_(spec), device_(device) {}
    // Prover::prove (prover.rs:50-88)
    // r_y_out: the second sumcheck's point (the verifier re-derives it; handed out for tests and tools)
    // prepared: the circuit's matrices already on the device (must come from the same statement and field)
    ZincProof prove(const ccs::Statement_Z &statement, const ccs::Witness_Z &wit, KeccakTranscript &transcript,
                    const ccs::CCS_Z &ccs, const FieldConfig &config, std::vector<Limbs> *r_y_out = nullptr,
                    PreparedCcs *prepared = nullptr) const;
    // the same from the z vector itself (x || 1 || w, at most ccs.m entries; shorter vectors are zero-extended)
    ZincProof prove_z(const ccs::Statement_Z &statement, const int64_t *z_ccs, size_t z_len, KeccakTranscript &transcript,
                      const ccs::CCS_Z &ccs, const FieldConfig &config, std::vector<Limbs> *r_y_out = nullptr,
                      PreparedCcs *prepared = nullptr) const;
    // prepare_for_random_field_piop (:172-191, the z vector) + SpartanProver::prove (:130-161)
    std::pair<SpartanProof, std::vector<Limbs>> spartan_prove(const ccs::Statement_Z &statement, const int64_t *z_ccs, size_t z_len,
                                                              KeccakTranscript &transcript, const ccs::CCS_Z &ccs,
                                                              const FieldConfig &config, PreparedCcs *prepared = nullptr) const;
    // B proofs of ONE circuit, each with its own z, transcript and field: for every instance exactly what spartan_prove
    // does -- the same proof, r_y and transcript afterwards.  From 2 instances on, with s <= 16 and one limb count in all
    // configs (and not below the line of min_spartan_batch, zinc_zip.cpp), the matrices go to the device ONCE, as integers
    // (zip_ccs_batch), the tables of all proofs are built with a launch count that does not depend on B, and each of the
    // two sumchecks is ONE zip_sumcheck_prove_batch call over the device tables.  ZIP_HIP_BATCH=0, one instance and every
    // shape the batch does not serve take the loop over spartan_prove.  Every shape check of spartan_prove runs on every
    // instance before any transcript is touched.
    struct ZVector {
        const int64_t *z = nullptr;
        size_t len = 0;
    };
    using SpartanOutput = std::pair<SpartanProof, std::vector<Limbs>>;
    std::vector<SpartanOutput> spartan_prove_batch(const ccs::Statement_Z &statement, const ccs::CCS_Z &ccs,
                                                   const std::vector<ZVector> &zs, const std::vector<KeccakTranscript *> &transcripts,
                                                   const std::vector<FieldConfig> &configs) const;
    // the same from borrowed CSR arrays (ccs.t matrices of 2^s columns): nothing is copied on the host
    std::vector<SpartanOutput> spartan_prove_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs,
                                                   const std::vector<ZVector> &zs, const std::vector<KeccakTranscript *> &transcripts,
                                                   const std::vector<FieldConfig> &configs) const;
    // The PCS step of B proofs of one ccs, r_y[i] and transcripts[i] as spartan_prove_batch left them: the ZipProofs,
    // the transcripts afterwards and the errors of the loop over pcs_step, member after member.  One commit and one open
    // for all of them (zip::commit_z_mle_and_prove_evaluation_batch) -- unless ZIP_HIP_BATCH=0 is set, there is one
    // instance, the spec asks for more than one proximity test, the codeword is above 8192, the fields differ in their
    // limb count, or B is below the line of min_pcs_batch (zinc_zip.cpp; ZIP_HIP_PCS_MIN_BATCH=n moves it): then the loop.
    std::vector<zip::ZipProof> pcs_step_batch(const ccs::CCS_Z &ccs, const std::vector<ZVector> &zs,
                                              const std::vector<std::vector<Limbs>> &r_y,
                                              const std::vector<KeccakTranscript *> &transcripts,
                                              const std::vector<FieldConfig> &configs) const;
    // spartan_prove_batch, then pcs_step_batch.
    std::vector<ZincProof> prove_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs, const std::vector<ZVector> &zs,
                                       const std::vector<KeccakTranscript *> &transcripts, const std::vector<FieldConfig> &configs,
                                       std::vector<std::vector<Limbs>> *r_y_out = nullptr) const;
    // get_z_ccs_and_z_mle (:222-239): x || 1 || w, zero-extended to ccs.m
    static IntVec get_z_ccs(const int64_t *x, size_t l, const int64_t *w, size_t w_len, size_t m);
    static IntVec get_z_ccs(const ccs::Statement_Z &statement, const ccs::Witness_Z &wit, const ccs::CCS_Z &ccs) {
        return get_z_ccs(statement.public_input.data(), statement.public_input.size(), wit.w_ccs.data(), wit.w_ccs.size(), ccs.m);
    }

  private:
    // commit_z_mle_and_prove_evaluation over z zero-extended to 2^s_prime (prover.rs:305-327)
    zip::ZipProof pcs_step(const int64_t *z_ccs, size_t z_len, const ccs::CCS_Z &ccs, const std::vector<Limbs> &r_y,
                           KeccakTranscript &transcript, const FieldConfig &config) const;
    zip::LinearCodeSpec lc_spec_;
    int device_;
};

// VerificationPoints (src/zinc/verifier.rs:275-279)
struct VerificationPoints {
    std::vector<Limbs> rx_ry;
    Limbs e_y{}, gamma{};
};
// ZincVerifier (src/zinc/verifier.rs).  The sumcheck verifiers are O(s * d) field operations on the host; the
// Zip verifier and the evaluation of the matrix MLEs at (r_x, r_y) run on the device.  The draw_random_field check
// of Verifier::verify (:53-57) is verify_checked's; verify itself takes the field it is handed.
// For B proofs: verify_batch, check_field_batch and verify_batch_checked.
class ZincVerifier {
  public:
    explicit ZincVerifier(zip::LinearCodeSpec spec = {}, int device = 0) : lc_spec_(spec), device_(device) {}
    // Verifier::verify (:45-76) without the field check; throws SpartanError / ZipError{InvalidPcsOpen}
    void verify(const ccs::Statement_Z &statement, const ZincProof &proof, KeccakTranscript &transcript, const ccs::CCS_Z &ccs,
                const FieldConfig &config, PreparedCcs *prepared = nullptr) const;
    // Verifier::verify (:45-76) whole: first draw_random_field(statement.public_input, transcript) (:53-57) and throw
    // FieldConfigError if it is not `config` (same limbs, same modulus) -- before any other work --, then verify
    void verify_checked(const ccs::Statement_Z &statement, const ZincProof &proof, KeccakTranscript &transcript,
                        const ccs::CCS_Z &ccs, const FieldConfig &config, PreparedCcs *prepared = nullptr) const;
    // the check alone (:53-57): draws the field of `config.limbs` limbs from the public input on `transcript` and throws
    // FieldConfigError unless it is `config`; the transcript is then where the reference's verify continues
    void check_field(const int64_t *public_input, size_t l, KeccakTranscript &transcript, const FieldConfig &config) const;
    // SpartanVerifier::verify (:105-139)
    VerificationPoints spartan_verify(const SpartanProof &proof, const ccs::CCS_Z &ccs, KeccakTranscript &transcript,
                                      const FieldConfig &config) const;
    // verify_pcs_proof (:221-273)
    void verify_pcs_proof(const ccs::Statement_Z &statement, const zip::ZipProof &zip_proof, const VerificationPoints &points,
                          const ccs::CCS_Z &ccs, KeccakTranscript &transcript, const FieldConfig &config,
                          PreparedCcs *prepared = nullptr) const {
        verify_pcs_proof(statement, zip_proof.z_comm, zip_proof.v, zip_proof.pcs_proof.data(), zip_proof.pcs_proof.size(), points,
                         ccs, transcript, config, prepared);
    }
    // the same over borrowed proof bytes
    void verify_pcs_proof(const ccs::Statement_Z &statement, const zip::MultilinearZipCommitment &z_comm, const Limbs &v,
                          const uint8_t *pcs_proof, size_t pcs_proof_len, const VerificationPoints &points,
                          const ccs::CCS_Z &ccs, KeccakTranscript &transcript, const FieldConfig &config,
                          PreparedCcs *prepared = nullptr) const;

    // B proofs of ONE circuit, each with its own transcript and field (what ZincProver::prove_batch makes): for every
    // proof exactly what `verify` does -- outcome i and transcripts[i] afterwards are what the loop over verify leaves,
    // for rejected proofs as well -- but the call does not stop at the first reject: it returns one outcome per proof.
    // The batched path: per member spartan_verify on the host (a member that fails there has its outcome and leaves the
    // batch); per survivor RaaCode::make on its transcript, its two permutations, the squeezes of a fresh PcsTranscript
    // and the point's tensors; ONE zip_batch_verify_codes with the streams passed by pointer; ONE
    // zip_ccs_batch_eval_matrices over the circuit as integers (no PreparedCcs per field); per member, in the loop's
    // order, the PCS verdict and then gamma-combination * v == e_y.
    // The loop over verify runs instead with ZIP_HIP_BATCH=0, one instance, more than one proximity test, codewords above
    // 16384, s above 16, differing limb counts, or B below the line of min_verify_batch (zinc_zip.cpp;
    // ZIP_HIP_VERIFY_MIN_BATCH=n moves it).
    // std::logic_error is a shape the reference panics on: thrown for the first member that has it, before any device
    // work.  (An encode_wide overflow inside a proof stream, the one panic the device finds, is thrown when that member's
    // turn comes, as the loop throws it; the batched path has then moved the later members' transcripts already.)
    // Not part of this: the field check of verify_checked -- that is check_field_batch, and verify_batch_checked runs
    // the two one after the other.
    struct BatchProof {  // one ZincProof, its bytes borrowed
        const SpartanProof *spartan_proof = nullptr;
        const zip::MultilinearZipCommitment *z_comm = nullptr;
        const Limbs *v = nullptr;
        const uint8_t *pcs_proof = nullptr;
        size_t pcs_proof_len = 0;
    };
    struct BatchOutcome {
        // (FieldConfig: verify_batch_checked alone -- the member's drawn field is not the one handed over)
        enum Kind { Accepted, Spartan, Zip, FieldConfig } kind = Accepted;
        ZipError::Kind zip_kind = ZipError::InvalidPcsOpen;  // kind == Zip: InvalidPcsOpen, Transcript or InvalidPcsParam
        std::string message;                                 // what() of what verify would have thrown for this proof alone
        bool accepted() const { return kind == Accepted; }
    };
    std::vector<BatchOutcome> verify_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs, const std::vector<BatchProof> &proofs,
                                           const std::vector<KeccakTranscript *> &transcripts,
                                           const std::vector<FieldConfig> &configs) const;
    std::vector<BatchOutcome> verify_batch(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs, const std::vector<const ZincProof *> &proofs,
                                           const std::vector<KeccakTranscript *> &transcripts,
                                           const std::vector<FieldConfig> &configs) const;

    // check_field for every member of a batch: result[i] = the field drawn from public_inputs[i] on transcripts[i], at
    // configs[i].limbs limbs, IS configs[i].  Every transcript is left where check_field leaves it, for the members that
    // fail as well.  The members of one limb count are one draw_random_field_batch.
    std::vector<bool> check_field_batch(const std::vector<const int64_t *> &public_inputs, const std::vector<size_t> &lens,
                                        const std::vector<KeccakTranscript *> &transcripts,
                                        const std::vector<zinc::FieldConfig> &configs) const;
    // verify_checked for every member: check_field_batch, then verify_batch over the members that passed.  A member
    // that failed the field check has kind FieldConfig and its transcript where check_field left it.
    std::vector<BatchOutcome> verify_batch_checked(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs,
                                                   const std::vector<const int64_t *> &public_inputs, const std::vector<size_t> &lens,
                                                   const std::vector<BatchProof> &proofs,
                                                   const std::vector<KeccakTranscript *> &transcripts,
                                                   const std::vector<zinc::FieldConfig> &configs) const;
    std::vector<BatchOutcome> verify_batch_checked(const zip_sparse_matrix *matrices, const ccs::CCS_Z &ccs,
                                                   const std::vector<const int64_t *> &public_inputs, const std::vector<size_t> &lens,
                                                   const std::vector<const ZincProof *> &proofs,
                                                   const std::vector<KeccakTranscript *> &transcripts,
                                                   const std::vector<zinc::FieldConfig> &configs) const;

  private:
    zip::LinearCodeSpec lc_spec_;
    int device_;
};
}  // namespace zinc
