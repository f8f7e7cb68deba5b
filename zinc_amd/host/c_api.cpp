// C facade over zinc_zip.hpp (include/zinc_zip_host.h): opaque handles + error-code mapping.
#include <string>

#include "zinc_zip.hpp"
#include "zinc_zip_host.h"

using namespace zinc;
using namespace zinc::zip;

struct zinc_transcript { KeccakTranscript t; };
struct zinc_zip_params { MultilinearZipParams pp; };
struct zinc_zip_data { MultilinearZipData d; };
struct zinc_pcs_transcript { PcsTranscript t; };

namespace {
thread_local std::string g_err;

template <class F>
int32_t guarded(F &&f) {
    try {
        f();
        return ZINC_OK;
    } catch (const zinc::FieldConfigError &e) {
        g_err = e.what();
        return ZINC_ERR_FIELD_CONFIG;
    } catch (const zinc::SpartanError &e) {
        g_err = e.what();
        return ZINC_ERR_SPARTAN;
    } catch (const ZipError &e) {
        g_err = e.what();
        return e.kind == ZipError::InvalidPcsParam ? ZINC_ERR_INVALID_PARAM
               : (e.kind == ZipError::InvalidPcsOpen || e.kind == ZipError::Transcript) ? ZINC_ERR_INVALID_OPEN
                                                                                        : ZINC_ERR_DEVICE;
    } catch (const std::logic_error &e) {  // where the reference panics
        g_err = e.what();
        return ZINC_ERR_PANIC;
    } catch (const std::exception &e) {
        g_err = e.what();
        return ZINC_ERR_DEVICE;
    }
}
Limbs load(const uint64_t *p, uint32_t n) {
    Limbs l{};
    for (uint32_t i = 0; i < n; i++) l[i] = p[i];
    return l;
}
}  // namespace

extern "C" {

const char *zinc_last_error(void) { return g_err.c_str(); }

zinc_transcript *zinc_transcript_new(void) { return new zinc_transcript(); }
void zinc_transcript_free(zinc_transcript *t) { delete t; }
void zinc_transcript_absorb(zinc_transcript *t, const uint8_t *bytes, size_t len) { t->t.absorb(bytes, len); }
uint64_t zinc_transcript_get_u64(zinc_transcript *t) { return t->t.get_u64(); }
void zinc_transcript_get_integer_challenges(zinc_transcript *t, size_t n, int64_t *out) {
    const auto v = t->t.get_integer_challenges_i64(n);
    for (size_t i = 0; i < n; i++) out[i] = v[i];
}
int32_t zinc_transcript_get_challenge(zinc_transcript *t, const uint64_t *modulus, uint32_t limbs, uint64_t *out) {
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        const Limbs c = t->t.get_challenge(f);
        for (uint32_t i = 0; i < limbs; i++) out[i] = c[i];
    });
}

int32_t zinc_transcript_export(const zinc_transcript *t, uint64_t *st, uint8_t *buf, uint32_t *buflen) {
    if (!t || !st || !buf || !buflen) return ZINC_ERR_NULL;
    zip_keccak_state k;
    t->t.export_state(&k);
    std::memcpy(st, k.st, sizeof k.st);
    std::memcpy(buf, k.buf, sizeof k.buf);
    *buflen = k.buflen;
    return ZINC_OK;
}
int32_t zinc_transcript_import(zinc_transcript *t, const uint64_t *st, const uint8_t *buf, uint32_t buflen) {
    if (!t || !st || !buf) return ZINC_ERR_NULL;
    if (buflen >= 136) {
        g_err = "zinc_transcript_import: buflen is not below the Keccak-256 rate (136)";
        return ZINC_ERR_INVALID_PARAM;
    }
    zip_keccak_state k{};
    std::memcpy(k.st, st, sizeof k.st);
    std::memcpy(k.buf, buf, buflen);
    k.buflen = buflen;
    t->t.import_state(k);
    return ZINC_OK;
}

int32_t zinc_get_prime(zinc_transcript *t, uint32_t limbs, int32_t device, uint64_t *prime_out, uint32_t *candidates_tried_out) {
    if (!t || !prime_out) return ZINC_ERR_NULL;
    return guarded([&] {
        const Limbs p = prime_gen::get_prime(t->t, limbs, device, candidates_tried_out);
        for (uint32_t i = 0; i < limbs; i++) prime_out[i] = p[i];
    });
}
int32_t zinc_draw_random_field(const int64_t *public_input, size_t l, zinc_transcript *t, uint32_t limbs, int32_t device,
                               uint64_t *modulus_out) {
    if (!t || !modulus_out || (l && !public_input)) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = draw_random_field(public_input, l, t->t, limbs, device);
        for (uint32_t i = 0; i < limbs; i++) modulus_out[i] = f.modulus[i];
    });
}
int32_t zinc_get_prime_batch(zinc_transcript *const *transcripts, uint32_t n, uint32_t limbs, int32_t device, uint64_t *primes_out,
                             uint32_t *candidates_tried_out) {
    if (!transcripts || !primes_out) return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n; i++)
        if (!transcripts[i]) return ZINC_ERR_NULL;
    return guarded([&] {
        std::vector<KeccakTranscript *> tr(n);
        for (uint32_t i = 0; i < n; i++) tr[i] = &transcripts[i]->t;
        const std::vector<Limbs> p = prime_gen::get_prime_batch(tr, limbs, device, candidates_tried_out);
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = 0; j < limbs; j++) primes_out[(size_t)i * limbs + j] = p[i][j];
    });
}
int32_t zinc_draw_random_field_batch(const int64_t *const *public_inputs, const size_t *lens, zinc_transcript *const *transcripts,
                                     uint32_t n, uint32_t limbs, int32_t device, uint64_t *moduli_out) {
    if (!public_inputs || !lens || !transcripts || !moduli_out) return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n; i++)
        if (!transcripts[i] || (lens[i] && !public_inputs[i])) return ZINC_ERR_NULL;
    return guarded([&] {
        std::vector<KeccakTranscript *> tr(n);
        for (uint32_t i = 0; i < n; i++) tr[i] = &transcripts[i]->t;
        const std::vector<FieldConfig> f = draw_random_field_batch(std::vector<const int64_t *>(public_inputs, public_inputs + n),
                                                                   std::vector<size_t>(lens, lens + n), tr, limbs, device);
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = 0; j < limbs; j++) moduli_out[(size_t)i * limbs + j] = f[i].modulus[j];
    });
}
int32_t zinc_verifier_check_field_batch(const int64_t *const *public_inputs, const size_t *lens, zinc_transcript *const *transcripts,
                                        uint32_t n, const uint64_t *moduli, const uint32_t *limbs, int32_t device, uint8_t *same_out) {
    if (!public_inputs || !lens || !transcripts || !moduli || !limbs || !same_out) return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n; i++)
        if (!transcripts[i] || (lens[i] && !public_inputs[i])) return ZINC_ERR_NULL;
    return guarded([&] {
        std::vector<KeccakTranscript *> tr(n);
        std::vector<FieldConfig> f;
        for (uint32_t i = 0; i < n; i++) {
            tr[i] = &transcripts[i]->t;
            f.push_back(FieldConfig::make(moduli + (size_t)i * 4, limbs[i]));
        }
        const std::vector<bool> same = zinc::ZincVerifier({}, device).check_field_batch(
            std::vector<const int64_t *>(public_inputs, public_inputs + n), std::vector<size_t>(lens, lens + n), tr, f);
        for (uint32_t i = 0; i < n; i++) same_out[i] = same[i] ? 1 : 0;
    });
}

int32_t zinc_field_constants(const uint64_t *modulus, uint32_t limbs, uint64_t *r, uint64_t *r2, uint64_t *inv) {
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        for (uint32_t i = 0; i < limbs; i++) {
            r[i] = f.r[i];
            r2[i] = f.r2[i];
        }
        *inv = f.inv;
    });
}
int32_t zinc_field_mul(const uint64_t *modulus, uint32_t limbs, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        Limbs x = load(a, limbs);
        f.mul_assign(x, load(b, limbs));
        for (uint32_t i = 0; i < limbs; i++) out[i] = x[i];
    });
}
int32_t zinc_map_to_field_i64(const uint64_t *modulus, uint32_t limbs, const int64_t *v, size_t n, uint64_t *out) {
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        for (size_t k = 0; k < n; k++) {
            const Limbs x = map_to_field(f, v[k]);
            for (uint32_t i = 0; i < limbs; i++) out[k * limbs + i] = x[i];
        }
    });
}
int32_t zinc_build_eq_x_r(const uint64_t *modulus, uint32_t limbs, const uint64_t *r, uint32_t nvars, uint64_t *out) {
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<Limbs> rv(nvars);
        for (uint32_t t = 0; t < nvars; t++) rv[t] = load(r + (size_t)t * limbs, limbs);
        const auto eq = build_eq_x_r(f, rv.data(), nvars);
        for (size_t k = 0; k < eq.size(); k++)
            for (uint32_t i = 0; i < limbs; i++) out[k * limbs + i] = eq[k][i];
    });
}

void zinc_shuffle_seeded_perm(uint64_t seed, uint32_t len, uint32_t *perm) {
    const auto p = shuffle_seeded_perm(seed, len);
    for (uint32_t i = 0; i < len; i++) perm[i] = p[i];
}

void zinc_kat_seed_from_u64(uint64_t seed, uint32_t *words, uint32_t n_words) { kat_seed_from_u64(seed, words, n_words); }

// NULL: DefaultLinearCodeSpec
static LinearCodeSpec spec_of(const zinc_linear_code_spec *spec) {
    LinearCodeSpec s;
    if (spec) {
        s.num_column_opening = spec->num_column_opening;
        s.repetition_factor = spec->repetition_factor;
        s.num_proximity_testing = spec->num_proximity_testing;
    }
    return s;
}

int32_t zinc_raa_code_new(uint64_t poly_size, zinc_transcript *transcript, zinc_raa_code *out) {
    return zinc_raa_code_new_spec(nullptr, poly_size, transcript, out);
}
int32_t zinc_raa_code_new_spec(const zinc_linear_code_spec *spec, uint64_t poly_size, zinc_transcript *transcript,
                               zinc_raa_code *out) {
    if (!out) return ZINC_ERR_NULL;
    return guarded([&] {
        RaaCode c;
        if (transcript) {
            KeccakSeedSource src(transcript->t);
            c = RaaCode::make(spec_of(spec), poly_size, src);
        } else {
            MockTranscript mock;
            c = RaaCode::make(spec_of(spec), poly_size, mock);
        }
        *out = {c.row_len, c.repetition_factor, c.num_column_opening, c.num_proximity_testing, c.perm_1_seed, c.perm_2_seed};
    });
}

int32_t zinc_zip_setup(uint64_t poly_size, const zinc_raa_code *code, int32_t device, zinc_zip_params **out) {
    if (!code || !out) return ZINC_ERR_NULL;
    *out = nullptr;
    return guarded([&] {
        RaaCode c;
        c.row_len = code->row_len;
        c.repetition_factor = code->repetition_factor;
        c.num_column_opening = code->num_column_opening;
        c.num_proximity_testing = code->num_proximity_testing;
        c.perm_1_seed = code->perm_1_seed;
        c.perm_2_seed = code->perm_2_seed;
        auto *pp = new zinc_zip_params{MultilinearZip::setup(poly_size, c, device)};
        *out = pp;
    });
}
void zinc_zip_params_free(zinc_zip_params *pp) { delete pp; }
void zinc_zip_release_cached_contexts(void) { MultilinearZip::release_cached_contexts(); }
void zinc_zip_params_geometry(const zinc_zip_params *pp, uint32_t *num_vars, uint32_t *num_rows, uint32_t *row_len,
                              uint32_t *codeword_len) {
    *num_vars = pp->pp.num_vars;
    *num_rows = pp->pp.num_rows;
    *row_len = pp->pp.linear_code.row_len;
    *codeword_len = pp->pp.linear_code.codeword_len();
}

int32_t zinc_zip_commit(const zinc_zip_params *pp, const int64_t *evals, size_t n_evals, uint32_t poly_num_vars,
                        int32_t with_merkle, uint8_t *roots_out, zinc_zip_data **out) {
    if (!pp || !out) return ZINC_ERR_NULL;
    *out = nullptr;
    return guarded([&] {
        if (with_merkle) {
            auto res = MultilinearZip::commit(pp->pp, evals, n_evals, poly_num_vars);
            if (roots_out) std::memcpy(roots_out, res.second.roots.data(), res.second.roots.size() * 32);
            *out = new zinc_zip_data{std::move(res.first)};
        } else {
            *out = new zinc_zip_data{MultilinearZip::commit_no_merkle(pp->pp, evals, n_evals, poly_num_vars)};
        }
    });
}
void zinc_zip_data_free(zinc_zip_data *d) { delete d; }

int32_t zinc_zip_data_download(const zinc_zip_data *d, uint64_t *rows_out, uint8_t *layers_out, uint8_t *roots_out) {
    if (!d) return ZINC_ERR_NULL;
    return guarded([&] {
        const int32_t rc = zip_commit_download(d->d.handle.get(), rows_out, layers_out, roots_out);
        if (rc) throw ZipError(ZipError::Device, std::string("zip_commit_download: ") + zip_ctx_last_error(d->d.ctx.get()));
    });
}

int32_t zinc_zip_data_upload(const zinc_zip_params *pp, const uint64_t *rows, const uint8_t *layers,
                             const uint8_t *roots, zinc_zip_data **out) {
    if (!pp || !rows || !out) return ZINC_ERR_NULL;
    *out = nullptr;
    return guarded([&] {
        zip_commitment *h = nullptr;
        const int32_t rc = zip_commitment_upload(pp->pp.ctx.get(), rows, layers, roots, &h);
        if (rc) throw ZipError(ZipError::Device, std::string("zip_commitment_upload: ") + zip_ctx_last_error(pp->pp.ctx.get()));
        MultilinearZipData data;
        data.ctx = pp->pp.ctx;
        data.handle = std::shared_ptr<zip_commitment>(h, zip_commitment_free);
        *out = new zinc_zip_data{std::move(data)};
    });
}

int32_t zinc_merkle_tree_new(uint32_t depth, const uint64_t *leaves, size_t n_leaves, uint32_t leaf_limbs,
                             int32_t device, uint8_t *layers_out) {
    if (!leaves || !layers_out) return ZINC_ERR_NULL;
    return guarded([&] {
        if (n_leaves == 0 || (n_leaves & (n_leaves - 1))) throw std::logic_error("assertion failed: leaves.len().is_power_of_two()");
        if (n_leaves != ((size_t)1 << depth)) throw std::logic_error("assertion failed: leaves.len() == 1 << merkle_depth");
        const int32_t rc = zip_merkle_trees(device, leaves, leaf_limbs, depth, 1, ZIP_MEM_HOST, layers_out);
        if (rc) throw ZipError(ZipError::Device, std::string("zip_merkle_trees: ") + zip_strerror(rc));
    });
}

zinc_pcs_transcript *zinc_pcs_transcript_new(void) { return new zinc_pcs_transcript(); }
void zinc_pcs_transcript_free(zinc_pcs_transcript *t) { delete t; }
size_t zinc_pcs_transcript_len(const zinc_pcs_transcript *t) { return t->t.stream.size(); }
void zinc_pcs_transcript_copy(const zinc_pcs_transcript *t, uint8_t *out) {
    std::memcpy(out, t->t.stream.data(), t->t.stream.size());
}
uint64_t zinc_pcs_transcript_probe(const zinc_pcs_transcript *t) {
    KeccakTranscript copy = t->t.fs_transcript;
    return copy.get_u64();
}

int32_t zinc_zip_open(const zinc_zip_params *pp, const int64_t *evals, size_t n_evals, uint32_t poly_num_vars,
                      const zinc_zip_data *data, const uint64_t *point, size_t point_len, const uint64_t *modulus,
                      uint32_t limbs, zinc_pcs_transcript *transcript) {
    if (!pp || !data || !transcript) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<Limbs> pt(point_len);
        for (size_t i = 0; i < point_len; i++) pt[i] = load(point + i * limbs, limbs);
        MultilinearZip::open(pp->pp, evals, n_evals, poly_num_vars, data->d, pt.data(), point_len, f, transcript->t);
    });
}

int32_t zinc_zip_batch_commit(const zinc_zip_params *pp, const int64_t *const *polys, const size_t *n_evals,
                              const uint32_t *poly_num_vars, size_t n_polys, uint8_t *roots_out, zinc_zip_data **out) {
    if (!pp || (n_polys && (!polys || !n_evals || !poly_num_vars || !out))) return ZINC_ERR_NULL;
    for (size_t i = 0; i < n_polys; i++) out[i] = nullptr;
    return guarded([&] {
        std::vector<PolyRef> refs(n_polys);
        for (size_t i = 0; i < n_polys; i++) refs[i] = {polys[i], n_evals[i], poly_num_vars[i]};
        auto res = MultilinearZip::batch_commit(pp->pp, refs.data(), n_polys);
        const size_t root_bytes = (size_t)pp->pp.num_rows * 32;
        for (size_t i = 0; i < n_polys; i++) {
            if (roots_out) std::memcpy(roots_out + i * root_bytes, res[i].second.roots.data(), root_bytes);
            out[i] = new zinc_zip_data{std::move(res[i].first)};
        }
    });
}

int32_t zinc_zip_batch_open(const zinc_zip_params *pp, const int64_t *const *polys, const size_t *n_evals,
                            const uint32_t *poly_num_vars, const zinc_zip_data *const *datas, const uint64_t *const *points,
                            size_t n_polys, const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript) {
    if (!pp || !transcript || (n_polys && (!polys || !n_evals || !poly_num_vars || !datas || !points))) return ZINC_ERR_NULL;
    for (size_t i = 0; i < n_polys; i++)
        if (!datas[i]) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<PolyRef> refs(n_polys);
        std::vector<std::vector<Limbs>> pts(n_polys);
        std::vector<const Limbs *> pt_ptrs(n_polys);
        std::vector<const MultilinearZipData *> ds(n_polys);
        for (size_t i = 0; i < n_polys; i++) {
            refs[i] = {polys[i], n_evals[i], poly_num_vars[i]};
            pts[i].resize(poly_num_vars[i]);
            for (uint32_t k = 0; k < poly_num_vars[i]; k++) pts[i][k] = load(points[i] + (size_t)k * limbs, limbs);
            pt_ptrs[i] = pts[i].data();
            ds[i] = &datas[i]->d;
        }
        MultilinearZip::batch_open(pp->pp, refs.data(), ds.data(), pt_ptrs.data(), n_polys, f, transcript->t);
    });
}

int32_t zinc_zip_batch_open_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                       const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript,
                                       const uint64_t *eval_rows, size_t n_polys, int64_t *coeffs_out, uint32_t *cols_out) {
    if (!modulus || !transcript || (n_polys && (!eval_rows || (n_cols && !cols_out) || (num_rows > 1 && !coeffs_out))))
        return ZINC_ERR_NULL;
    return guarded([&] {
        if (!codeword_len) throw ZipError(ZipError::InvalidPcsParam, "codeword_len is 0");
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        MultilinearZip::batch_open_challenges(num_rows, row_len, codeword_len, n_cols, f, transcript->t, eval_rows, n_polys,
                                              coeffs_out, cols_out);
    });
}

int32_t zinc_zip_open_challenges(uint32_t num_rows, uint32_t codeword_len, uint32_t num_column_opening,
                                 uint32_t num_proximity_testing, const uint64_t *modulus, uint32_t limbs,
                                 zinc_pcs_transcript *transcript, int64_t *coeffs_out, uint32_t *cols_out) {
    if (!modulus || !transcript || (num_column_opening && !cols_out)) return ZINC_ERR_NULL;
    return guarded([&] {
        if (!codeword_len) throw ZipError(ZipError::InvalidPcsParam, "codeword_len is 0");
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        const auto ch = MultilinearZip::open_challenges(num_rows, codeword_len, num_column_opening, num_proximity_testing, f,
                                                        transcript->t);
        if (!ch.first.empty() && !coeffs_out) throw ZipError(ZipError::InvalidPcsParam, "coeffs_out is NULL");
        std::copy(ch.first.begin(), ch.first.end(), coeffs_out);
        std::copy(ch.second.begin(), ch.second.end(), cols_out);
    });
}

zinc_pcs_transcript *zinc_pcs_transcript_from_proof(const uint8_t *proof, size_t len) {
    auto *t = new zinc_pcs_transcript();
    t->t = PcsTranscript::from_proof(proof, len);
    return t;
}
size_t zinc_pcs_transcript_position(const zinc_pcs_transcript *t) { return t->t.read_pos; }

int32_t zinc_zip_verify(const zinc_zip_params *vp, const uint8_t *roots, const uint64_t *point, size_t point_len,
                        const uint64_t *eval, const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript) {
    if (!vp || !roots || !eval || !transcript) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<Limbs> pt(point_len);
        for (size_t i = 0; i < point_len; i++) pt[i] = load(point + i * limbs, limbs);
        MultilinearZipCommitment comm;
        comm.roots.resize(vp->pp.num_rows);
        std::memcpy(comm.roots.data(), roots, (size_t)vp->pp.num_rows * 32);
        MultilinearZip::verify(vp->pp, comm, pt.data(), point_len, load(eval, limbs), transcript->t, f);
    });
}

int32_t zinc_zip_batch_verify(const zinc_zip_params *vp, const uint8_t *roots, const uint64_t *const *points,
                              const size_t *point_lens, const uint64_t *evals, size_t n_polys, const uint64_t *modulus,
                              uint32_t limbs, zinc_pcs_transcript *transcript) {
    if (!vp || !transcript || (n_polys && (!roots || !points || !point_lens || !evals))) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        const size_t root_bytes = (size_t)vp->pp.num_rows * 32;
        std::vector<MultilinearZipCommitment> comms(n_polys);
        std::vector<const MultilinearZipCommitment *> comm_ptrs(n_polys);
        std::vector<std::vector<Limbs>> pts(n_polys);
        std::vector<const Limbs *> pt_ptrs(n_polys);
        std::vector<Limbs> evs(n_polys);
        for (size_t i = 0; i < n_polys; i++) {
            comms[i].roots.resize(vp->pp.num_rows);
            std::memcpy(comms[i].roots.data(), roots + i * root_bytes, root_bytes);
            comm_ptrs[i] = &comms[i];
            pts[i].resize(point_lens[i]);
            for (size_t k = 0; k < point_lens[i]; k++) pts[i][k] = load(points[i] + k * limbs, limbs);
            pt_ptrs[i] = pts[i].data();
            evs[i] = load(evals + i * limbs, limbs);
        }
        MultilinearZip::batch_verify_z(vp->pp, comm_ptrs.data(), pt_ptrs.data(), point_lens, evs.data(), n_polys, transcript->t, f);
    });
}

int32_t zinc_zip_batch_verify_challenges(uint32_t num_rows, uint32_t row_len, uint32_t codeword_len, uint32_t n_cols,
                                         const uint64_t *modulus, uint32_t limbs, zinc_pcs_transcript *transcript,
                                         const uint8_t *proofs, size_t stream_len, size_t n_polys, int64_t *coeffs_out,
                                         uint32_t *cols_out) {
    if (!modulus || !transcript || (n_polys && (!proofs || (n_cols && !cols_out) || (num_rows > 1 && !coeffs_out))))
        return ZINC_ERR_NULL;
    return guarded([&] {
        if (!codeword_len) throw ZipError(ZipError::InvalidPcsParam, "codeword_len is 0");
        if (stream_len < (size_t)row_len * limbs * 8) throw ZipError(ZipError::InvalidPcsParam, "stream_len is shorter than the evaluation row");
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        MultilinearZip::batch_verify_challenges(num_rows, row_len, codeword_len, n_cols, f, transcript->t, proofs, stream_len,
                                                n_polys, coeffs_out, cols_out);
    });
}

int32_t zinc_zip_evaluate(const zinc_zip_params *pp, const int64_t *evals, size_t n_evals, const uint64_t *point,
                          size_t point_len, const uint64_t *modulus, uint32_t limbs, uint64_t *out) {
    if (!pp || !evals || !out) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<Limbs> pt(point_len);
        for (size_t i = 0; i < point_len; i++) pt[i] = load(point + i * limbs, limbs);
        const Limbs v = MultilinearZip::evaluate(pp->pp, evals, n_evals, pt.data(), point_len, f);
        for (uint32_t i = 0; i < limbs; i++) out[i] = v[i];
    });
}

struct zinc_zip_proof {
    zinc::zip::ZipProof p;
    uint32_t limbs;
};
int32_t zinc_commit_z_mle_and_prove_evaluation(const int64_t *z_evals, size_t m, const uint64_t *r_y, size_t r_y_len,
                                               zinc_transcript *transcript, const uint64_t *modulus, uint32_t limbs,
                                               int32_t device, zinc_zip_proof **out) {
    return zinc_commit_z_mle_and_prove_evaluation_spec(nullptr, z_evals, m, r_y, r_y_len, transcript, modulus, limbs, device, out);
}
int32_t zinc_commit_z_mle_and_prove_evaluation_spec(const zinc_linear_code_spec *spec, const int64_t *z_evals, size_t m,
                                                    const uint64_t *r_y, size_t r_y_len, zinc_transcript *transcript,
                                                    const uint64_t *modulus, uint32_t limbs, int32_t device,
                                                    zinc_zip_proof **out) {
    if (!z_evals || !transcript || !out) return ZINC_ERR_NULL;
    *out = nullptr;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<Limbs> pt(r_y_len);
        for (size_t i = 0; i < r_y_len; i++) pt[i] = load(r_y + i * limbs, limbs);
        auto *res = new zinc_zip_proof{
            zinc::zip::commit_z_mle_and_prove_evaluation(spec_of(spec), z_evals, m, pt.data(), r_y_len, transcript->t, f, device),
            limbs};
        *out = res;
    });
}
size_t zinc_zip_proof_len(const zinc_zip_proof *p) { return p->p.pcs_proof.size(); }
size_t zinc_zip_proof_num_roots(const zinc_zip_proof *p) { return p->p.z_comm.roots.size(); }
void zinc_zip_proof_read(const zinc_zip_proof *p, uint8_t *roots_out, uint64_t *v_out, uint8_t *pcs_proof_out) {
    if (roots_out) std::memcpy(roots_out, p->p.z_comm.roots.data(), p->p.z_comm.roots.size() * 32);
    if (v_out)
        for (uint32_t i = 0; i < p->limbs; i++) v_out[i] = p->p.v[i];
    if (pcs_proof_out) std::memcpy(pcs_proof_out, p->p.pcs_proof.data(), p->p.pcs_proof.size());
}
void zinc_zip_proof_free(zinc_zip_proof *p) { delete p; }

int32_t zinc_sumcheck_prove_product(zinc_transcript *transcript, const uint64_t *const *mles, uint32_t n_mles,
                                    uint32_t nvars, uint32_t degree, const uint64_t *modulus, uint32_t limbs,
                                    int32_t device, uint64_t *msgs_out, uint64_t *randomness_out) {
    if (!transcript || !mles || !msgs_out || !randomness_out) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<const uint64_t *> tables(mles, mles + n_mles);
        const auto res = zinc::sumcheck::prove_as_subprotocol_product(transcript->t, tables, nvars, degree, f, device);
        for (size_t r = 0; r < res.proof.msgs.size(); r++) {
            for (uint32_t e = 0; e <= degree; e++)
                for (uint32_t i = 0; i < limbs; i++)
                    msgs_out[(r * (degree + 1) + e) * limbs + i] = res.proof.msgs[r][e][i];
            for (uint32_t i = 0; i < limbs; i++) randomness_out[r * limbs + i] = res.randomness[r][i];
        }
    });
}

int32_t zinc_sumcheck_prove_ccs(zinc_transcript *transcript, const uint64_t *const *mles, uint32_t n_mles,
                                uint32_t nvars, uint32_t degree, uint32_t n_terms, const uint64_t *c,
                                const uint32_t *s_masks, const uint64_t *modulus, uint32_t limbs, int32_t device,
                                uint64_t *msgs_out, uint64_t *randomness_out) {
    if (!transcript || !mles || !c || !s_masks || !msgs_out || !randomness_out) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<const uint64_t *> tables(mles, mles + n_mles);
        std::vector<Limbs> cv(n_terms);
        std::vector<std::vector<uint32_t>> S(n_terms);
        for (uint32_t t = 0; t < n_terms; t++) {
            cv[t] = load(c + (size_t)t * limbs, limbs);
            for (uint32_t j = 0; j < 32; j++)
                if ((s_masks[t] >> j) & 1u) S[t].push_back(j);
        }
        const auto res = zinc::sumcheck::prove_as_subprotocol_ccs(transcript->t, tables, nvars, degree, cv, S, f, device);
        for (size_t r = 0; r < res.proof.msgs.size(); r++) {
            for (uint32_t e = 0; e <= degree; e++)
                for (uint32_t i = 0; i < limbs; i++)
                    msgs_out[(r * (degree + 1) + e) * limbs + i] = res.proof.msgs[r][e][i];
            for (uint32_t i = 0; i < limbs; i++) randomness_out[r * limbs + i] = res.randomness[r][i];
        }
    });
}

int32_t zinc_sumcheck_prove_batch(zinc_transcript *const *transcripts, uint32_t n_instances, const uint64_t *const *mles,
                                  uint32_t n_mles, uint32_t nvars, uint32_t degree, const uint32_t *n_terms, const uint64_t *c,
                                  const uint32_t *s_masks, const uint64_t *moduli, const uint32_t *limbs, int32_t device,
                                  uint64_t *msgs_out, uint64_t *randomness_out) {
    if (!transcripts || !mles || !moduli || !limbs || !msgs_out || !randomness_out) return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n_instances; i++)
        if (!transcripts[i] || (n_terms && n_terms[i] && (!c || !s_masks))) return ZINC_ERR_NULL;
    return guarded([&] {
        std::vector<zinc::sumcheck::BatchInstance> inst(n_instances);
        for (uint32_t i = 0; i < n_instances; i++) {
            zinc::sumcheck::BatchInstance &b = inst[i];
            b.transcript = &transcripts[i]->t;
            b.mles.assign(mles + (size_t)i * n_mles, mles + (size_t)(i + 1) * n_mles);
            b.config = FieldConfig::make(moduli + (size_t)i * 4, limbs[i]);
            const uint32_t nt = n_terms ? n_terms[i] : 0;
            if (nt > 8) throw ZipError(ZipError::InvalidPcsParam, "more than 8 CCS terms in an instance of the batch");
            b.ccs = nt != 0;
            for (uint32_t t = 0; t < nt; t++) {
                b.c.push_back(load(c + ((size_t)i * 8 + t) * 4, limbs[i]));
                b.S.emplace_back();
                for (uint32_t j = 0; j < 32; j++)
                    if ((s_masks[(size_t)i * 8 + t] >> j) & 1u) b.S.back().push_back(j);
            }
        }
        const auto res = zinc::sumcheck::prove_as_subprotocol_batch(inst, nvars, degree, device);
        size_t m_at = 0, r_at = 0;  // instance-major, each instance with its own number of limbs
        for (uint32_t i = 0; i < n_instances; i++)
            for (size_t r = 0; r < res[i].proof.msgs.size(); r++) {
                for (uint32_t e = 0; e <= degree; e++)
                    for (uint32_t l = 0; l < limbs[i]; l++) msgs_out[m_at++] = res[i].proof.msgs[r][e][l];
                for (uint32_t l = 0; l < limbs[i]; l++) randomness_out[r_at++] = res[i].randomness[r][l];
            }
    });
}

int32_t zinc_sumcheck_prove_products(zinc_transcript *transcript, const uint64_t *const *mles, uint32_t n_mles,
                                     uint32_t nvars, uint32_t degree, uint32_t n_products, const uint64_t *coeffs,
                                     const uint32_t *masks, const uint64_t *modulus, uint32_t limbs, int32_t device,
                                     uint64_t *msgs_out, uint64_t *randomness_out) {
    if (!transcript || !mles || !coeffs || !masks || !msgs_out || !randomness_out) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        std::vector<const uint64_t *> tables(mles, mles + n_mles);
        std::vector<std::pair<Limbs, std::vector<uint32_t>>> products(n_products);
        for (uint32_t p = 0; p < n_products; p++) {
            products[p].first = load(coeffs + (size_t)p * limbs, limbs);
            for (uint32_t j = 0; j < 32; j++)
                if ((masks[p] >> j) & 1u) products[p].second.push_back(j);
        }
        const auto res = zinc::sumcheck::prove_as_subprotocol_products(transcript->t, tables, nvars, degree, products, f, device);
        for (size_t r = 0; r < res.proof.msgs.size(); r++) {
            for (uint32_t e = 0; e <= degree; e++)
                for (uint32_t i = 0; i < limbs; i++)
                    msgs_out[(r * (degree + 1) + e) * limbs + i] = res.proof.msgs[r][e][i];
            for (uint32_t i = 0; i < limbs; i++) randomness_out[r * limbs + i] = res.randomness[r][i];
        }
    });
}

int32_t zinc_sumcheck_verify(zinc_transcript *transcript, uint32_t nvars, uint32_t degree, const uint64_t *claimed_sum,
                             const uint64_t *msgs, uint32_t n_rounds, uint32_t evals_per_round, const uint64_t *modulus,
                             uint32_t limbs, uint64_t *point_out, uint64_t *expected_out) {
    if (!transcript || !claimed_sum || (n_rounds && !msgs)) return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        zinc::sumcheck::SumcheckProof proof;
        for (uint32_t r = 0; r < n_rounds; r++) {
            proof.msgs.emplace_back();
            for (uint32_t e = 0; e < evals_per_round; e++)
                proof.msgs.back().push_back(load(msgs + ((size_t)r * evals_per_round + e) * limbs, limbs));
        }
        const zinc::sumcheck::SubClaim claim =
            zinc::sumcheck::verify_as_subprotocol(transcript->t, nvars, degree, load(claimed_sum, limbs), proof, f);
        if (point_out)
            for (size_t i = 0; i < claim.point.size(); i++)
                for (uint32_t k = 0; k < limbs; k++) point_out[i * limbs + k] = claim.point[i][k];
        if (expected_out)
            for (uint32_t k = 0; k < limbs; k++) expected_out[k] = claim.expected_evaluation[k];
    });
}

namespace {
zinc::ccs::CCS_Z square_ccs(uint32_t t, uint32_t s) {
    zinc::ccs::CCS_Z ccs;
    ccs.m = ccs.n = (size_t)1 << s;
    ccs.s = ccs.s_prime = s;
    ccs.t = t;
    return ccs;
}
}  // namespace

struct zinc_prepared_ccs {
    std::unique_ptr<zinc::PreparedCcs> p;
    uint32_t t, s;
};

int32_t zinc_prover_prepare(const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, const uint64_t *modulus,
                            uint32_t limbs, int32_t device, zinc_prepared_ccs **out) {
    if (!constraints || !modulus || !out) return ZINC_ERR_NULL;
    *out = nullptr;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        *out = new zinc_prepared_ccs{std::make_unique<zinc::PreparedCcs>(constraints, t, s, f, device), t, s};
    });
}
void zinc_prepared_ccs_free(zinc_prepared_ccs *p) { delete p; }

int32_t zinc_prover_prove(const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, uint32_t d, uint32_t q,
                          const uint32_t *s_masks, const int64_t *c, const int64_t *public_input, size_t l,
                          const int64_t *w_ccs, size_t w_len, zinc_transcript *transcript, const uint64_t *modulus,
                          uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared, int32_t with_pcs,
                          uint64_t *msgs1_out, uint64_t *msgs2_out, uint64_t *v_s_out, uint64_t *r_y_out,
                          zinc_zip_proof **zip_proof_out) {
    return zinc_prover_prove_spec(nullptr, constraints, t, s, d, q, s_masks, c, public_input, l, w_ccs, w_len, transcript, modulus,
                                  limbs, device, prepared, with_pcs, msgs1_out, msgs2_out, v_s_out, r_y_out, zip_proof_out);
}
int32_t zinc_prover_prove_spec(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                               uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, const int64_t *public_input,
                               size_t l, const int64_t *w_ccs, size_t w_len, zinc_transcript *transcript,
                               const uint64_t *modulus, uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared,
                               int32_t with_pcs, uint64_t *msgs1_out, uint64_t *msgs2_out, uint64_t *v_s_out,
                               uint64_t *r_y_out, zinc_zip_proof **zip_proof_out) {
    if ((!constraints && !prepared) || !s_masks || !c || !transcript || !msgs1_out || !msgs2_out || !v_s_out || !r_y_out ||
        (l && !public_input) || (w_len && !w_ccs) || (with_pcs && !zip_proof_out))
        return ZINC_ERR_NULL;
    if (zip_proof_out) *zip_proof_out = nullptr;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        zinc::ccs::CCS_Z ccs = square_ccs(t, s);
        ccs.l = l;
        ccs.q = q;
        ccs.d = d;
        for (uint32_t i = 0; i < q; i++) {
            ccs.c.push_back(c[i]);
            ccs.S.emplace_back();
            for (uint32_t j = 0; j < 32; j++)
                if ((s_masks[i] >> j) & 1u) ccs.S.back().push_back(j);
        }
        zinc::ccs::Statement_Z st;
        st.constraints.resize(t);  // the matrices go to the device straight from the caller's arrays
        st.public_input.assign(public_input, public_input + l);
        std::unique_ptr<zinc::PreparedCcs> own;  // per proof, as the reference maps the matrices per proof
        if (!prepared) own = std::make_unique<zinc::PreparedCcs>(constraints, t, s, f, device);
        zinc::PreparedCcs *prep = prepared ? prepared->p.get() : own.get();
        const zinc::IntVec z = zinc::ZincProver::get_z_ccs(public_input, l, w_ccs, w_len, ccs.m);  // x || 1 || w
        const zinc::ZincProver prover(spec_of(spec), device);
        zinc::SpartanProof sp;
        std::vector<Limbs> r_y;
        if (with_pcs) {
            auto proof = prover.prove_z(st, z.data(), z.size(), transcript->t, ccs, f, &r_y, prep);
            sp = std::move(proof.spartan_proof);
            *zip_proof_out = new zinc_zip_proof{std::move(proof.zip_proof), limbs};
        } else {
            auto res = prover.spartan_prove(st, z.data(), z.size(), transcript->t, ccs, f, prep);
            sp = std::move(res.first);
            r_y = std::move(res.second);
        }
        auto put = [&](uint64_t *dst, const Limbs &v) {
            for (uint32_t i = 0; i < limbs; i++) dst[i] = v[i];
        };
        for (size_t r = 0; r < sp.linearization_sumcheck.msgs.size(); r++)
            for (uint32_t e = 0; e <= d + 1; e++) put(msgs1_out + (r * (d + 2) + e) * limbs, sp.linearization_sumcheck.msgs[r][e]);
        for (size_t r = 0; r < sp.second_sumcheck.msgs.size(); r++)
            for (uint32_t e = 0; e < 3; e++) put(msgs2_out + (r * 3 + e) * limbs, sp.second_sumcheck.msgs[r][e]);
        for (size_t k = 0; k < sp.V_s.size(); k++) put(v_s_out + k * limbs, sp.V_s[k]);
        for (size_t i = 0; i < r_y.size(); i++) put(r_y_out + i * limbs, r_y[i]);
    });
}

int32_t zinc_prover_prove_batch(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, uint32_t n_instances,
                                const int64_t *const *public_inputs, const size_t *l, const int64_t *const *w_ccs,
                                const size_t *w_len, zinc_transcript *const *transcripts, const uint64_t *moduli,
                                const uint32_t *limbs, int32_t device, int32_t with_pcs, uint64_t *msgs1_out, uint64_t *msgs2_out,
                                uint64_t *v_s_out, uint64_t *r_y_out, zinc_zip_proof **zip_proofs_out) {
    if (!constraints || !s_masks || !c || !public_inputs || !l || !w_ccs || !w_len || !transcripts || !moduli || !limbs ||
        !msgs1_out || !msgs2_out || !v_s_out || !r_y_out || (with_pcs && !zip_proofs_out))
        return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n_instances; i++) {
        if (!transcripts[i] || (l[i] && !public_inputs[i]) || (w_len[i] && !w_ccs[i])) return ZINC_ERR_NULL;
        if (zip_proofs_out) zip_proofs_out[i] = nullptr;
    }
    return guarded([&] {
        zinc::ccs::CCS_Z ccs = square_ccs(t, s);
        ccs.q = q;
        ccs.d = d;
        for (uint32_t i = 0; i < q; i++) {
            ccs.c.push_back(c[i]);
            ccs.S.emplace_back();
            for (uint32_t j = 0; j < 32; j++)
                if ((s_masks[i] >> j) & 1u) ccs.S.back().push_back(j);
        }
        std::vector<zinc::IntVec> z(n_instances);
        std::vector<zinc::ZincProver::ZVector> zs(n_instances);
        std::vector<zinc::KeccakTranscript *> tr(n_instances);
        std::vector<FieldConfig> f;
        for (uint32_t i = 0; i < n_instances; i++) {
            z[i] = zinc::ZincProver::get_z_ccs(public_inputs[i], l[i], w_ccs[i], w_len[i], ccs.m);  // x || 1 || w
            zs[i] = {z[i].data(), z[i].size()};
            tr[i] = &transcripts[i]->t;
            f.push_back(FieldConfig::make(moduli + (size_t)i * 4, limbs[i]));
        }
        const zinc::ZincProver prover(spec_of(spec), device);
        std::vector<zinc::SpartanProof> sp(n_instances);
        std::vector<std::vector<Limbs>> r_y(n_instances);
        if (with_pcs) {
            auto proofs = prover.prove_batch(constraints, ccs, zs, tr, f, &r_y);
            for (uint32_t i = 0; i < n_instances; i++) {
                sp[i] = std::move(proofs[i].spartan_proof);
                zip_proofs_out[i] = new zinc_zip_proof{std::move(proofs[i].zip_proof), limbs[i]};
            }
        } else {
            auto res = prover.spartan_prove_batch(constraints, ccs, zs, tr, f);
            for (uint32_t i = 0; i < n_instances; i++) {
                sp[i] = std::move(res[i].first);
                r_y[i] = std::move(res[i].second);
            }
        }
        size_t m1 = 0, m2 = 0, vs = 0, ry = 0;  // instance-major, each instance with its own number of limbs
        for (uint32_t i = 0; i < n_instances; i++) {
            auto put = [&](uint64_t *dst, size_t &at, const Limbs &v) {
                for (uint32_t k = 0; k < limbs[i]; k++) dst[at++] = v[k];
            };
            for (const auto &round : sp[i].linearization_sumcheck.msgs)
                for (uint32_t e = 0; e <= d + 1; e++) put(msgs1_out, m1, round[e]);
            for (const auto &round : sp[i].second_sumcheck.msgs)
                for (uint32_t e = 0; e < 3; e++) put(msgs2_out, m2, round[e]);
            for (const Limbs &v : sp[i].V_s) put(v_s_out, vs, v);
            for (const Limbs &v : r_y[i]) put(r_y_out, ry, v);
        }
    });
}

int32_t zinc_prover_pcs_step_batch(const zinc_linear_code_spec *spec, uint32_t s, uint32_t n_instances, const int64_t *const *z,
                                   const size_t *z_len, const uint64_t *r_y, zinc_transcript *const *transcripts,
                                   const uint64_t *moduli, const uint32_t *limbs, int32_t device, zinc_zip_proof **zip_proofs_out) {
    if (!z || !z_len || !r_y || !transcripts || !moduli || !limbs || !zip_proofs_out) return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n_instances; i++) {
        if (!transcripts[i] || (z_len[i] && !z[i])) return ZINC_ERR_NULL;
        zip_proofs_out[i] = nullptr;
    }
    return guarded([&] {
        const zinc::ccs::CCS_Z ccs = square_ccs(1, s);  // (the PCS step reads m and s_prime alone)
        std::vector<zinc::ZincProver::ZVector> zs(n_instances);
        std::vector<zinc::KeccakTranscript *> tr(n_instances);
        std::vector<std::vector<Limbs>> points(n_instances);
        std::vector<FieldConfig> f;
        size_t at = 0;
        for (uint32_t i = 0; i < n_instances; i++) {
            zs[i] = {z[i], z_len[i]};
            tr[i] = &transcripts[i]->t;
            f.push_back(FieldConfig::make(moduli + (size_t)i * 4, limbs[i]));
            points[i].assign(s, Limbs{});
            for (uint32_t k = 0; k < s; k++)
                for (uint32_t j = 0; j < limbs[i]; j++) points[i][k][j] = r_y[at++];
        }
        auto proofs = zinc::ZincProver(spec_of(spec), device).pcs_step_batch(ccs, zs, points, tr, f);
        for (uint32_t i = 0; i < n_instances; i++) zip_proofs_out[i] = new zinc_zip_proof{std::move(proofs[i]), limbs[i]};
    });
}

}  // extern "C"
namespace {
// zinc_verifier_verify_batch (public_inputs == nullptr) and zinc_verifier_verify_batch_checked
int32_t verify_batch_impl(const int64_t *const *public_inputs, const size_t *public_input_lens,
                          const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                          uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, uint32_t n_instances,
                          zinc_transcript *const *transcripts, const uint64_t *moduli, const uint32_t *limbs,
                          int32_t device, const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s,
                          const uint8_t *const *roots, const size_t *n_roots, const uint64_t *v,
                          const uint8_t *const *pcs_proofs, const size_t *pcs_proof_lens, int32_t *results_out,
                          char *messages_out, size_t message_cap) {
    if (!constraints || !s_masks || !c || !transcripts || !moduli || !limbs || !msgs1 || !msgs2 || !v_s || !roots || !n_roots || !v ||
        !pcs_proofs || !pcs_proof_lens || !results_out || (messages_out && !message_cap))
        return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n_instances; i++)
        if (!transcripts[i] || (n_roots[i] && !roots[i]) || (pcs_proof_lens[i] && !pcs_proofs[i])) return ZINC_ERR_NULL;
    return guarded([&] {
        zinc::ccs::CCS_Z ccs = square_ccs(t, s);
        ccs.q = q;
        ccs.d = d;
        for (uint32_t i = 0; i < q; i++) {
            ccs.c.push_back(c[i]);
            ccs.S.emplace_back();
            for (uint32_t j = 0; j < 32; j++)
                if ((s_masks[i] >> j) & 1u) ccs.S.back().push_back(j);
        }
        std::vector<zinc::SpartanProof> sp(n_instances);
        std::vector<zinc::zip::MultilinearZipCommitment> comms(n_instances);
        std::vector<Limbs> vs(n_instances);
        std::vector<zinc::ZincVerifier::BatchProof> proofs(n_instances);
        std::vector<zinc::KeccakTranscript *> tr(n_instances);
        std::vector<FieldConfig> f;
        size_t m1 = 0, m2 = 0, at_vs = 0, at_v = 0;  // instance-major, each instance with its own number of limbs
        for (uint32_t i = 0; i < n_instances; i++) {
            const uint32_t fl = limbs[i];
            f.push_back(FieldConfig::make(moduli + (size_t)i * 4, fl));
            auto take = [&](const uint64_t *src, size_t &at, size_t rounds, size_t per) {
                zinc::sumcheck::SumcheckProof p;
                for (size_t r = 0; r < rounds; r++) {
                    p.msgs.emplace_back();
                    for (size_t e = 0; e < per; e++, at += fl) p.msgs.back().push_back(load(src + at, fl));
                }
                return p;
            };
            sp[i].linearization_sumcheck = take(msgs1, m1, s, d + 2);
            sp[i].second_sumcheck = take(msgs2, m2, s, 3);
            for (uint32_t k = 0; k < t; k++, at_vs += fl) sp[i].V_s.push_back(load(v_s + at_vs, fl));
            vs[i] = load(v + at_v, fl);
            at_v += fl;
            comms[i].roots.resize(n_roots[i]);
            if (n_roots[i]) std::memcpy(comms[i].roots.data(), roots[i], n_roots[i] * 32);
            proofs[i] = {&sp[i], &comms[i], &vs[i], pcs_proofs[i], pcs_proof_lens[i]};  // the proof bytes are read in place
            tr[i] = &transcripts[i]->t;
        }
        const zinc::ZincVerifier verifier(spec_of(spec), device);
        std::vector<zinc::ZincVerifier::BatchOutcome> outcomes;
        if (public_inputs) {
            const std::vector<const int64_t *> x(public_inputs, public_inputs + n_instances);
            const std::vector<size_t> l(public_input_lens, public_input_lens + n_instances);
            outcomes = verifier.verify_batch_checked(constraints, ccs, x, l, proofs, tr, f);
        } else {
            outcomes = verifier.verify_batch(constraints, ccs, proofs, tr, f);
        }
        for (uint32_t i = 0; i < n_instances; i++) {
            const auto &o = outcomes[i];
            using O = zinc::ZincVerifier::BatchOutcome;
            results_out[i] = o.kind == O::Accepted  ? ZINC_OK
                             : o.kind == O::Spartan ? ZINC_ERR_SPARTAN
                             : o.kind == O::FieldConfig ? ZINC_ERR_FIELD_CONFIG
                             : o.zip_kind == ZipError::InvalidPcsParam ? ZINC_ERR_INVALID_PARAM
                                                                       : ZINC_ERR_INVALID_OPEN;
            if (messages_out) {
                char *dst = messages_out + (size_t)i * message_cap;
                const size_t n = std::min(o.message.size(), message_cap - 1);
                std::memcpy(dst, o.message.data(), n);
                dst[n] = 0;
            }
        }
    });
}
}  // namespace
extern "C" {

int32_t zinc_verifier_verify_batch(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                   uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, uint32_t n_instances,
                                   zinc_transcript *const *transcripts, const uint64_t *moduli, const uint32_t *limbs,
                                   int32_t device, const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s,
                                   const uint8_t *const *roots, const size_t *n_roots, const uint64_t *v,
                                   const uint8_t *const *pcs_proofs, const size_t *pcs_proof_lens, int32_t *results_out,
                                   char *messages_out, size_t message_cap) {
    return verify_batch_impl(nullptr, nullptr, spec, constraints, t, s, d, q, s_masks, c, n_instances, transcripts, moduli, limbs, device,
                             msgs1, msgs2, v_s, roots, n_roots, v, pcs_proofs, pcs_proof_lens, results_out, messages_out, message_cap);
}
int32_t zinc_verifier_verify_batch_checked(const int64_t *const *public_inputs, const size_t *public_input_lens,
                                           const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t,
                                           uint32_t s, uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c,
                                           uint32_t n_instances, zinc_transcript *const *transcripts, const uint64_t *moduli,
                                           const uint32_t *limbs, int32_t device, const uint64_t *msgs1, const uint64_t *msgs2,
                                           const uint64_t *v_s, const uint8_t *const *roots, const size_t *n_roots, const uint64_t *v,
                                           const uint8_t *const *pcs_proofs, const size_t *pcs_proof_lens, int32_t *results_out,
                                           char *messages_out, size_t message_cap) {
    if (!public_inputs || !public_input_lens) return ZINC_ERR_NULL;
    for (uint32_t i = 0; i < n_instances; i++)
        if (public_input_lens[i] && !public_inputs[i]) return ZINC_ERR_NULL;
    return verify_batch_impl(public_inputs, public_input_lens, spec, constraints, t, s, d, q, s_masks, c, n_instances, transcripts,
                             moduli, limbs, device, msgs1, msgs2, v_s, roots, n_roots, v, pcs_proofs, pcs_proof_lens, results_out,
                             messages_out, message_cap);
}

int32_t zinc_verifier_verify(const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, uint32_t d, uint32_t q,
                             const uint32_t *s_masks, const int64_t *c, zinc_transcript *transcript, const uint64_t *modulus,
                             uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared, const uint64_t *msgs1,
                             const uint64_t *msgs2, const uint64_t *v_s, int32_t with_pcs, const uint8_t *roots,
                             size_t n_roots, const uint64_t *v, const uint8_t *pcs_proof, size_t pcs_proof_len,
                             uint64_t *rx_ry_out, uint64_t *e_y_out, uint64_t *gamma_out) {
    return zinc_verifier_verify_checked(nullptr, 0, 0, constraints, t, s, d, q, s_masks, c, transcript, modulus, limbs, device,
                                        prepared, msgs1, msgs2, v_s, with_pcs, roots, n_roots, v, pcs_proof, pcs_proof_len,
                                        rx_ry_out, e_y_out, gamma_out);
}
int32_t zinc_verifier_verify_spec(const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                  uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, zinc_transcript *transcript,
                                  const uint64_t *modulus, uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared,
                                  const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s, int32_t with_pcs,
                                  const uint8_t *roots, size_t n_roots, const uint64_t *v, const uint8_t *pcs_proof,
                                  size_t pcs_proof_len, uint64_t *rx_ry_out, uint64_t *e_y_out, uint64_t *gamma_out) {
    return zinc_verifier_verify_checked_spec(spec, nullptr, 0, 0, constraints, t, s, d, q, s_masks, c, transcript, modulus, limbs,
                                             device, prepared, msgs1, msgs2, v_s, with_pcs, roots, n_roots, v, pcs_proof,
                                             pcs_proof_len, rx_ry_out, e_y_out, gamma_out);
}

int32_t zinc_verifier_verify_checked(const int64_t *public_input, size_t l, int32_t check_field,
                                     const zip_sparse_matrix *constraints, uint32_t t, uint32_t s, uint32_t d, uint32_t q,
                                     const uint32_t *s_masks, const int64_t *c, zinc_transcript *transcript,
                                     const uint64_t *modulus, uint32_t limbs, int32_t device, zinc_prepared_ccs *prepared,
                                     const uint64_t *msgs1, const uint64_t *msgs2, const uint64_t *v_s, int32_t with_pcs,
                                     const uint8_t *roots, size_t n_roots, const uint64_t *v, const uint8_t *pcs_proof,
                                     size_t pcs_proof_len, uint64_t *rx_ry_out, uint64_t *e_y_out, uint64_t *gamma_out) {
    return zinc_verifier_verify_checked_spec(nullptr, public_input, l, check_field, constraints, t, s, d, q, s_masks, c, transcript,
                                             modulus, limbs, device, prepared, msgs1, msgs2, v_s, with_pcs, roots, n_roots, v,
                                             pcs_proof, pcs_proof_len, rx_ry_out, e_y_out, gamma_out);
}
int32_t zinc_verifier_verify_checked_spec(const zinc_linear_code_spec *spec, const int64_t *public_input, size_t l,
                                          int32_t check_field, const zip_sparse_matrix *constraints, uint32_t t, uint32_t s,
                                          uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c,
                                          zinc_transcript *transcript, const uint64_t *modulus, uint32_t limbs, int32_t device,
                                          zinc_prepared_ccs *prepared, const uint64_t *msgs1, const uint64_t *msgs2,
                                          const uint64_t *v_s, int32_t with_pcs, const uint8_t *roots, size_t n_roots,
                                          const uint64_t *v, const uint8_t *pcs_proof, size_t pcs_proof_len, uint64_t *rx_ry_out,
                                          uint64_t *e_y_out, uint64_t *gamma_out) {
    if ((!constraints && !prepared && with_pcs) || !s_masks || !c || !transcript || !msgs1 || !msgs2 || !v_s ||
        (with_pcs && (!roots || !v || !pcs_proof)) || (check_field && l && !public_input))
        return ZINC_ERR_NULL;
    return guarded([&] {
        const FieldConfig f = FieldConfig::make(modulus, limbs);
        if (check_field)  // verifier.rs:53-57, before any other work
            zinc::ZincVerifier(spec_of(spec), device).check_field(public_input, l, transcript->t, f);
        zinc::ccs::CCS_Z ccs = square_ccs(t, s);
        ccs.q = q;
        ccs.d = d;
        for (uint32_t i = 0; i < q; i++) {
            ccs.c.push_back(c[i]);
            ccs.S.emplace_back();
            for (uint32_t j = 0; j < 32; j++)
                if ((s_masks[i] >> j) & 1u) ccs.S.back().push_back(j);
        }
        zinc::SpartanProof sp;
        auto take = [&](const uint64_t *src, size_t rounds, size_t per) {
            zinc::sumcheck::SumcheckProof p;
            for (size_t r = 0; r < rounds; r++) {
                p.msgs.emplace_back();
                for (size_t e = 0; e < per; e++) p.msgs.back().push_back(load(src + (r * per + e) * limbs, limbs));
            }
            return p;
        };
        sp.linearization_sumcheck = take(msgs1, s, d + 2);
        sp.second_sumcheck = take(msgs2, s, 3);
        for (uint32_t k = 0; k < t; k++) sp.V_s.push_back(load(v_s + (size_t)k * limbs, limbs));
        const zinc::ZincVerifier verifier(spec_of(spec), device);
        const zinc::VerificationPoints pts = verifier.spartan_verify(sp, ccs, transcript->t, f);
        auto put = [&](uint64_t *dst, const Limbs &x) {
            if (dst)
                for (uint32_t i = 0; i < limbs; i++) dst[i] = x[i];
        };
        if (rx_ry_out)
            for (size_t i = 0; i < pts.rx_ry.size(); i++) put(rx_ry_out + i * limbs, pts.rx_ry[i]);
        put(e_y_out, pts.e_y);
        put(gamma_out, pts.gamma);
        if (!with_pcs) return;
        zinc::ccs::Statement_Z st;
        st.constraints.resize(t);
        std::unique_ptr<zinc::PreparedCcs> own;
        if (!prepared) own = std::make_unique<zinc::PreparedCcs>(constraints, t, s, f, device);
        zinc::zip::MultilinearZipCommitment z_comm;
        z_comm.roots.resize(n_roots);
        std::memcpy(z_comm.roots.data(), roots, n_roots * 32);
        verifier.verify_pcs_proof(st, z_comm, load(v, limbs), pcs_proof, pcs_proof_len, pts, ccs, transcript->t, f,
                                  prepared ? prepared->p.get() : own.get());  // the proof bytes are read in place
    });
}

}  // extern "C"
