"""The batched Zinc verifier without a device: the new symbols are exported and declared as the two headers state them, the
knob is documented, and a stand-alone C++ caller (tests/native/verify_batch_check.cpp, built with the address and
undefined-behaviour sanitizers, nothing preloaded) gets the documented answer from every new entry point on a machine that
has no GPU.  What needs a live handle is in tests/test_gpu_batch_verify_codes.py and tests/test_gpu_ccs_batch_eval.py, the
verifier's use of both in tests/test_gpu_verify_batch.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

from zinc_amd import cabi, pcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (return type, parameter list) exactly as the header declares it, whitespace collapsed
ZIP_SIGNATURES = {
    "zip_batch_verify_codes": ("int32_t", "zip_ctx *ctx, uint32_t n_polys, const uint32_t *perms1, const uint32_t *perms2, "
                                          "const uint8_t *roots, const uint8_t *const *proofs, const size_t *proof_lens, "
                                          "zip_mem_kind proofs_kind, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, "
                                          "const uint64_t *q0_mont, const uint64_t *q1_mont, const uint64_t *evals_mont, "
                                          "const zip_field *const *fields, zip_verify_report *reports"),
    "zip_batch_verify_codes_counts": ("void", "uint64_t *calls, uint64_t *members"),
    "zip_ccs_batch_eval_matrices": ("int32_t", "zip_ccs_batch *b, const zip_field *const *fields, uint32_t n, const uint64_t *r_x, "
                                               "const uint64_t *r_y, uint64_t *v_xy_out"),
}
ZINC_SIGNATURES = {
    "zinc_verifier_verify_batch": ("int32_t", "const zinc_linear_code_spec *spec, const zip_sparse_matrix *constraints, uint32_t t, "
                                              "uint32_t s, uint32_t d, uint32_t q, const uint32_t *s_masks, const int64_t *c, "
                                              "uint32_t n_instances, zinc_transcript *const *transcripts, const uint64_t *moduli, "
                                              "const uint32_t *limbs, int32_t device, const uint64_t *msgs1, const uint64_t *msgs2, "
                                              "const uint64_t *v_s, const uint8_t *const *roots, const size_t *n_roots, "
                                              "const uint64_t *v, const uint8_t *const *pcs_proofs, const size_t *pcs_proof_lens, "
                                              "int32_t *results_out, char *messages_out, size_t message_cap"),
}


def _declared(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^;]*)\);", text, re.M)
    assert m, name
    return m.group(1), " ".join(m.group(2).split())


def test_symbols_exported_and_declared_with_the_headers_signatures():
    for name, want in ZIP_SIGNATURES.items():
        assert name in cabi.EXPORTED_SYMBOLS, name
        assert hasattr(cabi.lib(), name), name
        assert _declared("zip_hip.h", name) == want, name
    for name, want in ZINC_SIGNATURES.items():
        assert name in pcs.EXPORTED_SYMBOLS, name
        assert hasattr(pcs.lib(), name), name
        assert _declared("zinc_zip_host.h", name) == want, name
    assert cabi.lib().zip_abi_version() == 3
    # the Python side of them
    assert callable(cabi.ZipContext.batch_verify_codes) and callable(cabi.CcsBatch.eval_matrices)
    assert callable(pcs.ZincVerifier.verify_batch)
    a = C.c_uint64(7)
    cabi.lib().zip_batch_verify_codes_counts(None, C.byref(a))
    assert a.value == cabi.batch_verify_codes_counts()[1]


def test_the_knob_and_the_entry_points_are_documented():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ZIP_HIP_VERIFY_MIN_BATCH" in readme
    header = open(os.path.join(ROOT, "include", "zip_hip.h")).read()
    # the two "Not part of" paragraphs no longer name what now exists
    assert "until then such" not in header and "the verifier's V_xy (zip_ccs_eval_matrices)\n * in a batch" not in header


def test_every_entry_point_answers_a_c_caller_without_a_device(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    lib_dir = os.path.dirname(cabi.lib()._name)
    assert os.path.dirname(pcs.lib()._name) == lib_dir
    exe = str(tmp_path / "verify_batch_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "native", "verify_batch_check.cpp"),
           f"-L{lib_dir}", "-lzinc_zip", "-lzip_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # (the program touches no device; what the HIP runtime allocates while the library loads is not this test's to count)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("ZIP_HIP_BATCH", None)
    env.pop("ZIP_HIP_VERIFY_MIN_BATCH", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "verify_batch_check ok" in r.stdout
