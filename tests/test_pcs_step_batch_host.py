"""The batch family with a code and a field per member, without a device: the symbols are exported and declared as
include/zip_hip.h states them, and a stand-alone C++ caller (tests/native/batch_codes_check.cpp, built with the address and
undefined-behaviour sanitizers) gets the documented answer from every entry point on a machine that has no GPU.  What
needs a live ctx is in tests/test_gpu_batch_codes.py, the prover's use of it in tests/test_gpu_pcs_step_batch.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

from zinc_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (return type, parameter list) exactly as the header declares it, whitespace collapsed
SIGNATURES = {
    "zip_batch_commit_codes": ("int32_t", "zip_ctx *ctx, const int64_t *evals, size_t n_evals, uint32_t n_polys, zip_mem_kind evals_kind, "
                                          "const uint32_t *perms1, const uint32_t *perms2, uint8_t *roots_out, zip_batch **out"),
    "zip_batch_open_eval_fields": ("int32_t", "zip_batch *b, const uint64_t *q0_mont, const zip_field *const *fields, uint64_t *rows_out, "
                                              "zip_mem_kind out_kind"),
    "zip_batch_open_fields": ("int32_t", "zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, "
                                         "const uint64_t *q0_mont, const zip_field *const *fields, uint8_t *proofs_out, zip_mem_kind out_kind"),
    "zip_batch_codes_counts": ("void", "uint64_t *commits, uint64_t *members, uint64_t *field_opens"),
}


def test_symbols_exported_and_declared_with_the_headers_signatures():
    text = open(os.path.join(ROOT, "include", "zip_hip.h")).read()
    for name, (ret, params) in SIGNATURES.items():
        assert name in cabi.EXPORTED_SYMBOLS, name
        assert hasattr(cabi.lib(), name), name
        m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^;]*)\);", text, re.M)
        assert m, name
        assert m.group(1) == ret, name
        assert " ".join(m.group(2).split()) == params, name
    assert cabi.lib().zip_abi_version() == 3
    # the Python side of them
    assert callable(cabi.ZipContext.batch_commit_codes) and callable(cabi.Batch.open_eval_fields) and callable(cabi.Batch.open_fields)
    a = C.c_uint64(7)
    cabi.lib().zip_batch_codes_counts(None, C.byref(a), None)
    assert a.value == cabi.batch_codes_counts()[1]


def test_the_host_mirror_exports_what_prove_batch_needs():
    from zinc_amd import pcs

    assert "zinc_prover_pcs_step_batch" in pcs.EXPORTED_SYMBOLS
    assert hasattr(pcs.lib(), "zinc_prover_pcs_step_batch") and hasattr(pcs.lib(), "zinc_prover_prove_batch")
    assert callable(pcs.ZincProver.pcs_step_batch)
    header = open(os.path.join(ROOT, "include", "zinc_zip_host.h")).read()
    assert re.search(r"\bzinc_prover_pcs_step_batch\s*\(", header)
    knobs = open(os.path.join(ROOT, "README.md")).read()
    assert "ZIP_HIP_PCS_MIN_BATCH" in knobs


def test_every_entry_point_answers_a_c_caller_without_a_device(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    lib_dir = os.path.dirname(cabi.lib()._name)
    exe = str(tmp_path / "batch_codes_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "native", "batch_codes_check.cpp"),
           f"-L{lib_dir}", "-lzip_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # (the program touches no device; what the HIP runtime allocates while the library loads is not this test's to count)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "batch_codes_check ok" in r.stdout
