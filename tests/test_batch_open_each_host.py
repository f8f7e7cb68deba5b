"""zip_batch_open_each without a device: the two symbols are exported and declared as include/zip_hip.h states them, the
Python side exists, the mirror's batched PCS step calls the new entry point, and a stand-alone C++ caller
(tests/native/batch_open_each_check.cpp, built with the address and undefined-behaviour sanitizers) gets the documented
answer on a machine that has no GPU.  What needs a live batch is in tests/test_gpu_batch_open_each.py, the prover's use of
it in tests/test_gpu_pcs_step_batch_each.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

from zinc_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (return type, parameter list) exactly as the header declares it, whitespace collapsed
SIGNATURES = {
    "zip_batch_open_each": ("int32_t", "zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, "
                                       "const uint64_t *q0_mont, const zip_field *const *fields, uint8_t *const *proofs_out, "
                                       "zip_mem_kind out_kind, size_t window_bytes"),
    "zip_batch_open_each_counts": ("void", "uint64_t *calls, uint64_t *members, uint64_t *windows, uint64_t *last_staging_bytes"),
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
    assert re.search(r"#define ZIP_HIP_ABI_VERSION 3\b", text)
    # the Python side of them
    assert callable(cabi.Batch.open_each) and callable(cabi.batch_open_each_counts)
    counts = cabi.batch_open_each_counts()
    assert len(counts) == 4
    a = C.c_uint64(7)
    cabi.lib().zip_batch_open_each_counts(None, None, C.byref(a), None)
    assert a.value == counts[2]
    # no batch: ZIP_ERR_NULL before anything else is looked at
    assert cabi.lib().zip_batch_open_each(None, None, None, 3, None, None, None, cabi.MEM_HOST, 0) == cabi.ZIP_ERR_NULL


def test_the_mirrors_batched_pcs_step_delivers_stream_by_stream():
    """step 5 of commit_z_mle_and_prove_evaluation_batch hands the ZipProofs' own bytes to ONE zip_batch_open_each; the
    block of B streams and its cut are gone.  (MultilinearZip::batch_open keeps zip_batch_open: one shared stream.)"""
    src = open(os.path.join(ROOT, "zinc_amd", "host", "zinc_zip.cpp")).read()
    start = src.index("zip::commit_z_mle_and_prove_evaluation_batch(const LinearCodeSpec")
    body = src[start: src.index("\nnamespace {", start)]
    assert body.count("zip_batch_open_each(") == 1
    assert "zip_batch_open_fields(" not in body and "ByteStream streams" not in body
    assert "zip_batch_open(" in src


def test_the_entry_point_answers_a_c_caller_without_a_device(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    lib_dir = os.path.dirname(cabi.lib()._name)
    exe = str(tmp_path / "batch_open_each_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "native", "batch_open_each_check.cpp"),
           f"-L{lib_dir}", "-lzip_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # (the program touches no device; what the HIP runtime allocates while the library loads is not this test's to count)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "batch_open_each_check ok" in r.stdout
