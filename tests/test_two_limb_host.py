"""Two-limb witnesses without a device: a stand-alone C++ caller (tests/native/two_limb_check.cpp, built with the address
and undefined-behaviour sanitizers) gets the documented answer from zip_ctx_create's admission, from every refusal that
needs no ctx and from every two-limb entry point's NULL checks; and the test helpers' own model of the verifier agrees
with the CPU oracle.  What needs a live ctx is in tests/test_gpu_two_limb_*.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _oracle as orc
import _two_limb as tl
from zinc_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_point_answers_a_c_caller_without_a_device(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    lib_dir = os.path.dirname(cabi.lib()._name)
    exe = str(tmp_path / "two_limb_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "native", "two_limb_check.cpp"),
           f"-L{lib_dir}", "-lzip_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # (the program makes no ctx; what the HIP runtime allocates while the library loads is not this test's to count)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "two_limb_check ok" in r.stdout


def test_witness_builders_plant_the_extremes():
    z = tl.Zip2(8)
    w = tl.to_ints(tl.witness(z, "random"))
    C_, n = z.row_len, z.row_len * z.num_rows
    assert [w[0], w[C_ - 1], w[n - C_], w[n - 1]] == [tl.INT2_MIN, tl.INT2_MAX, 0, -1]
    assert set(tl.to_ints(tl.witness(z, "max"))) == {tl.INT2_MAX} and set(tl.to_ints(tl.witness(z, "min"))) == {tl.INT2_MIN}
    low = tl.witness(z, "lowtop")
    assert not low[:, 1].any() and (low[:, 0] >> np.uint64(63)).all()
    w1 = tl.to_ints(tl.witness(tl.Zip2(1), "random"))
    assert w1 == [tl.INT2_MIN, tl.INT2_MAX]


@pytest.mark.parametrize("modulus,fl", tl.MODULI + [(tl.MOD_M127, 2)])
def test_the_two_maps_in_python_integers(modulus, fl):
    """orc_field_from_int as the issue reads it: Int<2> over W = fl words (the signed modulus bites when the top bit is
    set and 2^(64 fl) - q <= |w|), Int<8> over 8 words (plain |v| mod q) -- so the values the GPU test feeds
    zip_field_map_int do reach both sides of every edge."""
    f = orc.make_field(modulus, fl)
    rm = (1 << (64 * fl)) % modulus
    top = modulus >> (64 * fl - 1)
    m = (1 << (64 * fl)) - modulus if top else modulus
    bites = plain = 0
    for width in (2, 8):
        for limbs, v in zip(tl.field_map_values(modulus, fl, width, n=96), tl.to_ints(tl.field_map_values(modulus, fl, width, n=96))):
            mag = abs(v)
            red = mag % (m if width == 2 else modulus)
            want = red * rm % modulus
            if v < 0 and want:
                want = modulus - want
            assert orc.limbs_to_int(orc.field_from_int(f, limbs)) == want, (width, v)
            if width == 2 and top:
                bites += mag >= m
                plain += mag < m
    if top and m < (1 << 127):
        assert bites and plain  # both sides of 2^(64 fl) - q


@pytest.mark.parametrize("modulus,fl", tl.VERIFY_MODULI)
def test_the_model_agrees_with_the_oracle_on_honest_and_tampered_proofs(modulus, fl):
    inst = tl.instance(8, modulus, fl)
    assert inst.oracle_rc(inst.proof, inst.roots, inst.ev) == 0
    assert inst.expect(inst.proof, inst.roots, inst.ev) == dict(verdict=tl.ACCEPT, column=0, bad_merkle_paths=0, malformed_paths=0)
    flipped = inst.proof.copy()
    flipped[inst.val_at(3, 2)] ^= 1
    assert inst.oracle_rc(flipped, inst.roots, inst.ev) != 0
    for name, mutate, claim in tl.tamper_cases(inst) + [tl.overflow_case(inst)]:
        proof, roots, ev = mutate(inst.proof, inst.roots, inst.ev)
        want = inst.expect(proof, roots, ev)
        for key, value in claim.items():
            assert want[key] == value, (name, want, claim)
        rc = inst.oracle_rc(proof, roots, ev)
        assert rc != 0, name
        if want["verdict"] == tl.OVERFLOW:
            assert rc == orc.ORC_ERR_OVERFLOW, name


def test_proximity_coefficients_use_both_limbs():
    inst = tl.instance(8, tl.BENCH_MODULUS, 4)
    assert inst.coeffs[:, 1].any() and any(c < 0 for c in inst.coeffs_int) and any(c >= 1 << 64 for c in inst.coeffs_int)
