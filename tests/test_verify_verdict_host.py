"""CPU: zinc_amd/csrc/verify_verdict.h -- the one place the library turns the verifier's reduced facts into a verdict and
a failing column, for zip_verify's host code and batch_verify_report_kernel alike -- compiled for the host and held, over
every combination of the facts, to the order tests/_verify_cases.py's Model.report applies (which
test_verify_cases_host.py holds to the oracle)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

import _verify_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vv(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    so = str(tmp_path_factory.mktemp("verify_verdict") / "libverify_verdict_check.so")
    cmd = [cxx, "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{os.path.join(ROOT, 'zinc_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "native", "verify_verdict_check.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return C.CDLL(so)


def test_every_combination_of_the_facts_gives_the_models_verdict(vv):
    whys = [w for w in range(1, 8)]  # every non-empty subset of {proximity, malformed, Merkle}
    firsts = [(None, 0)] + [(k, w) for k in (3, 11) for w in whys]
    n = 0
    for overflow, (first, why), eval_differs, noncanonical in itertools.product((False, True), firsts, (False, True), (False, True)):
        below, above = (1, 20) if first is None else (first - 2, first + 2)
        for first_q0 in (None, below, above):
            want = vc.verdict_order(overflow, first, why, eval_differs, noncanonical, first_q0)
            verdict, column = C.c_int32(-3), C.c_uint32(12345)
            vv.vv_verdict(int(overflow), C.c_int64(-1 if first is None else first), C.c_uint32(why), int(eval_differs), int(noncanonical),
                          C.c_int64(-1 if first_q0 is None else first_q0), C.byref(verdict), C.byref(column))
            assert (verdict.value, column.value) == want, (overflow, first, why, eval_differs, noncanonical, first_q0)
            n += 1
    assert n == 2 * 15 * 2 * 2 * 3


def test_the_order_itself():
    """verdict_order on the cases whose answer the reference's text fixes (verify_z.rs:60-188), so that the comparison
    above is not one function against its own translation."""
    P, M, K = vc.FAILS_PROXIMITY, vc.FAILS_MALFORMED, vc.FAILS_MERKLE
    assert vc.verdict_order(False, None, 0, False, False, None) == (vc.ACCEPT, 0)
    assert vc.verdict_order(True, 3, P | M | K, True, True, 1) == (vc.OVERFLOW, 0)
    assert vc.verdict_order(False, 3, P | M | K, True, True, 1) == (vc.PROXIMITY_TESTING, 3)
    assert vc.verdict_order(False, 3, M | K, True, True, 1) == (vc.MALFORMED, 3)
    assert vc.verdict_order(False, 3, K, True, True, 1) == (vc.MERKLE, 3)
    assert vc.verdict_order(False, None, 0, True, True, 1) == (vc.EVAL_CONSISTENCY, 0)
    assert vc.verdict_order(False, None, 0, False, True, 1) == (vc.MALFORMED, 0)
    assert vc.verdict_order(False, None, 0, False, False, 1) == (vc.PROXIMITY_Q0, 1)
