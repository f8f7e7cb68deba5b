"""CPU: the word-wise chain step of zinc_amd/csrc/prime_dev.cuh (prime_next_candidate_words, what every lane of
prime_chain_batch_kernel runs) compiled for the host -- against the byte-addressed prime_next_candidate and against the
oracle's KeccakTranscript, for 300 consecutive candidates from every starting buflen 0 .. 135 at 2 / 3 / 4 limbs: every
residue of buflen mod 8 and every straddle of the rate boundary, by the clone's counter and by the candidate's bytes.
The same source is also a program of its own, built with the address and undefined-behaviour sanitizers and run once."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _oracle as orc
import _prime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "prime_chain_check.cpp")
INCLUDE = f"-I{os.path.join(ROOT, 'zinc_amd', 'csrc')}"
COUNT = 300


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    so = os.path.join(str(tmp_path_factory.mktemp("prime_chain")), "libprime_chain_check.so")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", INCLUDE, SOURCE, "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    lib.pc_chain_words.restype = C.c_uint32
    return lib


@pytest.mark.parametrize("fl", _prime.FLS)
def test_word_wise_step_equals_the_byte_step_and_the_oracle_chain(pc, fl):
    orc.build()
    boundary = 0
    for p in range(136):
        k = orc.new_transcript()
        orc.absorb(k, bytes((11 * i + 3 * p + fl) & 0xFF for i in range(136 + p)))  # one full block, then p pending bytes
        assert k.buflen == p
        st0, pending0 = _prime.sponge(k)
        st = np.array(st0, np.uint64)
        buf = np.full(136, 0xA5, np.uint8)  # bytes at and beyond buflen are ignored on input
        buf[:p] = np.frombuffer(pending0, np.uint8)
        cands = np.zeros((COUNT, fl), np.uint64)
        st_out, buf_out, len_out = np.zeros((COUNT, 25), np.uint64), np.ones((COUNT, 136), np.uint8), np.zeros(COUNT, np.uint32)
        differ = pc.pc_chain_words(fl, C.c_void_p(st.ctypes.data), C.c_void_p(buf.ctypes.data), p, COUNT, C.c_void_p(cands.ctypes.data),
                                   C.c_void_p(st_out.ctypes.data), C.c_void_p(buf_out.ctypes.data), C.c_void_p(len_out.ctypes.data))
        assert differ == 0, (p, "candidates at which the word-wise step and prime_next_candidate part")
        for i in range(COUNT):
            want = _prime.next_candidate(k, fl)
            assert orc.limbs_to_int(cands[i]) == want, (p, i)
            n = int(k.buflen)
            assert int(len_out[i]) == n, (p, i)
            assert st_out[i].tolist() == [int(k.st[w]) for w in range(25)], (p, i)
            assert bytes(buf_out[i, :n]) == bytes(k.buf[:n]) and not buf_out[i, n:].any(), (p, i)
        boundary += int(np.count_nonzero(np.diff(len_out.astype(np.int64)) < 0))
    assert boundary > 136, "the chains crossed the rate boundary many times"


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "prime_chain_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DPRIME_CHAIN_CHECK_MAIN", INCLUDE, SOURCE, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"{3 * 136 * COUNT} steps, 0 differ" in r.stdout
