"""CPU: zinc_amd/csrc/keccak_dev.cuh -- Keccak-f[1600], the absorb_random_field byte stream, get_challenge with every
branch and the signed-FieldMap reduction -- compiled for the host and driven against the oracle's KeccakTranscript.  It
is the code sumcheck_tail_kernel runs on the device and zip_sumcheck_prove's host thread runs above the tail."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODULI = [
    (106319353542452952636349991594949358997917625194731877894581586278529202198383, 4),
    ((1 << 256) - 189, 4),                 # no spare bit: values are reduced modulo 189 first
    ((1 << 255) + (99 << 128) + 12345, 4),  # no spare bit, a large 2^256 - q
    ((1 << 190) - 11 * (1 << 64) - 59, 3),
    ((1 << 128) + 51, 3),                   # 129 bits: the hi mask keeps nothing
    ((1 << 129) + (1 << 64) + 1, 3),
    ((1 << 192) - 1233, 3),                 # no spare bit
    ((1 << 128) - 159, 2),                  # no spare bit
    (57316695564490278656402085503, 2),
]


@pytest.fixture(scope="module")
def kd(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    so = str(tmp_path_factory.mktemp("keccak_dev") / "libkeccak_dev_check.so")
    cmd = [cxx, "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{os.path.join(ROOT, 'zinc_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "native", "keccak_dev_check.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return C.CDLL(so)


@pytest.mark.parametrize("modulus,fl", MODULI)
def test_rounds_equal_the_oracles_transcript_at_every_offset(kd, modulus, fl):
    orc.build()
    f = orc.make_field(modulus, fl)
    mod = np.array(orc.int_to_limbs(modulus, fl), dtype=np.uint64)
    r2 = np.array([f.r2[i] for i in range(fl)], dtype=np.uint64)
    rng = np.random.default_rng(fl)
    n_rounds = 4
    for p in range(137):
        ne = 2 + p % 4
        vals = [int.from_bytes(rng.bytes(40), "little") % modulus for _ in range(n_rounds * ne)]
        msgs = np.ascontiguousarray(orc.field_elems(vals, fl), dtype=np.uint64).reshape(n_rounds, ne, fl)
        k = orc.new_transcript()
        orc.absorb(k, bytes(range(p)))
        st = np.array([k.st[i] for i in range(25)], dtype=np.uint64)
        buf = np.zeros(136, np.uint8)
        buf[: k.buflen] = np.frombuffer(bytes(k.buf[: k.buflen]), np.uint8)
        buflen = C.c_uint32(k.buflen)
        r_out = np.zeros((n_rounds, fl), np.uint64)
        rc = kd.kd_rounds(fl, C.c_void_p(mod.ctypes.data), C.c_void_p(r2.ctypes.data), C.c_uint64(f.inv), C.c_void_p(st.ctypes.data),
                          C.c_void_p(buf.ctypes.data), C.byref(buflen), C.c_void_p(msgs.ctypes.data), ne, n_rounds,
                          C.c_void_p(r_out.ctypes.data))
        assert rc == 0
        for i in range(n_rounds):
            for e in range(ne):
                orc.absorb_field(k, f, orc.limbs_to_int(msgs[i, e]))
            want = (C.c_uint64 * orc.ORC_MAX_FL)()
            orc.lib().orc_tr_get_challenge(C.byref(k), C.byref(f), want)
            assert [int(x) for x in r_out[i]] == [int(want[j]) for j in range(fl)], (p, i)
            assert orc.limbs_to_int(r_out[i]) < modulus
            orc.absorb_field(k, f, orc.limbs_to_int(r_out[i]))
        assert [int(x) for x in st] == [int(k.st[i]) for i in range(25)], p
        assert buflen.value == k.buflen and bytes(buf[: k.buflen]) == bytes(k.buf[: k.buflen]), p
        assert not buf[k.buflen:].any(), p


@pytest.mark.parametrize("modulus,fl", MODULI)
def test_map_of_nvars_and_degree(kd, modulus, fl):
    orc.build()
    f = orc.make_field(modulus, fl)
    mod = np.array(orc.int_to_limbs(modulus, fl), dtype=np.uint64)
    r2 = np.array([f.r2[i] for i in range(fl)], dtype=np.uint64)
    for v in (0, 1, 2, 4, 30, 1 << 20):
        out = np.zeros(fl, np.uint64)
        assert kd.kd_map_u128(fl, C.c_void_p(mod.ctypes.data), C.c_void_p(r2.ctypes.data), C.c_uint64(f.inv), C.c_uint64(v), C.c_uint64(0),
                              C.c_void_p(out.ctypes.data)) == 0
        want = (C.c_uint64 * orc.ORC_MAX_FL)()
        orc.lib().orc_field_from_u128(C.byref(f), C.c_uint64(v), C.c_uint64(0), want)
        assert [int(x) for x in out] == [int(want[j]) for j in range(fl)], v
