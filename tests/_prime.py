"""Expected values for the prime-generation tests, none of them from the code under test: a strong probable-prime test
to base 2 on Python's pow, the candidate chain of prime_gen::get_prime (src/prime_gen.rs:8-26) on the oracle's
KeccakTranscript (orc_tr_get_random_bytes, orc_keccak_update) and int.from_bytes, and the candidate lists."""
import ctypes as C
import functools
import os
import random
import shutil
import subprocess

import numpy as np

import _oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLS = (2, 3, 4)


def sprp2(n: int) -> bool:
    """MillerRabin::test_base_two().is_probably_prime() for odd n >= 3"""
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    z = pow(2, d, n)
    if z in (1, n - 1):
        return True
    for _ in range(s - 1):
        z = z * z % n
        if z == n - 1:
            return True
        if z == 1:
            return False
    return False


@functools.lru_cache(maxsize=None)
def adversarial(fl: int):
    """odd values >= 3 below 2^(64 fl) where an implementation can go wrong: tiny values in full-width limbs, base-2
    pseudoprimes, Fermat and Mersenne shapes (strong pseudoprimes to base 2 when composite), primes without a spare
    bit, the all-ones value, a semiprime of Mersenne primes, and every shape of n - 1 = d 2^s"""
    top = 1 << (64 * fl)
    v = [3, 5, 7, 9, 561, 2047, 3277, 4033, (1 << 32) + 1, (1 << 64) + 1, (1 << 128) + 1]
    v += [(1 << e) - 1 for e in (67, 89, 127, 137, 211)]
    v += [(1 << 128) - 159, (1 << 192) - 237, (1 << 256) - 189, top - 1, ((1 << 61) - 1) * ((1 << 89) - 1)]
    v += [d * (1 << s) + 1 for s in (1, 2, 63, 64, 65, 64 * fl - 2) for d in (1, 3, 5, 7, 9, 11, 13, 15, 255)]
    return tuple(sorted({n for n in v if 3 <= n < top}))


@functools.lru_cache(maxsize=None)
def random_odd(fl: int, count: int, seed: int = 1):
    rng = random.Random(1000 * fl + seed)
    return tuple(rng.getrandbits(64 * fl) | 1 | (rng.getrandbits(1) << (64 * fl - 1)) for _ in range(count))


def _random_prime(rng, bits):
    while True:
        p = rng.getrandbits(bits) | 1 | (1 << (bits - 1))
        if all(pow(a, p - 1, p) == 1 for a in (2, 3, 5, 7)) and sprp2(p):
            return p


@functools.lru_cache(maxsize=None)
def semiprimes(fl: int, count: int):
    rng = random.Random(77 + fl)
    out = []
    while len(out) < count:
        a = rng.randrange(8, 64 * fl - 8)
        out.append(_random_prime(rng, a) * _random_prime(rng, 64 * fl - a))
    return tuple(out)


def limbs(values, fl: int) -> np.ndarray:
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(fl)] for v in values], dtype=np.uint64).reshape(-1, fl)


# ---- the candidate chain on the oracle's transcript
def next_candidate(k: "orc.Keccak", fl: int) -> int:
    """hash_int + the even fix-up of get_prime; k absorbs the bytes"""
    buf = (C.c_uint8 * (8 * fl))()
    orc.lib().orc_tr_get_random_bytes(C.byref(k), C.c_size_t(8 * fl), buf)
    orc.absorb(k, bytes(buf))
    n = int.from_bytes(bytes(buf), "big")
    return n if n % 2 else (n - 1) % (1 << (64 * fl))


def sponge(k: "orc.Keccak"):
    """(st, pending bytes) of an oracle transcript"""
    return [int(k.st[i]) for i in range(25)], bytes(k.buf[: k.buflen])


def transcript(seed_k: int) -> "orc.Keccak":
    """the twelve transcripts: fresh for 0, else one that absorbed bytes([k]) * k"""
    k = orc.new_transcript()
    if seed_k:
        orc.absorb(k, bytes([seed_k]) * seed_k)
    return k


@functools.lru_cache(maxsize=None)
def reference_get_prime(seed_k: int, fl: int, prefix: bytes = b""):
    """the reference's loop on the oracle's transcript -> (prime, candidates tried, st, pending bytes afterwards)"""
    orc.build()
    k = transcript(seed_k)
    if prefix:
        orc.absorb(k, prefix)
    tried = 0
    while True:
        n = next_candidate(k, fl)
        tried += 1
        if n >= 3 and sprp2(n):
            st, pending = sponge(k)
            return n, tried, tuple(st), pending


def public_input_bytes(xs) -> bytes:
    """cast_slice(input.as_words()) of every Int<1> public input: 8 little-endian bytes each (two's complement)"""
    return b"".join((int(x) & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little") for x in xs)


def build_host_check(out_dir: str, opt: str = "-O1") -> C.CDLL:
    """tests/native/prime_dev_check.cpp: prime_dev.cuh compiled for the host with g++"""
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    so = os.path.join(out_dir, "libprime_dev_check.so")
    cmd = [cxx, opt, "-std=c++17", "-shared", "-fPIC", f"-I{os.path.join(ROOT, 'zinc_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "native", "prime_dev_check.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    lib.pd_get_prime.restype = C.c_uint32
    lib.pd_batch_knob.restype = C.c_uint32
    lib.pd_batch_knob.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
    return lib
