"""Builders shared by the tests of num_proximity_testing = T > 1 (no GPU, no ctypes beyond _oracle).

A test sets z.p.num_proximity_testing = T on its own _oracle.Zip: orc_open loops over the tests and orc_proof_len counts
them, but orc_open hands back test 0's coefficients only.  The others come from replaying orc_tr_get_integer_challenge
on a copy of the transcript, in the order the reference squeezes them: test 0 .. test T-1, then the columns.

Stream for num_rows > 1 (open_z.rs:100-143, commit.rs:726):
    u'_0 | ... | u'_{T-1}   row_len x 64 bytes each, Int<8> little-endian
    per opening             num_rows x 32 bytes, then num_rows records of be64(depth) | depth x 32 bytes
    evaluation row          row_len x 8*fl bytes, big-endian Montgomery
"""
import ctypes as C
import functools

import numpy as np

import _oracle as orc

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59


def copy_transcript(k: orc.Keccak) -> orc.Keccak:
    return orc.Keccak.from_buffer_copy(k)


def squeeze_coeffs(k: orc.Keccak, n: int) -> np.ndarray:
    """n Int<1> challenges (get_integer_challenges, open_z.rs:104); advances k."""
    out = np.zeros(n, dtype=np.uint64)
    w = C.c_uint64()
    for i in range(n):
        orc.lib().orc_tr_get_integer_challenge(C.byref(k), 1, C.byref(w))
        out[i] = w.value
    return out.view(np.int64)


def squeeze_cols(k: orc.Keccak, f: orc.Field, cw: int, n: int) -> np.ndarray:
    """squeeze_challenge_idx (pcs_transcript.rs:174-179): the first 4 little-endian bytes of the Montgomery value."""
    return np.array([(orc.get_challenge(k, f) & 0xFFFFFFFF) % cw for _ in range(n)], dtype=np.uint32)


def stream_len(z, T, n_cols, fl):
    """commit.rs:712-737"""
    u = T * z.row_len * 8 * z.m_limbs if z.num_rows > 1 else 0
    return u + n_cols * z.num_rows * (8 * z.k_limbs + 8 + 32 * z.depth) + z.row_len * 8 * fl


def u_primes(proof, z, T):
    """The T proximity rows of a stream as Python ints, [T][row_len]."""
    raw = proof[: T * z.row_len * 64].tobytes()
    return [[int.from_bytes(raw[64 * (t * z.row_len + c): 64 * (t * z.row_len + c) + 64], "little", signed=True)
             for c in range(z.row_len)] for t in range(T)]


def combine_int(coeffs, evals, num_rows, row_len):
    """sum_r coeffs[r] * w[r][c] in Python integers"""
    w = np.asarray(evals, dtype=np.int64).reshape(num_rows, row_len).astype(object)
    c = np.asarray(coeffs, dtype=np.int64).astype(object)
    return [int(x) for x in (c[:, None] * w).sum(axis=0)]


def u_prime_bytes(u):
    return np.frombuffer(b"".join(int(x).to_bytes(64, "little", signed=True) for x in u), dtype=np.uint8)


class Inst:
    pass


def witness(num_vars, seed=0, small=False):
    n = 1 << num_vars
    if small:
        return np.random.default_rng(seed).integers(-128, 128, size=n, dtype=np.int64)
    evals = orc.splitmix64(0x5A494E43 + seed, n).copy()
    evals[: min(n, 3)] = np.array([-(2**63), 2**63 - 1, -1], dtype=np.int64)[: min(n, 3)]
    return evals


@functools.lru_cache(maxsize=None)
def committed(num_vars, seed=0, small=False):
    """(evals, rows, layers, roots) of the reference geometry: the commitment does not depend on T, the field or the
    number of openings, so the instances of one size share it."""
    evals = witness(num_vars, seed, small)
    out = (evals,) + orc.Zip(num_vars).commit(evals)
    for a in out:
        a.setflags(write=False)
    return out


def make(num_vars, T, modulus=BENCH_MODULUS, fl=4, n_cols=8, seed=0, evals=None, geometry=None, fs=None, commit=None):
    """An honest commit + open on the oracle with T proximity tests and n_cols openings."""
    i = Inst()
    z = orc.Zip(num_vars, geometry=geometry)
    z.p.num_proximity_testing = T
    z.p.num_column_opening = n_cols
    f = orc.make_field(modulus, fl)
    point = orc.point_to_field(f, np.random.default_rng(seed + 1).integers(-50, 50, size=num_vars, dtype=np.int64))
    if commit is not None:
        evals, rows, layers, roots = commit
    else:
        if evals is None:
            evals = witness(num_vars, seed, small=(fl == 2))
        rows, layers, roots = z.commit(evals)
    fs = fs if fs is not None else orc.new_transcript()
    replay = copy_transcript(fs)
    proof, cols, coeffs0 = z.open(f, evals, rows, layers, point, fs)
    R = z.num_rows
    coeffs = squeeze_coeffs(replay, T * R).reshape(T, R) if R > 1 else None
    assert R == 1 or np.array_equal(coeffs[0], coeffs0)
    assert np.array_equal(squeeze_cols(replay, f, z.codeword_len, n_cols), cols)
    lr = R.bit_length() - 1
    i.z, i.f, i.T, i.modulus, i.fl, i.evals, i.point, i.rows, i.layers = z, f, T, modulus, fl, evals, point, rows, layers
    i.roots, i.proof, i.cols, i.coeffs, i.fs_after = roots, proof, cols, coeffs, fs
    i.q0 = orc.build_eq_x_r(f, point[num_vars - lr:]) if lr else None
    i.q1 = orc.build_eq_x_r(f, point[: num_vars - lr]) if num_vars - lr else None
    i.ev = z.mle_eval(f, evals, point)
    i.R, i.C, i.cw, i.d, i.n_cols = R, z.row_len, z.codeword_len, z.depth, n_cols
    i.u_bytes = T * i.C * 64 if R > 1 else 0
    i.col_bytes = R * (32 + 8 + 32 * i.d)
    return i


@functools.lru_cache(maxsize=None)
def instance(num_vars, T, modulus=BENCH_MODULUS, fl=4, n_cols=8, seed=0):
    """Shared instances: built once per process, never modified."""
    i = make(num_vars, T, modulus, fl, n_cols, seed, commit=committed(num_vars, seed, fl == 2))
    i.proof.setflags(write=False)
    return i
