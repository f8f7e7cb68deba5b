"""Two-limb witnesses (INT_LIMBS = 2): witness builders, the oracle at n_limbs = 2 (the existing _oracle.Zip methods cast
to int64, so the generic entry points are called directly here), and a plain Python-int model of
MultilinearZip::verify for 64-byte column entries and Int<16> proximity rows.

No GPU here.  Everything is bit-exact: there are no tolerances.

Stream layout for num_rows > 1:
    u'            row_len x 128 bytes, Int<16> little-endian
    per opening   num_rows x 64 bytes (Int<8> column entries), then num_rows records of be64(depth) | depth x 32 bytes
    evaluation    row_len x 8*fl bytes, big-endian Montgomery
"""
import ctypes as C
import functools

import numpy as np

import _oracle as orc
from _verify_cases import (ACCEPT, EVAL_CONSISTENCY, FAILS_MALFORMED, FAILS_MERKLE, FAILS_PROXIMITY, MALFORMED, MERKLE,
                           OVERFLOW, PROXIMITY_Q0, PROXIMITY_TESTING, raa_encode, verdict_order)

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503  # about 2^95.5: two-limb witnesses exceed it
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
MOD_NO_SPARE = (1 << 256) - 189              # the quirk, already below 2^64
MOD_QUIRK_100 = (1 << 256) - (1 << 100) - 1  # odd, top bit set, 2^256 - q = 2^100 + 1: bites only for two-limb witnesses
MOD_QUIRK_2LIMB = (1 << 128) - 159           # the two-limb counterpart: 2^128 - q = 159
MOD_M127 = (1 << 127) - 1                    # two limbs, top bit clear: a plain reduction of the witness
# every modulus of the parity tests
MODULI = [(BENCH_MODULUS, 4), (MOD_3LIMB, 3), (TEST_MODULUS_2, 2), (MOD_NO_SPARE, 4), (MOD_QUIRK_100, 4), (MOD_QUIRK_2LIMB, 2)]
# the moduli under which the reference's verifier accepts its own two-limb proofs: no signed-modulus reduction bites in
# the prover's map (the verifier maps Int<8> entries over 8 words and never applies it)
VERIFY_MODULI = [(BENCH_MODULUS, 4), (MOD_3LIMB, 3), (TEST_MODULUS_2, 2), (MOD_M127, 2)]

INT2_MIN, INT2_MAX = -(1 << 127), (1 << 127) - 1
INT16_MIN, INT16_MAX = -(1 << 1023), (1 << 1023) - 1
N_COLS = 12


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def to_limbs(values, n_limbs=2):
    """Python ints -> [n, n_limbs] uint64, two's complement, little-endian limbs."""
    return np.array([orc.int_to_limbs(int(v), n_limbs) for v in values], dtype=np.uint64).reshape(len(values), n_limbs)


def to_ints(limbs):
    """[n, L] uint64 limbs -> signed Python ints."""
    return [orc.limbs_to_int(row, signed=True) for row in np.asarray(limbs, dtype=np.uint64)]


def witness(z, kind="random", seed=0):
    """[2^num_vars, 2] uint64.  random: uniform 128-bit two's complement from a seeded generator with -2^127, 2^127 - 1,
    0 and -1 planted at the first and last position of the first and last row.  max / min: every entry 2^127 - 1 /
    -2^127, the rows that reach the 128 + 2 log2(cw) bound of the scan lanes.  lowtop: high limbs zero, low limbs with
    their top bit set (a sign extension applied to the low limb shows)."""
    n, C_ = z.num_rows * z.row_len, z.row_len
    if kind == "max":
        return np.tile(to_limbs([INT2_MAX]), (n, 1))
    if kind == "min":
        return np.tile(to_limbs([INT2_MIN]), (n, 1))
    rng = np.random.default_rng(0x5A494E43 + seed)
    w = rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    if kind == "lowtop":
        w[:, 1] = 0
        w[:, 0] |= np.uint64(1 << 63)
        return w
    assert kind == "random"
    planted = to_limbs([INT2_MIN, INT2_MAX, 0, -1])
    for pos, v in zip((0, C_ - 1, n - C_, n - 1), planted):
        w[pos] = v
    if n == 2:  # (two positions: the extremes)
        w[0], w[1] = planted[0], planted[1]
    return w


def challenge_like(n, seed):
    """[n, 2] full-range Int<2> values with both extremes among them (what get_integer_challenge(2) can return)."""
    c = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    ext = to_limbs([INT2_MIN, INT2_MAX])
    c[: min(n, 2)] = ext[: min(n, 2)]
    return c


class Zip2:
    """The oracle's geometry at n_limbs = 2 (K = Int<8>, M = Int<16>) and its generic entry points."""

    def __init__(self, num_vars, geometry=None, rep=2, n_cols=N_COLS):
        self.z = z = orc.Zip(num_vars, n_limbs=2, rep=rep, geometry=geometry)
        assert (z.n_limbs, z.k_limbs, z.m_limbs) == (2, 8, 16)
        z.p.num_column_opening = n_cols
        self.n_cols = n_cols
        for name in ("num_vars", "row_len", "num_rows", "codeword_len", "rep", "depth", "perm1", "perm2", "tree_hashes"):
            setattr(self, name, getattr(z, name))

    def ctx(self, cabi):
        return cabi.ZipContext(self.num_vars, self.perm1, self.perm2, rep=self.rep, n_limbs=2, k_limbs=8, m_limbs=16,
                               geometry_override=(self.row_len, self.num_rows, self.codeword_len))

    def commit(self, evals, merkle=True):
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        assert evals.shape == (self.num_rows * self.row_len, 2)
        rows = np.zeros((self.num_rows * self.codeword_len, 8), dtype=np.uint64)
        layers = np.zeros((self.num_rows, self.tree_hashes, 32), dtype=np.uint8) if merkle else None
        roots = np.zeros((self.num_rows, 32), dtype=np.uint8) if merkle else None
        rc = orc.lib().orc_commit(C.byref(self.z.p), _u64p(evals), _u64p(rows), _u8p(layers) if merkle else None,
                                  _u8p(roots) if merkle else None)
        assert rc == 0, rc
        return rows, layers, roots

    def combine_rows_int(self, coeffs, evals):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        out = np.zeros((self.row_len, 16), dtype=np.uint64)
        rc = orc.lib().orc_combine_rows_int(_u64p(coeffs), 2, _u64p(evals), 2, self.num_rows, self.row_len, _u64p(out), 16)
        return rc, out

    def combine_rows_field(self, f, q0, evals):
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        q0 = np.ascontiguousarray(q0, dtype=np.uint64)
        out = np.zeros((self.row_len, f.fl), dtype=np.uint64)
        orc.lib().orc_combine_rows_field(C.byref(f), _u64p(q0), _u64p(evals), 2, self.num_rows, self.row_len, _u64p(out))
        return out

    def map_to_field(self, f, evals):
        """phi of every witness entry: the evaluation row of a one-row matrix"""
        return np.stack([orc.field_from_int(f, v) for v in np.ascontiguousarray(evals, dtype=np.uint64)])

    def proof_len(self, fl):
        return self.z.proof_len(fl)

    def open(self, f, evals, rows, layers, point, fs=None):
        """-> (proof, cols, coeffs [num_rows, 2]): orc_open with the columns and coefficients it squeezed itself"""
        fs = fs or orc.new_transcript()
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        point = np.ascontiguousarray(point, dtype=np.uint64)
        cap = self.proof_len(f.fl)
        proof = np.zeros(cap, dtype=np.uint8)
        plen = C.c_size_t(0)
        cols = np.zeros(self.n_cols, dtype=np.uint32)
        coeffs = np.zeros((self.num_rows, 2), dtype=np.uint64)
        rc = orc.lib().orc_open(C.byref(self.z.p), C.byref(f), _u64p(evals), _u64p(rows), _u8p(layers), _u64p(point),
                                C.byref(fs), _u8p(proof), C.c_size_t(cap), C.byref(plen), _u32p(cols), _u64p(coeffs))
        assert rc == 0, rc
        assert plen.value == cap, (plen.value, cap)
        return proof, cols, coeffs

    def verify(self, f, roots, point, eval_mont, proof, check_merkle=True):
        return self.z.verify(f, roots, point, eval_mont, proof, check_merkle=check_merkle)

    def mle_eval(self, f, evals, point):
        evals = np.ascontiguousarray(evals, dtype=np.uint64)
        point = np.ascontiguousarray(point, dtype=np.uint64)
        out = (C.c_uint64 * orc.ORC_MAX_FL)()
        orc.lib().orc_mle_eval_field(C.byref(f), _u64p(evals), 2, self.num_vars, _u64p(point), out)
        return orc.limbs_to_int(out[: f.fl])

    def tensors(self, f, point):
        """(q0, q1) = point_to_tensor: eq of the last log2(num_rows) coordinates, eq of the others (None when empty)"""
        lr = self.num_rows.bit_length() - 1
        q0 = orc.build_eq_x_r(f, point[self.num_vars - lr:]) if lr else None
        q1 = orc.build_eq_x_r(f, point[: self.num_vars - lr]) if self.num_vars - lr else None
        return q0, q1


def make_point(f, num_vars, seed=3):
    ints = np.random.default_rng(seed).integers(-100, 100, size=num_vars, dtype=np.int64)
    return orc.point_to_field(f, ints) if num_vars else np.zeros((0, f.fl), dtype=np.uint64)


def field_map_values(modulus, fl, width, n=512, seed=11):
    """[n, width] uint64: what zip_field_map_int is pinned on.  Width 2: the planted extremes, values on both sides of
    2^(64 fl) - q and of q (where those fit 127 bits), random values.  Width 8: values that fill all 512 bits, the
    extremes, small values."""
    bits = 64 * width
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = [lo, hi, 0, -1, 1, lo + 1, hi - 1]
    for edge in ((1 << (64 * fl)) - modulus, modulus, 2 * modulus, ((1 << (64 * fl)) - modulus) * 2):
        for d in (-1, 0, 1):
            for s in (1, -1):
                v = s * (edge + d)
                if lo <= v <= hi:
                    vals.append(v)
    rng = np.random.default_rng(seed + width)
    while len(vals) < n:
        raw = int.from_bytes(rng.bytes(bits // 8), "little")
        v = raw - (1 << bits) if raw >> (bits - 1) else raw  # uniform over the whole signed range
        if len(vals) % 3 == 0:
            v >>= int(rng.integers(0, bits))  # a third of them shorter (the shift keeps the sign)
        vals.append(v)
    return to_limbs(vals[:n], width)


# ---------------------------------------------------------------------------------------------------------------------
# An honest proof with everything both verifiers need, and the byte offsets of its parts
# ---------------------------------------------------------------------------------------------------------------------
class Instance:
    def __init__(self, num_vars, modulus, fl, seed=5, geometry=None, rep=2, n_cols=N_COLS):
        self.z = z = Zip2(num_vars, geometry=geometry, rep=rep, n_cols=n_cols)
        self.modulus, self.fl = modulus, fl
        self.f = f = orc.make_field(modulus, fl)
        self.evals = witness(z, "random", seed)
        self.point = make_point(f, num_vars, seed + 1)
        self.rows, self.layers, self.roots = z.commit(self.evals)
        self.proof, self.cols, self.coeffs = z.open(f, self.evals, self.rows, self.layers, self.point)
        self.q0, self.q1 = z.tensors(f, self.point)
        self.ev = z.mle_eval(f, self.evals, self.point)
        self.R, self.C, self.cw, self.d, self.n_cols = z.num_rows, z.row_len, z.codeword_len, z.depth, z.n_cols
        assert self.R > 1 and self.C > 1
        self.u_bytes = self.C * 128
        self.rec_bytes = 8 + 32 * self.d
        self.col_bytes = self.R * (64 + self.rec_bytes)
        self.row_off = self.u_bytes + self.n_cols * self.col_bytes
        self.need = self.row_off + self.C * 8 * fl
        assert self.proof.size == self.need
        self.rm = (1 << (64 * fl)) % modulus
        self.rinv = pow(self.rm, -1, modulus)
        self.coeffs_int = to_ints(self.coeffs)
        self.q0_std = [self.std(orc.limbs_to_int(x)) for x in self.q0]
        self.q1_std = [self.std(orc.limbs_to_int(x)) for x in self.q1]
        for a in (self.proof, self.roots):
            a.setflags(write=False)

    def std(self, mont):
        return mont * self.rinv % self.modulus

    def mont(self, std):
        return std * self.rm % self.modulus

    def val_at(self, k, r):
        return self.u_bytes + k * self.col_bytes + 64 * r

    def rec_at(self, k, r):
        return self.u_bytes + k * self.col_bytes + 64 * self.R + r * self.rec_bytes

    def node_at(self, k, r, level):
        return self.rec_at(k, r) + 8 + 32 * level

    def row_at(self, c):
        return self.row_off + c * 8 * self.fl

    def oracle_rc(self, proof, roots, ev):
        return self.z.verify(self.f, roots, self.point, ev, proof)

    def u_prime(self, proof):
        raw = proof[: self.u_bytes].tobytes()
        return [int.from_bytes(raw[128 * c: 128 * c + 128], "little", signed=True) for c in range(self.C)]

    def with_u_prime(self, proof, u):
        p = proof.copy()
        p[: self.u_bytes] = np.frombuffer(b"".join(int(x).to_bytes(128, "little", signed=True) for x in u), dtype=np.uint8)
        return p

    def value(self, proof, k, r):
        o = self.val_at(k, r)
        return int.from_bytes(proof[o: o + 64].tobytes(), "little", signed=True)

    def set_value(self, proof, k, r, v):
        o = self.val_at(k, r)
        proof[o: o + 64] = np.frombuffer(int(v).to_bytes(64, "little", signed=True), dtype=np.uint8)

    def row_elems(self, proof):
        n = 8 * self.fl
        raw = proof[self.row_off: self.need].tobytes()
        return [int.from_bytes(raw[n * c: n * c + n], "big") for c in range(self.C)]

    def dot_q1(self, row_wire):
        return self.mont(sum(self.std(x) * b for x, b in zip(row_wire, self.q1_std)) % self.modulus)

    # ---- the model: the reference's order of checks over Python ints (verify_z.rs:60-188), with the report's counts --
    def expect(self, proof, roots, ev):
        """-> dict(verdict, column, bad_merkle_paths, malformed_paths), what zip_verify must report"""
        q = self.modulus
        proof = np.ascontiguousarray(proof, dtype=np.uint8)
        roots = np.ascontiguousarray(roots, dtype=np.uint8)
        if proof.size < self.need:
            return dict(verdict=MALFORMED, column=0, bad_merkle_paths=0, malformed_paths=0)
        enc_u, lo, hi = raa_encode(self.z, self.u_prime(proof))
        overflow = lo < INT16_MIN or hi > INT16_MAX
        wire = self.row_elems(proof)
        enc_f = raa_encode(self.z, [self.std(x) for x in wire])[0]
        L, pa, ra = orc.lib(), proof.ctypes.data, roots.ctypes.data
        prefix = self.d.to_bytes(8, "big")
        first = first_q0 = None
        why = n_bad = n_mal = 0
        for k in range(self.n_cols):
            col = int(self.cols[k])
            v = [self.value(proof, k, r) for r in range(self.R)]
            isum = sum(c * x for c, x in zip(self.coeffs_int, v))
            fsum = sum(a * x for a, x in zip(self.q0_std, v)) % q  # phi_8(v) = sign (|v| mod q): v mod q
            mal = bad = 0
            for r in range(self.R):
                o = self.rec_at(k, r)
                if proof[o: o + 8].tobytes() != prefix:
                    mal += 1
                elif L.orc_merkle_verify(self.d, C.c_void_p(pa + o + 8), C.c_void_p(ra + 32 * r),
                                         C.c_void_p(pa + self.val_at(k, r)), 8, col) != 0:
                    bad += 1
            n_bad, n_mal = n_bad + bad, n_mal + mal
            w = (FAILS_PROXIMITY if isum != enc_u[col] else 0) | (FAILS_MALFORMED if mal else 0) | (FAILS_MERKLE if bad else 0)
            if w and first is None:
                first, why = k, w
            if first_q0 is None and fsum != enc_f[col] % q:
                first_q0 = k
        verdict, column = verdict_order(overflow, first, why, self.dot_q1(wire) != ev, any(x >= q for x in wire), first_q0)
        return dict(verdict=verdict, column=column, bad_merkle_paths=n_bad, malformed_paths=n_mal)


@functools.lru_cache(maxsize=None)
def instance(num_vars, modulus, fl, geometry=None, rep=2, n_cols=N_COLS):
    """The shared honest proofs of the verifier tests, built once per process and never modified.  geometry =
    (row_len, num_rows, codeword_len) with its rep: a slice of a real geometry instead of the whole shape of num_vars."""
    return Instance(num_vars, modulus, fl, geometry=geometry, rep=rep, n_cols=n_cols)


# ---------------------------------------------------------------------------------------------------------------------
# The tamper catalogue: (name, mutate, claim).  mutate(proof, roots, ev) -> (proof, roots, ev) never writes into its
# arguments.  claim: the verdict the one-limb catalogue (tests/_verify_cases.py) defines for the section, and the failing
# column where the construction fixes it; the model above supplies the complete report.
# ---------------------------------------------------------------------------------------------------------------------
def _flip_bit(at_byte, bit):
    def mutate(proof, roots, ev):
        p = proof.copy()
        p[at_byte + bit // 8] ^= np.uint8(1 << (bit % 8))
        return p, roots, ev
    return mutate


def _flip_root(r):
    def mutate(proof, roots, ev):
        ro = roots.copy()
        ro[r, 0] ^= 1
        return proof, ro, ev
    return mutate


def _pair_move(inst, k, r, s):
    def mutate(proof, roots, ev):
        p = proof.copy()
        inst.set_value(p, k, r, inst.value(p, k, r) + inst.coeffs_int[s])
        inst.set_value(p, k, s, inst.value(p, k, s) - inst.coeffs_int[r])
        return p, roots, ev
    return mutate


def tamper_cases(inst):
    i, out = inst, []
    c = i.C // 2
    out.append((f"u'[{c}] bit 0", _flip_bit(128 * c, 0), dict(verdict=PROXIMITY_TESTING)))
    # bit 1023 turns an honest element (about 256 bits) into one near -+2^1023: encode_wide leaves Int<16>
    out.append((f"u'[{c}] bit 1023", _flip_bit(128 * c, 1023), dict(verdict=OVERFLOW, column=0)))
    for k, r in ((0, 0), (i.n_cols - 1, i.R - 1)):
        for bit in (0, 160, 511):
            out.append((f"value[{k},{r}] bit {bit}", _flip_bit(i.val_at(k, r), bit), dict(verdict=PROXIMITY_TESTING)))
    k, r = i.n_cols // 2, i.R - 1
    out.append((f"path[{k},{r}] level {i.d - 1}", _flip_bit(i.node_at(k, r, i.d - 1) + 5, 4), dict(verdict=MERKLE, column=k)))
    out.append((f"prefix[{k},{r}]", _flip_bit(i.rec_at(k, r) + 7, 0), dict(verdict=MALFORMED, column=k)))
    c1 = next(c for c in range(i.C) if i.q1_std[c])  # (an element <row, q1> can see)
    out.append((f"evaluation row[{c1}]", _flip_bit(i.row_at(c1) + 8 * i.fl - 1, 0), dict(verdict=EVAL_CONSISTENCY, column=0)))
    out.append(("root[0]", _flip_root(0), dict(verdict=MERKLE, column=0)))
    out.append(("wrong claimed evaluation", lambda p, ro, ev: (p, ro, (ev + 1) % i.modulus), dict(verdict=EVAL_CONSISTENCY, column=0)))
    out.append(("one byte short", lambda p, ro, ev: (p[:-1], ro, ev), dict(verdict=MALFORMED, column=0)))
    k = i.n_cols // 3
    out.append((f"pair move [{k}: 1,{i.R - 2}]", _pair_move(i, k, 1, i.R - 2), dict(verdict=MERKLE, column=k)))
    return out


def overflow_case(inst):
    """u' = 2^1022 e_c: it fits Int<16>, twice it does not, and every element is read at least twice by the encoding."""
    c = inst.C - 1
    return (f"u' = 2^1022 at {c}", lambda p, ro, ev: (inst.with_u_prime(p, [(1 << 1022) if j == c else 0 for j in range(inst.C)]), ro, ev),
            dict(verdict=OVERFLOW, column=0))


# ---------------------------------------------------------------------------------------------------------------------
# The verifier shapes of the regime tests (tests/test_gpu_two_limb_regimes.py on the device, and
# tests/test_two_limb_regimes_host.py, which holds the model to the oracle on the same shapes and cases first):
# (num_vars, modulus, fl, (row_len, num_rows, codeword_len), rep)
# ---------------------------------------------------------------------------------------------------------------------
# 2048 rows: every thread of tl_verify_columns_kernel walks 8 of them
REGIME_MANY_ROWS = [(13, BENCH_MODULUS, 4, (4, 2048, 8), 2), (13, TEST_MODULUS_2, 2, (4, 2048, 8), 2)]
# codewords of 2048 / 4096 / 65536: encode_wide(u') over Int<16> by 1024 threads that own 2 / 4 / 64 positions each
REGIME_WIDE_CODEWORDS = [(11, BENCH_MODULUS, 4, (1024, 2, 2048), 2), (11, MOD_3LIMB, 3, (1024, 2, 2048), 2),
                         (12, BENCH_MODULUS, 4, (1024, 4, 4096), 4), (15, BENCH_MODULUS, 4, (16384, 2, 65536), 4)]


def regime_instance(num_vars, modulus, fl, geometry, rep):
    inst = instance(num_vars, modulus, fl, geometry, rep)
    assert (inst.C, inst.R, inst.cw) == geometry
    return inst


def below_overflow_case(inst):
    """overflow_case's companion: u' = 2^1000 e_c.  No prefix sum of either pass leaves Int<16> (2^1000 rep cw < 2^1023
    for every codeword a ctx admits), so the encoding is formed and the openings simply do not match it."""
    c = inst.C - 1
    return (f"u' = 2^1000 at {c}", lambda p, ro, ev: (inst.with_u_prime(p, [(1 << 1000) if j == c else 0 for j in range(inst.C)]), ro, ev),
            dict(verdict=PROXIMITY_TESTING, column=0))


def fill_512_case(inst, seed=9):
    """Every column entry of every opening filled with 512 random bits, -2^511 and 2^511 - 1 planted at the first and
    the last row of the first opening: the sums of num_rows 128 x 512-bit products and the 512-bit reductions."""
    def mutate(proof, roots, ev):
        p = proof.copy()
        rng = np.random.default_rng(seed)
        for k in range(inst.n_cols):
            p[inst.val_at(k, 0): inst.val_at(k, 0) + 64 * inst.R] = np.frombuffer(rng.bytes(64 * inst.R), dtype=np.uint8)
        inst.set_value(p, 0, 0, -(1 << 511))
        inst.set_value(p, 0, inst.R - 1, (1 << 511) - 1)
        return p, roots, ev
    return ("entries that fill all 512 bits", mutate,
            dict(verdict=PROXIMITY_TESTING, column=0, bad_merkle_paths=inst.n_cols * inst.R, malformed_paths=0))


def many_rows_cases(inst):
    """The catalogue at 2048 rows, and three tampers that no thread meets at its first row: row 256 is the first row of
    a second iteration, row 2047 the last row of the last one, row 1300 lies in the sixth."""
    i = inst
    assert i.R == 2048 and i.n_cols > 9 and i.d >= 2
    out = tamper_cases(i) + [overflow_case(i)]
    out.append(("value[5,2047] bit 0", _flip_bit(i.val_at(5, 2047), 0), dict(verdict=PROXIMITY_TESTING, column=5)))
    out.append(("value[7,256] bit 0", _flip_bit(i.val_at(7, 256), 0), dict(verdict=PROXIMITY_TESTING, column=7)))
    out.append(("path[9,1300] level 1", _flip_bit(i.node_at(9, 1300, 1) + 17, 2), dict(verdict=MERKLE, column=9, bad_merkle_paths=1)))
    out.append(fill_512_case(i))
    return out


def wide_codeword_cases(inst):
    """What encode_wide(u') decides at a codeword of 1024 and more: both u' flips of the catalogue, the overflow and its
    companion one bit lower, and one value and one evaluation-row tamper (the rest of the verdict order) beside them."""
    i = inst
    picked = [c for c in tamper_cases(i) if c[0].startswith(("u'[", "value[0,0] bit 0", "evaluation row["))]
    assert len(picked) == 4, [c[0] for c in picked]
    return picked + [overflow_case(i), below_overflow_case(i)]
