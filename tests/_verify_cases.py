"""Proof builders, a tamper catalogue and a plain Python-int model of MultilinearZip::verify for the verifier tests.

No GPU and no ctypes beyond _oracle: tests/test_verify_cases_host.py confirms every expectation made here against the
CPU oracle, tests/test_gpu_verify_soundness.py then holds zip_verify to the same expectations.

Stream layout for num_rows > 1 (pcs_transcript.rs, open_z.rs:93-143):
    u'            row_len x 64 bytes, Int<8> little-endian
    per opening   num_rows x 32 bytes (Int<4> column entries), then num_rows records of be64(depth) | depth x 32 bytes
    evaluation    row_len x 8*fl bytes, big-endian Montgomery
"""
import ctypes as C
import functools

import numpy as np

import _oracle as orc

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59

# zip_verify_verdict (include/zip_hip.h)
ACCEPT, PROXIMITY_TESTING, EVAL_CONSISTENCY, PROXIMITY_Q0, MERKLE, MALFORMED, OVERFLOW = range(7)
VERDICT_NAMES = ["ACCEPT", "PROXIMITY_TESTING", "EVAL_CONSISTENCY", "PROXIMITY_Q0", "MERKLE", "MALFORMED", "OVERFLOW"]

# name -> (num_vars, (row_len, num_rows, codeword_len) or None for the reference's own geometry)
GEOMETRIES = {"base": (10, None), "tall": (11, (4, 512, 8)), "wide": (11, (1024, 2, 2048))}
INT8_MIN, INT8_MAX = -(1 << 511), (1 << 511) - 1  # Int<8>, the type of u' and of its encoding


def honest_tuple(num_vars, geometry, modulus, fl, seed=0, small=False):
    """An honest commit + open on the oracle: (z, f, evals, point, roots, proof, cols, coeffs, q0, q1, ev)."""
    z = orc.Zip(num_vars, geometry=geometry)
    f = orc.make_field(modulus, fl)
    n = 1 << num_vars
    if small:
        evals = np.random.default_rng(seed).integers(-128, 128, size=n, dtype=np.int64)
    else:
        evals = orc.splitmix64(0x5A494E43 + seed, n).copy()
        evals[: min(n, 3)] = np.array([-(2**63), 2**63 - 1, -1], dtype=np.int64)[: min(n, 3)]
    point = orc.point_to_field(f, np.random.default_rng(seed + 1).integers(-50, 50, size=num_vars, dtype=np.int64))
    rows, layers, roots = z.commit(evals)
    proof, cols, coeffs = z.open(f, evals, rows, layers, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:]) if lr else None
    q1 = orc.build_eq_x_r(f, point[: num_vars - lr]) if num_vars - lr else None
    ev = z.mle_eval(f, evals, point)
    return z, f, evals, point, roots, proof, cols, coeffs, q0, q1, ev


class Instance:
    """One proof with everything the verifiers need, and the byte offsets of its parts.  num_rows > 1, row_len > 1."""

    def __init__(self, z, modulus, fl, f, point, roots, proof, cols, coeffs, q0, q1, ev):
        self.z, self.modulus, self.fl, self.f, self.point = z, modulus, fl, f, point
        self.roots, self.proof, self.cols, self.coeffs, self.q0, self.q1, self.ev = roots, proof, cols, coeffs, q0, q1, ev
        self.R, self.C, self.cw, self.d, self.n_cols = z.num_rows, z.row_len, z.codeword_len, z.depth, len(cols)
        assert self.R > 1 and self.C > 1 and z.k_limbs == 4 and z.m_limbs == 8
        self.u_bytes = self.C * 64
        self.rec_bytes = 8 + 32 * self.d
        self.col_bytes = self.R * (32 + self.rec_bytes)
        self.row_off = self.u_bytes + self.n_cols * self.col_bytes
        self.need = self.row_off + self.C * 8 * fl
        assert proof.size == self.need
        # the field in plain integers: Montgomery radix 2^(64 fl)
        self.rm = (1 << (64 * fl)) % modulus
        self.rinv = pow(self.rm, -1, modulus)
        self.coeffs_int = [int(c) for c in coeffs]
        self.q0_std = [self.std(orc.limbs_to_int(x)) for x in q0]
        self.q1_std = [self.std(orc.limbs_to_int(x)) for x in q1]

    def std(self, mont):
        return mont * self.rinv % self.modulus

    def mont(self, std):
        return std * self.rm % self.modulus

    def val_at(self, k, r):
        return self.u_bytes + k * self.col_bytes + 32 * r

    def rec_at(self, k, r):
        return self.u_bytes + k * self.col_bytes + 32 * self.R + r * self.rec_bytes

    def node_at(self, k, r, level):
        return self.rec_at(k, r) + 8 + 32 * level

    def row_at(self, c):
        return self.row_off + c * 8 * self.fl

    def oracle_rc(self, proof, roots, ev):
        return self.z.verify(self.f, roots, self.point, ev, proof)  # check_merkle=True

    # ---- reading and writing the parts of a stream --------------------------------------------------------------
    def u_prime(self, proof):
        raw = proof[: self.u_bytes].tobytes()
        return [int.from_bytes(raw[64 * c: 64 * c + 64], "little", signed=True) for c in range(self.C)]

    def with_u_prime(self, proof, u):
        p = proof.copy()
        p[: self.u_bytes] = np.frombuffer(b"".join(int(x).to_bytes(64, "little", signed=True) for x in u), dtype=np.uint8)
        return p

    def value(self, proof, k, r):
        o = self.val_at(k, r)
        return int.from_bytes(proof[o: o + 32].tobytes(), "little", signed=True)

    def set_value(self, proof, k, r, v):
        o = self.val_at(k, r)
        proof[o: o + 32] = np.frombuffer(int(v).to_bytes(32, "little", signed=True), dtype=np.uint8)

    def row_elems(self, proof):
        """The evaluation row as the raw big-endian integers on the wire (Montgomery, not range-checked)."""
        n = 8 * self.fl
        raw = proof[self.row_off: self.need].tobytes()
        return [int.from_bytes(raw[n * c: n * c + n], "big") for c in range(self.C)]

    def set_row_elem(self, proof, c, x):
        n = 8 * self.fl
        proof[self.row_at(c): self.row_at(c) + n] = np.frombuffer(int(x).to_bytes(n, "big"), dtype=np.uint8)

    def dot_q1(self, row_wire):
        """<row, q1> as the Montgomery integer both verifiers compare with the claimed evaluation."""
        return self.mont(sum(self.std(x) * b for x, b in zip(row_wire, self.q1_std)) % self.modulus)


def raa_encode(z, row):
    """RAA over Python ints: repeat, out[j] = in[perm[j]], prefix sum, permute, prefix sum (code_raa.rs:89-171).
    Returns (codeword, lo, hi): the extreme values any running sum of either pass takes."""
    n = z.row_len
    cur = [row[int(p) % n] for p in z.perm1]
    lo = hi = 0
    for perm in (None, z.perm2):
        if perm is not None:
            cur = [cur[int(p)] for p in perm]
        acc = 0
        for j, x in enumerate(cur):
            acc += x
            cur[j] = acc
        lo, hi = min(lo, min(cur)), max(hi, max(cur))
    return cur, lo, hi


def honest(num_vars, geometry, modulus, fl, seed=0):
    z, f, evals, point, roots, proof, cols, coeffs, q0, q1, ev = honest_tuple(num_vars, geometry, modulus, fl, seed,
                                                                              small=(fl == 2))
    return Instance(z, modulus, fl, f, point, roots, proof, cols, coeffs, q0, q1, ev)


def wide_proof(num_vars, geometry, modulus, fl, seed=0, bits=240):
    """A proof the reference accepts whose column entries fill Int<4>: witness rows drawn in +-2^bits, far outside
    the i64 rows `commit` takes, so the commitment, u', the openings and the evaluation row are assembled here."""
    h = honest(num_vars, geometry, modulus, fl, seed)  # cols, coeffs, q0, q1 depend only on the fresh transcript
    z, R, Cn, d, q = h.z, h.R, h.C, h.d, modulus
    rng = np.random.default_rng(1000 + seed)

    def draw():
        x = int.from_bytes(rng.bytes(bits // 8), "little")
        return -x if rng.integers(2) else x

    W = [[draw() for _ in range(Cn)] for _ in range(R)]
    enc = [raa_encode(z, w)[0] for w in W]
    assert all(-(1 << 255) <= x < (1 << 255) for e in enc for x in e), "column entries must fit Int<4>"
    limbs = np.array([[orc.int_to_limbs(x, 4) for x in e] for e in enc], dtype=np.uint64)  # [R, cw, 4]
    layers = np.stack([orc.merkle_tree(d, limbs[r]) for r in range(R)])                     # [R, tree, 32]
    roots = np.ascontiguousarray(layers[:, -1, :])
    cols = h.cols.astype(np.int64)
    # the sibling of the node above leaf `col` at each level; layer l starts at sum_{i<l} 2^(d-i) (pcs/utils.rs:163-176)
    offs = np.cumsum([0] + [1 << (d - l) for l in range(d)])[:d]
    paths = np.stack([layers[:, offs[l] + ((cols >> l) ^ 1), :] for l in range(d)], axis=2)  # [R, n, d, 32]
    for k, r in ((0, 0), (len(cols) - 1, R - 1)):  # the gather above is orc.merkle_path, vectorised
        assert np.array_equal(paths[r, k], orc.merkle_path(d, layers[r], int(cols[k])))
    n = len(cols)
    rec = np.zeros((n, R, 8 + 32 * d), dtype=np.uint8)
    rec[:, :, :8] = np.frombuffer(d.to_bytes(8, "big"), dtype=np.uint8)
    rec[:, :, 8:] = paths.transpose(1, 0, 2, 3).reshape(n, R, 32 * d)
    vals = np.ascontiguousarray(limbs[:, cols, :].transpose(1, 0, 2)).view(np.uint8).reshape(n, R * 32)
    u = [sum(h.coeffs_int[r] * W[r][c] for r in range(R)) for c in range(Cn)]
    row_std = [sum(h.q0_std[r] * W[r][c] for r in range(R)) % q for c in range(Cn)]
    row_wire = [h.mont(x) for x in row_std]
    proof = np.concatenate([
        np.frombuffer(b"".join(x.to_bytes(64, "little", signed=True) for x in u), dtype=np.uint8),
        np.concatenate([vals, rec.reshape(n, -1)], axis=1).reshape(-1),
        np.frombuffer(b"".join(x.to_bytes(8 * fl, "big") for x in row_wire), dtype=np.uint8)])
    ev = h.dot_q1(row_wire)
    return Instance(z, modulus, fl, h.f, h.point, roots, proof, h.cols, h.coeffs, h.q0, h.q1, ev)


@functools.lru_cache(maxsize=None)
def instance(geometry, modulus, fl, wide_entries=False):
    """The shared instances of the tests, built once per process and never modified."""
    nv, geo = GEOMETRIES[geometry]
    inst = (wide_proof if wide_entries else honest)(nv, geo, modulus, fl, seed=5)
    inst.name = f"{geometry}-fl{fl}" + ("-wide-entries" if wide_entries else "")
    inst.model = Model(inst)
    for a in (inst.proof, inst.roots):
        a.setflags(write=False)
    return inst


# ---------------------------------------------------------------------------------------------------------------------
# The model: the reference's order of checks (verify_z.rs:60-188) over Python ints, with the device's report fields.
# ---------------------------------------------------------------------------------------------------------------------
class Expect:
    """report: what zip_verify must return.  oracle: the class of the oracle's return code --
    'accept' (0), 'overflow' (ORC_ERR_OVERFLOW), 'transcript' (ORC_ERR_TRANSCRIPT: short stream, or the first record
    the oracle reads with a wrong length prefix has one above 64), 'noncanonical' (0 or ORC_ERR_PROOF, see the host
    test), 'reject' (any non-zero)."""

    def __init__(self, verdict, column, bad, malformed, oracle):
        self.report = {"verdict": verdict, "column": column, "bad_merkle_paths": bad, "malformed_paths": malformed}
        self.oracle = oracle

    def __repr__(self):
        return f"Expect({VERDICT_NAMES[self.report['verdict']]}, {self.report}, oracle={self.oracle})"


class Model:
    """Evaluates every opening of the instance's own proof once; report() re-evaluates only the openings whose bytes
    (or whose rows' roots) differ from it, which keeps a 70 MB proof affordable."""

    def __init__(self, inst):
        self.i = inst
        self.base_sec = inst.proof[inst.u_bytes: inst.row_off].reshape(inst.n_cols, inst.col_bytes)
        self.base_roots = inst.roots
        self.prefix = np.frombuffer(inst.d.to_bytes(8, "big"), dtype=np.uint8)
        all_rows = range(inst.R)
        self.facts = [self._opening(inst.proof, inst.roots, k, all_rows, None) for k in range(inst.n_cols)]

    def _opening(self, proof, roots, k, merkle_rows, old):
        """(sum_r coeffs[r] v[r], sum_r q0[r] phi(v[r]) in standard form, {row: wrong prefix}, {rows whose path misses
        the root}).  With `old`, only merkle_rows are hashed again and the rest is kept."""
        i = self.i
        if old is None:
            raw = proof[i.val_at(k, 0): i.val_at(k, 0) + 32 * i.R].tobytes()
            v = [int.from_bytes(raw[32 * r: 32 * r + 32], "little", signed=True) for r in range(i.R)]
            isum = sum(c * x for c, x in zip(i.coeffs_int, v))
            fsum = sum(a * x for a, x in zip(i.q0_std, v)) % i.modulus  # phi(v) = sign (|v| mod q) = v mod q
            recs = proof[i.rec_at(k, 0): i.rec_at(k, 0) + i.R * i.rec_bytes].reshape(i.R, i.rec_bytes)
            mal = {int(r): int.from_bytes(recs[r, :8].tobytes(), "big")
                   for r in np.flatnonzero((recs[:, :8] != self.prefix).any(axis=1))}
            bad = set()
        else:
            isum, fsum, mal, bad = old
            bad = bad - set(merkle_rows)
        L, pa, ra, col = orc.lib(), proof.ctypes.data, roots.ctypes.data, int(i.cols[k])
        for r in merkle_rows:
            if r not in mal and L.orc_merkle_verify(i.d, C.c_void_p(pa + i.rec_at(k, r) + 8), C.c_void_p(ra + 32 * r),
                                                    C.c_void_p(pa + i.val_at(k, r)), 4, col) != 0:
                bad.add(r)
        return isum, fsum, mal, bad

    def report(self, proof, roots, ev):
        i, q = self.i, self.i.modulus
        proof = np.ascontiguousarray(proof, dtype=np.uint8)
        roots = np.ascontiguousarray(roots, dtype=np.uint8)
        if proof.size < i.need:  # the reference runs out of stream; the device looks no further
            return Expect(MALFORMED, 0, 0, 0, "transcript")
        facts = list(self.facts)
        sec = proof[i.u_bytes: i.row_off].reshape(i.n_cols, i.col_bytes)
        changed = set(int(k) for k in np.flatnonzero((sec != self.base_sec).any(axis=1)))
        for k in changed:
            facts[k] = self._opening(proof, roots, k, range(i.R), None)
        rows = [int(r) for r in np.flatnonzero((roots != self.base_roots).any(axis=1))]
        if rows:
            for k in range(i.n_cols):
                if k not in changed:
                    facts[k] = self._opening(proof, roots, k, rows, facts[k])
        n_bad = sum(len(f[3]) for f in facts)
        n_mal = sum(len(f[2]) for f in facts)
        # encode_wide(u') with checked additions (verify_z.rs:75-77, int.rs:122-134)
        enc_u, lo, hi = raa_encode(i.z, i.u_prime(proof))
        overflow = lo < INT8_MIN or hi > INT8_MAX
        # per opening: the proximity test over Z, then its Merkle records in stream order (verify_z.rs:88-127)
        first, why = None, 0
        for k, (isum, _, mal, bad) in enumerate(facts):
            why = ((FAILS_PROXIMITY if isum != enc_u[int(i.cols[k])] else 0) | (FAILS_MALFORMED if mal else 0)
                   | (FAILS_MERKLE if bad else 0))
            if why:
                first = k
                break
        # verify_evaluation_z (verify_z.rs:129-163); elements >= q: the device's deliberate deviation
        wire = i.row_elems(proof)
        eval_differs = i.dot_q1(wire) != ev
        noncanonical = any(x >= q for x in wire)
        enc_f = raa_encode(i.z, [i.std(x) for x in wire])[0]
        first_q0 = next((k for k, (_, fsum, _, _) in enumerate(facts)  # verify_proximity_q_0 (verify_z.rs:165-188)
                         if fsum != enc_f[int(i.cols[k])] % q), None)
        verdict, column = verdict_order(overflow, first, why, eval_differs, noncanonical, first_q0)
        oracle = {ACCEPT: "accept", OVERFLOW: "overflow"}.get(verdict, "reject")
        if verdict == MALFORMED:
            mal = facts[first][2] if first is not None else None
            oracle = "noncanonical" if mal is None else "transcript" if mal[min(mal)] > 64 else "reject"
        return Expect(verdict, column, n_bad, n_mal, oracle)


# what an opening fails, as bits (zinc_amd/csrc/verify_verdict.h passes the same facts)
FAILS_PROXIMITY, FAILS_MALFORMED, FAILS_MERKLE = 1, 2, 4


def verdict_order(overflow, first, why, eval_differs, noncanonical, first_q0):
    """(verdict, column) from the reduced facts, in the reference's order of checks (verify_z.rs:60-188): first = the first
    opening that fails its proximity test over Z, a length prefix or a path (None: no opening does) and why = which of
    those, as FAILS_* bits; first_q0 = the first opening that fails the proximity test over F_q."""
    if overflow:
        return OVERFLOW, 0
    if first is not None:  # per opening: proximity, then its records in stream order
        if why & FAILS_PROXIMITY:
            return PROXIMITY_TESTING, first
        return (MALFORMED if why & FAILS_MALFORMED else MERKLE), first
    if eval_differs:
        return EVAL_CONSISTENCY, 0
    if noncanonical:  # after the consistency check
        return MALFORMED, 0
    if first_q0 is not None:
        return PROXIMITY_Q0, first_q0
    return ACCEPT, 0


def expected_report(inst, proof, roots, ev):
    return inst.model.report(proof, roots, ev)


# ---------------------------------------------------------------------------------------------------------------------
# The tamper catalogue.  Case.mutate(proof, roots, ev) -> (proof, roots, ev) never writes into its arguments.
# Case.claim: what the construction itself promises (a subset of the report's fields); the host test holds the model
# to it, so a claim and the model can only be wrong together with the oracle noticing.
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, mutate, **claim):
        self.name, self.mutate, self.claim = name, mutate, claim

    def __repr__(self):
        return self.name


def _flip(*ats):
    """XOR bytes of the proof: (offset, mask) pairs."""
    def mutate(proof, roots, ev):
        p = proof.copy()
        for at, mask in ats:
            p[at] ^= mask
        return p, roots, ev
    return mutate


def _flip_root(r):
    def mutate(proof, roots, ev):
        ro = roots.copy()
        ro[r, 0] ^= 1
        return proof, ro, ev
    return mutate


def _chain(*mutators):
    def mutate(proof, roots, ev):
        for m in mutators:
            proof, roots, ev = m(proof, roots, ev)
        return proof, roots, ev
    return mutate


def _openings(inst):
    return [0, inst.n_cols // 2, inst.n_cols - 1]


def _rows(inst):
    return [0, inst.R - 1] + ([255, 256] if inst.R > 256 else [])


def value_cases(inst):
    """Column entries: lowest bit and sign bit, first / middle / last opening, first / last row and, where there are
    two 256-row blocks, both sides of their border."""
    i, out = inst, []
    for k in _openings(i):
        for r in _rows(i):
            out.append(Case(f"value[{k},{r}] limb 0 bit 0", _flip((i.val_at(k, r), 1)),
                            verdict=PROXIMITY_TESTING, column=k, bad_merkle_paths=1, malformed_paths=0))
            out.append(Case(f"value[{k},{r}] limb 3 bit 63", _flip((i.val_at(k, r) + 31, 0x80)),
                            verdict=PROXIMITY_TESTING, column=k, bad_merkle_paths=1, malformed_paths=0))
    return out


def position_cases(inst):
    """Every other section of the stream, the roots, the claimed evaluation and the stream's length."""
    i, out = inst, []
    even = next(k for k in range(i.n_cols) if i.cols[k] % 2 == 0)
    odd = next(k for k in range(i.n_cols) if i.cols[k] % 2 == 1)
    for k, r in ((even, i.R - 1), (odd, 0)):
        for level in range(i.d):
            out.append(Case(f"path[{k},{r}] level {level} (column {int(i.cols[k])})",
                            _flip((i.node_at(k, r, level) + 5, 0x10)),
                            verdict=MERKLE, column=k, bad_merkle_paths=1, malformed_paths=0))
    k, r = i.n_cols // 2, i.R - 1
    for byte in (0, 7):
        out.append(Case(f"prefix[{k},{r}] byte {byte}", _flip((i.rec_at(k, r) + byte, 1)),
                        verdict=MALFORMED, column=k, bad_merkle_paths=0, malformed_paths=1))
    for c in (0, i.C // 2, i.C - 1):
        out.append(Case(f"u'[{c}]", _flip((64 * c + 1, 1)), verdict=PROXIMITY_TESTING, bad_merkle_paths=0))
    for c in (0, i.C - 1):
        # (a point with a coordinate 1 has q1[c] == 0 for half the c: <row, q1> then cannot see element c, the
        # proximity check over F_q still does)
        out.append(Case(f"evaluation row[{c}]", _flip((i.row_at(c) + 8 * i.fl - 1, 1)),
                        verdict=EVAL_CONSISTENCY if i.q1_std[c] else PROXIMITY_Q0, bad_merkle_paths=0, malformed_paths=0))
    out.append(Case("wrong claimed evaluation", lambda p, ro, ev: (p, ro, (ev + 1) % i.modulus),
                    verdict=EVAL_CONSISTENCY, column=0, bad_merkle_paths=0, malformed_paths=0))
    for r in (0, i.R - 1):
        out.append(Case(f"root[{r}]", _flip_root(r),
                        verdict=MERKLE, column=0, bad_merkle_paths=i.n_cols, malformed_paths=0))
    out.append(Case("one byte short", lambda p, ro, ev: (p[:-1], ro, ev),
                    verdict=MALFORMED, column=0, bad_merkle_paths=0, malformed_paths=0))
    out.append(Case("40 bytes of trailing garbage",
                    lambda p, ro, ev: (np.concatenate([p, np.arange(7, 47, dtype=np.uint8)]), ro, ev),
                    verdict=ACCEPT, column=0, bad_merkle_paths=0, malformed_paths=0))
    return out


def count_cases(inst):
    """5 path records and 3 length prefixes, all distinct, over several openings (num_rows >= 8)."""
    i = inst
    last = i.n_cols - 1
    paths = [(5, 0), (5, i.R - 1), (9, 3), (i.n_cols // 2, 1), (last, i.R - 1)]
    prefixes = [(5, 1), (7, 0), (i.n_cols // 2, i.R - 1)]
    hit = [(i.node_at(k, r, (k + r) % i.d) + 9, 0x40) for k, r in paths]
    both = _flip(*hit, *[(i.rec_at(k, r) + 7, 2) for k, r in prefixes])
    # the same without the prefix in opening 5: the first affected opening then only has bad paths
    later = _flip(*hit, *[(i.rec_at(k, r) + 7, 2) for k, r in [(6, 1)] + prefixes[1:]])
    return [Case("5 paths + 3 prefixes, malformed first", both,
                 verdict=MALFORMED, column=5, bad_merkle_paths=5, malformed_paths=3),
            Case("5 paths + 3 prefixes, merkle first", later,
                 verdict=MERKLE, column=5, bad_merkle_paths=5, malformed_paths=3)]


def _combo(inst, k, r, s):
    def mutate(proof, roots, ev):
        p = proof.copy()
        inst.set_value(p, k, r, inst.value(p, k, r) + inst.coeffs_int[s])
        inst.set_value(p, k, s, inst.value(p, k, s) - inst.coeffs_int[r])
        return p, roots, ev
    return mutate


def combination_cases(inst):
    """v[r] += coeffs[s], v[s] -= coeffs[r]: sum_r coeffs[r] v[r] is unchanged, two leaves are not."""
    i = inst
    k = i.n_cols // 3
    pairs = [(1, i.R - 2)] + ([(3, 300)] if i.R > 256 else [])  # (3, 300): two different 256-row blocks
    return [Case(f"combination preserving [{k}: {r},{s}]", _combo(i, k, r, s),
                 verdict=MERKLE, column=k, bad_merkle_paths=2, malformed_paths=0) for r, s in pairs]


def _q0_only(inst, c):
    """Replaces evaluation-row element c and claims the evaluation that the new row gives."""
    def mutate(proof, roots, ev):
        p = proof.copy()
        wire = inst.row_elems(p)
        wire[c] = (wire[c] % inst.modulus + 1) % inst.modulus
        inst.set_row_elem(p, c, wire[c])
        return p, roots, inst.dot_q1(wire)
    return mutate


def _q0_only_later(inst):
    """Adds delta to evaluation-row elements 0 and 1 with enc(delta)[cols[0]] == 0 and claims the evaluation of the
    new row: the proximity check over F_q first fails at a later opening.  Returns (mutate, that opening)."""
    i, q = inst, inst.modulus
    j0 = int(i.cols[0])
    e0 = raa_encode(i.z, [int(j == 0) for j in range(i.C)])[0]
    e1 = raa_encode(i.z, [int(j == 1) for j in range(i.C)])[0]
    delta = (e1[j0], -e0[j0])
    later = next(k for k in range(i.n_cols) if (delta[0] * e0[int(i.cols[k])] + delta[1] * e1[int(i.cols[k])]) % q)

    def mutate(proof, roots, ev):
        p = proof.copy()
        wire = i.row_elems(p)
        for c in (0, 1):
            wire[c] = i.mont((i.std(wire[c]) + delta[c]) % q)
            i.set_row_elem(p, c, wire[c])
        return p, roots, i.dot_q1(wire)
    return mutate, later


def wide_entry_cases(inst):
    i = inst
    k, r = i.n_cols // 2 + 1, i.R // 2
    q0_later, later = _q0_only_later(i)
    assert later > 0
    return [Case(f"wide value[{k},{r}] sign bit", _flip((i.val_at(k, r) + 31, 0x80)),
                 verdict=PROXIMITY_TESTING, column=k, bad_merkle_paths=1, malformed_paths=0),
            *combination_cases(i),
            Case("evaluation row consistent with its claim, rows are not", _q0_only(i, 1),
                 verdict=PROXIMITY_Q0, bad_merkle_paths=0, malformed_paths=0),
            Case(f"the same, invisible to opening 0 and first seen in opening {later}", q0_later,
                 verdict=PROXIMITY_Q0, column=later, bad_merkle_paths=0, malformed_paths=0)]


def _set_u(inst, sparse):
    return lambda p, ro, ev: (inst.with_u_prime(p, [sparse.get(c, 0) for c in range(inst.C)]), ro, ev)


def overflow_elements(inst):
    """Base: both ends of the row.  Wide: the elements that pass 0 reads at codeword positions 0 and 1, the two halves
    of the first thread's chunk when each thread owns two positions."""
    if inst.cw > 1024:
        return sorted({int(inst.z.perm1[0]) % inst.C, int(inst.z.perm1[1]) % inst.C})
    return [0, inst.C - 1]


def overflow_cases(inst):
    """u' = v e_c.  Every running sum of enc(e_c) is non-negative and non-decreasing, so the largest is m_c, its last
    entry, and v e_c overflows Int<8> exactly when v m_c leaves [-2^511, 2^511 - 1]."""
    i, out = inst, []
    for c in overflow_elements(i):
        unit, lo, hi = raa_encode(i.z, [int(j == c) for j in range(i.C)])
        m = max(unit)
        assert lo == 0 and hi == m == unit[-1] and m > 1
        top, bottom = INT8_MAX // m, -((1 << 511) // m)
        for name, v, verdict in ((f"u' = {c}: largest that fits", top, PROXIMITY_TESTING),
                                 (f"u' = {c}: largest that fits + 1", top + 1, OVERFLOW),
                                 (f"u' = {c}: smallest that fits", bottom, PROXIMITY_TESTING),
                                 (f"u' = {c}: smallest that fits - 1", bottom - 1, OVERFLOW)):
            out.append(Case(name, _set_u(i, {c: v}), verdict=verdict, column=0, bad_merkle_paths=0, malformed_paths=0))
    out.append(Case("u' = {0: max, 1: -max}: total 0, a prefix overflows", _set_u(i, {0: INT8_MAX, 1: -INT8_MAX}),
                    verdict=OVERFLOW, column=0, bad_merkle_paths=0, malformed_paths=0))
    return out


def _noncanonical(inst, c):
    def mutate(proof, roots, ev):
        p = proof.copy()
        x = inst.row_elems(p)[c]
        assert x < inst.modulus and x + inst.modulus < 1 << (64 * inst.fl), "x + q must fit the element's bytes"
        inst.set_row_elem(p, c, x + inst.modulus)
        return p, roots, ev
    return mutate


def noncanonical_cases(inst):
    """x + q in place of x (fields whose elements leave room for it): the same residue, another representation."""
    i = inst
    wrong_eval = lambda p, ro, ev: (p, ro, (ev + 1) % i.modulus)
    return [*[Case(f"non-canonical evaluation row[{c}]", _noncanonical(i, c),
                   verdict=MALFORMED, column=0, bad_merkle_paths=0, malformed_paths=0) for c in (0, i.C - 1)],
            Case("wrong evaluation + non-canonical element", _chain(_noncanonical(i, 2), wrong_eval),
                 verdict=EVAL_CONSISTENCY, column=0, bad_merkle_paths=0, malformed_paths=0),
            Case("non-canonical element + q0-only failure", _chain(_q0_only(i, 1), _noncanonical(i, i.C - 2)),
                 verdict=MALFORMED, column=0, bad_merkle_paths=0, malformed_paths=0)]


def precedence_cases(inst):
    i = inst
    c = overflow_elements(i)[0]
    m = max(raa_encode(i.z, [int(j == c) for j in range(i.C)])[0])
    out = [Case("overflow + value tamper", _chain(_set_u(i, {c: INT8_MAX // m + 1}), _flip((i.val_at(1, 1), 4))),
                verdict=OVERFLOW, column=0, bad_merkle_paths=1, malformed_paths=0)]
    # u' + delta with enc(delta)[cols[0]] == 0: opening 0 still passes the proximity test, a later one does not
    j0 = int(i.cols[0])
    e0 = raa_encode(i.z, [int(j == 0) for j in range(i.C)])[0]
    e1 = raa_encode(i.z, [int(j == 1) for j in range(i.C)])[0]
    delta = {0: e1[j0], 1: -e0[j0]}
    enc_delta = [delta[0] * a + delta[1] * b for a, b in zip(e0, e1)]
    later = next((k for k in range(i.n_cols) if enc_delta[int(i.cols[k])]), None)
    if later is not None:  # (always, unless every opened column sits where enc(e_0) and enc(e_1) are proportional)
        def add_delta(p, ro, ev):
            u = i.u_prime(p)
            return i.with_u_prime(p, [u[0] + delta[0], u[1] + delta[1]] + u[2:]), ro, ev
        assert later > 0
        out.append(Case(f"path tamper in opening 0 + u' tamper first seen in opening {later}",
                        _chain(add_delta, _flip((i.node_at(0, 1, 0), 1))),
                        verdict=MERKLE, column=0, bad_merkle_paths=1, malformed_paths=0))
        out.append(Case("the u' tamper of the case above alone", add_delta,
                        verdict=PROXIMITY_TESTING, column=later, bad_merkle_paths=0, malformed_paths=0))
    return out


# (instance key, case group) pairs: what the host test confirms on the oracle and the GPU test runs on the device
FIELDS_BASE = [(BENCH_MODULUS, 4), (MOD_3LIMB, 3), (TEST_MODULUS_2, 2)]
PLAN = (
    [(("base", q, fl, False), g) for q, fl in FIELDS_BASE for g in ("value", "position", "count", "combination", "precedence")]
    + [(("base", q, fl, True), "wide_entry") for q, fl in FIELDS_BASE]
    + [(("base", BENCH_MODULUS, 4, False), "overflow"), (("base", MOD_3LIMB, 3, False), "noncanonical"),
       (("base", TEST_MODULUS_2, 2, False), "noncanonical")]
    + [(("tall", BENCH_MODULUS, 4, False), g) for g in ("value", "position", "count", "combination", "overflow")]
    + [(("tall", BENCH_MODULUS, 4, True), "wide_entry")]
    + [(("wide", MOD_3LIMB, 3, False), g) for g in ("overflow", "noncanonical", "precedence")]
    + [(("wide", TEST_MODULUS_2, 2, False), "noncanonical")]
)
GROUPS = {"value": value_cases, "position": position_cases, "count": count_cases, "combination": combination_cases,
          "wide_entry": wide_entry_cases, "overflow": overflow_cases, "noncanonical": noncanonical_cases,
          "precedence": precedence_cases}


def plan_id(entry):
    (geometry, _, fl, wide_entries), group = entry
    return f"{geometry}-fl{fl}{'-wide-entries' if wide_entries else ''}-{group}"


def cases(key, group):
    """[(name, mutate, Expect)] for one instance and one group."""
    inst = instance(*key)
    out = []
    for c in GROUPS[group](inst):
        want = expected_report(inst, *c.mutate(inst.proof, inst.roots, inst.ev))
        out.append((c, want))
    return inst, out
