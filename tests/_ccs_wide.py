"""CCS instances with four to seven matrices as plain CSR arrays (test data, no field arithmetic): the shapes whose
first sumcheck runs over five to eight tables (M_0 z .. M_{t-1} z, eq).

  wide_ccs(s, S, c, seed)   a satisfied instance with m = n = 2^s for any S that lists 0..t-1 in order and whose last
                            term is one matrix with coefficient 1 or -1
  SHAPES                    the five shapes the tests use; instance(name, s) builds one
  bumped(inst)              the same circuit with the last witness entry off by one (row n - 3 no longer holds)
"""
import functools

import numpy as np

import _ccs

_MASK = (1 << 64) - 1
_VALUES = (1, 2, -1, 3)


def _stream(seed):
    """SplitMix64, one word per next()"""
    x = seed & _MASK
    while True:
        x = (x + 0x9E3779B97F4A7C15) & _MASK
        v = x
        v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
        v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & _MASK
        yield v ^ (v >> 31)


def _generate(s, S, c, seed):
    """-> (rows of the t matrices, z) in Python integers"""
    n = 1 << s
    t = sum(len(Si) for Si in S)
    assert [j for Si in S for j in Si] == list(range(t)) and len(S) == len(c)
    assert len(S[-1]) == 1 and c[-1] in (1, -1)
    rnd = _stream(seed)
    z = [0] * n
    z[0], z[1] = 3, 1
    rows = [[] for _ in range(t)]
    for r in range(n - 2):
        out = r + 2
        total = 0
        for Si, ci in zip(S[:-1], c[:-1]):
            prod = 1
            for j in Si:
                entries = {}
                for _ in range(1 + next(rnd) % 2):
                    v, col = _VALUES[next(rnd) % 4], next(rnd) % min(out, 4)
                    entries[col] = entries.get(col, 0) + v  # duplicate columns are merged
                row = sorted((col, v) for col, v in entries.items() if v)
                rows[j].append([(v, col) for col, v in row])
                prod *= sum(v * z[col] for col, v in row)
            total += ci * prod
        rows[S[-1][0]].append([(1, out)])
        z[out] = -c[-1] * total
    return rows, z


def wide_ccs(s, S, c, seed):
    """Row r < n - 2 fixes z[r + 2]: every matrix of every term but the last has one or two small entries in columns that
    are already known (below min(r + 2, 4)), the last term is the single entry (1, r + 2), and z[r + 2] is chosen so
    that sum_i c_i prod_{j in S_i} (M_j z)[r] = 0.  The last two rows are empty.  The witness must fit i64 with room."""
    rows, z = _generate(s, S, c, seed)
    assert max(abs(v) for v in z) < 1 << 62
    n = 1 << s
    mats = [_ccs.CsrMatrix(n, n, rows[j]) for j in range(len(rows))]
    return _ccs.CcsInstance(n, n, s, s, max(len(Si) for Si in S), mats, [list(Si) for Si in S], c, z)


# name -> (S, c): MLEs of the first sumcheck = t + 1, its degree = d + 1
SHAPES = {
    "plonk6": ([[0], [1], [2], [3, 4], [5]], [2, 1, -1, 1, -1]),     # qL a + qR b + qO c + qM a b + qC: 7 / 3
    "t7d3": ([[0, 1, 2], [3, 4], [5], [6]], [1, 2, -3, 1]),          # 8 / 4
    "t5d3": ([[0, 1, 2], [3], [4]], [1, -1, 1]),                     # 6 / 4
    "t4": ([[0, 1], [2], [3]], [1, -1, -1]),                         # 5 / 3
    "t7d2": ([[0, 1], [2, 3], [4, 5], [6]], [1, -1, 5, -1]),         # 8 / 3
}


@functools.lru_cache(maxsize=None)
def _seed(name, s):
    """z[2] and z[3] feed every later row, through products of up to three sums: the first seed from the shape's own
    start whose witness stays below 2^62"""
    S, c = SHAPES[name]
    seed = 0x5A494E43 + 131 * s + sum(name.encode())
    while max(abs(v) for v in _generate(s, S, c, seed)[1]) >= 1 << 62:
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def instance(name, s):
    """(shared between tests: read-only)"""
    S, c = SHAPES[name]
    return wide_ccs(s, S, c, _seed(name, s))


def bumped(inst):
    z = inst.z.copy()
    z[-1] += 1
    return _ccs.CcsInstance(inst.m, inst.n, inst.s, inst.s_prime, inst.d, inst.matrices, inst.S, inst.c, z)


def row_identity_holds(inst):
    """sum_i c_i prod_{j in S_i} (M_j z)[r] == 0 for every row, in Python integers"""
    z = [int(v) for v in inst.z]
    mz = []
    for M in inst.matrices:
        ptr, col, val = M.row_ptr.tolist(), M.col_idx.tolist(), M.values.tolist()
        mz.append([sum(val[e] * z[col[e]] for e in range(ptr[r], ptr[r + 1])) for r in range(M.n_rows)])
    for r in range(inst.m):
        total = 0
        for Si, ci in zip(inst.S, inst.c):
            prod = 1
            for j in Si:
                prod *= mz[j][r]
            total += ci * prod
        if total:
            return False
    return True
