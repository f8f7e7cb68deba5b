"""One random sparse circuit shared by several proofs (test data, no field arithmetic), for the batch entry points:

  circuit(s, t, seed)      t CSR matrices of 2^s columns with everything a sparse kernel can trip over:
                             - 0..4 entries per row, in distinct columns;
                             - matrix 0 hits column `hot` = 2^s / 2 in EVERY row (one long CSC column);
                             - matrix 1 has fewer rows than 2^s (its missing rows are zero rows);
                             - row 2^s / 3 is empty in every matrix but the first, column 0 is empty in every matrix;
                             - the stored values start with 1, -1, 5, INT64_MIN, INT64_MAX and an explicit 0, spread over
                               the first entries of the matrices, then mix small values and full 63-bit ones.
                           The circuit is NOT satisfied by anything: it feeds table and prover comparisons, where only
                           the arithmetic matters.
  witnesses(s, n, seed)    n vectors z = (x, 1, w) of int64 over the full range; every third one is shorter than 2^s
  instances(s, t, zs, ..)  _ccs.CcsInstance per z, all sharing the matrix objects of one circuit

  MODULI                   per limb count, the fields the members of one call draw from

2^s = 2 or 4 has no room for all of the above at once; what fits is kept (features() says what a circuit has)."""
import functools

import numpy as np

import _ccs

Q256 = 115792089237316195423570985008687907853269984665640564039457584007913129639747  # spartan_benches.rs:152 (top bit set)
QSTARK = 3618502788666131213697322783095070105623107215331596699973092056135872020481  # spartan_benches.rs:161
QBENCH = 106319353542452952636349991594949358997917625194731877894581586278529202198383
Q192 = 312829638388039969874974628075306023441          # zinc/tests.rs:28
Q128 = 57316695564490278656402085503
# per limb count: different moduli for the members of one call; each set has one with the top bit set whose distance
# to 2^(64 limbs) fits a limb (the quirk_mod path of field_from_i64)
MODULI = {
    2: [Q128, (1 << 127) - 1, (1 << 128) - 159, (1 << 107) - 1],
    3: [Q192, (1 << 192) - 237, (1 << 191) - 19, (1 << 160) - 47],
    4: [Q256, QSTARK, QBENCH, (1 << 255) - 19],
}

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SPECIAL = (1, -1, 5, INT64_MIN, INT64_MAX, 0)
_SMALL = (1, -1, 5, 2, -7)


def _shape(t):
    """S pairs the matrices up in order, the last term is a single matrix: (S, c, d)"""
    S = [[j, j + 1] for j in range(0, t - 1, 2)]
    if t % 2:
        S.append([t - 1])
    c = [(1, -1, 5, -1)[i % 4] for i in range(len(S))]
    return S, c, max(len(Si) for Si in S)


@functools.lru_cache(maxsize=None)
def circuit(s, t=7, seed=0xC0FFEE):
    """-> (matrices, S, c, d); shared between tests: read-only"""
    m = 1 << s
    rng = np.random.default_rng(seed + 1000 * s + t)
    hot, dead, empty_row = m // 2, 0, m // 3
    usable = [col for col in range(m) if col not in (hot, dead)]
    usable_hot = usable + [hot]
    # everything random is drawn up front: per (row, matrix) a count, four column picks and four values
    want = rng.integers(0, 5, size=(m, t)).tolist()
    pick = rng.integers(0, 1 << 30, size=(m, t, 4)).tolist()
    small = rng.integers(0, 3, size=(m, t, 4)).astype(bool)
    value = np.where(small, np.array(_SMALL)[rng.integers(0, len(_SMALL), size=(m, t, 4))],
                     rng.integers(INT64_MIN, INT64_MAX, size=(m, t, 4), endpoint=True)).tolist()
    # row by row across the matrices, so the special values land in several of them
    n_rows = [m - 1 - m // 8 if k == 1 else m for k in range(t)]
    rows = [[[] for _ in range(n_rows[k])] for k in range(t)]
    n_entry = 0
    for r in range(m):
        for k in range(t):
            if r >= n_rows[k] or (k and r == empty_row):
                continue
            cols = {hot} if k == 0 else set()
            pool = usable if k == 0 else usable_hot
            if pool:
                for j in range(want[r][k] - len(cols)):
                    cols.add(pool[pick[r][k][j] % len(pool)])  # (a repeated pick: one entry fewer)
            for j, col in enumerate(sorted(cols)):
                v = SPECIAL[n_entry] if n_entry < len(SPECIAL) else value[r][k][j]
                n_entry += 1
                rows[k][r].append((v, col))
    mats = [_ccs.CsrMatrix(n_rows[k], m, rows[k]) for k in range(t)]
    S, c, d = _shape(t)
    return tuple(mats), S, c, d


def features(mats):
    """what a circuit really has (the smallest sizes cannot hold everything)"""
    m = mats[0].n_cols
    vals = np.concatenate([M.values for M in mats])
    return dict(
        full_column=any(np.bincount(M.col_idx, minlength=m).max(initial=0) == M.n_rows == m for M in mats),
        short_matrix=any(M.n_rows < m for M in mats),
        empty_row=any((np.diff(M.row_ptr.astype(np.int64)) == 0).any() for M in mats),
        empty_column=all((np.bincount(M.col_idx, minlength=m) == 0).any() for M in mats),
        max_row=max(int(np.diff(M.row_ptr.astype(np.int64)).max(initial=0)) for M in mats),
        specials=all(v in vals for v in SPECIAL),
    )


def witnesses(s, n, seed=0x5EED):
    m = 1 << s
    rng = np.random.default_rng(seed + s)
    out = []
    for i in range(n):
        length = m if i % 3 != 1 else max(1, m - 1 - m // 5)
        z = rng.integers(INT64_MIN, INT64_MAX, size=length, endpoint=True, dtype=np.int64)
        z[i % length] = (INT64_MIN, INT64_MAX, 0, -1)[i % 4]
        if length > 1:
            z[1] = 1
        out.append(z)
    return out


def instances(s, t, zs, seed=0xC0FFEE):
    mats, S, c, d = circuit(s, t, seed)
    m = 1 << s
    return [_ccs.CcsInstance(m, m, s, s, d, list(mats), S, c, z) for z in zs]
