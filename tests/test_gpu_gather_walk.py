"""The packed gather whose addressing stays on the scalar unit (open_columns_ilv_scalar_kernel), bit-exact against the
CPU oracle: there are no tolerances here.  Needs a real MI355X.

run_open_columns (zip_hip.hip) takes that kernel for a packed handle whose launch has its table (wg_tab) and whose
blocks are all 32 or 64 whole rows at depth 12 .. 14: raw buffer loads and stores, the lane's share of an address a
32-bit offset inside the block's span, the opening's share scalar.  (The file's name is of the form that was measured
first, a workgroup walking 5 openings of its row block; the column counts below sat on that walk's edges and on both
rules of its table -- 8 | n or not, as gather_order has them -- and they still cover one opening, repeated columns,
both neighbours of a pair, the sorted list and the eighths per XCD.)

  geometry (row_len, rows, cw)   depth   instance (rows per block)
  B  (2048, 128, 4096)           12      scalar<1, 12>: no `has3` lanes; two chunks of 64 rows = two launches of 2 blocks
  C  (4096, 64, 8192)            13      scalar<1, 13>: the benchmark's instance, `has3` on wave 0
  D  (8192, 64, 16384)           14      scalar<1, 14> under STREAM=0 RPB=32 (by default this geometry gathers without
                                         an image, through open_columns_ilv_kernel<false, 1>: unchanged)
                                         scalar<2, 14> under STREAM=0 RPB=64: D commits in one chunk of 64 rows
  RPB=64                                 scalar<2, D>: two passes per block
  RPB=40                                 blocks of 40 + 24 rows: not whole, open_columns_ilv_kernel's general loop"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _oracle as orc
from _openings import _expected_openings

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
KNOB_NAMES = ("ZIP_HIP_GATHER_RPB", "ZIP_HIP_GATHER_STREAM", "ZIP_HIP_CHUNK_ROUNDS", "ZIP_HIP_NO_COMPACT_ROWS",
              "ZIP_HIP_CHUNKS", "ZIP_HIP_PACKED", "ZIP_HIP_CLASSES", "ZIP_HIP_FORCE_WAIT_TIMEOUT")
GEOS = {"B": (18, (2048, 128, 4096)), "C": (18, (4096, 64, 8192)), "D": (19, (8192, 64, 16384))}
WALK = 5  # the walk that was measured (see above)
KNOBS = {
    "none": {},
    "rpb64": {"ZIP_HIP_GATHER_RPB": "64"},
    "rpb40": {"ZIP_HIP_GATHER_RPB": "40"},
    "image32": {"ZIP_HIP_GATHER_STREAM": "0", "ZIP_HIP_GATHER_RPB": "32"},
    "image64": {"ZIP_HIP_GATHER_STREAM": "0", "ZIP_HIP_GATHER_RPB": "64"},
}
# 1, W - 1, W, W + 1, 2 W + 3 (8 does not divide them: the table is the sorted list), 8 | n (an eighth of the sorted
# list per XCD: 1, 6 and 125 entries each), and the protocol's count
COUNTS = [1, WALK - 1, WALK, WALK + 1, 2 * WALK + 3, 8, 48, 1000]
PATHS = ["commit_open", "hinted"]
_CASES = ([(g, "none", n) for g in "BC" for n in COUNTS]
          + [(g, "rpb64", n) for g in "BC" for n in (WALK + 1, 48, 1000)]
          + [("C", "rpb40", 2 * WALK + 3), ("C", "rpb40", 48)]
          + [("D", "image32", n) for n in (2 * WALK + 3, 1000)]
          + [("D", "image64", n) for n in (13, 1000)])  # scalar<2, 14>: D's one chunk of 64 rows as one block per opening


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    from zinc_amd import cabi

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, torch


def _columns(cw, n):
    """n columns in no order: the codeword's ends, a column three times (twice for n = 4), both neighbours of a pair and
    the pair's own neighbours in the next line, the rest pseudo-random (so some share upper tree nodes, some do not)"""
    fixed = [cw - 1, 5, 0, 5, 6, 7, 5, 8, 9, cw - 2]
    rnd = (orc.splitmix64(0xC01 + n, max(n, 1)).astype(np.uint64) % np.uint64(cw)).astype(np.uint32)
    cols = np.concatenate([np.array(fixed[:n], dtype=np.uint32), rnd[: max(0, n - len(fixed))]])
    assert cols.size == n and int(cols.max()) < cw
    return cols


@functools.lru_cache(maxsize=None)
def _oracle_commit(gid):
    nv, geo = GEOS[gid]
    z = orc.Zip(nv, geometry=geo)
    f = orc.make_field(BENCH_MODULUS, 4)
    n = 1 << nv
    evals = orc.splitmix64(0x5A494E43 + 97 + ord(gid), n).copy()
    evals[:4] = np.array([-(2**63), 2**63 - 1, -1, 0], dtype=np.int64)
    rows, layers, roots = z.commit(evals)
    coeffs = orc.splitmix64(1234 + ord(gid), z.num_rows).copy()
    coeffs[:2] = [-(2**63), 2**63 - 1]
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, orc.point_to_field(f, np.arange(3, lr + 3, dtype=np.int64)))
    rc, u = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    row = z.combine_rows_field(f, q0, evals)
    o = SimpleNamespace(z=z, evals=evals, rows=rows, layers=layers, roots=roots, coeffs=coeffs, q0=q0,
                        u=np.ascontiguousarray(u.astype("<u8")).view(np.uint8).reshape(-1),
                        row=np.ascontiguousarray(row[:, ::-1].astype(">u8")).view(np.uint8).reshape(-1))
    for a in (evals, rows, layers, roots, coeffs, q0, o.u, o.row):
        a.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _oracle_openings(gid, n):
    o = _oracle_commit(gid)
    cols = _columns(o.z.codeword_len, n)
    openings = _expected_openings(o.z, o.rows, o.layers, cols)
    cols.setflags(write=False)
    openings.setflags(write=False)
    return cols, openings


def _assert_same_bytes(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("gid,knob,n", _CASES, ids=[f"{g}-{k}-{n}" for g, k, n in _CASES])
def test_scalar_gather_writes_the_oracles_openings(env, monkeypatch, gid, knob, n, path):
    cabi, torch = env
    o = _oracle_commit(gid)
    cols, openings = _oracle_openings(gid, n)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    z = o.z
    ctx = cabi.ZipContext(z.num_vars, z.perm1, z.perm2, geometry_override=(z.row_len, z.num_rows, z.codeword_len))  # (reads the knobs)
    ctx.set_speculation(False)
    d_evals = torch.from_numpy(o.evals.copy()).cuda()  # (the cached witness stays read-only)
    out = torch.full((ctx.proof_len(n, 4),), 0xAA, dtype=torch.uint8, device="cuda")  # a byte nobody wrote shows
    torch.cuda.synchronize()  # the fill runs on torch's stream, the library on its own
    if path == "commit_open":
        _, roots, _ = ctx.commit_open(d_evals, o.coeffs, cols, o.q0, zf, out=out)
    else:
        com, roots = ctx.commit(d_evals, hint_cols=cols)
        com.open(d_evals, o.coeffs, cols, o.q0, zf, out=out)
        com.free()
    ctx.synchronize()
    got = out.cpu().numpy()
    ctx.close()
    what = f"{gid} {knob} {n} columns {path}"
    assert np.array_equal(roots, o.roots)
    assert got.size == o.u.size + openings.size + o.row.size
    _assert_same_bytes(got[: o.u.size], o.u, what + ": u'")
    _assert_same_bytes(got[o.u.size: o.u.size + openings.size], openings, what + ": openings")
    _assert_same_bytes(got[o.u.size + openings.size:], o.row, what + ": evaluation row")
