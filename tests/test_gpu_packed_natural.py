"""The packed 8-entry commit kernel (raa_commit_kernel<8, true, kStorePacked>) with natural ownership: every lane hashes
the 8-leaf subtree over its own entries and places its stores by a per-lane base rank + a popcount of its own store
mask.  Bit-exact against the CPU oracle (there are no tolerances here).  Needs a real MI355X.

Which commits reach that kernel (dispatch_commit / commit_geom / get_hint_plan of zip_hip.hip): a commit that carries
an opening hint -- zip_commit_hinted, zip_commit_open -- of codeword length 512, 1024, 2048, 4096 or 8192 (cw / 8 = 64 ..
1024 threads; 16384 has the 16-entry kernel, 256 and below store everything) under the default knobs.

Rows: 1 (a lone row), 4 (one whole interleave group of the packed block and of `layers`), 5 (a straddled group).  Five
rows are no power of two: they are a row shard (rows 0..4 of 8), committed hinted and opened with zip_open_shard (its
openings are compared; the partial row combinations are not this kernel's).

The bytes in HBM are those of the strided kernel before it, by design: these tests guard parity with the oracle on the
shapes and hint lists where the rank arithmetic can go wrong, not which code path produced the bytes.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _oracle as orc
import test_gpu_gather_variants as gv
from _openings import _expected_openings

pytestmark = pytest.mark.gpu

BENCH_MODULUS = gv.BENCH_MODULUS
CWS = (512, 1024, 2048, 4096, 8192)
ROWS = (1, 4, 5)


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    from zinc_amd import cabi

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, torch


def _hint_lists(cw, bench_cols):
    """Column lists that stress the rank arithmetic (lane t owns columns 8t .. 8t+7; a wave is 512 columns)."""
    lists = {
        "one": [37],
        "pair": [100, 101],                          # c and c ^ 1: each the other's level-0 sibling
        "lane": list(range(40, 48)),                 # all eight entries of lane 5: all 22 bits of its store mask
        "wave-edges": [63, 64, 511, 512],            # lane 7 | 8 (a level-3 store's 64th column), wave 0 | 1
        "ends": [0, cw - 1],
        "mixed": [0, 1, 2, 3, 8, 9, 40, 47, 63, 64, 65, 511, 512, 513, cw // 2 - 1, cw // 2, cw - 8, cw - 2, cw - 1, 40],
        "bench": [int(c) for c in bench_cols],       # the 1000 columns a fresh transcript squeezes (bench.py's)
    }
    return {k: np.array([c for c in v if c < cw], dtype=np.uint32) for k, v in lists.items()}


@functools.lru_cache(maxsize=None)
def _oracle_case(cw, rows):
    """The oracle's commit of `rows` rows of codeword length cw (rep 2), and what the row combinations need."""
    row_len = cw // 2
    full_rows = 8 if rows == 5 else rows  # (5 rows: the first five of a polynomial of eight)
    nv = (row_len * full_rows).bit_length() - 1
    z = orc.Zip(nv, geometry=(row_len, rows, cw), seeds=(cw, cw + 100))
    f = orc.make_field(BENCH_MODULUS, 4)
    evals = gv._witness(nv, seed=7 + rows)[: rows * row_len].copy()
    rows_o, layers_o, roots_o = z.commit(evals)
    coeffs = orc.splitmix64(cw + rows, rows).copy()
    coeffs[0] = -(2**63)
    q0 = orc.build_eq_x_r(f, orc.point_to_field(f, np.arange(3, 6, dtype=np.int64)))[:rows].copy() if rows > 1 else None
    o = SimpleNamespace(z=z, f=f, nv=nv, full_rows=full_rows, evals=evals, rows=rows_o, layers=layers_o, roots=roots_o,
                        coeffs=coeffs, q0=q0)
    if rows > 1:
        o.u, o.row = gv._proof_sections(z, f, evals, coeffs, q0)
    for a in (evals, rows_o, layers_o, roots_o, coeffs):
        a.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _bench_cols(cw):
    """The columns MultilinearZip::open squeezes from a fresh transcript at this codeword length (one row suffices)."""
    o = _oracle_case(cw, 1)
    point = orc.point_to_field(o.f, np.arange(-5, o.nv - 5, dtype=np.int64))
    proof, cols, _ = o.z.open(o.f, o.evals, o.rows, o.layers, point, orc.new_transcript())
    lr_row = np.ascontiguousarray(proof[proof.size - o.z.row_len * 32:])
    cols.setflags(write=False)
    return cols, lr_row


def _check_download(com, o, what):
    """the handle completes itself from the packed blocks when asked for rows and trees: every stored member is read"""
    rows, layers, roots = com.download()
    assert np.array_equal(roots, o.roots), what
    gv._assert_same_bytes(rows.view(np.uint8).reshape(-1), np.ascontiguousarray(o.rows).view(np.uint8).reshape(-1), what + ": rows")
    gv._assert_same_bytes(layers.reshape(-1), o.layers[:, : 2 * o.z.codeword_len - 2].reshape(-1), what + ": trees")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cw", CWS)
def test_packed_commit_matches_oracle(env, monkeypatch, cw, rows):
    cabi, torch = env
    gv._set_knobs(monkeypatch, {})
    o = _oracle_case(cw, rows)
    z = o.z
    zf = cabi.make_field(BENCH_MODULUS, 4)
    bench_cols, bench_tail = _bench_cols(cw)
    ctx = cabi.ZipContext(o.nv, z.perm1, z.perm2, geometry_override=(z.row_len, o.full_rows, cw),
                          row_begin=0, row_count=rows if rows != o.full_rows else 0)
    ctx.set_speculation(False)
    d_evals = torch.from_numpy(o.evals.copy()).cuda()
    for name, cols in _hint_lists(cw, bench_cols).items():
        what = f"cw {cw}, {rows} rows, hint '{name}'"
        want = _expected_openings(z, o.rows, o.layers, cols)
        if rows == o.full_rows:  # zip_commit_open: the whole proof
            out = torch.full((ctx.proof_len(cols.size, 4),), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _, roots, com = ctx.commit_open(d_evals, o.coeffs if rows > 1 else None, cols, o.q0, zf, out=out, keep=True)
            ctx.synchronize()
            got = out.cpu().numpy()
            u = o.u.size if rows > 1 else 0
            assert got.size == u + want.size + z.row_len * 32, what
            gv._assert_same_bytes(got[u: u + want.size], want, what + ": openings")
            if rows > 1:
                gv._assert_same_bytes(got[:u], o.u, what + ": u'")
                gv._assert_same_bytes(got[u + want.size:], o.row, what + ": evaluation row")
            else:  # (one row: no u', and the evaluation row is the oracle's own open's)
                gv._assert_same_bytes(got[want.size:], bench_tail, what + ": evaluation row")
        else:  # a row shard: hinted commit, then zip_open_shard
            com, roots = ctx.commit(d_evals, hint_cols=cols)
            upart = torch.zeros((z.row_len, 8), dtype=torch.int64, device="cuda")
            fpart = torch.zeros((z.row_len, 4), dtype=torch.int64, device="cuda")
            wire = torch.full((want.size,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            com.open_shard(d_evals, o.coeffs, cols, o.q0, zf, upart, fpart, wire)
            ctx.synchronize()
            gv._assert_same_bytes(wire.cpu().numpy(), want, what + ": openings")
        assert np.array_equal(roots, o.roots), what
        _check_download(com, o, what)
        com.free()
    ctx.close()


@functools.lru_cache(maxsize=None)
def _oracle_rounds():
    """1024 rows of the benchmark's geometry (row_len 4096, cw 8192: the 1024-thread instance, one workgroup per CU):
    four rounds on 256 CUs.  Hand-made columns, as the schedule cases of test_gpu_gather_variants take them."""
    nv, geo = 22, (4096, 1024, 8192)
    z = orc.Zip(nv, geometry=geo, seeds=(nv, nv + 100))
    f = orc.make_field(BENCH_MODULUS, 4)
    evals = gv._witness(nv, seed=83)
    rows, layers, roots = z.commit(evals)
    cols = np.array([0, 8191, 5, 5, 6, 7, 63, 64, 511, 512] + list(range(40, 48)) + [331 * k + 17 for k in range(1, 24)],
                    dtype=np.uint32)
    coeffs = orc.splitmix64(88, z.num_rows).copy()
    coeffs[:2] = [-(2**63), 2**63 - 1]
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, orc.point_to_field(f, np.arange(3, lr + 3, dtype=np.int64)))
    u, row = gv._proof_sections(z, f, evals, coeffs, q0)
    openings = _expected_openings(z, rows, layers, cols)
    del rows, layers
    o = SimpleNamespace(z=z, evals=evals, roots=roots, cols=cols, coeffs=coeffs, q0=q0, u=u, row=row, openings=openings)
    for a in (evals, roots, cols, coeffs, q0, u, row, openings):
        a.setflags(write=False)
    return o


def test_packed_commit_consecutive_chunk_ends(env, monkeypatch):
    """ZIP_HIP_CHUNK_ROUNDS=1,1,1,1 on 1024 rows of the 1024-thread instance (the benchmark's; four rounds on 256 CUs):
    every round ends a chunk, so three deferred chunk ends (ChunkFinisher::after_hash) in consecutive rows and then the
    last one (after_loop) run over the row loop's three barriers.  The profile says the schedule took effect: one gather
    launch per round."""
    cabi, torch = env
    o = _oracle_rounds()
    gv._set_knobs(monkeypatch, {"ZIP_HIP_CHUNK_ROUNDS": "1,1,1,1"})
    rounds = gv._commit_rounds(torch, (o.z.row_len, o.z.num_rows, o.z.codeword_len))
    got, roots, prof = gv._run_sched_path(cabi, torch, o, "commit_open", profile=True)
    assert np.array_equal(roots, o.roots)
    gv._assert_sections(got, o, "cw 8192, rounds-1,1,1,1, commit_open")
    assert prof["open_columns_kernel"][0] == gv._expected_chunks(rounds, {"ZIP_HIP_CHUNK_ROUNDS": "1,1,1,1"}), prof
