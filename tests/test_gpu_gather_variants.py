"""The column gather's kernel instances and the commit kernel's chunk schedules, on shapes small enough for the suite:
every variant bit-exact against the CPU oracle (there are no tolerances here).  Needs a real MI355X.

run_open_columns (zip_hip.hip) picks one of eight kernel instances from the geometry, from whether a block is 32 * P
whole rows, and from knobs that zip_ctx_create reads (so a test sets them with monkeypatch.setenv BEFORE it makes its
context -- no child process).  All instances are launched under the one name `open_columns_kernel`: a test cannot read
the instance back, the tables below say which one each case reaches as derived from run_open_columns."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _oracle as orc
from _openings import _expected_openings

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
KNOB_NAMES = ("ZIP_HIP_GATHER_RPB", "ZIP_HIP_GATHER_STREAM", "ZIP_HIP_CHUNK_ROUNDS", "ZIP_HIP_NO_COMPACT_ROWS",
              "ZIP_HIP_CHUNKS", "ZIP_HIP_PACKED", "ZIP_HIP_CLASSES", "ZIP_HIP_FORCE_WAIT_TIMEOUT")


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    from zinc_amd import cabi

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, torch


def _witness(num_vars, seed=0):
    """(the pattern of test_gpu_parity._witness: splitmix with the i64 extremes forced in)"""
    n = 1 << num_vars
    w = orc.splitmix64(0x5A494E43 + seed, n).copy()
    w[:4] = np.array([-(2**63), 2**63 - 1, -1, 0], dtype=np.int64)
    return w


def _set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _ctx(cabi, z):
    ctx = cabi.ZipContext(z.num_vars, z.perm1, z.perm2, geometry_override=(z.row_len, z.num_rows, z.codeword_len))
    ctx.set_speculation(False)
    return ctx


def _assert_same_bytes(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}")


def _proof_sections(z, f, evals, coeffs, q0):
    """u' (write_integer: limbs little-endian) and the evaluation row (big-endian bytes of the Montgomery value), the
    sections before and behind the openings, from the oracle's row combinations"""
    rc, u = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    row = z.combine_rows_field(f, q0, evals)
    return (np.ascontiguousarray(u.astype("<u8")).view(np.uint8).reshape(-1),
            np.ascontiguousarray(row[:, ::-1].astype(">u8")).view(np.uint8).reshape(-1))


# ------------------------------------------------------------------------------------------------ 2a: the gather matrix
# Slices (row_len, rows, cw) of the real geometries; the depth is what selects the path.
#   A  depth  9: 8-entry commit kernel of 64 threads, the smallest shape with hints.  Hinted: two priority classes =
#                chunks of 32 rows (row_lo = 0, 32).  depth < 12: every ilv instance takes the general loop.
#   B  depth 12: 512 threads, two workgroups per CU.  Hinted: two classes = chunks of 64 rows.  First depth with `whole`,
#                no `has3` lanes (level wave + 12 does not exist).
#   C  depth 13: the benchmark's geometry, 1024 threads, one chunk of 64 rows.  `has3` on wave 0.
#   D  depth 14: the 16-entry kernel; it leaves 11.2 KB of LDS per CU -> 16 records -> default: no image.  `has3` on
#                waves 0 and 1.
GEOS = {"A": (14, (256, 64, 512)), "B": (18, (2048, 128, 4096)), "C": (18, (4096, 64, 8192)), "D": (19, (8192, 64, 16384))}

# Which instance each (geometry, knob, path) reaches, from run_open_columns.  `rpb` = 32 (D: 16) unless RPB is 2..128
# (then RPB & ~1); `stream` = the STREAM knob if set, else rpb < 32.  A block is `whole` when depth >= 12 and it has
# exactly 32 * P rows; everything else ("general") walks the predicated loop.
#
# PACKED handle (paths `hinted`, `commit_open`), one launch per chunk (A: 2 x 32 rows, B: 2 x 64, C / D: 1 x 64):
#   knob                 instance, rows per block          A          B / C                   D
#   none                 ilv<true,1>, 32 (D: <false,1>)    general    whole                   <false,1> whole
#   RPB=64               ilv<true,2>, 64                   general*   whole                   whole
#   STREAM=1             ilv<false,1>, 32                  general    whole                   whole
#   STREAM=1 RPB=64      ilv<false,2>, 64                  general*   whole                   whole
#   STREAM=0             ilv<true,1>, 32 (D: 16)           general    whole                   general (16-row blocks)
#   RPB=20               ilv<false,1>, 20 (20 < 32 streams)    general, ragged: 20 + 12 (A), 20 + 20 + 20 + 4
#   STREAM=0 RPB=20      ilv<true,1>, 20                       general, ragged, through the LDS image
#   RPB=2                ilv<false,1>, 32 (below 4: default)   as STREAM=1
#   STREAM=0 RPB=2       ilv<true,1>, 4                        general, one group of four rows per block
#   RPB=128              ilv<true,1>, 128                      general, the chunk's 32 / 64 rows in one block
#   RPB=96               ilv<true,1>, 96                       general
#   STREAM=1 RPB=4096    ilv<false,1>, 4096                    general, one block walks every row of the chunk
#   (* the 64-row block holds a 32-row chunk: not 32 * P rows)
# NATURAL handle (paths `plain`: one launch of all rows; `commit_open_natural`: ZIP_HIP_PACKED=0, the chunks above; and
# every path under NO_COMPACT_ROWS=1, which keeps Int<4> row entries and so switches packing off):
#   none                 open_columns_kernel<32>, 32 (B plain: the lone launch takes 96 + 32); D: stream_kernel<32>, 32
#   RPB=64               open_columns_kernel<32>, 64
#   STREAM=1 [RPB=64]    open_columns_stream_kernel<32>, 32 [64]
#   STREAM=0             open_columns_kernel<32>, 32 (D: 16)
#   RPB=20 / RPB=2       open_columns_stream_kernel<32>, 20 / 2 (rpb < 32 streams), ragged ends
#   STREAM=0 RPB=20 / 2  open_columns_kernel<32>, 20 / 2, ragged ends
#   RPB=128 / RPB=96     open_columns_kernel<32>, min(rows, 128 / 96): the value copy's limit of 128 rows per block
#   STREAM=1 RPB=4096    open_columns_stream_kernel<32>, all rows of the launch in one block
KNOBS = {
    "none": {},
    "rpb64": {"ZIP_HIP_GATHER_RPB": "64"},
    "stream": {"ZIP_HIP_GATHER_STREAM": "1"},
    "stream-rpb64": {"ZIP_HIP_GATHER_STREAM": "1", "ZIP_HIP_GATHER_RPB": "64"},
    "nostream": {"ZIP_HIP_GATHER_STREAM": "0"},
    "rpb20": {"ZIP_HIP_GATHER_RPB": "20"},
    "nostream-rpb20": {"ZIP_HIP_GATHER_STREAM": "0", "ZIP_HIP_GATHER_RPB": "20"},
    "rpb2": {"ZIP_HIP_GATHER_RPB": "2"},
    "nostream-rpb2": {"ZIP_HIP_GATHER_STREAM": "0", "ZIP_HIP_GATHER_RPB": "2"},
    "rpb128": {"ZIP_HIP_GATHER_RPB": "128"},
    "rpb96": {"ZIP_HIP_GATHER_RPB": "96"},
    "stream-rpb4096": {"ZIP_HIP_GATHER_STREAM": "1", "ZIP_HIP_GATHER_RPB": "4096"},
    "nocompact": {"ZIP_HIP_NO_COMPACT_ROWS": "1"},
}
_SHORT = ["none", "rpb64", "stream", "stream-rpb64", "nostream", "rpb20", "nostream-rpb20"]
PATHS = ["plain", "hinted", "commit_open", "commit_open_natural"]
_MATRIX = [(g, k, p) for g in "ABCD" for k in (KNOBS if g in "BC" else _SHORT) for p in PATHS]


@functools.lru_cache(maxsize=None)
def _oracle_open(gid):
    """The oracle's commit and whole proof (z.open on a fresh transcript: its 1000 columns), once per geometry."""
    nv, geo = GEOS[gid]
    z = orc.Zip(nv, geometry=geo)
    f = orc.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv, seed=41 + ord(gid))
    point = orc.point_to_field(f, np.arange(-5, nv - 5, dtype=np.int64))
    rows, layers, roots = z.commit(evals)
    proof, cols, coeffs = z.open(f, evals, rows, layers, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    o = SimpleNamespace(z=z, evals=evals, rows=rows, layers=layers, roots=roots, proof=proof, cols=cols, coeffs=coeffs,
                        q0=orc.build_eq_x_r(f, point[nv - lr:]))
    for a in (evals, rows, layers, roots, proof, cols, coeffs, o.q0):
        a.setflags(write=False)
    return o


@pytest.mark.parametrize("gid,knob,path", _MATRIX, ids=["-".join(c) for c in _MATRIX])
def test_gather_variant_writes_the_oracles_proof(env, monkeypatch, gid, knob, path):
    cabi, torch = env
    o = _oracle_open(gid)
    z = o.z
    zf = cabi.make_field(BENCH_MODULUS, 4)
    knobs = dict(KNOBS[knob])
    if path == "commit_open_natural":
        knobs["ZIP_HIP_PACKED"] = "0"
    _set_knobs(monkeypatch, knobs)
    ctx = _ctx(cabi, z)  # (reads the knobs)
    d_evals = torch.from_numpy(o.evals.copy()).cuda()  # (the cached witness stays read-only)
    out = torch.full((o.proof.size,), 0xAA, dtype=torch.uint8, device="cuda")  # a byte nobody wrote shows
    torch.cuda.synchronize()  # the fill runs on torch's stream, the library on its own
    if path == "plain":
        com, roots = ctx.commit(d_evals)
        com.open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out)
    elif path == "hinted":
        com, roots = ctx.commit(d_evals, hint_cols=o.cols)
        com.open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out)
    else:
        _, roots, com = ctx.commit_open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out, keep=True)
    ctx.synchronize()
    assert np.array_equal(roots, o.roots)
    _assert_same_bytes(out.cpu().numpy(), o.proof, f"{gid} {knob} {path}: proof")
    # the handle completes itself when asked for what went into the proof instead of into rows / layers
    rows, layers, roots2 = com.download()
    assert np.array_equal(roots2, o.roots)
    assert np.array_equal(rows, o.rows)
    assert np.array_equal(layers, o.layers[:, : 2 * z.codeword_len - 2])
    com.free()
    ctx.close()


# -------------------------------------------------------------------------- 2b: codewords 32768 / 65536, 32-row slices
# The slab commit kernel stores everything (no hints, no packing): natural layout on every path.
#   none        open_columns_kernel<32> at depth 15 (2 * 15 + 1 = 31 lanes per row), <64> at depth 16
#   STREAM=1    open_columns_stream_kernel<64> at both depths (2 * depth + 3 > 32)
LARGE = {"cw32768": (19, (16384, 32, 32768)), "cw65536": (20, (32768, 32, 65536))}


def _spread_cols(cw, n):
    """n hand-made columns: 0, cw - 1, a duplicate, a sibling pair, the rest spread over the codeword"""
    cols = [0, cw - 1, 5, 5, 6, 7] + [(cw // (n - 5)) * k + (37 * k) % 29 for k in range(1, n - 5)]
    assert len(cols) == n and max(cols) < cw
    return np.array(cols, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle_sections(key, n_cols, seed):
    """The oracle's commit of a geometry of LARGE / SCHED and the three sections of the proof of hand-made columns."""
    nv, geo = (LARGE.get(key) or SCHED[key])
    z = orc.Zip(nv, geometry=geo, seeds=(nv, nv + 100))
    f = orc.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv, seed=seed)
    rows, layers, roots = z.commit(evals)
    cols = _spread_cols(z.codeword_len, n_cols)
    coeffs = orc.splitmix64(seed + 5, z.num_rows).copy()
    coeffs[:2] = [-(2**63), 2**63 - 1]
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, orc.point_to_field(f, np.arange(3, lr + 3, dtype=np.int64)))
    u, row = _proof_sections(z, f, evals, coeffs, q0)
    openings = _expected_openings(z, rows, layers, cols)
    del rows, layers
    o = SimpleNamespace(z=z, evals=evals, roots=roots, cols=cols, coeffs=coeffs, q0=q0, u=u, row=row, openings=openings)
    for a in (evals, roots, cols, coeffs, q0, u, row, openings):
        a.setflags(write=False)
    return o


def _assert_sections(got, o, what):
    assert got.size == o.u.size + o.openings.size + o.row.size
    _assert_same_bytes(got[: o.u.size], o.u, what + ": u'")
    _assert_same_bytes(got[o.u.size: o.u.size + o.openings.size], o.openings, what + ": openings")
    _assert_same_bytes(got[o.u.size + o.openings.size:], o.row, what + ": evaluation row")


@pytest.mark.parametrize("path", ["plain", "commit_open"])
@pytest.mark.parametrize("knob", ["none", "stream"])
@pytest.mark.parametrize("key", sorted(LARGE))
def test_large_codeword_gather_variants(env, monkeypatch, key, knob, path):
    cabi, torch = env
    o = _oracle_sections(key, 16, 61)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    _set_knobs(monkeypatch, KNOBS[knob])
    ctx = _ctx(cabi, o.z)
    d_evals = torch.from_numpy(o.evals.copy()).cuda()  # (the cached witness stays read-only)
    out = torch.full((ctx.proof_len(o.cols.size, 4),), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if path == "plain":
        com, roots = ctx.commit(d_evals)
        com.open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out)
        com.free()
    else:
        _, roots, _ = ctx.commit_open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out)
    ctx.synchronize()
    assert np.array_equal(roots, o.roots)
    _assert_sections(out.cpu().numpy(), o, f"{key} {knob} {path}")
    ctx.close()


# --------------------------------------------------- 2c: chunk schedules, where the commit needs more than one round
#   E  8192 rows of the one-wave 8-entry kernel (8 resident per CU): 4 rounds on 256 CUs
#   F  1024 rows of the 512-thread kernel (2 per CU): 2 rounds; `whole` gathers across a chunk boundary
#   H  512 rows of the 16-entry kernel (1 per CU): 2 rounds
SCHED = {"E": (21, (256, 8192, 512)), "F": (21, (2048, 1024, 4096)), "H": (22, (8192, 512, 16384))}
SCHEDULES = {
    "none": {},
    "rounds-1,1,1,1": {"ZIP_HIP_CHUNK_ROUNDS": "1,1,1,1"},  # single-round chunks, consecutive chunk ends
    "rounds-3,1": {"ZIP_HIP_CHUNK_ROUNDS": "3,1"},
    "rounds-1,3": {"ZIP_HIP_CHUNK_ROUNDS": "1,3"},
    "rounds-2,2": {"ZIP_HIP_CHUNK_ROUNDS": "2,2"},
    "rounds-4": {"ZIP_HIP_CHUNK_ROUNDS": "4"},
    "rounds-5,4,3,2,1,1": {"ZIP_HIP_CHUNK_ROUNDS": "5,4,3,2,1,1"},  # cut to the rounds there are
    "rounds-1,1": {"ZIP_HIP_CHUNK_ROUNDS": "1,1"},
    "chunks-1": {"ZIP_HIP_CHUNKS": "1"},
    "chunks-3": {"ZIP_HIP_CHUNKS": "3"},
    "chunks-4": {"ZIP_HIP_CHUNKS": "4"},
}
_E_SCHEDULES = ["none", "rounds-1,1,1,1", "rounds-3,1", "rounds-1,3", "rounds-2,2", "rounds-4", "rounds-5,4,3,2,1,1",
                "chunks-1", "chunks-3", "chunks-4"]
_SCHED_CASES = [("E", s) for s in _E_SCHEDULES] + [(g, s) for g in "FH" for s in ("none", "rounds-1,1", "chunks-1")]


def _commit_rounds(torch, geo):
    """Rounds of the persistent commit kernel: rows / (CUs x resident workgroups per CU) -- commit_geom and
    commit_wgs_per_cu of zip_hip.hip (threads and LDS of the 8-entry and the 16-entry kernel)."""
    row_len, rows, cw = geo
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cw == 16384:
        threads, lds = 1024, 512 + 16 * 1026 * 8 + 16 * 1026 + 1024 * 4 + 64
    else:
        assert 512 <= cw < 16384
        threads = cw // 8
        lds = 512 + 8 * (threads + 4) * 12 + row_len * 8 + 64
    per_cu = max(1, min(2048 // threads, (160 * 1024) // lds, 8))
    resident = min(cus * per_cu, rows)
    return -(-rows // resident)


def _expected_chunks(rounds, knobs):
    """Chunks of the schedule commit_impl makes of `rounds` rounds under these knobs."""
    n = int(knobs.get("ZIP_HIP_CHUNKS", 0))
    sched = []
    if not n and "ZIP_HIP_CHUNK_ROUNDS" in knobs and rounds <= 64:
        used = 0
        for v in (int(t) for t in knobs["ZIP_HIP_CHUNK_ROUNDS"].split(",")):
            if used < rounds and v >= 1:
                sched.append(min(v, rounds - used))
                used += sched[-1]
    if sched:
        return len(sched)
    if not n and rounds >= 12 and rounds <= 64:  # (the default from 12 rounds up: not reached on a whole MI355X)
        return min(16, rounds // 2) if rounds >= 24 else min(8, rounds // 3)
    nch = min(n or (min(8, rounds // 4) if rounds >= 8 else 2 if rounds >= 2 else 1), rounds)
    per = -(-rounds // nch)
    return -(-rounds // per)


def test_expected_chunks_rule():
    """(the test's own restatement of commit_impl's schedule, pinned at 4 and 2 rounds: what E and F / H take on 256 CUs)"""
    want4 = {"none": 2, "rounds-1,1,1,1": 4, "rounds-3,1": 2, "rounds-1,3": 2, "rounds-2,2": 2, "rounds-4": 1,
             "rounds-5,4,3,2,1,1": 1, "chunks-1": 1, "chunks-3": 2, "chunks-4": 4}
    for s, n in want4.items():
        assert _expected_chunks(4, SCHEDULES[s]) == n, s
    for s, n in {"none": 2, "rounds-1,1": 2, "chunks-1": 1}.items():
        assert _expected_chunks(2, SCHEDULES[s]) == n, s


def _run_sched_path(cabi, torch, o, path, profile=False):
    """-> (proof bytes, roots, profile): the open is enqueued behind the still running commit of a DEVICE witness
    (no roots are asked of the commit call: delivering them would wait for it)"""
    zf = cabi.make_field(BENCH_MODULUS, 4)
    ctx = _ctx(cabi, o.z)
    ctx.set_profiling(profile)
    d_evals = torch.from_numpy(o.evals.copy()).cuda()  # (the cached witness stays read-only)
    out = torch.full((ctx.proof_len(o.cols.size, 4),), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if path == "commit_open":
        _, roots, _ = ctx.commit_open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out)
    else:
        com, _ = ctx.commit(d_evals, want_roots=False, hint_cols=o.cols if path == "hinted" else None)
        com.open(d_evals, o.coeffs, o.cols, o.q0, zf, out=out)
        roots = com.download(rows=False, layers=False)[2]
        com.free()
    ctx.synchronize()
    prof = ctx.profile_read() if profile else None
    got = out.cpu().numpy()
    ctx.close()
    return got, roots, prof


@functools.lru_cache(maxsize=None)
def _default_knob_proof(gid):
    """The proof a default-knob context writes (plain commit + open), once per geometry; the caller has cleared the knobs."""
    import torch
    from zinc_amd import cabi

    assert not any(k in os.environ for k in KNOB_NAMES)
    got, roots, _ = _run_sched_path(cabi, torch, _oracle_sections(gid, 24, 71), "plain")
    got.setflags(write=False)
    return got, roots


@pytest.mark.parametrize("gid", sorted(SCHED))
def test_default_schedule_proof_equals_oracle(env, monkeypatch, gid):
    _set_knobs(monkeypatch, {})
    o = _oracle_sections(gid, 24, 71)
    got, roots = _default_knob_proof(gid)
    assert np.array_equal(roots, o.roots)
    _assert_sections(got, o, f"{gid} default")


@pytest.mark.parametrize("path", ["plain", "hinted", "commit_open"])
@pytest.mark.parametrize("gid,sched", _SCHED_CASES, ids=["-".join(c) for c in _SCHED_CASES])
def test_chunk_schedule_writes_the_same_proof(env, monkeypatch, gid, sched, path):
    cabi, torch = env
    o = _oracle_sections(gid, 24, 71)
    _set_knobs(monkeypatch, {})
    ref, _ = _default_knob_proof(gid)
    _set_knobs(monkeypatch, SCHEDULES[sched])
    got, roots, _ = _run_sched_path(cabi, torch, o, path)
    assert np.array_equal(roots, o.roots)
    u = o.u.size
    _assert_same_bytes(got[u: u + o.openings.size], o.openings, f"{gid} {sched} {path}: openings")
    _assert_same_bytes(got, ref, f"{gid} {sched} {path}: proof against the default schedule's")


@pytest.mark.parametrize("path", ["plain", "hinted", "commit_open"])
@pytest.mark.parametrize("gid,sched", _SCHED_CASES, ids=["-".join(c) for c in _SCHED_CASES])
def test_chunk_schedule_takes_effect(env, monkeypatch, gid, sched, path):
    """The knob took effect: one gather launch per chunk of the schedule, each behind one wait on the chunk's arrival
    counter.  (Profiled, so on its own: the events between the kernels sit on the overlap the other tests exercise.)
    A plain commit of ONE chunk has no counters -- its open waits for the whole commit through an event, no wait kernel;
    a hinted one (rows >= CUs) publishes its single chunk through a counter too."""
    cabi, torch = env
    o = _oracle_sections(gid, 24, 71)
    _set_knobs(monkeypatch, SCHEDULES[sched])
    chunks = _expected_chunks(_commit_rounds(torch, SCHED[gid][1]), SCHEDULES[sched])
    got, _, prof = _run_sched_path(cabi, torch, o, path, profile=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counters = chunks > 1 or (path != "plain" and o.z.num_rows >= cus)
    assert prof["open_columns_kernel"][0] == chunks, prof
    assert prof.get("wait_counter_kernel", (0, 0.0))[0] == (chunks if counters else 0), prof
    u = o.u.size
    _assert_same_bytes(got[u: u + o.openings.size], o.openings, f"{gid} {sched} {path}: openings")
