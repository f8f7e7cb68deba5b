#!/usr/bin/env python3
"""The PCS step of ZincProver::prove_batch: pcs_step_batch (one zip_batch_commit_codes, one zip_batch_open_eval_fields,
one zip_batch_open_each for all proofs: every stream straight into its ZipProof) against the loop over pcs_step of the
SAME build (ZIP_HIP_BATCH=0: per proof a context for its code, a commit, an evaluation, an open -- code this family does
not touch), per instance count B: B proofs of one circuit of t = 3 matrices, every proof with its own z, its own
(distinct) 4-limb modulus and its own transcript, hence its own RAA code.  The batch leg runs with
ZIP_HIP_PCS_MIN_BATCH=2, so it is the batch from two instances on whatever the mirror's own line says (B = 1 is the loop
in both legs).  Timed twice: the PCS step alone, on the points and transcripts an untimed spartan_prove_batch left
(every repetition starts from copies of those transcripts), and the whole prove_batch, which says what share of a batch
proof the PCS step is.  Host clocks around calls that end in a device synchronise; the legs alternate after one warm-up
of each, and the warm-up also compares the two legs' proofs.

A third leg runs in the same process, alternated like the other two: the open of such a batch alone, through the C ABI,
in the two deliveries -- zip_batch_open_fields into ONE host block of B streams that is then cut into B buffers, and
zip_batch_open_each into B buffers of their own, sized first.  The first is a PROXY in numpy (fill, open, one copy per
member) for what the mirror's step 5 did before it delivered per member (resize, open, assign); that C++ code is gone
and is not what runs here.  Same batch, same challenges, fresh destinations on every repetition as the mirror's are; the
two agree byte for byte.  --windows 16,64,256 times zip_batch_open_each at those window_bytes (MiB) as well, and --laps
prints the mirror's stage laps (ZINC_HOST_TIMING=1) of one batched step.

Every (rows, B) cell runs in a process of its own under its own time limit; after a cell that fails or runs out of time
nothing further is started.  GPU box.

usage: pcs_batch_times.py [--reps N] [--sizes 10,12,14,16] [--counts 1,2,16,256] [--md FILE] [--limit SECONDS]
                          [--windows 16,64,256] [--laps]"""
import argparse
import os
import statistics
import subprocess
import sys
import time
import types

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="10,12,14,16")
ap.add_argument("--counts", default="1,2,16,256")
ap.add_argument("--md", default=None, help="write the table as markdown to this file")
ap.add_argument("--limit", type=int, default=240, help="seconds one (rows, B) cell may take")
ap.add_argument("--windows", default="", help="MiB: time zip_batch_open_each at these window_bytes too (B >= 2)")
ap.add_argument("--laps", action="store_true", help="print the stage laps of one batched step per cell (B >= 2)")
ap.add_argument("--cell", default=None, help="(internal) s,B: measure this one cell and print its row")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE, FL = 106319353542452952636349991594949358997917625194731877894581586278529202198383, 4
S, COEFFS, D = [[0, 1], [2]], [1, -1], 2
HEAD = ("| rows | B | PCS loop ms median (min .. max) | PCS batch ms median (min .. max) | loop / batch | batch wins beyond the loop's spread | "
        "prove_batch, PCS looped: ms | prove_batch, PCS batched: ms | PCS share before | PCS share after | "
        "open alone, one block + cut: ms | open alone, per member: ms | block / per member | stream bytes x B |")


def circuit(s):
    """three matrices, two entries per row: the diagonal and a second column that differs per matrix"""
    m = 1 << s
    rows = np.arange(m, dtype=np.uint32)
    mats = []
    for k, (a, b) in enumerate(((1, 5), (-1, 1), (1, -1))):
        other = (rows * np.uint32(2 * k + 3) + np.uint32(k + 1)) % np.uint32(m)
        other = np.where(other == rows, (rows + 1) % m, other).astype(np.uint32)
        cols = np.stack([rows, other], axis=1)
        vals = np.tile(np.array([a, b], dtype=np.int64), (m, 1))
        order = np.argsort(cols, axis=1)
        mats.append(types.SimpleNamespace(n_rows=m, n_cols=m, row_ptr=np.arange(0, 2 * m + 1, 2, dtype=np.uint32),
                                          col_idx=np.take_along_axis(cols, order, 1).reshape(-1).copy(),
                                          values=np.take_along_axis(vals, order, 1).reshape(-1).copy()))
    return mats


class Config:
    def __init__(self, pcs, s, B):
        self.pcs, self.s, self.B, self.mats = pcs, s, B, circuit(s)
        rng = np.random.default_rng(s * 1000 + B)
        self.z = rng.integers(-(1 << 40), 1 << 40, size=(B, 1 << s), dtype=np.int64)
        self.z[:, 1] = 1
        self.fields = [pcs.FieldConfig(BASE - 2 * i, FL) for i in range(B)]  # odd and distinct: every proof has its own field
        self.prover = pcs.ZincProver()
        self.xs, self.ws = [self.z[i, :1] for i in range(B)], [self.z[i, 2:] for i in range(B)]
        # the state the PCS step starts from: what the Spartan part leaves (untimed)
        ts = self.fresh()
        os.environ["ZIP_HIP_BATCH"] = "1"
        sp = self.prover.spartan_prove_batch(self.mats, s, D, S, COEFFS, self.xs, self.ws, ts, self.fields)
        self.r_y = [p["r_y"] for p in sp]
        self.after_spartan = [t.state() for t in ts]

    def fresh(self):
        ts = []
        for i in range(self.B):
            t = self.pcs.KeccakTranscript()
            t.absorb(bytes([i & 255, i >> 8]))
            ts.append(t)
        return ts

    def leg(self, batched):
        os.environ["ZIP_HIP_BATCH"] = "1" if batched else "0"  # ("0": the loop, in the Spartan part as well)

    def pcs_step(self, batched):
        ts = self.fresh()
        for t, st in zip(ts, self.after_spartan):
            t.set_state(st)
        self.leg(batched)
        t0 = time.perf_counter()
        out = self.prover.pcs_step_batch(self.s, list(self.z), self.r_y, ts, self.fields)
        return time.perf_counter() - t0, out

    def prove(self, pcs_batched):
        """the whole prove_batch, the Spartan part batched in both legs: only the PCS step differs"""
        ts = self.fresh()
        os.environ["ZIP_HIP_BATCH"] = "1"
        os.environ["ZIP_HIP_PCS_MIN_BATCH"] = "2" if pcs_batched else str(1 << 30)
        t0 = time.perf_counter()
        out = self.prover.prove_batch(self.mats, self.s, D, S, COEFFS, self.xs, self.ws, ts, self.fields)
        dt = time.perf_counter() - t0
        os.environ["ZIP_HIP_PCS_MIN_BATCH"] = "2"
        return dt, [p["zip_proof"] for p in out]


def same(a, b):
    return all(np.array_equal(pa[k], pb[k]) for pa, pb in zip(a, b) for k in ("z_comm", "v", "pcs_proof"))


class OpenAlone:
    """Step 5 of the batched PCS step alone, through the C ABI: B members of the geometry of 2^s rows, each with its own
    code and modulus, 1000 openings, random challenges"""

    def __init__(self, cabi, pcs, s, B):
        self.cabi, self.B = cabi, B
        rng = np.random.default_rng(77 * s + B)
        row_len, num_rows, cw = cabi.geometry(s, 2)
        perms = [np.stack([pcs.shuffle_seeded_perm(1000 * k + 2 * i + 1, cw) for i in range(B)]) for k in (1, 2)]
        self.ctx = cabi.ZipContext(s, perms[0][0], perms[1][0])
        z = rng.integers(-(1 << 40), 1 << 40, size=(B, 1 << s), dtype=np.int64)
        self.batch = self.ctx.batch_commit_codes(z, perms[0], perms[1], want_roots=False)
        self.fields = [cabi.make_field(BASE - 2 * i, FL) for i in range(B)]
        self.n_cols = 1000
        self.cols = rng.integers(0, cw, size=(B, self.n_cols), dtype=np.uint32)
        self.coeffs = rng.integers(-(1 << 62), 1 << 62, size=(B, num_rows), dtype=np.int64) if num_rows > 1 else None
        q0 = rng.integers(0, 1 << 63, size=(B, num_rows, FL), dtype=np.uint64)
        q0[:, :, FL - 1] >>= 2  # below every modulus
        self.q0 = q0 if num_rows > 1 else None
        self.len = self.ctx.proof_len(self.n_cols, FL)

    def block_and_cut(self):
        """resize (a fresh block, touched), one open into it, one fresh copy per member"""
        t0 = time.perf_counter()
        block = np.empty((self.B, self.len), dtype=np.uint8)
        block.fill(0)
        self.batch.open_fields(self.coeffs, self.cols, self.q0, self.fields, out=block)
        outs = [block[i].copy() for i in range(self.B)]
        return time.perf_counter() - t0, outs

    def per_member(self, window_bytes=0):
        """B fresh buffers, touched, one open that fills them"""
        t0 = time.perf_counter()
        outs = []
        for _ in range(self.B):
            o = np.empty(self.len, dtype=np.uint8)
            o.fill(0)
            outs.append(o)
        self.batch.open_each(self.coeffs, self.cols, self.q0, self.fields, outs=outs, window_bytes=window_bytes)
        return time.perf_counter() - t0, outs


def cell(s, B):
    from zinc_amd import cabi, pcs

    os.environ["ZIP_HIP_PCS_MIN_BATCH"] = "2"
    cfg = Config(pcs, s, B)
    before = cabi.batch_codes_counts()
    (_, a), (_, b) = cfg.pcs_step(False), cfg.pcs_step(True)  # warm-up: pool blocks, code objects -- and the legs' proofs
    assert same(a, b), "the legs differ"
    took = cabi.batch_codes_counts()
    assert (took[0] - before[0], took[2] - before[2]) == ((1, 2) if B >= 2 else (0, 0)), "the batch leg took the other path"
    assert cabi.batch_open_each_counts()[0] == (1 if B >= 2 else 0), "the batch leg delivers per member"
    (_, pa), (_, pb) = cfg.prove(False), cfg.prove(True)
    assert same(pa, pb) and same(pa, a), "prove_batch's legs differ"
    reps = args.reps if B < 256 else max(3, args.reps // 2)
    alone = OpenAlone(cabi, pcs, s, B) if B >= 2 else None
    windows = [int(x) for x in args.windows.split(",") if x] if alone else []
    if alone:  # warm-up, and the two deliveries agree
        (_, x), (_, y) = alone.block_and_cut(), alone.per_member()
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), "the two deliveries differ"
        for w in windows:
            assert all(np.array_equal(p, q) for p, q in zip(x, alone.per_member(w << 20)[1])), f"window {w} MiB differs"
        del x, y
    tl, tb, wl, wb, ob, oe = [], [], [], [], [], []
    ow = {w: [] for w in windows}
    for _ in range(reps):  # alternating
        tl.append(1e3 * cfg.pcs_step(False)[0])
        tb.append(1e3 * cfg.pcs_step(True)[0])
        wl.append(1e3 * cfg.prove(False)[0])
        wb.append(1e3 * cfg.prove(True)[0])
        if alone:
            ob.append(1e3 * alone.block_and_cut()[0])
            oe.append(1e3 * alone.per_member()[0])
            for w in windows:
                ow[w].append(1e3 * alone.per_member(w << 20)[0])
    ml, mb, mwl, mwb = statistics.median(tl), statistics.median(tb), statistics.median(wl), statistics.median(wb)
    wins = ml - mb > max(tl) - min(tl)
    print(f"ROW | 2^{s} | {B} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {mb:.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {ml / mb:.2f} | "
          f"{'yes' if wins else 'no'} | {mwl:.3f} | {mwb:.3f} | {ml / mwl:.0%} | {mb / mwb:.0%} | "
          + (f"{statistics.median(ob):.3f} ({min(ob):.3f} .. {max(ob):.3f}) | {statistics.median(oe):.3f} ({min(oe):.3f} .. {max(oe):.3f}) | "
             f"{statistics.median(ob) / statistics.median(oe):.2f} | {alone.len * B} |" if alone else "- | - | - | - |"), flush=True)
    for w in windows:
        print(f"WINDOW | 2^{s} | {B} | {w} MiB | {statistics.median(ow[w]):.3f} ({min(ow[w]):.3f} .. {max(ow[w]):.3f}) |", flush=True)
    if args.laps and B >= 2:
        os.environ["ZINC_HOST_TIMING"] = "1"
        print(f"LAPS 2^{s} x {B}: one batched pcs_step_batch, stage laps on stderr", flush=True)
        cfg.pcs_step(True)
        del os.environ["ZINC_HOST_TIMING"]


def main():
    if args.cell:
        s, B = (int(x) for x in args.cell.split(","))
        return cell(s, B)
    print(HEAD, flush=True)
    rows = []
    for s in [int(x) for x in args.sizes.split(",")]:
        for B in [int(x) for x in args.counts.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", f"{s},{B}", "--reps", str(args.reps), "--windows", args.windows]
            if args.laps:
                cmd.append("--laps")
            child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            t0, r = time.monotonic(), None
            while r is None:
                try:
                    out, err = child.communicate(timeout=min(60, max(1, args.limit - (time.monotonic() - t0))))
                    r = types.SimpleNamespace(returncode=child.returncode, stdout=out, stderr=err)
                except subprocess.TimeoutExpired:
                    if time.monotonic() - t0 < args.limit:
                        print(f"(2^{s} x {B}: {time.monotonic() - t0:.0f} s so far)", flush=True)  # a long cell is not a silent one
                        continue
                    child.kill()
                    child.communicate()
                    print(f"2^{s} x {B}: no result within {args.limit} s; nothing further is started", flush=True)
                    return 1
            row = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
            if r.returncode != 0 or not row:
                print(f"2^{s} x {B}: exit status {r.returncode}; nothing further is started\n{(r.stdout + r.stderr)[-3000:]}", flush=True)
                return 1
            print(row[0], flush=True)
            rows.append(row[0])
            for ln in r.stdout.splitlines():
                if ln.startswith("WINDOW "):
                    print(ln, flush=True)
            for ln in r.stderr.splitlines():
                if args.laps and ln.startswith("[zinc]   pcs"):
                    print(f"LAP 2^{s} x {B} {ln}", flush=True)
            if args.md:
                with open(args.md, "w") as fh:
                    fh.write(HEAD + "\n" + "|---" * 14 + "|\n" + "\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
