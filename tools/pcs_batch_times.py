#!/usr/bin/env python3
"""The PCS step of ZincProver::prove_batch: pcs_step_batch (one zip_batch_commit_codes, one zip_batch_open_eval_fields, one
zip_batch_open_fields for all proofs) against the loop over pcs_step of the SAME build (ZIP_HIP_BATCH=0: per proof a
context for its code, a commit, an evaluation, an open -- code this family does not touch), per instance count B: B
proofs of one circuit of t = 3 matrices, every proof with its own z, its own (distinct) 4-limb modulus and its own
transcript, hence its own RAA code.  The batch leg runs with ZIP_HIP_PCS_MIN_BATCH=2, so it is the batch from two
instances on whatever the mirror's own line says (B = 1 is the loop in both legs).  Timed twice: the PCS step alone, on
the points and transcripts an untimed spartan_prove_batch left (every repetition starts from copies of those
transcripts), and the whole prove_batch, which says what share of a batch proof the PCS step is.  Host clocks around
calls that end in a device synchronise; the legs alternate after one warm-up of each, and the warm-up also compares the
two legs' proofs.

Every (rows, B) cell runs in a process of its own under its own time limit; after a cell that fails or runs out of time
nothing further is started.  GPU box.

usage: pcs_batch_times.py [--reps N] [--sizes 10,12,14,16] [--counts 1,2,16,256] [--md FILE] [--limit SECONDS]"""
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
ap.add_argument("--cell", default=None, help="(internal) s,B: measure this one cell and print its row")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE, FL = 106319353542452952636349991594949358997917625194731877894581586278529202198383, 4
S, COEFFS, D = [[0, 1], [2]], [1, -1], 2
HEAD = ("| rows | B | PCS loop ms median (min .. max) | PCS batch ms median (min .. max) | loop / batch | batch wins beyond the loop's spread | "
        "prove_batch, PCS looped: ms | prove_batch, PCS batched: ms | PCS share before | PCS share after |")


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


def cell(s, B):
    from zinc_amd import cabi, pcs

    os.environ["ZIP_HIP_PCS_MIN_BATCH"] = "2"
    cfg = Config(pcs, s, B)
    before = cabi.batch_codes_counts()
    (_, a), (_, b) = cfg.pcs_step(False), cfg.pcs_step(True)  # warm-up: pool blocks, code objects -- and the legs' proofs
    assert same(a, b), "the legs differ"
    took = cabi.batch_codes_counts()
    assert (took[0] - before[0], took[2] - before[2]) == ((1, 2) if B >= 2 else (0, 0)), "the batch leg took the other path"
    (_, pa), (_, pb) = cfg.prove(False), cfg.prove(True)
    assert same(pa, pb) and same(pa, a), "prove_batch's legs differ"
    reps = args.reps if B < 256 else max(3, args.reps // 2)
    tl, tb, wl, wb = [], [], [], []
    for _ in range(reps):  # alternating
        tl.append(1e3 * cfg.pcs_step(False)[0])
        tb.append(1e3 * cfg.pcs_step(True)[0])
        wl.append(1e3 * cfg.prove(False)[0])
        wb.append(1e3 * cfg.prove(True)[0])
    ml, mb, mwl, mwb = statistics.median(tl), statistics.median(tb), statistics.median(wl), statistics.median(wb)
    wins = ml - mb > max(tl) - min(tl)
    print(f"ROW | 2^{s} | {B} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {mb:.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {ml / mb:.2f} | "
          f"{'yes' if wins else 'no'} | {mwl:.3f} | {mwb:.3f} | {ml / mwl:.0%} | {mb / mwb:.0%} |", flush=True)


def main():
    if args.cell:
        s, B = (int(x) for x in args.cell.split(","))
        return cell(s, B)
    print(HEAD, flush=True)
    rows = []
    for s in [int(x) for x in args.sizes.split(",")]:
        for B in [int(x) for x in args.counts.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", f"{s},{B}", "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"2^{s} x {B}: no result within {args.limit} s; nothing further is started", flush=True)
                return 1
            row = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
            if r.returncode != 0 or not row:
                print(f"2^{s} x {B}: exit status {r.returncode}; nothing further is started\n{(r.stdout + r.stderr)[-3000:]}", flush=True)
                return 1
            print(row[0], flush=True)
            rows.append(row[0])
            if args.md:
                with open(args.md, "w") as fh:
                    fh.write(HEAD + "\n" + "|---" * 10 + "|\n" + "\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
