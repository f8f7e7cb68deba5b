#!/usr/bin/env python3
"""ZincProver::spartan_prove_batch against the loop over spartan_prove of the SAME build (ZIP_HIP_BATCH=0: the
one-at-a-time code, unchanged), per instance count B: B proofs of one circuit with t = 3 matrices of two entries per
row, every proof with its own z, its own (distinct) 4-limb modulus and its own transcript.  The batch leg runs with
ZIP_HIP_SPARTAN_MIN_BATCH=2, so it is the batch from two instances on whatever the mirror's own line says (B = 1 is the
loop in both legs).  Reported separately: the table calls alone -- zip_ccs_batch_create / set_z / eq_tables /
second_tables / free against zip_ccs_create / set_z / eq_table / second_table / free per instance.  Host clocks around
calls that end in a device synchronise, the legs alternating after one warm-up of each; the warm-up also compares the
two legs' proofs.  GPU box.

usage: spartan_batch_times.py [--reps N] [--sizes 10,12,14,16] [--counts 1,2,16,256] [--md FILE]"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="10,12,14,16")
ap.add_argument("--counts", default="1,2,16,256")
ap.add_argument("--md", default=None, help="write the table as markdown to this file")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zinc_amd import cabi, pcs  # noqa: E402

BASE, FL = 106319353542452952636349991594949358997917625194731877894581586278529202198383, 4
S, COEFFS, D = [[0, 1], [2]], [1, -1], 2


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
    def __init__(self, s, B):
        self.s, self.B, self.mats = s, B, circuit(s)
        rng = np.random.default_rng(s * 1000 + B)
        self.z = rng.integers(-(1 << 40), 1 << 40, size=(B, 1 << s), dtype=np.int64)
        self.z[:, 1] = 1
        self.moduli = [BASE - 2 * i for i in range(B)]  # odd and distinct: every proof pays for its own field
        self.fields = [pcs.FieldConfig(q, FL) for q in self.moduli]
        self.abi_fields = [cabi.make_field(q, FL) for q in self.moduli]
        self.prover = pcs.ZincProver()
        r = np.random.default_rng(7).integers(0, 1 << 62, size=(B, s + 1, FL), dtype=np.uint64)
        r[..., FL - 1] >>= np.uint64(6)  # canonical residues of every modulus above
        self.r, self.gamma = np.ascontiguousarray(r[:, :s]), np.ascontiguousarray(r[:, s])

    def prove(self, batched):
        os.environ["ZIP_HIP_BATCH"] = "1" if batched else "0"
        ts = []
        for i in range(self.B):
            t = pcs.KeccakTranscript()
            t.absorb(bytes([i & 255, i >> 8]))
            ts.append(t)
        xs, ws = [self.z[i, :1] for i in range(self.B)], [self.z[i, 2:] for i in range(self.B)]
        t0 = time.perf_counter()
        out = self.prover.spartan_prove_batch(self.mats, self.s, D, S, COEFFS, xs, ws, ts, self.fields)
        return time.perf_counter() - t0, out

    def tables(self, batched):
        t0 = time.perf_counter()
        if batched:
            b = cabi.CcsBatch(self.mats, self.s, FL, self.B)
            b.set_z(self.abi_fields, list(self.z))
            b.eq_tables(self.r, 0)
            vs = b.second_tables(self.r, self.gamma)
            b.free()
        else:
            vs = []
            for i in range(self.B):
                c = cabi.Ccs(self.mats, self.s, self.abi_fields[i])
                c.set_z(self.z[i])
                c.eq_table(self.r[i], 0)
                vs.append(c.second_table(self.r[i], self.gamma[i]))
                c.free()
        return time.perf_counter() - t0, np.asarray(vs)


def main():
    os.environ["ZIP_HIP_SPARTAN_MIN_BATCH"] = "2"
    head = ("| rows | B | loop ms median (min .. max) | batch ms median (min .. max) | loop / batch | batch wins beyond the loop's spread | "
            "tables alone: loop ms | tables alone: batch ms | share of the loop |")
    print(head, flush=True)
    rows = []
    for s in [int(x) for x in args.sizes.split(",")]:
        for B in [int(x) for x in args.counts.split(",")]:
            cfg = Config(s, B)
            (_, a), (_, b) = cfg.prove(False), cfg.prove(True)  # warm-up: pool blocks, code objects -- and the legs' proofs
            for pa, pb in zip(a, b):
                assert all(np.array_equal(pa[k], pb[k]) for k in ("msgs1", "msgs2", "V_s", "r_y")), "the legs differ"
            (_, va), (_, vb) = cfg.tables(False), cfg.tables(True)
            assert np.array_equal(va, vb), "the table legs differ"
            reps = args.reps if B < 256 else max(3, args.reps // 2)
            tl, tb, ul, ub = [], [], [], []
            for _ in range(reps):  # alternating
                tl.append(1e3 * cfg.prove(False)[0])
                tb.append(1e3 * cfg.prove(True)[0])
                ul.append(1e3 * cfg.tables(False)[0])
                ub.append(1e3 * cfg.tables(True)[0])
            ml, mb = statistics.median(tl), statistics.median(tb)
            wins = ml - mb > max(tl) - min(tl)
            row = (f"| 2^{s} | {B} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {mb:.3f} ({min(tb):.3f} .. {max(tb):.3f}) | "
                   f"{ml / mb:.2f} | {'yes' if wins else 'no'} | {statistics.median(ul):.3f} | {statistics.median(ub):.3f} | "
                   f"{statistics.median(ul) / ml:.0%} |")
            print(row, flush=True)
            rows.append(row)
            if args.md:
                with open(args.md, "w") as fh:
                    fh.write(head + "\n" + "|---" * 9 + "|\n" + "\n".join(rows) + "\n")
            del cfg
    print("zip_ccs_batch counters (kernel launches, instances):", cabi.ccs_batch_counts(), flush=True)


if __name__ == "__main__":
    main()
