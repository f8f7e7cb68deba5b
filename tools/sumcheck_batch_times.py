#!/usr/bin/env python3
"""zip_sumcheck_prove_batch against the loop of zip_sumcheck_init + zip_sumcheck_prove + zip_sumcheck_free of the SAME
build, per instance count B: B small sumchecks of one shape, every instance with its own tables, its own (distinct)
modulus and its own transcript.  Shapes: the product of K = 2 tables at degree 2, and the CCS combination over K = 4 at
degree 3; 3- and 4-limb fields; tables already in HBM ("device": the upload is not part of either time) and host tables
("host": both forms copy them).  Both legs are host clocks around calls that end in a device synchronise, taken in
alternating runs after one warm-up of each; the warm-up also compares the two legs' bytes.  GPU box.

At most --table-gib of distinct tables are made per configuration; beyond that instances share tables round-robin
(the batch's L2 sees repeats the loop's does not: the note in the output says when that happened).

usage: sumcheck_batch_times.py [--reps N] [--sizes 10,12,14,16] [--counts 1,16,256,1024] [--limbs 3,4]
                               [--mem device,host] [--md FILE] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="10,12,14,16")
ap.add_argument("--counts", default="1,16,256,1024")
ap.add_argument("--limbs", default="3,4")
ap.add_argument("--mem", default="device,host")
ap.add_argument("--table-gib", type=float, default=1.0)
ap.add_argument("--md", default=None, help="write the table as markdown to this file")
ap.add_argument("--json", default=None, help="append one JSON line per measurement to this file")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from zinc_amd import cabi  # noqa: E402

BASE = {3: (1 << 190) - 11 * (1 << 64) - 59, 4: 106319353542452952636349991594949358997917625194731877894581586278529202198383}
SHAPES = {"product K=2 d=2": (2, 2, False), "ccs K=4 d=3": (4, 3, True)}


class Config:
    def __init__(self, K, degree, ccs, fl, nv, B, mem):
        self.K, self.degree, self.fl, self.nv, self.B, self.mem = K, degree, fl, nv, B, mem
        per_set = K * (1 << nv) * fl * 8
        self.n_sets = max(1, min(B, int(args.table_gib * (1 << 30)) // per_set))
        rng = np.random.default_rng(nv * 100 + K)
        self.host = rng.integers(0, 1 << 62, size=(self.n_sets, K, 1 << nv, fl), dtype=np.uint64)
        self.host[..., fl - 1] >>= np.uint64(6 if fl == 4 else 4)  # canonical residues of every modulus below
        if mem == "device":
            self.dev = torch.from_numpy(self.host.view(np.int64)).cuda()
            torch.cuda.synchronize()
            base, step = self.dev.data_ptr(), (1 << nv) * fl * 8
            addr = lambda s, k: base + (s * K + k) * step  # noqa: E731
            self.kind = cabi.MEM_DEVICE
        else:
            addr = lambda s, k: self.host[s, k].ctypes.data  # noqa: E731
            self.kind = cabi.MEM_HOST
        self.ptrs = [(C.c_void_p * K)(*[addr(i % self.n_sets, k) for k in range(K)]) for i in range(B)]
        moduli = [BASE[fl] - 2 * i for i in range(B)]  # odd and distinct: every instance pays for its own field
        self.fields = [cabi.make_field(q, fl) for q in moduli]
        R = 1 << (64 * fl)
        lim = lambda v: [(v >> (64 * j)) & (2**64 - 1) for j in range(fl)]  # noqa: E731
        self.combs = [cabi.make_comb([0b011, 0b100], [lim(R % q), lim((q - 1) * R % q)]) if ccs else None for q in moduli]
        self.msgs = np.zeros((2, B, nv, degree + 1, fl), np.uint64)
        self.rand = np.zeros((2, B, nv, fl), np.uint64)
        self.states = None
        self.arr = (cabi.SumcheckInstance * B)()

    def reset(self):
        self.states = [cabi.KeccakState.make(buf=bytes([i & 255, i >> 8])) for i in range(self.B)]
        for i in range(self.B):
            self.arr[i].mles = C.cast(self.ptrs[i], C.c_void_p)
            self.arr[i].comb = C.pointer(self.combs[i]) if self.combs[i] is not None else None
            self.arr[i].field = C.pointer(self.fields[i])
            self.arr[i].transcript = C.pointer(self.states[i])

    def loop(self):
        L, m, r = cabi.lib(), self.msgs[0], self.rand[0]
        self.reset()
        t0 = time.perf_counter()
        for i in range(self.B):
            h = C.c_void_p()
            rc = L.zip_sumcheck_init(0, self.ptrs[i], self.kind, self.K, self.nv, self.degree,
                                     C.byref(self.combs[i]) if self.combs[i] is not None else None, C.byref(self.fields[i]), C.byref(h))
            assert rc == 0, rc
            rc = L.zip_sumcheck_prove(h, C.byref(self.states[i]), m[i].ctypes.data, r[i].ctypes.data)
            assert rc == 0, rc
            L.zip_sumcheck_free(h)
        return time.perf_counter() - t0

    def batch(self):
        L = cabi.lib()
        self.reset()
        t0 = time.perf_counter()
        rc = L.zip_sumcheck_prove_batch(0, self.arr, self.B, self.kind, self.K, self.nv, self.degree, self.msgs[1].ctypes.data,
                                        self.rand[1].ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt


def main():
    rows = []
    head = ("| shape | limbs | num_vars | B | tables | loop ms median (min .. max) | batch ms median (min .. max) | loop / batch | "
            "batch us per instance | batch wins beyond the loop's spread |")
    print(head, flush=True)
    for name, (K, degree, ccs) in SHAPES.items():
        for fl in [int(x) for x in args.limbs.split(",")]:
            for nv in [int(x) for x in args.sizes.split(",")]:
                for mem in args.mem.split(","):
                    for B in [int(x) for x in args.counts.split(",")]:
                        cfg = Config(K, degree, ccs, fl, nv, B, mem)
                        cfg.loop()  # warm-up: pool blocks, code objects -- and the bytes of the two legs
                        cfg.batch()
                        assert np.array_equal(cfg.msgs[0], cfg.msgs[1]) and np.array_equal(cfg.rand[0], cfg.rand[1]), "the legs differ"
                        reps = args.reps if B < 1024 else max(3, args.reps // 2)
                        tl, tb = [], []
                        for _ in range(reps):  # alternating
                            tl.append(1e3 * cfg.loop())
                            tb.append(1e3 * cfg.batch())
                        ml, mb = statistics.median(tl), statistics.median(tb)
                        wins = ml - mb > max(tl) - min(tl)
                        shared = "" if cfg.n_sets == B else f" ({cfg.n_sets} table sets shared)"
                        row = (f"| {name} | {fl} | {nv} | {B} | {mem}{shared} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | "
                               f"{mb:.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {ml / mb:.2f} | {1e3 * mb / B:.1f} | {'yes' if wins else 'no'} |")
                        print(row, flush=True)
                        rows.append(row)
                        if args.json:
                            with open(args.json, "a") as fh:
                                fh.write(json.dumps(dict(shape=name, limbs=fl, nv=nv, B=B, mem=mem, loop_ms=tl, batch_ms=tb,
                                                         table_sets=cfg.n_sets)) + "\n")
                        if args.md:
                            with open(args.md, "w") as fh:
                                fh.write(head + "\n" + "|---" * 10 + "|\n" + "\n".join(rows) + "\n")
                        del cfg
    print("batch counters (launches, instances, streamed rounds):", cabi.sumcheck_batch_counts(), flush=True)


if __name__ == "__main__":
    main()
