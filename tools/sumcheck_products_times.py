#!/usr/bin/env python3
"""Sum-of-products sumcheck (the reference's bench shape: rand_poly, 7 products of 2..4 multiplicands over 21 MLEs,
3-limb prime 1 of the benchmark) at 2^20 and 2^12: one zip_sumcheck_init_products handle ("fused") against the loop of
one handle per product ("loop"), with DEVICE-resident tables (the upload is not part of the time; challenges are fixed
in advance, so neither form pays for a transcript) and with HOST tables through the host mirror (upload and transcript
included, ZIP_HIP_SUMCHECK_FUSED=0 / 1).  Per-round times for the large rounds.  GPU box.

usage: sumcheck_products_times.py [--tree DIR] [--reps N] [--sizes 20,12]
  --tree DIR   import zinc_amd from another checkout's tree (a build of another commit); a tree whose library lacks
               zip_sumcheck_init_products is timed on the loop alone."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sizes", default="20,12")
ap.add_argument("--json", default=None, help="append one JSON line per measurement to this file")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from zinc_amd import cabi, pcs  # noqa: E402

Q, FL = 312829638388039969874974628075306023441, 3  # sumcheck_benches.rs:43
PRODUCTS = (2, 3, 4, 2, 3, 4, 3)
DEGREE = max(PRODUCTS)
K = sum(PRODUCTS)
HAVE_FUSED = hasattr(cabi.lib(), "zip_sumcheck_init_products")
LARGE_ROUNDS = 6


def emit(rec):
    rec["tree"] = ROOT
    if args.json:
        with open(args.json, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def make(nv):
    rng = np.random.default_rng(7)
    tables = np.zeros((K, 1 << nv, FL), dtype=np.uint64)
    tables[:, :, :2] = rng.integers(0, 2**63, size=(K, 1 << nv, 2), dtype=np.int64).view(np.uint64)  # < q
    masks, k = [], 0
    for m in PRODUCTS:
        masks.append(sum(1 << (k + i) for i in range(m)))
        k += m
    coeffs = np.zeros((len(PRODUCTS), FL), dtype=np.uint64)
    coeffs[:, 0] = rng.integers(1, 2**62, size=len(PRODUCTS))
    chal = np.zeros((nv, FL), dtype=np.uint64)
    chal[:, :2] = rng.integers(0, 2**63, size=(nv, 2), dtype=np.int64).view(np.uint64)
    return tables, masks, coeffs, chal


def run_loop(dev, nv, masks, coeffs, chal, field):
    """what prove_as_subprotocol_products' loop does per round: P round_begin, P round_end (the host sum left out)"""
    L = cabi.lib()
    hs, k = [], 0
    for p, m in enumerate(PRODUCTS):
        comb = cabi.make_comb([(1 << (m - 1)) - 1], coeffs[p:p + 1])
        hs.append(cabi.Sumcheck(dev[k:k + m], nv, DEGREE, field, comb=comb))
        k += m
    out = np.zeros((len(hs), DEGREE + 1, FL), dtype=np.uint64)
    outp = [out[i].ctypes.data for i in range(len(hs))]
    times = []
    for i in range(nv):
        rp = None if i == 0 else chal[i - 1].ctypes.data
        t0 = time.perf_counter()
        for h in hs:
            rc = L.zip_sumcheck_round_begin(h._h, rp)
            assert rc == 0, rc
        for h, o in zip(hs, outp):
            rc = L.zip_sumcheck_round_end(h._h, o)
            assert rc == 0, rc
        times.append(time.perf_counter() - t0)
    for h in hs:
        h.free()
    return times


def run_fused(dev, nv, masks, coeffs, chal, field):
    L = cabi.lib()
    h = cabi.Sumcheck(dev, nv, DEGREE, field, comb=cabi.make_comb(masks, coeffs), products=True)
    out = np.zeros((DEGREE + 1, FL), dtype=np.uint64)
    times = []
    for i in range(nv):
        rp = None if i == 0 else chal[i - 1].ctypes.data
        t0 = time.perf_counter()
        rc = L.zip_sumcheck_round(h._h, rp, out.ctypes.data)
        assert rc == 0, rc
        times.append(time.perf_counter() - t0)
    h.free()
    return times


def report(what, nv, runs):
    totals = [1e3 * sum(r) for r in runs]
    med = statistics.median(totals)
    print(f"2^{nv} {what:22s} total ms: median {med:8.3f}  min {min(totals):8.3f}  max {max(totals):8.3f}  "
          f"runs {' '.join(f'{t:.3f}' for t in totals)}", flush=True)
    if nv > LARGE_ROUNDS + 2 and all(len(r) == nv for r in runs):  # (the mirror's runs are one time each)
        per = [statistics.median(1e3 * r[i] for r in runs) for i in range(LARGE_ROUNDS)]
        rest = statistics.median(1e3 * sum(r[LARGE_ROUNDS:]) for r in runs)
        print(f"      rounds 1..{LARGE_ROUNDS} (median ms): {' '.join(f'{t:.3f}' for t in per)}; the other {nv - LARGE_ROUNDS}: {rest:.3f}", flush=True)
    emit(dict(what=what, nv=nv, total_ms=totals, median_ms=med))


def main():
    field = cabi.make_field(Q, FL)
    pfield = pcs.FieldConfig(Q, FL)
    print(f"tree {ROOT}; fused entry point: {'yes' if HAVE_FUSED else 'no'}", flush=True)
    for nv in [int(x) for x in args.sizes.split(",")]:
        tables, masks, coeffs, chal = make(nv)
        dev = [torch.from_numpy(tables[k].view(np.int64)).cuda() for k in range(K)]
        torch.cuda.synchronize()
        forms = [("device loop", run_loop)] + ([("device fused", run_fused)] if HAVE_FUSED else [])
        for what, fn in forms:
            fn(dev, nv, masks, coeffs, chal, field)  # warm-up: pool blocks, code objects
            report(what, nv, [fn(dev, nv, masks, coeffs, chal, field) for _ in range(args.reps)])
        del dev
        mk = np.array(masks, dtype=np.uint32)
        for what, knob in [("host mirror loop", "0")] + ([("host mirror fused", "1")] if HAVE_FUSED else []):
            os.environ["ZIP_HIP_SUMCHECK_FUSED"] = knob
            runs = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                pcs.sumcheck_prove_products(pcs.KeccakTranscript(), tables, DEGREE, mk, coeffs, pfield)
                if rep:
                    runs.append([time.perf_counter() - t0])
            report(what, nv, runs)
        os.environ.pop("ZIP_HIP_SUMCHECK_FUSED", None)


if __name__ == "__main__":
    main()
