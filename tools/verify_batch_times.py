#!/usr/bin/env python3
"""ZincVerifier::verify_batch against the loop over verify of the SAME build, per instance count B: B proofs of one circuit
of t = 3 matrices (what an untimed prove_batch makes), every proof with its own (distinct, prime) 4-limb modulus and its own
transcript, hence its own RAA code; 1000 openings.  The batch leg runs with ZIP_HIP_VERIFY_MIN_BATCH=2, the loop leg with
ZIP_HIP_BATCH=0.  Measured separately:
  whole   verify_batch, batched against looped (the host work of both sumcheck verifiers is in both legs)
  PCS     zip_batch_verify_codes (a code, a field and a stream pointer per member) against the loop of zip_verify on
          per-member contexts -- a zip_ctx_create with the member's permutations, one zip_verify, the ctx destroyed --,
          on the challenges an untimed host walk left
  V_xy    zip_ccs_batch_eval_matrices on one handle (its creation included: verify_batch makes one per call) against the
          loop of a zip_ccs in the member's field (what PreparedCcs is) plus zip_ccs_eval_matrices
Host clocks around calls that end in a device synchronise; the legs alternate after one warm-up of each, and the warm-up
also compares the two legs' results.  Reported: medians and the loop's spread; the batch "wins" where it beats the loop by
more than that spread.

Every (rows, B) cell runs in a process of its own under its own time limit; after a cell that fails or runs out of time
nothing further is started.  A cell whose proof streams do not fit half the device's free memory is left out and listed.
GPU box.

usage: verify_batch_times.py [--reps N] [--sizes 10,12,14,16] [--counts 2,16,256] [--md FILE] [--limit SECONDS]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="10,12,14,16")
ap.add_argument("--counts", default="2,16,256")
ap.add_argument("--md", default=None, help="write the table as markdown to this file")
ap.add_argument("--limit", type=int, default=240, help="seconds one (rows, B) cell may take")
ap.add_argument("--cell", default=None, help="(internal) s,B: measure this one cell and print its row")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BASE, FL = 106319353542452952636349991594949358997917625194731877894581586278529202198383, 4
S, COEFFS, D = [[0, 1], [2]], [1, -1], 2
HEAD = ("| rows | B | whole: loop ms median (min .. max) | whole: batch ms | loop / batch | wins | PCS: loop ms median (min .. max) | "
        "PCS: batch ms | loop / batch | wins | V_xy: loop ms median (min .. max) | V_xy: batch ms | loop / batch | wins |")


def is_probable_prime(n):
    """Miller-Rabin to fixed bases (the verifier inverts by Fermat's little theorem: its moduli must be primes)"""
    if n < 2 or n % 2 == 0:
        return n == 2
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def moduli(B):
    """B distinct 4-limb primes, downwards from BASE: every proof has its own field"""
    out, q = [], BASE
    while len(out) < B:
        if is_probable_prime(q):
            out.append(q)
        q -= 2
    return out


def circuit(s):
    """A = B = C = I: z_i * z_i = z_i, satisfied by every 0/1 vector (the proofs are honest and accepted)"""
    import types

    m = 1 << s
    idx = np.arange(m, dtype=np.uint32)
    one = types.SimpleNamespace(n_rows=m, n_cols=m, row_ptr=np.arange(m + 1, dtype=np.uint32), col_idx=idx, values=np.ones(m, dtype=np.int64))
    return [one, one, one]


class Config:
    def __init__(self, cabi, pcs, s, B):
        self.cabi, self.pcs, self.s, self.B, self.mats = cabi, pcs, s, B, circuit(s)
        rng = np.random.default_rng(s * 1000 + B)
        z = rng.integers(0, 2, size=(B, 1 << s), dtype=np.int64)
        z[:, 1] = 1
        qs = moduli(B)
        self.fields = [pcs.FieldConfig(q, FL) for q in qs]
        self.zfields = [cabi.make_field(q, FL) for q in qs]
        os.environ["ZIP_HIP_BATCH"] = "1"
        self.proofs = pcs.ZincProver().prove_batch(self.mats, s, D, S, COEFFS, [z[i, :1] for i in range(B)], [z[i, 2:] for i in range(B)],
                                                   self.fresh(), self.fields)
        self.verifier = pcs.ZincVerifier()
        self._pcs_inputs()

    def fresh(self):
        ts = []
        for i in range(self.B):
            t = self.pcs.KeccakTranscript()
            t.absorb(bytes([i & 255, i >> 8]))
            ts.append(t)
        return ts

    def _pcs_inputs(self):
        """the host walk of every member (untimed): the Spartan part, the code of its transcript, the squeezes, the tensors"""
        pcs, cabi, s = self.pcs, self.cabi, self.s
        self.row_len, self.num_rows, self.cw = cabi.geometry(s)
        lr = self.num_rows.bit_length() - 1
        ts = self.fresh()
        self.r_x, self.r_y, p1, p2, cols, coeffs, q0, q1 = [], [], [], [], [], [], [], []
        for proof, t, f in zip(self.proofs, ts, self.fields):
            pts = self.verifier.spartan_verify(self.mats, s, D, S, COEFFS, proof, t, f)
            self.r_x.append(pts["rx_ry"][:s])
            self.r_y.append(pts["rx_ry"][s:])
            code = pcs.RaaCode(1 << s, t)
            assert code.codeword_len() == self.cw
            p1.append(pcs.shuffle_seeded_perm(code.perm_1_seed, self.cw))
            p2.append(pcs.shuffle_seeded_perm(code.perm_2_seed, self.cw))
            k, c = pcs.MultilinearZip.open_challenges(self.num_rows, self.cw, 1000, 1, f, pcs.PcsTranscript.from_proof(proof["zip_proof"]["pcs_proof"]))
            cols.append(c)
            coeffs.append(k[0] if k is not None else None)
            q0.append(f.build_eq_x_r(self.r_y[-1][s - lr:]) if lr else None)
            q1.append(f.build_eq_x_r(self.r_y[-1][: s - lr]) if s - lr else None)
        stack = lambda a: None if a[0] is None else np.stack(a)
        self.perms1, self.perms2, self.cols = np.stack(p1), np.stack(p2), np.stack(cols)
        self.coeffs, self.q0, self.q1 = stack(coeffs), stack(q0), stack(q1)
        self.roots = np.stack([p["zip_proof"]["z_comm"] for p in self.proofs])
        self.streams = [p["zip_proof"]["pcs_proof"] for p in self.proofs]
        self.evs = np.stack([p["zip_proof"]["v"] for p in self.proofs])
        self.shared = cabi.ZipContext(s, p1[0], p2[0])

    # ---- the three measurements: (seconds, result)
    def whole(self, batched):
        os.environ["ZIP_HIP_BATCH"] = "1" if batched else "0"
        ts = self.fresh()
        t0 = time.perf_counter()
        out = self.verifier.verify_batch(self.mats, self.s, D, S, COEFFS, self.proofs, ts, self.fields)
        return time.perf_counter() - t0, [None if e is None else (type(e).__name__, str(e)) for e in out]

    def pcs_part(self, batched):
        cabi, pick = self.cabi, lambda a, i: None if a is None else a[i]
        t0 = time.perf_counter()
        if batched:
            out = self.shared.batch_verify_codes(self.perms1, self.perms2, self.roots, self.streams, self.coeffs, self.cols, self.q0, self.q1,
                                                 self.evs, self.zfields)
        else:
            out = []
            for i in range(self.B):
                own = cabi.ZipContext(self.s, self.perms1[i], self.perms2[i])
                out.append(own.verify(self.roots[i], self.streams[i], pick(self.coeffs, i), self.cols[i], pick(self.q0, i), pick(self.q1, i),
                                      self.evs[i], self.zfields[i]))
                own.close()
        return time.perf_counter() - t0, out

    def vxy(self, batched):
        cabi = self.cabi
        t0 = time.perf_counter()
        if batched:
            h = cabi.CcsBatch(self.mats, self.s, FL, self.B)
            out = h.eval_matrices(self.zfields, np.stack(self.r_x), np.stack(self.r_y))
            h.free()
        else:
            rows = []
            for i in range(self.B):
                one = cabi.Ccs(self.mats, self.s, self.zfields[i])
                rows.append(one.eval_matrices(self.r_x[i], self.r_y[i]))
                one.free()
            out = np.stack(rows)
        return time.perf_counter() - t0, out


def cell(s, B):
    import torch

    from zinc_amd import cabi, pcs

    os.environ["ZIP_HIP_VERIFY_MIN_BATCH"] = "2"
    ctx = cabi.ZipContext(s, np.arange(cabi.geometry(s)[2], dtype=np.uint32), np.arange(cabi.geometry(s)[2], dtype=np.uint32))
    need = B * ctx.proof_len(1000, FL)
    ctx.close()
    free, _ = torch.cuda.mem_get_info()
    if need > free // 2:
        print(f"SKIP | 2^{s} | {B} | {need / 2**30:.1f} GiB of proof streams, {free / 2**30:.1f} GiB free on the device", flush=True)
        return
    cfg = Config(cabi, pcs, s, B)
    before = cabi.batch_verify_codes_counts()
    (_, a), (_, b) = cfg.whole(False), cfg.whole(True)  # warm-up: pool blocks, code objects -- and the legs' results
    assert a == b, "the legs' outcomes differ"
    assert all(x is None for x in a), "an honest proof was rejected"
    assert cabi.batch_verify_codes_counts() == (before[0] + 1, before[1] + B), "the batch leg took the other path"
    (_, a), (_, b) = cfg.pcs_part(False), cfg.pcs_part(True)
    assert a == b, "the PCS legs' reports differ"
    (_, a), (_, b) = cfg.vxy(False), cfg.vxy(True)
    assert np.array_equal(a, b), "the V_xy legs differ"
    reps = args.reps if B < 256 else max(3, args.reps // 2)
    cols = []
    for fn in (cfg.whole, cfg.pcs_part, cfg.vxy):
        tl, tb = [], []
        for _ in range(reps):  # alternating
            tl.append(1e3 * fn(False)[0])
            tb.append(1e3 * fn(True)[0])
        ml, mb = statistics.median(tl), statistics.median(tb)
        wins = ml - mb > max(tl) - min(tl)
        cols.append(f"{ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {mb:.3f} | {ml / mb:.2f} | {'yes' if wins else 'no'}")
    print(f"ROW | 2^{s} | {B} | " + " | ".join(cols) + " |", flush=True)


def main():
    if args.cell:
        s, B = (int(x) for x in args.cell.split(","))
        return cell(s, B)
    print(HEAD, flush=True)
    rows, skipped = [], []

    def write():
        if args.md:
            with open(args.md, "w") as fh:
                fh.write(HEAD + "\n" + "|---" * 14 + "|\n" + "\n".join(rows) + "\n")
                if skipped:
                    fh.write("\nLeft out (the streams do not fit half the device's free memory):\n\n" + "\n".join("- " + x for x in skipped) + "\n")

    for s in [int(x) for x in args.sizes.split(",")]:
        for B in [int(x) for x in args.counts.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", f"{s},{B}", "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"2^{s} x {B}: no result within {args.limit} s; nothing further is started", flush=True)
                write()
                return 1
            row = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
            skip = [ln[5:] for ln in r.stdout.splitlines() if ln.startswith("SKIP ")]
            if r.returncode != 0 or not (row or skip):
                print(f"2^{s} x {B}: exit status {r.returncode}; nothing further is started\n{(r.stdout + r.stderr)[-3000:]}", flush=True)
                write()
                return 1
            if skip:
                print("left out: " + skip[0], flush=True)
                skipped.append(skip[0])
            else:
                print(row[0], flush=True)
                rows.append(row[0])
            write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
