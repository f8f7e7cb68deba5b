#!/usr/bin/env python3
"""Batched verifier against the loop at the sizes of the reference's own Zip benches (benches/zip_benches.rs:
2^12 .. 2^16): wall time per polynomial of

  batch  one zip_batch_verify call for B proofs (one launch set, one copy of B reports back), and
  loop   B calls of zip_verify, one per proof,

on the same ctx, over the same device-resident proofs that zip_batch_open made (honest proofs, 1000 column openings
each; both legs must accept all of them), every call marshalled once.  The legs alternate, every repetition runs a leg
often enough to last about 150 ms, and the figure is the median over the repetitions (the spread is printed beside it).
The table goes to profiles/batch_verify_small.md, with the B from which the batch wins at every size.

usage: batch_verify_times.py [--reps N] [--num-vars 12,13,..] [--batches 1,16,..] [--bench-ab PARENT_TREE [--pairs N]] [--out FILE]
--bench-ab: before anything here touches the GPU, `python bench.py` is run in child processes, alternating between
PARENT_TREE (a built checkout of the parent commit) and this tree: --pairs pairs with the parent first, then as many
with the branch first, and all of them are recorded in the same file."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_COLS = 1000
MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383  # benches/zip_benches.rs:253
FL = 4


def bench_pairs(parent_tree, pairs, steps, warmup, branch_first):
    rows = []
    env = dict(os.environ)
    env.pop("ZIP_HIP_LIB_PATH", None)
    order = (("branch", ROOT), ("parent", parent_tree)) if branch_first else (("parent", parent_tree), ("branch", ROOT))
    for k in range(pairs):
        for name, tree in order:
            res = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                                  str(warmup)], env=env, cwd=tree, capture_output=True, text=True, timeout=900)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
            if res.returncode or not line:
                raise RuntimeError(f"bench.py ({name}) failed: {res.returncode}\n{res.stderr[-2000:]}")
            out = json.loads(line[-1])
            rows.append((k, "branch first" if branch_first else "parent first", name, out["ms_per_step"], out["value"]))
            print(f"bench.py pair {k} ({rows[-1][1]}) {name}: {out['ms_per_step']} ms per step, {out['value']} {out.get('unit', '')}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--num-vars", default="12,13,14,15,16")
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--bench-ab", metavar="PARENT_TREE")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_verify_small.md"))
    args = ap.parse_args()
    nvs = [int(x) for x in args.num_vars.split(",")]
    Bs = [int(x) for x in args.batches.split(",")]

    pairs = []
    if args.bench_ab:
        parent = os.path.abspath(args.bench_ab)
        pairs = bench_pairs(parent, args.pairs, args.bench_steps, args.bench_warmup, False)
        pairs += bench_pairs(parent, args.pairs, args.bench_steps, args.bench_warmup, True)

    import torch  # (after the child processes: this process initialises the GPU from here on)
    from zinc_amd import cabi, pcs, perm

    if cabi.device_count() < 1:
        sys.exit("batch_verify_times.py needs a HIP device; there is no CPU fallback")
    zf = cabi.make_field(MODULUS, FL)
    field = pcs.FieldConfig(MODULUS, FL)
    L = cabi.lib()
    table = {}
    for nv in nvs:
        row_len, num_rows, cw = cabi.geometry(nv)
        lr = num_rows.bit_length() - 1
        ctx = cabi.ZipContext(nv, perm.shuffle_seeded_perm(1, cw), perm.shuffle_seeded_perm(2, cw))
        plen = ctx.proof_len(N_COLS, FL)
        for B in Bs:
            rng = np.random.default_rng(nv * 1000 + B)
            try:
                witness = torch.from_numpy(rng.integers(-(2**63), 2**63 - 1, size=(B, 1 << nv), dtype=np.int64)).cuda()
                proofs = torch.empty((B, plen), dtype=torch.uint8, device="cuda")
                coeffs = rng.integers(-(2**63), 2**63 - 1, size=(B, num_rows), dtype=np.int64)
                cols = rng.integers(0, cw, size=(B, N_COLS), dtype=np.uint32)
                points = [field.map_to_field(rng.integers(-100, 100, size=nv, dtype=np.int64)) for _ in range(B)]
                q0 = np.stack([field.build_eq_x_r(pt[nv - lr:]) for pt in points])
                q1 = np.stack([field.build_eq_x_r(pt[: nv - lr]) for pt in points])
                # honest proofs and their claims, made on the device
                batch = ctx.batch_commit(witness)
                batch.open(coeffs, cols, q0, zf, out=proofs)
                roots = np.ascontiguousarray(batch.roots)
                evs = np.stack([ctx.mle_eval(witness[i], q0[i], q1[i], zf) for i in range(B)])
                batch.free()

                reps_b = (cabi.VerifyReport * B)()
                args_b = (ctx._h, B, roots.ctypes.data, proofs.data_ptr(), cabi.MEM_DEVICE, B * plen, coeffs.ctypes.data,
                          cols.ctypes.data, N_COLS, q0.ctypes.data, q1.ctypes.data, evs.ctypes.data, C.byref(zf), reps_b)
                reps_l = (cabi.VerifyReport * B)()
                args_l = [(ctx._h, roots[i].ctypes.data, proofs[i].data_ptr(), cabi.MEM_DEVICE, plen, coeffs[i].ctypes.data,
                           cols[i].ctypes.data, N_COLS, q0[i].ctypes.data, q1[i].ctypes.data, evs[i].ctypes.data, C.byref(zf),
                           C.byref(reps_l[i])) for i in range(B)]

                def leg_batch():
                    rc = L.zip_batch_verify(*args_b)
                    if rc:
                        ctx._check(rc, "zip_batch_verify")

                def leg_loop():
                    for a in args_l:
                        rc = L.zip_verify(*a)
                        if rc:
                            ctx._check(rc, "zip_verify")

                legs = {"batch": leg_batch, "loop": leg_loop}
                inner = {}
                for name, fn in legs.items():  # warm-up, and how many runs of the leg make about 150 ms
                    fn()
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    inner[name] = max(1, min(1000, int(0.15 / max(dt, 1e-6))))
                for reps in (reps_b, reps_l):
                    bad = [(i, r.verdict) for i, r in enumerate(reps) if r.verdict != cabi.VERIFY_ACCEPT]
                    if bad:
                        raise AssertionError(f"2^{nv} B={B}: honest proofs rejected: {bad[:4]}")
                times = {name: [] for name in legs}
                for _ in range(args.reps):
                    for name, fn in legs.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _k in range(inner[name]):
                            fn()
                        times[name].append((time.perf_counter() - t0) / inner[name] / B)
                table[(nv, B)] = {name: (statistics.median(v), min(v), max(v)) for name, v in times.items()}
                b, l = table[(nv, B)]["batch"], table[(nv, B)]["loop"]
                print(f"2^{nv} B={B}: batch {b[0] * 1e6:.1f} us per polynomial [{b[1] * 1e6:.1f} .. {b[2] * 1e6:.1f}], "
                      f"loop {l[0] * 1e6:.1f} us [{l[1] * 1e6:.1f} .. {l[2] * 1e6:.1f}], loop / batch {l[0] / b[0]:.2f}", flush=True)
            except (cabi.ZipError, RuntimeError, MemoryError) as e:  # (torch reports a refused allocation as RuntimeError)
                if "memory" not in str(e).lower() and "alloc" not in str(e).lower():
                    raise
                table[(nv, B)] = None
                print(f"2^{nv} B={B}: memory refused ({str(e).splitlines()[0][:120]})", flush=True)
            finally:
                witness = proofs = args_b = args_l = None
                torch.cuda.empty_cache()
        ctx.close()

    lines = ["# Batched verifier against the loop at 2^12 .. 2^16", "",
             "Written by `tools/batch_verify_times.py` on one MI355X.  Wall time per polynomial, device-resident honest proofs made by",
             f"zip_batch_open, {N_COLS} column openings, 4-limb field; `batch` = one zip_batch_verify call for B proofs, `loop` = B calls of",
             f"zip_verify on the same ctx (every call marshalled once).  Medians of {args.reps} alternated repetitions of about 150 ms each,",
             "[min .. max] beside them; every call returns after its own synchronise.", "",
             "| num_vars | B | batch us / polynomial | loop us / polynomial | loop / batch |", "|---|---|---|---|---|"]
    for nv in nvs:
        for B in Bs:
            r = table.get((nv, B))
            if r is None:
                lines.append(f"| {nv} | {B} | memory refused | | |")
                continue
            b, l = r["batch"], r["loop"]
            lines.append(f"| {nv} | {B} | {b[0] * 1e6:.1f} [{b[1] * 1e6:.1f} .. {b[2] * 1e6:.1f}] | {l[0] * 1e6:.1f} [{l[1] * 1e6:.1f} .. {l[2] * 1e6:.1f}] "
                         f"| {l[0] / b[0]:.2f} |")
    lines += ["", "From which B the batch wins (its median below the loop's):", ""]
    any_win = False
    for nv in nvs:
        wins = [B for B in Bs if table.get((nv, B)) and table[(nv, B)]["batch"][0] < table[(nv, B)]["loop"][0]]
        any_win |= bool(wins)
        lines.append(f"- 2^{nv}: " + (f"from B = {min(wins)} (wins at B in {wins})" if wins else "the batch wins at no measured B"))
    if not any_win:
        lines += ["", "The batch wins nowhere at these sizes."]
    lost = [f"2^{nv} B = {B}" for nv in nvs for B in Bs
            if table.get((nv, B)) and table[(nv, B)]["batch"][0] >= table[(nv, B)]["loop"][0]]
    if lost and any_win:
        lines += ["", "The batch loses at " + ", ".join(lost) + "."]
    if pairs:
        lines += ["", "## bench.py on the parent commit and on this branch", "",
                  f"`python bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}`, same box, alternated; the parent leg runs in a built",
                  f"checkout of the parent commit.  {args.pairs} pairs with the parent first, then {args.pairs} with the branch first (the order effect",
                  "profiles/batch_small.md left open).  No kernel on that path changes, so the expectation is \"unchanged within the",
                  "box's own run-to-run spread\".", "",
                  "| pair | order | build | ms per step | MCoeffs/s |", "|---|---|---|---|---|"]
        for k, order, name, ms, v in pairs:
            lines.append(f"| {k} | {order} | {name} | {ms} | {v} |")
        for order in ("parent first", "branch first"):
            pm = [ms for _, o, n, ms, _ in pairs if n == "parent" and o == order]
            bm = [ms for _, o, n, ms, _ in pairs if n == "branch" and o == order]
            lines += ["", f"{order}: parent {min(pm)} .. {max(pm)} ms per step, branch {min(bm)} .. {max(bm)} ms per step."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
