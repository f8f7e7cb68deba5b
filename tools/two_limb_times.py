#!/usr/bin/env python3
"""What a two-limb (INT_LIMBS = 2) ctx costs beside a one-limb ctx, on one MI355X, at 2^20 and 2^24, device-resident
witness and proof, 1000 column openings, the 256-bit bench modulus:

  calls    zip_commit, zip_open, zip_commit_open and zip_verify of a two-limb ctx, and in the same process the one-limb
           plain zip_commit with no hint (speculation off: the full-materialisation path), zip_open and zip_verify --
           the comparison.  Host clock around calls that end in a synchronise;
  kernels  every kernel of the two-limb path by HIP events (zip_ctx_profile_read): ms per launch.

The legs alternate, every repetition runs a leg often enough to last about 150 ms, the figure is the median over the
repetitions with [min .. max] beside it.  The shader clock of the box is read from a profiled one-limb commit kernel.
The table goes to profiles/two_limb.md.

usage: two_limb_times.py [--reps N] [--num-vars 20,24] [--bench-ab PARENT_TREE [--pairs N]] [--out FILE]
--bench-ab: before anything here touches the GPU, `python bench.py` (one limb) is run in child processes, alternating
between PARENT_TREE (a built checkout of the parent commit) and this tree, and recorded in the same file."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from proximity_times import alternate, bench_pairs, fmt  # noqa: E402  (the same alternation and the same bench A/B)

N_COLS = 1000
MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383  # benches/zip_benches.rs:253
FL = 4
LEGS = ("two-limb zip_commit", "two-limb zip_open", "two-limb zip_commit_open", "two-limb zip_verify",
        "one-limb zip_commit (no hint)", "one-limb zip_open", "one-limb zip_verify")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--num-vars", default="20,24")
    ap.add_argument("--bench-ab", metavar="PARENT_TREE")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_limb.md"))
    args = ap.parse_args()
    nvs = [int(x) for x in args.num_vars.split(",")]
    assert args.reps >= 6, "medians of at least six alternated runs"

    pairs = []
    if args.bench_ab:
        parent = os.path.abspath(args.bench_ab)
        pairs = bench_pairs(parent, args.pairs, args.bench_steps, args.bench_warmup, False)
        pairs += bench_pairs(parent, args.pairs, args.bench_steps, args.bench_warmup, True)

    import torch  # (after the child processes: this process initialises the GPU from here on)
    from zinc_amd import cabi, pcs, perm

    if cabi.device_count() < 1:
        sys.exit("two_limb_times.py needs a HIP device; there is no CPU fallback")
    zf = cabi.make_field(MODULUS, FL)
    field = pcs.FieldConfig(MODULUS, FL)
    sync = torch.cuda.synchronize
    walls, kernels, clocks, sizes = {}, {}, {}, {}
    for nv in nvs:
        row_len, num_rows, cw = cabi.geometry(nv)
        lr = num_rows.bit_length() - 1
        rng = np.random.default_rng(nv)
        p1, p2 = perm.shuffle_seeded_perm(1, cw), perm.shuffle_seeded_perm(2, cw)
        ctx2 = cabi.ZipContext(nv, p1, p2, n_limbs=2, k_limbs=8, m_limbs=16)
        ctx1 = cabi.ZipContext(nv, p1, p2)
        ctx1.set_speculation(False)  # plain commits store everything: the full-materialisation path
        w2 = torch.from_numpy(rng.integers(-(2**63), 2**63 - 1, size=(1 << nv, 2), dtype=np.int64)).cuda()
        w1 = torch.from_numpy(rng.integers(-(2**63), 2**63 - 1, size=1 << nv, dtype=np.int64)).cuda()
        c2 = rng.integers(-(2**63), 2**63 - 1, size=(num_rows, 2), dtype=np.int64)
        c1 = rng.integers(-(2**63), 2**63 - 1, size=num_rows, dtype=np.int64)
        cols = rng.integers(0, cw, size=N_COLS, dtype=np.uint32)
        point = field.map_to_field(rng.integers(-100, 100, size=nv, dtype=np.int64))
        q0, q1 = field.build_eq_x_r(point[nv - lr:]), field.build_eq_x_r(point[: nv - lr])
        ev2 = np.ascontiguousarray(ctx2.mle_eval(w2, q0, q1, zf), dtype=np.uint64)
        ev1 = np.ascontiguousarray(ctx1.mle_eval(w1, q0, q1, zf), dtype=np.uint64)
        proof2 = torch.empty(ctx2.proof_len(N_COLS, FL), dtype=torch.uint8, device="cuda")
        proof1 = torch.empty(ctx1.proof_len(N_COLS, FL), dtype=torch.uint8, device="cuda")
        sizes[nv] = (proof2.numel(), proof1.numel(), num_rows * cw * 64, num_rows * cw * 32)
        com2, roots2 = ctx2.commit(w2)
        com1, roots1 = ctx1.commit(w1)
        com2.open(w2, c2, cols, q0, zf, out=proof2)
        com1.open(w1, c1, cols, q0, zf, out=proof1)
        ctx1.set_speculation(False)

        def commit_leg(ctx, w):
            def leg():
                com, _ = ctx.commit(w, want_roots=False)
                com.free()  # (waits for the commit: the handle's blocks go back to the ctx's pool)
            return leg

        def verify_leg(ctx, roots, proof, c, ev, what):
            def leg():
                rep = ctx.verify(roots, proof, c, cols, q0, q1, ev, zf)
                if rep["verdict"] != cabi.VERIFY_ACCEPT:
                    raise AssertionError(f"2^{nv} {what}: honest proof rejected: {rep}")
            return leg

        legs = {
            LEGS[0]: commit_leg(ctx2, w2),
            LEGS[1]: lambda: com2.open(w2, c2, cols, q0, zf, out=proof2),
            LEGS[2]: lambda: ctx2.commit_open(w2, c2, cols, q0, zf, out=proof2, want_roots=False),
            LEGS[3]: verify_leg(ctx2, roots2, proof2, c2, ev2, "two-limb"),
            LEGS[4]: commit_leg(ctx1, w1),
            LEGS[5]: lambda: com1.open(w1, c1, cols, q0, zf, out=proof1),
            LEGS[6]: verify_leg(ctx1, roots1, proof1, c1, ev1, "one-limb"),
        }
        walls[nv] = alternate(legs, args.reps, sync)
        for name in LEGS:
            print(f"2^{nv} {name}: {fmt(walls[nv][name])} ms", flush=True)

        # the shader clock of this box, from a profiled one-limb commit kernel
        ctx1.set_profiling(True)
        legs[LEGS[4]]()
        clocks[nv] = ctx1.commit_clock_mhz()
        ctx1.profile_read()
        ctx1.set_profiling(False)
        # every kernel of the two-limb path, ms per launch
        ctx2.set_profiling(True)
        ctx2.profile_read()
        kernels[nv] = {}
        for what in LEGS[:4]:
            if what == LEGS[2]:
                continue  # (commit_open launches what commit and open launch)
            for _ in range(5):
                legs[what]()
            kernels[nv][what] = {k: (n / 5, ms / n) for k, (n, ms) in ctx2.profile_read().items()}
        ctx2.set_profiling(False)
        com1.free()
        com2.free()
        w1 = w2 = proof1 = proof2 = None
        ctx1.close()
        ctx2.close()
        torch.cuda.empty_cache()

    L = ["# Two-limb witnesses (INT_LIMBS = 2): what they cost beside one limb", "",
         "Written by `tools/two_limb_times.py` on one MI355X (shader clock during a profiled one-limb commit kernel: "
         + ", ".join(f"2^{nv}: {clocks[nv]:.0f} MHz" for nv in nvs) + f").  {N_COLS} column openings, 4-limb field, device-resident",
         f"witness and proof, every leg warmed up once.  Medians of {args.reps} alternated repetitions of about 150 ms each, [min .. max] beside them.", "",
         "## Calls", "",
         "Host clock around calls that end in a synchronise.  The one-limb legs run in the same process on a ctx with",
         "speculation off: its plain `zip_commit` takes no hint and stores every row entry and every tree node, which is what a",
         "two-limb commit always does.", "",
         "| num_vars | call | ms per call | against the one-limb call |", "|---|---|---|---|"]
    base = {LEGS[0]: LEGS[4], LEGS[1]: LEGS[5], LEGS[3]: LEGS[6]}
    for nv in nvs:
        for name in LEGS:
            r = walls[nv][name]
            if name == LEGS[2]:
                ref = walls[nv][LEGS[4]][0] + walls[nv][LEGS[5]][0]
                rel = f"{r[0] / ref:.2f}x one-limb commit + open"
            else:
                rel = f"{r[0] / walls[nv][base[name]][0]:.2f}x" if name in base else ""
            L.append(f"| {nv} | {name} | {fmt(r)} | {rel} |")
    L += ["", "Bytes: " + "; ".join(f"2^{nv}: proof {sizes[nv][0] / 2**20:.1f} MiB (one limb {sizes[nv][1] / 2**20:.1f}), row entries "
                                   f"{sizes[nv][2] / 2**20:.0f} MiB (one limb, Int<4>: {sizes[nv][3] / 2**20:.0f})" for nv in nvs) + ".", "",
          "## Kernels of the two-limb path", "",
          "HIP events around every launch (`zip_ctx_profile_read`), 5 calls each: launches per call and mean ms per launch.", "",
          "| num_vars | call | kernel | launches per call | ms per launch |", "|---|---|---|---|---|"]
    for nv in nvs:
        for what, ks in kernels[nv].items():
            for k, (n, ms) in sorted(ks.items()):
                L.append(f"| {nv} | {what} | {k} | {n:g} | {ms:.4f} |")
    if pairs:
        L += ["", "## bench.py (one limb, 2^24) on the parent commit and on this branch", "",
              f"`python bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}`, same box, alternated; the parent leg runs in a built",
              f"checkout of the parent commit.  {args.pairs} pairs with the parent first, then {args.pairs} with the branch first.  No one-limb kernel",
              "instance and no launch on that path changes, so the expectation is \"unchanged within the box's own run-to-run spread\".", "",
              "| pair | order | build | ms per step | MCoeffs/s |", "|---|---|---|---|---|"]
        for k, order, name, ms, v in pairs:
            L.append(f"| {k} | {order} | {name} | {ms} | {v} |")
        pm = [ms for _, _, n, ms, _ in pairs if n == "parent"]
        bm = [ms for _, _, n, ms, _ in pairs if n == "branch"]
        med = round(statistics.median(bm), 4)
        inside = min(pm) <= med <= max(pm)
        L += ["", f"Parent: {min(pm)} .. {max(pm)} ms per step over its {len(pm)} runs (median {round(statistics.median(pm), 4)}).  Branch: {min(bm)} .. {max(bm)}, "
              f"median {med}: " + ("inside the parent's own run-to-run range." if inside else "OUTSIDE the parent's own run-to-run range.")]
    notes = os.path.join(os.path.dirname(args.out), "two_limb_notes.md")
    if os.path.exists(notes):  # the reading of the figures, kept beside them and appended as it stands
        L += ["", open(notes).read().rstrip()]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
