#!/usr/bin/env python3
"""What a proximity test beyond the first costs (zip_ctx_set_proximity_tests), on one MI355X, at 2^20 and 2^24:

  step     one zip_commit_open call (device witness, device proof, 1000 column openings, every call marshalled once) at
           T = 1, 2, 4, 8 on ONE ctx whose count is switched between the legs;
  kernels  the new pass (combine_rows_extra_kernel) and the folds alone, by HIP events around zip_open_testing, beside
           test 0's pass (combine_rows_kernel);
  verify   one zip_verify call over the device-resident proof at T = 1, 2, 8, and by HIP events the share of
           verify_extra_tests_kernel and of the further encode_row_kernel launches.

The legs alternate (as tools/ab_step.sh alternates two builds), every repetition runs a leg often enough to last about
150 ms, the figure is the median over the repetitions with [min .. max] beside it.  The shader clock of the box is read
from a profiled commit kernel.  The table goes to profiles/proximity_tests.md.

usage: proximity_times.py [--reps N] [--num-vars 20,24] [--bench-ab PARENT_TREE [--pairs N]] [--out FILE]
--bench-ab: before anything here touches the GPU, `python bench.py` (which runs at T = 1) is run in child processes,
alternating between PARENT_TREE (a built checkout of the parent commit) and this tree: --pairs pairs with the parent
first, then as many with the branch first, all recorded in the same file."""
import argparse
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
STEP_T = (1, 2, 4, 8)
VERIFY_T = (1, 2, 8)


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


def alternate(legs, reps, sync):
    """legs: name -> callable.  -> name -> (median, min, max) seconds per call."""
    inner = {}
    for name, fn in legs.items():  # warm-up, and how many runs of the leg make about 150 ms
        fn()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        inner[name] = max(1, min(1000, int(0.15 / max(time.perf_counter() - t0, 1e-6))))
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            sync()
            t0 = time.perf_counter()
            for _k in range(inner[name]):
                fn()
            sync()
            times[name].append((time.perf_counter() - t0) / inner[name])
    return {name: (statistics.median(v), min(v), max(v)) for name, v in times.items()}


def fmt(r, scale=1e3):
    return f"{r[0] * scale:.3f} [{r[1] * scale:.3f} .. {r[2] * scale:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--num-vars", default="20,24")
    ap.add_argument("--bench-ab", metavar="PARENT_TREE")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proximity_tests.md"))
    args = ap.parse_args()
    nvs = [int(x) for x in args.num_vars.split(",")]

    pairs = []
    if args.bench_ab:
        parent = os.path.abspath(args.bench_ab)
        pairs = bench_pairs(parent, args.pairs, args.bench_steps, args.bench_warmup, False)
        pairs += bench_pairs(parent, args.pairs, args.bench_steps, args.bench_warmup, True)

    import torch  # (after the child processes: this process initialises the GPU from here on)
    from zinc_amd import cabi, pcs, perm

    if cabi.device_count() < 1:
        sys.exit("proximity_times.py needs a HIP device; there is no CPU fallback")
    zf = cabi.make_field(MODULUS, FL)
    field = pcs.FieldConfig(MODULUS, FL)
    sync = torch.cuda.synchronize
    steps, kernels, verifies, clocks = {}, {}, {}, {}
    for nv in nvs:
        row_len, num_rows, cw = cabi.geometry(nv)
        lr = num_rows.bit_length() - 1
        rng = np.random.default_rng(nv)
        ctx = cabi.ZipContext(nv, perm.shuffle_seeded_perm(1, cw), perm.shuffle_seeded_perm(2, cw))
        witness = torch.from_numpy(rng.integers(-(2**63), 2**63 - 1, size=1 << nv, dtype=np.int64)).cuda()
        coeffs = rng.integers(-(2**63), 2**63 - 1, size=(max(STEP_T), num_rows), dtype=np.int64)
        cols = rng.integers(0, cw, size=N_COLS, dtype=np.uint32)
        point = field.map_to_field(rng.integers(-100, 100, size=nv, dtype=np.int64))
        q0, q1 = field.build_eq_x_r(point[nv - lr:]), field.build_eq_x_r(point[: nv - lr])
        ev = ctx.mle_eval(witness, q0, q1, zf)
        proofs, calls = {}, {}
        for T in STEP_T:
            ctx.set_proximity_tests(T)
            proofs[T] = torch.empty(ctx.proof_len(N_COLS, FL), dtype=torch.uint8, device="cuda")
            calls[T] = ctx.commit_open_prepared(witness, coeffs[:T], cols, q0, zf, proofs[T])

        def step_leg(T):
            def leg():
                ctx.set_proximity_tests(T)
                calls[T]()
            return leg

        steps[nv] = alternate({T: step_leg(T) for T in STEP_T}, args.reps, sync)
        print(f"2^{nv} zip_commit_open ms: " + ", ".join(f"T={T} {fmt(steps[nv][T])}" for T in STEP_T), flush=True)

        # the shader clock of this box, from a profiled commit kernel
        ctx.set_proximity_tests(1)
        ctx.set_profiling(True)
        calls[1]()
        clocks[nv] = ctx.commit_clock_mhz()
        ctx.profile_read()
        # the new pass and the folds alone (zip_open_testing: test 0's pass, the new pass, T folds)
        kernels[nv] = {}
        u_out = torch.empty(max(STEP_T) * row_len * 8, dtype=torch.int64, device="cuda")
        for T in STEP_T:
            ctx.set_proximity_tests(T)
            for _ in range(20):
                ctx.open_testing(witness, coeffs[:T], out=u_out)
            kernels[nv][T] = {k: (n, ms / n) for k, (n, ms) in ctx.profile_read().items()}
        ctx.set_profiling(False)

        # the verifier: honest device-resident proofs (every leg must accept)
        roots = ctx.commit(witness)[1]
        evm = np.ascontiguousarray(ev, dtype=np.uint64)

        def verify_leg(T):
            def leg():
                ctx.set_proximity_tests(T)
                rep = ctx.verify(roots, proofs[T], coeffs[:T], cols, q0, q1, evm, zf)
                if rep["verdict"] != cabi.VERIFY_ACCEPT:
                    raise AssertionError(f"2^{nv} T={T}: honest proof rejected: {rep}")
            return leg

        verifies[nv] = {"wall": alternate({T: verify_leg(T) for T in VERIFY_T}, args.reps, sync), "kernels": {}}
        ctx.set_profiling(True)
        ctx.profile_read()
        for T in VERIFY_T:
            for _ in range(5):
                verify_leg(T)()
            verifies[nv]["kernels"][T] = {k: (n / 5, ms / 5) for k, (n, ms) in ctx.profile_read().items()}
        ctx.set_profiling(False)
        print(f"2^{nv} zip_verify ms: " + ", ".join(f"T={T} {fmt(verifies[nv]['wall'][T])}" for T in VERIFY_T), flush=True)
        witness = proofs = calls = u_out = None
        ctx.close()
        torch.cuda.empty_cache()

    L = ["# Proximity tests beyond one: what an extra test costs", "",
         "Written by `tools/proximity_times.py` on one MI355X (shader clock during a profiled commit kernel: "
         + ", ".join(f"2^{nv}: {clocks[nv]:.0f} MHz" for nv in nvs) + f").  {N_COLS} column openings, 4-limb field, device-resident",
         f"witness and proof.  Medians of {args.reps} alternated repetitions of about 150 ms each, [min .. max] beside them.", "",
         "## zip_commit_open, one call per step", "",
         "One ctx, its count switched between the legs.  T = 1 launches what a ctx without the notion launches.", "",
         "| num_vars | T | ms per step | over T = 1 |", "|---|---|---|---|"]
    for nv in nvs:
        for T in STEP_T:
            r = steps[nv][T]
            L.append(f"| {nv} | {T} | {fmt(r)} | {(r[0] - steps[nv][1][0]) * 1e3:+.3f} ms ({r[0] / steps[nv][1][0]:.3f}x) |")
    L += ["", "## The new pass and its folds alone", "",
          "HIP events around every launch of zip_open_testing (no commit kernel beside them): mean ms per launch over 20 calls.", "",
          "| num_vars | T | combine_rows_kernel (test 0) | combine_rows_extra_kernel (tests 1 .. T-1) | combine_finalize_kernel, per launch (launches per call) |",
          "|---|---|---|---|---|"]
    for nv in nvs:
        for T in STEP_T:
            k = kernels[nv][T]
            extra = f"{k['combine_rows_extra_kernel'][1]:.4f}" if "combine_rows_extra_kernel" in k else "not launched"
            fin = k["combine_finalize_kernel"]
            L.append(f"| {nv} | {T} | {k['combine_rows_kernel'][1]:.4f} | {extra} | {fin[1]:.4f} ({fin[0] // 20}) |")
    L += ["", "## zip_verify, one call per proof", "",
          "Wall time of the call (it returns after its own synchronise), and by HIP events the kernels an extra test adds: ms per call.", "",
          "| num_vars | T | ms per call | verify_extra_tests_kernel | encode_row_kernel (all launches) | verify_columns_kernel |",
          "|---|---|---|---|---|---|"]
    for nv in nvs:
        for T in VERIFY_T:
            k = verifies[nv]["kernels"][T]
            extra = f"{k['verify_extra_tests_kernel'][1]:.4f}" if "verify_extra_tests_kernel" in k else "not launched"
            L.append(f"| {nv} | {T} | {fmt(verifies[nv]['wall'][T])} | {extra} | {k['encode_row_kernel'][1]:.4f} ({k['encode_row_kernel'][0]:.0f} launches) "
                     f"| {k['verify_columns_kernel'][1]:.4f} |")
    if pairs:
        L += ["", "## bench.py on the parent commit and on this branch", "",
              f"`python bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}` (it runs at T = 1), same box, alternated; the parent leg runs",
              f"in a built checkout of the parent commit.  {args.pairs} pairs with the parent first, then {args.pairs} with the branch first.  No kernel on",
              "that path changes, so the expectation is \"unchanged within the box's own run-to-run spread\".", "",
              "| pair | order | build | ms per step | MCoeffs/s |", "|---|---|---|---|---|"]
        for k, order, name, ms, v in pairs:
            L.append(f"| {k} | {order} | {name} | {ms} | {v} |")
        pm = [ms for _, _, n, ms, _ in pairs if n == "parent"]
        bm = [ms for _, _, n, ms, _ in pairs if n == "branch"]
        med = round(statistics.median(bm), 4)
        inside = min(pm) <= med <= max(pm)
        L += ["", f"Parent: {min(pm)} .. {max(pm)} ms per step over its {len(pm)} runs (median {round(statistics.median(pm), 4)}).  Branch: {min(bm)} .. {max(bm)}, "
              f"median {med}: " + ("inside the parent's own run-to-run range." if inside else "OUTSIDE the parent's own run-to-run range.")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
