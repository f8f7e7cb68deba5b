#!/usr/bin/env python3
"""CCS with more than three matrices at 2^nv constraints (the shapes of tests/_ccs_wide.py): per-round wall times of the
first sumcheck -- t + 1 = 5..8 tables, sumcheck_round_wide_kernel -- over the zip_ccs tables in HBM, and
SpartanProver::prove through the C facade with HOST buffers in and out, as tools/zinc_prover_times.py times the R1CS
instance.  The instance is built like tests/_ccs_wide.wide_ccs (every row fixes one witness entry from entries in the
columns 0..3) but with numpy, row-parallel: 2^20 rows in pure Python take minutes.  GPU box.

  python3 tools/sumcheck_wide_times.py 20 --shapes plonk6 t7d3 --prove plonk6"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ccs  # noqa: E402
import _ccs_wide  # noqa: E402

STARK = 3618502788666131213697322783095070105623107215331596699973092056135872020481  # spartan_benches.rs:161


def big_instance(name, s, seed=7):
    """rows 0, 1 (which fix z[2], z[3]) from the Python generator, every later row from numpy: one or two entries per
    matrix in columns 0..3, the last term's matrix the entry (1, r + 2)"""
    S, c = _ccs_wide.SHAPES[name]
    n, t = 1 << s, sum(len(Si) for Si in S)
    while True:
        rows4, z4 = _ccs_wide._generate(2, S, c, seed)
        zmax = max(abs(v) for v in z4)
        if sum(abs(ci) for ci in c) * (6 * zmax) ** max(len(Si) for Si in S) < 1 << 62:
            break
        seed += 1
    rng = np.random.default_rng(seed)
    m = n - 4                        # rows 2 .. n - 3
    z = np.zeros(n, dtype=np.int64)
    z[:4] = z4
    values = np.array(_ccs_wide._VALUES, dtype=np.int64)
    mats, total = [None] * t, np.zeros(m, dtype=np.int64)
    for Si, ci in zip(S[:-1], c[:-1]):
        prod = np.ones(m, dtype=np.int64)
        for j in Si:
            c1, c2 = rng.integers(0, 4, size=m), rng.integers(0, 4, size=m)
            v1, v2 = values[rng.integers(0, 4, size=m)], values[rng.integers(0, 4, size=m)]
            two = (rng.integers(0, 2, size=m) == 1) & (c1 != c2)  # (a duplicate column: left out instead of merged)
            prod *= v1 * z[c1] + np.where(two, v2 * z[c2], 0)
            cnt = np.concatenate([[len(r) for r in rows4[j]], 1 + two.astype(np.int64), [0, 0]])
            M = _ccs.CsrMatrix.__new__(_ccs.CsrMatrix)
            M.n_rows = M.n_cols = n
            M.row_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
            head_c = [col for r in rows4[j] for _, col in r]
            head_v = [v for r in rows4[j] for v, _ in r]
            body = np.stack([c1, np.where(two, c2, -1)], axis=1).ravel()
            body_v = np.stack([v1, v2], axis=1).ravel()
            M.col_idx = np.concatenate([head_c, body[body >= 0]]).astype(np.uint32)
            M.values = np.concatenate([head_v, body_v[body >= 0]]).astype(np.int64)
            mats[j] = M
        total += ci * prod
    z[4:] = -c[-1] * total
    last = _ccs.CsrMatrix.__new__(_ccs.CsrMatrix)
    last.n_rows = last.n_cols = n
    last.row_ptr = np.minimum(np.arange(n + 1), n - 2).astype(np.uint32)
    last.col_idx = np.arange(2, n, dtype=np.uint32)
    last.values = np.ones(n - 2, dtype=np.int64)
    mats[S[-1][0]] = last
    return _ccs.CcsInstance(n, n, s, s, max(len(Si) for Si in S), mats, [list(Si) for Si in S], c, z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nv", type=int, nargs="?", default=20)
    ap.add_argument("--shapes", nargs="*", default=["plonk6", "t7d3"])
    ap.add_argument("--prove", nargs="*", default=["plonk6"])
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--check", action="store_true", help="compare the Spartan proof with the CPU oracle's (slow)")
    args = ap.parse_args()
    if args.check:
        import _oracle as orc

        orc.build()  # before the first GPU call: a GPU-initialised process must not fork + exec make
    from zinc_amd import cabi, pcs

    fl, s = 4, args.nv
    zf, field = cabi.make_field(STARK, fl), pcs.FieldConfig(STARK, fl)
    R = 1 << (64 * fl)
    insts = {name: big_instance(name, s) for name in dict.fromkeys(args.shapes + args.prove)}
    if s <= 10:
        assert all(_ccs_wide.row_identity_holds(i) for i in insts.values())

    for name in args.shapes:
        inst = insts[name]
        d = cabi.Ccs(inst.matrices, s, zf)
        d.set_z(inst.z)
        rng = np.random.default_rng(1)
        r = rng.integers(0, 1 << 62, size=(s, fl), dtype=np.uint64)  # (canonical: below 2^254 < q)
        r[:, fl - 1] >>= np.uint64(8)
        d.eq_table(r, 0)
        tables = [d.table(cabi.CCS_MZ, k) for k in range(inst.t)] + [d.table(cabi.CCS_EQ, 0)]
        comb = cabi.make_comb(inst.masks, np.array([[(ci % STARK * R % STARK) >> (64 * i) & (2**64 - 1) for i in range(fl)] for ci in inst.c], dtype=np.uint64))
        best = np.full(s, np.inf)
        for rep in range(args.reps + 1):  # the first repetition warms up
            sc = cabi.Sumcheck(tables, s, inst.d + 1, zf, comb=comb)
            times = []
            for i in range(s):
                t0 = time.perf_counter()
                sc.round(None if i == 0 else r[i])
                times.append(time.perf_counter() - t0)
            sc.free()
            if rep:
                best = np.minimum(best, times)
        d.free()
        print(f"{name} 2^{s}: {inst.t + 1} tables, degree {inst.d + 1}; zip_sumcheck_round wall time per round (best of {args.reps}), us:")
        print("   " + " ".join(f"{1e6 * x:.0f}" for x in best) + f"   total {1e3 * best.sum():.2f} ms", flush=True)

    L = pcs.lib()
    for name in args.prove:
        inst = insts[name]
        arr, _keep = pcs.ZincProver._abi_matrices(inst.matrices)
        x, w = inst.z[:1], inst.z[2:]
        masks, cv = inst.masks, np.array(inst.c, dtype=np.int64)
        sp = dict(msgs1=np.zeros((s, inst.d + 2, fl), np.uint64), msgs2=np.zeros((s, 3, fl), np.uint64),
                  V_s=np.zeros((inst.t, fl), np.uint64), r_y=np.zeros((s, fl), np.uint64))
        prep = C.c_void_p()
        assert L.zinc_prover_prepare(arr, inst.t, s, field._m.ctypes.data, fl, 0, C.byref(prep)) == 0, L.zinc_last_error()

        def run(prepared):
            t = pcs.KeccakTranscript()
            h = C.c_void_p()
            t0 = time.perf_counter()
            rc = L.zinc_prover_prove(arr, inst.t, s, inst.d, inst.q, masks.ctypes.data, cv.ctypes.data, x.ctypes.data, x.size,
                                     w.ctypes.data, w.size, t._h, field._m.ctypes.data, fl, 0, prepared, 0, sp["msgs1"].ctypes.data,
                                     sp["msgs2"].ctypes.data, sp["V_s"].ctypes.data, sp["r_y"].ctypes.data, C.byref(h))
            dt = time.perf_counter() - t0
            assert rc == 0, L.zinc_last_error()
            return dt

        for rep in range(args.reps):
            ts, tsp = run(None), run(prep)
            print(f"{name} 2^{s} (stark): SpartanProver::prove {1e3 * ts:8.2f} ms;  with the circuit prepared: {1e3 * tsp:8.2f} ms", flush=True)
        L.zinc_prepared_ccs_free(prep)
        if args.check:
            want = orc.Ccs(inst).spartan_prove(orc.make_field(STARK, fl), orc.new_transcript())
            print("device proof identical to the oracle's:", all(np.array_equal(sp[k], want[k]) for k in sp))


if __name__ == "__main__":
    main()
