#!/usr/bin/env python3
"""Wall time of a device sumcheck with the tables resident in HBM, two legs in one process on the same tables, alternating:

  per-round  nv calls of zip_sumcheck_round, the caller stepping the host mirror's KeccakTranscript between them as
             prove_as_subprotocol does (absorb the message, get_challenge, absorb the challenge); the framing is built
             in Python here, a few microseconds per round on top of what a C++ or Rust caller pays
  no-keccak  the same calls with a fixed challenge and no transcript at all: a lower bound for the per-round path
  one-call   zip_sumcheck_prove: the same rounds, the transcript included (host-stepped above the tail, on the device
             in the tail kernel)

usage: sumcheck_times.py [--ccs] [--reps N] [nv ...]     product shape (K = 2, degree 2) or CCS shape (K = 4, degree 3)
ZIP_HIP_SUMCHECK_TAIL=n moves the tail bound (README.md); nv = the bound times the tail kernel alone.
At nv <= 22 the product shape also goes through the host mirror (tables uploaded from the host) with
ZIP_HIP_SUMCHECK_ONECALL=0 and =1."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from zinc_amd import cabi, pcs  # noqa: E402
import torch  # noqa: E402

args = sys.argv[1:]
ccs = "--ccs" in args
reps = 11
if "--reps" in args:
    at = args.index("--reps")
    if at + 1 >= len(args):
        sys.exit("--reps needs a number")
    reps = int(args[at + 1])
    del args[at:at + 2]
nvs = [int(a) for a in args if not a.startswith("--")] or [20, 24]
fl = 4
K, degree = (4, 3) if ccs else (2, 2)
zf = cabi.make_field(bench.BENCH_MODULUS, fl)
comb = None
if ccs:
    R = 1 << (64 * fl)
    q = bench.BENCH_MODULUS
    c = [[(v >> (64 * i)) & (2**64 - 1) for i in range(fl)] for v in (R % q, (q - 1) * R % q)]
    comb = cabi.make_comb([0b011, 0b100], c)

for nv in nvs:
    n = 1 << nv
    rng = np.random.default_rng(1)
    mles = rng.integers(0, 1 << 62, size=(K, n, fl), dtype=np.uint64)
    mles[..., fl - 1] >>= np.uint64(6)
    dev = [torch.from_numpy(mles[k].view(np.int64)).cuda() for k in range(K)]
    r = np.array([3, 1, 4, 1], dtype=np.uint64)
    field = pcs.FieldConfig(bench.BENCH_MODULUS, fl)
    mod_be = bench.BENCH_MODULUS.to_bytes(8 * fl, "big")

    def framed(v):  # absorb_random_field: 0x3 | modulus BE | 0x5 | 0x1 | value BE | 0x3
        return b"\x03" + mod_be + b"\x05\x01" + v[::-1].byteswap().tobytes() + b"\x03"

    per_round, no_keccak, one_call, last = [], [], [], 0.0
    for rep in range(reps + 2):  # two warm-up rounds of the three legs
        sc = cabi.Sumcheck(dev, nv, degree, zf, comb=comb)
        t = pcs.KeccakTranscript()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ch = None
        for i in range(nv):
            ev = sc.round(ch)
            t.absorb(b"".join(framed(e) for e in ev))
            ch = t.get_challenge(field)
            t.absorb(framed(ch))
        dt_k = time.perf_counter() - t0
        sc.free()
        sc = cabi.Sumcheck(dev, nv, degree, zf, comb=comb)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(nv):
            t1 = time.perf_counter()
            sc.round(None if i == 0 else r)
            last = time.perf_counter() - t1
        dt_a = time.perf_counter() - t0
        sc.free()
        sc = cabi.Sumcheck(dev, nv, degree, zf, comb=comb)
        state = cabi.KeccakState.make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.prove(state)
        dt_b = time.perf_counter() - t0
        sc.free()
        if rep >= 2:
            per_round.append(dt_k)
            no_keccak.append(dt_a)
            one_call.append(dt_b)
    med_k, med_a, med_b = statistics.median(per_round), statistics.median(no_keccak), statistics.median(one_call)
    shape = f"{'ccs' if ccs else 'product'} K={K} degree={degree}"
    print(f"2^{nv} {shape}: per-round with Keccak {med_k * 1e3:.3f} ms [{min(per_round) * 1e3:.3f} .. {max(per_round) * 1e3:.3f}]; "
          f"no-keccak {med_a * 1e3:.3f} ms [{min(no_keccak) * 1e3:.3f} .. {max(no_keccak) * 1e3:.3f}], last round {last * 1e6:.0f} us; "
          f"one-call {med_b * 1e3:.3f} ms [{min(one_call) * 1e3:.3f} .. {max(one_call) * 1e3:.3f}]; medians of {reps}, "
          f"TAIL={os.environ.get('ZIP_HIP_SUMCHECK_TAIL', 'default')}", flush=True)
    if nv <= 22 and not ccs:
        legs = {"0": [], "1": []}
        for rep in range(reps + 1):
            for leg in legs:
                os.environ["ZIP_HIP_SUMCHECK_ONECALL"] = leg
                t = pcs.KeccakTranscript()
                t0 = time.perf_counter()
                pcs.sumcheck_prove_product(t, mles, degree, field)
                if rep:
                    legs[leg].append(time.perf_counter() - t0)
        os.environ.pop("ZIP_HIP_SUMCHECK_ONECALL", None)
        print(f"2^{nv}: prove_as_subprotocol through the host mirror (tables uploaded from the host): per-round loop, Keccak on the "
              f"host {statistics.median(legs['0']) * 1e3:.3f} ms; one call {statistics.median(legs['1']) * 1e3:.3f} ms", flush=True)
