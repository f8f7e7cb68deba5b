#!/usr/bin/env python3
"""zip_get_prime_batch against the loop of zip_get_prime (profiles/prime_batch.md).  Per FIELD_LIMBS 2 / 3 / 4 and per
n = 2, 4, 16, 64, 256 members -- member i a fresh transcript that absorbed the public input [i] -- warm medians of three legs:

  - the batch call (one zip_get_prime_batch at the default window);
  - the loop of zip_get_prime over the same transcripts: the comparison, with its own run-to-run spread (max - min of the
    warm runs);
  - the CPU restatement: the lane function and the chain of zinc_amd/csrc/prime_dev.cuh compiled for the host with g++ -O2,
    the reference's sequential loop on one core, as tools/prime_times.py does it.
Every prime and count of the batch is checked against the loop's, and the loop's against the CPU restatement's.
Then the window: w = 16, 32, 64, 128 at n = 16 and n = 256.  With --kernel-trace: the three kernels' own times, from a
child of this script run under rocprofv3 --kernel-trace --stats (one batch call of 256 members per limb count).  GPU box."""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FLS = (2, 3, 4)
SIZES = (2, 4, 16, 64, 256)
WINDOWS = (16, 32, 64, 128)


def sponges(n):
    """(st, pending) of n fresh transcripts, member i having absorbed the 8 little-endian bytes of i"""
    from zinc_amd import pcs

    out = []
    for i in range(n):
        t = pcs.KeccakTranscript()
        t.absorb(int(i).to_bytes(8, "little"))
        out.append(t.state())
    return out


def state_array(cabi, members):
    arr = (cabi.KeccakState * len(members))()
    for i, (st, pending) in enumerate(members):
        k = cabi.KeccakState.make(st, pending)
        C.memmove(C.byref(arr[i]), C.byref(k), C.sizeof(cabi.KeccakState))
    return arr


def run_batch(cabi, fresh, n, fl):
    arr = (cabi.KeccakState * n)()
    C.memmove(arr, fresh, C.sizeof(arr))
    primes, tried = np.zeros((n, fl), np.uint64), np.zeros(n, np.uint32)
    t0 = time.perf_counter()
    rc = cabi.lib().zip_get_prime_batch(0, arr, n, fl, primes.ctypes.data, tried.ctypes.data_as(C.POINTER(C.c_uint32)))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt, primes, tried


def run_loop(cabi, fresh, n, fl):
    arr = (cabi.KeccakState * n)()
    C.memmove(arr, fresh, C.sizeof(arr))
    primes, tried = np.zeros((n, fl), np.uint64), np.zeros(n, np.uint32)
    L = cabi.lib()
    args = [(C.byref(arr[i]), primes[i].ctypes.data, C.cast(tried.ctypes.data + 4 * i, C.POINTER(C.c_uint32))) for i in range(n)]
    t0 = time.perf_counter()
    for state, prime, count in args:
        rc = L.zip_get_prime(0, state, fl, prime, count)
        assert rc == 0, rc
    dt = time.perf_counter() - t0
    return dt, primes, tried


def worker():
    """one batch call of 256 members per limb count at the default window (the traced child)"""
    from zinc_amd import cabi

    fresh = state_array(cabi, sponges(256))
    for fl in FLS:
        run_batch(cabi, fresh, 256, fl)


def kernel_trace():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--worker"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            print("rocprofv3 failed:", r.stderr[-2000:])
            return
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    if "prime_" in row["Name"]:
                        print(f"kernel {row['Name'].split('(')[0]:50s} launches {row['Calls']:>4s}  avg {float(row['AverageNs']) / 1e3:8.1f} us"
                              f"  min {float(row['MinNs']) / 1e3:8.1f}  max {float(row['MaxNs']) / 1e3:8.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement leg")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker()
    if args.kernel_trace:  # first: the child is started before this process makes its first HIP call
        kernel_trace()
    import prime_times

    with tempfile.TemporaryDirectory() as d:
        pd = None if args.no_cpu else prime_times.build_host_restatement(d)  # before the first HIP call
        from zinc_amd import cabi

        os.environ.pop("ZIP_HIP_PRIME_BATCH_WINDOW", None)
        os.environ.pop("ZIP_HIP_PRIME_BATCH", None)
        members = sponges(max(SIZES))
        us = lambda t: f"{1e6 * t:9.0f}"  # noqa: E731
        for fl in FLS:
            for n in SIZES:
                fresh = state_array(cabi, members[:n])
                batch, loop = [], []
                for rep in range(args.reps + 1):  # alternated; the first pair warms up
                    b, l = run_batch(cabi, fresh, n, fl), run_loop(cabi, fresh, n, fl)
                    assert np.array_equal(b[1], l[1]) and np.array_equal(b[2], l[2]), (fl, n)
                    if rep:
                        batch.append(b[0])
                        loop.append(l[0])
                cpu = "not measured"
                if pd is not None:
                    runs = []
                    for _ in range(3 if n <= 16 else 1):
                        total = 0.0
                        for i in range(n):
                            dt, tried, prime = prime_times.cpu_get_prime(pd, members[i][0], members[i][1], fl)
                            assert tried == int(l[2][i]) and prime == sum(int(w) << (64 * k) for k, w in enumerate(l[1][i])), (fl, n, i)
                            total += dt
                        runs.append(total)
                    cpu = us(statistics.median(runs))
                mb, ml, spread = statistics.median(batch), statistics.median(loop), max(loop) - min(loop)
                print(f"FL {fl} n {n:3d}: longest chain {int(l[2].max()):4d}  batch {us(mb)} us (min {us(min(batch))} max {us(max(batch))})"
                      f"  loop {us(ml)} us (min {us(min(loop))} max {us(max(loop))} spread {us(spread)})  CPU {cpu} us"
                      f"  loop/batch {ml / mb:5.2f}x  {'WINS' if ml - mb > spread else 'no win'}", flush=True)
        total = {w: 0.0 for w in WINDOWS}
        for fl in FLS:
            for n in (16, 256):
                fresh = state_array(cabi, members[:n])
                for w in WINDOWS:
                    os.environ["ZIP_HIP_PRIME_BATCH_WINDOW"] = str(w)
                    ts = [run_batch(cabi, fresh, n, fl)[0] for _ in range(args.reps + 1)][1:]
                    total[w] += statistics.median(ts)
                    print(f"FL {fl} n {n:3d} window {w:4d}: batch {us(statistics.median(ts))} us", flush=True)
        os.environ.pop("ZIP_HIP_PRIME_BATCH_WINDOW", None)
        for w in WINDOWS:
            print(f"window {w:4d}: sum of the six medians {us(total[w])} us", flush=True)


if __name__ == "__main__":
    main()
