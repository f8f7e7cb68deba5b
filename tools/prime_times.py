#!/usr/bin/env python3
"""get_prime on the device against its CPU restatement (profiles/prime_gen.md).  Per FIELD_LIMBS 2 / 3 / 4 over the
twelve transcripts of tests/test_gpu_prime.py (fresh, and bytes([k]) * k absorbed for k = 1 .. 11):

  - warm zip_get_prime wall time (median of --reps runs) at every batch width of --widths, and the candidates tried;
  - the CPU restatement: the same lane function (zinc_amd/csrc/prime_dev.cuh) compiled for the host with g++ -O2, in
    the reference's sequential loop on one core, on the same transcripts;
  - with --kernel-trace: the kernel's own time, from a child of this script run under rocprofv3 --kernel-trace --stats
    at the default width (one zip_get_prime per transcript and FL).
GPU box.  Every prime and count is checked against the CPU restatement's."""
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
FLS = (2, 3, 4)


def sponge(k):
    """(st, pending) of a transcript that absorbed bytes([k]) * k, from the host mirror"""
    from zinc_amd import pcs

    t = pcs.KeccakTranscript()
    if k:
        t.absorb(bytes([k]) * k)
    return t.state()


def build_host_restatement(out_dir):
    """prime_dev.cuh for the host: g++ -O2 over tests/native/prime_dev_check.cpp, the one host wrapper of that header
    (the tests build the same file at -O1).  Nothing else of tests/ is used: no oracle, no test helper."""
    so = os.path.join(out_dir, "libprime_dev_check.so")
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{os.path.join(ROOT, 'zinc_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "native", "prime_dev_check.cpp"), "-o", so]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(so)
    lib.pd_get_prime.restype = C.c_uint32
    return lib


def cpu_get_prime(pd, st, pending, fl):
    st = np.array(st, np.uint64)
    buf = np.zeros(136, np.uint8)
    buf[: len(pending)] = np.frombuffer(pending, np.uint8)
    n = C.c_uint32(len(pending))
    out = np.zeros(fl, np.uint64)
    t0 = time.perf_counter()
    tried = pd.pd_get_prime(fl, C.c_void_p(st.ctypes.data), C.c_void_p(buf.ctypes.data), C.byref(n), C.c_void_p(out.ctypes.data), 65536)
    dt = time.perf_counter() - t0
    return dt, tried, sum(int(w) << (64 * i) for i, w in enumerate(out))


def worker():
    """one zip_get_prime per transcript and FL at the default width (the traced child)"""
    from zinc_amd import cabi

    for fl in FLS:
        for k in range(12):
            st, pending = sponge(k)
            cabi.get_prime(cabi.KeccakState.make(st, pending), fl)


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
                    if "prime_test_base2_kernel" in row["Name"]:
                        print(f"kernel {row['Name'].split('(')[0]:50s} launches {row['Calls']:>4s}  avg {float(row['AverageNs']) / 1e3:8.1f} us"
                              f"  min {float(row['MinNs']) / 1e3:8.1f}  max {float(row['MaxNs']) / 1e3:8.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--widths", default="64,128,256,512,1024")
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker()
    if args.kernel_trace:  # first: the child is started before this process makes its first HIP call
        kernel_trace()
    with tempfile.TemporaryDirectory() as d:
        pd = build_host_restatement(d)  # before the first HIP call: a GPU-initialised process must not fork
        from zinc_amd import cabi

        widths = [int(w) for w in args.widths.split(",")]
        total = {}
        for fl in FLS:
            cpu, tried, want = [], [], []
            for k in range(12):
                st, pending = sponge(k)
                runs = [cpu_get_prime(pd, st, pending, fl) for _ in range(max(3, args.reps // 3))]
                cpu.append(statistics.median(r[0] for r in runs))
                tried.append(runs[0][1])
                want.append(runs[0][2])
            print(f"FL {fl}: candidates tried {tried}")
            print(f"FL {fl}: CPU restatement, one core, us  {[round(1e6 * t) for t in cpu]}  median {1e6 * statistics.median(cpu):.0f}  sum {1e6 * sum(cpu):.0f}")
            for w in widths:
                os.environ["ZIP_HIP_PRIME_BATCH"] = str(w)
                dev = []
                for k in range(12):
                    st, pending = sponge(k)
                    ts = []
                    for rep in range(args.reps + 1):
                        state = cabi.KeccakState.make(st, pending)
                        t0 = time.perf_counter()
                        got = cabi.get_prime(state, fl)
                        if rep:
                            ts.append(time.perf_counter() - t0)
                        assert got == (want[k], tried[k]), (fl, k, w)
                    dev.append(statistics.median(ts))
                total[fl, w] = (statistics.median(dev), sum(dev))
                print(f"FL {fl}: device, width {w:4d}, us      {[round(1e6 * t) for t in dev]}  median {1e6 * statistics.median(dev):.0f}  sum {1e6 * sum(dev):.0f}"
                      f"  CPU/device over the twelve {sum(cpu) / sum(dev):.1f}x")
            os.environ.pop("ZIP_HIP_PRIME_BATCH", None)
        for w in widths:
            print(f"width {w:4d}: median over the twelve, us: " + "  ".join(f"FL {fl} {1e6 * total[fl, w][0]:.0f}" for fl in FLS)
                  + f"   all 36: {1e6 * sum(total[fl, w][1] for fl in FLS):.0f}")


if __name__ == "__main__":
    main()
