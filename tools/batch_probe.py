#!/usr/bin/env python3
"""Batched commit against what callers can do today, per commit.

For log_n in {8, 10, 12, 14, 16, 18} at blowup 8 and B in {1, 16, 64, 256,
1024} members (B * footprint under about 8 GiB: 8.6 still runs), in one
process, warm, the median of --reps runs, in microseconds per commit:
  (a) a loop of fri_commit_device,
  (b) fri_commit_device_async with three commits pending,
  (c) fri_commit_batch_device of all B members in one call,
and, apart, the batch's first call (buffers and tables allocated).
(a) and (b) cost the same per commit whatever B is, so they run over
min(B, 64) of the members.  Every member has its own random coefficients on
the device; (c)'s roots are checked against (a)'s for the members (a) ran.

    python tools/batch_probe.py [--reps 7] [--out profiles/commit_batch.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stark-prover_amd", "python"))
import fri_amd  # noqa: E402

LOGS = (8, 10, 12, 14, 16, 18)
BATCHES = (1, 16, 64, 256, 1024)
LIMIT = 9 << 30       # "about 8 GiB": 256 members at 2^18 and 1024 at 2^16 take 8.6 GiB


def footprint(log_n, d):
    """Bytes of HBM per member (fri_amd.h: layers, trees, two coefficient buffers, the transform's input)."""
    R = min(max(d - 1, 0).bit_length(), log_n)
    lay = 4 * ((2 << log_n) - (1 << (log_n - R)))
    tre = 32 * sum((2 << (log_n - k)) - 1 for k in range(R + 1))
    return lay + tre + 2 * 4 * (d // 2 + 1) + (4 * d if log_n > fri_amd.BATCH_LDE_LDS_MAX_LOG_N else 0)


def med_us(fn, reps, per):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6 / per)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    args = ap.parse_args()
    reps = max(args.reps, 5)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = fri_amd.load_library()
    ctx = fri_amd.Context(0, max(max(args.logs), 12))
    ch = fri_amd.ChannelState()
    say(f"batch_probe: {lib.fri_version().decode()}, blowup 8, us per commit, median of {reps} (warm, one process)")
    say("(a) loop of fri_commit_device  (b) fri_commit_device_async, 3 pending  (c) fri_commit_batch_device")
    say(f"{'log_n':>5} {'B':>5} {'MiB/member':>10} {'(a)':>9} {'(b)':>9} {'(c)':>9} {'(c) first call [ms]':>20}")
    table = {}
    for log_n in args.logs:
        d = (1 << log_n) // 8
        fp = footprint(log_n, d)
        for B in BATCHES:
            if B * fp > LIMIT:
                say(f"{log_n:>5} {B:>5} {fp / 2**20:>10.2f}   (skipped: {B * fp / 2**30:.1f} GiB)")
                continue
            rng = np.random.default_rng(1000 * log_n + B)
            host = rng.integers(0, fri_amd.P, B * d, dtype=np.uint64).astype(np.uint32)
            dev = fri_amd.DeviceBuffer(host)
            base = dev.data_ptr()
            m = min(B, 64)
            res1 = fri_amd.CommitResult()
            roots_a = []

            def loop():
                roots_a.clear()
                for b in range(m):
                    rc = lib.fri_commit_device(ctx.h, base + 4 * b * d, d, log_n, 5, ctypes.byref(ch), 0, None,
                                               ctypes.byref(res1))
                    assert rc == 0, rc
                    roots_a.append(bytes(res1.roots[0]))

            def piped():
                pend = []
                t = ctypes.c_uint64()
                for b in range(m):
                    if len(pend) == 3:
                        assert lib.fri_commit_wait(ctx.h, pend.pop(0), ctypes.byref(res1)) == 0
                    rc = lib.fri_commit_device_async(ctx.h, base + 4 * b * d, d, log_n, 5, ctypes.byref(ch), 0, None,
                                                     ctypes.byref(t))
                    assert rc == 0, rc
                    pend.append(t.value)
                for tk in pend:
                    assert lib.fri_commit_wait(ctx.h, tk, ctypes.byref(res1)) == 0

            resb = (fri_amd.CommitResult * B)()
            status = (ctypes.c_int * B)()

            def batch():
                rc = lib.fri_commit_batch_device(ctx.h, base, d, B, log_n, 5, None, 0, None, resb, status)
                assert rc == 0, rc

            loop()
            piped()                                   # warm: plans, graphs, lanes
            a = med_us(loop, reps, m)
            b_ = med_us(piped, reps, m)
            t0 = time.perf_counter()
            batch()
            first_ms = (time.perf_counter() - t0) * 1e3
            c = med_us(batch, reps, B)
            assert [bytes(resb[i].roots[0]) for i in range(m)] == roots_a, "batch and loop disagree"
            table[(log_n, B)] = (a, b_, c)
            say(f"{log_n:>5} {B:>5} {fp / 2**20:>10.2f} {a:>9.1f} {b_:>9.1f} {c:>9.1f} {first_ms:>20.2f}")
            del dev
    say()
    cap = None
    for log_n in args.logs:
        if (log_n, 256) in table:
            a, b_, c = table[(log_n, 256)]
            verdict = "faster" if c < b_ else "SLOWER"
            say(f"2^{log_n}, B = 256: (c) {c:.1f} us is {verdict} than (b) {b_:.1f} us per commit ({b_ / c:.1f}x)")
            if 14 <= log_n <= 18 and c < b_:
                cap = log_n
    for log_n in args.logs:
        wins = [B for B in BATCHES if (log_n, B) in table and table[(log_n, B)][2] < table[(log_n, B)][0]]
        say(f"2^{log_n}: (c) beats (a) from B = {min(wins) if wins else 'none measured'}")
    say(f"largest measured log_n in 14..18 where (c) beats (b) at B = 256: {cap}")
    say(f"FRI_BATCH_MAX_LOG_N in this build: {fri_amd.BATCH_MAX_LOG_N}")
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
