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

--prove: the batched prover against a loop of prove_fibsq, per proof.  For
log_t in {7, 10, 13} at blowup 8, with 8 and 32 queries, through the Python
mirror, warm, one process, the median of --reps runs, in microseconds per proof:
  (a) a loop of prove_fibsq (over min(B, 16) members: its cost per proof does
      not depend on B),
  (b) prove_fibsq_batch of B = 16, 64, 256, 1024, 4096 members (--batches),
  (c) the same with device_queries=True: the query phase, the channels' draws
      and sends included, in one fri_batch_query_phase,
each as the whole mirror call (trace on the host, channel hashing in Python
included) and as the time inside its device calls alone; (b)'s device time is
split into the trace commit, the composition commit and the query rounds, and
(c)'s query column is its one query-phase call.  Every member's transcript of
(b) and of (c) is checked against (a)'s for the members (a) ran.

    python tools/batch_probe.py --prove [--reps 7] [--batches 16 64 256] [--out profiles/prove_batch.txt]

--verify: the batched verifier against loops of the host verifier, per proof.
For log_t in {7, 13} at blowup 8, with 8 and 32 queries, B = 16, 64, 256, 4096
transcripts from prove_fibsq_batch (min(B, 256) proved, repeated up to B), warm,
the median of --reps runs, in microseconds per proof:
  (a) fri_verify_batch, the device call with its copies (Context.verify_batch),
      and the same call with FRI_VERIFY_SERIAL=1 (the two kernels on one stream);
  (b) the two kernel classes alone (a profiling context: verify_chain, verify_open);
  (c) packing in the C++ mirror: verify_fibsq_batch's whole call in
      build/verify_native less (a);
against a loop of the C++ verify_fibsq on one core and over 16 threads
(build/verify_native, over min(B, 256) members).

    python tools/batch_probe.py --verify [--reps 5] [--out profiles/verify_batch.txt] [--grinding-bits N]
--grinding-bits N proves with N bits of proof of work and verifies with N bits
(fri_verify_batch_pow, and the host verifiers at the same bits).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
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


PROVE_LOG_T = (7, 10, 13)
PROVE_BATCHES = (16, 64, 256, 1024, 4096)
PROVE_QUERIES = (8, 32)
PROVE_LOG_BLOWUP = 3


class TimedContext:
    """A Context whose device calls of the two provers are timed, by group."""
    GROUPS = {"trace_commit": "trace", "trace_commit_batch": "trace", "fibsq_composition_commit": "comp",
              "fibsq_composition_commit_batch": "comp", "trace_decommit": "query", "decommit_query": "query",
              "batch_decommit_query": "query", "batch_query_round": "query", "batch_query_phase": "query"}

    def __init__(self, ctx):
        self._ctx = ctx
        self.reset()

    def reset(self):
        self.t = {"trace": 0.0, "comp": 0.0, "query": 0.0}

    def __getattr__(self, name):
        fn = getattr(self._ctx, name)
        group = self.GROUPS.get(name)
        if group is None:
            return fn

        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t[group] += time.perf_counter() - t0
        return timed


def prove_mode(args, reps, say):
    lib = fri_amd.load_library()
    lb = PROVE_LOG_BLOWUP
    ctx = TimedContext(fri_amd.Context(0, max(PROVE_LOG_T) + lb))
    say(f"batch_probe --prove: {lib.fri_version().decode()}, blowup {1 << lb}, us per proof, median of {reps} "
        "(warm, one process, Python mirror)")
    say("(a) loop of prove_fibsq  (b) prove_fibsq_batch  (c) prove_fibsq_batch(device_queries=True);")
    say("whole: the mirror call;  device: inside its device calls;")
    say("trace / comp / query: (b)'s device time in fri_trace_commit_batch, fri_fibsq_composition_commit_batch and")
    say("the fri_batch_query_round rounds;  (c) query: its one fri_batch_query_phase call")
    say(f"{'log_t':>5} {'Q':>3} {'B':>4} {'(a) whole':>10} {'(a) device':>10} {'(b) whole':>10} {'(b) device':>10} "
        f"{'trace':>8} {'comp':>8} {'query':>8} {'device (a)/(b)':>14} {'(c) whole':>10} {'(c) device':>10} "
        f"{'(c) query':>10} {'whole (b)/(c)':>13}")
    table = {}
    batches = tuple(args.batches) if args.batches else PROVE_BATCHES

    def measure(fn, per):
        whole, dev, parts = [], [], []
        for _ in range(reps):
            ctx.reset()
            t0 = time.perf_counter()
            fn()
            whole.append((time.perf_counter() - t0) * 1e6 / per)
            dev.append(sum(ctx.t.values()) * 1e6 / per)
            parts.append(tuple(ctx.t[g] * 1e6 / per for g in ("trace", "comp", "query")))
        i = sorted(range(reps), key=lambda j: dev[j])[reps // 2]
        return statistics.median(whole), dev[i], parts[i]

    for log_t in PROVE_LOG_T:
        for Q in PROVE_QUERIES:
            for B in batches:
                a1s = [1000003 * b + 3141592 for b in range(B)]
                m = min(B, 16)
                proofs_a = []

                def loop():
                    proofs_a.clear()
                    for b in range(m):
                        ch = fri_amd.Channel()
                        fri_amd.prove_fibsq(a1s[b], log_t, lb, Q, ch, ctx=ctx)
                        proofs_a.append(ch.proof)

                proofs_b = []

                def batch():
                    chans = [fri_amd.Channel() for _ in a1s]
                    fri_amd.prove_fibsq_batch(a1s, log_t, lb, Q, chans, ctx=ctx)
                    proofs_b[:] = [ch.proof for ch in chans[:m]]

                proofs_c = []

                def batch_dev():
                    chans = [fri_amd.Channel() for _ in a1s]
                    fri_amd.prove_fibsq_batch(a1s, log_t, lb, Q, chans, ctx=ctx, device_queries=True)
                    proofs_c[:] = [ch.proof for ch in chans[:m]]

                loop()
                batch()                               # warm: plans, graphs, the batch's buffers and tables
                batch_dev()                           # ... and the query phase's staging
                assert proofs_a == proofs_b, "batch and loop disagree"
                assert proofs_a == proofs_c, "the device-queries batch and the loop disagree"
                aw, ad, _ = measure(loop, m)
                bw, bd, (tr, co, qu) = measure(batch, B)
                cw, cd, (_, _, cq) = measure(batch_dev, B)
                table[(log_t, Q, B)] = (ad, bd, aw, bw, cw, cd)
                say(f"{log_t:>5} {Q:>3} {B:>4} {aw:>10.1f} {ad:>10.1f} {bw:>10.1f} {bd:>10.1f} {tr:>8.1f} {co:>8.1f} "
                    f"{qu:>8.1f} {ad / bd:>13.1f}x {cw:>10.1f} {cd:>10.1f} {cq:>10.1f} {bw / cw:>12.2f}x")
    say()
    for log_t in PROVE_LOG_T:
        for Q in PROVE_QUERIES:
            if (log_t, Q, 256) in table:
                ad, bd, aw, bw = table[(log_t, Q, 256)][:4]
                say(f"log_t {log_t}, {Q} queries, B = 256: (b) device {bd:.1f} us is "
                    f"{'faster' if bd < ad else 'SLOWER'} than (a) {ad:.1f} us per proof ({ad / bd:.1f}x); "
                    f"whole {bw:.1f} against {aw:.1f} us ({aw / bw:.1f}x)")
            wins = [B for B in batches if table[(log_t, Q, B)][1] < table[(log_t, Q, B)][0]]
            wins_w = [B for B in batches if table[(log_t, Q, B)][3] < table[(log_t, Q, B)][2]]
            say(f"    (b) beats (a) from B = {min(wins) if wins else 'none measured'} (device), "
                f"{min(wins_w) if wins_w else 'none measured'} (whole)")
            # the smallest B from which (c)'s whole call is faster than (b)'s at every larger measured B
            lose = [B for B in batches if not table[(log_t, Q, B)][4] < table[(log_t, Q, B)][3]]
            above = [B for B in batches if not lose or B > max(lose)]
            say(f"log_t {log_t}, {Q} queries: (c) whole beats (b) whole from B = "
                f"{min(above) if above else 'none measured'}; slower at B = {lose if lose else 'none measured'}")
    ctx.close()


VERIFY_SHAPES = ((7, 8), (7, 32), (13, 8), (13, 32))      # (log_t, queries)
VERIFY_BATCHES = (16, 64, 256, 4096)
VERIFY_THREADS = 16


def verify_mode(args, reps, say):
    lib = fri_amd.load_library()
    lb, bits = PROVE_LOG_BLOWUP, args.grinding_bits
    native = os.path.join(ROOT, "stark-prover_amd", "build", "verify_native")
    ctx = fri_amd.Context(0, max(t for t, _ in VERIFY_SHAPES) + lb)
    say(f"batch_probe --verify: {lib.fri_version().decode()}, blowup {1 << lb}, us per proof, median of {reps} "
        f"(warm; transcripts from prove_fibsq_batch; {bits} grinding bits)")
    say("(a) fri_verify_batch with its copies, two streams / FRI_VERIFY_SERIAL=1   (b) kernel classes alone   "
        "(c) packing in the C++ mirror")
    say(f"loop 1 / loop {VERIFY_THREADS}: a loop of the C++ verify_fibsq on one core / over {VERIFY_THREADS} threads;  "
        "min-max: the spread of (a) over the runs")
    say(f"{'log_t':>5} {'Q':>3} {'B':>5} {'(a)':>9} {'(a) min-max':>15} {'(a) serial':>10} {'chain':>9} {'open':>9} "
        f"{'(c) pack':>9} {'whole C++':>9} {'loop 1':>8} {'loop ' + str(VERIFY_THREADS):>8}")
    table = {}
    for log_t, Q in VERIFY_SHAPES:
        L = log_t + lb
        m = 256
        a1s = [1000003 * b + 3141592 for b in range(m)]
        chans = [fri_amd.Channel() for _ in a1s]
        sps = fri_amd.prove_fibsq_batch(a1s, log_t, lb, Q, chans, ctx=ctx, grinding_bits=bits)
        pk = fri_amd.pack_transcripts([ch.proof for ch in chans], L, [sp.fri.n_layers for sp in sps], Q,
                                      (1 << L) - 2 * (1 << lb) - 1, 3, log_t, lb, [sp.a_last for sp in sps],
                                      grinding_bits=bits)
        assert not pk.reasons.any() and not pk.host.any()
        for B in VERIFY_BATCHES:
            rep = -(-B // m)
            cut = lambda a: np.ascontiguousarray(np.concatenate([a] * rep)[:B])   # noqa: E731
            pb = fri_amd.PackedTranscripts(pk.shape, cut(pk.chan), cut(pk.n_layers), cut(pk.a_last), cut(pk.head),
                                           cut(pk.indices), cut(pk.values), cut(pk.paths), cut(pk.reasons), cut(pk.host),
                                           cut(pk.nonces), bits)
            a = pb.abi_args()
            call = lambda: ctx.verify_batch(*a, grinding_bits=bits, nonces=pb.nonces)   # noqa: E731
            assert not call().any(), "the device rejected an honest transcript"
            ts = sorted(med_us(call, 1, B) for _ in range(reps))
            dev, lo, hi = ts[reps // 2], ts[0], ts[-1]
            os.environ["FRI_VERIFY_SERIAL"] = "1"
            call()
            serial = med_us(call, reps, B)
            del os.environ["FRI_VERIFY_SERIAL"]
            ctx.set_profiling(True)
            ctx.reset_profile()
            for _ in range(reps):
                call()
            chain, opn = (ctx.profile(c)[0] * 1e3 / reps / B for c in ("verify_chain", "verify_open"))
            ctx.set_profiling(False)
            out = subprocess.run([native, str(log_t), str(lb), str(Q), str(B), str(reps), str(VERIFY_THREADS),
                                  str(bits)],
                                 capture_output=True, text=True, timeout=1500)
            nat = json.loads(out.stdout.strip().splitlines()[-1])
            assert nat.get("accepted"), out.stdout + out.stderr
            table[(log_t, Q, B)] = (dev, nat["loop_1"], nat["loop_n"], chain, opn, nat["batch_whole"], serial, lo, hi)
            say(f"{log_t:>5} {Q:>3} {B:>5} {dev:>9.2f} {f'{lo:.2f}-{hi:.2f}':>15} {serial:>10.2f} {chain:>9.2f} "
                f"{opn:>9.2f} {nat['batch_whole'] - dev:>9.2f} {nat['batch_whole']:>9.2f} {nat['loop_1']:>8.1f} "
                f"{nat['loop_n']:>8.2f}")
    say()
    for log_t, Q in VERIFY_SHAPES:
        for name, col in (("one core", 1), (f"{VERIFY_THREADS} threads", 2)):
            wins = [B for B in VERIFY_BATCHES if table[(log_t, Q, B)][0] < table[(log_t, Q, B)][col]]
            wins_w = [B for B in VERIFY_BATCHES if table[(log_t, Q, B)][5] < table[(log_t, Q, B)][col]]
            say(f"log_t {log_t}, {Q} queries: the device call beats the loop on {name} from B = "
                f"{min(wins) if wins else 'none measured'}; the whole C++ mirror call from B = "
                f"{min(wins_w) if wins_w else 'none measured'}")
        dev, _, _, chain, opn, _, serial, lo, hi = table[(log_t, Q, 256)]
        say(f"    B = 256: two streams {dev:.2f} us (runs {lo:.2f}-{hi:.2f}), one stream {serial:.2f} us; kernels alone: "
            f"chain {chain:.2f}, open {opn:.2f}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    ap.add_argument("--prove", action="store_true", help="the batched prover against a loop of prove_fibsq")
    ap.add_argument("--batches", type=int, nargs="*", default=None, help="--prove: the batch sizes (default: all)")
    ap.add_argument("--verify", action="store_true", help="the batched verifier against loops of verify_fibsq")
    ap.add_argument("--grinding-bits", type=int, default=0, help="--verify: prove and verify with this many bits")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    if args.verify:
        lines = []

        def say_v(s=""):
            print(s, flush=True)
            lines.append(s)

        verify_mode(args, reps, say_v)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.prove:
        lines = []

        def say_p(s=""):
            print(s, flush=True)
            lines.append(s)

        prove_mode(args, reps, say_p)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
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
