#!/usr/bin/env python3
"""Proof-of-work grinding on the device against the host routes.

In one process, warm, on GPU 0:
  (i)   fri_grind from nonce 0 at 16, 20, 24 and 28 bits over --states distinct
        states each (the work is geometric: a state needs about 2^bits
        nonces): the whole call's time by the host clock (the call ends in a
        synchronise), per state the best of --reps calls, and the nonces it
        had to look at, answer + 1, per second;
  (ii)  the kernel alone: whole windows of 2^28 nonces at 32 bits that hold no
        hit, timed by device events (a profiling context, class "grind");
  (iii) fri_grind_batch of B = 16, 256, 4096 distinct states at 8, 12, 16 and
        20 bits, the whole call, in answer + 1 nonces per second summed over
        the members;
  (iv)  the host routes: the C++ mirror's grind_host on one core and over 16
        threads (build/grind_native) and the Python mirror's hashlib loop;
  (v)   the crossover: the median over 32 states of the whole call of fri_grind
        at 2..16 bits (per state the best of 3, through this mirror) against
        both host routes at the same sizes (one run per state);
  (vi)  the instructions of k_grind's loop per nonce, from its assembly, their
        issue units as DESIGN.md section 5 counts them, and the achieved share
        of the measured VALU ceiling (64 T units/s, bench/valu_cal.hip).
Every answer is checked against the host route where that is affordable
(up to 20 bits).

    python tools/grind_probe.py [--reps 5] [--states 16] [--asm file.s] [--out profiles/grind.txt]
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stark-prover_amd", "python"))
import fri_amd  # noqa: E402

PKG = os.path.join(ROOT, "stark-prover_amd")
HALF_RATE = ("v_alignbit", "v_add3", "v_perm", "v_lshl_or", "v_mul_lo", "v_mul_hi", "v_mad_u64_u32")
VALU_CEILING = 64e12          # units/s, measured by bench/valu_cal.hip
VALU_NOMINAL = 78.6e12        # 256 CU x 128 lane-ops/clk x 2.4 GHz


def state_of(tag, i):
    return hashlib.sha256(b"grind probe %s %d" % (tag.encode(), i)).digest()


def host_grind(state, bits, first=0):
    head = hashlib.sha256(state.hex().encode())
    v = first
    while True:
        h = head.copy()
        h.update(b"%016x" % v)
        if int.from_bytes(h.digest()[:4], "big") >> (32 - bits) == 0:
            return v
        v += 1


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def loop_instructions(asm_path):
    """Instructions of k_grind's depth-1 loop blocks: (all, valu, issue units)."""
    text = open(asm_path).read()
    start = text.index("_ZN3fri7k_grindENS_9GrindTaskE:")
    body = text[start:text.index(".Lfunc_end", start)].split("\n")
    depth, n_all, valu, units = 0, 0, 0, 0
    for line in body:
        s = line.strip()
        if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", s):
            m = re.search(r"Depth=(\d+)", s)
            depth = int(m.group(1)) if m else 0
            continue
        if depth != 1 or not s or s[0] in ";.":
            continue
        op = s.split()[0]
        n_all += 1
        if op.startswith("v_"):
            valu += 1
            units += 2 if op.startswith(HALF_RATE) else 1
    return n_all, valu, units


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states", type=int, default=16)
    ap.add_argument("--asm", default=None, help="assembly of csrc/fri_prover.hip (default: compiled here)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grind.txt"))
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    ctx = fri_amd.Context(0, 12)
    ctx.grind(state_of("warm", 0), 20)
    ctx.grind_batch([state_of("warm", i) for i in range(64)], 12)
    say("# tools/grind_probe.py: fri_grind / fri_grind_batch on one MI355X, warm, one process")
    say(f"# {fri_amd.load_library().fri_version().decode()}; reps {a.reps}, states {a.states}")
    say()

    say("(i) fri_grind from nonce 0, the whole call (host clock; launches, read-back and copies included)")
    say("    per state the best of reps calls (one call at 28 bits); median, min and max over the states")
    say("  bits  states  median ms   min ms   max ms   nonces looked at   M nonces/s (sum / sum)")
    for bits in (16, 20, 24, 28):
        ts, need = [], 0
        for i in range(a.states):
            st = state_of("single%d" % bits, i)
            best = None
            for _ in range(a.reps if bits <= 24 else 1):
                (nonce, _after), t = timed(lambda: ctx.grind(st, bits))
                best = t if best is None else min(best, t)
            if bits <= 20:
                assert nonce == host_grind(st, bits), (bits, i)
            ts.append(best)
            need += nonce + 1
        say(f"  {bits:4d}  {a.states:6d}  {statistics.median(ts) * 1e3:9.3f}  {min(ts) * 1e3:7.3f}  {max(ts) * 1e3:7.3f}"
            f"  {need:17d}  {need / sum(ts) / 1e6:12.1f}")
    say()

    say("(ii) the kernel alone: windows of 2^28 nonces at 32 bits without a hit (device events, class \"grind\")")
    prof = fri_amd.Context(0, 12)
    prof.set_profiling(True)
    prof.set_grind_window(28)
    prof.grind(state_of("warm", 1), 32, 0, (1 << 28) - 1)
    prof.reset_profile()
    rates = []
    for i in range(8):
        prof.reset_profile()
        if prof.grind(state_of("raw", i), 32, 0, (1 << 28) - 1) is None:
            ms, launches, _ = prof.profile("grind")
            assert launches == 1
            rates.append((1 << 28) / (ms * 1e-3))
            say(f"  state {i}: {ms:8.3f} ms  {rates[-1] / 1e9:7.2f} G nonces/s")
    prof.close()
    raw = statistics.median(rates)
    say(f"  median {raw / 1e9:.2f} G nonces/s; 2^28 nonces take {(1 << 28) / raw * 1e3:.1f} ms")
    say()

    say("(iii) fri_grind_batch from nonce 0, the whole call, median of reps")
    say("      B  bits    call ms   nonces looked at   M nonces/s   us per member")
    for B in (16, 256, 4096):
        for bits in (8, 12, 16, 20):
            sts = [state_of("batch%d" % bits, i) for i in range(B)]
            ts = []
            for _ in range(a.reps if bits < 20 else 2):
                got, t = timed(lambda: ctx.grind_batch(sts, bits))
                ts.append(t)
            need = sum(g[0] + 1 for g in got)
            if bits <= 12:
                assert all(g[0] == host_grind(st, bits) for g, st in zip(got[:64], sts))
            t = statistics.median(ts)
            say(f"  {B:5d}  {bits:4d}  {t * 1e3:9.3f}  {need:17d}  {need / t / 1e6:11.1f}  {t * 1e6 / B:14.2f}")
    say()

    say("(iv) the host routes")
    native = os.path.join(PKG, "build", "grind_native")
    sweep = list(range(2, 17, 2))
    nat = json.loads(subprocess.run([native, "22", "3", "16"] + [str(b) for b in sweep], capture_output=True, text=True,
                                    check=True, timeout=600).stdout)
    say(f"  C++ mirror grind_host (SHA extensions: {nat['sha_accelerated']}): {nat['rate_1'] / 1e6:.2f} M nonces/s on one core, "
        f"{nat['rate_n'] / 1e6:.1f} M nonces/s over {nat['threads']} threads")
    answers, t = timed(lambda: [host_grind(state_of("py", i), 14) for i in range(8)])
    n_py = sum(v + 1 for v in answers)
    say(f"  Python mirror (hashlib loop): {n_py / t / 1e6:.2f} M nonces/s on one core")
    say()

    say("(v) the crossover: median whole call over 32 states, microseconds")
    say("    per state the device call is the best of 3 (through the Python mirror: ctypes included, a C caller pays less),")
    say("    each host loop one run; the medians are over the states")
    say("  bits   fri_grind (Python call)   C++ grind_host   Python hashlib loop")
    cross = {"cpp": None, "py": None}
    for bits in sweep:
        dev, py = [], []
        for i in range(32):
            st = state_of("cross%d" % bits, i)
            dev.append(min(timed(lambda: ctx.grind(st, bits))[1] for _ in range(3)))
            py.append(timed(lambda: host_grind(st, bits))[1])
        d, p, c = statistics.median(dev) * 1e6, statistics.median(py) * 1e6, nat["grind_us"][str(bits)]
        say(f"  {bits:4d}   {d:23.1f}   {c:14.1f}   {p:19.1f}")
        for key, host in (("cpp", c), ("py", p)):
            if d < host and cross[key] is None:
                cross[key] = bits
            elif d >= host:
                cross[key] = None
    say(f"  the device call is faster from {cross['cpp']} bits up than the C++ host route and from {cross['py']} bits up "
        f"than the Python one (the smallest measured sizes from which it wins at every larger one)")
    say()

    say("(vi) k_grind's loop, per nonce (one row of 64 nonces per pass)")
    asm = a.asm
    if asm is None:
        asm = os.path.join(tempfile.mkdtemp(), "fri_prover.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", asm, os.path.join(PKG, "csrc", "fri_prover.hip")], check=True)
    n_all, valu, units = loop_instructions(asm)
    say(f"  {n_all} instructions, {valu} of them VALU = {units} issue units (half rate counts twice; DESIGN.md section 5: "
        f"a leaf hash is 1288 instructions = 2009 units)")
    say(f"  {raw / 1e9:.2f} G nonces/s x {units} units = {raw * units / 1e12:.1f} T units/s: "
        f"{100 * raw * units / VALU_NOMINAL:.0f}% of the nominal 78.6 T, {100 * raw * units / VALU_CEILING:.0f}% of the measured "
        f"64 T ceiling (the layer-0 leaf kernel: 60.4 T, 94%)")
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
