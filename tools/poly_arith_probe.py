"""fri_poly_mul / fri_poly_div_rem / fri_poly_compose timings on the GPU
(no device: the context creation fails and so does this tool).

 (i)  the crossover behind FRI_POLY_DIRECT_MAX: fri_poly_mul under
      FRI_POLY_FORCE_DIRECT and FRI_POLY_FORCE_NTT, alternating, short operand
      1, 2, 4, ..., FRI_POLY_DIRECT_LIMIT against long operands of 2^10, 2^16
      and 2^20 coefficients;
 (ii) mul, div_rem and compose at a few sizes, beside the C oracle's
      schoolbook (the reference's algorithm, one thread) where that takes
      seconds, not minutes, and beside the sum of two fri_lde and one
      fri_interpolate at the product's transform size (the same three
      transforms through existing entry points).

 (iii) with --roots FILE, instead of (i) and (ii): fri_poly_from_roots for
      every candidate leaf size (fri_debug_set_roots_leaf) at 2^10, 2^14, 2^16
      and 2^20 roots, beside the C oracle's orc_poly_from_roots up to 2^14 and
      beside 2^10 successive fri_poly_mul by a linear factor (the only device
      route before fri_poly_from_roots); and fri_lagrange_basis at n = 256,
      1024 and 4096, beside the device-to-host copy of its n^2 words alone.
      This is the table behind FRI_ROOTS_LEAF (profiles/poly_roots.txt).


 (iv) with --multipoint FILE, instead of the above: fri_evaluate_ex with
      d = count = 2^10 .. 2^20 and fri_interpolate_points_ex with n = 2^10 ..
      2^20 under FRI_MP_FORCE_DIRECT (as far as the quadratic kernels finish
      in reasonable time, resp. are accepted) and FRI_MP_FORCE_TREE,
      alternating, each table twice; and both tree calls at 2^16 for every
      candidate leaf size.  These are the tables behind FRI_MP_EVAL_MIN and
      FRI_MP_INTERP_MIN (profiles/poly_multipoint.txt).

Every figure is the median of REPS synchronous C-ABI calls after WARM
warm-ups, host clock around the call (uploads and read-back included).
Shapes are seeded.
Usage: poly_arith_probe.py [--out FILE | --roots FILE | --multipoint FILE]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stark-prover_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fri_amd  # noqa: E402
import fri_oracle as fo  # noqa: E402

P = fri_amd.P
WARM, REPS = 3, 11
LOG_MAX = 22
_lines = []


def say(s=""):
    print(s, flush=True)
    _lines.append(s)


def coeffs(seed, n):
    a = fo.splitmix64_np(seed, n)
    if n and a[-1] == 0:
        a[-1] = 1
    return np.ascontiguousarray(a.astype(np.uint32))


def median_ms(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def mul_call(ctx, a, b, flags):
    out = np.empty(a.size + b.size, dtype=np.uint32)
    ln = ctypes.c_size_t()
    pa, pb, po = fri_amd._ptr(a), fri_amd._ptr(b), fri_amd._ptr(out)

    def call():
        rc = ctx.lib.fri_poly_mul(ctx.h, pa, a.size, pb, b.size, flags, po, out.size, ctypes.byref(ln))
        assert rc == 0, ctx.lib.fri_last_error(ctx.h)
    return call


def div_call(ctx, a, b):
    q = np.empty(a.size, dtype=np.uint32)
    r = np.empty(max(a.size, b.size), dtype=np.uint32)
    lq, lr = ctypes.c_size_t(), ctypes.c_size_t()
    pa, pb, pq, pr = (fri_amd._ptr(v) for v in (a, b, q, r))

    def call():
        rc = ctx.lib.fri_poly_div_rem(ctx.h, pa, a.size, pb, b.size, pq, q.size, ctypes.byref(lq), pr, r.size,
                                      ctypes.byref(lr))
        assert rc == 0, ctx.lib.fri_last_error(ctx.h)
    return call


def transforms_ms(ctx, la, lb):
    """Two fri_lde and one fri_interpolate at N = next_pow2(la + lb - 1)."""
    log_n = max(0, (la + lb - 2).bit_length())
    a, b, ys = coeffs(1, la), coeffs(2, lb), coeffs(3, 1 << log_n)
    ev = np.empty(1 << log_n, dtype=np.uint32)
    ln = ctypes.c_size_t()
    pa, pb, py, pe = (fri_amd._ptr(v) for v in (a, b, ys, ev))

    def call():
        assert ctx.lib.fri_lde(ctx.h, pa, la, log_n, 1, pe) == 0
        assert ctx.lib.fri_lde(ctx.h, pb, lb, log_n, 1, pe) == 0
        assert ctx.lib.fri_interpolate(ctx.h, py, log_n, 1, pe, ctypes.byref(ln)) == 0
    return median_ms(call), log_n


def oracle_s(corc, kind, a, b):
    """One run of the C oracle's schoolbook mul / div_rem (one thread), seconds."""
    p64 = ctypes.POINTER(ctypes.c_uint64)
    a64, b64 = np.ascontiguousarray(a.astype(np.uint64)), np.ascontiguousarray(b.astype(np.uint64))
    o1 = np.zeros(a.size + b.size, dtype=np.uint64)
    o2 = np.zeros(a.size + b.size, dtype=np.uint64)
    t0 = time.perf_counter()
    if kind == "mul":
        corc.orc_poly_mul(a64.ctypes.data_as(p64), a.size, b64.ctypes.data_as(p64), b.size, o1.ctypes.data_as(p64), P)
    else:
        lq, lr = ctypes.c_size_t(), ctypes.c_size_t()
        corc.orc_poly_div_rem(a64.ctypes.data_as(p64), a.size, b64.ctypes.data_as(p64), b.size,
                              o1.ctypes.data_as(p64), ctypes.byref(lq), o2.ctypes.data_as(p64), ctypes.byref(lr), P)
    return time.perf_counter() - t0


def crossover(ctx):
    say("(i) fri_poly_mul, direct kernel vs NTT path [ms, median of %d]; long operand 2^10 / 2^16 / 2^20" % REPS)
    say("%8s  %10s %10s   %10s %10s   %10s %10s" % ("short", "direct", "ntt", "direct", "ntt", "direct", "ntt"))
    best = {}
    ls = 1
    while ls <= fri_amd.POLY_DIRECT_LIMIT:
        row = "%8d " % ls
        for log_l in (10, 16, 20):
            a, b = coeffs(100 + log_l, 1 << log_l), coeffs(200 + ls, ls)
            fd, fn = mul_call(ctx, a, b, fri_amd.POLY_FORCE_DIRECT), mul_call(ctx, a, b, fri_amd.POLY_FORCE_NTT)
            for _ in range(WARM):
                fd()
                fn()
            td, tn = [], []
            for _ in range(REPS):                                   # alternating
                t0 = time.perf_counter()
                fd()
                t1 = time.perf_counter()
                fn()
                t2 = time.perf_counter()
                td.append(t1 - t0)
                tn.append(t2 - t1)
            d, n = 1e3 * statistics.median(td), 1e3 * statistics.median(tn)
            row += " %10.3f %10.3f  " % (d, n)
            if d <= n and best.get(log_l, 0) == ls // 2:            # contiguous from 1
                best[log_l] = ls
        say(row)
        ls *= 2
    for log_l in (10, 16, 20):
        say("largest short length (contiguous from 1) with direct <= ntt at long 2^%d: %d" % (log_l, best.get(log_l, 0)))
    say("FRI_POLY_DIRECT_MAX in this build: %d" % fri_amd.POLY_DIRECT_MAX)


def sizes(ctx, corc):
    say()
    say("(ii) whole calls [ms, median of %d]; oracle = C oracle schoolbook, one thread, one run" % REPS)
    for la, lb in ((1 << 10, 1 << 10), (1 << 12, 1 << 12), (1 << 14, 1 << 14), (1 << 16, 1 << 16),
                   (1 << 20, 1 << 20), (1 << 20, 2)):
        a, b = coeffs(la, la), coeffs(la + lb, lb)
        t = median_ms(mul_call(ctx, a, b, 0))
        tt, log_n = transforms_ms(ctx, la, lb)
        orc = "%8.3f s" % oracle_s(corc, "mul", a, b) if la * lb <= 1 << 28 else "   (skipped)"
        say("mul      %8d x %-8d %9.3f ms   2 fri_lde + fri_interpolate at 2^%-2d %9.3f ms   oracle %s"
            % (la, lb, t, log_n, tt, orc))
    for la, lb in ((1 << 10, 1 << 10), (1 << 16, 1 << 16), (1 << 20, 1 << 20), (1 << 20, 2),
                   ((1 << 11) - 1, 1 << 10), ((1 << 13) - 1, 1 << 12), ((1 << 15) - 1, 1 << 14),
                   ((1 << 17) - 1, 1 << 16), ((1 << 21) - 1, 1 << 20)):
        a, b = coeffs(3 * la, la), coeffs(5 * la + lb, lb)
        t = median_ms(div_call(ctx, a, b))
        tt, log_n = transforms_ms(ctx, la - lb + 1, lb)
        orc = "%8.3f s" % oracle_s(corc, "div", a, b) if (la - lb + 1) * lb <= 1 << 28 else "   (skipped)"
        say("div_rem  %8d / %-8d %9.3f ms   2 fri_lde + fri_interpolate at 2^%-2d %9.3f ms   oracle %s"
            % (la, lb, t, log_n, tt, orc))
    g = fo.fe_pow(5, (P - 1) >> 10, P)
    for name, p, q in (("1023 o linear", coeffs(7, 1023), np.array([0, g], dtype=np.uint32)),
                       ("2^10 o 2^6", coeffs(8, 1 << 10), coeffs(9, 1 << 6))):
        t0 = time.perf_counter()
        ctx.poly_compose(p, q)
        first = 1e3 * (time.perf_counter() - t0)
        t = median_ms(lambda: ctx.poly_compose(p, q))
        say("compose  %-20s %9.3f ms   (first call %.3f ms; through the Python mirror)" % (name, t, first))


ROOTS_LEAVES = (128, 256, 512, 1024, 2048)


def roots_call(ctx, r):
    out = np.empty(r.size + 1, dtype=np.uint32)
    ln = ctypes.c_size_t()
    pr, po = fri_amd._ptr(r), fri_amd._ptr(out)

    def call():
        rc = ctx.lib.fri_poly_from_roots(ctx.h, pr, r.size, 0, po, out.size, ctypes.byref(ln))
        assert rc == 0, ctx.lib.fri_last_error(ctx.h)
    return call, out


def d2h_ms(words):
    """A plain device-to-host hipMemcpy of `words` words into pageable memory."""
    hip = ctypes.CDLL("libamdhip64.so")
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(words * 4)) == 0
    host = np.empty(words, dtype=np.uint32)
    t = median_ms(lambda: hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), dev, ctypes.c_size_t(words * 4), 2))
    hip.hipFree(dev)
    return t


def roots(ctx, corc):
    p64 = ctypes.POINTER(ctypes.c_uint64)
    corc.orc_poly_from_roots.restype = ctypes.c_size_t
    corc.orc_poly_from_roots.argtypes = [p64, ctypes.c_size_t, p64, ctypes.c_uint64]
    say("(iii) fri_poly_from_roots, whole call [ms, median of %d] per leaf size (roots per LDS leaf subtree)" % REPS)
    say("%8s " % "n" + "".join(" %9d" % lf for lf in ROOTS_LEAVES) + "   oracle (one thread, one run)")
    best = {}
    for log_n in (10, 14, 16, 20):
        n = 1 << log_n
        r = coeffs(900 + log_n, n)
        call, out = roots_call(ctx, r)
        ts = {lf: [] for lf in ROOTS_LEAVES}
        for lf in ROOTS_LEAVES:
            ctx.set_roots_leaf(lf)
            for _ in range(WARM):
                call()
        for _ in range(REPS):                                       # the candidates alternate
            for lf in ROOTS_LEAVES:
                ctx.set_roots_leaf(lf)
                t0 = time.perf_counter()
                call()
                ts[lf].append(time.perf_counter() - t0)
        med = {lf: 1e3 * statistics.median(ts[lf]) for lf in ROOTS_LEAVES}
        best[log_n] = min(ROOTS_LEAVES, key=lambda lf: med[lf])
        orc = "   (skipped)"
        if log_n <= 14:
            r64 = np.ascontiguousarray(r.astype(np.uint64))
            o64 = np.zeros(n + 1, dtype=np.uint64)
            t0 = time.perf_counter()
            corc.orc_poly_from_roots(r64.ctypes.data_as(p64), n, o64.ctypes.data_as(p64), P)
            orc = "%9.3f s" % (time.perf_counter() - t0)
            assert np.array_equal(out.astype(np.uint64), o64)
        say("%8d " % n + "".join(" %9.3f" % med[lf] for lf in ROOTS_LEAVES) + "   " + orc)
    ctx.set_roots_leaf(0)
    for log_n in (16, 20):
        say("lowest median at n = 2^%d: leaf %d" % (log_n, best[log_n]))
    say("FRI_ROOTS_LEAF in this build: %d (the 2^16 winner when the two differ)" % fri_amd.ROOTS_LEAF)
    # the parent's only device route: one fri_poly_mul by (x - r) per root
    r = coeffs(910, 1 << 10)

    def chain():
        acc = np.array([1], dtype=np.uint32)
        for v in r:
            acc = ctx.poly_mul(acc, np.array([(P - int(v)) % P, 1], dtype=np.uint32))
        return acc
    t0 = time.perf_counter()
    z = chain()
    t = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(z, ctx.poly_from_roots(r))
    say("n = 1024 as 1024 successive fri_poly_mul by a linear factor (Python mirror, one run): %9.3f ms" % t)
    say()
    say("fri_lagrange_basis, whole call [ms, median of %d]; copy = a device-to-host hipMemcpy of n^2 words alone" % REPS)
    for n in (256, 1024, 4096):
        xs = np.unique(coeffs(920 + n, n + 64))[:n].astype(np.uint32)
        xs = np.ascontiguousarray(xs[np.random.default_rng(n).permutation(n)])
        out = np.empty((n, n), dtype=np.uint32)
        px, po = fri_amd._ptr(xs), fri_amd._ptr(out)

        def call():
            rc = ctx.lib.fri_lagrange_basis(ctx.h, px, n, po, out.size)
            assert rc == 0, ctx.lib.fri_last_error(ctx.h)
        t, c = median_ms(call), d2h_ms(n * n)
        say("n = %5d  call %9.3f ms   copy %9.3f ms   call - copy %9.3f ms" % (n, t, c, t - c))


def mp_eval_call(ctx, c, xs, flags):
    out = np.empty(xs.size, dtype=np.uint32)
    pc, px, po = fri_amd._ptr(c), fri_amd._ptr(xs), fri_amd._ptr(out)

    def call():
        rc = ctx.lib.fri_evaluate_ex(ctx.h, pc, c.size, px, xs.size, flags, po)
        assert rc == 0, ctx.lib.fri_last_error(ctx.h)
    return call, out


def mp_interp_call(ctx, xs, ys, flags):
    out = np.empty(xs.size, dtype=np.uint32)
    ln = ctypes.c_size_t()
    px, py, po = fri_amd._ptr(xs), fri_amd._ptr(ys), fri_amd._ptr(out)

    def call():
        rc = ctx.lib.fri_interpolate_points_ex(ctx.h, px, py, xs.size, flags, po, ctypes.byref(ln))
        assert rc == 0, ctx.lib.fri_last_error(ctx.h)
    return call, out


def alternating_ms(calls):
    """Medians of the given calls [ms], the candidates alternating."""
    for c in calls:
        for _ in range(WARM):
            c()
    ts = [[] for _ in calls]
    for _ in range(REPS):
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            c()
            ts[i].append(time.perf_counter() - t0)
    return [1e3 * statistics.median(t) for t in ts]


def distinct_points(seed, n):
    u = np.unique(fo.splitmix64_np(seed, n + 64))
    return np.ascontiguousarray(u[np.random.default_rng(seed).permutation(u.size)][:n].astype(np.uint32))


MP_EVAL_DIRECT_LOG_MAX = 18      # 2^36 Horner steps; 2^20 would be 2^40
MP_INTERP_DIRECT_LOG_MAX = 17    # the direct kernels' limit


def crossover_from(rows):
    """The smallest power of two from which the tree is not slower than the
    direct path (rows: log_n -> (direct, tree), direct None where not run)."""
    best = None
    for log_n in sorted(rows, reverse=True):
        d, t = rows[log_n]
        if d is not None and t > d:
            break
        best = log_n
    return best


def multipoint(ctx):
    TREE, DIRECT = fri_amd.MP_FORCE_TREE, fri_amd.MP_FORCE_DIRECT
    cross = {"evaluate": [], "interpolate": []}
    for run in (1, 2):
        say("(iv) run %d: fri_evaluate_ex, d = count, whole call [ms, median of %d]" % (run, REPS))
        say("%8s %12s %12s" % ("d=count", "direct", "tree"))
        rows = {}
        for log_n in range(10, 21):
            n = 1 << log_n
            c, xs = coeffs(1300 + log_n, n), distinct_points(1400 + log_n, n)
            tree, got = mp_eval_call(ctx, c, xs, TREE)
            if log_n <= MP_EVAL_DIRECT_LOG_MAX:
                direct, want = mp_eval_call(ctx, c, xs, DIRECT)
                td, tt = alternating_ms([direct, tree])
                assert np.array_equal(got, want)
            else:
                td, tt = None, alternating_ms([tree])[0]
            rows[log_n] = (td, tt)
            say("%8s %12s %12.3f" % ("2^%d" % log_n, "%.3f" % td if td is not None else "-", tt))
        cross["evaluate"].append(crossover_from(rows))
        say()
        say("(iv) run %d: fri_interpolate_points_ex, whole call [ms, median of %d]" % (run, REPS))
        say("%8s %12s %12s" % ("n", "direct", "tree"))
        rows = {}
        for log_n in range(10, 21):
            n = 1 << log_n
            xs, ys = distinct_points(1500 + log_n, n), coeffs(1600 + log_n, n)
            tree, got = mp_interp_call(ctx, xs, ys, TREE)
            if log_n <= MP_INTERP_DIRECT_LOG_MAX:
                direct, want = mp_interp_call(ctx, xs, ys, DIRECT)
                td, tt = alternating_ms([direct, tree])
                assert np.array_equal(got, want)
            else:
                td, tt = None, alternating_ms([tree])[0]
            rows[log_n] = (td, tt)
            say("%8s %12s %12.3f" % ("2^%d" % log_n, "%.3f" % td if td is not None else "-", tt))
        cross["interpolate"].append(crossover_from(rows))
        say()
    for k in ("evaluate", "interpolate"):
        say("%s: tree not slower than direct from 2^%s upwards (run 1), 2^%s (run 2)" % (k, *cross[k]))
    say("FRI_MP_EVAL_MIN, FRI_MP_INTERP_MIN in this build: %d, %d" % (fri_amd.MP_EVAL_MIN, fri_amd.MP_INTERP_MIN))
    say()
    say("leaf size at 2^16 (tree paths, fri_debug_set_roots_leaf) [ms, median of %d]" % REPS)
    say("%12s " % "" + "".join(" %9d" % lf for lf in (64,) + ROOTS_LEAVES))
    n = 1 << 16
    c, xs, ys = coeffs(1700, n), distinct_points(1701, n), coeffs(1702, n)
    for name, call in (("evaluate", mp_eval_call(ctx, c, xs, TREE)[0]),
                       ("interpolate", mp_interp_call(ctx, xs, ys, TREE)[0])):
        ts = {lf: [] for lf in (64,) + ROOTS_LEAVES}
        for lf in ts:
            ctx.set_roots_leaf(lf)
            for _ in range(WARM):
                call()
        for _ in range(REPS):
            for lf in ts:
                ctx.set_roots_leaf(lf)
                t0 = time.perf_counter()
                call()
                ts[lf].append(time.perf_counter() - t0)
        say("%12s " % name + "".join(" %9.3f" % (1e3 * statistics.median(ts[lf])) for lf in ts))
    ctx.set_roots_leaf(0)
    say("FRI_ROOTS_LEAF in this build: %d" % fri_amd.ROOTS_LEAF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--roots", metavar="FILE", help="run the from_roots / Lagrange section (iii) alone and write it here")
    ap.add_argument("--multipoint", metavar="FILE",
                    help="run the multipoint evaluation / interpolation section (iv) alone and write it here")
    args = ap.parse_args()
    ctx = fri_amd.Context(0, LOG_MAX)                              # raises without a gfx950 device
    corc = fo.load_c_oracle()
    corc.orc_set_num_threads(1)
    say("poly_arith_probe: %s, context 2^%d" % (ctx.lib.fri_version().decode(), LOG_MAX))
    if args.multipoint:
        multipoint(ctx)
    elif args.roots:
        roots(ctx, corc)
    else:
        crossover(ctx)
        sizes(ctx, corc)
    ctx.close()
    out = args.multipoint or args.roots or args.out
    if out:
        with open(out, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
