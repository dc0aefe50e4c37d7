"""GPU: every dispatch tier of the kernel-level entry points, through the
Python mirror, word for word against the C oracle.

fri_lde, fri_interpolate, fri_fold, fri_merkle_root, fri_batch_inverse and the
direct kernels of fri_evaluate / fri_interpolate_points choose a kernel
instance, a mid-level schedule or a segment count from the shape alone.  The
hand-picked shapes of tests/test_gpu_parity.py leave whole instances unrun;
this file sweeps the sizes instead.  Its shape tables are built from n alone
(fractions of n and their neighbours, sizes on either side of a power of two),
never from the library's dispatch rules, so they stay complete when a
threshold moves; the unmarked tests at the end check the tables themselves on
the CPU.  Every comparison is against the oracle (orc_lde,
orc_interpolate_coset, orc_fold_eval, orc_merkle_build, orc_batch_inverse,
orc_poly_evaluate, orc_interpolate_lagrange), never against another GPU path,
and exact: integer field arithmetic and SHA-256 have no tolerance.  Seeded
values are fri_oracle.splitmix64_np streams.  A failure names the entry point
and the (shape, offset, ...) at which it happened."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

P = 3221225473
_P64 = ctypes.POINTER(ctypes.c_uint64)


# ------------------------------------------------------------------ tables --
LDE_LOGS = list(range(1, 21))
INTT_LOGS = list(range(0, 21))
FOLD_LOGS = list(range(1, 19))
MERKLE_POW2_LOGS = list(range(0, 23))
MERKLE_RAGGED = sorted({(1 << L) + s for L in range(2, 14) for s in (-1, 1)} | {3 << k for k in range(11)})
TRACE_SHAPES = [(8, 3), (12, 2), (14, 1), (13, 4)]                    # log_t + log_blowup = 11, 14, 15, 17
BATCH_INVERSE_SIZES = [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) + 3]
# (d, count): every d range with counts on either side of the bound at which the
# lane count stops growing; the d straddle multiples of the lane count
EVAL_DIRECT = [(4095, 70), (4096, 1), (8191, 3), (8192, 5), (16383, 1023), (16385, 3), (32767, 511), (32768, 2),
               (65535, 255), (65536, 127), (131071, 63), (131072, 63), (131072, 64), (131073, 1)]
INTERP_DIRECT_LAGRANGE = [511, 512, 1023, 1024, 2047, 2048, 8192]
INTERP_DIRECT_COSET = [1 << 15, (1 << 15) + 1, 1 << 16, 1 << 17]      # 2^17: the direct kernels' documented limit


def lde_degrees(n):
    """Coefficient counts of one LDE size: the fractions of n at which a
    zero-padded first pass could change, each with its upper neighbour."""
    cand = (1, n // 8, n // 8 + 1, n // 4, n // 4 + 1, n // 2, n // 2 + 1, n - 1, n)
    return sorted({min(max(d, 1), n) for d in cand})


# ----------------------------------------------------------------- helpers --
def seeded(seed, n):
    import fri_oracle as fo
    return fo.splitmix64_np(seed, n) if n else np.zeros(0, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def offsets():
    """1, the generator, p - 1 and one seeded value above 2^31."""
    big = next(int(v) for v in seeded(20261, 64) if v > (1 << 31))
    return (1, 5, P - 1, big)


def _c64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _p(a):
    return a.ctypes.data_as(_P64)


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32))


def same(got, want, what):
    """Every word of `got` (uint32 from the library) equals the oracle's `want`."""
    got = np.asarray(got)
    want = _c64(want)
    assert got.dtype == np.uint32, what
    assert got.size == want.size, f"{what}: length {got.size}, oracle {want.size}"
    bad = np.flatnonzero(got.astype(np.uint64) != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} words differ, first at {int(bad[0])}: "
                           f"got {int(got[bad[0]])}, oracle {int(want[bad[0]])}")


def c_lde(corc, c, log_n, offset):
    c = _c64(c)
    d = c.size
    if not d:
        c = np.zeros(1, dtype=np.uint64)
    out = np.empty(1 << log_n, dtype=np.uint64)
    assert corc.orc_lde(_p(c), d, log_n, offset, 5, P, _p(out)) == 0
    return out


def c_interpolate_coset(corc, ys, log_n, offset):
    ys = _c64(ys)
    out = np.empty(1 << log_n, dtype=np.uint64)
    ln = corc.orc_interpolate_coset(_p(ys), log_n, offset, 5, P, _p(out))
    return out[:ln]


def c_merkle_nodes(corc, values):
    """orc_merkle_build's nodes (leaves first, then every level up to the root) as bytes."""
    v = _c64(values)
    cnt = corc.orc_merkle_nodes_count(v.size)
    buf = np.empty(32 * cnt, dtype=np.uint8)
    corc.orc_merkle_build(_p(v), v.size, buf.ctypes.data_as(ctypes.c_char_p))
    return buf


def horner_all(corc, c, xs):
    c = _c64(c)
    pc = _p(c)
    return np.array([corc.orc_poly_evaluate(pc, c.size, int(x), P) for x in xs], dtype=np.uint64)


def c_lagrange(corc, xs, ys):
    xs, ys = _c64(xs), _c64(ys)
    want = np.empty(xs.size, dtype=np.uint64)
    ln = corc.orc_interpolate_lagrange(_p(xs), _p(ys), xs.size, _p(want), P)
    return want[:ln]


LAGRANGE_SPLIT_FROM = 4096      # the oracle's Lagrange sum costs about 0.4 us * n^2 on one core
LAGRANGE_PARTS = 8


def c_lagrange_split(corc, xs, ys, parts=LAGRANGE_PARTS):
    """orc_interpolate_lagrange over `parts` slices A of the points, one thread
    each (ctypes releases the GIL), joined exactly.  With Z_B the polynomial
    whose roots are the points outside A, L_i = L_i^A * Z_B / Z_B(x_i) for i in
    A, so f = sum over A of Z_B * interpolate(xs_A, ys_A / Z_B(xs_A)): every
    step is an oracle function (from_roots, Horner, batch inverse with
    inverse(0) = 0, the Lagrange sum, poly_mul)."""
    from concurrent.futures import ThreadPoolExecutor
    xs, ys = _c64(xs), _c64(ys)
    n = xs.size
    corc.orc_poly_from_roots.restype = ctypes.c_size_t
    corc.orc_poly_from_roots.argtypes = [_P64, ctypes.c_size_t, _P64, ctypes.c_uint64]

    def term(k):
        lo, hi = k * n // parts, (k + 1) * n // parts
        rest = _c64(np.concatenate([xs[:lo], xs[hi:]]))
        zb = np.ones(rest.size + 1, dtype=np.uint64)                         # no other points: Z_B = 1
        assert corc.orc_poly_from_roots(_p(rest), rest.size, _p(zb), P) == (rest.size + 1 if rest.size else 0)
        at = horner_all(corc, zb, xs[lo:hi])
        inv = np.empty_like(at)
        corc.orc_batch_inverse(_p(at), _p(inv), at.size, P)
        fa = c_lagrange(corc, xs[lo:hi], ys[lo:hi] * inv % np.uint64(P))     # factors below 2^32
        out = np.zeros(n, dtype=np.uint64)
        if fa.size:
            fa = _c64(fa)
            corc.orc_poly_mul(_p(fa), fa.size, _p(zb), zb.size, _p(out), P)  # at most (hi - lo) + (n - hi + lo + 1) - 1 = n words
        return out

    with ThreadPoolExecutor(parts) as pool:
        f = np.zeros(n, dtype=np.uint64)
        for t in pool.map(term, range(parts)):
            f = (f + t) % np.uint64(P)
    return np.trim_zeros(f, "b")


def merkle_values(seed, n):
    """Seeded leaves; leaves 0, 1 and n - 1 hold 0, 1 and p - 1."""
    v = seeded(seed, n).copy()
    for i, x in ((0, 0), (1, 1), (n - 1, P - 1)):
        if 0 <= i < n:
            v[i] = x
    return v


@functools.lru_cache(maxsize=None)
def _coset(log_n):
    """The coset 5 * <w_{2^log_n}> in natural order (the oracle's LDE of the
    polynomial x) and a seeded permutation of its indices."""
    import fri_oracle as fo
    pts = c_lde(fo.load_c_oracle(), [0, 1], log_n, 5)
    return pts, np.argsort(seeded(4100 + log_n, 1 << log_n), kind="stable")


# ------------------------------------------------------- 1. forward NTT ----
@pytest.mark.gpu
@pytest.mark.parametrize("log_n", LDE_LOGS)
def test_lde_every_first_pass(ctx, corc, log_n):
    """fri_lde against orc_lde, every output word: each size with coefficient
    counts on both sides of n/8, n/4, n/2 and n (the rows a zero-padded first
    pass skips are not read, so a wrong instance gives wrong values, not a
    fault), four offsets, c[0] = 0 and c[d-1] = p - 1."""
    n = 1 << log_n
    for d in lde_degrees(n):
        c = seeded(1000 * log_n + d, d).copy()
        c[0] = 0
        c[d - 1] = P - 1
        c32 = _u32(c)
        for off in offsets():
            same(ctx.lde(c32, log_n, off), c_lde(corc, c, log_n, off), f"fri_lde log_n={log_n} d={d} offset={off}")
    for off in offsets():
        got = ctx.lde(np.zeros(0, dtype=np.uint32), log_n, off)      # the zero polynomial: the oracle starts at d = 1
        assert got.dtype == np.uint32 and got.size == n and not got.any(), f"fri_lde log_n={log_n} d=0 offset={off}"
    if log_n <= 12:
        c = np.full(n, P - 1, dtype=np.uint64)
        for off in offsets():
            same(ctx.lde(_u32(c), log_n, off), c_lde(corc, c, log_n, off),
                 f"fri_lde log_n={log_n} d={n} all p-1 offset={off}")


# ------------------------------------------------------- 2. inverse NTT ----
@pytest.mark.gpu
@pytest.mark.parametrize("log_n", INTT_LOGS)
def test_interpolate_every_size(ctx, corc, log_n):
    """fri_interpolate against orc_interpolate_coset, coefficients and length:
    seeded values (full length), zeros (length 0), a constant (length 1) and
    the oracle's LDE of a polynomial with n/2 + 1 coefficients."""
    n = 1 << log_n
    half = seeded(7000 + log_n, n // 2 + 1).copy()
    half[-1] = P - 1
    const = int(seeded(7100 + log_n, 1)[0]) or 1
    for off in offsets():
        inputs = (("seeded", seeded(7200 + log_n, n), n),
                  ("zeros", np.zeros(n, dtype=np.uint64), 0),
                  ("constant", np.full(n, const, dtype=np.uint64), 1),
                  ("lde of n/2+1 coefficients", c_lde(corc, half, log_n, off), n // 2 + 1))
        for name, ys, length in inputs:
            what = f"fri_interpolate log_n={log_n} offset={off} ys={name}"
            want = c_interpolate_coset(corc, ys, log_n, off)
            assert want.size == length, what
            same(ctx.interpolate(_u32(ys), off), want, what)


# -------------------------------------------------------------- 3. fold ----
@pytest.mark.gpu
@pytest.mark.parametrize("log_m", FOLD_LOGS)
def test_fold_every_size(ctx, corc, log_m):
    """fri_fold against orc_fold_eval: betas 0, 1, p - 1 and a seeded one, four
    offsets, seeded layers with planted pairs whose difference (first layer)
    or sum (second layer) is zero."""
    m = 1 << log_m
    h = m // 2
    w = corc.orc_fe_pow(5, (P - 1) >> log_m, P)
    planted = sorted({0, h // 3, h // 2, h - 1})
    betas = (0, 1, P - 1, int(seeded(8100 + log_m, 1)[0]))
    for kind in ("equal", "opposite"):
        layer = seeded(8000 + log_m, m).copy()
        for i in planted:
            layer[i + h] = layer[i] if kind == "equal" else (P - int(layer[i])) % P
        l32 = _u32(layer)
        for off in offsets():
            for beta in betas:
                want = np.empty(h, dtype=np.uint64)
                corc.orc_fold_eval(_p(layer), m, off, w, beta, P, _p(want))
                same(ctx.fold(l32, off, beta), want, f"fri_fold log_m={log_m} offset={off} beta={beta} pairs={kind}")


# ------------------------------------------------------------ 4. Merkle ----
@pytest.mark.gpu
@pytest.mark.parametrize("L", MERKLE_POW2_LOGS)
def test_merkle_root_every_power_of_two(ctx, corc, L):
    """The non-commit instantiations of the leaf, mid and top kernels: the
    mid-level schedule changes with every L."""
    n = 1 << L
    v = merkle_values(9000 + L, n)
    nodes = c_merkle_nodes(corc, v)
    assert ctx.merkle_root(_u32(v)) == nodes[-32:].tobytes(), f"fri_merkle_root n=2^{L}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", MERKLE_RAGGED)
def test_merkle_root_ragged_sizes(ctx, corc, n):
    """2^L - 1, 2^L + 1 and 3 * 2^k leaves: a lone right-most node is promoted
    at the first, the last or every second level."""
    v = merkle_values(9100 + n, n)
    nodes = c_merkle_nodes(corc, v)
    assert ctx.merkle_root(_u32(v)) == nodes[-32:].tobytes(), f"fri_merkle_root n={n}"


@pytest.mark.gpu
@pytest.mark.parametrize("log_t,lb", TRACE_SHAPES)
def test_trace_tree_nodes_along_opened_paths(ctx, corc, log_t, lb):
    """fri_trace_commit: LDE and root against the oracle's tree of the oracle's
    LDE; fri_trace_decommit: every sibling digest against that tree's node, and
    the path hashed up to the root."""
    L = log_t + lb
    n, B = 1 << L, 1 << lb
    trace = seeded(9200 + L, 1 << log_t)
    what = f"fri_trace_commit log_t={log_t} log_blowup={lb}"
    root, coeffs, lde = ctx.trace_commit(_u32(trace), lb)
    want_c = c_interpolate_coset(corc, trace, log_t, 1)
    same(coeffs, want_c, what + " coefficients")
    want_lde = c_lde(corc, want_c, L, 5)
    same(lde, want_lde, what + " LDE")
    nodes = c_merkle_nodes(corc, want_lde)
    assert nodes.size == 32 * (2 * n - 1)
    assert root == nodes[-32:].tobytes(), what + " root"

    def node(level, j):                       # leaves first, then each level: level l starts at 2n - (2n >> l)
        o = 32 * (2 * n - (2 * n >> level) + j)
        return nodes[o:o + 32].tobytes()

    for index in (0, int(seeded(9300 + L, 1)[0]) % n, n - 1):
        opened = ctx.trace_decommit(index, B, 3, L)
        assert len(opened) == 3
        for j, (val, path) in enumerate(opened):
            leaf = (index + j * B) % n
            where = f"fri_trace_decommit log_t={log_t} log_blowup={lb} index={index} j={j}"
            assert val == int(want_lde[leaf]), where
            assert len(path) == 32 * L, where
            h = hashlib.sha256(val.to_bytes(8, "big")).digest()
            for l in range(L):
                sib = path[32 * l:32 * l + 32]
                assert sib == node(l, (leaf >> l) ^ 1), f"{where} level={l}"
                h = hashlib.sha256(h + sib if (leaf >> l) % 2 == 0 else sib + h).digest()
            assert h == root, where


# ----------------------------------------------------- 5. batch inverse ----
def _batch_inverse_patterns(n, seed):
    x = seeded(seed, n).copy()
    x[x == 0] = 1
    yield "no zeros", x
    yield "all zeros", np.zeros(n, dtype=np.uint64)
    one = np.zeros(n, dtype=np.uint64)
    one[(2 * n) // 3] = x[0]
    yield "all zeros but one", one
    ends = x.copy()
    ends[0] = ends[n - 1] = 0
    yield "x[0] = x[n-1] = 0", ends
    stride = (n + 15) // 16                  # a whole lane's elements: g + k * ceil(n / 16)
    g = stride // 2
    lane = x.copy()
    lane[g::stride] = 0
    yield f"lane g={g} stride={stride} zero", lane
    units = x.copy()
    units[n // 3] = 1
    units[n // 2] = P - 1
    yield "1 and p-1", units


def _check_batch_inverse(c, corc, n, seed, tag=""):
    for name, x in _batch_inverse_patterns(n, seed):
        want = np.empty(n, dtype=np.uint64)
        corc.orc_batch_inverse(_p(x), _p(want), n, P)
        same(c.batch_inverse(_u32(x)), want, f"fri_batch_inverse{tag} n={n} pattern={name}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCH_INVERSE_SIZES)
def test_batch_inverse_every_word(ctx, corc, n):
    _check_batch_inverse(ctx, corc, n, 10000 + n)


@pytest.mark.gpu
def test_batch_inverse_chunk_loop(corc):
    """n above the context's 2^log_n_max runs in chunks of that size: one full
    chunk and one element, and two full chunks and five."""
    import fri_amd
    small = fri_amd.Context(0, 10)
    try:
        for n in ((1 << 10) + 1, 2 * (1 << 10) + 5):
            _check_batch_inverse(small, corc, n, 10500 + n, tag=" log_n_max=10")
    finally:
        small.close()


# ------------------------------------------------- 6. direct evaluation ----
@pytest.mark.gpu
@pytest.mark.parametrize("d,count", EVAL_DIRECT)
def test_evaluate_direct_every_lane_count(ctx, corc, d, count):
    """The coefficients split over the lanes of a point, Horner in the C oracle
    at every point; 0, 1 and p - 1 are among the points (with fewer than three
    points, in a second call)."""
    c = seeded(11000 + d + count, d)
    c32 = _u32(c)
    special = np.array([0, 1, P - 1], dtype=np.uint64)
    xs = seeded(11500 + d + count, count).copy()
    sets = [xs]
    if count >= 3:
        xs[:3] = special
    else:
        sets.append(np.roll(special, d % 3)[:count])
    for pts in sets:
        same(ctx.evaluate(c32, _u32(pts), mode="direct"), horner_all(corc, c, pts),
             f"fri_evaluate direct d={d} count={count} first points={[int(v) for v in pts[:3]]}")


@pytest.mark.gpu
def test_evaluate_direct_many_points_one_lane_each(ctx, corc):
    """count = 2^16 goes back to one lane per point: the points are a permuted
    coset, so the expected values are the oracle's LDE, permuted."""
    k, d = 16, 4096
    pts, perm = _coset(k)
    c = seeded(11900, d)
    same(ctx.evaluate(_u32(c), _u32(pts[perm]), mode="direct"), c_lde(corc, c, k, 5)[perm],
         f"fri_evaluate direct d={d} count={1 << k}")


# ---------------------------------------------- 7. direct interpolation ----
def _distinct_points(seed, n):
    xs = np.unique(seeded(seed, n + 64))[:n]
    return xs[np.argsort(seeded(seed + 1, n), kind="stable")]


@pytest.mark.gpu
@pytest.mark.parametrize("n", INTERP_DIRECT_LAGRANGE)
def test_interpolate_direct_matches_lagrange(ctx, corc, n):
    """Distinct seeded points against the oracle's Lagrange sum (from
    LAGRANGE_SPLIT_FROM points on, computed over slices of the points)."""
    xs = _distinct_points(12000 + n, n)
    ys = seeded(12100 + n, n)
    want = c_lagrange_split(corc, xs, ys) if n >= LAGRANGE_SPLIT_FROM else c_lagrange(corc, xs, ys)
    same(ctx.interpolate_points(_u32(xs), _u32(ys), mode="direct"), want, f"fri_interpolate_points direct n={n}")


@pytest.mark.gpu
def test_interpolate_direct_duplicates_across_segments(ctx, corc):
    """Repeated points (their basis polynomials vanish through inverse(0) = 0)
    whose copies lie at opposite ends and in the middle of the point range."""
    n = 2048
    xs = _distinct_points(12300, n).copy()
    xs[n - 4] = xs[3]
    xs[n // 2 + 5] = xs[5]
    xs[n - 1] = xs[n // 2 - 1]
    ys = seeded(12301, n)
    same(ctx.interpolate_points(_u32(xs), _u32(ys), mode="direct"), c_lagrange(corc, xs, ys),
         f"fri_interpolate_points direct n={n} with duplicates")


@pytest.mark.gpu
@pytest.mark.parametrize("n", INTERP_DIRECT_COSET)
def test_interpolate_direct_large_permuted_coset(ctx, corc, n):
    """Beyond the quadratic oracle: the points are a permuted coset cut to n.
    A whole coset carries seeded values (oracle: coset interpolation); a cut one
    carries the oracle's LDE of a polynomial with n coefficients, which is then
    the interpolant."""
    k = (n - 1).bit_length()
    pts, perm = _coset(k)
    what = f"fri_interpolate_points direct n={n}"
    if n == 1 << k:
        ys = seeded(12400 + k, n)
        nat = np.empty(n, dtype=np.uint64)
        nat[perm] = ys
        want = c_interpolate_coset(corc, nat, k, 5)
    else:
        want = seeded(12500 + k, n).copy()
        want[-1] = P - 1
        ys = c_lde(corc, want, k, 5)[perm][:n]
    same(ctx.interpolate_points(_u32(pts[perm][:n]), _u32(ys), mode="direct"), want, what)


# ------------------------------------------- the tables themselves (CPU) ----
def test_lde_table_has_both_sides_of_every_padding_bound():
    """For every size and every count z of skippable stages that fits, some d
    has n >> (z+1) < d <= n >> z, and n >> z and its upper neighbour are both
    there, so an off-by-one in either direction meets a shape."""
    for log_n in LDE_LOGS:
        n = 1 << log_n
        ds = lde_degrees(n)
        assert all(1 <= d <= n for d in ds) and n in ds
        for z in range(0, min(3, log_n) + 1):
            assert any((n >> (z + 1)) < d <= (n >> z) for d in ds), (log_n, z)
            if z:
                assert (n >> z) in ds and (n >> z) + 1 in ds, (log_n, z)


def test_split_lagrange_sum_equals_the_single_call(corc):
    """The sliced oracle of the n = 8192 case is the oracle: same words as one
    orc_interpolate_lagrange call, repeated points within and across slices included."""
    assert max(INTERP_DIRECT_LAGRANGE) >= LAGRANGE_SPLIT_FROM > 2048
    for n, parts in ((1, 1), (7, 8), (257, 8), (300, 3)):
        xs = _distinct_points(13000 + n, n).copy()
        if n > 100:
            xs[n - 2] = xs[1]                      # across slices
            xs[4] = xs[3]                          # within one
        ys = seeded(13100 + n, n)
        assert np.array_equal(c_lagrange_split(corc, xs, ys, parts), c_lagrange(corc, xs, ys)), (n, parts)


def test_size_tables_reach_every_residue_and_neighbour():
    assert {k % 8 for k in LDE_LOGS} == set(range(8)) and LDE_LOGS == list(range(1, 21))
    assert {k % 8 for k in INTT_LOGS} == set(range(8)) and INTT_LOGS == list(range(0, 21))
    assert FOLD_LOGS == list(range(1, 19))
    assert MERKLE_POW2_LOGS == list(range(0, 23))
    for L in range(2, 14):
        assert (1 << L) - 1 in MERKLE_RAGGED and (1 << L) + 1 in MERKLE_RAGGED
    assert all(3 << k in MERKLE_RAGGED for k in range(11))
    assert sorted(t + b for t, b in TRACE_SHAPES) == [11, 14, 15, 17]
    for k in (4, 8, 12, 16):                                     # each power of two with both neighbours
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= set(BATCH_INVERSE_SIZES)
    assert sum(d * c for d, c in EVAL_DIRECT) < 10 ** 8          # Horner products of the oracle side
    ds = {d for d, _ in EVAL_DIRECT}
    for k in range(12, 18):                                      # every doubling of d: just below it, and at or above it
        assert (1 << k) - 1 in ds and ds & {1 << k, (1 << k) + 1}, k
    for k in (9, 10, 11):
        assert {(1 << k) - 1, 1 << k} <= set(INTERP_DIRECT_LAGRANGE)
    assert max(INTERP_DIRECT_COSET) == 1 << 17
