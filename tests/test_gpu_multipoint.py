"""GPU: fri_evaluate_ex / fri_interpolate_points_ex on the product tree
(Polynomial::evaluate, ops.rs:76-83; Polynomial::interpolate on arbitrary
points, ops.rs:239-241 -> interpolation.rs:121-152) through the Python mirror.

Every comparison is word for word against the oracle, never against another
GPU path: Horner (orc_poly_evaluate) at every point and the Lagrange sum
(orc_interpolate_lagrange, interpolate_lagrange_polynomials) at the sizes the
quadratic oracle reaches; beyond them the points are a seeded permutation of
a coset, which the tree cannot see, and the expected words come from the
oracle's O(n log n) orc_lde / orc_interpolate_coset.  The sizes are those at
which the tree takes another path: one leaf subtree, several, the LDS levels
(products up to 4096 words), one and two batched NTT levels, padding with
zero roots, both leaf modes.  No tolerances: field arithmetic is exact."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 3221225473
_P64 = ctypes.POINTER(ctypes.c_uint64)


def _c64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _p(a):
    return a.ctypes.data_as(_P64)


def seeded(seed, n):
    import fri_oracle as fo
    return fo.splitmix64_np(seed, n) if n else np.zeros(0, dtype=np.uint64)


def _leaf():
    import fri_amd
    return fri_amd.ROOTS_LEAF


def next_pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def horner_all(corc, c, xs):
    c = _c64(c)
    corc.orc_poly_evaluate.restype = ctypes.c_uint64
    corc.orc_poly_evaluate.argtypes = [_P64, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64]
    pc = _p(c)
    return np.array([corc.orc_poly_evaluate(pc, c.size, int(x), P) for x in xs], dtype=np.uint64)


def c_lagrange(corc, xs, ys):
    xs, ys = _c64(xs), _c64(ys)
    want = np.empty(max(1, xs.size), dtype=np.uint64)
    corc.orc_interpolate_lagrange.restype = ctypes.c_size_t
    corc.orc_interpolate_lagrange.argtypes = [_P64, _P64, ctypes.c_size_t, _P64, ctypes.c_uint64]
    ln = corc.orc_interpolate_lagrange(_p(xs), _p(ys), xs.size, _p(want), P)
    return want[:ln]


def c_lde(corc, c, log_n):
    c = _c64(c)
    out = np.empty(1 << log_n, dtype=np.uint64)
    corc.orc_lde.restype = ctypes.c_int
    corc.orc_lde.argtypes = [_P64, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                             ctypes.c_uint64, _P64]
    assert corc.orc_lde(_p(c), c.size, log_n, 5, 5, P, _p(out)) == 0
    return out


def c_interpolate_coset(corc, ys, log_n):
    ys = _c64(ys)
    out = np.empty(1 << log_n, dtype=np.uint64)
    corc.orc_interpolate_coset.restype = ctypes.c_size_t
    corc.orc_interpolate_coset.argtypes = [_P64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                           _P64]
    ln = corc.orc_interpolate_coset(_p(ys), log_n, 5, 5, P, _p(out))
    return out[:ln]


@functools.lru_cache(maxsize=None)
def _coset(log_n):
    """The coset 5 * <w_{2^log_n}> in natural order (the oracle's LDE of the
    polynomial x) and a seeded permutation of its indices."""
    import fri_oracle as fo
    pts = c_lde(fo.load_c_oracle(), [0, 1], log_n)
    return pts, np.random.default_rng(4000 + log_n).permutation(1 << log_n)


def same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.uint32
    assert got.size == len(want), (got.size, len(want))
    assert np.array_equal(got.astype(np.uint64), _c64(want))


def points(seed, count):
    """Seeded points with 0, 1, p - 1 and a few repeated values."""
    xs = seeded(seed, count).copy()
    if count > 3:
        xs[0], xs[1], xs[2] = 0, 1, P - 1
        xs[count // 2] = xs[count // 3]
        xs[count - 1] = xs[0]
    if count > 200:
        xs[count - 70] = xs[5]          # across leaf subtrees in both leaf modes
    return xs


# ------------------------------------------------------------ evaluation ----
def _eval_counts():
    L = _leaf()
    return sorted({1, 2, 3, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1, 4095, 4096, 4097, 8193})


def _eval_cases():
    """(count, d, small_leaf); below 63 points both leaf modes are one leaf subtree."""
    out = []
    for count in _eval_counts():
        for d in sorted({0, 1, count, next_pow2(count)}):
            out.append((count, d, False))
            if count >= 63:
                out.append((count, d, True))
    return out


@functools.lru_cache(maxsize=None)
def _eval_expected(count, d):
    """Seeded inputs of one (count, d) with Horner at every point, shared by the leaf modes."""
    import fri_oracle as fo
    xs = points(7000 + count, count)
    c = seeded(9000 + 3 * count + d, d)
    return xs, c, horner_all(fo.load_c_oracle(), c, xs)


@pytest.mark.parametrize("count,d,small_leaf", _eval_cases())
def test_evaluate_tree_matches_horner(ctx, count, d, small_leaf):
    xs, c, want = _eval_expected(count, d)
    same(ctx.evaluate(c, xs, mode="tree", small_leaf=small_leaf), want)


@pytest.mark.parametrize("small_leaf", [False, True])
def test_evaluate_tree_all_points_equal(ctx, corc, small_leaf):
    count = 2 * _leaf() + 1
    xs = np.full(count, 123456789, dtype=np.uint64)
    c = seeded(31, count)
    same(ctx.evaluate(c, xs, mode="tree", small_leaf=small_leaf), horner_all(corc, c, xs))


@pytest.mark.parametrize("d,count", [(5000, 100), (70000, 300), (3, 5000)])
def test_evaluate_tree_degree_differs_from_point_count(ctx, corc, d, count):
    xs = points(d + count, count)
    c = seeded(d * 3 + count, d)
    same(ctx.evaluate(c, xs, mode="tree"), horner_all(corc, c, xs))


@pytest.mark.parametrize("k,count", [(17, (1 << 16) + 3), (20, 1 << 20)])
def test_evaluate_tree_large_every_value(ctx, corc, k, count):
    """d = count; the points are a permuted coset cut to `count`, so the
    expected values are the oracle's LDE, permuted; 64 positions hold
    arbitrary points instead, checked by Horner."""
    pts, perm = _coset(k)
    c = seeded(500 + k, count)
    xs = pts[perm][:count].copy()
    want = c_lde(corc, c, k)[perm][:count].copy()
    pos = np.random.default_rng(k).choice(count, 64, replace=False)
    xs[pos] = seeded(600 + k, 64)
    want[pos] = horner_all(corc, c, xs[pos])
    same(ctx.evaluate(c, xs, mode="tree"), want)


def test_evaluate_automatic_choice_around_threshold(ctx, corc):
    import fri_amd
    for m in (fri_amd.MP_EVAL_MIN - 1, fri_amd.MP_EVAL_MIN, fri_amd.MP_EVAL_MIN + 1):
        k = max(1, (m - 1).bit_length())
        pts, perm = _coset(k)
        c = seeded(700 + m, m)
        same(ctx.evaluate(c, pts[perm][:m]), c_lde(corc, c, k)[perm][:m])


# --------------------------------------------------------- interpolation ----
@pytest.mark.parametrize("small_leaf", [False, True])
@pytest.mark.parametrize("n,seed,dups", [(1, 1, 0), (2, 2, 0), (3, 3, 1), (5, 4, 0), (7, 5, 2), (16, 6, 0),
                                         (17, 7, 3), (33, 8, 0), (40, 9, 5)])
def test_interpolate_tree_matches_lagrange(ctx, oracle, n, seed, dups, small_leaf):
    r = np.random.default_rng(seed)
    xs = [int(v) for v in r.integers(0, P, n)]
    for i in range(dups):
        xs[int(r.integers(0, n))] = xs[int(r.integers(0, n))]
    ys = [int(v) for v in r.integers(0, P, n)]
    if n > 2:
        ys[1] = 0
    got = ctx.interpolate_points(xs, ys, mode="tree", small_leaf=small_leaf)
    assert got.tolist() == oracle.interpolate_lagrange_polynomials(xs, ys, P)


def _interp_tiers():
    return sorted({_leaf() + 1, 4096, 4999, 8193})


@functools.lru_cache(maxsize=None)
def _interp_expected(n):
    import fri_oracle as fo
    r = np.random.default_rng(n)
    xs = np.unique(r.integers(0, P, n + 64, dtype=np.uint64))[:n]
    r.shuffle(xs)
    ys = r.integers(0, P, n, dtype=np.uint64)
    return xs, ys, c_lagrange(fo.load_c_oracle(), xs, ys)


@pytest.mark.parametrize("small_leaf", [False, True])
@pytest.mark.parametrize("n", _interp_tiers())
def test_interpolate_tree_tiers(ctx, n, small_leaf):
    """Several leaf subtrees, the last LDS level (4096), padding (4999) and two
    batched NTT levels (8193) against the C oracle's Lagrange sum, whose O(n^2)
    is the cost of the first case of each n (computed once for both leaf modes);
    the result evaluates back to ys through the direct kernels."""
    xs, ys, want = _interp_expected(n)
    got = ctx.interpolate_points(xs, ys, mode="tree", small_leaf=small_leaf)
    same(got, want)
    assert np.array_equal(ctx.evaluate(got, xs, mode="direct").astype(np.uint64), ys)


def test_interpolate_beyond_the_direct_limit_shuffled_coset(ctx, corc):
    """n = 2^18 (the direct kernels stop at 2^17): a permuted coset with
    seeded values against the oracle's coset interpolation, every coefficient."""
    k = 18
    pts, perm = _coset(k)
    ys = seeded(818, 1 << k)
    nat = np.empty(1 << k, dtype=np.uint64)
    nat[perm] = ys
    same(ctx.interpolate_points(pts[perm], ys), c_interpolate_coset(corc, nat, k))


def test_interpolate_beyond_the_direct_limit_padded(ctx, corc):
    """n = 2^17 + 1 distinct points (padded with 2^17 - 1 zero roots) carrying
    the values of a polynomial with n coefficients: the interpolant is it."""
    k, n = 18, (1 << 17) + 1
    pts, perm = _coset(k)
    c = seeded(917, n)
    ys = c_lde(corc, c, k)[perm][:n]
    same(ctx.interpolate_points(pts[perm][:n], ys), np.trim_zeros(c, "b"))


@pytest.mark.parametrize("small_leaf", [False, True])
def test_interpolate_tree_repeated_and_special_points(ctx, corc, small_leaf):
    L = _leaf()
    n = 2 * L + 1
    xs = np.unique(seeded(41, n + 64))[:n]
    np.random.default_rng(41).shuffle(xs)
    xs[3] = 0                           # meets the zero padding
    xs[L + 7] = xs[10]                  # one value in two leaf subtrees
    xs[2 * L] = P - 1
    ys = seeded(42, n).copy()
    ys[0] = ys[L] = ys[n - 1] = 0
    same(ctx.interpolate_points(xs, ys, mode="tree", small_leaf=small_leaf), c_lagrange(corc, xs, ys))


def test_interpolate_automatic_choice_around_threshold(ctx, corc):
    import fri_amd
    for n in (fri_amd.MP_INTERP_MIN - 1, fri_amd.MP_INTERP_MIN, fri_amd.MP_INTERP_MIN + 1):
        k = max(1, (n - 1).bit_length())
        pts, perm = _coset(k)
        c = seeded(1100 + n, n)
        ys = c_lde(corc, c, k)[perm][:n]
        same(ctx.interpolate_points(pts[perm][:n], ys), np.trim_zeros(c, "b"))


@pytest.mark.parametrize("leaf", [64, 128, 256, 1024, 2048])
def test_tree_follows_the_roots_leaf_setting(ctx, corc, leaf):
    """fri_debug_set_roots_leaf sizes the leaf subtrees of both calls: three of
    them, the last one a single point beside the zero padding."""
    n = 2 * leaf + 1
    xs = np.unique(seeded(60 + leaf, n + 64))[:n]
    np.random.default_rng(leaf).shuffle(xs)
    ys, f = seeded(61 + leaf, n), seeded(62 + leaf, n)
    ctx.set_roots_leaf(leaf)
    try:
        got_f = ctx.interpolate_points(xs, ys, mode="tree")
        got_v = ctx.evaluate(f, xs, mode="tree")
    finally:
        ctx.set_roots_leaf(0)
    same(got_f, c_lagrange(corc, xs, ys))
    same(got_v, horner_all(corc, f, xs))


# ---------------------------------------------------------------- errors ----
def _rc_eval(c, coeffs, xs, flags):
    import fri_amd
    a, x = fri_amd._u32(coeffs), fri_amd._u32(xs)
    out = np.empty(max(1, x.size), dtype=np.uint32)
    return c.lib.fri_evaluate_ex(c.h, fri_amd._ptr(a), a.size, fri_amd._ptr(x), x.size, flags, fri_amd._ptr(out))


def _rc_interp(c, xs, ys, flags):
    import fri_amd
    x, y = fri_amd._u32(xs), fri_amd._u32(ys)
    out = np.empty(max(1, x.size), dtype=np.uint32)
    ln = ctypes.c_size_t()
    return c.lib.fri_interpolate_points_ex(c.h, fri_amd._ptr(x), fri_amd._ptr(y), x.size, flags, fri_amd._ptr(out),
                                           ctypes.byref(ln))


def test_flag_and_value_errors(ctx):
    import fri_amd
    both = fri_amd.MP_FORCE_TREE | fri_amd.MP_FORCE_DIRECT
    for flags in (both, both | fri_amd.MP_SMALL_LEAF, 8, 1 << 31):
        assert _rc_eval(ctx, [1, 2], [3, 4], flags) == fri_amd.FRI_EINVAL
        assert _rc_interp(ctx, [1, 2], [3, 4], flags) == fri_amd.FRI_EINVAL
    for mode in (None, "tree", "direct"):
        with pytest.raises(fri_amd.FriError) as e:
            ctx.evaluate([1, P], [3, 4], mode=mode)
        assert e.value.code == fri_amd.FRI_EINVAL
        with pytest.raises(fri_amd.FriError) as e:
            ctx.evaluate([1, 2], [P, 4], mode=mode)
        assert e.value.code == fri_amd.FRI_EINVAL
        with pytest.raises(fri_amd.FriError) as e:
            ctx.interpolate_points([1, 2], [P, 4], mode=mode)
        assert e.value.code == fri_amd.FRI_EINVAL
        with pytest.raises(fri_amd.FriError):
            ctx.interpolate_points([1, 2], [3], mode=mode)              # interpolation.rs:127 panics
    assert ctx.evaluate([], [5, 6], mode="tree").tolist() == [0, 0]
    assert ctx.evaluate([5], [], mode="tree").tolist() == []
    assert ctx.interpolate_points([], [], mode="tree").tolist() == []


def test_forced_tree_outside_its_sizes(corc):
    import fri_amd
    small = fri_amd.Context(0, 12)
    try:
        xs = seeded(1, 2049)                       # N = 4096: d + N - 1 > 2^12 for d >= 2
        with pytest.raises(fri_amd.FriError) as e:
            small.evaluate([1, 2], xs, mode="tree")
        assert e.value.code == fri_amd.FRI_EINVAL and "FRI_MP_FORCE_TREE" in str(e.value)
        with pytest.raises(fri_amd.FriError) as e:
            small.evaluate(seeded(2, 2049), [1, 2], mode="tree")        # next_pow2(d) > 2^11
        assert e.value.code == fri_amd.FRI_EINVAL and "FRI_MP_FORCE_TREE" in str(e.value)
        with pytest.raises(fri_amd.FriError) as e:
            small.interpolate_points(xs, xs, mode="tree")               # next_pow2(n) > 2^11
        assert e.value.code == fri_amd.FRI_EINVAL and "FRI_MP_FORCE_TREE" in str(e.value)
        # the automatic choice still serves these through the direct kernels
        c = seeded(2, 2049)
        same(small.evaluate(c, xs[:5]), horner_all(corc, c, xs[:5]))
        ux = np.unique(xs)
        same(small.interpolate_points(ux, ux), [0, 1])
        # ... and the tree at the largest sizes that fit
        ys = seeded(3, 2048)
        same(small.interpolate_points(ux[:2048], ys, mode="tree"), c_lagrange(corc, ux[:2048], ys))
        same(small.evaluate(c[:2048], ux[:2048], mode="tree"), horner_all(corc, c[:2048], ux[:2048]))
    finally:
        small.close()


def test_out_of_memory_leaves_the_context_usable(corc):
    import fri_amd
    c = fri_amd.Context(0, 16)
    try:
        xs, ys, want = _interp_expected(4096)           # shared with the tier test
        f = seeded(7, xs.size)
        c.set_device_cap(c.device_bytes()[0] + 4096)    # no room for the retained levels
        for call in (lambda: c.interpolate_points(xs, ys, mode="tree"), lambda: c.evaluate(f, xs, mode="tree")):
            with pytest.raises(fri_amd.FriError) as e:
                call()
            assert e.value.code == fri_amd.FRI_ENOMEM
        c.set_device_cap(0)
        same(c.interpolate_points(xs, ys, mode="tree"), want)
        same(c.evaluate(f, xs, mode="tree"), horner_all(corc, f, xs))
    finally:
        c.close()


# --------------------------------------------------- unchanged neighbours ----
def test_from_roots_unchanged_after_tree_calls(ctx, corc):
    """The retained levels live in the grown scratch: the product tree of
    fri_poly_from_roots still moves between the context buffers."""
    L = _leaf()
    for n in (65, L + 1, 4097, 8193):
        xs = np.unique(seeded(50 + n, n + 64))[:n]
        ctx.evaluate(seeded(51 + n, n), xs, mode="tree")
        ctx.interpolate_points(xs, seeded(52 + n, n), mode="tree", small_leaf=n < 4097)
    r = seeded(77, 2 * L + 1)
    want = np.zeros(r.size + 1, dtype=np.uint64)
    corc.orc_poly_from_roots.restype = ctypes.c_size_t
    corc.orc_poly_from_roots.argtypes = [_P64, ctypes.c_size_t, _P64, ctypes.c_uint64]
    ln = corc.orc_poly_from_roots(_p(_c64(r)), r.size, _p(want), P)
    same(ctx.poly_from_roots(r), want[:ln])
