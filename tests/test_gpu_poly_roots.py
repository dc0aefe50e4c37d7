"""GPU: fri_poly_from_roots / fri_lagrange_basis (gen_polynomial_from_roots,
gen_lagrange_polynomials; src/polynomial/interpolation.rs:9-23, 46-115)
through the Python mirror, bit-exact against the oracle.

Z is compared coefficient by coefficient with the C oracle's schoolbook
orc_poly_from_roots up to 4097 roots, at every size at which the tree takes
another path (one leaf, several leaves, LDS levels, batched NTT levels), in
both leaf modes; above that the tests check the length, the leading 1, Z at
roots and Z(t) = prod (t - x_i).  The basis is compared with the Python
oracle up to n = 257; at n = 1024 and 4096 (the segmented row kernel) every
stored word enters the partition of unity, and rows are compared with
w_i * Z / (x - x_i) from the C oracle.  No tolerances: field arithmetic is
exact."""
import ctypes

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


def distinct(seed, n):
    """n distinct seeded points: unique, then a seeded permutation, then n of them."""
    u = np.unique(seeded(seed, n + 64))
    assert u.size >= n
    return u[np.random.default_rng(seed).permutation(u.size)][:n]


def c_from_roots(corc, roots):
    r = _c64(roots)
    out = np.zeros(r.size + 1, dtype=np.uint64)
    corc.orc_poly_from_roots.restype = ctypes.c_size_t
    corc.orc_poly_from_roots.argtypes = [_P64, ctypes.c_size_t, _P64, ctypes.c_uint64]
    n = corc.orc_poly_from_roots(_p(r), r.size, _p(out), P)
    return out[:n]


def c_eval(corc, c, x):
    c = _c64(c)
    return int(corc.orc_poly_evaluate(_p(c), c.size, int(x), P))


def c_div_rem(corc, a, b):
    a, b = _c64(a), _c64(b)
    q = np.zeros(max(1, a.size), dtype=np.uint64)
    r = np.zeros(max(1, a.size), dtype=np.uint64)
    lq, lr = ctypes.c_size_t(), ctypes.c_size_t()
    assert corc.orc_poly_div_rem(_p(a), a.size, _p(b), b.size, _p(q), ctypes.byref(lq), _p(r), ctypes.byref(lr),
                                 P) == 0
    return q[: lq.value], r[: lr.value]


def same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.uint32
    assert got.size == len(want), (got.size, len(want))
    assert np.array_equal(got.astype(np.uint64), _c64(want))


def prod_mod(v):
    """prod v mod p for a uint64 array of canonical values (pairwise, vectorised)."""
    v = np.asarray(v, dtype=np.uint64) % np.uint64(P)
    while v.size > 1:
        if v.size & 1:
            v = np.append(v, np.uint64(1))
        # both factors < 2^32: the product fits 64 bits
        v = (v[0::2] * v[1::2]) % np.uint64(P)
    return int(v[0]) if v.size else 1


def _leaf():
    import fri_amd
    return fri_amd.ROOTS_LEAF


def _sizes():
    L = _leaf()
    return sorted({0, 1, 2, 3, 63, 64, 65, 127, 129, L - 1, L, L + 1, 2 * L + 1, 4097})


# ------------------------------------------------------------ from_roots ----
@pytest.fixture(scope="module")
def roots_and_z(corc):
    """Seeded roots of every compared size with the C oracle's Z, computed once."""
    out = {}
    for n in _sizes():
        r = seeded(1000 + n, n)
        out[n] = (r, c_from_roots(corc, r))
    return out


@pytest.mark.parametrize("small_leaf", [False, True])
def test_from_roots_matches_oracle(ctx, roots_and_z, small_leaf):
    for n, (r, want) in roots_and_z.items():
        if small_leaf and n < 63:
            continue
        got = ctx.poly_from_roots(r, small_leaf=small_leaf)
        assert got.size == (n + 1 if n else 0), n
        same(got, want)


@pytest.mark.parametrize("small_leaf", [False, True])
def test_from_roots_special_roots(ctx, corc, small_leaf):
    n = 200
    base = seeded(31, n)
    equal = np.full(n, base[0], dtype=np.uint64)
    special = base.copy()
    special[[0, 77, 199]] = [0, 1, P - 1]
    dup = base.copy()
    dup[7] = dup[3]
    for r in (equal, special, dup, np.zeros(n, dtype=np.uint64)):
        same(ctx.poly_from_roots(r, small_leaf=small_leaf), c_from_roots(corc, r))


@pytest.mark.parametrize("n", [(1 << 16) + 3, (1 << 18) + 1, 1 << 20])   # 2^20: no padding, a 12-stage first pass
def test_from_roots_large(ctx, corc, n):
    r = seeded(5000 + n, n)
    z = ctx.poly_from_roots(r)
    assert z.dtype == np.uint32 and z.size == n + 1 and z[-1] == 1
    pos = [0, n - 1] + [int(v) % n for v in seeded(n, 14)]
    for i in pos:
        assert c_eval(corc, z, r[i]) == 0, i
    for t in [0, 1, P - 1, int(seeded(n + 1, 1)[0])]:
        want = prod_mod((np.uint64(t) + np.uint64(P) - r) % np.uint64(P))
        assert c_eval(corc, z, t) == want, t


def test_from_roots_errors(ctx):
    import fri_amd
    with pytest.raises(fri_amd.FriError) as e:
        ctx.poly_from_roots(np.array([1, P, 3], dtype=np.uint32))
    assert e.value.code == fri_amd.FRI_EINVAL
    # out_cap = n: FRI_EINVAL with the needed length n + 1 in *len_out
    n = 10
    r = np.arange(1, n + 1, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    ln = ctypes.c_size_t(0)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = ctx.lib.fri_poly_from_roots(ctx.h, r.ctypes.data_as(u32p), n, 0, out.ctypes.data_as(u32p), n,
                                     ctypes.byref(ln))
    assert rc == fri_amd.FRI_EINVAL and ln.value == n + 1
    # an unknown flag bit
    out = np.zeros(n + 1, dtype=np.uint32)
    rc = ctx.lib.fri_poly_from_roots(ctx.h, r.ctypes.data_as(u32p), n, 2, out.ctypes.data_as(u32p), n + 1,
                                     ctypes.byref(ln))
    assert rc == fri_amd.FRI_EINVAL
    # more roots than the context holds
    small = fri_amd.Context(0, 10)
    try:
        assert small.poly_from_roots(np.arange(1024, dtype=np.uint32)).size == 1025
        with pytest.raises(fri_amd.FriError) as e:
            small.poly_from_roots(np.arange(1025, dtype=np.uint32))
        assert e.value.code == fri_amd.FRI_EINVAL
    finally:
        small.close()


# -------------------------------------------------------------- Lagrange ----
def py_basis(oracle, xs):
    n = len(xs)
    rows = oracle.gen_lagrange_polynomials([int(v) for v in xs], P)
    out = np.zeros((n, n), dtype=np.uint64)
    for i, row in enumerate(rows):
        assert len(row) <= n
        out[i, : len(row)] = row
    return out


LAGRANGE_FULL = [("n1", 1), ("n2", 2), ("n3", 3), ("n64", 64), ("n65", 65), ("n257", 257), ("dup5", None),
                 ("dup65", None)]


@pytest.mark.parametrize("name,n", LAGRANGE_FULL)
def test_lagrange_matches_oracle(ctx, oracle, name, n):
    dups = []
    if name == "dup5":
        xs = np.array([1, 2, 3, 2, 5], dtype=np.uint64)
        dups = [1, 3]
    elif name == "dup65":
        xs = distinct(65, 65)
        xs[40] = xs[11]
        dups = [11, 40]
    else:
        xs = distinct(900 + n, n)
    got = ctx.lagrange_basis(xs)
    assert got.dtype == np.uint32 and got.shape == (xs.size, xs.size)
    assert np.array_equal(got.astype(np.uint64), py_basis(oracle, xs))
    for i in dups:
        assert not got[i].any()
    if name == "n1":
        assert got.tolist() == [[1]]


def test_lagrange_empty(ctx):
    assert ctx.lagrange_basis(np.zeros(0, dtype=np.uint32)).shape == (0, 0)


@pytest.mark.parametrize("n", [1024, 4096])
def test_lagrange_large(ctx, corc, n):
    xs = distinct(7000 + n, n)
    L = ctx.lagrange_basis(xs)
    assert L.dtype == np.uint32 and L.shape == (n, n)
    assert int(L.max()) < P
    # sum_i L_i = 1: every stored word enters a column sum (n values < 2^32: no 64-bit overflow)
    cols = L.sum(axis=0, dtype=np.uint64) % np.uint64(P)
    want = np.zeros(n, dtype=np.uint64)
    want[0] = 1
    assert np.array_equal(cols, want)
    z = ctx.poly_from_roots(xs)
    zc = c_from_roots(corc, xs)
    same(z, zc)
    rows = [int(v) % n for v in seeded(n + 5, 8)]
    for i in rows:
        q, r = c_div_rem(corc, zc, [(P - int(xs[i])) % P, 1])
        assert r.size == 0 and q.size == n
        d = prod_mod(np.delete((xs[i] + np.uint64(P) - xs) % np.uint64(P), i))
        w = pow(d, P - 2, P)
        assert np.array_equal(L[i].astype(np.uint64), (q * np.uint64(w)) % np.uint64(P)), i   # q, w < 2^32
    pairs = [(int(a) % n, int(b) % n) for a, b in seeded(n + 6, 24).reshape(12, 2)] + [(i, i) for i in rows[:4]]
    for i, j in pairs:
        assert c_eval(corc, L[i], xs[j]) == (1 if i == j else 0), (i, j)


def test_lagrange_errors(ctx):
    import fri_amd
    with pytest.raises(fri_amd.FriError) as e:
        ctx.lagrange_basis(np.arange(fri_amd.LAGRANGE_MAX + 1, dtype=np.uint32))
    assert e.value.code == fri_amd.FRI_EINVAL
    u32p = ctypes.POINTER(ctypes.c_uint32)
    xs = np.arange(1, 9, dtype=np.uint32)
    out = np.zeros(63, dtype=np.uint32)
    assert ctx.lib.fri_lagrange_basis(ctx.h, xs.ctypes.data_as(u32p), 8, out.ctypes.data_as(u32p), 63) == \
        fri_amd.FRI_EINVAL
    with pytest.raises(fri_amd.FriError) as e:
        ctx.lagrange_basis(np.array([1, 2, P], dtype=np.uint32))
    assert e.value.code == fri_amd.FRI_EINVAL


def test_lagrange_consistent_with_interpolate_points(ctx):
    n = 257
    xs = distinct(4242, n)
    ys = seeded(4243, n)
    L = ctx.lagrange_basis(xs).astype(np.uint64)
    acc = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        acc = (acc + (L[i] * ys[i]) % np.uint64(P)) % np.uint64(P)
    want = np.zeros(n, dtype=np.uint64)
    f = ctx.interpolate_points(xs, ys)
    want[: f.size] = f
    assert np.array_equal(acc, want)


def test_module_level_functions(ctx, corc):
    import fri_amd
    assert fri_amd.gen_lagrange_polynomials_parallel is fri_amd.gen_lagrange_polynomials
    r = seeded(11, 130)
    same(fri_amd.gen_polynomial_from_roots(r, ctx=ctx), c_from_roots(corc, r))
    xs = np.array([1, 2, 3, 2, 5], dtype=np.uint32)
    assert np.array_equal(fri_amd.gen_lagrange_polynomials(xs, ctx=ctx), ctx.lagrange_basis(xs))
