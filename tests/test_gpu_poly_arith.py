"""GPU: fri_poly_mul / fri_poly_div_rem / fri_poly_compose (Polynomial::
mul_assign, div_rem, compose; src/polynomial/ops.rs:114-237) through the
Python mirror, bit-exact against the oracle.

Operands up to 2^12 (+1) coefficients are compared coefficient by coefficient
with the C oracle's schoolbook orc_poly_mul / orc_poly_div_rem; above that the
tests check the exact lengths and the identities (ab)(x) = a(x) b(x),
a(x) = q(x) b(x) + r(x), (p o q)(x) = p(q(x)) with orc_poly_evaluate at 16
seeded points that include 0, 1 and p - 1.  No tolerances: field arithmetic
is exact and quotient and remainder are unique."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 3221225473
FULL_MAX = 4097          # schoolbook comparison up to this many coefficients per operand

_P64 = ctypes.POINTER(ctypes.c_uint64)


def _c64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _p(a):
    return a.ctypes.data_as(_P64)


def rnd(seed, n):
    """n seeded coefficients, the top one nonzero (a polynomial of exactly n)."""
    import fri_oracle as fo
    a = fo.splitmix64_np(seed, n)
    if n and a[-1] == 0:
        a[-1] = 1
    return a


def c_mul(corc, a, b):
    a, b = _c64(a), _c64(b)
    out = np.zeros(max(1, a.size + b.size), dtype=np.uint64)
    n = corc.orc_poly_mul(_p(a), a.size, _p(b), b.size, _p(out), P)
    return out[:n]


def c_div_rem(corc, a, b):
    a, b = _c64(a), _c64(b)
    q = np.zeros(max(1, a.size), dtype=np.uint64)
    r = np.zeros(max(1, a.size), dtype=np.uint64)
    lq, lr = ctypes.c_size_t(), ctypes.c_size_t()
    assert corc.orc_poly_div_rem(_p(a), a.size, _p(b), b.size, _p(q), ctypes.byref(lq), _p(r), ctypes.byref(lr),
                                 P) == 0
    return q[: lq.value], r[: lr.value]


def c_eval(corc, c, x):
    c = _c64(c)
    return int(corc.orc_poly_evaluate(_p(c), c.size, int(x), P))


@pytest.fixture(scope="module")
def points():
    import fri_oracle as fo
    return [0, 1, P - 1] + [int(v) for v in fo.splitmix64_np(777, 13)]


def same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.uint32
    assert got.size == len(want), (got.size, len(want))
    assert np.array_equal(got.astype(np.uint64), _c64(want))


def check_mul(ctx, corc, points, a, b, force=None):
    got = ctx.poly_mul(a, b, force=force)
    assert got.dtype == np.uint32
    if max(len(a), len(b)) <= FULL_MAX:
        same(got, c_mul(corc, a, b))
    else:
        assert got.size == len(a) + len(b) - 1 and got[-1] != 0
        for x in points:
            assert c_eval(corc, got, x) == c_eval(corc, a, x) * c_eval(corc, b, x) % P, x
    return got


def check_div_rem(ctx, corc, points, a, b):
    q, r = ctx.poly_div_rem(a, b)
    assert q.dtype == np.uint32 and r.dtype == np.uint32
    la, lb = len(a), len(b)                     # callers pass trimmed operands
    if la <= 2 * FULL_MAX:
        wq, wr = c_div_rem(corc, a, b)
        same(q, wq)
        same(r, wr)
    else:
        assert q.size == la - lb + 1 and q[-1] != 0
        assert r.size < lb and (r.size == 0 or r[-1] != 0)
        for x in points:
            assert c_eval(corc, a, x) == (c_eval(corc, q, x) * c_eval(corc, b, x) + c_eval(corc, r, x)) % P, x
    return q, r


# ------------------------------------------------------------------- mul ----
def _split(total):
    la = total // 2 + 1
    return la, total - la + 1


MUL_SHAPES = [_split((1 << k) + d) for k in (1, 6, 8, 13, 16) for d in (-1, 0, 1)]
MUL_SHAPES += [(1, 1), (1, 5000), (5000, 1), (4096, 4096), (1 << 16, 1 << 16)]
MUL_SHAPES = list(dict.fromkeys(MUL_SHAPES))


@pytest.mark.parametrize("la,lb", MUL_SHAPES)
def test_mul_shapes(ctx, corc, points, la, lb):
    """la + lb - 1 = 2^k - 1, 2^k, 2^k + 1: the first sizes at which a cyclic
    wrap-around or a switch of the transform path would show."""
    check_mul(ctx, corc, points, rnd(la, la), rnd(1000 + lb, lb))


def test_mul_zero_and_trailing_zeros(ctx, corc):
    a = rnd(1, 100)
    assert ctx.poly_mul(a, []).size == 0                           # ops.rs:115-121
    assert ctx.poly_mul([], a).size == 0
    assert ctx.poly_mul([], []).size == 0
    assert ctx.poly_mul(a, [0, 0, 0]).size == 0                    # an operand of trailing zeros only
    assert ctx.poly_mul(np.zeros(7, dtype=np.uint32), a).size == 0
    padded_a = np.concatenate([a, np.zeros(29, dtype=np.uint64)])  # trimmed first, as Polynomial::new does
    b = rnd(2, 31)
    padded_b = np.concatenate([b, np.zeros(3, dtype=np.uint64)])
    same(ctx.poly_mul(padded_a, padded_b), c_mul(corc, a, b))
    # the top coefficient is lead(a) * lead(b) != 0: the full la + lb - 1 come back
    got = ctx.poly_mul([5, 0, P - 1], [7, P - 2])
    same(got, c_mul(corc, [5, 0, P - 1], [7, P - 2]))
    assert got.size == 4 and got[-1] == (P - 1) * (P - 2) % P


def test_mul_direct_threshold(ctx, corc, points):
    """The short operand at 1, 2, POLY_DIRECT_MAX and POLY_DIRECT_MAX + 1 (the
    first length that takes the transforms), against a long operand that
    spans several workgroups of the direct kernel."""
    import fri_amd
    a = rnd(3, 3000)
    for ls in (1, 2, fri_amd.POLY_DIRECT_MAX, fri_amd.POLY_DIRECT_MAX + 1):
        b = rnd(10 + ls, ls)
        check_mul(ctx, corc, points, a, b)
        check_mul(ctx, corc, points, b, a)


@pytest.mark.parametrize("la,lb", [(1, 1), (2, 1), (300, 2), (3000, 64), (257, 257), (5000, 1000), (4096, 4096),
                                   (70000, 4096)])
def test_mul_forced_paths_agree(ctx, corc, points, la, lb):
    a, b = rnd(20 + la, la), rnd(30 + lb, lb)
    d = check_mul(ctx, corc, points, a, b, force="direct")
    n = check_mul(ctx, corc, points, a, b, force="ntt")
    assert np.array_equal(d, n)
    assert np.array_equal(ctx.poly_mul(b, a, force="direct"), d)


def test_mul_errors(ctx):
    import fri_amd
    lim = fri_amd.POLY_DIRECT_LIMIT
    a, b = rnd(4, lim + 1), rnd(5, lim + 1)
    with pytest.raises(fri_amd.FriError) as e:                     # beyond the direct kernel's hard limit
        ctx.poly_mul(a, b, force="direct")
    assert e.value.code == fri_amd.FRI_EINVAL
    assert ctx.poly_mul(a, b[:lim], force="direct").size == 2 * lim
    bad = np.array([1, 2, P], dtype=np.uint32)
    for x, y in ((bad, [1, 2]), ([1, 2], bad)):
        with pytest.raises(fri_amd.FriError) as e:                 # a value >= p
            ctx.poly_mul(x, y)
        assert e.value.code == fri_amd.FRI_EINVAL
    small = fri_amd.Context(0, 12)
    try:
        assert small.poly_mul(rnd(6, 2049), rnd(7, 2048)).size == 4096
        with pytest.raises(fri_amd.FriError) as e:                 # next_pow2(la + lb - 1) > 2^log_n_max
            small.poly_mul(rnd(6, 2049), rnd(7, 2049))
        assert e.value.code == fri_amd.FRI_EINVAL
        with pytest.raises(fri_amd.FriError) as e:                 # ... on the direct path too
            small.poly_mul(rnd(6, 4096), rnd(7, 2))
        assert e.value.code == fri_amd.FRI_EINVAL
    finally:
        small.close()
    # an output capacity that is too small: FRI_EINVAL and the needed length
    x, y = fri_amd._u32([1, 2, 3]), fri_amd._u32([4, 5])
    out = np.empty(3, dtype=np.uint32)
    ln = ctypes.c_size_t()
    rc = ctx.lib.fri_poly_mul(ctx.h, fri_amd._ptr(x), 3, fri_amd._ptr(y), 2, 0, fri_amd._ptr(out), 3, ctypes.byref(ln))
    assert rc == fri_amd.FRI_EINVAL and ln.value == 4


# --------------------------------------------------------------- div_rem ----
QUOT_LENS = [1, 2] + [(1 << j) + d for j in (3, 6, 11) for d in (-1, 0, 1)]


@pytest.mark.parametrize("k", QUOT_LENS)
def test_div_rem_grid(ctx, corc, points, k):
    """Quotient length k crossed with the divisor lengths 1 (a constant != 1),
    2 (x - c), 3, 64; with k = 1 the divisor is as long as the dividend."""
    for lb in (1, 2, 3, 64):
        la = k + lb - 1
        a = rnd(100 * k + lb, la)
        if lb == 1:
            b = np.array([123456789], dtype=np.uint64)
        elif lb == 2:
            b = np.array([P - 987654321, 1], dtype=np.uint64)      # x - c
        else:
            b = rnd(7 * k + lb, lb)
        q, r = check_div_rem(ctx, corc, points, a, b)
        assert q.size == k


@pytest.mark.parametrize("la", [1, 5, 64, 1000])
def test_div_rem_longer_divisor(ctx, corc, la):
    """deg a < deg b: q = 0 and r = a (ops.rs:145-147)."""
    a, b = rnd(la, la), rnd(la + 50, la + 1)
    q, r = ctx.poly_div_rem(a, b)
    assert q.size == 0
    same(r, a)
    q, r = ctx.poly_div_rem([], b)                                 # 0 / b
    assert q.size == 0 and r.size == 0


@pytest.mark.parametrize("lq,lb", [(1, 1), (9, 2), (65, 64), (300, 301), (2049, 3), (2048, 2048)])
def test_div_rem_exact(ctx, corc, lq, lb):
    """The dividend built as q * b with the oracle: q back, r of length 0."""
    q0, b = rnd(40 + lq, lq), rnd(50 + lb, lb)
    a = c_mul(corc, q0, b)
    q, r = ctx.poly_div_rem(a, b)
    same(q, q0)
    assert r.size == 0
    # operands padded with zeros are trimmed first
    q, r = ctx.poly_div_rem(np.concatenate([a, np.zeros(5, dtype=np.uint64)]),
                            np.concatenate([b, np.zeros(2, dtype=np.uint64)]))
    same(q, q0)
    assert r.size == 0


def test_div_rem_remainder_trims_and_non_monic(ctx, corc, points):
    """a = q b + r with a short r: the remainder's high coefficients vanish;
    the divisor is not monic."""
    for lq, lb, lr in ((100, 70, 3), (513, 129, 1), (33, 2000, 1000)):
        q0, b, r0 = rnd(60 + lq, lq), rnd(70 + lb, lb), rnd(80 + lr, lr)
        assert b[-1] != 1
        a = c_mul(corc, q0, b)
        a[:lr] = (a[:lr] + r0) % np.uint64(P)
        q, r = check_div_rem(ctx, corc, points, a, b)
        same(q, q0)
        same(r, r0)


def test_div_rem_vanishing_polynomial(ctx, corc, oracle):
    """The sparse x^T - 1 by (x - g^(T-2))(x - g^(T-1)), T = 2^10 (STARK-101's
    transition denominator): exact."""
    T = 1 << 10
    g = oracle.fe_pow(5, (P - 1) >> 10, P)
    gl, gp = oracle.fe_pow(g, T - 1, P), oracle.fe_pow(g, T - 2, P)
    den = ctx.poly_mul([P - gp, 1], [P - gl, 1])
    same(den, c_mul(corc, [P - gp, 1], [P - gl, 1]))
    xT1 = np.zeros(T + 1, dtype=np.uint64)
    xT1[0], xT1[T] = P - 1, 1
    q, r = ctx.poly_div_rem(xT1, den)
    wq, wr = c_div_rem(corc, xT1, den)
    same(q, wq)
    assert r.size == 0 and wr.size == 0 and q.size == T - 1


def test_div_rem_large(ctx, corc, points):
    """2^16 by 2^8 + 1 coefficients, by the identity."""
    a, b = rnd(91, 1 << 16), rnd(92, (1 << 8) + 1)
    q, r = check_div_rem(ctx, corc, points, a, b)
    assert q.size == (1 << 16) - (1 << 8)


def test_div_rem_errors(ctx):
    import fri_amd
    for b in ([], [0, 0, 0]):
        with pytest.raises(fri_amd.FriError) as e:
            ctx.poly_div_rem([1, 2, 3], b)
        assert e.value.code == fri_amd.FRI_EINVAL and "Division by zero polynomial" in str(e.value)   # ops.rs:143
    with pytest.raises(fri_amd.FriError) as e:
        ctx.poly_div_rem(np.array([P], dtype=np.uint32), [1, 1])
    assert e.value.code == fri_amd.FRI_EINVAL
    small = fri_amd.Context(0, 12)
    try:
        a = rnd(8, 4096)
        q, r = small.poly_div_rem(a[:1024], [5, 1])                # every la <= 2^(log_n_max - 2) is accepted
        assert q.size == 1023 and r.size == 1
        with pytest.raises(fri_amd.FriError) as e:                 # next_pow2(la - lb + 1) > 2^(log_n_max - 1)
            small.poly_div_rem(a, [5, 1])
        assert e.value.code == fri_amd.FRI_EINVAL
    finally:
        small.close()


# --------------------------------------------------------------- compose ----
def test_compose_edge_cases(ctx, oracle):
    """The ops.rs edge cases at p: p zero, q zero, q constant (including a
    constant that makes the result trim to zero)."""
    p = [3, 0, 2, 1]                                               # x^3 + 2 x^2 + 3
    assert ctx.poly_compose([], [1, 2]).size == 0
    assert ctx.poly_compose([0, 0], [1, 2]).size == 0
    same(ctx.poly_compose(p, []), [3])                             # p(0)
    same(ctx.poly_compose(p, [0, 0]), [3])
    same(ctx.poly_compose(p, [2]), [oracle.poly_evaluate(p, 2, P)])
    same(ctx.poly_compose([7], [1, 2, 3]), [7])                    # a constant p
    same(ctx.poly_compose([P - 4, 0, 1], [2]), [])                 # (x^2 - 4)(2) = 0: trims to zero
    same(ctx.poly_compose([0, 5], []), [])                         # 5 x at 0
    same(ctx.poly_compose([1, 1], [0, 1]), [1, 1])                 # q = x
    same(ctx.poly_compose(p, [1, 1]), oracle.poly_compose(p, [1, 1], P))


def test_compose_65_17(ctx, oracle):
    p, q = [int(v) for v in rnd(201, 65)], [int(v) for v in rnd(202, 17)]
    got = ctx.poly_compose(p, q)
    same(got, oracle.poly_compose(p, q, P))
    assert got.size == 64 * 16 + 1


def test_compose_linear(ctx, oracle):
    """f(g x), deg f = 1022: what STARK-101's transition constraint composes."""
    f = [int(v) for v in rnd(203, 1023)]
    g = oracle.fe_pow(5, (P - 1) >> 10, P)
    same(ctx.poly_compose(f, [0, g]), oracle.poly_compose(f, [0, g], P))


def test_compose_large_by_identity(ctx, corc, points):
    p, q = rnd(204, 1 << 10), rnd(205, 1 << 6)
    got = ctx.poly_compose(p, q)
    assert got.size == 1023 * 63 + 1 and got[-1] != 0
    for x in points:
        assert c_eval(corc, got, x) == c_eval(corc, p, c_eval(corc, q, x)), x


def test_compose_errors(ctx):
    import fri_amd
    small = fri_amd.Context(0, 12)
    try:
        assert small.poly_compose(rnd(9, 64), rnd(10, 66)).size == 4096
        with pytest.raises(fri_amd.FriError) as e:                 # deg p * deg q + 1 > 2^log_n_max
            small.poly_compose(rnd(9, 65), rnd(10, 66))
        assert e.value.code == fri_amd.FRI_EINVAL
        with pytest.raises(fri_amd.FriError) as e:
            small.poly_compose(np.array([1, P], dtype=np.uint32), [0, 1])
        assert e.value.code == fri_amd.FRI_EINVAL
    finally:
        small.close()


# ------------------------------------------------------------ end to end ----
def test_fibsq_composition_polynomial(ctx, oracle):
    """STARK-101 part 2 at log_t = 8 with the mirror's polynomial functions,
    composed exactly as fri_oracle.fibsq_cp_faithful composes it: the same
    coefficient list, every remainder empty."""
    import fri_amd
    log_t, T = 8, 256
    trace = oracle.fibsq_trace(3141592, T)
    f = ctx.interpolate(trace, offset=1)                           # the trace polynomial on <w_T>
    alphas = [11, 22, 33]
    want = oracle.fibsq_cp_faithful([int(v) for v in f], log_t, trace[-1], alphas)
    g = oracle.fe_pow(5, (P - 1) >> log_t, P)
    glast, gprev = oracle.fe_pow(g, T - 1, P), oracle.fe_pow(g, T - 2, P)
    x_minus = lambda c: [(P - c) % P, 1]                           # noqa: E731
    mul = lambda a, b: fri_amd.poly_mul(a, b, ctx=ctx)             # noqa: E731
    div = lambda a, b: fri_amd.poly_div_rem(a, b, ctx=ctx)         # noqa: E731
    p0, r0 = div(fri_amd.poly_sub(f, [1]), x_minus(1))
    p1, r1 = div(fri_amd.poly_sub(f, [trace[-1]]), x_minus(glast))
    f1 = fri_amd.poly_compose(f, [0, g], ctx=ctx)
    f2 = fri_amd.poly_compose(f, [0, g * g % P], ctx=ctx)
    num = fri_amd.poly_sub(fri_amd.poly_sub(f2, mul(f1, f1)), mul(f, f))
    xT1 = [P - 1] + [0] * (T - 1) + [1]
    z, rz = div(xT1, mul(x_minus(gprev), x_minus(glast)))
    p2, r2 = div(num, z)
    assert r0.size == 0 and r1.size == 0 and rz.size == 0 and r2.size == 0
    cp = np.zeros(0, dtype=np.uint32)
    for a, pk in zip(alphas, (p0, p1, p2)):
        cp = fri_amd.poly_add(cp, fri_amd.poly_scalar_mul(pk, a))
    same(cp, want)
    assert cp.size - 1 == T
