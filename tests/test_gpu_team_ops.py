"""GPU: the kernel-level entry points on a team context (fri_ctx_create_multi),
word for word against the C oracle.

include/fri_amd.h gives a team context the caller's log_n_max: the kernel-level
calls (fri_lde, fri_interpolate, fri_fold, fri_merkle_root, fri_batch_inverse,
fri_evaluate, fri_trace_commit, fri_fibsq_composition_commit) run on rank 0 and
take every size up to 2^log_n_max, although the other ranks hold only a shard.
The shapes (G, L) are the smallest on each branch of the ranks' shard bound
sub = max(L - log2 G, min(L, 19)): (2, 20) takes min(L, 19), (2, 21) and (4, 22)
take L - log2 G; each call runs at 2^L, above every rank's shard.  Every rank
sits on GPU 0 (peer transport), one context per shape.

Every expected value is the oracle's (orc_lde, orc_interpolate_coset,
orc_fold_eval, orc_merkle_build, orc_batch_inverse, orc_poly_evaluate,
orc_fibsq_prove_commit, orc_fri_commit_fast), never another GPU context's, and
exact: integer field arithmetic and SHA-256 have no tolerance.  The oracle's
results are computed once per shape and shared by the tests that need them."""
import functools

import numpy as np
import pytest

import stored_proof as sp
from prover_check import oracle_fibsq_commit
from test_gpu_tier_sweep import (P, _p, _u32, c_interpolate_coset, c_lde, c_merkle_nodes, horner_all, merkle_values,
                                 same, seeded)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 20), (2, 21), (4, 22)]


def shard_bound(G, L):
    """log2 of what ranks 1..G-1 hold (include/fri_amd.h, fri_ctx_create_multi)."""
    return max(L - (G.bit_length() - 1), min(L, 19))


@pytest.fixture(scope="module", params=SHAPES, ids=[f"G{G}-L{L}" for G, L in SHAPES])
def team(request):
    import fri_amd
    G, L = request.param
    cx = fri_amd.Context.multi([0] * G, L, transport="peer")
    yield G, L, cx
    cx.close()


@functools.lru_cache(maxsize=None)
def lde_case(L, blowup_log):
    """(coefficients, the oracle's LDE on 5 * <w_{2^L}>): d = 2^L >> blowup_log, c[0] = 0, c[d-1] = p - 1."""
    import fri_oracle as fo
    d = (1 << L) >> blowup_log
    c = seeded(30000 + 10 * L + blowup_log, d).copy()
    c[0] = 0
    c[d - 1] = P - 1
    return c, c_lde(fo.load_c_oracle(), c, L, 5)


@functools.lru_cache(maxsize=None)
def merkle_case(L):
    import fri_oracle as fo
    v = merkle_values(31000 + L, 1 << L)
    return v, c_merkle_nodes(fo.load_c_oracle(), v)[-32:].tobytes()


@functools.lru_cache(maxsize=None)
def inverse_case(L):
    """2^L seeded values with zeros at both ends and at a few interior positions, and the oracle's inverses."""
    import fri_oracle as fo
    n = 1 << L
    x = seeded(32000 + L, n).copy()
    x[x == 0] = 1
    for i in (0, 1, n // 3, n // 2 - 1, n // 2, (1 << (L - 1)) + 1, n - 2, n - 1):
        x[i] = 0
    x[2] = 1
    x[3] = P - 1
    want = np.empty(n, dtype=np.uint64)
    fo.load_c_oracle().orc_batch_inverse(_p(x), _p(want), n, P)
    return x, want


# ------------------------------------------------------ the entry points ----
@pytest.mark.parametrize("blowup_log", [3, 0])
def test_lde(team, blowup_log):
    G, L, cx = team
    c, want = lde_case(L, blowup_log)
    same(cx.lde(_u32(c), L), want, f"fri_lde on a team of {G}, log_n={L}, d={c.size}")


def test_interpolate(team, corc):
    """fri_interpolate of the LDE gives the coefficients back (their top one is p - 1: the full length)."""
    G, L, cx = team
    c, ys = lde_case(L, 3)
    want = c_interpolate_coset(corc, ys, L, 5)
    assert np.array_equal(want, c)
    same(cx.interpolate(_u32(ys)), want, f"fri_interpolate on a team of {G}, log_n={L}")


def test_fold(team, corc):
    G, L, cx = team
    m = 1 << L
    layer = seeded(33000 + L, m)
    l32 = _u32(layer)
    w = corc.orc_fe_pow(5, (P - 1) >> L, P)
    for beta in (int(seeded(33100 + L, 1)[0]), 0, P - 1):
        want = np.empty(m // 2, dtype=np.uint64)
        corc.orc_fold_eval(_p(layer), m, 5, w, beta, P, _p(want))
        same(cx.fold(l32, 5, beta), want, f"fri_fold on a team of {G}, log_m={L}, beta={beta}")


def test_merkle_root(team, corc):
    """2^L leaves, and 2^(L-1) + 1: ragged, and just above a shard-sized bound."""
    G, L, cx = team
    v, root = merkle_case(L)
    assert cx.merkle_root(_u32(v)) == root, f"fri_merkle_root on a team of {G}, n=2^{L}"
    n = (1 << (L - 1)) + 1
    v = merkle_values(31500 + L, n)
    assert cx.merkle_root(_u32(v)) == c_merkle_nodes(corc, v)[-32:].tobytes(), \
        f"fri_merkle_root on a team of {G}, n={n}"


def test_batch_inverse(team):
    G, L, cx = team
    x, want = inverse_case(L)
    same(cx.batch_inverse(_u32(x)), want, f"fri_batch_inverse on a team of {G}, n=2^{L}")


def test_evaluate(team, corc):
    G, L, cx = team
    c = seeded(34000 + L, 1 << L)
    xs = np.array([1, P - 1, int(seeded(34100 + L, 1)[0])], dtype=np.uint64)
    same(cx.evaluate(_u32(c), _u32(xs)), horner_all(corc, c, xs), f"fri_evaluate on a team of {G}, d=2^{L}, 3 points")


def test_trace_and_composition_commit(team, corc, oracle):
    """fri_trace_commit and fri_fibsq_composition_commit at log_t = L - 3,
    blowup 8: trace root, LDE and the FRI transcript of the composition
    polynomial against orc_fibsq_prove_commit."""
    import fri_amd
    G, L, cx = team
    a1, log_t, lb = 3141592, L - 3, 3
    och, root, alphas, res, fe, _, _, _ = oracle_fibsq_commit(corc, oracle, a1, log_t, lb)
    trace = fri_amd.fibsq_trace(a1, 1 << log_t)
    got_root, _, lde = cx.trace_commit(trace, lb)
    assert got_root == root, f"fri_trace_commit on a team of {G}, log_t={log_t}: root"
    same(lde, fe, f"fri_trace_commit on a team of {G}, log_t={log_t}: LDE")
    ch = fri_amd.Channel()
    ch.send(root.hex().encode())
    assert [ch.receive_random_field_element() for _ in range(3)] == alphas
    out = cx.fibsq_composition_commit(log_t, lb, int(trace[-1]), alphas, channel_state=bytes.fromhex(ch.state))
    want = ([bytes(res.roots[k]) for k in range(res.n_layers)], [int(res.betas[k]) for k in range(res.n_rounds)],
            int(res.final_value), int(res.final_degree), och.state.decode())
    assert sp.transcript_of(out) == want, f"fri_fibsq_composition_commit on a team of {G}, log_t={log_t}"
    assert out.n_rounds == log_t + 1


# --------------------------------------------------- what still refuses ----
def _refused(call):
    import fri_amd
    with pytest.raises(fri_amd.FriError) as e:
        call()
    assert e.value.code == fri_amd.FRI_EINVAL, e.value
    return True


def test_above_log_n_max_is_refused(team):
    G, L, cx = team
    assert _refused(lambda: cx.lde(np.arange(8, dtype=np.uint32), L + 1))


def test_bound_is_the_callers_log_n_max(team):
    """A team created for 2^(L-1) refuses 2^L at every entry point: rank 0
    takes what its creator asked for, not anything."""
    import fri_amd
    G, L, _ = team
    n = 1 << L
    small = fri_amd.Context.multi([0] * G, L - 1)
    try:
        ones = np.ones(n, dtype=np.uint32)
        assert _refused(lambda: small.lde(ones[:8], L))
        assert _refused(lambda: small.interpolate(ones))
        assert _refused(lambda: small.fold(ones, 5, 1))
        assert _refused(lambda: small.merkle_root(ones))
        assert _refused(lambda: small.merkle_root(ones[: n // 2 + 1]))
        assert _refused(lambda: small.evaluate(ones, ones[:3]))
        assert _refused(lambda: small.trace_commit(fri_amd.fibsq_trace(5, n >> 3), 3, readback=False))
        assert small.merkle_root(ones[: n // 2]) == c_merkle_root_of_ones(n // 2)
    finally:
        small.close()


@functools.lru_cache(maxsize=None)
def c_merkle_root_of_ones(n):
    import fri_oracle as fo
    return c_merkle_nodes(fo.load_c_oracle(), np.ones(n, dtype=np.uint64))[-32:].tobytes()


def test_other_ranks_keep_the_shard_bound(team):
    G, L, cx = team
    sub = shard_bound(G, L)
    assert sub < L
    r1 = cx.team_rank(1)
    assert _refused(lambda: r1.lde(np.arange(8, dtype=np.uint32), sub + 1))
    assert _refused(lambda: r1.merkle_root(np.ones((1 << sub) + 1, dtype=np.uint32)))


# ------------------------- kernel-level calls beside a resident sharded commit ----
def test_resident_sharded_commit_survives_kernel_level_calls(team, corc, oracle, oracle_commit):
    """A sharded commit of 2^L stays readable while fri_lde, fri_merkle_root
    and fri_batch_inverse run at 2^L on the same context (rank 0's scratch is
    theirs, the plan's layers and trees are not), and the team commits the next
    polynomial correctly afterwards."""
    from test_dist import check_transport_schedule
    from test_gpu_stored_proof import _check_query
    G, L, cx = team
    n = 1 << L
    coeffs = oracle.splitmix64_np(35000 + L, n >> 3).astype(np.uint32)
    full = sp.oracle_commit_full(corc, oracle, coeffs, L)
    res = cx.commit(coeffs, L)
    assert sp.transcript_of(res) == sp.transcript_want(full)
    assert cx.team_rank(1).transport_log(), "the commit did not run sharded"
    c, lde = lde_case(L, 3)
    same(cx.lde(_u32(c), L), lde, f"fri_lde beside a resident commit, team of {G}, log_n={L}")
    v, root = merkle_case(L)
    assert cx.merkle_root(_u32(v)) == root
    x, inv = inverse_case(L)
    same(cx.batch_inverse(_u32(x)), inv, f"fri_batch_inverse beside a resident commit, team of {G}, n=2^{L}")
    for index in (n // 2 + 1, int(seeded(35100 + L, 1)[0]) % n):
        _check_query(cx, full, L, index)
    for k in (0, 1):
        msg = sp.value_report(k, L, cx.layer(k, L), full.values[k])
        assert msg is None, msg
    seed = 36 + L
    got = cx.commit(oracle.splitmix64_np(seed, n >> 3).astype(np.uint32), L)
    want = oracle_commit(L, seed)
    roots, betas, final_value, final_degree, state = sp.transcript_of(got)
    assert {"roots": [r.hex() for r in roots], "betas": betas, "final_value": final_value,
            "final_degree": final_degree, "state": state} == want
    check_transport_schedule([cx.team_rank(r).transport_log() for r in range(G)])
