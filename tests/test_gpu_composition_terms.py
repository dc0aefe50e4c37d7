"""GPU: the composition kernels' terms and verdicts, traces that are not
FibonacciSq, and the trace openings of the batched query kernels.

k_fibsq_cp and k_fibsq_cp_batch elsewhere only see valid FibonacciSq traces
with channel-drawn alphas, and the batch only opens three trace values B apart
that never wrap.  Here one batch holds a member per isolated term, a member
whose composition is the zero polynomial, an ordinary member and four violated
ones; another holds zero, constant, all-(p-1) and random traces; and
fri_batch_query_round / fri_batch_query_phase open 1, 2 and 8 trace values at
strides from 0 to 2^63 + 5, past the end of the LDE.  Every output is compared
with tests/prover_model.py (inputs and model pinned on the CPU by
tests/test_prover_model_host.py), never with another device path."""
import numpy as np
import pytest

import prover_model as pm

pytestmark = pytest.mark.gpu

import fri_amd  # noqa: E402

P = fri_amd.P
FRI_EDEGREE = fri_amd.FRI_EDEGREE
VAL_FILL, PATH_FILL, IDX_FILL = 0xA5A5A5A5, 0x5A, 0x7777777777777777


def _states(count):
    return [bytes([b + 1] * 32) for b in range(count)]


def _models(corc, oracle, members, log_t, lb, offset):
    return [pm.commit(corc, oracle, m.trace, log_t, lb, offset, m.a_last, m.alphas, st.hex())
            for m, st in zip(members, _states(len(members)))]


def _commit_batch(ctx, members, log_t, lb, offset):
    """trace and composition batch of `members`: (trace roots, status); a
    failed member's FRI_EDEGREE is left in the status."""
    traces = np.stack([m.trace for m in members]).astype(np.uint32)
    roots = ctx.trace_commit_batch(traces, lb, offset)
    try:
        ctx.fibsq_composition_commit_batch(log_t, lb, [m.a_last for m in members], [m.alphas for m in members], offset,
                                           channel_states=_states(len(members)))
    except fri_amd.FriError as e:
        assert e.code == FRI_EDEGREE
    return roots, ctx.batch_status


def _check_batch(ctx, members, models, roots, status, log_t, lb):
    """Verdicts by the degree alone; every accepted member's result bytes and
    layers are the model's; a refused member serves nothing."""
    L, T = log_t + lb, 1 << log_t
    assert [m.cp_degree for m in models] == [m.degree for m in members]
    pm.same(status, [FRI_EDEGREE if m.cp_degree > T else 0 for m in models], "status")
    for b, (mem, m) in enumerate(zip(members, models)):
        pm.same(roots[b].hex(), m.tr.root.hex(), (mem.name, "trace root"))
        r = ctx.batch_results[b]
        if status[b]:
            assert bytes(r) == bytes(fri_amd.CommitResult()), mem.name
            continue
        pm.assert_result(r, lambda k: ctx.batch_layer(b, k, L), m, fri_amd.CommitResult, mem.name)


def _round_arrays(batch, tc, ml, L):
    return (np.full((batch, tc + 2 * ml), VAL_FILL, dtype=np.uint32),
            np.full((batch, 32 * L * tc + sum(64 * (L - k) for k in range(ml))), PATH_FILL, dtype=np.uint8))


def _check_round(ctx, models, served, indices, tc, stride, L):
    """One fri_batch_query_round against record(): every word and byte of every
    row, the untouched ones included."""
    ml = max(pm.n_layers(m) for m, s in zip(models, served) if s)
    values, paths = _round_arrays(len(models), tc, ml, L)
    _, _, lens = ctx.batch_query_round(indices, trace_count=tc, trace_stride=stride, values=values, paths=paths)
    for b, m in enumerate(models):
        what = (b, indices[b], tc, stride)
        if not served[b]:
            assert lens[b] == 0 and (values[b] == VAL_FILL).all() and (paths[b] == PATH_FILL).all(), what
            continue
        wv, wp = pm.record(m, indices[b], tc, stride, ml, VAL_FILL, PATH_FILL)
        pm.same(lens[b], pm.paths_len(m, tc), (what, "paths_len"))
        pm.same(values[b], wv, (what, "values"))
        pm.same(paths[b], wp, (what, "paths"))


def _check_phase(ctx, models, served, q, max_index, tc, stride, L):
    """One fri_batch_query_phase against phase(): indices, records, lengths and
    final states.  Returns the model's indices of the served members."""
    batch = len(models)
    ml = max(pm.n_layers(m) for m, s in zip(models, served) if s)
    values, paths = _round_arrays(batch * q, tc, ml, L)
    values, paths = values.reshape(batch, q, -1), paths.reshape(batch, q, -1)
    idx = np.full((batch, q), IDX_FILL, dtype=np.uint64)
    states = [bytes.fromhex(m.state) if s else bytes([0xEE] * 32) for m, s in zip(models, served)]
    _, _, _, lens, out = ctx.batch_query_phase(q, max_index, states, trace_count=tc, trace_stride=stride, indices=idx,
                                               values=values, paths=paths)
    drawn = []
    for b, m in enumerate(models):
        what = (b, tc, stride)
        if not served[b]:
            assert lens[b] == 0 and out[b] == states[b], what
            assert (idx[b] == IDX_FILL).all() and (values[b] == VAL_FILL).all() and (paths[b] == PATH_FILL).all(), what
            continue
        want = pm.phase(m, m.state, q, max_index, tc, stride, ml, VAL_FILL, PATH_FILL)
        pm.same([int(i) for i in idx[b]], want.indices, (what, "indices"))
        pm.same(lens[b], pm.paths_len(m, tc), (what, "paths_len"))
        for r, (wv, wp) in enumerate(want.records):
            pm.same(values[b, r], wv, (what, "values of query", r))
            pm.same(paths[b, r], wp, (what, "paths of query", r))
        pm.same(out[b].hex(), want.state, (what, "state"))
        drawn += want.indices
    return drawn


# ---- 1. the composition's terms and verdicts ---------------------------------------
@pytest.mark.parametrize("offset", [5, 7])
@pytest.mark.parametrize("log_t,lb", [(4, 2), (6, 3), (10, 3)])
def test_terms_and_verdicts(ctx, corc, oracle, log_t, lb, offset):
    L, T, B = log_t + lb, 1 << log_t, 1 << lb
    n = 1 << L
    members = pm.isolated_members(log_t) + [pm.ordinary_member(log_t)] + pm.violated_members(log_t, lb)
    models = _models(corc, oracle, members, log_t, lb, offset)
    states = _states(len(members))
    # the single pair, member by member
    for mem, m, st in zip(members, models, states):
        root, coeffs, lde = ctx.trace_commit(mem.trace.astype(np.uint32), lb, offset)
        pm.same(root.hex(), m.tr.root.hex(), (mem.name, "trace root"))
        pm.same(coeffs, m.tr.coeffs, (mem.name, "trace coefficients"))
        pm.same(lde, m.tr.lde, (mem.name, "trace LDE"))
        if m.cp_degree > T:
            with pytest.raises(fri_amd.FriError) as e:
                ctx.fibsq_composition_commit(log_t, lb, mem.a_last, mem.alphas, offset, channel_state=st)
            assert e.value.code == FRI_EDEGREE, mem.name
            continue
        r = ctx.fibsq_composition_commit(log_t, lb, mem.a_last, mem.alphas, offset, channel_state=st)
        pm.assert_result(r, lambda k: ctx.layer(k, L), m, fri_amd.CommitResult, mem.name)
    # the degree decides: the violated traces with the recurrence's alpha alone
    rec = pm.recurrence_only(log_t, lb)
    rec_models = _models(corc, oracle, rec, log_t, lb, offset)
    roots, status = _commit_batch(ctx, rec, log_t, lb, offset)
    assert [s == 0 for s in status] == [m.name in pm.BOUNDARY_ONLY for m in rec]
    _check_batch(ctx, rec, rec_models, roots, status, log_t, lb)
    # the batch: FRI_EDEGREE exactly for the four violated members
    roots, status = _commit_batch(ctx, members, log_t, lb, offset)
    assert status == [0] * 5 + [FRI_EDEGREE] * 4
    _check_batch(ctx, members, models, roots, status, log_t, lb)
    assert len({pm.n_layers(m) for m in models[:5]}) > 1         # the accepted members end at different layers
    assert pm.n_layers(models[3]) == 1                           # ... the zero composition after one
    # the queries over that batch: failed members left out and untouched
    served = [s == 0 for s in status]
    _check_round(ctx, models, served, [(37 * b + 3) % (n - 2 * B) for b in range(9)], 3, B, L)
    _check_round(ctx, models, served, [n - 1 - b for b in range(9)], 0, 0, L)
    _check_phase(ctx, models, served, 2, n - 2 * B - 1, 3, B, L)
    _check_phase(ctx, models, served, 2, (1 << 32) - 1, 0, 0, L)


# ---- 2. traces that are not FibonacciSq, and the trace openings --------------------
def _trace_members(log_t):
    """zero, constant, all-(p-1) and two random traces, accepted through the
    last-row term alone (alphas (0, a, 0), a_last = the last row: a constant
    trace's composition is the zero polynomial), and a valid FibonacciSq member."""
    T = 1 << log_t
    out = []
    for name, t in (("zero", np.zeros(T, dtype=np.uint64)), ("constant", np.full(T, 12345, dtype=np.uint64)),
                    ("all_p_minus_1", np.full(T, P - 1, dtype=np.uint64)), ("random_a", pm.random_trace(501, T)),
                    ("random_b", pm.random_trace(502, T))):
        out.append(pm.Member(name, t, int(t[-1]), [0, 99, 0], -1 if name[0] != "r" else T - 2))
    return out + [pm.ordinary_member(log_t)]


@pytest.mark.parametrize("log_t,lb", [(2, 1), (4, 2), (6, 3)])
def test_trace_openings(ctx, corc, oracle, log_t, lb):
    L, B, offset = log_t + lb, 1 << lb, 7
    n = 1 << L
    members = _trace_members(log_t)
    models = _models(corc, oracle, members, log_t, lb, offset)
    roots, status = _commit_batch(ctx, members, log_t, lb, offset)
    assert status == [0] * 6
    _check_batch(ctx, members, models, roots, status, log_t, lb)
    served = [True] * 6
    for tc in (1, 2, 8):
        for stride in (0, 1, B, n - 1, n, n + 3, (1 << 63) + 5):
            _check_round(ctx, models, served, [0 if b % 2 else n - 1 for b in range(6)], tc, stride, L)
            _check_round(ctx, models, served, [n - 1 if b % 2 else 0 for b in range(6)], tc, stride, L)
    # prove_fibsq's openings with the draw up to the last index: index + 2B wraps
    drawn = _check_phase(ctx, models, served, 16, n - 1, 3, B, L)
    assert any(i + 2 * B >= n for i in drawn)
    for tc in (1, 8):
        for stride in (1, n + 3):
            _check_phase(ctx, models, served, 2, n - 1, tc, stride, L)
