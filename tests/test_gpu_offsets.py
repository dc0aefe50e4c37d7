"""GPU: the batched commit and the provers off the default coset.

Every accepted call of the batch family elsewhere in the suite runs at offset
5.  Here fri_commit_batch, the batch's table cache (batch_tables, keyed by
log_n and offset), fri_trace_commit_batch, fri_fibsq_composition_commit_batch
and the three prover routes run at other offsets, and every output is compared
with tests/prover_model.py (the C oracle and the Python twin; anchored on the
CPU by tests/test_prover_model_host.py), never with another device path.

The shapes are the smallest at which a path changes: n = 8 (the composition
lane's wrap), L = 9 / 10 (the tile boundary, the first tiled tree), L = 12 (the
last LDS transform), L = 13 (the first batched transform and the first L with
two entries in the high power table), and (13, 1): the trace's interpolation
through the batched transform, with a one-element last layer."""
import ctypes
import hashlib

import numpy as np
import pytest

import prover_model as pm

pytestmark = pytest.mark.gpu

import fri_amd  # noqa: E402

P = fri_amd.P
FRI_EINVAL = fri_amd.FRI_EINVAL
SHAPES = [(2, 1), (6, 3), (7, 3), (9, 3), (10, 3), (13, 1)]
A1S = [3141592, 7, P - 2]
OFFSET_NAMES = ["7", "p-2", "big", "w_2n"]


def _state(tag):
    return hashlib.sha256(tag).digest()


def _batch_member(ctx, b, model, log_n, what):
    pm.assert_result(ctx.batch_results[b], lambda k: ctx.batch_layer(b, k, log_n), model, fri_amd.CommitResult,
                     (what, b))


# ---- 1. fri_commit_batch off the default coset -------------------------------------
def _plain_batch(ctx, corc, oracle, log_n, offset, seed):
    n = 1 << log_n
    ds = [1, 2, n // 8, n // 8 + 1]
    polys = [oracle.splitmix64_np(seed + b, d) for b, d in enumerate(ds)]
    states = [None if b == 0 else _state(b"plain %d" % b) for b in range(len(ds))]
    res = ctx.commit_batch([p.astype(np.uint32) for p in polys], log_n, offset, channel_states=states)
    assert ctx.batch_status == [0] * len(ds)
    models = [pm.plain_commit(corc, oracle, p, log_n, offset, st.hex() if st else "") for p, st in zip(polys, states)]
    for b, m in enumerate(models):
        _batch_member(ctx, b, m, log_n, ("commit_batch", log_n, offset))
    return res


@pytest.mark.parametrize("offset", [1, 7, P - 1, pm.BIG_OFFSET], ids=["1", "7", "p-1", "big"])
@pytest.mark.parametrize("log_n", [3, 9, 12, 13])
def test_commit_batch_off_the_default_coset(ctx, corc, oracle, log_n, offset):
    res = _plain_batch(ctx, corc, oracle, log_n, offset, 40)
    if log_n > 3:
        assert len({r.n_layers for r in res}) > 1           # members of mixed degree end at different layers


# ---- 2. the table cache -------------------------------------------------------------
def _fibsq_batch(ctx, corc, oracle, log_t, lb, offset):
    """trace and composition batch of three valid members with given alphas,
    a coset interpolation at a third offset between the two calls (the batch's
    inverse transform shares the context's power tables with it)."""
    L = log_t + lb
    traces = [pm.recurrence_trace(1, a1, 1 << log_t) for a1 in A1S]
    alphas = [[11 + b, 22 + b, 33 + b] for b in range(3)]
    states = [_state(b"fibsq %d" % b) for b in range(3)]
    got = ctx.trace_commit_batch(np.stack(traces).astype(np.uint32), lb, offset)
    ys = oracle.splitmix64_np(77, 1 << L)
    pm.same(ctx.interpolate(ys.astype(np.uint32), 11), pm.interpolate_coset(corc, ys, L, 11), "interpolate at 11")
    ctx.fibsq_composition_commit_batch(log_t, lb, [int(t[-1]) for t in traces], alphas, offset, channel_states=states)
    assert ctx.batch_status == [0, 0, 0]
    for b in range(3):
        m = pm.commit(corc, oracle, traces[b], log_t, lb, offset, int(traces[b][-1]), alphas[b], states[b].hex())
        pm.same(got[b].hex(), m.tr.root.hex(), (log_t, lb, offset, b, "trace root"))
        _batch_member(ctx, b, m, L, ("composition", log_t, lb, offset))


def _single_commit(ctx, corc, oracle, log_n, offset):
    c = oracle.splitmix64_np(91, (1 << log_n) // 8)
    r = ctx.commit(c.astype(np.uint32), log_n, offset)
    pm.assert_result(r, lambda k: ctx.layer(k, log_n), pm.plain_commit(corc, oracle, c, log_n, offset),
                     fri_amd.CommitResult, ("commit", log_n, offset))


def test_plain_batch_tables_follow_the_offset(ctx, corc, oracle):
    # 5 -> 7 -> 5 at one log_n, 7 at another log_n and back; single commits at a third offset between
    for step, (log_n, offset) in enumerate([(9, 5), (9, 7), (9, 5), (13, 7), (9, 7), (13, 5), (13, 7), (9, 5)]):
        _plain_batch(ctx, corc, oracle, log_n, offset, 60 + step)
        if step % 2:
            _single_commit(ctx, corc, oracle, log_n, 11)


def test_prover_batch_tables_follow_the_offset(ctx, corc, oracle):
    for step, (log_t, lb, offset) in enumerate([(6, 3, 5), (6, 3, 7), (6, 3, 5), (10, 3, 7), (6, 3, 7), (10, 3, 5),
                                                (10, 3, 7)]):
        _fibsq_batch(ctx, corc, oracle, log_t, lb, offset)
        if step % 2:
            _single_commit(ctx, corc, oracle, log_t + lb, 11)
    # a plain batch and a prover batch share the tables too
    _plain_batch(ctx, corc, oracle, 13, 5, 80)
    _fibsq_batch(ctx, corc, oracle, 10, 3, 7)
    _plain_batch(ctx, corc, oracle, 13, 7, 81)
    _fibsq_batch(ctx, corc, oracle, 10, 3, 5)


# ---- 3. the provers at the accepted offsets ----------------------------------------
_MODELS = {}


def _proofs(corc, oracle, log_t, lb, offset):
    key = (log_t, lb, offset)
    if key not in _MODELS:
        _MODELS[key] = [pm.prove(corc, oracle, pm.recurrence_trace(1, a1, 1 << log_t), log_t, lb, offset, 2,
                                 state=_state(b"prover %d" % b).hex() if b else "") for b, a1 in enumerate(A1S)]
    return _MODELS[key]


@pytest.mark.parametrize("route", ["single", "round", "device"])
@pytest.mark.parametrize("which", range(4), ids=OFFSET_NAMES)
@pytest.mark.parametrize("log_t,lb", SHAPES)
def test_provers_at_the_accepted_offsets(ctx, corc, oracle, log_t, lb, which, route):
    offset = pm.accepted_offsets(log_t, lb)[which]
    want = _proofs(corc, oracle, log_t, lb, offset)
    chans = [fri_amd.Channel(state=_state(b"prover %d" % b).hex() if b else "") for b in range(3)]
    if route == "single":
        proofs = [fri_amd.prove_fibsq(a1, log_t, lb, 2, ch, offset, ctx=ctx) for a1, ch in zip(A1S, chans)]
    else:
        proofs = fri_amd.prove_fibsq_batch(A1S, log_t, lb, 2, chans, offset, ctx=ctx, device_queries=route == "device")
    for b, (pr, ch, w) in enumerate(zip(proofs, chans, want)):
        m = w.model
        pm.same(pr.trace_root.hex(), m.tr.root.hex(), (b, "trace root"))
        pm.same((pr.alphas, pr.a_last), (w.alphas, m.a_last), (b, "alphas, a_last"))
        pm.same([r.hex()[:16] for r in pr.fri.roots], [r.hex()[:16] for r in pm.roots(m)], (b, "roots"))
        pm.same(pr.fri.betas, pm.betas(m), (b, "betas"))
        pm.same((pr.fri.final_value, pr.fri.final_degree), (m.res.final_value, m.res.final_degree), (b, "final"))
        pm.same(pr.queries, w.queries, (b, "queries"))
        pm.same([x.hex()[:32] for x in ch.proof], [x.hex()[:32] for x in w.messages], (b, "messages"))
        assert ch.proof == w.messages, b
        pm.same(ch.state, w.state, (b, "state"))
    # the transcripts verify at their offset, and only there
    nls = [pm.n_layers(w.model) for w in want]
    a_last = [w.model.a_last for w in want]
    starts = [_state(b"prover %d" % b).hex() if b else "" for b in range(3)]
    for b, ch in enumerate(chans):
        assert fri_amd.verify_fibsq(ch.proof, a_last[b], log_t, lb, 2, nls[b], offset=offset, channel_state=starts[b]), b
        assert not fri_amd.verify_fibsq(ch.proof, a_last[b], log_t, lb, 2, nls[b], offset=5, channel_state=starts[b]), b
    reasons = []
    ok = fri_amd.verify_fibsq_batch([ch.proof for ch in chans], a_last, log_t, lb, 2, nls, offset=offset,
                                    channel_states=starts, ctx=ctx, reasons=reasons)
    assert ok == [True] * 3 and [int(r) for r in reasons] == [0, 0, 0]


@pytest.mark.parametrize("log_t,lb", SHAPES)
def test_refused_offsets(ctx, log_t, lb):
    T = 1 << log_t
    traces = np.stack([fri_amd.fibsq_trace(a1, T) for a1 in A1S])
    for offset in pm.refused_offsets(log_t, lb):
        roots = ctypes.create_string_buffer(b"\x77" * 96, 96)
        assert ctx.lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(traces), log_t, lb, offset, 3, roots) == FRI_EINVAL
        assert roots.raw == b"\x77" * 96, offset
        # the single trace commit takes any coset; the composition on it does not
        ctx.trace_commit(traces[0], lb, offset, readback=False)
        with pytest.raises(fri_amd.FriError) as e:
            ctx.fibsq_composition_commit(log_t, lb, int(traces[0, -1]), [1, 2, 3], offset)
        assert e.value.code == FRI_EINVAL, offset
