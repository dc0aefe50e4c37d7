"""GPU: the whole query phase on the device, channel included
(fri_batch_query_phase; k_query_chain and k_batch_query_all), through the
Context method and through prove_fibsq_batch / decommit_fri_batch with
device_queries=True.

A batch is never compared with itself.  The yardsticks are the C oracle
(prover_check.check_proof_matches_c_oracle, per member), the round route --
fri_batch_query_round with the host Channel (hashlib) drawing and absorbing --
and the golden transcripts."""
import hashlib
from collections import defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fri_amd  # noqa: E402

P = fri_amd.P
FRI_EINVAL, FRI_ESTATE = fri_amd.FRI_EINVAL, fri_amd.FRI_ESTATE
VAL_FILL, PATH_FILL, IDX_FILL = 0xA5A5A5A5, 0x5A, 0x7777777777777777


def _proof_sha(msgs):
    return hashlib.sha256(b"".join(len(m).to_bytes(4, "little") + m for m in msgs)).hexdigest()


# ---- 1. whole proofs by the device route, every member against the C oracle ----
@pytest.mark.parametrize("log_t,lb,members,q", [
    (2, 1, 3, 2),     # L = 3
    (2, 2, 3, 2),     # L = 4
    (6, 3, 3, 2),     # L = 9: the tile boundary
    (7, 3, 3, 2),     # L = 10: the first tiled tree
    (10, 3, 3, 2),    # L = 13: the first batched transform
    (13, 1, 3, 2),    # L = 14
    (14, 4, 2, 1),    # the cap
])
def test_device_route_matches_c_oracle(ctx, corc, oracle, log_t, lb, members, q):
    from prover_check import check_proof_matches_c_oracle
    a1s = [3141592, 7, P - 2][:members]
    chans = [fri_amd.Channel() for _ in a1s]
    proofs = fri_amd.prove_fibsq_batch(a1s, log_t, lb, q, chans, ctx=ctx, device_queries=True)
    assert [p.fri.member for p in proofs] == list(range(members))
    for a1, pr, ch in zip(a1s, proofs, chans):
        assert len(pr.queries) == q
        check_proof_matches_c_oracle(fri_amd, corc, oracle, pr, ch, a1, log_t, lb, q)


def test_golden_transcripts_as_batches(ctx, golden):
    groups = defaultdict(list)
    for c in golden["fibsq"]:
        groups[(c["log_t"], c["log_blowup"], c["queries"])].append(c)
    assert groups
    for (log_t, lb, q), cases in groups.items():
        chans = [fri_amd.Channel(state=c["channel_in"]) for c in cases]
        proofs = fri_amd.prove_fibsq_batch([c["a1"] for c in cases], log_t, lb, q, chans, ctx=ctx,
                                           device_queries=True)
        for c, pr, ch in zip(cases, proofs, chans):
            assert pr.trace_root.hex() == c["trace_root"] and pr.alphas == c["alphas"], c["name"]
            assert pr.queries == c["query_indices"], c["name"]
            assert ch.state == c["channel_out"], c["name"]
            assert len(ch.proof) == c["messages"] and _proof_sha(ch.proof) == c["proof_sha256"], c["name"]


# ---- 2. FRI only, against the round route ---------------------------------------
def _commit(ctx, polys, log_n, tag=b"member"):
    """A plain batch whose channels start from different non-empty states:
    (results, the members' states after the commit)."""
    chans = [fri_amd.Channel() for _ in polys]
    for b, ch in enumerate(chans):
        ch.send(tag + b" %d" % b)
    try:
        res = ctx.commit_batch(polys, log_n, channel_states=[bytes.fromhex(ch.state) for ch in chans])
    except fri_amd.FriError:
        res = ctx.batch_results                     # (a failed member: the others are served)
    return res, [bytes(r.channel_out.digest) if r.n_layers else bytes.fromhex(ch.state) for r, ch in zip(res, chans)]


def _arrays(B, q, log_n, max_layers, tc):
    _, vw, pb = fri_amd.verify_record_strides(log_n, max_layers, tc)
    return (np.full((B, q), IDX_FILL, dtype=np.uint64), np.full((B, q, vw), VAL_FILL, dtype=np.uint32),
            np.full((B, q, max(pb, 1)), PATH_FILL, dtype=np.uint8))


def _round_route(ctx, states, n_layers, log_n, q, max_index, skip=None, tc=0, stride=0):
    """The parent's route: per round every served member's host Channel draws
    its index, ONE fri_batch_query_round opens them, every channel hashes its
    record.  Returns what fri_batch_query_phase returns, in arrays pre-filled
    like _arrays'."""
    B = len(states)
    served = [bool(n_layers[b]) and not (skip is not None and skip[b]) for b in range(B)]
    ml = max([n_layers[b] for b in range(B) if served[b]], default=1)
    idx, values, paths = _arrays(B, q, log_n, ml, tc)
    chans = [fri_amd.Channel(state=s.hex()) for s in states]
    lens = [0] * B
    for r in range(q):
        draw = [ch.receive_random_int(0, max_index, True) if served[b] else 0 for b, ch in enumerate(chans)]
        v = np.ascontiguousarray(values[:, r])
        p = np.ascontiguousarray(paths[:, r])
        _, _, lens = ctx.batch_query_round(draw, skip=[0 if s else 1 for s in served], trace_count=tc,
                                           trace_stride=stride, values=v, paths=p)
        values[:, r], paths[:, r] = v, p
        for b, ch in enumerate(chans):
            if not served[b]:
                continue
            idx[b, r] = draw[b]
            trace, openings = fri_amd.batch_round_records(v[b], p[b], lens[b], tc, n_layers[b], log_n)
            for val, path in trace:
                ch.send(val.to_bytes(8, "big"))
                ch.send(path)
            fri_amd._send_openings(openings, ch)
    return idx, values, paths, lens if q else [0] * B, [bytes.fromhex(ch.state) for ch in chans]


def _phase_equals_round(ctx, states, n_layers, log_n, q, max_index, skip=None, what=""):
    served = [bool(n_layers[b]) and not (skip is not None and skip[b]) for b in range(len(states))]
    ml = max([n_layers[b] for b in range(len(states)) if served[b]], default=1)
    want = _round_route(ctx, states, n_layers, log_n, q, max_index, skip)
    idx, values, paths = _arrays(len(states), q, log_n, ml, 0)
    gen = ctx.batch_info()
    got = ctx.batch_query_phase(q, max_index, states, skip=skip, indices=idx, values=values, paths=paths)
    assert ctx.batch_info() == gen, what
    assert (got[0] == want[0]).all(), what                  # indices
    assert (got[1] == want[1]).all(), what                  # every value word, the untouched ones included
    assert (got[2] == want[2]).all(), what                  # every path byte
    assert got[3] == want[3] and got[4] == want[4], what    # paths_len and the final states
    return got


def _polys(oracle, seed, count, d):
    return [oracle.splitmix64_np(seed + b, d).astype(np.uint32) for b in range(count)]


@pytest.mark.parametrize("log_n,ds,q,max_index", [
    (1, [2, 2, 2], 3, 1),                   # the last layer has one element: its value is sent twice
    (1, [1, 1], 2, 5),                      # a single layer
    (3, [1, 2, 5, 8], 3, 7),                # the members differ in layer count
    (3, [1, 2, 5, 8], 2, (1 << 32) - 1),    # ... and an index far beyond the codeword
    (10, [128] * 3, 2, 1023),
    (13, [1024] * 3, 2, 8191),
])
def test_fri_only_equals_the_round_route(ctx, oracle, log_n, ds, q, max_index):
    polys = [oracle.splitmix64_np(50 + b, d).astype(np.uint32) for b, d in enumerate(ds)]
    res, states = _commit(ctx, polys, log_n)
    nls = [r.n_layers for r in res]
    if len(set(ds)) > 1:
        assert len(set(nls)) > 1
    if log_n == 1 and ds[0] == 2:
        assert nls == [2] * len(ds)
    _phase_equals_round(ctx, states, nls, log_n, q, max_index, what=(log_n, ds))


@pytest.mark.parametrize("B,q,max_index", [
    (1, 1, 0),
    (64, 2, 5),
    (65, 33, 15),               # 2^log_n - 1
    (130, 2, (1 << 32) - 1),
    (5, 0, 5),                  # no queries: nothing is written
])
def test_wave_boundaries_queries_and_ranges(ctx, oracle, B, q, max_index):
    log_n = 4
    res, states = _commit(ctx, _polys(oracle, 900, B, 4), log_n)
    got = _phase_equals_round(ctx, states, [r.n_layers for r in res], log_n, q, max_index, what=(B, q, max_index))
    if q == 0:
        assert got[3] == [0] * B and got[4] == states


# ---- 3. members left out, and the argument errors ---------------------------------
def test_skipped_and_failed_members_are_left_out(ctx, oracle):
    log_n = 6
    polys = _polys(oracle, 300, 5, 8)
    polys[2] = polys[2].copy()
    polys[2][3] = P                                          # not canonical: member 2's commit fails
    res, states = _commit(ctx, polys, log_n)
    assert ctx.batch_status[2] == FRI_EINVAL and res[2].n_layers == 0
    nls = [r.n_layers for r in res]
    skip = [0, 1, 0, 0, 0]
    idx, values, paths, lens, out = _phase_equals_round(ctx, states, nls, log_n, 3, 63, skip=skip)
    for b in (1, 2):
        assert lens[b] == 0 and out[b] == states[b]
        assert (idx[b] == IDX_FILL).all() and (values[b] == VAL_FILL).all() and (paths[b] == PATH_FILL).all()
    for b in (0, 3, 4):
        assert lens[b] == sum(64 * (log_n - k) for k in range(nls[b])) and out[b] != states[b]
    # everyone skipped: FRI_OK, nothing written
    i2, v2, p2 = _arrays(5, 2, log_n, 1, 0)
    got = ctx.batch_query_phase(2, 63, states, skip=[1] * 5, indices=i2, values=v2, paths=p2)
    assert got[3] == [0] * 5 and got[4] == states
    assert (i2 == IDX_FILL).all() and (v2 == VAL_FILL).all() and (p2 == PATH_FILL).all()


def test_argument_errors_write_nothing(ctx, oracle):
    log_n = 6
    res, states = _commit(ctx, _polys(oracle, 400, 3, 8), log_n)
    ml = max(r.n_layers for r in res)

    def refused(code, q=2, max_index=63, st=states, tc=0, arrays=None, **kw):
        idx, values, paths = arrays or _arrays(3, q, log_n, ml, tc)
        with pytest.raises(fri_amd.FriError) as e:
            ctx.batch_query_phase(q, max_index, st, trace_count=tc, indices=idx, values=values, paths=paths, **kw)
        assert e.value.code == code, str(e.value)
        assert (idx == IDX_FILL).all() and (values == VAL_FILL).all() and (paths == PATH_FILL).all()
        return str(e.value)

    refused(FRI_EINVAL, st=[states[0], None, states[2]])                 # an empty state draws nothing
    ctx.batch_query_phase(2, 63, [states[0], None, states[2]], skip=[0, 1, 0])   # ... unless its member is left out
    ctx.batch_query_phase(0, 63, [None] * 3)                             # ... or there is no query
    refused(FRI_EINVAL, max_index=1 << 32)
    refused(FRI_EINVAL, tc=9)
    assert "trace batch" in refused(FRI_ESTATE, tc=3, trace_stride=8)    # a plain batch has no trace batch behind it
    # strides too small: the needed paths stride comes back, as the round's
    small = _arrays(3, 2, log_n, ml, 0)
    small = (small[0], small[1], np.full((3, 2, 64), PATH_FILL, dtype=np.uint8))
    refused(FRI_EINVAL, arrays=small)
    assert ctx.round_needed == sum(64 * (log_n - k) for k in range(ml))
    small = _arrays(3, 2, log_n, ml, 0)
    refused(FRI_EINVAL, arrays=(small[0], np.full((3, 2, 1), VAL_FILL, dtype=np.uint32), small[2]))
    # a later single commit: no resident batch
    _phase_equals_round(ctx, states, [r.n_layers for r in res], log_n, 1, 63)   # still served after all of that
    ctx.commit([1, 2, 3], log_n)
    assert "no resident batch" in refused(FRI_ESTATE)


def test_trace_index_range_and_multi_gpu_context(ctx):
    log_t, lb, L = 4, 2, 6
    chans = [fri_amd.Channel(), fri_amd.Channel()]
    proofs = fri_amd.prove_fibsq_batch([3, 4], log_t, lb, 0, chans, ctx=ctx)
    states = [bytes.fromhex(ch.state) for ch in chans]
    idx, values, paths = _arrays(2, 1, L, proofs[0].fri.n_layers, 3)
    with pytest.raises(fri_amd.FriError) as e:               # a trace opening past the LDE
        ctx.batch_query_phase(1, 1 << L, states, trace_count=3, trace_stride=4, indices=idx, values=values,
                              paths=paths)
    assert e.value.code == FRI_EINVAL
    assert (idx == IDX_FILL).all() and (values == VAL_FILL).all() and (paths == PATH_FILL).all()
    team = fri_amd.Context.multi([0, 0], 20, transport="peer")
    try:
        with pytest.raises(fri_amd.FriError) as e:
            team.batch_query_phase(1, 5, [states[0]])
        assert e.value.code == FRI_EINVAL and "multi-GPU" in str(e.value)
    finally:
        team.close()


def test_profiling_context_refused(oracle):
    cx = fri_amd.Context(0, 12)
    try:
        res, states = _commit(cx, _polys(oracle, 500, 2, 8), 6)
        cx.set_profiling(True)
        with pytest.raises(fri_amd.FriError) as e:
            cx.batch_query_phase(1, 63, states)
        assert e.value.code == FRI_ESTATE
        cx.set_profiling(False)
        _phase_equals_round(cx, states, [r.n_layers for r in res], 6, 1, 63)
    finally:
        cx.close()


# ---- 4. chunking -------------------------------------------------------------------
def test_chunks_give_the_same_bytes(ctx, oracle):
    log_n = 7
    polys = [oracle.splitmix64_np(70 + b, d).astype(np.uint32) for b, d in enumerate([16, 16, 3, 16, 16])]
    res, states = _commit(ctx, polys, log_n)
    nls = [r.n_layers for r in res]
    one = _phase_equals_round(ctx, states, nls, log_n, 3, 127, skip=[0, 0, 0, 1, 0])
    ctx.set_query_chunk(2)
    try:
        two = _phase_equals_round(ctx, states, nls, log_n, 3, 127, skip=[0, 0, 0, 1, 0])
    finally:
        ctx.set_query_chunk(0)
    for a, b in zip(one[:3], two[:3]):
        assert (a == b).all()
    assert one[3:] == two[3:]


# ---- 5. residency ------------------------------------------------------------------
def test_the_batch_stays_resident_and_served(ctx):
    log_t, lb, L, q = 5, 3, 8, 2
    a1s = [11, 12, 13]
    want = [fri_amd.Channel() for _ in a1s]
    fri_amd.prove_fibsq_batch(a1s, log_t, lb, q, want, ctx=ctx)                  # the round route
    chans = [fri_amd.Channel() for _ in a1s]
    proofs = fri_amd.prove_fibsq_batch(a1s, log_t, lb, 0, chans, ctx=ctx)
    gen = ctx.batch_info()
    states = [bytes.fromhex(ch.state) for ch in chans]
    nl = proofs[0].fri.n_layers
    idx, values, paths, lens, out = ctx.batch_query_phase(q, (1 << L) - 2 * (1 << lb) - 1, states, trace_count=3,
                                                          trace_stride=1 << lb, max_layers=nl)
    assert ctx.batch_info() == gen
    for b, ch in enumerate(chans):
        ch.take_over_queries(fri_amd.query_phase_messages(idx[b], values[b], paths[b], nl, L, 3), q, out[b].hex())
        assert ch.proof == want[b].proof and ch.state == want[b].state and ch.compressed_proof == want[b].compressed_proof
    # the round still serves the same batch, with the same records
    v, p, l2 = ctx.batch_query_round([int(i) for i in idx[:, 1]], trace_count=3, trace_stride=1 << lb)
    for b in range(3):
        assert l2[b] == lens[b] and (p[b][:l2[b]] == paths[b, 1][:lens[b]]).all(), b
        assert (v[b][:3 + 2 * nl] == values[b, 1]).all(), b
    # the trace batch gone (a plain batch), then the batch gone (a single commit)
    ctx.commit_batch([[1, 2, 3]] * 3, L)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_query_phase(1, 5, states, trace_count=3, trace_stride=1 << lb)
    assert e.value.code == FRI_ESTATE
    ctx.batch_query_phase(1, 5, states)
    ctx.commit([1, 2, 3], L)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_query_phase(1, 5, states)
    assert e.value.code == FRI_ESTATE


# ---- 6. round trip into the batched verifier ---------------------------------------
def test_outputs_feed_the_batched_verifier(ctx):
    log_t, lb, q, B = 6, 3, 3, 67
    L = log_t + lb
    max_index = (1 << L) - 2 * (1 << lb) - 1
    a1s = [1000003 * b + 5 for b in range(B)]
    chans = [fri_amd.Channel() for _ in range(B)]
    proofs = fri_amd.prove_fibsq_batch(a1s, log_t, lb, 0, chans, ctx=ctx)
    nls = [p.fri.n_layers for p in proofs]
    ml = max(nls)
    states = [bytes.fromhex(ch.state) for ch in chans]
    idx, values, paths, lens, _ = ctx.batch_query_phase(q, max_index, states, trace_count=3, trace_stride=1 << lb,
                                                        max_layers=ml)
    assert all(lens)
    hw, vw, pb = fri_amd.verify_record_strides(L, ml, 3)
    assert values.shape == (B, q, vw) and paths.shape == (B, q, pb)
    # the head from the commit results: trace root, alphas, layer roots, betas, final value
    words = lambda digest: np.frombuffer(digest, dtype=">u4").astype(np.uint32)      # noqa: E731
    head = np.zeros((B, hw), dtype=np.uint32)
    for b, pr in enumerate(proofs):
        head[b, 0:8] = words(pr.trace_root)
        head[b, 8:11] = pr.alphas
        for k, root in enumerate(pr.fri.roots):
            head[b, 11 + 8 * k: 19 + 8 * k] = words(root)
        head[b, 11 + 8 * ml: 11 + 8 * ml + len(pr.fri.betas)] = pr.fri.betas
        head[b, 11 + 9 * ml - 1] = pr.fri.final_value
    shape = fri_amd.VerifyShape(L, ml, q, 3, log_t, lb, fri_amd.GENERATOR, max_index)
    a_last = np.array([pr.a_last for pr in proofs], dtype=np.uint32)
    verdict = ctx.verify_batch(shape, B, np.zeros((B, 36), dtype=np.uint8), np.array(nls, dtype=np.uint32), a_last,
                               head, hw, idx, values, vw, paths, pb)
    assert not verdict.any(), verdict
    # ... and it is a check: one flipped path byte of one member is found
    paths[5, 1, 40] ^= 1
    verdict = ctx.verify_batch(shape, B, np.zeros((B, 36), dtype=np.uint8), np.array(nls, dtype=np.uint32), a_last,
                               head, hw, idx, values, vw, paths, pb)
    assert verdict[5] and not np.delete(verdict, 5).any()


# ---- 7. the round stages through the same chunks ------------------------------------
def _fri_only_round_case(ctx, oracle):
    log_n = 7
    polys = [oracle.splitmix64_np(70 + b, d).astype(np.uint32) for b, d in enumerate([16, 16, 3, 16, 16])]
    res, _ = _commit(ctx, polys, log_n)
    nls = [r.n_layers for r in res]
    assert len(set(nls)) > 1
    return log_n, max(nls), dict(indices=[5, 77, (1 << 40) + 3, 9, 127], skip=[0, 0, 0, 1, 0])


def _trace_round_case(ctx, oracle):
    chans = [fri_amd.Channel() for _ in range(5)]
    proofs = fri_amd.prove_fibsq_batch([3, 4, 5, 6, 7], 4, 2, 0, chans, ctx=ctx)
    return 6, max(p.fri.n_layers for p in proofs), dict(indices=[0, 17, 55, 3, 63], trace_count=3, trace_stride=4)


@pytest.mark.parametrize("case", [_fri_only_round_case, _trace_round_case])
def test_round_chunks_give_the_same_bytes(ctx, oracle, case):
    log_n, ml, kw = case(ctx, oracle)
    tc, skip = kw.get("trace_count", 0), kw.get("skip", [0] * 5)

    def run():
        _, values, paths = _arrays(5, 1, log_n, ml, tc)
        values, paths = np.ascontiguousarray(values[:, 0]), np.ascontiguousarray(paths[:, 0])
        return ctx.batch_query_round(values=values, paths=paths, **kw)

    one = run()
    for b in range(5):
        if skip[b]:
            assert one[2][b] == 0 and (one[0][b] == VAL_FILL).all() and (one[1][b] == PATH_FILL).all()
        else:
            assert one[2][b] >= 32 * log_n * tc + 64 * log_n and not (one[1][b][:one[2][b]] == PATH_FILL).all()
    try:
        for chunk in (1, 2, 3):
            ctx.set_query_chunk(chunk)
            got = run()
            assert (got[0] == one[0]).all() and (got[1] == one[1]).all() and got[2] == one[2], chunk
    finally:
        ctx.set_query_chunk(0)


# ---- 8. the round against the single-proof gather ------------------------------------
@pytest.mark.parametrize("log_n,ds,indices", [
    (3, [1, 2, 5, 8], [(1 << 40) + 5] * 4),    # the members differ in layer count; an index far beyond the codeword
    (1, [2, 2, 2], [0, 1, 5]),                 # the last layer has one element
])
def test_round_records_equal_the_members_decommitments(ctx, oracle, log_n, ds, indices):
    """The round and the phase share one gather kernel, so "phase equals round"
    does not check the gather itself: fri_batch_decommit_query goes through
    k_decommit_gather, one member at a time."""
    polys = [oracle.splitmix64_np(50 + b, d).astype(np.uint32) for b, d in enumerate(ds)]
    res, _ = _commit(ctx, polys, log_n)
    nls = [r.n_layers for r in res]
    if len(set(ds)) > 1:
        assert len(set(nls)) > 1
    else:
        assert nls == [2] * len(ds)
    values, paths, lens = ctx.batch_query_round(indices)
    for b, nl in enumerate(nls):
        assert lens[b] == sum(64 * (log_n - k) for k in range(nl))
        _, openings = fri_amd.batch_round_records(values[b], paths[b], lens[b], 0, nl, log_n)
        want = ctx.batch_decommit_query(b, indices[b], nl, log_n)
        assert len(openings) == nl and openings == want, (b, nl)
        assert all(len(o[2]) == len(o[3]) == 32 * (log_n - k) for k, o in enumerate(want))
