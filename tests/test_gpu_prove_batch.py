"""GPU: the batched prover: fri_trace_commit_batch,
fri_fibsq_composition_commit_batch and fri_batch_query_round, driven by
fri_amd.prove_fibsq_batch and by the Context methods.

Every member's transcript must be byte for byte what prove_fibsq gives for the
same a1 and the same incoming channel.  The yardsticks are the C oracle
(prover_check.check_proof_matches_c_oracle, per member), the golden
transcripts and the single-proof path on the same context; a batch is never
compared with itself.  The shapes are the smallest at which a path changes:
the n = 8 wrap of the composition kernel, one tile / the tile boundary / the
first tiled tree of the trace trees, the last LDS and the first batched
transform of the LDE and of the two interpolations, and the cap."""
import copy
import ctypes
import hashlib
from collections import defaultdict

import numpy as np
import pytest

import degree_cases as dc

pytestmark = pytest.mark.gpu

import fri_amd  # noqa: E402

P = fri_amd.P
CAP = fri_amd.BATCH_MAX_LOG_N
FRI_EINVAL, FRI_ESTATE, FRI_EDEGREE, FRI_ENOMEM = (fri_amd.FRI_EINVAL, fri_amd.FRI_ESTATE, fri_amd.FRI_EDEGREE,
                                                   fri_amd.FRI_ENOMEM)


def _proof_sha(msgs):
    return hashlib.sha256(b"".join(len(m).to_bytes(4, "little") + m for m in msgs)).hexdigest()


def _single(ctx, a1, log_t, lb, queries, first=None, state=""):
    """prove_fibsq on the same context: (proof, channel)."""
    ch = fri_amd.Channel(state=state)
    if first is not None:
        ch.send(first)
    return fri_amd.prove_fibsq(a1, log_t, lb, queries, ch, ctx=ctx), ch


# ---- 1. every member against the C oracle -------------------------------------
@pytest.mark.parametrize("log_t,lb,members", [
    (2, 1, 3),     # n = 8: fewer points than one composition lane's 16 (the wrap)
    (2, 2, 3),
    (5, 3, 3),     # one tile
    (6, 3, 3),     # the tile boundary, L = 9
    (7, 3, 3),     # the first tiled tree
    (9, 3, 3),     # the last LDS LDE and interpolation, L = 12
    (10, 3, 3),    # the first batched transform; the trace's interpolation still in LDS
    (13, 1, 3),    # the trace's interpolation through the batched transform
    (14, 4, 2),    # the cap
])
def test_members_match_c_oracle(ctx, corc, oracle, log_t, lb, members):
    from prover_check import check_proof_matches_c_oracle
    assert log_t + lb <= CAP
    a1s = [3141592, 7, P - 2][:members]
    chans = [fri_amd.Channel() for _ in a1s]
    proofs = fri_amd.prove_fibsq_batch(a1s, log_t, lb, 2, chans, ctx=ctx)
    assert [p.fri.member for p in proofs] == list(range(members))
    for a1, pr, ch in zip(a1s, proofs, chans):
        check_proof_matches_c_oracle(fri_amd, corc, oracle, pr, ch, a1, log_t, lb, 2)


# ---- 2. members against the single path ---------------------------------------
def test_members_match_single_path(ctx):
    log_t, lb, q, B = 6, 3, 3, 67
    a1s = [1000003 * b + 5 for b in range(B)]
    chans = [fri_amd.Channel() for _ in range(B)]
    for b, ch in enumerate(chans):
        ch.send(b"member %d" % b)              # each channel starts from another non-empty state
    proofs = fri_amd.prove_fibsq_batch(a1s, log_t, lb, q, chans, ctx=ctx)
    for b in range(B):
        pr, ch = _single(ctx, a1s[b], log_t, lb, q, first=b"member %d" % b)
        assert chans[b].proof == ch.proof and chans[b].state == ch.state, b
        assert proofs[b].trace_root == pr.trace_root and proofs[b].alphas == pr.alphas, b
        assert proofs[b].queries == pr.queries and proofs[b].fri.roots == pr.fri.roots, b


def test_golden_transcripts_as_batches(ctx, golden):
    groups = defaultdict(list)
    for c in golden["fibsq"]:
        groups[(c["log_t"], c["log_blowup"], c["queries"])].append(c)
    assert groups
    for (log_t, lb, q), cases in groups.items():
        chans = [fri_amd.Channel(state=c["channel_in"]) for c in cases]
        proofs = fri_amd.prove_fibsq_batch([c["a1"] for c in cases], log_t, lb, q, chans, ctx=ctx)
        for c, pr, ch in zip(cases, proofs, chans):
            assert pr.trace_root.hex() == c["trace_root"] and pr.alphas == c["alphas"], c["name"]
            assert pr.fri.betas == c["betas"] and [r.hex() for r in pr.fri.roots] == c["roots"], c["name"]
            assert pr.fri.final_value == c["final_value"] and pr.queries == c["query_indices"], c["name"]
            assert ch.state == c["channel_out"], c["name"]
            assert len(ch.proof) == c["messages"] and _proof_sha(ch.proof) == c["proof_sha256"], c["name"]


# ---- 3. more workgroups than CUs -----------------------------------------------
def test_more_members_than_cus(ctx):
    log_t, lb, q, B = 4, 2, 2, 300
    a1s = [2 * b + 3 for b in range(B)]
    chans = [fri_amd.Channel() for _ in range(B)]
    proofs = fri_amd.prove_fibsq_batch(a1s, log_t, lb, q, chans, ctx=ctx)
    for b in range(B):
        assert fri_amd.verify_fibsq(chans[b].proof, proofs[b].a_last, log_t, lb, q, len(proofs[b].fri.roots)), b
    for b in (0, 255, 256, 299):
        _, ch = _single(ctx, a1s[b], log_t, lb, q)
        assert chans[b].proof == ch.proof and chans[b].state == ch.state, b


# ---- 4. a violated member ------------------------------------------------------
def test_violated_member_is_isolated(ctx):
    log_t, lb, L = 8, 3, 11
    traces = np.stack([fri_amd.fibsq_trace(11 + b, 1 << log_t) for b in range(4)])
    a_last = [int(t[-1]) for t in traces]
    alphas = [[100 + b, 200 + b, 300 + b] for b in range(4)]
    states = [bytes([b + 1] * 32) for b in range(4)]
    # the single path first: results and layers of members 0, 1, 3
    want = {}
    for b in (0, 1, 3):
        ctx.trace_commit(traces[b], lb, readback=False)
        r = ctx.fibsq_composition_commit(log_t, lb, a_last[b], alphas[b], channel_state=states[b])
        want[b] = (bytes(r), [ctx.layer(k, L).copy() for k in range(r.n_layers)])
    roots = ctx.trace_commit_batch(traces, lb)
    assert len(roots) == 4
    bad = list(a_last)
    bad[2] = (bad[2] + 1) % P
    with pytest.raises(fri_amd.FriError) as e:
        ctx.fibsq_composition_commit_batch(log_t, lb, bad, alphas, channel_states=states)
    assert e.value.code == FRI_EDEGREE and "member 2" in str(e.value)
    assert ctx.batch_status == [0, 0, FRI_EDEGREE, 0]
    for b in (0, 1, 3):
        r = ctx.batch_results[b]
        assert bytes(r) == want[b][0], b
        assert r.n_layers == len(want[b][1])
        for k, lay in enumerate(want[b][1]):
            assert (ctx.batch_layer(b, k, L) == lay).all(), (b, k)
    buf = np.zeros(1 << L, dtype=np.uint32)
    assert ctx.lib.fri_batch_layer_copy(ctx.h, 2, 0, fri_amd._ptr(buf), buf.size) == FRI_ESTATE
    values = np.full((4, 3 + 2 * (L + 1)), 0xA5A5A5A5, dtype=np.uint32)
    paths = np.full((4, 3 * 32 * L + sum(64 * (L - k) for k in range(L + 1))), 0x5A, dtype=np.uint8)
    _, _, lens = ctx.batch_query_round([5, 6, 7, 8], trace_count=3, trace_stride=1 << lb, values=values, paths=paths)
    assert lens[2] == 0 and (values[2] == 0xA5A5A5A5).all() and (paths[2] == 0x5A).all()
    for b in (0, 1, 3):
        nl = ctx.batch_results[b].n_layers
        assert lens[b] == 3 * 32 * L + sum(64 * (L - k) for k in range(nl)), b
        # the openings equal the single-member read-back's
        _, openings = fri_amd.batch_round_records(values[b], paths[b], lens[b], 3, nl, L)
        assert openings == ctx.batch_decommit_query(b, 5 + b, nl, L), b


# ---- 5. the query round on a plain fri_commit_batch -----------------------------
def test_query_round_on_a_plain_batch(ctx, oracle):
    log_n, d = 10, 128
    n = 1 << log_n
    cases = [dc.chain(10, 128, {0: ("cancel", 21), 3: ("phantom", 2)}, 1001, "10_cancel0_phantom3"),
             dc.cancel(10, 128, 0, -1, 1002)]
    polys = [c.coeffs for c in cases] + [oracle.splitmix64_np(31, d).astype(np.uint32)]
    betas = [c.betas for c in cases] + [dc.make_betas(77)]
    chans = [fri_amd.Channel() for _ in polys]
    for b, ch in enumerate(chans):
        ch.send(b"plain %d" % b)
    res = ctx.commit_batch(polys, log_n, channel_states=[bytes.fromhex(ch.state) for ch in chans], forced_betas=betas)
    assert len({r.n_layers for r in res}) > 1               # the members end at different layers
    gen = ctx.batch_info()[0]
    proofs = []
    for b, (r, ch) in enumerate(zip(res, chans)):
        proofs.append(fri_amd._mirror_commit(r, fri_amd.BatchMember(ctx, b), log_n, ch, generation=gen))
        proofs[-1].member = b
    ref = [copy.deepcopy(ch) for ch in chans]
    for p, ch in zip(proofs, ref):
        fri_amd.decommit_fri(3, n - 1, p, ch)                # member by member
    fri_amd.decommit_fri_batch(3, n - 1, proofs, chans)
    for b, (ch, want) in enumerate(zip(chans, ref)):
        assert ch.proof == want.proof and ch.state == want.state, b
    # the trace openings need a trace batch behind the batch
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_query_round([1, 2, 3], trace_count=3, trace_stride=8)
    assert e.value.code == FRI_ESTATE
    # a skip mask leaves the skipped records untouched
    values = np.full((3, 2 * (log_n + 1)), 0xA5A5A5A5, dtype=np.uint32)
    paths = np.full((3, sum(64 * (log_n - k) for k in range(log_n + 1))), 0x5A, dtype=np.uint8)
    _, _, lens = ctx.batch_query_round([9, 10, 11], skip=[0, 1, 0], values=values, paths=paths)
    assert lens[1] == 0 and (values[1] == 0xA5A5A5A5).all() and (paths[1] == 0x5A).all()
    for b in (0, 2):
        _, openings = fri_amd.batch_round_records(values[b], paths[b], lens[b], 0, res[b].n_layers, log_n)
        assert openings == ctx.batch_decommit_query(b, 9 + b, res[b].n_layers, log_n), b
    # an index beyond the codeword is taken mod each layer's size, as fri_decommit_query takes it
    v2, p2, l2 = ctx.batch_query_round([n + 9, 10, 3 * n + 11], skip=[0, 1, 0])
    for b in (0, 2):
        assert l2[b] == lens[b] and (v2[b][:2 * res[b].n_layers] == values[b][:2 * res[b].n_layers]).all(), b
        assert (p2[b][:l2[b]] == paths[b][:lens[b]]).all(), b
    # strides too small: FRI_EINVAL and the needed bytes
    small = np.zeros((3, 64), dtype=np.uint8)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_query_round([9, 10, 11], paths=small)
    assert e.value.code == FRI_EINVAL
    assert ctx.round_needed == sum(64 * (log_n - k) for k in range(max(r.n_layers for r in res)))
    assert not small.any()


# ---- 6. errors and residency ----------------------------------------------------
def test_argument_errors(ctx):
    lib = ctx.lib
    roots = ctypes.create_string_buffer(b"\x77" * 64, 64)
    tr = np.ones((2, 1 << (CAP - 2)), dtype=np.uint32)
    assert lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(tr), CAP - 2, 3, 5, 2, roots) == FRI_EINVAL   # L = cap + 1
    tr = np.stack([fri_amd.fibsq_trace(3, 64), fri_amd.fibsq_trace(4, 64)])
    tr[1, 17] = P                                                                     # not canonical
    assert lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(tr), 6, 3, 5, 2, roots) == FRI_EINVAL
    assert b"member 1" in lib.fri_last_error(ctx.h) and roots.raw == b"\x77" * 64
    assert lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(tr), 6, 0, 5, 2, roots) == FRI_EINVAL   # blowup 1
    assert lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(tr), 6, 3, 5, 0, roots) == FRI_EINVAL   # no members
    assert lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(tr), 6, 3, P, 2, roots) == FRI_EINVAL   # offset >= p
    assert lib.fri_trace_commit_batch(ctx.h, fri_amd._ptr(tr), 6, 3, 1, 2, roots) == FRI_EINVAL   # 1^T = 1 in <w_B>
    assert roots.raw == b"\x77" * 64


def test_composition_needs_the_matching_trace_batch(ctx):
    log_t, lb = 6, 3
    traces = np.stack([fri_amd.fibsq_trace(3 + b, 1 << log_t) for b in range(3)])
    a_last = [int(t[-1]) for t in traces]
    alphas = [[1, 2, 3]] * 3
    ctx.trace_commit_batch(traces, lb)
    for args in ((log_t + 1, lb, a_last, alphas), (log_t, lb, a_last[:2], alphas[:2]), (log_t, lb + 1, a_last, alphas)):
        with pytest.raises(fri_amd.FriError) as e:
            ctx.fibsq_composition_commit_batch(*args)
        assert e.value.code == FRI_ESTATE
    with pytest.raises(fri_amd.FriError) as e:          # alpha >= p (a uint32 array is not checked on the host)
        ctx.fibsq_composition_commit_batch(log_t, lb, a_last, np.array([1, 2, 3, 4, P, 6, 7, 8, 9], dtype=np.uint32))
    assert e.value.code == FRI_EINVAL and "member 1" in str(e.value)
    res = ctx.fibsq_composition_commit_batch(log_t, lb, a_last, alphas)
    assert [r.n_layers for r in res] == [log_t + 2] * 3
    ctx.batch_query_round([1, 2, 3], trace_count=3, trace_stride=1 << lb)
    # a plain batch drops the trace batch, a single commit the batch
    ctx.commit_batch([[1, 2, 3]] * 3, log_t + lb)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_query_round([1, 2, 3], trace_count=3, trace_stride=1 << lb)
    assert e.value.code == FRI_ESTATE
    ctx.batch_query_round([1, 2, 3])
    ctx.commit([1, 2, 3], log_t + lb)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_query_round([1, 2, 3])
    assert e.value.code == FRI_ESTATE


def test_single_prove_after_a_batch_matches_golden(ctx, golden):
    c = golden["fibsq"][2]
    fri_amd.prove_fibsq_batch([5, 6], c["log_t"], c["log_blowup"], 1, [fri_amd.Channel(), fri_amd.Channel()], ctx=ctx)
    ch = fri_amd.Channel(state=c["channel_in"])
    fri_amd.prove_fibsq(c["a1"], c["log_t"], c["log_blowup"], c["queries"], ch, ctx=ctx)
    assert ch.state == c["channel_out"] and _proof_sha(ch.proof) == c["proof_sha256"]


def test_enomem_keeps_what_was_resident():
    cx = fri_amd.Context(0, 14)
    try:
        log_t, lb, L = 9, 3, 12
        a1s = list(range(3, 43))
        small = [fri_amd.Channel(), fri_amd.Channel()]
        proofs = fri_amd.prove_fibsq_batch(a1s[:2], log_t, lb, 1, small, ctx=cx)
        info = cx.batch_info()
        layer1 = cx.batch_layer(1, 1, L)
        # 40 members' trace trees alone take 10 MiB
        cx.set_device_cap(cx.device_bytes()[0] + (1 << 20))
        with pytest.raises(fri_amd.FriError) as e:
            fri_amd.prove_fibsq_batch(a1s, log_t, lb, 1, [fri_amd.Channel() for _ in a1s], ctx=cx)
        assert e.value.code == FRI_ENOMEM
        assert cx.batch_info() == info and (cx.batch_layer(1, 1, L) == layer1).all()
        # ... the older trace batch included: a query round still opens it, as before
        v, p, lens = cx.batch_query_round(proofs[0].queries[:1] + proofs[1].queries[:1], trace_count=3,
                                          trace_stride=1 << lb)
        trace, _ = fri_amd.batch_round_records(v[0], p[0], lens[0], 3, proofs[0].fri.n_layers, L)
        assert small[0].proof[-(6 + 4 * proofs[0].fri.n_layers):][:6] == \
            [x for val, path in trace for x in (val.to_bytes(8, "big"), path)]
        cx.set_device_cap(0)
        chans = [fri_amd.Channel() for _ in a1s]
        out = fri_amd.prove_fibsq_batch(a1s, log_t, lb, 1, chans, ctx=cx)
        assert all(fri_amd.verify_fibsq(ch.proof, pr.a_last, log_t, lb, 1, len(pr.fri.roots))
                   for pr, ch in zip(out, chans))
    finally:
        cx.close()
