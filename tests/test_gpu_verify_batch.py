"""The batched verifier on the device (fri_verify_batch: k_verify_chain and
k_verify_open) against the existing host verifiers.  Transcripts come from the
Python oracle (CPU code independent of the device) or from the existing GPU
provers; every expected verdict comes from fri_amd.verify_fri / verify_fibsq."""
import hashlib

import numpy as np
import pytest

import verify_batch_cases as vc

pytestmark = pytest.mark.gpu

P = vc.P
S1, S2 = hashlib.sha256(b"one").hexdigest(), hashlib.sha256(b"two").hexdigest()


def masks(fri_amd, ctx, msgs, a_last, log_t, lb, q, nl, states=None):
    reasons = []
    ok = fri_amd.verify_fibsq_batch(msgs, a_last, log_t, lb, q, nl, channel_states=states, ctx=ctx, reasons=reasons)
    assert ok == [r == 0 for r in reasons]
    return reasons


@pytest.mark.parametrize("shape", [(2, 1, 2), (2, 2, 1), (4, 2, 3), (6, 3, 2)])
def test_accepts_oracle_transcripts(ctx, shape):
    import fri_amd
    log_t, lb, q = shape
    states = ["", S1, S2]
    cases = [vc.fibsq_case(a1, log_t, lb, q, st) for a1, st in zip((3, 99, 31337), states)]
    msgs, a_last, nl = [list(c[0]) for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    for m, a, k, st in zip(msgs, a_last, nl, states):
        assert fri_amd.verify_fibsq(m, a, log_t, lb, q, k, channel_state=st)
    assert masks(fri_amd, ctx, msgs, a_last, log_t, lb, q, nl, states) == [0, 0, 0]


def test_accepts_gpu_made_proofs(ctx):
    import fri_amd
    # one from the batched prover at its cap, one from the single prover one above it
    ch = fri_amd.Channel()
    sp = fri_amd.prove_fibsq_batch([3141592], 14, 4, 2, [ch], ctx=ctx)[0]
    assert fri_amd.verify_fibsq(ch.proof, sp.a_last, 14, 4, 2, sp.fri.n_layers)
    assert masks(fri_amd, ctx, [ch.proof], [sp.a_last], 14, 4, 2, [sp.fri.n_layers]) == [0]
    ch = fri_amd.Channel()
    sp = fri_amd.prove_fibsq(2718281, 15, 4, 2, ch, ctx=ctx)
    assert fri_amd.verify_fibsq(ch.proof, sp.a_last, 15, 4, 2, sp.fri.n_layers)
    assert masks(fri_amd, ctx, [ch.proof], [sp.a_last], 15, 4, 2, [sp.fri.n_layers]) == [0]


@pytest.mark.parametrize("shape", [(4, 2, 2), (2, 1, 1)])
def test_every_flipped_message(ctx, shape):
    import fri_amd
    log_t, lb, q = shape
    L = log_t + lb
    msgs, a_last, nl = vc.fibsq_case(99, log_t, lb, q)
    msgs = list(msgs)
    cls = vc.message_classes(L, nl, q, 3)
    assert len(cls) == len(msgs)
    flipped = [i for i, m in enumerate(msgs) if m]
    batch = [msgs] + [vc.flip(msgs, i) for i in flipped]
    B = len(batch)
    got = masks(fri_amd, ctx, batch, [a_last] * B, log_t, lb, q, [nl] * B)
    want = [fri_amd.verify_fibsq(m, a_last, log_t, lb, q, nl) for m in batch]
    assert want == [True] + [False] * (B - 1)
    assert [r == 0 for r in got] == want
    bit = {"root": fri_amd.VERIFY_CHANNEL, "alpha": fri_amd.VERIFY_CHANNEL, "beta": fri_amd.VERIFY_CHANNEL,
           "index": fri_amd.VERIFY_CHANNEL, "final": fri_amd.VERIFY_FINAL,
           "trace_value": fri_amd.VERIFY_TRACE_PATH, "trace_path": fri_amd.VERIFY_TRACE_PATH,
           "value": fri_amd.VERIFY_FRI_PATH, "path": fri_amd.VERIFY_FRI_PATH}
    for r, i in zip(got[1:], flipped):
        need = bit[cls[i]]
        if cls[i] == "root" and r & fri_amd.VERIFY_MALFORMED:
            continue                     # the flip left the root message non-hex: decided on the host
        assert r & need, (i, cls[i], r)


def test_forgeries_with_honest_channels(ctx):
    import fri_amd
    V = fri_amd
    a = vc.forged_fibsq(4, 2, 3, cp_seed=3)                   # not the composition
    a1 = vc.forged_fibsq(2, 1, 2, cp_seed=3)                  # ... with degree T = n/2: a one-element last layer
    b = vc.forged_fibsq(4, 2, 3, tweak=lambda k, ev, last: [(v + 1) % P for v in ev] if k == 1 else ev)
    c = vc.forged_fibsq(4, 2, 3, tweak=lambda k, ev, last: [(v + 1) % P for v in ev] if last else ev)
    assert a1[2] == 3 + 1
    for (m, al, nl), (log_t, lb, q) in ((a, (4, 2, 3)), (a1, (2, 1, 2)), (b, (4, 2, 3)), (c, (4, 2, 3))):
        assert not fri_amd.verify_fibsq(m, al, log_t, lb, q, nl)
    ra, rb, rc = masks(fri_amd, ctx, [a[0], b[0], c[0]], [a[1], b[1], c[1]], 4, 2, 3, [a[2], b[2], c[2]])
    ra1, = masks(fri_amd, ctx, [a1[0]], [a1[1]], 2, 1, 2, [a1[2]])
    for r in (ra, ra1):
        assert r & V.VERIFY_COMPOSITION
        assert not r & (V.VERIFY_FRI_PATH | V.VERIFY_FOLD | V.VERIFY_FINAL | V.VERIFY_CHANNEL | V.VERIFY_TRACE_PATH)
    assert rb & V.VERIFY_FOLD and not rb & (V.VERIFY_FRI_PATH | V.VERIFY_TRACE_PATH | V.VERIFY_CHANNEL)
    assert rc & V.VERIFY_FINAL and not rc & V.VERIFY_CHANNEL


def test_fri_only_mixed_layers(ctx):
    import fri_amd
    coeffs = [5, 1, 64, 2, 16]                                # shuffled: 4, 1, 7, 2 and 5 layers
    cases = [vc.fri_case(7 + d, d, 6, 2, 63) for d in coeffs]
    msgs, nl = [list(c[0]) for c in cases], [c[1] for c in cases]
    assert nl == [4, 1, 7, 2, 5]
    for m, k in zip(msgs, nl):
        assert fri_amd.verify_fri(m, 6, k, 2, 63)
    reasons = []
    assert fri_amd.verify_fri_batch(msgs, 6, nl, 2, 63, ctx=ctx, reasons=reasons) == [True] * 5
    assert reasons == [0] * 5
    swapped = list(nl)
    swapped[0], swapped[2] = swapped[2], swapped[0]
    want = [fri_amd.verify_fri(m, 6, k, 2, 63) for m, k in zip(msgs, swapped)]
    assert want == [False, True, False, True, True]
    assert fri_amd.verify_fri_batch(msgs, 6, swapped, 2, 63, ctx=ctx) == want


def ragged_batch(B):
    """B transcripts at (2, 2, 1), every 7th with one flipped path byte."""
    msgs, a_last, nl = [], [], []
    cls = None
    for b in range(B):
        m, a, k = vc.fibsq_case(2 + b, 2, 2, 1)
        m = list(m)
        if b % 7 == 6:
            cls = vc.message_classes(4, k, 1, 3)
            paths = [i for i, c in enumerate(cls) if c in ("path", "trace_path")]
            m = vc.flip(m, paths[b % len(paths)])
        msgs.append(m)
        a_last.append(a)
        nl.append(k)
    return msgs, a_last, nl


@pytest.mark.parametrize("B", [1, 63, 65, 300])
def test_ragged_and_many(ctx, B):
    import fri_amd
    msgs, a_last, nl = ragged_batch(B)
    got = masks(fri_amd, ctx, msgs, a_last, 2, 2, 1, nl)
    assert [r != 0 for r in got] == [b % 7 == 6 for b in range(B)]
    for b in (0, 6, B - 1):
        if b < B:
            assert fri_amd.verify_fibsq(msgs[b], a_last[b], 2, 2, 1, nl[b]) == (got[b] == 0)
    try:
        ctx.set_verify_chunk(64)
        assert masks(fri_amd, ctx, msgs, a_last, 2, 2, 1, nl) == got
    finally:
        ctx.set_verify_chunk(0)


def test_chunk_of_one(ctx):
    import fri_amd
    msgs, a_last, nl = ragged_batch(7)
    msgs, a_last, nl = msgs[2:], a_last[2:], nl[2:]          # B = 5, the last one flipped
    got = masks(fri_amd, ctx, msgs, a_last, 2, 2, 1, nl)
    assert [r != 0 for r in got] == [False] * 4 + [True]
    try:
        ctx.set_verify_chunk(1)
        assert masks(fri_amd, ctx, msgs, a_last, 2, 2, 1, nl) == got
    finally:
        ctx.set_verify_chunk(0)


def test_prover_to_verifier(ctx):
    import fri_amd
    B = 67
    chans = [fri_amd.Channel() for _ in range(B)]
    sps = fri_amd.prove_fibsq_batch([1000 + 3 * b for b in range(B)], 6, 3, 3, chans, ctx=ctx)
    msgs, a_last, nl = [ch.proof for ch in chans], [sp.a_last for sp in sps], [sp.fri.n_layers for sp in sps]
    assert fri_amd.verify_fibsq_batch(msgs, a_last, 6, 3, 3, nl, ctx=ctx) == [True] * B
    assert fri_amd.verify_fibsq(msgs[5], a_last[5], 6, 3, 3, nl[5])
    a_last[5] = (a_last[5] + 1) % P
    assert not fri_amd.verify_fibsq(msgs[5], a_last[5], 6, 3, 3, nl[5])
    assert fri_amd.verify_fibsq_batch(msgs, a_last, 6, 3, 3, nl, ctx=ctx) == [b != 5 for b in range(B)]


def test_no_side_effects(ctx):
    import fri_amd
    chans = [fri_amd.Channel() for _ in range(3)]
    sps = fri_amd.prove_fibsq_batch([5, 6, 7], 4, 2, 2, chans, ctx=ctx)
    L = 6
    before = (ctx.commit_info(), ctx.batch_info(), ctx.batch_layer(1, 1, L).copy())
    msgs, a_last, nl = [ch.proof for ch in chans], [sp.a_last for sp in sps], [sp.fri.n_layers for sp in sps]
    assert fri_amd.verify_fibsq_batch(msgs, a_last, 4, 2, 2, nl, ctx=ctx) == [True] * 3
    after = (ctx.commit_info(), ctx.batch_info(), ctx.batch_layer(1, 1, L))
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    values, paths, lens = ctx.batch_query_round([1, 2, 3], trace_count=3, trace_stride=4)
    assert all(n > 0 for n in lens)
    assert int(values[1, 3]) == int(ctx.batch_layer(1, 0, L)[2])


def packed_case(fri_amd):
    msgs, a_last, nl = vc.fibsq_case(99, 4, 2, 2)
    return fri_amd.pack_transcripts([list(msgs)] * 2, 6, [nl] * 2, 2, 64 - 8 - 1, 3, 4, 2, [a_last] * 2)


def test_errors(ctx):
    import fri_amd
    pk = packed_case(fri_amd)
    base = list(pk.abi_args())
    assert list(ctx.verify_batch(*base)) == [0, 0]

    def refused(**change):
        args = list(base)
        sh = fri_amd.VerifyShape.from_buffer_copy(pk.shape)
        for k, v in change.items():
            if hasattr(sh, k):
                setattr(sh, k, v)
        args[0] = sh
        if "batch" in change:
            args[1] = change["batch"]
        if "a_last" in change:
            args[4] = change["a_last"]
        for name, pos in (("head_stride", 6), ("values_stride", 9), ("paths_stride", 11)):
            if name in change:
                args[pos] = change[name]
        verdict = np.full(2, 0xDEADBEEF, dtype=np.uint32)
        with pytest.raises(fri_amd.FriError) as e:
            ctx.verify_batch(*args, verdict=verdict)
        assert e.value.code == fri_amd.FRI_EINVAL, change
        assert list(verdict) == [0xDEADBEEF] * 2, change

    refused(log_n=0)
    refused(log_n=25)                                  # above the context's 24
    refused(max_layers=8)                              # log_n + 2
    refused(num_queries=fri_amd.VERIFY_MAX_QUERIES + 1)
    refused(trace_count=2)
    refused(log_t=5)                                   # log_t + log_blowup != log_n
    refused(offset=P)
    refused(a_last=np.array([pk.a_last[0], P], dtype=np.uint32))
    refused(head_stride=base[6] - 1)
    refused(values_stride=base[9] - 1)
    refused(paths_stride=base[11] - 1)
    refused(batch=0)
    team = fri_amd.Context.multi([0, 0], 12)
    try:
        verdict = np.full(2, 0xDEADBEEF, dtype=np.uint32)
        with pytest.raises(fri_amd.FriError) as e:
            team.verify_batch(*base, verdict=verdict)
        assert e.value.code == fri_amd.FRI_EINVAL and list(verdict) == [0xDEADBEEF] * 2
    finally:
        team.close()
    # a packed value >= p: MALFORMED for that member only
    pk2 = packed_case(fri_amd)
    pk2.values[1, 0, 3] = P
    got = ctx.verify_batch(*pk2.abi_args())
    assert got[0] == 0 and got[1] & fri_amd.VERIFY_MALFORMED


def test_staging_out_of_memory():
    import fri_amd
    c = fri_amd.Context(0, 14)
    try:
        pk = packed_case(fri_amd)
        held = c.device_bytes()[0]
        c.set_device_cap(held + 64)                    # below one member's staging
        with pytest.raises(fri_amd.FriError) as e:
            c.verify_batch(*pk.abi_args())
        assert e.value.code == fri_amd.FRI_ENOMEM
        c.set_device_cap(0)
        assert list(c.verify_batch(*pk.abi_args())) == [0, 0]
    finally:
        c.close()
