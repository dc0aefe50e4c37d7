"""fri_verify_batch_pow on the device: the grinding nonce in the batched
verifier (fri_amd.h).  Every expected mask is
verify_pow_model.expected_masks over the same packed arrays the device gets;
the model is anchored on verify_fri / verify_fibsq by test_verify_pow_host.py,
which also pins what the batches of verify_pow_cases.py cover (every mask of
the nonce check, nonces with a high word, a ragged wave, a one-element layer).
Then the call without bits, the chunks, both prover routes end to end, the raw
ABI's refusals and the profiling classes."""
import copy

import numpy as np
import pytest

import grind_model as gm
import verify_mask_corpus as mc
import verify_pow_cases as pc
from verify_pow_model import expected_masks

pytestmark = pytest.mark.gpu

BATCH_NAMES = [n for n, _ in pc.batches()]


def device_masks(ctx, pk, **kw):
    kw.setdefault("grinding_bits", pk.grinding_bits)
    kw.setdefault("nonces", pk.nonces)
    return [int(m) for m in ctx.verify_batch(*pk.abi_args(), **kw)]


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_masks_are_the_models(ctx, name):
    import fri_amd
    batch = dict(pc.batches())[name]
    pk = batch.pk
    want = [int(m) for m in expected_masks(pk)]
    got = device_masks(ctx, pk)
    assert got == want, [(n, g, w) for n, g, w in zip(batch.names, got, want) if g != w]
    assert 0 in want and fri_amd.VERIFY_POW in want
    # the mirror over the same messages: the masks, and a loop of the host verifier
    reasons = []
    sh = pk.shape
    if sh.trace_count:
        ok = fri_amd.verify_fibsq_batch(batch.msgs, batch.a_last, sh.log_t, sh.log_blowup, sh.num_queries, batch.nls,
                                        channel_states=batch.states, ctx=ctx, reasons=reasons,
                                        grinding_bits=batch.bits)
    else:
        ok = fri_amd.verify_fri_batch(batch.msgs, sh.log_n, batch.nls, sh.num_queries, sh.max_index,
                                      channel_states=batch.states, ctx=ctx, reasons=reasons, grinding_bits=batch.bits)
    assert reasons == want and ok == [w == 0 for w in want]
    assert ok == [batch.verify(b) for b in range(pk.batch)]


def test_other_bits_on_the_same_records(ctx):
    """The ragged batch under every bits value up to 9 and under 32: only the
    POW class moves, as the model says."""
    import fri_amd
    pk = pc.fri_ragged_batch().pk
    base = [int(m) for m in expected_masks(pk, 1)]
    for bits in (1, 2, 3, 5, 8, 9, 32):
        want = [int(m) for m in expected_masks(pk, bits)]
        assert [w & ~fri_amd.VERIFY_POW for w in want] == [w & ~fri_amd.VERIFY_POW for w in base]
        assert device_masks(ctx, pk, grinding_bits=bits) == want, bits
    assert all(w & fri_amd.VERIFY_POW for w in want)                  # no state of the corpus has 32 bits


def test_zero_bits_is_fri_verify_batch(ctx):
    """fri_verify_batch_pow(..., 0, NULL) = fri_verify_batch on a plain batch."""
    import ctypes
    import fri_amd
    batch = mc.flipped_fri_mixed()
    pk = batch.pk
    want = [int(m) for m in ctx.verify_batch(*pk.abi_args())]
    assert 0 in want and any(want)
    sh, B, chan, nl, a_last, head, hs, idx, vals, vs, paths, ps = pk.abi_args()
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))      # noqa: E731
    for nonces in (None, np.full(B, 2 ** 64 - 1, np.uint64)):              # ignored with 0 bits
        verdict = np.full(B, 0xDEADBEEF, dtype=np.uint32)
        rc = ctx.lib.fri_verify_batch_pow(ctx.h, ctypes.byref(sh), B, chan.ctypes.data_as(ctypes.POINTER(
            fri_amd.ChannelState)), u32(nl), None, u32(head), hs, idx.ctypes.data_as(u64p), u32(vals), vs,
            paths.ctypes.data_as(u8p), ps, 0, nonces.ctypes.data_as(u64p) if nonces is not None else None,
            u32(verdict))
        assert rc == fri_amd.FRI_OK and [int(v) for v in verdict] == want


def test_chunks_take_their_own_nonces(ctx):
    batch = pc.fri_ragged_batch()
    want = [int(m) for m in expected_masks(batch.pk)]
    try:
        for chunk in (5, 64):
            ctx.set_verify_chunk(chunk)
            assert device_masks(ctx, batch.pk) == want, chunk
    finally:
        ctx.set_verify_chunk(0)


def _flip_nonce(msgs, pos):
    m = bytearray(msgs[pos])
    assert len(m) == 8
    m[7] ^= 1
    return msgs[:pos] + [bytes(m)] + msgs[pos + 1:]


@pytest.mark.parametrize("device_queries", [False, True])
def test_prove_fibsq_batch_to_the_verifier(ctx, device_queries):
    import fri_amd
    log_t, lb, q, B = 3, 2, 2, 4
    chans = [fri_amd.Channel(), fri_amd.Channel(state=mc.S1), fri_amd.Channel(), fri_amd.Channel(state=mc.S2)]
    states = [ch.state for ch in chans]
    sps = fri_amd.prove_fibsq_batch([7, 99, 3141592, 12345], log_t, lb, q, chans, ctx=ctx,
                                    device_queries=device_queries, grinding_bits=8)
    msgs, a_last, nl = [ch.proof for ch in chans], [sp.a_last for sp in sps], [sp.fri.n_layers for sp in sps]

    def both(m, bits):
        reasons = []
        got = fri_amd.verify_fibsq_batch(m, a_last, log_t, lb, q, nl, channel_states=states, ctx=ctx, reasons=reasons,
                                         grinding_bits=bits)
        assert got == [fri_amd.verify_fibsq(m[b], a_last[b], log_t, lb, q, nl[b], channel_state=states[b],
                                            grinding_bits=bits) for b in range(B)]
        assert got == [r == 0 for r in reasons]
        return got, reasons
    assert both(msgs, 8) == ([True] * B, [0] * B)
    assert both(msgs, 0) == ([False] * B, [fri_amd.VERIFY_MALFORMED] * B)     # one message too many
    flipped = [_flip_nonce(m, 4 + 2 * n) for m, n in zip(msgs, nl)]
    got, reasons = both(flipped, 8)
    assert got == [False] * B
    assert all(r and not r & ~(fri_amd.VERIFY_POW | fri_amd.VERIFY_CHANNEL) for r in reasons)


@pytest.mark.parametrize("device_queries", [False, True])
def test_decommit_fri_batch_to_the_verifier(ctx, device_queries):
    import fri_amd
    import fri_oracle as fo
    log_n, q, B = 6, 2, 4
    polys = [fo.splitmix64_field(40 + b, d) for b, d in enumerate((16, 1, 32, 5))]
    chans = [fri_amd.Channel(), fri_amd.Channel(state=mc.S1), fri_amd.Channel(), fri_amd.Channel(state=mc.S2)]
    states = [ch.state for ch in chans]
    proofs = fri_amd.fri_commit_batch(polys, log_n, chans, ctx=ctx)
    fri_amd.decommit_fri_batch(q, 63, proofs, chans, device_queries=device_queries, grinding_bits=8)
    msgs, nl = [ch.proof for ch in chans], [p.n_layers for p in proofs]
    assert len(set(nl)) == 4

    def both(m, bits):
        reasons = []
        got = fri_amd.verify_fri_batch(m, log_n, nl, q, 63, channel_states=states, ctx=ctx, reasons=reasons,
                                       grinding_bits=bits)
        assert got == [fri_amd.verify_fri(m[b], log_n, nl[b], q, 63, channel_state=states[b], grinding_bits=bits)
                       for b in range(B)]
        assert got == [r == 0 for r in reasons]
        return got, reasons
    assert both(msgs, 8) == ([True] * B, [0] * B)
    assert both(msgs, 0)[0] == [False] * B
    flipped = [_flip_nonce(m, 2 * n) for m, n in zip(msgs, nl)]
    got, reasons = both(flipped, 8)
    assert got == [False] * B
    assert all(r and not r & ~(fri_amd.VERIFY_POW | fri_amd.VERIFY_CHANNEL) for r in reasons)


def test_twenty_bits_from_fri_grind(ctx):
    import fri_amd
    import fri_oracle as fo
    ch0, r = pc._fri_commit(71, 64, 6, "")
    ch = copy.deepcopy(ch0)
    nonce, after = ctx.grind(bytes.fromhex(ch.state), 20)
    assert (nonce, after.hex()) == gm.grind(ch.state, 0, nonce)
    ch.send(nonce.to_bytes(8, "big"))
    have = gm.zero_bits(ch.state)
    assert ch.state == after.hex() and 20 <= have < 32
    fo.decommit_fri(2, 63, r.layers, r.trees, ch)
    nl = len(r.roots)
    for bits, want in ((20, 0), (have, 0), (have + 1, fri_amd.VERIFY_POW), (32, fri_amd.VERIFY_POW)):
        reasons = []
        assert fri_amd.verify_fri_batch([ch.proof], 6, [nl], 2, 63, ctx=ctx, reasons=reasons,
                                        grinding_bits=bits) == [want == 0]
        assert reasons == [want]
        assert fri_amd.verify_fri(ch.proof, 6, nl, 2, 63, grinding_bits=bits) == (want == 0)


def test_raw_abi_refusals(ctx):
    import fri_amd
    pk = pc.one_element_batch().pk
    for kw in (dict(grinding_bits=33), dict(grinding_bits=8, nonces=None), dict(grinding_bits=2 ** 31)):
        verdict = np.full(pk.batch, 0xDEADBEEF, dtype=np.uint32)
        with pytest.raises(fri_amd.FriError) as e:
            device_masks(ctx, pk, verdict=verdict, **kw)
        assert e.value.code == fri_amd.FRI_EINVAL, kw
        assert list(verdict) == [0xDEADBEEF] * pk.batch, kw
    assert device_masks(ctx, pk) == [int(m) for m in expected_masks(pk)]       # the context goes on


def test_profiling_classes(ctx):
    import fri_amd
    batch = pc.fri_ragged_batch()
    want = [int(m) for m in expected_masks(batch.pk)]
    c = fri_amd.Context(0, 14)
    try:
        c.set_profiling(True)
        c.set_verify_chunk(16)
        c.reset_profile()
        assert device_masks(c, batch.pk) == want
        chunks = (batch.pk.batch + 15) // 16
        assert c.profile("verify_chain")[1] == chunks and c.profile("verify_open")[1] == chunks
    finally:
        c.close()
