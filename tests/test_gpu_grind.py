"""GPU: proof-of-work grinding on the device (fri_grind, fri_grind_batch;
DESIGN.md section 4h).  Every nonce and every state after the send is compared
with the hashlib model (tests/grind_model.py), which is recomputed only up to
16 bits; the 20-bit rows are compared with their constants."""
import ctypes
import hashlib

import pytest

import fri_amd
import grind_model as gm

pytestmark = pytest.mark.gpu
LAST = gm.LAST
S = gm.S


@pytest.fixture(scope="module")
def gctx():
    c = fri_amd.Context(0, 13)
    yield c
    c.close()


@pytest.fixture()
def window(gctx):
    """Sets the nonces per launch for one test; automatic again afterwards."""
    yield gctx.set_grind_window
    gctx.set_grind_window(0)


def _raw(state):
    return bytes.fromhex(state) if state else None


def _grind(ctx, state, bits, first=0, last=LAST):
    got = ctx.grind(_raw(state), bits, first, last)
    return None if got is None else (got[0], got[1].hex())


def _state_of(i):
    return hashlib.sha256(b"grind member %d" % i).hexdigest() if i % 3 else ""


@pytest.mark.parametrize("state", ["", S], ids=["empty", "S"])
@pytest.mark.parametrize("bits", [0, 1, 4, 8, 12, 16])
def test_tiers_equal_the_model(gctx, state, bits):
    assert _grind(gctx, state, bits) == gm.grind(state, bits)


def test_known_answers(gctx):
    for state, bits, first, nonce, after in gm.KATS:
        assert _grind(gctx, state, bits, first) == (nonce, after), (state[:8], bits, first)


def test_many_hits_in_one_window_still_the_smallest(gctx, window):
    window(16)                                     # about 4096 hits at 4 bits
    for state in ("", S, _state_of(1), _state_of(2)):
        assert _grind(gctx, state, 4) == gm.grind(state, 4)
        assert _grind(gctx, state, 4, 12345) == gm.grind(state, 4, 12345)


@pytest.mark.parametrize("log_window", [6, 10])
@pytest.mark.parametrize("bits", [12, 16])
def test_small_windows_give_the_automatic_answer(gctx, window, bits, log_window):
    auto = [_grind(gctx, st, bits) for st in ("", S)]
    window(log_window)
    assert [_grind(gctx, st, bits) for st in ("", S)] == auto == [gm.grind(st, bits) for st in ("", S)]


def _raw_grind(ctx, state, bits, first, last):
    """fri_grind over ctypes with a recognisable chan_out: (rc, found, nonce, chan_out bytes, has_state)."""
    cin, cout = fri_amd.ChannelState(), fri_amd.ChannelState()
    if state:
        ctypes.memmove(cin.digest, bytes.fromhex(state), 32)
        cin.has_state = 1
    ctypes.memset(ctypes.byref(cout), 0x5A, ctypes.sizeof(cout))
    nonce, found = ctypes.c_uint64(0xABCD), ctypes.c_uint32(7)
    rc = ctx.lib.fri_grind(ctx.h, ctypes.byref(cin), bits, first, last, ctypes.byref(nonce), ctypes.byref(found),
                           ctypes.byref(cout))
    return rc, found.value, nonce.value, bytes(cout.digest), cout.has_state


@pytest.mark.parametrize("state,bits", [("", 12), (S, 12), (S, 16)], ids=["empty-12", "S-12", "S-16"])
def test_bounds_of_the_range(gctx, state, bits):
    nu, after = gm.grind(state, bits)
    rc, found, nonce, out, has = _raw_grind(gctx, state, bits, 0, nu - 1)
    assert (rc, found) == (fri_amd.FRI_OK, 0) and out == b"\x5a" * 32 and has == 0x5A5A5A5A and nonce == 0xABCD
    assert _raw_grind(gctx, state, bits, 0, nu) == (fri_amd.FRI_OK, 1, nu, bytes.fromhex(after), 1)
    assert _grind(gctx, state, bits, nu) == (nu, after)
    assert _grind(gctx, state, bits, nu, nu) == (nu, after)
    assert _grind(gctx, state, bits, nu + 1) == gm.grind(state, bits, nu + 1)


@pytest.mark.parametrize("count", [1, 63, 65, 257, 1000003])
def test_ragged_ranges(gctx, window, count):
    # nu is the smallest from 0, so a range that ends at nu holds it alone
    # and one that ends before it holds nothing
    bits = 20 if count > 257 else 16
    nu, after = next((k[3], k[4]) for k in gm.KATS if k[0] == S and k[1] == bits and k[2] == 0)
    for log_window in (0, 7):
        window(log_window)
        assert _grind(gctx, S, bits, nu - count + 1, nu) == (nu, after)
        assert _grind(gctx, S, bits, nu - count, nu - 1) is None
        # ... and one that begins at nu holds it first
        assert _grind(gctx, S, bits, nu, nu + count - 1) == (nu, after)
    if count <= 257:
        for first in (0, 1, 62, 1000, 4095):
            assert _grind(gctx, S, 4, first, first + count - 1) == gm.grind(S, 4, first, first + count - 1)
            assert _grind(gctx, "", 6, first, first + count - 1) == gm.grind("", 6, first, first + count - 1)


def test_carries(gctx, window):
    rows = [k for k in gm.KATS if k[2]]
    assert len(rows) == 3
    for log_window in (0, 5, 6):
        window(log_window)
        for state, bits, first, nonce, after in rows:
            assert _grind(gctx, state, bits, first) == (nonce, after)
        # the top of the range: the walk ends at 2^64 - 1
        top = gm.grind(S, 8, LAST - 4095)
        assert _grind(gctx, S, 8, LAST - 4095) == top and top[0] == 0xFFFFFFFFFFFFF07E
        assert _grind(gctx, S, 16, LAST - 7) == gm.grind(S, 16, LAST - 7, LAST)
        assert _grind(gctx, S, 0, LAST) == gm.grind(S, 0, LAST, LAST)
        # a range across 2^32 whose only hit lies beyond the carry
        assert _grind(gctx, S, 8, 2 ** 32 - 3, 0x10000003D) == (0x10000003D, rows[0][4])
        assert _grind(gctx, S, 8, 2 ** 32 - 3, 0x10000003C) is None


def test_argument_errors_write_nothing(gctx):
    lib, E = gctx.lib, fri_amd.FRI_EINVAL
    assert _raw_grind(gctx, S, 33, 0, 9) == (E, 7, 0xABCD, b"\x5a" * 32, 0x5A5A5A5A)
    assert _raw_grind(gctx, S, 8, 10, 9) == (E, 7, 0xABCD, b"\x5a" * 32, 0x5A5A5A5A)
    cin = fri_amd.ChannelState()
    nonce, found = ctypes.c_uint64(3), ctypes.c_uint32(3)
    assert lib.fri_grind(gctx.h, ctypes.byref(cin), 8, 0, 9, None, ctypes.byref(found), None) == E
    assert lib.fri_grind(gctx.h, ctypes.byref(cin), 8, 0, 9, ctypes.byref(nonce), None, None) == E
    assert nonce.value == 3 and found.value == 3
    chs = (fri_amd.ChannelState * 2)()
    ctypes.memset(chs, 0x5A, ctypes.sizeof(chs))
    nn, ff = (ctypes.c_uint64 * 2)(5, 5), (ctypes.c_uint32 * 2)(5, 5)
    for batch, bits, c, n, f in ((0, 8, chs, nn, ff), (65536, 8, chs, nn, ff), (2, 33, chs, nn, ff),
                                 (2, 8, None, nn, ff), (2, 8, chs, None, ff), (2, 8, chs, nn, None)):
        assert lib.fri_grind_batch(gctx.h, batch, c, bits, LAST, n, f) == E
    assert list(nn) == [5, 5] and list(ff) == [5, 5] and bytes(chs) == b"\x5a" * ctypes.sizeof(chs)
    assert lib.fri_debug_set_grind_window(gctx.h, 33) == E
    # a chan_in of NULL is Channel::new(), a chan_out of NULL is not written
    assert lib.fri_grind(gctx.h, None, 8, 0, LAST, ctypes.byref(nonce), ctypes.byref(found), None) == fri_amd.FRI_OK
    assert (nonce.value, found.value) == (gm.grind("", 8)[0], 1)


def test_profiling_and_team_contexts():
    c = fri_amd.Context(0, 12)
    try:
        c.set_profiling(True)
        with pytest.raises(fri_amd.FriError) as e:
            c.grind_batch([None, bytes.fromhex(S)], 8)
        assert e.value.code == fri_amd.FRI_ESTATE
        assert _grind(c, S, 12) == gm.grind(S, 12)
        ms, launches, _ = c.profile("grind")
        assert launches >= 1 and ms > 0
        c.set_profiling(False)
        assert [(g[0], g[1].hex()) for g in c.grind_batch([None, bytes.fromhex(S)], 8)] == \
            [gm.grind("", 8), gm.grind(S, 8)]
    finally:
        c.close()
    team = fri_amd.Context.multi([0, 0], 12)
    try:
        assert _grind(team, S, 12) == gm.grind(S, 12)          # rank 0 serves it
        with pytest.raises(fri_amd.FriError) as e:
            team.grind_batch([None, bytes.fromhex(S)], 8)
        assert e.value.code == fri_amd.FRI_EINVAL
    finally:
        team.close()


def test_a_grind_leaves_the_resident_commit_alone(gctx, oracle):
    coeffs = oracle.splitmix64_field(11, 128)
    gctx.commit(coeffs, 10)
    info = gctx.commit_info()
    opened = gctx.decommit_query(777, info[2], 10)
    assert _grind(gctx, S, 12) == gm.grind(S, 12)
    assert [(g[0], g[1].hex()) for g in gctx.grind_batch([None, bytes.fromhex(S)], 8)] == \
        [gm.grind("", 8), gm.grind(S, 8)]
    assert gctx.commit_info() == info
    assert gctx.decommit_query(777, info[2], 10) == opened


@pytest.mark.parametrize("batch", [1, 2, 67])
def test_batch_equals_the_single_call_member_by_member(gctx, window, batch):
    bits = 10
    states = [_state_of(i + 1) for i in range(batch)]
    if batch > 2:
        assert "" in states and len(set(states)) > batch // 2
    want = [gm.grind(st, bits) for st in states]
    single = [_grind(gctx, st, bits) for st in states]
    assert single == want
    for log_window in (0, 6):
        window(log_window)
        got = gctx.grind_batch([_raw(st) for st in states], bits)
        assert [(g[0], g[1].hex()) for g in got] == want
    # a range that ends below the largest answer: those members find nothing, the others are served
    window(0)
    top = max(w[0] for w in want)
    for log_window in (0, 6):
        window(log_window)
        got = gctx.grind_batch([_raw(st) for st in states], bits, last=top - 1)
        for b, (g, w) in enumerate(zip(got, want)):
            assert (g is None) if w[0] == top else ((g[0], g[1].hex()) == w), b
    # ... and their states stay what came in (the raw call)
    chs = (fri_amd.ChannelState * batch)()
    for b, st in enumerate(states):
        if st:
            ctypes.memmove(chs[b].digest, bytes.fromhex(st), 32)
            chs[b].has_state = 1
    nn, ff = (ctypes.c_uint64 * batch)(*([9] * batch)), (ctypes.c_uint32 * batch)(*([9] * batch))
    assert gctx.lib.fri_grind_batch(gctx.h, batch, chs, bits, top - 1, nn, ff) == fri_amd.FRI_OK
    for b, (st, w) in enumerate(zip(states, want)):
        if w[0] == top:
            assert ff[b] == 0 and nn[b] == 9 and chs[b].has_state == (1 if st else 0)
            assert bytes(chs[b].digest) == (bytes.fromhex(st) if st else bytes(32))
        else:
            assert ff[b] == 1 and nn[b] == w[0] and bytes(chs[b].digest).hex() == w[1] and chs[b].has_state == 1


# ---- provers ------------------------------------------------------------------
SHAPE = (6, 3, 3)          # log_t, log_blowup, queries


@pytest.fixture(scope="module")
def single_proofs(gctx):
    """prove_fibsq(..., grinding_bits=8) of five members, by the default route
    (the device's: GRIND_DEVICE_MIN_BITS is 8)."""
    log_t, lb, q = SHAPE
    out = []
    for a1 in range(3, 8):
        ch = fri_amd.Channel()
        sp = fri_amd.prove_fibsq(a1, log_t, lb, q, ch, ctx=gctx, grinding_bits=8)
        out.append((a1, ch, sp))
    return out


def test_prove_fibsq_grinds_by_both_routes(gctx, monkeypatch, single_proofs):
    log_t, lb, q = SHAPE
    a1, ch, sp = single_proofs[0]
    runs = []
    for min_bits in (0, 33):                       # the device route, the host route
        monkeypatch.setattr(fri_amd, "GRIND_DEVICE_MIN_BITS", min_bits)
        c = fri_amd.Channel()
        fri_amd.prove_fibsq(a1, log_t, lb, q, c, ctx=gctx, grinding_bits=8)
        runs.append(c)
    assert runs[0].proof == runs[1].proof == ch.proof and runs[0].state == runs[1].state == ch.state
    assert runs[0].compressed_proof == runs[1].compressed_proof
    # the nonce is the model's for the state after the final value's send
    head = fri_amd.Channel()
    fri_amd.prove_fibsq(a1, log_t, lb, 0, head, ctx=gctx)
    pos = len(head.proof)
    nonce, _ = gm.grind(head.state, 8)
    assert ch.proof[:pos] == head.proof and ch.proof[pos] == nonce.to_bytes(8, "big")
    nl = sp.fri.n_layers
    assert pos == 4 + 2 * nl
    assert fri_amd.verify_fibsq(ch.proof, sp.a_last, log_t, lb, q, nl, grinding_bits=8)
    assert not fri_amd.verify_fibsq(ch.proof, sp.a_last, log_t, lb, q, nl, grinding_bits=0)
    assert not fri_amd.verify_fibsq(ch.proof, sp.a_last, log_t, lb, q, nl)
    # no grinding: today's transcript
    plain, zero = fri_amd.Channel(), fri_amd.Channel()
    fri_amd.prove_fibsq(a1, log_t, lb, q, plain, ctx=gctx)
    fri_amd.prove_fibsq(a1, log_t, lb, q, zero, ctx=gctx, grinding_bits=0)
    assert plain.proof == zero.proof and plain.state == zero.state and len(plain.proof) == len(ch.proof) - 1
    assert fri_amd.verify_fibsq(plain.proof, sp.a_last, log_t, lb, q, nl)


@pytest.mark.parametrize("min_bits", [0, 33], ids=["device-grind", "host-grind"])
@pytest.mark.parametrize("device_queries", [False, True], ids=["rounds", "device-queries"])
def test_prove_fibsq_batch_is_the_loop(gctx, monkeypatch, single_proofs, device_queries, min_bits):
    log_t, lb, q = SHAPE
    monkeypatch.setattr(fri_amd, "GRIND_DEVICE_MIN_BITS", min_bits)
    chans = [fri_amd.Channel() for _ in single_proofs]
    proofs = fri_amd.prove_fibsq_batch([a1 for a1, _, _ in single_proofs], log_t, lb, q, chans, ctx=gctx,
                                       device_queries=device_queries, grinding_bits=8)
    for (a1, ch, sp), c, p in zip(single_proofs, chans, proofs):
        assert c.proof == ch.proof and c.state == ch.state and c.compressed_proof == ch.compressed_proof, a1
        assert p.queries == sp.queries
        assert fri_amd.verify_fibsq(c.proof, p.a_last, log_t, lb, q, p.fri.n_layers, grinding_bits=8)


@pytest.mark.parametrize("min_bits", [0, 33], ids=["device-grind", "host-grind"])
def test_decommit_fri_with_grinding_is_the_loop(gctx, monkeypatch, oracle, min_bits):
    log_n, q = 10, 3
    monkeypatch.setattr(fri_amd, "GRIND_DEVICE_MIN_BITS", min_bits)
    polys = [oracle.splitmix64_field(20 + b, 128 - b) for b in range(5)]
    loop = []
    for poly in polys:
        ch = fri_amd.Channel()
        proof = fri_amd.fri_commit(poly, log_n, ch, ctx=gctx)
        fri_amd.decommit_fri(q, (1 << log_n) - 1, proof, ch, grinding_bits=8)
        assert fri_amd.verify_fri(ch.proof, log_n, proof.n_layers, q, (1 << log_n) - 1, grinding_bits=8)
        assert not fri_amd.verify_fri(ch.proof, log_n, proof.n_layers, q, (1 << log_n) - 1)
        loop.append(ch)
    # the reference's signature takes it too
    ch = fri_amd.Channel()
    proof = fri_amd.fri_commit(polys[0], log_n, ch, ctx=gctx)
    fri_amd.decommit_fri(q, (1 << log_n) - 1, proof.fri_layers, proof.fri_merkles, ch, grinding_bits=8)
    assert ch.proof == loop[0].proof and ch.state == loop[0].state
    for device_queries in (False, True):
        chans = [fri_amd.Channel() for _ in polys]
        proofs = fri_amd.fri_commit_batch(polys, log_n, chans, ctx=gctx)
        fri_amd.decommit_fri_batch(q, (1 << log_n) - 1, proofs, chans, device_queries=device_queries,
                                   grinding_bits=8)
        for c, want in zip(chans, loop):
            assert c.proof == want.proof and c.state == want.state and c.compressed_proof == want.compressed_proof
