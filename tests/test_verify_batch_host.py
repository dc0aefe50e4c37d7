"""The batched verifier's host side (fri_amd.pack_transcripts /
unpack_transcripts and the mirrors' host decisions): pure CPU code, no device.
Transcripts come from the Python oracle; expected verdicts from the existing
host verifiers."""
import hashlib

import numpy as np
import pytest

import verify_batch_cases as vc

P = vc.P
S1, S2 = hashlib.sha256(b"one").hexdigest(), hashlib.sha256(b"two").hexdigest()
FIBSQ_SHAPES = [(2, 1, 2), (2, 2, 1), (4, 2, 3), (6, 3, 2)]
MIXED = [5, 1, 64, 2, 16]      # coefficients of the mixed FRI batch, log_n = 6, in shuffled order


def fibsq_batch(shape):
    log_t, lb, q = shape
    cases = [vc.fibsq_case(a1, log_t, lb, q, st) for a1, st in ((3, ""), (99, S1), (31337, S2))]
    return [list(c[0]) for c in cases], [c[1] for c in cases], [c[2] for c in cases], ["", S1, S2]


@pytest.mark.parametrize("shape", FIBSQ_SHAPES)
def test_pack_unpack_returns_the_oracle_messages(shape):
    import fri_amd
    log_t, lb, q = shape
    L = log_t + lb
    msgs, a_last, nl, states = fibsq_batch(shape)
    for m, a, k, st in zip(msgs, a_last, nl, states):
        assert fri_amd.verify_fibsq(m, a, log_t, lb, q, k, channel_state=st)
    pk = fri_amd.pack_transcripts(msgs, L, nl, q, (1 << L) - 2 * (1 << lb) - 1, 3, log_t, lb, a_last,
                                  channel_states=states)
    assert not pk.reasons.any() and not pk.host.any()
    assert fri_amd.unpack_transcripts(pk) == msgs
    assert [int(x) for x in pk.n_layers] == nl and [int(x) for x in pk.a_last] == a_last
    assert [int(x) for x in pk.chan[:, 32]] == [0, 1, 1]
    assert pk.chan[1, :32].tobytes().hex() == S1


def test_pack_unpack_mixed_fri_batch():
    import fri_amd
    cases = [vc.fri_case(7 + d, d, 6, 2, 63) for d in MIXED]
    msgs, nl = [list(c[0]) for c in cases], [c[1] for c in cases]
    assert sorted(nl) == [1, 2, 4, 5, 7]
    for m, k in zip(msgs, nl):
        assert fri_amd.verify_fri(m, 6, k, 2, 63)
    pk = fri_amd.pack_transcripts(msgs, 6, nl, 2, 63)
    assert pk.shape.max_layers == 7 and pk.a_last is None
    assert not pk.reasons.any() and not pk.host.any()
    assert fri_amd.unpack_transcripts(pk) == msgs


def test_record_strides_are_the_query_rounds():
    """A (member, query) record is what fri_batch_query_round documents:
    trace_count + 2 n_layers words; trace_count paths of 32 L bytes, then per
    layer two paths of 32 (L - k) bytes."""
    import fri_amd
    for L, ml, tc in ((6, 5, 3), (6, 7, 0), (3, 4, 3), (18, 15, 3)):
        hw, vw, pb = fri_amd.verify_record_strides(L, ml, tc)
        assert vw == tc + 2 * ml
        assert pb == tc * 32 * L + sum(2 * 32 * (L - k) for k in range(ml))
        assert hw == (8 + 3 if tc else 0) + 8 * ml + (ml - 1) + 1
    msgs, a_last, nl, states = fibsq_batch((4, 2, 3))
    pk = fri_amd.pack_transcripts(msgs, 6, nl, 3, 64 - 8 - 1, 3, 4, 2, a_last, channel_states=states)
    ml = max(nl)
    assert pk.head.shape == (3, 11 + 9 * ml) and pk.values.shape == (3, 3, 3 + 2 * ml)
    assert pk.paths.shape == (3, 3, fri_amd.verify_record_strides(6, ml, 3)[2])
    assert pk.indices.shape == (3, 3) and pk.indices.dtype == np.uint64


def test_packer_host_decisions():
    import fri_amd
    log_t, lb, q = 4, 2, 2
    L = log_t + lb
    msgs, a_last, nl = vc.fibsq_case(99, log_t, lb, q)
    msgs = list(msgs)
    cls = vc.message_classes(L, nl, q, 3)
    assert len(cls) == len(msgs)
    big = list(msgs)
    i_val = cls.index("value")
    big[i_val] = (P + 5).to_bytes(8, "big")
    upper = list(msgs)
    upper[4] = msgs[4].upper()                 # the first layer root, same digest
    assert upper[4] != msgs[4] and cls[4] == "root"
    batch = [msgs, msgs[:-1], msgs + [msgs[-1]], big, upper]
    args = (log_t, lb, q)
    want = [fri_amd.verify_fibsq(m, a_last, *args, nl) for m in batch]
    assert want == [True, False, False, False, False]
    pk = fri_amd.pack_transcripts(batch, L, [nl] * 5, q, (1 << L) - 2 * (1 << lb) - 1, 3, log_t, lb, [a_last] * 5)
    M = fri_amd.VERIFY_MALFORMED
    assert [int(r) for r in pk.reasons] == [0, M, M, M, 0]
    assert [bool(h) for h in pk.host] == [False, False, False, False, True]
    # every member but the intact one is decided here: no device is needed
    reasons = []
    got = fri_amd.verify_fibsq_batch(batch[1:], [a_last] * 4, *args, [nl] * 4, reasons=reasons)
    assert got == want[1:] and all(reasons)
    # a doubled one-element value that differs, a wrong length, an n_layers out of range
    m2, nl2 = vc.fri_case(7 + 64, 64, 6, 2, 63)
    assert nl2 == 7                                # log_n + 1 layers: the last has one element
    c2 = vc.message_classes(6, nl2, 2, 0)
    first = next(i for i in range(len(c2) - 1) if c2[i] == "value" and c2[i + 1] == "value")
    dbl = list(m2)
    dbl[first] = ((int.from_bytes(dbl[first], "big") + 1) % P).to_bytes(8, "big")
    short_path = list(m2)
    j = c2.index("path")
    short_path[j] = short_path[j][:-1]
    pk2 = fri_amd.pack_transcripts([dbl, short_path, list(m2)], 6, [nl2, nl2, 9], 2, 63)
    assert [int(r) for r in pk2.reasons] == [M, M, M]
    for m, k in ((dbl, nl2), (short_path, nl2), (list(m2), 9)):
        assert not fri_amd.verify_fri(m, 6, k, 2, 63)


def test_empty_batch_and_mismatched_lengths():
    import fri_amd
    assert fri_amd.verify_fri_batch([], 6, [], 2, 63) == []
    assert fri_amd.verify_fibsq_batch([], [], 4, 2, 2, []) == []
    msgs, a_last, nl = vc.fibsq_case(99, 4, 2, 2)
    with pytest.raises(fri_amd.FriError):
        fri_amd.verify_fibsq_batch([list(msgs)], [a_last, a_last], 4, 2, 2, [nl])
    with pytest.raises(fri_amd.FriError):
        fri_amd.verify_fibsq_batch([list(msgs)], [a_last], 4, 2, 2, [nl, nl])
    with pytest.raises(fri_amd.FriError):
        fri_amd.verify_fibsq_batch([list(msgs)], [a_last], 4, 2, 2, [nl], channel_states=["", ""])
    with pytest.raises(fri_amd.FriError):
        fri_amd.verify_fri_batch([list(msgs)], 6, [], 2, 63)
    with pytest.raises(fri_amd.FriError):
        fri_amd.pack_transcripts([list(msgs)], 6, [nl], 2, 55, 3, 4, 2, None)
