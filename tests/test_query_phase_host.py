"""CPU: the host side of the device-run query phase (fri_batch_query_phase).
The header declares the two new entries with the argument lists the Python
ctypes table binds, each refuses a null context, the mirrors' argument errors
need no device, and the pure halves of the route -- query_phase_messages and
Channel.take_over_queries -- rebuild the query phase of a proof by the Python
oracle twin message for message."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fri_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "stark-prover_amd", "lib", "libfri_amd.so")
HDR = os.path.join(ROOT, "include", "fri_amd.h")
P = fri_amd.P

U32, SZ = ctypes.c_uint32, ctypes.c_size_t
CTYPES = {
    "fri_ctx*": ctypes.c_void_p,
    "uint32_t": U32,
    "uint64_t": ctypes.c_uint64,
    "size_t": SZ,
    "uint32_t*": ctypes.POINTER(U32),
    "uint64_t*": ctypes.POINTER(ctypes.c_uint64),
    "const uint8_t*": ctypes.POINTER(ctypes.c_uint8),
    "uint8_t*": ctypes.POINTER(ctypes.c_uint8),
    "size_t*": ctypes.POINTER(SZ),
    "fri_channel_state*": ctypes.POINTER(fri_amd.ChannelState),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "stark-prover_amd")], check=True)
    return fri_amd.load_library()


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\b\w+$", "", p).replace(" *", "*"))     # drop the parameter's name
    return out


def test_header_and_ctypes_table_agree(lib):
    for name in ("fri_batch_query_phase", "fri_debug_set_query_chunk"):
        params = _prototype(name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for i, (c, bound) in enumerate(zip(params, fn.argtypes)):
            assert bound is CTYPES[c], (name, i, c, bound)
    # the issue's argument order: the draw's shape, the channels, then the round's arguments
    assert _prototype("fri_batch_query_phase") == [
        "fri_ctx*", "uint32_t", "uint64_t", "fri_channel_state*", "const uint8_t*", "uint32_t", "uint64_t",
        "uint64_t*", "uint32_t*", "size_t", "uint8_t*", "size_t", "size_t*"]
    hdr = open(HDR).read()
    assert "profiles/prove_batch_device_queries.txt" in hdr
    assert os.path.exists(os.path.join(ROOT, "profiles", "prove_batch_device_queries.txt"))


def test_every_entry_refuses_a_null_context(lib):
    w = np.full(16, 0xA5A5A5A5, dtype=np.uint32)
    idx = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    chs = (fri_amd.ChannelState * 2)()
    chs[0].has_state = chs[1].has_state = 1
    pbuf = (ctypes.c_uint8 * 64)(*([0x5A] * 64))
    ln = (ctypes.c_size_t * 2)(9, 9)
    E = fri_amd.FRI_EINVAL
    assert lib.fri_batch_query_phase(None, 2, 7, chs, None, 0, 0, idx, fri_amd._ptr(w), 8, pbuf, 32, ln) == E
    assert lib.fri_debug_set_query_chunk(None, 2) == E
    assert list(ln) == [9, 9] and list(idx) == [7] * 4 and (w == 0xA5A5A5A5).all() and bytes(pbuf) == b"\x5a" * 64
    assert bytes(chs[0].digest) == bytes(32)


def test_mirror_argument_errors_need_no_device():
    assert fri_amd.prove_fibsq_batch([], 6, 3, 2, [], device_queries=True) == []      # (no context is opened)
    with pytest.raises(fri_amd.FriError) as e:
        fri_amd.prove_fibsq_batch([3, 4], 6, 3, 2, [fri_amd.Channel()], device_queries=True)
    assert e.value.code == fri_amd.FRI_EINVAL
    fri_amd.decommit_fri_batch(3, 63, [], [], device_queries=True)
    with pytest.raises(fri_amd.FriError) as e:
        fri_amd.decommit_fri_batch(3, 63, [], [fri_amd.Channel()], device_queries=True)
    assert e.value.code == fri_amd.FRI_EINVAL
    # the take-over: whole runs of equal length and a 64-character state
    ch = fri_amd.Channel()
    for msgs, q, state in (([b"a", b"b", b"c"], 2, "0" * 64), ([b"a"], 1, "00"), ([b"a"], 0, "0" * 64)):
        with pytest.raises(fri_amd.FriError) as e:
            ch.take_over_queries(msgs, q, state)
        assert e.value.code == fri_amd.FRI_EINVAL
    assert ch.proof == [] and ch.compressed_proof == [] and ch.state == ""
    ch.take_over_queries([], 0, "")                                   # no queries: nothing changes
    assert ch.proof == [] and ch.state == ""


def _rebuild_and_compare(oracle, och, before, pk, n_layers, log_n, trace_count, queries):
    """``och``: the oracle's channel after the whole proof; ``before``: a copy
    of it from before the query phase; ``pk``: the transcript packed."""
    assert not pk.reasons.any() and not pk.host.any()
    msgs = fri_amd.query_phase_messages(pk.indices[0], pk.values[0], pk.paths[0], n_layers, log_n, trace_count)
    tail = och.proof[len(before.proof):]
    assert len(msgs) == len(tail) and msgs == tail
    ch = fri_amd.Channel(state=before.state, proof=list(before.proof), compressed_proof=list(before.proof))
    ch.take_over_queries(msgs, queries, och.state)
    assert ch.proof == och.proof and ch.state == och.state
    # what receive_random_int(.., True) and send leave: an index is in `proof` alone
    per = len(msgs) // queries
    assert ch.compressed_proof == list(before.proof) + [m for i, m in enumerate(msgs) if i % per]
    # ... which is what a hashing channel fed the same phase ends with
    ref = fri_amd.Channel(state=before.state)
    for i, m in enumerate(msgs):
        if i % per == 0:
            assert ref.receive_random_int(0, pk.shape.max_index, True) == int.from_bytes(m, "big")
        else:
            ref.send(m)
    assert ref.state == och.state and ref.proof == msgs and ref.compressed_proof == ch.compressed_proof[len(before.proof):]


def test_messages_and_take_over_rebuild_a_fibsq_proof(oracle):
    import copy
    log_t, lb, q = 3, 2, 3
    L, B = log_t + lb, 1 << lb
    och = oracle.Channel()
    pr = oracle.fibsq_prove(3141592, log_t, lb, 0, och)
    before = copy.deepcopy(och)
    trace = oracle.fibsq_trace(3141592, 1 << log_t)
    f = oracle.interpolate_lagrange_polynomials(oracle.coset_domain(log_t, offset=1), trace, P)
    f_eval = [oracle.poly_evaluate(f, x, P) for x in oracle.coset_domain(L)]
    f_levels = oracle.merkle_levels(f_eval)
    for _ in range(q):                                                # fibsq_prove's query phase (fri_oracle.py)
        idx = och.receive_random_int(0, (1 << L) - 2 * B - 1, True)
        for j in range(3):
            och.send(oracle.fe_to_bytes(f_eval[idx + j * B]))
            och.send(oracle.merkle_proof(f_levels, idx + j * B))
        oracle.decommit_fri_layers(idx, pr.fri.layers, pr.fri.trees, och)
    whole = oracle.Channel()
    oracle.fibsq_prove(3141592, log_t, lb, q, whole)
    assert whole.proof == och.proof and whole.state == och.state      # (the split above is the oracle's prover)
    nl = len(pr.fri.roots)
    pk = fri_amd.pack_transcripts([och.proof], L, [nl], q, (1 << L) - 2 * B - 1, trace_count=3, log_t=log_t,
                                  log_blowup=lb, a_last=[trace[-1]])
    _rebuild_and_compare(oracle, och, before, pk, nl, L, 3, q)


def test_messages_and_take_over_rebuild_a_one_element_last_layer(oracle):
    import copy
    log_n, q = 2, 3
    och = oracle.Channel()
    och.send(b"not empty")
    start = och.state
    first = len(och.proof)
    res = oracle.fri_commit([5, 6, 7, 8], log_n, och)                 # blowup 1: layers of 4, 2 and 1 elements
    assert [len(l) for l in res.layers] == [4, 2, 1]
    before = copy.deepcopy(och)
    oracle.decommit_fri(q, 5, res.layers, res.trees, och)
    pk = fri_amd.pack_transcripts([och.proof[first:]], log_n, [3], q, 5, channel_states=[start])
    before.proof = before.proof[first:]
    och.proof = och.proof[first:]
    _rebuild_and_compare(oracle, och, before, pk, 3, log_n, 0, q)
    # the doubled value is there: 1 + 4 + 4 + 5 messages per query
    assert len(och.proof) - len(before.proof) == q * 14


def test_record_shape_function_against_the_sums_written_out():
    """record_paths_len is the mirror's one statement of a query record's
    paths: trace_count paths of log_n digests, then layer k's two of log_n - k
    digests.  verify_record_strides is it at max_layers."""
    for log_n in range(1, 7):
        for tc in (0, 3):
            for nl in range(0, log_n + 2):
                want = 0
                for _ in range(tc):
                    want += 32 * log_n
                for k in range(nl):
                    want += 32 * (log_n - k)          # the opened element's path
                    want += 32 * (log_n - k)          # its sibling's
                assert fri_amd.record_paths_len(log_n, tc, nl) == want, (log_n, tc, nl)
                hw, vw, pb = fri_amd.verify_record_strides(log_n, nl, tc)
                assert pb == fri_amd.record_paths_len(log_n, tc, nl) == want
                assert vw == tc + 2 * nl and hw == (11 if tc else 0) + 9 * nl
