"""CPU: proof-of-work grinding on the host.  The model
(tests/grind_model.py) reproduces the known answers; Channel.grind without a
context is the model; grinding_bits = 0 changes nothing for the golden
transcripts; and a transcript with a nonce is accepted up to the zero bits its
state really has and rejected above, without the nonce, with a short one and
with another one."""
import copy
import ctypes
import os
import re
import subprocess

import pytest

import fri_amd
import grind_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "stark-prover_amd", "lib", "libfri_amd.so")
HDR = os.path.join(ROOT, "include", "fri_amd.h")


def test_model_reproduces_every_kat():
    for state, bits, first, nonce, after in gm.KATS:
        assert gm.grind(state, bits, first) == (nonce, after), (state[:8], bits, first)
        assert gm.zero_bits(after) >= bits
        # the smallest: nothing from `first` up to it gives the bits
        if first < nonce <= first + (1 << 17):
            assert gm.grind(state, bits, first, nonce - 1) is None
    # the message is the 16 lowercase hex characters of be64(nonce) after the state's 64
    import hashlib
    assert hashlib.sha256((gm.S + "000000000000015b").encode()).hexdigest() == gm.KATS[6][4]
    assert hashlib.sha256(b"0000000000000002").hexdigest() == gm.KATS[0][4]


@pytest.mark.parametrize("state", ["", gm.S], ids=["empty", "S"])
@pytest.mark.parametrize("bits", [0, 1, 8, 12, 16])
def test_channel_grind_on_the_host_is_the_model(state, bits):
    ch = fri_amd.Channel(state=state, proof=[b"before"], compressed_proof=[b"before"])
    nonce = ch.grind(bits)
    want, after = gm.grind(state, bits)
    assert nonce == want and ch.state == after
    assert ch.proof == [b"before", want.to_bytes(8, "big")] == ch.compressed_proof
    assert fri_amd.state_has_zero_bits(ch.state, bits) and gm.zero_bits(ch.state) >= bits
    # from another start: the model's next answer
    ch = fri_amd.Channel(state=state)
    assert ch.grind(bits, first=want + 1) == gm.grind(state, bits, want + 1)[0]


def test_channel_grind_argument_errors():
    for bits, first in ((33, 0), (-1, 0), (8, -1), (8, 1 << 64)):
        ch = fri_amd.Channel(state=gm.S)
        with pytest.raises(fri_amd.FriError) as e:
            ch.grind(bits, first=first)
        assert e.value.code == fri_amd.FRI_EINVAL and ch.proof == [] and ch.state == gm.S
    for fn in (lambda: fri_amd.verify_fri([], 4, 1, 0, 15, grinding_bits=33),
               lambda: fri_amd.verify_fibsq([], 1, 4, 2, 0, 1, grinding_bits=-1),
               lambda: fri_amd.prove_fibsq_batch([], 6, 3, 2, [], grinding_bits=40),
               lambda: fri_amd.decommit_fri_batch(3, 63, [], [], grinding_bits=33)):
        with pytest.raises(fri_amd.FriError) as e:
            fn()
        assert e.value.code == fri_amd.FRI_EINVAL
    assert fri_amd.prove_fibsq_batch([], 6, 3, 2, [], grinding_bits=8) == []       # (no context is opened)
    fri_amd.decommit_fri_batch(3, 63, [], [], grinding_bits=8)
    assert 0 <= fri_amd.GRIND_DEVICE_MIN_BITS <= 33


def test_header_and_ctypes_table_agree():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "stark-prover_amd")], check=True)
    lib = fri_amd.load_library()
    types = {"fri_ctx*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
             "uint32_t*": ctypes.POINTER(ctypes.c_uint32), "uint64_t*": ctypes.POINTER(ctypes.c_uint64),
             "fri_channel_state*": ctypes.POINTER(fri_amd.ChannelState),
             "const fri_channel_state*": ctypes.POINTER(fri_amd.ChannelState)}
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    want = {"fri_grind": ["fri_ctx*", "const fri_channel_state*", "uint32_t", "uint64_t", "uint64_t", "uint64_t*",
                          "uint32_t*", "fri_channel_state*"],
            "fri_grind_batch": ["fri_ctx*", "uint32_t", "fri_channel_state*", "uint32_t", "uint64_t", "uint64_t*",
                                "uint32_t*"],
            "fri_debug_set_grind_window": ["fri_ctx*", "uint32_t"]}
    for name, params in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        got = [re.sub(r"\s*\b\w+$", "", " ".join(p.split())).replace(" *", "*") for p in m.group(1).split(",")]
        assert got == params, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and [types[p] for p in params] == list(fn.argtypes), name
    # every entry refuses a null context, with nothing written
    nonce, found = ctypes.c_uint64(77), ctypes.c_uint32(77)
    chs = (fri_amd.ChannelState * 2)()
    out = fri_amd.ChannelState()
    E = fri_amd.FRI_EINVAL
    assert lib.fri_grind(None, chs, 8, 0, 9, ctypes.byref(nonce), ctypes.byref(found), ctypes.byref(out)) == E
    nn, ff = (ctypes.c_uint64 * 2)(5, 5), (ctypes.c_uint32 * 2)(5, 5)
    assert lib.fri_grind_batch(None, 2, chs, 8, 9, nn, ff) == E
    assert lib.fri_debug_set_grind_window(None, 6) == E
    assert nonce.value == 77 and found.value == 77 and list(nn) == [5, 5] and list(ff) == [5, 5]
    assert bytes(out.digest) == bytes(32) and out.has_state == 0
    hdr = open(HDR).read()
    assert "profiles/grind.txt" in hdr and os.path.exists(os.path.join(ROOT, "profiles", "grind.txt"))


# ---- transcripts ------------------------------------------------------------
def test_zero_grinding_bits_leave_the_golden_transcripts_accepted(oracle, golden):
    for c in golden["cases"]:
        if c["forced_betas"] is not None:
            continue
        ch = oracle.Channel(state=c["channel_in"])
        r = oracle.fri_commit(c["coeffs"], c["log_n"], ch, offset=c["offset"])
        oracle.decommit_fri(3, (1 << c["log_n"]) - 1, r.layers, r.trees, ch)
        args = (ch.proof, c["log_n"], len(r.roots), 3, (1 << c["log_n"]) - 1, c["offset"], c["channel_in"])
        assert fri_amd.verify_fri(*args, grinding_bits=0) and fri_amd.verify_fri(*args), c["name"]
    for c in golden["fibsq"]:
        ch = oracle.Channel(state=c["channel_in"])
        oracle.fibsq_prove(c["a1"], c["log_t"], c["log_blowup"], c["queries"], ch)
        assert fri_amd.verify_fibsq(ch.proof, c["a_last"], c["log_t"], c["log_blowup"], c["queries"], c["n_layers"],
                                    channel_state=c["channel_in"], grinding_bits=0), c["name"]


def _ground(och, bits):
    """Grinds an oracle channel in place with the mirror's host route; returns
    the position of the nonce message."""
    ch = fri_amd.Channel(state=och.state)
    nonce = ch.grind(bits)
    assert nonce == gm.grind(och.state, bits)[0]
    och.proof.append(nonce.to_bytes(8, "big"))
    och.compressed_proof.append(nonce.to_bytes(8, "big"))
    och.state = ch.state
    return len(och.proof) - 1


def _accept_reject_cases(verify, msgs, pos, state_after):
    """`verify(messages, grinding_bits)` on a transcript whose message `pos`
    is the nonce and whose state after it is `state_after`."""
    have = gm.zero_bits(state_after)
    assert 8 <= have < 32
    for bits in range(1, have + 1):
        assert verify(msgs, bits), bits
    assert not verify(msgs, have + 1)                      # one bit more than the state has
    assert not verify(msgs, 0)                             # the nonce stands where an index is expected
    assert not verify(msgs[:pos] + msgs[pos + 1:], 8)      # the nonce is missing
    assert not verify(msgs[:pos] + [msgs[pos][4:]] + msgs[pos + 1:], 8)       # 4 bytes
    other = (int.from_bytes(msgs[pos], "big") + 1).to_bytes(8, "big")
    assert not verify(msgs[:pos] + [other] + msgs[pos + 1:], 8)                # another nonce: other indices follow
    assert not verify(msgs[:pos] + [msgs[pos], msgs[pos]] + msgs[pos + 1:], 8)


def test_verify_fri_with_a_nonce(oracle, golden):
    for name in ("rand_n7_s42", "channel_prefilled", "blowup1", "offset_3"):
        c = next(x for x in golden["cases"] if x["name"] == name)
        och = oracle.Channel(state=c["channel_in"])
        r = oracle.fri_commit(c["coeffs"], c["log_n"], och, offset=c["offset"])
        plain = copy.deepcopy(och)
        pos = _ground(och, 8)
        after = och.state
        oracle.decommit_fri(3, (1 << c["log_n"]) - 1, r.layers, r.trees, och)
        oracle.decommit_fri(3, (1 << c["log_n"]) - 1, r.layers, r.trees, plain)
        assert och.proof[:pos] == plain.proof[:pos] and och.proof[pos + 1:] != plain.proof[pos:]

        def verify(m, bits):
            return fri_amd.verify_fri(m, c["log_n"], len(r.roots), 3, (1 << c["log_n"]) - 1, c["offset"],
                                      c["channel_in"], grinding_bits=bits)
        _accept_reject_cases(verify, och.proof, pos, after)
        # the golden openings behind a nonce belong to other indices
        assert not verify(plain.proof[:pos] + [och.proof[pos]] + plain.proof[pos:], 8)


def test_verify_fibsq_with_a_nonce(oracle):
    log_t, lb, q = 3, 2, 3
    L, B = log_t + lb, 1 << lb
    och = oracle.Channel()
    pr = oracle.fibsq_prove(3141592, log_t, lb, 0, och)
    pos = _ground(och, 8)
    after = och.state
    trace = oracle.fibsq_trace(3141592, 1 << log_t)
    f = oracle.interpolate_lagrange_polynomials(oracle.coset_domain(log_t, offset=1), trace, fri_amd.P)
    f_eval = [oracle.poly_evaluate(f, x, fri_amd.P) for x in oracle.coset_domain(L)]
    f_levels = oracle.merkle_levels(f_eval)
    for _ in range(q):                                                # fibsq_prove's query phase (fri_oracle.py)
        idx = och.receive_random_int(0, (1 << L) - 2 * B - 1, True)
        for j in range(3):
            och.send(oracle.fe_to_bytes(f_eval[idx + j * B]))
            och.send(oracle.merkle_proof(f_levels, idx + j * B))
        oracle.decommit_fri_layers(idx, pr.fri.layers, pr.fri.trees, och)

    def verify(m, bits):
        return fri_amd.verify_fibsq(m, trace[-1], log_t, lb, q, len(pr.fri.roots), grinding_bits=bits)
    _accept_reject_cases(verify, och.proof, pos, after)
