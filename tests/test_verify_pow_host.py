"""CPU: the grinding nonce in the batched verifier (fri_verify_batch_pow,
DESIGN.md section 4g), everything short of the device.  The mask model
(verify_pow_model.py) is anchored on verify_fri / verify_fibsq over the ground
transcripts of verify_pow_cases.py and their tamperings; the corpus holds every
mask the device test relies on; pack_transcripts places, counts and refuses the
nonce message; the argument errors open no context; header, ctypes table and
the C++ mirror agree on the entry point."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fri_amd
import grind_model as gm
import verify_pow_cases as pc
from fri_amd import VERIFY_CHANNEL, VERIFY_MALFORMED, VERIFY_POW
from verify_pow_model import expected_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "stark-prover_amd", "lib", "libfri_amd.so")
HDR = os.path.join(ROOT, "include", "fri_amd.h")

BATCHES = dict(pc.batches())


# ---- the model against the host verifiers -----------------------------------
@pytest.mark.parametrize("name", list(BATCHES))
def test_model_is_zero_exactly_when_the_host_verifier_accepts(name):
    batch = BATCHES[name]
    want = expected_masks(batch.pk)
    assert batch.pk.grinding_bits == batch.bits
    for b, w in enumerate(want):
        assert (w == 0) == batch.verify(b), (batch.names[b], int(w))
    # a tampering leaves the openings' classes to the claimed values
    for n, w in zip(batch.names, want):
        if n.startswith(("honest", "grind8", "high32 ", "high63")):
            assert w == 0, n
        if n.startswith("weak"):
            assert w == VERIFY_POW, n
        if n.startswith(("index", "flipped_index")):
            assert w == VERIFY_CHANNEL, n
        if n.startswith(("behind", "nonce_plus_one", "high32+1")):
            assert w in (VERIFY_CHANNEL, VERIFY_CHANNEL | VERIFY_POW), n


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_bits_value_of_an_honest_member(name):
    """Accepted from 1 bit to the state's count, POW alone one bit above and
    at 32; the weak member is POW alone at its batch's bits and accepted below
    its own count."""
    batch = BATCHES[name]
    seen = 0
    for b, n in enumerate(batch.names):
        if not n.startswith(("honest", "grind8", "high32 ", "high63", "weak")) or seen >= 4:
            continue
        seen += 1
        have = gm.zero_bits(batch.grounds[b].after)
        assert have < 32
        for bits in list(range(1, have + 1)) + [have + 1, 32]:
            mask = int(expected_masks(batch.repack(b, bits))[0])
            assert mask == (0 if bits <= have else VERIFY_POW), (n, bits, have)
            assert batch.verify(b, bits) == (mask == 0), (n, bits)
    assert seen >= 2


def test_corpus_coverage():
    """What the device test's equality can see: every mask of the nonce check,
    the high-word nonces among the accepted, a one-element layer, mixed layer
    counts and channel states, accepted and rejected members interleaved."""
    masks = {n: [int(m) for m in expected_masks(b.pk)] for n, b in BATCHES.items()}
    for n, b in BATCHES.items():
        have = set(masks[n])
        assert 0 in have and VERIFY_POW in have, n
    every = set(m for ms in masks.values() for m in ms)
    assert {0, VERIFY_POW, VERIFY_POW | VERIFY_CHANNEL, VERIFY_CHANNEL} <= every
    # CHANNEL alone from a cause behind the nonce: the flipped index
    for n, b in BATCHES.items():
        for name, m in zip(b.names, masks[n]):
            if name.startswith(("index", "flipped_index")):
                assert m == VERIFY_CHANNEL
    rag = BATCHES["FRI ragged 4 bits"]
    m = masks["FRI ragged 4 bits"]
    assert rag.pk.batch == 67 == pc.RAGGED_MEMBERS
    assert len(set(rag.nls)) >= 4 and set(rag.states) == {"", pc.S1, pc.S2}
    assert any(a == 0 and b != 0 for a, b in zip(m, m[1:])) and any(a != 0 and b == 0 for a, b in zip(m, m[1:]))
    assert m[64:] != [0, 0, 0] and 0 in m[64:]                   # the ragged wave holds both
    nonces = [int(v) for v in rag.pk.nonces]
    ok_hi = [v for v, k in zip(nonces, m) if k == 0 and v >> 32]
    assert any(v >> 32 == 1 for v in ok_hi) and any(v >> 63 for v in ok_hi)
    assert any(0 < v < 2 ** 32 for v, k in zip(nonces, m) if k == 0)
    assert int(BATCHES["FRI one-element layer 8 bits"].pk.shape.max_layers) == 4       # log_n 3: depth 0 at the last
    for n in ("fibsq (3,2,2) 8 bits", "fibsq (3,2,3) 4 bits, high words"):
        assert BATCHES[n].pk.shape.trace_count == 3 and "" in BATCHES[n].states and len(set(BATCHES[n].states)) == 2
    assert any(v >> 32 for v in BATCHES["fibsq (3,2,3) 4 bits, high words"].pk.nonces)


# ---- the packer -------------------------------------------------------------
def test_packer_counts_places_and_refuses_the_nonce():
    g = pc.fri_ground(507, 16, 6, 2, 63, "", pc.HIGH32)
    plain_g = pc.fri_ground(507, 16, 6, 2, 63, "", pc.GRIND8)
    assert g.nonce >> 32 == 1
    pos, msgs = g.pos, g.msgs
    batch = [msgs,
             msgs[:pos] + msgs[pos + 1:],                         # the nonce is missing
             msgs[:pos] + [msgs[pos][4:]] + msgs[pos + 1:],       # 4 bytes
             msgs[:pos] + [msgs[pos]] * 2 + msgs[pos + 1:],       # doubled
             plain_g.msgs]
    pk = fri_amd.pack_transcripts(batch, 6, [g.nl] * 5, 2, 63, grinding_bits=4)
    assert [int(r) for r in pk.reasons] == [0, VERIFY_MALFORMED, VERIFY_MALFORMED, VERIFY_MALFORMED, 0]
    assert not pk.host.any() and pk.grinding_bits == 4
    assert pk.nonces.dtype == np.uint64 and pk.nonces.shape == (5,)
    assert [int(v) for v in pk.nonces] == [g.nonce, 0, 0, 0, plain_g.nonce]
    for b in range(5):
        assert fri_amd.verify_fri(batch[b], 6, g.nl, 2, 63, grinding_bits=4) == (b in (0, 4))
    # the message count with and without bits: a ground transcript packed without is malformed,
    # and a plain one packed with bits
    per_q = 1 + 4 * g.nl
    assert len(msgs) == 2 * g.nl + 1 + 2 * per_q and len(g.plain) == 2 * g.nl + 2 * per_q
    pk0 = fri_amd.pack_transcripts([msgs, g.plain], 6, [g.nl] * 2, 2, 63, grinding_bits=0)
    assert [int(r) for r in pk0.reasons] == [VERIFY_MALFORMED, 0] and [int(v) for v in pk0.nonces] == [0, 0]
    pk4 = fri_amd.pack_transcripts([msgs, g.plain], 6, [g.nl] * 2, 2, 63, grinding_bits=4)
    assert [int(r) for r in pk4.reasons] == [0, VERIFY_MALFORMED]
    # the round trip
    assert fri_amd.unpack_transcripts(pk4) == [msgs, None]
    assert fri_amd.unpack_transcripts(pk0) == [None, g.plain]
    # grinding_bits = 0 is the call without the argument, array by array
    old = fri_amd.pack_transcripts([msgs, g.plain], 6, [g.nl] * 2, 2, 63)
    assert old.grinding_bits == 0
    for f in ("chan", "n_layers", "head", "indices", "values", "paths", "reasons", "host", "nonces"):
        a, b = getattr(old, f), getattr(pk0, f)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), f
    assert old.a_last is None and pk0.a_last is None and bytes(old.shape) == bytes(pk0.shape)
    assert len(old.abi_args()) == 12 == len(pk4.abi_args())
    for bits in (33, -1):
        with pytest.raises(fri_amd.FriError) as e:
            fri_amd.pack_transcripts([msgs], 6, [g.nl], 2, 63, grinding_bits=bits)
        assert e.value.code == fri_amd.FRI_EINVAL


def test_fibsq_packer_places_the_nonce_behind_the_final_value():
    g = pc.fibsq_ground(7, 3, 2, 3, "", pc.HIGH63)
    assert g.nonce >> 63 and g.pos == 4 + 2 * g.nl
    pk = fri_amd.pack_transcripts([g.msgs], 5, [g.nl], 3, 23, 3, 3, 2, [g.a_last], grinding_bits=4)
    assert int(pk.reasons[0]) == 0 and int(pk.nonces[0]) == g.nonce
    assert fri_amd.unpack_transcripts(pk) == [g.msgs]


# ---- argument errors that open no context -----------------------------------
def test_grinding_bits_out_of_range_open_no_context():
    for bits in (33, -1):
        for fn in (lambda: fri_amd.verify_fri_batch([], 6, [], 2, 63, grinding_bits=bits),
                   lambda: fri_amd.verify_fibsq_batch([], [], 3, 2, 2, [], grinding_bits=bits),
                   lambda: fri_amd.verify_fri_batch([[b"x"]], 6, [1], 2, 63, grinding_bits=bits),
                   lambda: fri_amd.verify_fibsq_batch([[b"x"]], [1], 3, 2, 2, [1], grinding_bits=bits)):
            with pytest.raises(fri_amd.FriError) as e:
                fn()
            assert e.value.code == fri_amd.FRI_EINVAL
    reasons = [7]
    assert fri_amd.verify_fri_batch([], 6, [], 2, 63, grinding_bits=8, reasons=reasons) == [] and reasons == []
    assert fri_amd.verify_fibsq_batch([], [], 3, 2, 2, [], grinding_bits=32) == []
    # members the packer decides need no device either
    g = pc.fri_ground(507, 16, 6, 2, 63, "", pc.GRIND8)
    reasons = []
    assert fri_amd.verify_fri_batch([g.msgs[:g.pos] + g.msgs[g.pos + 1:]], 6, [g.nl], 2, 63, grinding_bits=8,
                                    reasons=reasons) == [False]
    assert reasons == [VERIFY_MALFORMED]


def test_header_and_ctypes_table_agree():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "stark-prover_amd")], check=True)
    lib = fri_amd.load_library()
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    types = {"fri_ctx*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
             "const uint32_t*": u32p, "uint32_t*": u32p, "const uint64_t*": u64p,
             "const uint8_t*": ctypes.POINTER(ctypes.c_uint8),
             "const fri_verify_shape*": ctypes.POINTER(fri_amd.VerifyShape),
             "const fri_channel_state*": ctypes.POINTER(fri_amd.ChannelState)}
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    plain = ["fri_ctx*", "const fri_verify_shape*", "uint32_t", "const fri_channel_state*", "const uint32_t*",
             "const uint32_t*", "const uint32_t*", "size_t", "const uint64_t*", "const uint32_t*", "size_t",
             "const uint8_t*", "size_t"]
    want = {"fri_verify_batch": plain + ["uint32_t*"],
            "fri_verify_batch_pow": plain + ["uint32_t", "const uint64_t*", "uint32_t*"]}
    for name, params in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        got = [re.sub(r"\s*\b\w+$", "", " ".join(p.split())).replace(" *", "*") for p in m.group(1).split(",")]
        assert got == params, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and [types[p] for p in params] == list(fn.argtypes), name
    m = re.search(r"#define\s+FRI_VERIFY_POW\s+(\d+)u", src)
    assert m and int(m.group(1)) == fri_amd.VERIFY_POW == 128
    bits = [fri_amd.VERIFY_CHANNEL, fri_amd.VERIFY_TRACE_PATH, fri_amd.VERIFY_COMPOSITION, fri_amd.VERIFY_FRI_PATH,
            fri_amd.VERIFY_FOLD, fri_amd.VERIFY_FINAL, fri_amd.VERIFY_MALFORMED, fri_amd.VERIFY_POW]
    assert bits == [1 << i for i in range(8)]
    # a null context is refused with nothing written
    verdict = (ctypes.c_uint32 * 2)(5, 5)
    sh = fri_amd.VerifyShape(6, 1, 0, 0, 0, 0, 5, 63)
    chs = (fri_amd.ChannelState * 2)()
    nl, nn = (ctypes.c_uint32 * 2)(1, 1), (ctypes.c_uint64 * 2)(0, 0)
    assert lib.fri_verify_batch_pow(None, ctypes.byref(sh), 2, chs, nl, None, nl, 9, None, None, 0, None, 0, 8, nn,
                                    verdict) == fri_amd.FRI_EINVAL
    assert list(verdict) == [5, 5]
    hdr = open(HDR).read()
    assert "profiles/verify_batch_pow.txt" in hdr
    assert os.path.exists(os.path.join(ROOT, "profiles", "verify_batch_pow.txt"))
