"""CPU: the host side of fri_commit_batch.  The header declares the new
entries (tests/test_abi_host.py then checks the library exports them), each
refuses a null context, and the Python mirror's padding, empty-list path and
per-member FRIProof bookkeeping run against a stub context: no device."""
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

ENTRIES = ("fri_commit_batch", "fri_commit_batch_device", "fri_batch_info", "fri_batch_layer_copy",
           "fri_batch_tree_level_copy", "fri_batch_commit_degrees", "fri_batch_decommit_query")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "stark-prover_amd")], check=True)
    return fri_amd.load_library()


def test_header_declares_the_batch_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    cap = int(re.search(r"#define\s+FRI_BATCH_MAX_LOG_N\s+(\d+)", src).group(1))
    assert 14 <= cap <= 18 and cap == fri_amd.BATCH_MAX_LOG_N
    assert int(re.search(r"#define\s+FRI_BATCH_LDE_LDS_MAX_LOG_N\s+(\d+)", src).group(1)) == fri_amd.BATCH_LDE_LDS_MAX_LOG_N
    # the cap's comment names the profile it came from
    assert "profiles/commit_batch.txt" in open(HDR).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "commit_batch.txt"))


def test_every_entry_refuses_a_null_context(lib):
    c = np.zeros(8, dtype=np.uint32)
    res, status = (fri_amd.CommitResult * 2)(), (ctypes.c_int * 2)()
    g, a, b = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    buf, ln = ctypes.create_string_buffer(64), ctypes.c_size_t()
    deg = (ctypes.c_int32 * 4)()
    E = fri_amd.FRI_EINVAL
    assert lib.fri_commit_batch(None, fri_amd._ptr(c), 4, 2, 10, 5, None, 0, None, res, status) == E
    assert lib.fri_commit_batch_device(None, c.ctypes.data, 4, 2, 10, 5, None, 0, None, res, status) == E
    assert lib.fri_batch_info(None, ctypes.byref(g), ctypes.byref(a), ctypes.byref(b)) == E
    assert lib.fri_batch_layer_copy(None, 0, 0, fri_amd._ptr(c), 8) == E
    assert lib.fri_batch_tree_level_copy(None, 0, 0, 0, buf, 64) == E
    assert lib.fri_batch_commit_degrees(None, 0, deg, 4, ctypes.byref(a)) == E
    assert lib.fri_batch_decommit_query(None, 0, 0, fri_amd._ptr(c), 8, buf, 64, ctypes.byref(ln)) == E
    assert list(status) == [0, 0]


def test_ragged_members_are_padded_with_zeros():
    c, d = fri_amd._pack_batch([[1, 2, 3], [], np.array([7], dtype=np.uint32), [4, 5, 6, fri_amd.P - 1, 0]])
    assert d == 5 and c.dtype == np.uint32 and c.shape == (4, 5) and c.flags["C_CONTIGUOUS"]
    assert c.tolist() == [[1, 2, 3, 0, 0], [0] * 5, [7, 0, 0, 0, 0], [4, 5, 6, fri_amd.P - 1, 0]]
    c, d = fri_amd._pack_batch([[], []])
    assert d == 0 and c.shape == (2, 0)
    c, d = fri_amd._pack_batch([])
    assert d == 0 and c.shape[0] == 0
    with pytest.raises(fri_amd.FriError):
        fri_amd._pack_batch([[1], [fri_amd.P]])          # not canonical: refused on the host, as _u32 does


def test_empty_list_touches_no_device():
    assert fri_amd.fri_commit_batch([], 10, []) == []    # (no context is opened: none could be, here)
    with pytest.raises(fri_amd.FriError):
        fri_amd.fri_commit_batch([[1, 2]], 10, [])       # one channel per polynomial


def test_openings_are_taken_apart_per_layer():
    """_openings (behind decommit_query, batch_decommit_query and
    batch_round_records) on a hand-built record of log_n = 3, n_layers = 2:
    three trace values and five trace-path bytes come first."""
    values = np.array([91, 92, 93, 10, 11, 20, 21], dtype=np.uint32)
    p0, s0, p1, s1 = bytes([1]) * 96, bytes([2]) * 96, bytes([3]) * 64, bytes([4]) * 64
    raw = b"trace" + p0 + s0 + p1 + s1
    assert fri_amd._openings(values, raw, 2, 3, 3, 5) == [(10, 11, p0, s0), (20, 21, p1, s1)]
    assert fri_amd._openings(values[3:], raw[5:], 2, 3) == [(10, 11, p0, s0), (20, 21, p1, s1)]
    assert fri_amd._openings(values, raw, 1, 3, 3, 5) == [(10, 11, p0, s0)]
    got = fri_amd._openings(values, raw, 2, 3, 3, 5)
    assert all(type(v) is int for t in got for v in t[:2]) and all(type(b) is bytes for t in got for b in t[2:])
    # a 1-element last layer has empty paths: log_n = 1 folded once
    a, b = bytes([7]) * 32, bytes([8]) * 32
    assert fri_amd._openings([5, 6, 9, 9], a + b, 2, 1) == [(5, 6, a, b), (9, 9, b"", b"")]
    assert fri_amd._openings([5, 6, 9, 9], a + b, 0, 1) == []
    # batch_round_records goes through it: one trace opening, then the two layers
    tl = 96
    paths = np.frombuffer(bytes([9]) * tl + p0 + s0 + p1 + s1 + b"junk", dtype=np.uint8)
    trace, openings = fri_amd.batch_round_records(values[2:], paths, tl + 320, 1, 2, 3)
    assert trace == [(93, bytes([9]) * tl)] and openings == [(10, 11, p0, s0), (20, 21, p1, s1)]
    with pytest.raises(fri_amd.FriError):
        fri_amd.batch_round_records(values[2:], paths, tl + 320, 1, 1, 3)     # the record holds two layers
    assert fri_amd._digests(a + b) == [a, b] and fri_amd._digests(b"") == []


class StubContext:
    """What fri_commit_batch and BatchMember call of a Context, recorded."""
    n_ranks = 1

    def __init__(self, log_n, n_layers):
        self.log_n, self.n_layers, self.gen, self.members, self.calls = log_n, n_layers, 41, 0, []

    def commit_batch(self, polys, log_n, offset=5, channel_states=None, forced_betas=None):
        self.gen += 1
        self.members = len(polys)
        self.calls.append(("commit_batch", len(polys), log_n, offset, list(channel_states)))
        out = []
        for b in range(len(polys)):
            r = fri_amd.CommitResult()
            r.n_layers, r.n_rounds, r.log_n, r.final_value, r.final_degree = self.n_layers, self.n_layers - 1, log_n, 100 + b, 0
            for k in range(self.n_layers):
                r.roots[k][:] = bytes([16 * b + k] * 32)
            for k in range(self.n_layers - 1):
                r.betas[k] = 1000 * b + k
            r.channel_out.digest[:] = bytes([200 + b] * 32)
            r.channel_out.has_state = 1
            out.append(r)
        return out

    def batch_info(self):
        return self.gen, self.members, self.log_n if self.members else 0

    def batch_commit_degrees(self, member):
        return list(range(self.n_layers - 1, -1, -1))

    def batch_layer(self, member, k, log_n):
        self.calls.append(("layer", member, k, log_n))
        return np.full(1 << (log_n - k), member, dtype=np.uint32)

    def batch_decommit_query(self, member, index, n_layers, log_n):
        self.calls.append(("decommit", member, index, n_layers, log_n))
        return [(member, k, bytes([k]) * (32 * (log_n - k)), bytes([k + 1]) * (32 * (log_n - k))) for k in range(n_layers)]


def test_proofs_remember_their_member():
    stub = StubContext(log_n=4, n_layers=3)
    chans = [fri_amd.Channel() for _ in range(3)]
    chans[1].send(b"before")
    st1 = chans[1].state
    proofs = fri_amd.fri_commit_batch([[1, 2], [3], [4, 5, 6]], 4, chans, ctx=stub)
    assert stub.calls[0] == ("commit_batch", 3, 4, 5, [None, bytes.fromhex(st1), None])
    assert [p.member for p in proofs] == [0, 1, 2] and all(p.generation == 42 for p in proofs)
    for b, (p, ch) in enumerate(zip(proofs, chans)):
        assert isinstance(p.ctx, fri_amd.BatchMember) and p.ctx.member == b
        assert p.roots == [bytes([16 * b + k] * 32) for k in range(3)] and p.betas == [1000 * b, 1000 * b + 1]
        own = ch.proof[1:] if b == 1 else ch.proof       # each member's messages went to its own channel
        assert own == [p.roots[0].hex().encode(), p.betas[0].to_bytes(8, "big"), p.roots[1].hex().encode(),
                       p.betas[1].to_bytes(8, "big"), p.roots[2].hex().encode(), (100 + b).to_bytes(8, "big")]
        assert ch.state == bytes([200 + b] * 32).hex()
    assert proofs[2].layer(1).tolist() == [2] * 8 and stub.calls[-1] == ("layer", 2, 1, 4)
    # decommitments and authentication paths go to the member's read-backs
    ch = fri_amd.Channel()
    ch.send(b"x")
    fri_amd.decommit_fri_layers(9, proofs[1], ch)
    assert stub.calls[-1] == ("decommit", 1, 9, 3, 4) and len(ch.proof) == 1 + 4 * 3
    path = proofs[2].fri_merkles[1].get_authentication_path(3)
    assert stub.calls[-1] == ("decommit", 2, 3, 3, 4) and path == bytes([1]) * (32 * 3)
    # a later commit on the context replaces every member's layers
    stub.gen += 1
    stub.members = 0
    for call in (lambda: proofs[0].layer(0), lambda: fri_amd.decommit_fri_layers(1, proofs[0], ch),
                 lambda: proofs[0].fri_merkles[0].get_authentication_path(0)):
        with pytest.raises(fri_amd.FriError) as e:
            call()
        assert e.value.code == fri_amd.FRI_ESTATE
