"""CPU: the host side of the batched prover.  The header declares the three
new entries with the argument lists the Python ctypes table binds (the
library then exports them: tests/test_abi_host.py), each refuses a null
context, and the Python mirrors' argument errors and empty paths need no
device."""
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

ENTRIES = ("fri_trace_commit_batch", "fri_fibsq_composition_commit_batch", "fri_batch_query_round")

# C parameter type -> the ctypes type the table must bind it with
U32, SZ = ctypes.c_uint32, ctypes.c_size_t
CTYPES = {
    "fri_ctx*": ctypes.c_void_p,
    "uint32_t": U32,
    "uint64_t": ctypes.c_uint64,
    "size_t": SZ,
    "const uint32_t*": ctypes.POINTER(U32),
    "uint32_t*": ctypes.POINTER(U32),
    "const uint64_t*": ctypes.POINTER(ctypes.c_uint64),
    "const uint8_t*": ctypes.POINTER(ctypes.c_uint8),
    "size_t*": ctypes.POINTER(SZ),
    "int*": ctypes.POINTER(ctypes.c_int),
    "const fri_channel_state*": ctypes.POINTER(fri_amd.ChannelState),
    "fri_commit_result*": ctypes.POINTER(fri_amd.CommitResult),
}
# output byte buffers: the table binds them as a byte pointer or as a string buffer
BYTES_OUT = (ctypes.POINTER(ctypes.c_uint8), ctypes.c_char_p)


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
    for name in ENTRIES:
        params = _prototype(name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for i, (c, bound) in enumerate(zip(params, fn.argtypes)):
            if c == "uint8_t*":
                assert bound in BYTES_OUT, (name, i, c)
            else:
                assert bound is CTYPES[c], (name, i, c, bound)
    # the composition's batch sits with the shape, before the per-member arrays
    assert _prototype("fri_fibsq_composition_commit_batch")[:5] == ["fri_ctx*"] + ["uint32_t"] * 4
    hdr = open(HDR).read()
    assert "profiles/prove_batch.txt" in hdr and os.path.exists(os.path.join(ROOT, "profiles", "prove_batch.txt"))


def test_every_entry_refuses_a_null_context(lib):
    w = np.zeros(16, dtype=np.uint32)
    idx = (ctypes.c_uint64 * 2)()
    roots = ctypes.create_string_buffer(64)
    res, status = (fri_amd.CommitResult * 2)(), (ctypes.c_int * 2)()
    chs = (fri_amd.ChannelState * 2)()
    pbuf = (ctypes.c_uint8 * 64)()
    ln = (ctypes.c_size_t * 2)()
    E = fri_amd.FRI_EINVAL
    assert lib.fri_trace_commit_batch(None, fri_amd._ptr(w), 3, 1, 5, 2, roots) == E
    assert lib.fri_fibsq_composition_commit_batch(None, 3, 1, 5, 2, fri_amd._ptr(w), fri_amd._ptr(w), chs, 0, res,
                                                  status) == E
    assert lib.fri_batch_query_round(None, idx, None, 0, 0, fri_amd._ptr(w), 8, pbuf, 32, ln) == E
    assert list(status) == [0, 0] and roots.raw == bytes(64) and list(ln) == [0, 0]


def test_mirror_argument_errors_need_no_device():
    assert fri_amd.prove_fibsq_batch([], 6, 3, 2, []) == []          # (no context is opened: none could be, here)
    with pytest.raises(fri_amd.FriError) as e:
        fri_amd.prove_fibsq_batch([3, 4], 6, 3, 2, [fri_amd.Channel()])
    assert e.value.code == fri_amd.FRI_EINVAL
    fri_amd.decommit_fri_batch(3, 63, [], [])
    with pytest.raises(fri_amd.FriError) as e:
        fri_amd.decommit_fri_batch(3, 63, [], [fri_amd.Channel()])
    assert e.value.code == fri_amd.FRI_EINVAL


def test_round_records_take_a_record_apart():
    log_n, tc, nl = 3, 2, 4                                          # layers of 8, 4, 2 and 1 elements
    values = np.arange(100, 100 + tc + 2 * nl, dtype=np.uint32)
    plen = tc * 32 * log_n + sum(64 * (log_n - k) for k in range(nl))
    paths = np.arange(plen + 5, dtype=np.uint32).astype(np.uint8)
    trace, openings = fri_amd.batch_round_records(values, paths, plen, tc, nl, log_n)
    raw = paths.tobytes()
    assert trace == [(100, raw[0:96]), (101, raw[96:192])]
    assert [(v, s) for v, s, _, _ in openings] == [(102, 103), (104, 105), (106, 107), (108, 109)]
    assert openings[0][2:] == (raw[192:288], raw[288:384]) and openings[1][2:] == (raw[384:448], raw[448:512])
    assert openings[3][2:] == (b"", b"")                              # the 1-element layer: no path
    with pytest.raises(fri_amd.FriError):
        fri_amd.batch_round_records(values, paths, 0, tc, nl, log_n)  # a member that was left out
