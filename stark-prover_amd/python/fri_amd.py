"""fri_amd — Python host mirror of the reference FRI-commit interface over
``libfri_amd.so`` (C ABI: include/fri_amd.h).

Mirrors the reference crate's surface for this path (same names, argument
meaning, error behaviour):

* ``Channel``            — src/channel/channel.rs (send / receive_random_field_element /
                           receive_random_int / proof / proof_size)
* ``MerkleTree``         — src/merkle/mod.rs (``MerkleTree(values).root() -> hex str``)
* ``fri_commit``         — src/fri/fri_commit.rs:72-122, returns ``FRIProof``
* ``lde`` / ``interpolate`` / ``evaluate`` / ``batch_inverse`` / ``fold`` — the
  polynomial / field kernels (src/polynomial/ops.rs, interpolation.rs,
  src/fields/element.rs, src/fri/fri_commit.rs:53-65).
* ``poly_mul`` / ``poly_div_rem`` / ``poly_compose`` — Polynomial::mul_assign,
  div_rem and compose (src/polynomial/ops.rs:114-237) on the device;
  ``poly_add`` / ``poly_sub`` / ``poly_scalar_mul`` — the O(n) ones on the host.

Every compute call goes through the HIP library; there is no CPU fallback.
If the library or a gfx950 GPU is missing the calls raise ``FriError``.
Where the reference panics, these raise ``FriError`` as well.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

P = 3221225473
GENERATOR = 5
MAX_ROUNDS = 32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", os.environ.get("FRI_AMD_LIB", "libfri_amd.so")))
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "fri_amd.h"))

FRI_OK, FRI_EINVAL, FRI_ENOMEM, FRI_EHIP, FRI_ENODEV, FRI_ERCCL, FRI_ESTATE, FRI_EDEGREE = range(8)
FLAG_FORCE_BETAS = 1
FLAG_NO_GRAPH = 2
FLAG_RANK_INPUTS = 4      # FRI_FLAG_RANK_INPUTS (fri_amd.h): team commit from the ranks' resident inputs
MAX_INFLIGHT = 4          # FRI_MAX_INFLIGHT (fri_amd.h): pipelined commits pending per context
DEFAULT_LANES = 3         # FRI_DEFAULT_LANES (fri_amd.h): commit lanes of a context
BATCH_MAX_LOG_N = 18      # FRI_BATCH_MAX_LOG_N (fri_amd.h): largest codeword of fri_commit_batch
BATCH_LDE_LDS_MAX_LOG_N = 12   # FRI_BATCH_LDE_LDS_MAX_LOG_N: the batch's LDE runs in LDS up to here
BATCH_MAX = 65535         # members of one fri_commit_batch call
POLY_FORCE_NTT = 1        # FRI_POLY_FORCE_* (fri_amd.h): fri_poly_mul's test/measurement hooks
POLY_FORCE_DIRECT = 2
POLY_DIRECT_LIMIT = 4096  # FRI_POLY_DIRECT_LIMIT: the direct kernel's hard limit (short operand)
POLY_DIRECT_MAX = 1024    # FRI_POLY_DIRECT_MAX: fri_poly_mul's measured crossover to the direct kernel
ROOTS_SMALL_LEAF = 1      # FRI_ROOTS_SMALL_LEAF: fri_poly_from_roots' test/measurement hook (leaves of 64 roots)
ROOTS_LEAF = 512          # FRI_ROOTS_LEAF: roots per LDS leaf subtree of the product tree
LAGRANGE_MAX = 4096       # FRI_LAGRANGE_MAX: fri_lagrange_basis' largest n
MP_FORCE_TREE = 1         # FRI_MP_FORCE_*: fri_evaluate_ex / fri_interpolate_points_ex test/measurement hooks
MP_FORCE_DIRECT = 2
MP_SMALL_LEAF = 4         # FRI_MP_SMALL_LEAF: leaf subtrees of 64 points
MP_EVAL_MIN = 65536       # FRI_MP_EVAL_MIN: evaluation takes the tree from min(d, count) >= this
MP_INTERP_MIN = 65536     # FRI_MP_INTERP_MIN: arbitrary-point interpolation takes the tree from n >= this
VERIFY_MAX_QUERIES = 1024   # FRI_VERIFY_MAX_QUERIES: queries per member of fri_verify_batch
GRIND_MAX_BITS = 32         # fri_grind: leading zero bits of the state after the nonce's send
# The provers grind on the host (hashlib) below this many bits and on the
# device (fri_grind / fri_grind_batch) from it up: the smallest measured size
# from which the whole device call, about 32 us with its launches, read-back
# and copies, beats the hashlib loop (78.6 us at 8 bits, 11.5 at 6;
# profiles/grind.txt, table (v), rows 6 and 8, from tools/grind_probe.py)
GRIND_DEVICE_MIN_BITS = 8
# FRI_VERIFY_*: the verdict bits of fri_verify_batch (0 = accepted)
VERIFY_CHANNEL, VERIFY_TRACE_PATH, VERIFY_COMPOSITION, VERIFY_FRI_PATH = 1, 2, 4, 8
VERIFY_FOLD, VERIFY_FINAL, VERIFY_MALFORMED = 16, 32, 64
VERIFY_POW = 128            # the state after the nonce's send lacks the grinding bits (fri_verify_batch_pow)


class FriError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fri_amd error {code}: {msg}")
        self.code = code


class ChannelState(ctypes.Structure):
    _fields_ = [("digest", ctypes.c_uint8 * 32), ("has_state", ctypes.c_uint32)]


class CommitResult(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_uint32), ("n_rounds", ctypes.c_uint32), ("log_n", ctypes.c_uint32),
                ("final_value", ctypes.c_uint32), ("final_degree", ctypes.c_int32),
                ("reserved", ctypes.c_uint32),
                ("roots", (ctypes.c_uint8 * 32) * (MAX_ROUNDS + 1)),
                ("betas", ctypes.c_uint32 * MAX_ROUNDS),
                ("channel_out", ChannelState)]


class VerifyShape(ctypes.Structure):
    """fri_verify_shape: the shape every member of a fri_verify_batch shares."""
    _fields_ = [("log_n", ctypes.c_uint32), ("max_layers", ctypes.c_uint32), ("num_queries", ctypes.c_uint32),
                ("trace_count", ctypes.c_uint32), ("log_t", ctypes.c_uint32), ("log_blowup", ctypes.c_uint32),
                ("offset", ctypes.c_uint32), ("max_index", ctypes.c_uint64)]


class Collectives(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p),
                ("allgather", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_size_t)),
                ("alltoall", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t)),
                ("sendrecv", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_int))]


class TransportOp(ctypes.Structure):
    """fri_transport_op: one entry of fri_debug_transport_log."""
    _fields_ = [("chan", ctypes.c_uint32), ("op", ctypes.c_uint32), ("peer", ctypes.c_int32),
                ("reserved", ctypes.c_uint32), ("bytes", ctypes.c_uint64)]


TRANSPORT_OPS = {1: "allgather", 2: "alltoall", 3: "sendrecv"}
TRANSPORTS = ("none", "rccl", "host", "loopback", "peer")     # FRI_TRANSPORT_* (fri_amd.h)

_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libfri_amd.so; raises FriError if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FriError(FRI_ENODEV, f"{path} missing: build it with `make -C stark-prover_amd`")
    lib = ctypes.CDLL(path)
    u32, sz, i32 = ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int
    pu32 = ctypes.POINTER(ctypes.c_uint32)
    vp = ctypes.c_void_p
    sig = {
        "fri_ctx_create": (i32, [i32, u32, ctypes.POINTER(vp)]),
        "fri_ctx_create_multi": (i32, [ctypes.POINTER(i32), u32, u32, i32, ctypes.POINTER(vp)]),
        "fri_debug_team_rank": (i32, [vp, u32, ctypes.POINTER(vp)]),
        "fri_debug_team_inject_failure": (i32, [vp, u32, ctypes.c_int64]),
        "fri_ctx_destroy": (i32, [vp]),
        "fri_last_error": (ctypes.c_char_p, [vp]),
        "fri_version": (ctypes.c_char_p, []),
        "fri_batch_inverse": (i32, [vp, pu32, pu32, sz]),
        "fri_lde": (i32, [vp, pu32, sz, u32, u32, pu32]),
        "fri_interpolate": (i32, [vp, pu32, u32, u32, pu32, ctypes.POINTER(sz)]),
        "fri_interpolate_points": (i32, [vp, pu32, pu32, sz, pu32, ctypes.POINTER(sz)]),
        "fri_evaluate": (i32, [vp, pu32, sz, pu32, sz, pu32]),
        "fri_evaluate_ex": (i32, [vp, pu32, sz, pu32, sz, u32, pu32]),
        "fri_interpolate_points_ex": (i32, [vp, pu32, pu32, sz, u32, pu32, ctypes.POINTER(sz)]),
        "fri_poly_mul": (i32, [vp, pu32, sz, pu32, sz, u32, pu32, sz, ctypes.POINTER(sz)]),
        "fri_poly_div_rem": (i32, [vp, pu32, sz, pu32, sz, pu32, sz, ctypes.POINTER(sz), pu32, sz,
                                   ctypes.POINTER(sz)]),
        "fri_poly_compose": (i32, [vp, pu32, sz, pu32, sz, pu32, sz, ctypes.POINTER(sz)]),
        "fri_poly_from_roots": (i32, [vp, pu32, sz, u32, pu32, sz, ctypes.POINTER(sz)]),
        "fri_lagrange_basis": (i32, [vp, pu32, sz, pu32, sz]),
        "fri_debug_set_roots_leaf": (i32, [vp, u32]),
        "fri_fold": (i32, [vp, pu32, u32, u32, u32, pu32]),
        "fri_merkle_root": (i32, [vp, pu32, sz, ctypes.c_char_p]),
        "fri_commit": (i32, [vp, pu32, sz, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                             ctypes.POINTER(CommitResult)]),
        "fri_commit_device": (i32, [vp, vp, sz, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                    ctypes.POINTER(CommitResult)]),
        "fri_commit_device_async": (i32, [vp, vp, sz, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                          ctypes.POINTER(ctypes.c_uint64)]),
        "fri_commit_wait": (i32, [vp, ctypes.c_uint64, ctypes.POINTER(CommitResult)]),
        "fri_commit_async": (i32, [vp, pu32, sz, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                   ctypes.POINTER(ctypes.c_uint64)]),
        "fri_ctx_input_buffer": (i32, [vp, sz, ctypes.POINTER(vp)]),
        "fri_ctx_input_upload": (i32, [vp, pu32, sz]),
        "fri_ctx_create_default": (i32, [u32, ctypes.POINTER(vp), ctypes.POINTER(u32)]),
        "fri_debug_team_force_copy": (i32, [vp, i32]),
        "fri_commit_info": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "fri_layer_copy": (i32, [vp, u32, pu32, sz]),
        "fri_tree_level_copy": (i32, [vp, u32, u32, ctypes.c_char_p, sz]),
        "fri_auth_path": (i32, [vp, u32, ctypes.c_uint64, pu32, ctypes.c_char_p, ctypes.POINTER(u32)]),
        "fri_trace_commit": (i32, [vp, pu32, u32, u32, u32, ctypes.c_char_p, pu32, ctypes.POINTER(sz), pu32]),
        "fri_decommit_query": (i32, [vp, ctypes.c_uint64, pu32, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]),
        "fri_fibsq_composition_commit": (i32, [vp, u32, u32, u32, u32, pu32, ctypes.POINTER(ChannelState), u32,
                                               ctypes.POINTER(CommitResult)]),
        "fri_fibsq_trace": (i32, [u32, u32, pu32]),
        "fri_trace_decommit": (i32, [vp, ctypes.c_uint64, ctypes.c_uint64, u32, pu32, ctypes.c_char_p, sz]),
        "fri_set_profiling": (i32, [vp, i32]),
        "fri_get_profile": (i32, [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "fri_reset_profile": (i32, [vp]),
        "fri_debug_inject_stall": (i32, [vp, i32]),
        "fri_debug_attach_loopback": (i32, [vp, i32, i32]),
        "fri_debug_plan_layout": (i32, [sz, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64), sz]),
        "fri_ctx_device_bytes": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "fri_debug_set_device_cap": (i32, [vp, ctypes.c_uint64]),
        "fri_debug_stamps": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), sz]),
        "fri_dist_unique_id": (i32, [ctypes.c_char_p]),
        "fri_dist_attach_rccl": (i32, [vp, i32, i32, ctypes.c_char_p]),
        "fri_dist_attach_host": (i32, [vp, i32, i32, ctypes.POINTER(Collectives)]),
        "fri_dist_detach": (i32, [vp]),
        "fri_dist_info": (i32, [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "fri_dist_selftest": (i32, [vp, sz]),
        "fri_commit_sharded": (i32, [vp, pu32, sz, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                     ctypes.POINTER(CommitResult)]),
        "fri_commit_sharded_device": (i32, [vp, vp, sz, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                            ctypes.POINTER(CommitResult)]),
        "fri_decommit_query_sharded": (i32, [vp, ctypes.c_uint64, pu32, sz, ctypes.c_char_p, sz,
                                             ctypes.POINTER(sz)]),
        "fri_debug_loopback_degrees": (i32, [vp, ctypes.POINTER(ctypes.c_int32), u32]),
        "fri_ctx_set_lanes": (i32, [vp, u32]),
        "fri_debug_ticket_lane": (i32, [vp, ctypes.c_uint64, ctypes.POINTER(i32)]),
        "fri_commit_degrees": (i32, [vp, ctypes.POINTER(ctypes.c_int32), sz, ctypes.POINTER(u32)]),
        "fri_commit_batch": (i32, [vp, pu32, sz, u32, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                   ctypes.POINTER(CommitResult), ctypes.POINTER(i32)]),
        "fri_commit_batch_device": (i32, [vp, vp, sz, u32, u32, u32, ctypes.POINTER(ChannelState), u32, pu32,
                                          ctypes.POINTER(CommitResult), ctypes.POINTER(i32)]),
        "fri_batch_info": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "fri_batch_layer_copy": (i32, [vp, u32, u32, pu32, sz]),
        "fri_batch_tree_level_copy": (i32, [vp, u32, u32, u32, ctypes.c_char_p, sz]),
        "fri_batch_commit_degrees": (i32, [vp, u32, ctypes.POINTER(ctypes.c_int32), sz, ctypes.POINTER(u32)]),
        "fri_batch_decommit_query": (i32, [vp, u32, ctypes.c_uint64, pu32, sz, ctypes.c_char_p, sz,
                                           ctypes.POINTER(sz)]),
        "fri_trace_commit_batch": (i32, [vp, pu32, u32, u32, u32, u32, ctypes.c_char_p]),
        "fri_fibsq_composition_commit_batch": (i32, [vp, u32, u32, u32, u32, pu32, pu32, ctypes.POINTER(ChannelState),
                                                     u32, ctypes.POINTER(CommitResult), ctypes.POINTER(i32)]),
        "fri_batch_query_round": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8), u32,
                                        ctypes.c_uint64, pu32, sz, ctypes.POINTER(ctypes.c_uint8), sz,
                                        ctypes.POINTER(sz)]),
        "fri_batch_query_phase": (i32, [vp, u32, ctypes.c_uint64, ctypes.POINTER(ChannelState),
                                        ctypes.POINTER(ctypes.c_uint8), u32, ctypes.c_uint64,
                                        ctypes.POINTER(ctypes.c_uint64), pu32, sz, ctypes.POINTER(ctypes.c_uint8), sz,
                                        ctypes.POINTER(sz)]),
        "fri_debug_set_query_chunk": (i32, [vp, u32]),
        "fri_grind": (i32, [vp, ctypes.POINTER(ChannelState), u32, ctypes.c_uint64, ctypes.c_uint64,
                            ctypes.POINTER(ctypes.c_uint64), pu32, ctypes.POINTER(ChannelState)]),
        "fri_grind_batch": (i32, [vp, u32, ctypes.POINTER(ChannelState), u32, ctypes.c_uint64,
                                  ctypes.POINTER(ctypes.c_uint64), pu32]),
        "fri_debug_set_grind_window": (i32, [vp, u32]),
        "fri_debug_transport_log": (i32, [vp, ctypes.POINTER(TransportOp), sz, ctypes.POINTER(sz)]),
        "fri_verify_batch": (i32, [vp, ctypes.POINTER(VerifyShape), u32, ctypes.POINTER(ChannelState), pu32, pu32,
                                   pu32, sz, ctypes.POINTER(ctypes.c_uint64), pu32, sz,
                                   ctypes.POINTER(ctypes.c_uint8), sz, pu32]),
        "fri_verify_batch_pow": (i32, [vp, ctypes.POINTER(VerifyShape), u32, ctypes.POINTER(ChannelState), pu32, pu32,
                                       pu32, sz, ctypes.POINTER(ctypes.c_uint64), pu32, sz,
                                       ctypes.POINTER(ctypes.c_uint8), sz, u32, ctypes.POINTER(ctypes.c_uint64),
                                       pu32]),
        "fri_debug_set_verify_chunk": (i32, [vp, u32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _u32(a) -> np.ndarray:
    if isinstance(a, np.ndarray) and a.dtype == np.uint32:
        # no widening copy: every library entry point checks canonicity itself
        # (FRI_EINVAL, raised by _check); the uint64 round trip below cost
        # about 1.5 ms per 2^21 coefficients
        return np.ascontiguousarray(a)
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    if arr.size and int(arr.max()) >= P:
        raise FriError(FRI_EINVAL, "field element not canonical (>= p)")
    return np.ascontiguousarray(arr.astype(np.uint32))


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _openings(values, raw: bytes, n_layers: int, log_n: int, first_value: int = 0, first_byte: int = 0):
    """decommit_query's tuples out of a gather record: layer k's two values from
    values[first_value + 2k:], its two paths of 32 (log_n - k) bytes after the earlier layers' from raw[first_byte:]."""
    out, off, v = [], first_byte, first_value
    for k in range(n_layers):
        pl = 32 * (log_n - k)
        out.append((int(values[v + 2 * k]), int(values[v + 2 * k + 1]), raw[off:off + pl], raw[off + pl:off + 2 * pl]))
        off += 2 * pl
    return out


def _digests(raw: bytes) -> List[bytes]:
    return [raw[i:i + 32] for i in range(0, len(raw), 32)]


def _check_resident(generation: Optional[int], log_n: int, g: int, ln: int, present, what: str) -> None:
    """Read-backs serve only the commit they were asked for: the resident
    codeword (if ``present``) must be 2^log_n and, for a FRIProof, still the
    commit of ``generation`` (a later commit on this context replaced its layers)."""
    if generation is not None and g != generation:
        raise FriError(FRI_ESTATE, "FRIProof layers were replaced by a later commit on the same context")
    if present and ln != log_n:
        raise FriError(FRI_ESTATE, f"resident {what} is 2^{ln}, not 2^{log_n}")


class Context:
    """Owns one fri_ctx (device buffers, stream, graphs) on one GPU, or, from
    ``Context.multi``, a team of ranks on several GPUs behind one context."""

    def __init__(self, device: int = 0, log_n_max: int = 20, _handle=None, _owner=True):
        self.lib = load_library()
        self.device = device
        self.log_n_max = log_n_max
        self.n_ranks = 1
        self._owner = _owner
        if _handle is not None:
            self.h = _handle
            return
        h = ctypes.c_void_p()
        rc = self.lib.fri_ctx_create(device, log_n_max, ctypes.byref(h))
        if rc != FRI_OK:
            raise FriError(rc, "fri_ctx_create failed (no gfx950 device?)")
        self.h = h

    @classmethod
    def multi(cls, devices: Sequence[int], log_n_max: int, transport: str = "auto") -> "Context":
        """fri_ctx_create_multi: ONE context over len(devices) GPUs (ranks;
        a device may repeat), driven from this thread.  commit / commit_device
        of a codeword >= 2^20 run coset-sharded over the ranks in one call;
        every read-back serves the whole commit.  transport: "auto" (the
        peer transport), "peer" or "rccl" (opt-in, distinct devices only)."""
        lib = load_library()
        kinds = {"auto": 0, "rccl": 1, "peer": 4}
        if transport not in kinds:
            raise FriError(FRI_EINVAL, f"transport must be one of {sorted(kinds)}")
        devs = (ctypes.c_int * len(devices))(*[int(x) for x in devices])
        h = ctypes.c_void_p()
        rc = lib.fri_ctx_create_multi(devs, len(devices), log_n_max, kinds[transport], ctypes.byref(h))
        if rc != FRI_OK:
            raise FriError(rc, f"fri_ctx_create_multi({list(devices)}, {log_n_max}, {transport}) failed")
        c = cls(int(devices[0]), log_n_max, _handle=h)
        c.n_ranks = len(devices)
        c.devices = [int(x) for x in devices]
        return c

    @classmethod
    def default(cls, log_n_max: int) -> "Context":
        """fri_ctx_create_default: the devices named by FRI_DEVICES (e.g.
        "0,0,0,0"), else every visible GPU (largest power-of-two count); one
        device is an ordinary context, several a team (peer transport, or
        FRI_TRANSPORT=rccl).  What the reference-shaped functions below use
        when no ctx is passed."""
        lib = load_library()
        h = ctypes.c_void_p()
        n = ctypes.c_uint32()
        rc = lib.fri_ctx_create_default(log_n_max, ctypes.byref(h), ctypes.byref(n))
        if rc != FRI_OK:
            raise FriError(rc, f"fri_ctx_create_default({log_n_max}) failed (FRI_DEVICES="
                               f"{os.environ.get('FRI_DEVICES', '')!r}; no gfx950 device?)")
        first = os.environ.get("FRI_DEVICES", "").split(",")[0].strip()      # rank 0's device (validated by the call)
        c = cls(int(first) if first else 0, log_n_max, _handle=h)
        c.n_ranks = n.value
        return c

    def input_buffer(self, d: int) -> int:
        """Device pointer of the context's input buffer (fri_ctx_input_buffer):
        the caller's; no commit writes it, commits from it read it in place."""
        p = ctypes.c_void_p()
        self._check(self.lib.fri_ctx_input_buffer(self.h, d, ctypes.byref(p)))
        return p.value

    def input_upload(self, coeffs) -> int:
        """Fill the input buffer with host coefficients (fri_ctx_input_upload;
        waits for the pending commits reading it) and return its pointer."""
        c = _u32(coeffs)
        self._check(self.lib.fri_ctx_input_upload(self.h, _ptr(c), c.size))
        return self.input_buffer(c.size)

    def force_copy(self, enable: bool = True):
        """Test hook (fri_debug_team_force_copy): a team's collectives copy with
        hipMemcpyPeerAsync per source instead of the pull kernel."""
        self._check(self.lib.fri_debug_team_force_copy(self.h, 1 if enable else 0))

    def team_rank(self, rank: int) -> "Context":
        """A non-owning view of rank ``rank``'s context (fri_debug_team_rank),
        for its transport log and device bytes."""
        h = ctypes.c_void_p()
        self._check(self.lib.fri_debug_team_rank(self.h, rank, ctypes.byref(h)))
        return Context(self.device, self.log_n_max, _handle=h, _owner=False)

    def inject_team_failure(self, rank: int, op_index: int):
        """Test hook (fri_debug_team_inject_failure): rank `rank` fails its
        op_index-th collective in the next team call."""
        self._check(self.lib.fri_debug_team_inject_failure(self.h, rank, op_index))

    def close(self):
        if self.h and self._owner:
            self.lib.fri_ctx_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != FRI_OK:
            raise FriError(rc, self.lib.fri_last_error(self.h).decode())

    # ---- kernel-level ops ------------------------------------------------
    def batch_inverse(self, xs) -> np.ndarray:
        a = _u32(xs)
        out = np.empty_like(a)
        self._check(self.lib.fri_batch_inverse(self.h, _ptr(a), _ptr(out), a.size))
        return out

    def lde(self, coeffs, log_n: int, offset: int = GENERATOR) -> np.ndarray:
        c = _u32(coeffs)
        out = np.empty(1 << log_n, dtype=np.uint32)
        self._check(self.lib.fri_lde(self.h, _ptr(c), c.size, log_n, offset, _ptr(out)))
        return out

    def interpolate(self, ys, offset: int = GENERATOR) -> np.ndarray:
        y = _u32(ys)
        log_n = int(y.size).bit_length() - 1
        if y.size != 1 << log_n:
            raise FriError(FRI_EINVAL, "coset interpolation needs a power-of-two point count")
        out = np.empty(y.size, dtype=np.uint32)
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_interpolate(self.h, _ptr(y), log_n, offset, _ptr(out), ctypes.byref(ln)))
        return out[: ln.value]

    @staticmethod
    def _mp_flags(mode, small_leaf) -> int:
        return {None: 0, "tree": MP_FORCE_TREE, "direct": MP_FORCE_DIRECT}[mode] | (MP_SMALL_LEAF if small_leaf else 0)

    def interpolate_points(self, xs, ys, mode: Optional[str] = None, small_leaf: bool = False) -> np.ndarray:
        """Polynomial::interpolate(xs, ys) on arbitrary points
        (interpolation.rs:121-152; fri_interpolate_points_ex), trimmed.
        mode: None (the measured choice), "tree" or "direct" (the
        FRI_MP_FORCE_* hooks); small_leaf: the FRI_MP_SMALL_LEAF hook."""
        x, y = _u32(xs), _u32(ys)
        if x.size != y.size:
            raise FriError(FRI_EINVAL, "Mismatched x and y lengths")   # interpolation.rs:127-133 panics
        out = np.empty(max(1, x.size), dtype=np.uint32)
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_interpolate_points_ex(self.h, _ptr(x), _ptr(y), x.size,
                                                       self._mp_flags(mode, small_leaf), _ptr(out), ctypes.byref(ln)))
        return out[: ln.value]

    def evaluate(self, coeffs, xs, mode: Optional[str] = None, small_leaf: bool = False) -> np.ndarray:
        """Polynomial::evaluate at every x (ops.rs:76-83; fri_evaluate_ex);
        mode and small_leaf as for interpolate_points."""
        c, x = _u32(coeffs), _u32(xs)
        out = np.empty(x.size, dtype=np.uint32)
        self._check(self.lib.fri_evaluate_ex(self.h, _ptr(c), c.size, _ptr(x), x.size,
                                             self._mp_flags(mode, small_leaf), _ptr(out)))
        return out

    def poly_mul(self, a, b, force: Optional[str] = None) -> np.ndarray:
        """a * b (Polynomial::mul_assign, ops.rs:114-138; fri_poly_mul), trimmed.
        force: None, "ntt" or "direct" (the FRI_POLY_FORCE_* hooks)."""
        flags = {None: 0, "ntt": POLY_FORCE_NTT, "direct": POLY_FORCE_DIRECT}[force]
        x, y = _u32(a), _u32(b)
        out = np.empty(max(1, x.size + y.size), dtype=np.uint32)
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_poly_mul(self.h, _ptr(x), x.size, _ptr(y), y.size, flags, _ptr(out), out.size,
                                          ctypes.byref(ln)))
        return out[: ln.value]

    def poly_div_rem(self, a, b):
        """(q, r) with a = q*b + r, deg r < deg b (Polynomial::div_rem,
        ops.rs:141-191; fri_poly_div_rem), both trimmed.  A zero divisor
        raises FriError(FRI_EINVAL, "Division by zero polynomial")."""
        x, y = _u32(a), _u32(b)
        q = np.empty(max(1, x.size), dtype=np.uint32)
        r = np.empty(max(1, x.size, y.size), dtype=np.uint32)
        lq, lr = ctypes.c_size_t(), ctypes.c_size_t()
        self._check(self.lib.fri_poly_div_rem(self.h, _ptr(x), x.size, _ptr(y), y.size, _ptr(q), q.size,
                                              ctypes.byref(lq), _ptr(r), r.size, ctypes.byref(lr)))
        return q[: lq.value], r[: lr.value]

    def poly_compose(self, p, q) -> np.ndarray:
        """p(q(x)) (Polynomial::compose, ops.rs:214-237; fri_poly_compose), trimmed."""
        x, y = _u32(p), _u32(q)
        lx = int(np.flatnonzero(x)[-1]) + 1 if x.any() else 0      # trimmed lengths size the output
        ly = int(np.flatnonzero(y)[-1]) + 1 if y.any() else 0
        out = np.empty(max(1, (lx - 1) * (ly - 1) + 1 if lx and ly > 1 else 1), dtype=np.uint32)
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_poly_compose(self.h, _ptr(x), x.size, _ptr(y), y.size, _ptr(out), out.size,
                                              ctypes.byref(ln)))
        return out[: ln.value]

    def poly_from_roots(self, roots, small_leaf: bool = False) -> np.ndarray:
        """Z(x) = prod (x - r) over `roots` (gen_polynomial_from_roots,
        interpolation.rs:9-23; fri_poly_from_roots): n + 1 coefficients, monic;
        no roots give the zero polynomial (length 0).  small_leaf: the
        FRI_ROOTS_SMALL_LEAF hook (leaf subtrees of 64 roots)."""
        r = _u32(roots)
        out = np.empty(r.size + 1, dtype=np.uint32)
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_poly_from_roots(self.h, _ptr(r), r.size, ROOTS_SMALL_LEAF if small_leaf else 0,
                                                 _ptr(out), out.size, ctypes.byref(ln)))
        return out[: ln.value]

    def lagrange_basis(self, xs) -> np.ndarray:
        """The Lagrange basis over `xs` (gen_lagrange_polynomials,
        interpolation.rs:46-78; fri_lagrange_basis): shape (n, n), row i the
        coefficients x^0..x^(n-1) of L_i, untrimmed; the rows of a repeated x
        are zero.  n <= LAGRANGE_MAX."""
        x = _u32(xs)
        out = np.empty((x.size, x.size), dtype=np.uint32)
        self._check(self.lib.fri_lagrange_basis(self.h, _ptr(x), x.size, _ptr(out), out.size))
        return out

    def set_roots_leaf(self, leaf: int):
        """Measurement hook (fri_debug_set_roots_leaf): roots per leaf subtree
        of this context's later poly_from_roots / lagrange_basis calls; 0
        restores ROOTS_LEAF."""
        self._check(self.lib.fri_debug_set_roots_leaf(self.h, leaf))

    def fold(self, layer, layer_offset: int, beta: int) -> np.ndarray:
        v = _u32(layer)
        log_m = int(v.size).bit_length() - 1
        out = np.empty(v.size // 2, dtype=np.uint32)
        self._check(self.lib.fri_fold(self.h, _ptr(v), log_m, layer_offset, beta, _ptr(out)))
        return out

    def merkle_root(self, values) -> bytes:
        v = _u32(values)
        root = ctypes.create_string_buffer(32)
        self._check(self.lib.fri_merkle_root(self.h, _ptr(v), v.size, root))
        return root.raw

    # ---- commit ----------------------------------------------------------
    def commit(self, coeffs, log_n: int, offset: int = GENERATOR, channel_state: Optional[bytes] = None,
               forced_betas: Optional[Sequence[int]] = None, graph: bool = True) -> CommitResult:
        c = _u32(coeffs)
        ch = ChannelState()
        if channel_state:
            ctypes.memmove(ch.digest, channel_state, 32)
            ch.has_state = 1
        flags = 0 if graph else FLAG_NO_GRAPH
        fb = None
        if forced_betas is not None:
            fbarr = np.zeros(MAX_ROUNDS, dtype=np.uint32)
            fbarr[: len(forced_betas)] = forced_betas
            fb = fbarr
            flags |= FLAG_FORCE_BETAS
        res = CommitResult()
        self._check(self.lib.fri_commit(self.h, _ptr(c), c.size, log_n, offset, ctypes.byref(ch), flags,
                                        _ptr(fb) if fb is not None else None, ctypes.byref(res)))
        return res

    def commit_device_async(self, d_coeffs, d: int, log_n: int, offset: int = GENERATOR,
                            channel_state: Optional[bytes] = None) -> int:
        """Enqueue a commit of device-resident coefficients (``d_coeffs``: a
        device pointer, e.g. from fri_ctx_input_buffer) and return its ticket
        at once (fri_commit_device_async; at most MAX_INFLIGHT pending)."""
        ch = ChannelState()
        if channel_state:
            ctypes.memmove(ch.digest, channel_state, 32)
            ch.has_state = 1
        t = ctypes.c_uint64()
        self._check(self.lib.fri_commit_device_async(self.h, d_coeffs, d, log_n, offset, ctypes.byref(ch), 0, None,
                                                     ctypes.byref(t)))
        return t.value

    def commit_async(self, coeffs, log_n: int, offset: int = GENERATOR,
                     channel_state: Optional[bytes] = None) -> int:
        """Enqueue a commit of host coefficients and return its ticket
        (fri_commit_async: the coefficients are copied before it returns)."""
        c = _u32(coeffs)
        ch = ChannelState()
        if channel_state:
            ctypes.memmove(ch.digest, channel_state, 32)
            ch.has_state = 1
        t = ctypes.c_uint64()
        self._check(self.lib.fri_commit_async(self.h, _ptr(c), c.size, log_n, offset, ctypes.byref(ch), 0, None,
                                              ctypes.byref(t)))
        return t.value

    def set_lanes(self, max_lanes: int):
        """Commit lanes of the pipelined commits (fri_ctx_set_lanes): each
        pending commit runs on the lane with the fewest pending commits, each
        lane a stream with its own plan, so consecutive commits overlap."""
        self._check(self.lib.fri_ctx_set_lanes(self.h, max_lanes))

    def ticket_lane(self, ticket: int) -> int:
        """Lane a pending pipelined commit was dealt to (fri_debug_ticket_lane)."""
        lane = ctypes.c_int()
        self._check(self.lib.fri_debug_ticket_lane(self.h, ticket, ctypes.byref(lane)))
        return lane.value

    def commit_wait(self, ticket: int, out: Optional[CommitResult] = None) -> CommitResult:
        """Wait for an enqueued commit and return its result (fri_commit_wait)."""
        res = out if out is not None else CommitResult()
        self._check(self.lib.fri_commit_wait(self.h, ticket, ctypes.byref(res)))
        return res

    # ---- batched commit ----------------------------------------------------
    def commit_batch(self, polys, log_n: int, offset: int = GENERATOR, channel_states=None, forced_betas=None,
                     d_coeffs: Optional[int] = None, d: Optional[int] = None, batch: Optional[int] = None):
        """fri_commit_batch: one CommitResult per member of ``polys`` (ragged
        members are padded with zeros to the longest).  channel_states: per
        member 32 digest bytes or None (fresh); forced_betas: per member a
        sequence of betas (test hook).  With ``d_coeffs`` (a device pointer to
        batch*d words) instead of polys: fri_commit_batch_device.  A member
        that failed raises FriError after the call; ``self.batch_status``
        keeps every member's code."""
        if d_coeffs is None:
            c, d = _pack_batch(polys)
            batch = c.shape[0]
            if batch == 0:
                self.batch_status = []
                return []
        chs = None
        if channel_states is not None:
            if len(channel_states) != batch:
                raise FriError(FRI_EINVAL, "one channel state per member")
            chs = (ChannelState * batch)()
            for b, st in enumerate(channel_states):
                if st:
                    ctypes.memmove(chs[b].digest, st, 32)
                    chs[b].has_state = 1
        flags, fb = 0, None
        if forced_betas is not None:
            if len(forced_betas) != batch:
                raise FriError(FRI_EINVAL, "one sequence of forced betas per member")
            fb = np.zeros((batch, MAX_ROUNDS), dtype=np.uint32)
            for b, row in enumerate(forced_betas):
                fb[b, : len(row)] = row
            flags |= FLAG_FORCE_BETAS
        res = (CommitResult * batch)()
        status = (ctypes.c_int * batch)()
        fbp = _ptr(fb) if fb is not None else None
        if d_coeffs is None:
            rc = self.lib.fri_commit_batch(self.h, _ptr(c), d, batch, log_n, offset, chs, flags, fbp, res, status)
        else:
            rc = self.lib.fri_commit_batch_device(self.h, d_coeffs, d, batch, log_n, offset, chs, flags, fbp, res,
                                                  status)
        self.batch_status = [int(x) for x in status]     # (all zero after a refused call: it writes nothing)
        self.batch_results = list(res)
        self._check(rc)
        return list(res)

    def batch_info(self):
        """(generation, members, log_n) of the resident batch; members = 0 when
        the last commit on the context was not a batch (fri_batch_info)."""
        g, b, ln = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.fri_batch_info(self.h, ctypes.byref(g), ctypes.byref(b), ctypes.byref(ln)))
        return g.value, b.value, ln.value

    def batch_layer(self, member: int, k: int, log_n: int) -> np.ndarray:
        out = np.empty(1 << (log_n - k), dtype=np.uint32)
        self._check(self.lib.fri_batch_layer_copy(self.h, member, k, _ptr(out), out.size))
        return out

    def batch_tree_level(self, member: int, k: int, level: int, log_n: int) -> List[bytes]:
        cnt = 1 << (log_n - k - level)
        buf = ctypes.create_string_buffer(32 * cnt)
        self._check(self.lib.fri_batch_tree_level_copy(self.h, member, k, level, buf, 32 * cnt))
        return _digests(buf.raw)

    def batch_commit_degrees(self, member: int) -> List[int]:
        out = (ctypes.c_int32 * (MAX_ROUNDS + 1))()
        n = ctypes.c_uint32()
        self._check(self.lib.fri_batch_commit_degrees(self.h, member, out, MAX_ROUNDS + 1, ctypes.byref(n)))
        return [int(out[k]) for k in range(n.value)]

    def batch_decommit_query(self, member: int, index: int, n_layers: int, log_n: int):
        """fri_batch_decommit_query: decommit_query's tuples for one member."""
        vals = np.empty(2 * n_layers, dtype=np.uint32)
        total = record_paths_len(log_n, 0, n_layers)
        buf = ctypes.create_string_buffer(max(total, 1))
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_batch_decommit_query(self.h, member, index, _ptr(vals), vals.size, buf, total,
                                                      ctypes.byref(ln)))
        return _openings(vals, buf.raw, n_layers, log_n)

    # ---- batched prover ----------------------------------------------------
    def trace_commit_batch(self, traces, log_blowup: int, offset: int = GENERATOR) -> List[bytes]:
        """fri_trace_commit_batch: the LDE Merkle root of every row of
        ``traces`` (batch x 2^log_t canonical values); LDEs and trees stay
        resident for fibsq_composition_commit_batch and batch_query_round."""
        tr = np.ascontiguousarray(np.stack([_u32(t).reshape(-1) for t in traces])) if len(traces) else \
            np.zeros((0, 0), dtype=np.uint32)
        batch, T = tr.shape
        if batch == 0:
            return []
        log_t = T.bit_length() - 1
        if T != 1 << log_t:
            raise FriError(FRI_EINVAL, "trace length must be a power of two")
        roots = ctypes.create_string_buffer(32 * batch)
        self._check(self.lib.fri_trace_commit_batch(self.h, _ptr(tr), log_t, log_blowup, offset, batch, roots))
        return [roots.raw[32 * b: 32 * b + 32] for b in range(batch)]

    def fibsq_composition_commit_batch(self, log_t: int, log_blowup: int, a_lasts, alphas, offset: int = GENERATOR,
                                       channel_states=None, graph: bool = True):
        """fri_fibsq_composition_commit_batch on the resident trace batch:
        one CommitResult per member.  alphas: three per member;
        channel_states: per member 32 digest bytes or None.  A member that
        failed raises FriError after the call; ``self.batch_status`` keeps
        every member's code and ``self.batch_results`` every result."""
        al_last = _u32(a_lasts).reshape(-1)
        batch = al_last.size
        if not (isinstance(alphas, np.ndarray) and alphas.dtype == np.uint32):
            alphas = np.asarray(alphas, dtype=np.uint64)
        al = _u32(alphas.reshape(-1))
        if al.size != 3 * batch:
            raise FriError(FRI_EINVAL, "three alphas per member")
        if channel_states is None:
            channel_states = [None] * batch
        if len(channel_states) != batch:
            raise FriError(FRI_EINVAL, "one channel state per member")
        chs = (ChannelState * max(batch, 1))()
        for b, st in enumerate(channel_states):
            if st:
                ctypes.memmove(chs[b].digest, st, 32)
                chs[b].has_state = 1
        res = (CommitResult * max(batch, 1))()
        status = (ctypes.c_int * max(batch, 1))()
        rc = self.lib.fri_fibsq_composition_commit_batch(self.h, log_t, log_blowup, offset, batch, _ptr(al_last),
                                                         _ptr(al), chs, 0 if graph else FLAG_NO_GRAPH, res, status)
        self.batch_status = [int(x) for x in status][:batch]
        self.batch_results = list(res)[:batch]
        self._check(rc)
        return self.batch_results

    def batch_query_round(self, indices, skip=None, trace_count: int = 0, trace_stride: int = 0, values=None,
                          paths=None):
        """fri_batch_query_round: one query of every member of the resident
        batch in one launch.  Returns (values, paths, paths_len): uint32
        (batch, values_stride) and uint8 (batch, paths_stride) arrays (the
        caller's, when given) and the bytes written per member, 0 for a
        member that was skipped or whose commit failed.  batch_round_records
        takes a member's record apart."""
        _, members, log_n = self.batch_info()
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64))
        if members and idx.size != members:
            raise FriError(FRI_EINVAL, "one index per member of the resident batch")
        batch = idx.size                          # (no resident batch: the library refuses before it reads any)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(np.asarray(skip, dtype=np.uint8))
            if sk.size != batch:
                raise FriError(FRI_EINVAL, "one skip flag per member")
        nl = log_n + 1
        if values is None:
            values = np.zeros((batch, trace_count + 2 * nl), dtype=np.uint32)
        if paths is None:
            paths = np.zeros((batch, max(record_paths_len(log_n, trace_count, nl), 1)),
                             dtype=np.uint8)
        if values.dtype != np.uint32 or paths.dtype != np.uint8 or values.ndim != 2 or paths.ndim != 2 or \
                values.shape[0] != batch or paths.shape[0] != batch or not values.flags["C_CONTIGUOUS"] or \
                not paths.flags["C_CONTIGUOUS"]:
            raise FriError(FRI_EINVAL, "values: C-contiguous uint32 (batch, stride); paths: uint8 (batch, stride)")
        ln = (ctypes.c_size_t * max(batch, 1))()
        u8p = ctypes.POINTER(ctypes.c_uint8)
        rc = self.lib.fri_batch_query_round(self.h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                            sk.ctypes.data_as(u8p) if sk is not None else None, trace_count,
                                            trace_stride, _ptr(values), values.shape[1], paths.ctypes.data_as(u8p),
                                            paths.shape[1], ln)
        self.round_needed = int(ln[0]) if rc == FRI_EINVAL else 0     # (too-small strides: the needed paths stride)
        self._check(rc)
        return values, paths, [int(x) for x in ln][:batch]

    def batch_query_phase(self, num_queries: int, max_index: int, channel_states, skip=None, trace_count: int = 0,
                          trace_stride: int = 0, max_layers: Optional[int] = None, indices=None, values=None,
                          paths=None):
        """fri_batch_query_phase: every query of every member of the resident
        batch in one call, the members' channels on the device: per member
        num_queries x (receive_random_int(0, max_index, True), then the
        round's sends).  ``channel_states``: per member the 32 digest bytes
        before the first draw, or None for an empty state.  Returns (indices,
        values, paths, paths_len, states): uint64 (batch, Q), uint32 (batch,
        Q, values_stride) and uint8 (batch, Q, paths_stride) arrays (the
        caller's, when given; the layout verify_batch takes), the bytes of one
        query's paths per member (0: left out, nothing of it written) and the
        members' states after the last send (a member left out keeps what
        came in).  ``max_layers`` sizes the arrays made here (default: log_n +
        1, the most a member can have).  query_phase_messages turns a
        member's rows into its messages."""
        _, members, log_n = self.batch_info()
        batch = len(channel_states)
        if members and batch != members:
            raise FriError(FRI_EINVAL, "one channel state per member of the resident batch")
        q = int(num_queries)
        if q < 0 or max_index < 0 or max_index >> 64 or q >> 32:
            raise FriError(FRI_EINVAL, "num_queries and max_index must be non-negative (32 and 64 bits)")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(np.asarray(skip, dtype=np.uint8))
            if sk.size != batch:
                raise FriError(FRI_EINVAL, "one skip flag per member")
        chs = (ChannelState * max(batch, 1))()
        for b, st in enumerate(channel_states):
            if st:
                if len(st) != 32:
                    raise FriError(FRI_EINVAL, "a channel state is 32 digest bytes or None")
                ctypes.memmove(chs[b].digest, bytes(st), 32)
                chs[b].has_state = 1
        nl = log_n + 1 if max_layers is None else int(max_layers)
        if indices is None:
            indices = np.zeros((batch, q), dtype=np.uint64)
        if values is None:
            values = np.zeros((batch, q, trace_count + 2 * nl), dtype=np.uint32)
        if paths is None:
            paths = np.zeros((batch, q, max(record_paths_len(log_n, trace_count, nl), 1)),
                             dtype=np.uint8)
        if indices.dtype != np.uint64 or values.dtype != np.uint32 or paths.dtype != np.uint8 or \
                indices.shape != (batch, q) or values.ndim != 3 or paths.ndim != 3 or \
                values.shape[:2] != (batch, q) or paths.shape[:2] != (batch, q) or \
                not all(a.flags["C_CONTIGUOUS"] for a in (indices, values, paths)):
            raise FriError(FRI_EINVAL, "indices: C-contiguous uint64 (batch, Q); values: uint32 (batch, Q, stride); "
                                       "paths: uint8 (batch, Q, stride)")
        ln = (ctypes.c_size_t * max(batch, 1))()
        u8p = ctypes.POINTER(ctypes.c_uint8)
        rc = self.lib.fri_batch_query_phase(self.h, q, max_index, chs,
                                            sk.ctypes.data_as(u8p) if sk is not None else None, trace_count,
                                            trace_stride, indices.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                            _ptr(values), values.shape[2], paths.ctypes.data_as(u8p), paths.shape[2],
                                            ln)
        self.round_needed = int(ln[0]) if rc == FRI_EINVAL else 0     # (too-small strides: the needed paths stride)
        self._check(rc)
        states = [bytes(chs[b].digest) if chs[b].has_state else None for b in range(batch)]
        return indices, values, paths, [int(x) for x in ln][:batch] if q else [0] * batch, states

    def set_query_chunk(self, members: int):
        """fri_debug_set_query_chunk: members per staging chunk of later
        batch_query_round and batch_query_phase calls (0: chosen by the
        staging budget)."""
        self._check(self.lib.fri_debug_set_query_chunk(self.h, members))

    def grind(self, state: Optional[bytes], bits: int, first: int = 0, last: int = 2 ** 64 - 1):
        """fri_grind: the smallest nonce in [first, last] whose 8-byte send
        leaves the channel with ``bits`` leading zero bits.  ``state``: the
        32 digest bytes of the channel before the send, or None for an empty
        state.  Returns (nonce, state after the send), or None when the range
        holds no such nonce."""
        if bits < 0 or first < 0 or last < 0 or bits >> 32 or first >> 64 or last >> 64:
            raise FriError(FRI_EINVAL, "bits, first and last must be non-negative (32 and 64 bits)")
        cin, cout = ChannelState(), ChannelState()
        if state:
            if len(state) != 32:
                raise FriError(FRI_EINVAL, "a channel state is 32 digest bytes or None")
            ctypes.memmove(cin.digest, bytes(state), 32)
            cin.has_state = 1
        nonce, found = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._check(self.lib.fri_grind(self.h, ctypes.byref(cin), bits, first, last, ctypes.byref(nonce),
                                       ctypes.byref(found), ctypes.byref(cout)))
        return (int(nonce.value), bytes(cout.digest)) if found.value else None

    def grind_batch(self, states, bits: int, last: int = 2 ** 64 - 1):
        """fri_grind_batch: Context.grind from 0 for every member of
        ``states`` (32 digest bytes, or None for an empty state) in shared
        launches.  Returns one (nonce, state after the send) or None per
        member."""
        batch = len(states)
        if bits < 0 or last < 0 or bits >> 32 or last >> 64:
            raise FriError(FRI_EINVAL, "bits and last must be non-negative (32 and 64 bits)")
        chs = (ChannelState * max(batch, 1))()
        for b, st in enumerate(states):
            if st:
                if len(st) != 32:
                    raise FriError(FRI_EINVAL, "a channel state is 32 digest bytes or None")
                ctypes.memmove(chs[b].digest, bytes(st), 32)
                chs[b].has_state = 1
        nonces = (ctypes.c_uint64 * max(batch, 1))()
        found = (ctypes.c_uint32 * max(batch, 1))()
        self._check(self.lib.fri_grind_batch(self.h, batch, chs, bits, last, nonces, found))
        return [(int(nonces[b]), bytes(chs[b].digest)) if found[b] else None for b in range(batch)]

    def set_grind_window(self, log_window: int):
        """fri_debug_set_grind_window: log2 of the nonces per launch of later
        grind / grind_batch calls (1..32; 0: chosen from ``bits``)."""
        self._check(self.lib.fri_debug_set_grind_window(self.h, log_window))

    def verify_batch(self, shape: "VerifyShape", batch: int, chan, n_layers, a_last, head, head_stride: int,
                     indices, values, values_stride: int, paths, paths_stride: int, verdict=None,
                     grinding_bits: int = 0, nonces=None) -> np.ndarray:
        """fri_verify_batch over the raw ABI: ``shape`` a VerifyShape, ``chan``
        a (batch, 36) uint8 array of fri_channel_state records, the other
        arrays as fri_amd.h lays them out (``PackedTranscripts.abi_args()``
        gives them all).  Returns the verdict masks, a uint32 array (the
        caller's ``verdict`` when given): 0 = accepted, else VERIFY_* bits.
        ``grinding_bits`` > 0: fri_verify_batch_pow with ``nonces``, a
        (batch,) uint64 array of the members' grinding nonces."""
        if verdict is None:
            verdict = np.zeros(max(batch, 1), dtype=np.uint32)
        u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
        args = (self.h, ctypes.byref(shape), batch,
                chan.ctypes.data_as(ctypes.POINTER(ChannelState)), _ptr(n_layers),
                _ptr(a_last) if a_last is not None else None, _ptr(head), head_stride,
                indices.ctypes.data_as(u64p), _ptr(values), values_stride,
                paths.ctypes.data_as(u8p), paths_stride)
        if grinding_bits:
            if grinding_bits < 0:
                raise FriError(FRI_EINVAL, "grinding_bits must be 0..32")
            if nonces is not None:
                nonces = np.ascontiguousarray(nonces, dtype=np.uint64)
            rc = self.lib.fri_verify_batch_pow(*args, grinding_bits,
                                               nonces.ctypes.data_as(u64p) if nonces is not None else None,
                                               _ptr(verdict))
        else:
            rc = self.lib.fri_verify_batch(*args, _ptr(verdict))
        self._check(rc)
        return verdict[:batch]

    def set_verify_chunk(self, members: int):
        """fri_debug_set_verify_chunk: members per upload and launch pair of
        later verify_batch calls (0: chosen by the staging budget)."""
        self._check(self.lib.fri_debug_set_verify_chunk(self.h, members))

    def commit_info(self):
        """(generation, log_n, n_layers) of the resident commit (fri_commit_info)."""
        g, ln, nl = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.fri_commit_info(self.h, ctypes.byref(g), ctypes.byref(ln), ctypes.byref(nl)))
        return g.value, ln.value, nl.value

    def _resident(self, log_n: int, generation: Optional[int] = None) -> None:
        g, ln, nl = self.commit_info()
        _check_resident(generation, log_n, g, ln, nl, "commit")

    def layer(self, k: int, log_n: int, generation: Optional[int] = None) -> np.ndarray:
        self._resident(log_n, generation)
        out = np.empty(1 << (log_n - k), dtype=np.uint32)
        self._check(self.lib.fri_layer_copy(self.h, k, _ptr(out), out.size))
        return out

    def tree_level(self, k: int, level: int, log_n: int) -> List[bytes]:
        self._resident(log_n)
        cnt = 1 << (log_n - k - level)
        buf = ctypes.create_string_buffer(32 * cnt)
        self._check(self.lib.fri_tree_level_copy(self.h, k, level, buf, 32 * cnt))
        return _digests(buf.raw)

    def auth_path(self, k: int, index: int, log_n: int):
        self._resident(log_n)
        depth = log_n - k
        buf = ctypes.create_string_buffer(32 * max(depth, 1))
        val = ctypes.c_uint32()
        dep = ctypes.c_uint32()
        self._check(self.lib.fri_auth_path(self.h, k, index, ctypes.byref(val), buf, ctypes.byref(dep)))
        return val.value, _digests(buf.raw[:32 * dep.value])

    def trace_commit(self, trace, log_blowup: int, offset: int = GENERATOR, readback: bool = True):
        """fri_trace_commit: (LDE Merkle root bytes, trimmed trace-polynomial
        coefficients, LDE values) for 2^log_t trace values (coefficients and
        LDE are None with readback=False: they stay on the device)."""
        tr = _u32(trace)
        log_t = tr.size.bit_length() - 1
        if tr.size != 1 << log_t:
            raise FriError(FRI_EINVAL, "trace length must be a power of two")
        root = ctypes.create_string_buffer(32)
        if not readback:
            self._check(self.lib.fri_trace_commit(self.h, _ptr(tr), log_t, log_blowup, offset, root, None, None,
                                                  None))
            return root.raw, None, None
        coeffs = np.empty(tr.size, dtype=np.uint32)
        lde = np.empty(tr.size << log_blowup, dtype=np.uint32)
        ln = ctypes.c_size_t()
        self._check(self.lib.fri_trace_commit(self.h, _ptr(tr), log_t, log_blowup, offset, root, _ptr(coeffs),
                                              ctypes.byref(ln), _ptr(lde)))
        return root.raw, coeffs[: ln.value], lde

    def fibsq_composition_commit(self, log_t: int, log_blowup: int, a_last: int, alphas: Sequence[int],
                                 offset: int = GENERATOR, channel_state: Optional[bytes] = None,
                                 graph: bool = True) -> CommitResult:
        """fri_fibsq_composition_commit: composition polynomial of the resident
        trace LDE, then the FRI commit of it (channel continued from
        ``channel_state``)."""
        al = _u32(alphas)
        if al.size != 3:
            raise FriError(FRI_EINVAL, "three alphas")
        ch = ChannelState()
        if channel_state:
            ctypes.memmove(ch.digest, channel_state, 32)
            ch.has_state = 1
        res = CommitResult()
        self._check(self.lib.fri_fibsq_composition_commit(self.h, log_t, log_blowup, offset, a_last, _ptr(al),
                                                          ctypes.byref(ch), 0 if graph else FLAG_NO_GRAPH,
                                                          ctypes.byref(res)))
        return res

    def trace_decommit(self, index: int, stride: int, count: int, depth: int):
        """fri_trace_decommit: [(LDE[index + j*stride], path bytes)] for j < count."""
        vals = np.empty(count, dtype=np.uint32)
        buf = ctypes.create_string_buffer(32 * depth * count)
        self._check(self.lib.fri_trace_decommit(self.h, index, stride, count, _ptr(vals), buf, len(buf)))
        pl = 32 * depth
        return [(int(vals[j]), buf.raw[j * pl:(j + 1) * pl]) for j in range(count)]

    def decommit_query(self, index: int, n_layers: int, log_n: int, generation: Optional[int] = None,
                       sharded: bool = False):
        """fri_decommit_query: per committed layer k, (value[idx], value[sib],
        path(idx), path(sib)) with idx = index % m_k, sib = (idx + m_k/2) % m_k.
        sharded: after commit_sharded, fri_decommit_query_sharded (collective:
        every rank calls it with the same index)."""
        self._resident(log_n, generation)
        if n_layers != self.commit_info()[2]:
            raise FriError(FRI_ESTATE, "layer count differs from the resident commit")
        vals = np.empty(2 * n_layers, dtype=np.uint32)
        total = record_paths_len(log_n, 0, n_layers)
        buf = ctypes.create_string_buffer(max(total, 1))
        ln = ctypes.c_size_t()
        fn = self.lib.fri_decommit_query_sharded if sharded else self.lib.fri_decommit_query
        self._check(fn(self.h, index, _ptr(vals), vals.size, buf, total, ctypes.byref(ln)))
        return _openings(vals, buf.raw, n_layers, log_n)

    # ---- multi-GPU ---------------------------------------------------------
    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = load_library().fri_dist_unique_id(buf)
        if rc != FRI_OK:
            raise FriError(rc, "ncclGetUniqueId failed")
        return buf.raw

    def attach_rccl(self, rank: int, world: int, uid: bytes):
        self._check(self.lib.fri_dist_attach_rccl(self.h, rank, world, uid))

    def attach_torch(self, rank: int, world: int):
        """Host-staged collectives over the default torch.distributed group
        (gloo on CPU tensors): used to run the sharded path with several
        ranks on one GPU (tests)."""
        import torch
        import torch.distributed as dist

        def as_np(ptr, nbytes):
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))

        def allgather(user, send, recv, b):
            try:
                src = torch.from_numpy(as_np(send, b).copy())
                outs = [torch.empty(b, dtype=torch.uint8) for _ in range(world)]
                dist.all_gather(outs, src)
                dst = as_np(recv, b * world)
                for r in range(world):
                    dst[r * b:(r + 1) * b] = outs[r].numpy()
                return 0
            except Exception:  # noqa: BLE001
                return 1

        def alltoall(user, send, recv, b):
            try:
                src = torch.from_numpy(as_np(send, b * world).copy())
                out = torch.empty(b * world, dtype=torch.uint8)
                dist.all_to_all_single(out, src)
                as_np(recv, b * world)[:] = out.numpy()
                return 0
            except Exception:  # noqa: BLE001
                return 1

        def sendrecv(user, send, recv, b, peer):
            try:
                src = torch.from_numpy(as_np(send, b).copy())
                out = torch.empty(b, dtype=torch.uint8)
                ops = [dist.P2POp(dist.isend, src, peer), dist.P2POp(dist.irecv, out, peer)]
                for r in dist.batch_isend_irecv(ops):
                    r.wait()
                as_np(recv, b)[:] = out.numpy()
                return 0
            except Exception:  # noqa: BLE001
                return 1

        t = Collectives._fields_
        self._cb = Collectives(None, t[1][1](allgather), t[2][1](alltoall), t[3][1](sendrecv))
        self._check(self.lib.fri_dist_attach_host(self.h, rank, world, ctypes.byref(self._cb)))

    def attach_loopback(self, rank: int, world: int):
        """Timing rehearsal (fri_debug_attach_loopback): collectives return
        this rank's own bytes; the transcript is not the real one."""
        self._check(self.lib.fri_debug_attach_loopback(self.h, rank, world))

    def loopback_degrees(self, degrees: Optional[Sequence[int]]):
        """The rehearsal's degree schedule (fri_debug_loopback_degrees): the
        per-layer degrees of a 1-GPU commit of the same polynomial
        (commit_degrees), so the rehearsal runs every round of the real
        commit although the coefficient fold is sharded. None clears it."""
        if not degrees:
            self._check(self.lib.fri_debug_loopback_degrees(self.h, None, 0))
            return
        a = (ctypes.c_int32 * len(degrees))(*[int(x) for x in degrees])
        self._check(self.lib.fri_debug_loopback_degrees(self.h, a, len(degrees)))

    def commit_degrees(self) -> List[int]:
        """deg(poly_k) of every layer of the resident commit (fri_commit_degrees)."""
        n = ctypes.c_uint32()
        buf = (ctypes.c_int32 * (MAX_ROUNDS + 1))()
        self._check(self.lib.fri_commit_degrees(self.h, buf, MAX_ROUNDS + 1, ctypes.byref(n)))
        return [int(buf[i]) for i in range(n.value)]

    def transport_log(self) -> List[tuple]:
        """(chan, op, peer, bytes) of every collective of the last sharded call
        (fri_debug_transport_log); op is "allgather", "alltoall" or "sendrecv"."""
        cnt = ctypes.c_size_t()
        self._check(self.lib.fri_debug_transport_log(self.h, None, 0, ctypes.byref(cnt)))
        buf = (TransportOp * max(1, cnt.value))()
        self._check(self.lib.fri_debug_transport_log(self.h, buf, cnt.value, ctypes.byref(cnt)))
        return [(e.chan, TRANSPORT_OPS[e.op], e.peer, e.bytes) for e in buf[:cnt.value]]

    def detach(self):
        self._check(self.lib.fri_dist_detach(self.h))

    def dist_info(self):
        """(rank, world, transport) as the attached transport reports them
        (transport: "none", "rccl", "host", "loopback" or "peer"; fri_dist_info)."""
        r, w, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.fri_dist_info(self.h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(t)))
        return r.value, w.value, TRANSPORTS[t.value]

    def dist_selftest(self, words_per_peer: int = 4096):
        self._check(self.lib.fri_dist_selftest(self.h, words_per_peer))

    def commit_sharded(self, coeffs, log_n: int, offset: int = GENERATOR, channel_state: Optional[bytes] = None,
                       forced_betas: Optional[Sequence[int]] = None) -> CommitResult:
        c = _u32(coeffs)
        ch = ChannelState()
        if channel_state:
            ctypes.memmove(ch.digest, channel_state, 32)
            ch.has_state = 1
        flags, fb = 0, None
        if forced_betas is not None:
            fb = np.zeros(MAX_ROUNDS, dtype=np.uint32)
            fb[: len(forced_betas)] = forced_betas
            flags |= FLAG_FORCE_BETAS
        res = CommitResult()
        self._check(self.lib.fri_commit_sharded(self.h, _ptr(c), c.size, log_n, offset, ctypes.byref(ch), flags,
                                                _ptr(fb) if fb is not None else None, ctypes.byref(res)))
        return res

    def set_profiling(self, on: bool):
        self._check(self.lib.fri_set_profiling(self.h, 1 if on else 0))

    def profile(self, cls: str):
        ms, n, b = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.fri_get_profile(self.h, cls.encode(), ctypes.byref(ms), ctypes.byref(n),
                                             ctypes.byref(b)))
        return ms.value, n.value, b.value

    def reset_profile(self):
        self._check(self.lib.fri_reset_profile(self.h))

    def set_device_cap(self, cap_bytes: int):
        """Test hook (fri_debug_set_device_cap): device allocations of this
        context beyond cap_bytes fail as out-of-memory; 0 removes the cap."""
        self._check(self.lib.fri_debug_set_device_cap(self.h, cap_bytes))

    def device_bytes(self):
        """(current, peak) HBM bytes held by this context (fri_ctx_device_bytes)."""
        cur, peak = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.fri_ctx_device_bytes(self.h, ctypes.byref(cur), ctypes.byref(peak)))
        return cur.value, peak.value


_HIP = None


def hip_runtime() -> ctypes.CDLL:
    """The HIP runtime libfri_amd.so is linked against (loaded with it): for
    a caller's own device buffers without a second runtime in the process
    (PyTorch bundles its own libamdhip64)."""
    global _HIP
    if _HIP is not None:
        return _HIP
    load_library()
    path = "libamdhip64.so.7"
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line and "/torch/" not in line:
                    path = line.split()[-1]
                    break
    except OSError:
        pass
    hip = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    _HIP = hip
    return hip


class DeviceBuffer:
    """A device copy of a uint32 array for fri_commit_device /
    fri_commit_device_async (hipMalloc, then an upload on a stream of its own,
    so the null stream never takes one of the process's hardware queues);
    freed with the object.  ``data_ptr()`` is the device pointer."""

    def __init__(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        hip = hip_runtime()
        self._hip = hip
        p = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(4, a.nbytes))) != 0:
            raise FriError(FRI_ENOMEM, "hipMalloc of a device buffer failed")
        self.ptr = p.value
        st = ctypes.c_void_p()
        if (hip.hipStreamCreate(ctypes.byref(st)) != 0 or
                hip.hipMemcpyAsync(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1, st) != 0 or
                hip.hipStreamSynchronize(st) != 0):
            raise FriError(FRI_EHIP, "upload of a device buffer failed")
        hip.hipStreamDestroy(st)

    def data_ptr(self) -> int:
        return self.ptr

    def __del__(self):
        if getattr(self, "ptr", None):
            self._hip.hipFree(self.ptr)
            self.ptr = None


def plan_layout(d: int, log_n: int, world: int = 1, rank: int = 0) -> dict:
    """The commit plan's layout (fri_debug_plan_layout; host only, no GPU):
    rounds bound, last sharded layer, per-layer slot sizes, x^-1 slices and
    the block the rank holds."""
    cap = 4 + 5 * (MAX_ROUNDS + 1)
    out = (ctypes.c_uint64 * cap)()
    rc = load_library().fri_debug_plan_layout(d, log_n, world, rank, out, cap)
    if rc != FRI_OK:
        raise FriError(rc, "fri_debug_plan_layout")
    rmax = int(out[0])
    layers = [dict(zip(("layer_words", "tree_words", "xinv_count", "xinv_start", "block"),
                       (int(x) for x in out[4 + 5 * k: 9 + 5 * k]))) for k in range(rmax + 1)]
    k_sw = int(out[1])
    return {"rmax": rmax, "k_sw": k_sw - (1 << 64) if k_sw >= 1 << 63 else k_sw, "bytes": int(out[2]),
            "coef_chunk_log2": int(out[3]), "layers": layers}


# ----------------------------------------------------------------------------
# Reference-shaped host objects
# ----------------------------------------------------------------------------
def state_has_zero_bits(state: str, bits: int) -> bool:
    """The grinding check: the ``bits`` most significant bits of a channel
    state (64 hex characters) are zero."""
    return len(state) == 64 and int(state, 16) >> (256 - bits) == 0


@dataclass
class Channel:
    """src/channel/channel.rs — host-side transcript (authoritative state).

    fri_commit() hands the state to the device, which replays the exact same
    send/receive sequence, and then appends the same proof messages here."""
    state: str = ""
    proof: List[bytes] = field(default_factory=list)
    compressed_proof: List[bytes] = field(default_factory=list)

    def send(self, message: bytes) -> None:                               # channel.rs:35-44
        self.state = hashlib.sha256((self.state + bytes(message).hex()).encode()).hexdigest()
        self.proof.append(bytes(message))
        self.compressed_proof.append(bytes(message))

    def receive_random_int(self, lo: int, hi: int, show_in_proof: bool) -> int:   # channel.rs:58-84
        if not self.state:
            raise FriError(FRI_ESTATE, "Channel state is not valid hex")   # channel.rs:65
        num = (int(self.state, 16) + lo) % ((hi - lo) + 1)
        self.state = hashlib.sha256(self.state.encode()).hexdigest()
        num &= (1 << 64) - 1
        if show_in_proof:
            self.proof.append(num.to_bytes(8, "big"))
        return num

    def receive_random_field_element(self) -> int:                        # channel.rs:47-55
        num = self.receive_random_int(0, P - 1, False)
        self.proof.append(num.to_bytes(8, "big"))
        return num % P

    def take_over_queries(self, messages: Sequence[bytes], num_queries: int, state: str) -> None:
        """The query phase as the device ran it (fri_batch_query_phase), taken
        over without hashing: ``messages`` are query_phase_messages' --
        num_queries runs of equal length, each a drawn index (be64) and its
        openings -- and ``state`` the channel after the last send.  Leaves in
        ``proof`` and ``compressed_proof`` what receive_random_int(.., True)
        and send leave there: an index in ``proof`` alone."""
        if num_queries == 0:
            if messages:
                raise FriError(FRI_EINVAL, "messages without a query")
            return
        per, rest = divmod(len(messages), num_queries)
        if rest or per < 1 or len(state) != 64:
            raise FriError(FRI_EINVAL, "num_queries runs of an index and its openings, and a 64-character state")
        for i, m in enumerate(messages):
            self.proof.append(bytes(m))
            if i % per:
                self.compressed_proof.append(bytes(m))
        self.state = state

    def grind(self, bits: int, ctx: Optional["Context"] = None, first: int = 0) -> int:
        """Proof of work before the query phase (fri_amd.h, fri_grind): finds
        the smallest nonce >= ``first`` whose send leaves the state with
        ``bits`` leading zero bits (0..32), sends it as an 8-byte message and
        returns it.  Without ``ctx`` the search is a host loop (hashlib), with
        one it runs on the device; the send and the check of the new state are
        the host's either way.  FriError when no nonce up to 2^64 - 1 does."""
        if not 0 <= bits <= GRIND_MAX_BITS or not 0 <= first < 1 << 64:
            raise FriError(FRI_EINVAL, "bits must be 0..32 and first below 2^64")
        nonce = None
        if ctx is None:
            head = hashlib.sha256(self.state.encode())
            for v in range(first, 1 << 64):
                h = head.copy()
                h.update(b"%016x" % v)
                if int.from_bytes(h.digest()[:4], "big") >> (32 - bits) == 0:
                    nonce = v
                    break
        else:
            got = ctx.grind(bytes.fromhex(self.state) if self.state else None, bits, first)
            nonce = got[0] if got else None
        if nonce is None:
            raise FriError(FRI_ESTATE, "no nonce in range gives the state the zero bits")
        self.send(nonce.to_bytes(8, "big"))
        if not state_has_zero_bits(self.state, bits):
            raise FriError(FRI_ESTATE, "the state after the nonce lacks the zero bits")
        return nonce

    def proof_size(self) -> int:                                         # channel.rs:88-90
        return sum(len(b) for b in self.proof)

    def compressed_proof_size(self) -> int:                               # channel.rs:93-95
        return sum(len(b) for b in self.compressed_proof)


class MerkleTree:
    """src/merkle/mod.rs:5-27 — SHA-256 tree over u64-BE leaves (GPU-built).
    A standalone tree keeps its root; the trees of an FRIProof
    (``FRIProof.fri_merkles``) are the device-resident ones of that commit
    and also serve authentication paths."""

    def __init__(self, values: Sequence[int], ctx: Optional[Context] = None):
        self._ctx = ctx or _default_ctx(max(1, (len(values) - 1).bit_length()))
        self._root = self._ctx.merkle_root(values)
        self._generation = None
        self._layer = None
        self._log_n = None
        self._sharded = False

    @classmethod
    def _on_device(cls, ctx: Context, generation: int, layer: int, log_n: int, root: bytes,
                   sharded: bool = False) -> "MerkleTree":
        t = cls.__new__(cls)
        t._ctx, t._root, t._generation, t._layer, t._log_n = ctx, root, generation, layer, log_n
        t._sharded = sharded
        return t

    def root(self) -> str:
        return self._root.hex()

    def get_authentication_path(self, idx: int) -> bytes:
        """rs_merkle single-leaf proof of leaf idx (sibling digests leaf ->
        root) from the device-resident tree (fri_auth_path)."""
        if self._generation is None:
            raise FriError(FRI_ESTATE, "a standalone tree keeps only its root")
        self._ctx._resident(self._log_n, self._generation)
        _, path = self._ctx.auth_path(self._layer, idx, self._log_n)
        return b"".join(path)


class BatchMember:
    """One member of a context's resident batch (fri_commit_batch) behind the
    read-back interface of a Context: what FRIProof, MerkleTree and the
    decommitment functions call (layer, tree_level, auth_path, decommit_query,
    commit_info, commit_degrees), served by the fri_batch_* read-backs."""

    def __init__(self, ctx: Context, member: int):
        self.ctx, self.member = ctx, member

    def commit_info(self):
        g, b, ln = self.ctx.batch_info()
        return g, (ln if b else 0), (len(self.commit_degrees()) if b else 0)

    def _resident(self, log_n: int, generation: Optional[int] = None) -> None:
        g, b, ln = self.ctx.batch_info()
        _check_resident(generation, log_n, g, ln, b, "batch")

    def commit_degrees(self) -> List[int]:
        return self.ctx.batch_commit_degrees(self.member)

    def layer(self, k: int, log_n: int, generation: Optional[int] = None) -> np.ndarray:
        self._resident(log_n, generation)
        return self.ctx.batch_layer(self.member, k, log_n)

    def tree_level(self, k: int, level: int, log_n: int) -> List[bytes]:
        self._resident(log_n)
        return self.ctx.batch_tree_level(self.member, k, level, log_n)

    def decommit_query(self, index: int, n_layers: int, log_n: int, generation: Optional[int] = None,
                       sharded: bool = False):
        self._resident(log_n, generation)
        if n_layers != len(self.commit_degrees()):
            raise FriError(FRI_ESTATE, "layer count differs from the resident member's")
        return self.ctx.batch_decommit_query(self.member, index, n_layers, log_n)

    def auth_path(self, k: int, index: int, log_n: int):
        # the opening of `index` in layer k is at idx_k = index mod 2^(log_n - k) = index
        self._resident(log_n)
        if not 0 <= index < (1 << (log_n - k)):
            raise FriError(FRI_EINVAL, "index out of range")
        val, _, path, _ = self.ctx.batch_decommit_query(self.member, index, len(self.commit_degrees()), log_n)[k]
        return val, _digests(path)


@dataclass
class FRIProof:
    """src/fri/fri_commit.rs:9-13 — layers/merkles read back lazily from the device."""
    ctx: Context             # (a BatchMember for a proof made by fri_commit_batch)
    log_n: int
    roots: List[bytes]
    betas: List[int]
    final_value: int
    final_degree: int
    generation: int = 0      # fri_commit_info generation of the commit that made it
    sharded: bool = False    # made by fri_commit_sharded: decommitments are collective
    member: Optional[int] = None   # made by fri_commit_batch: its member of that batch

    @property
    def n_layers(self) -> int:
        return len(self.roots)

    def layer(self, k: int) -> np.ndarray:
        return self.ctx.layer(k, self.log_n, self.generation)

    @property
    def fri_layers(self) -> List[np.ndarray]:
        return [self.layer(k) for k in range(self.n_layers)]

    def merkle_root(self, k: int) -> str:
        return self.roots[k].hex()

    @property
    def fri_merkles(self) -> List[MerkleTree]:
        """FRIProof.fri_merkles (fri_commit.rs:9-13): the commit's trees, device-backed."""
        return [MerkleTree._on_device(self.ctx, self.generation, k, self.log_n, r, self.sharded)
                for k, r in enumerate(self.roots)]

    @property
    def final_poly(self) -> List[int]:
        return [] if self.final_degree == -1 else [self.final_value]


def decommit_fri_layers(index: int, proof: "FRIProof", channel: Channel) -> None:
    """src/fri/fri_commit.rs:137-163 over the device-resident layers/trees:
    per layer send value, path, sibling value, sibling path (a 1-element
    layer first sends its value, as the reference does)."""
    _send_openings(proof.ctx.decommit_query(index, proof.n_layers, proof.log_n, proof.generation, proof.sharded),
                   channel)


def _send_openings(openings, channel: Channel) -> None:
    for val, sval, path, spath in openings:
        # the gather reads layers of 2^(log_n-k) >= 2 elements; a 1-element
        # layer (blowup 1) has idx = sib = 0 and empty paths
        if not path and not spath:
            channel.send(val.to_bytes(8, "big"))
        channel.send(val.to_bytes(8, "big"))
        channel.send(path)
        channel.send(sval.to_bytes(8, "big"))
        channel.send(spath)


def _check_grinding_bits(bits: int) -> None:
    if not 0 <= bits <= GRIND_MAX_BITS:
        raise FriError(FRI_EINVAL, "grinding_bits must be 0..32")


def _grind(channel: Channel, bits: int, ctx: "Context") -> None:
    """A prover's grinding step: nothing for 0 bits, else Channel.grind, on
    the host below GRIND_DEVICE_MIN_BITS and on ``ctx`` from it up."""
    _check_grinding_bits(bits)
    if bits:
        channel.grind(bits, ctx if bits >= GRIND_DEVICE_MIN_BITS else None)


def _grind_batch(channels: Sequence[Channel], bits: int, ctx: "Context") -> None:
    """_grind for every member's channel; on the device it is ONE
    fri_grind_batch on the members' states, and every channel then sends its
    nonce and must arrive at the state the device returned."""
    _check_grinding_bits(bits)
    if not bits:
        return
    if bits < GRIND_DEVICE_MIN_BITS:
        for ch in channels:
            ch.grind(bits)
        return
    got = ctx.grind_batch([bytes.fromhex(ch.state) if ch.state else None for ch in channels], bits)
    for b, (ch, g) in enumerate(zip(channels, got)):
        if g is None:
            raise FriError(FRI_ESTATE, f"member {b}: no nonce in range gives the state the zero bits")
        ch.send(g[0].to_bytes(8, "big"))
        if ch.state != g[1].hex() or not state_has_zero_bits(ch.state, bits):
            raise FriError(FRI_ESTATE, f"member {b}: the state after the nonce is not the device's")


def decommit_fri(num_queries: int, max_index: int, proof, merkles_or_channel, channel: Optional[Channel] = None,
                 grinding_bits: int = 0) -> None:
    """src/fri/fri_commit.rs:168-179: each index drawn with
    receive_random_int(0, max_index, true) from the transcript so far.
    Two forms: decommit_fri(q, max, proof, channel), or the reference's own
    decommit_fri(q, max, fri_layers, fri_merkles, channel) with the proof's
    ``fri_layers`` and device-backed ``fri_merkles`` (the commit is found
    through the trees; their generation must still be resident, and the
    openings must equal ``fri_layers``).  ``grinding_bits`` > 0: the channel
    first grinds that many bits (Channel.grind; fri_amd.h, fri_grind)."""
    if channel is None:
        _grind(merkles_or_channel, grinding_bits, proof.ctx.ctx if isinstance(proof.ctx, BatchMember) else proof.ctx)
        for _ in range(num_queries):
            idx = merkles_or_channel.receive_random_int(0, max_index, True)
            decommit_fri_layers(idx, proof, merkles_or_channel)
        return
    layers, merkles = proof, merkles_or_channel
    if not merkles or len(layers) != len(merkles):
        raise FriError(FRI_EINVAL, "one Merkle tree per FRI layer")
    t0 = merkles[0]
    if t0._generation is None or any(t._ctx is not t0._ctx or t._generation != t0._generation or t._layer != k
                                     for k, t in enumerate(merkles)):
        raise FriError(FRI_EINVAL, "fri_merkles are not the device-backed trees of one commit")
    ctx, log_n = t0._ctx, t0._log_n
    _grind(channel, grinding_bits, ctx.ctx if isinstance(ctx, BatchMember) else ctx)
    for _ in range(num_queries):
        idx = channel.receive_random_int(0, max_index, True)
        openings = ctx.decommit_query(idx, len(merkles), log_n, t0._generation, t0._sharded)
        for k, (v, sv, _, _) in enumerate(openings):
            m = 1 << (log_n - k)
            i = idx % m
            if len(layers[k]) != m or int(layers[k][i]) != v or int(layers[k][(i + m // 2) % m]) != sv:
                raise FriError(FRI_ESTATE, f"fri_layers do not belong to the commit of these fri_merkles (layer {k})")
        _send_openings(openings, channel)


def _merkle_path_ok(value: int, index: int, path: bytes, depth: int, root: bytes) -> bool:
    """rs_merkle single-leaf proof of a power-of-two tree: siblings leaf -> root."""
    if len(path) != 32 * depth:
        return False
    h = hashlib.sha256(value.to_bytes(8, "big")).digest()              # merkle/mod.rs:14-15
    for lvl in range(depth):
        sib = path[32 * lvl:32 * lvl + 32]
        h = hashlib.sha256(sib + h if (index >> lvl) & 1 else h + sib).digest()
    return h == root


def verify_fri(messages: Sequence[bytes], log_n: int, n_layers: int, num_queries: int, max_index: int,
               offset: int = GENERATOR, channel_state: str = "", grinding_bits: int = 0) -> bool:
    """Check a FRI transcript: the proof messages that fri_commit followed by
    decommit_fri append to Channel.proof (fri_commit.rs:72-179).

    The reference's verify_fri (src/fri/fri_verify.rs:12-177) is a sketch.
    It re-reads proof.last() and leaves the fold check as a placeholder, so
    this is the check it outlines, made complete:
      * replay a fresh channel from ``channel_state``: every root is sent;
        every beta and query index must be the one the replay draws; the
        final value is sent;
      * every authentication path must lead to its layer's root;
      * every layer k >= 1 value must equal the fold of its two parents:
        (a + b)/2 + beta (a - b) / (2 x);
      * the last layer must hold the final constant.
    ``n_layers`` = number of committed layers (the reference's
    expected_num_layers). Returns False on any mismatch or malformed transcript.
    ``grinding_bits`` > 0: an 8-byte nonce must follow the final value, and
    the state after its send must have that many leading zero bits (the
    nonce need not be the smallest).
    """
    return _verify_transcript(messages, log_n, n_layers, num_queries, max_index, offset, channel_state,
                              grinding_bits=grinding_bits)


class _Reject(Exception):
    pass


def _verify_transcript(messages, log_n, n_layers, num_queries, max_index, offset, channel_state,
                       pre_commit=None, on_query=None, grinding_bits=0) -> bool:
    """verify_fri's replay with two hooks for a STARK around the FRI:
    ``pre_commit(take, ch)`` consumes the messages before the first FRI root;
    ``on_query(take, ch, idx)`` those between a query index and its layer
    openings, and returns the value layer 0 must hold at idx (or None)."""
    _check_grinding_bits(grinding_bits)
    msgs = list(messages)
    pos = 0

    def take():
        nonlocal pos
        if pos >= len(msgs):
            raise ValueError("transcript ended early")
        pos += 1
        return msgs[pos - 1]

    try:
        ch = Channel(state=channel_state)
        if pre_commit is not None:
            pre_commit(take, ch)
        roots, betas = [], []
        for k in range(n_layers):
            r = take()
            if len(r) != 64:
                return False
            roots.append(bytes.fromhex(r.decode()))
            ch.send(r)
            if k < n_layers - 1:
                beta = ch.receive_random_field_element()
                if take() != beta.to_bytes(8, "big"):
                    return False
                betas.append(beta)
        fin = take()
        if len(fin) != 8:
            return False
        final = int.from_bytes(fin, "big")
        ch.send(fin)
        if grinding_bits:
            nonce = take()
            if len(nonce) != 8:
                return False
            ch.send(nonce)
            if not state_has_zero_bits(ch.state, grinding_bits):
                return False
        inv2 = pow(2, P - 2, P)
        for _ in range(num_queries):
            idx = ch.receive_random_int(0, max_index, True)
            if take() != idx.to_bytes(8, "big"):
                return False
            want0 = on_query(take, ch, idx) if on_query is not None else None
            prev = None                                  # (value at i, value at i + m/2, i, m) of layer k-1
            for k in range(n_layers):
                m = 1 << (log_n - k)
                depth = log_n - k
                extra = None
                if m == 1:
                    extra = take()                       # fri_commit.rs:147-149 sends layer[0] first
                    ch.send(extra)
                i = idx % m
                sib = (i + m // 2) % m
                vb, path, sb, spath = take(), take(), take(), take()
                if extra is not None and extra != vb:
                    return False
                for msg in (vb, path, sb, spath):
                    ch.send(msg)
                v, sv = int.from_bytes(vb, "big"), int.from_bytes(sb, "big")
                if v >= P or sv >= P:
                    return False
                if not (_merkle_path_ok(v, i, path, depth, roots[k]) and _merkle_path_ok(sv, sib, spath, depth, roots[k])):
                    return False
                if k == 0 and want0 is not None and v != want0:
                    return False
                if prev is not None:
                    pa, pb, pj, pm = prev                    # pa = L[pj], pb = L[pj + pm/2]
                    x = pow(offset, 1 << (k - 1), P) * pow(pow(GENERATOR, (P - 1) // pm, P), pj, P) % P
                    fold = ((pa + pb) + betas[k - 1] * (pa - pb) % P * pow(x, P - 2, P)) % P * inv2 % P
                    if fold != v:
                        return False
                j = i % (m // 2) if m > 1 else 0
                prev = (v, sv, j, m) if i < m // 2 or m == 1 else (sv, v, j, m)
                if k == n_layers - 1 and (v != final or sv != final):
                    return False
        return pos == len(msgs)
    except (ValueError, IndexError, UnicodeDecodeError, _Reject):
        return False


# ---- prover slice: STARK-101 FibonacciSq (BASELINE configs[3]) -------------
# src/prover, src/trace, src/composition are empty in the reference; the
# constraint system is STARK-101's (crate `stark-101`, Cargo.toml:2) on the
# full trace subgroup; see include/fri_amd.h (fri_fibsq_composition_commit).

def fibsq_trace(a1: int, T: int) -> np.ndarray:
    """a_0 = 1, a_1 = a1, a_{i+2} = a_{i+1}^2 + a_i^2 (mod p), T = 2^k rows
    (fri_fibsq_trace, host-side: the recurrence is one serial chain)."""
    log_t = T.bit_length() - 1
    if T != 1 << log_t:
        raise FriError(FRI_EINVAL, "trace length must be a power of two")
    out = np.empty(T, dtype=np.uint32)
    rc = load_library().fri_fibsq_trace(a1 % P, log_t, _ptr(out))
    if rc != FRI_OK:
        raise FriError(rc, "fri_fibsq_trace")
    return out


@dataclass
class StarkProof:
    trace_root: bytes
    alphas: List[int]
    a_last: int
    fri: FRIProof
    log_t: int
    log_blowup: int
    queries: List[int]


def prove_fibsq(a1: int, log_t: int, log_blowup: int, num_queries: int, channel: Channel,
                offset: int = GENERATOR, ctx: Optional[Context] = None, grinding_bits: int = 0) -> StarkProof:
    """STARK-101 prover on the GPU: trace -> LDE + Merkle (fri_trace_commit),
    send the trace root, draw alpha_0..2, composition polynomial + FRI commit
    (fri_fibsq_composition_commit), then per query (index drawn with
    receive_random_int(0, n - 2B - 1, true)) send f(x), f(gx), f(g^2 x) with
    their paths and the FRI layer openings (decommit_fri_layers,
    fri_commit.rs:137-163).  The transcript is ``channel.proof``.
    ``grinding_bits`` > 0: between the FRI commit's final value and the
    first query index the channel grinds that many bits (Channel.grind)."""
    _check_grinding_bits(grinding_bits)
    L = log_t + log_blowup
    B, n = 1 << log_blowup, 1 << L
    ctx = ctx or _default_ctx(L)
    trace = fibsq_trace(a1, 1 << log_t)
    root, _, _ = ctx.trace_commit(trace, log_blowup, offset, readback=False)
    channel.send(root.hex().encode())
    alphas = [channel.receive_random_field_element() for _ in range(3)]
    res = ctx.fibsq_composition_commit(log_t, log_blowup, int(trace[-1]), alphas, offset,
                                       channel_state=bytes.fromhex(channel.state))
    fri = _mirror_commit(res, ctx, L, channel)
    _grind(channel, grinding_bits, ctx)
    queries = []
    for _ in range(num_queries):
        idx = channel.receive_random_int(0, n - 2 * B - 1, True)
        queries.append(idx)
        for v, path in ctx.trace_decommit(idx, B, 3, L):
            channel.send(v.to_bytes(8, "big"))
            channel.send(path)
        decommit_fri_layers(idx, fri, channel)
    return StarkProof(root, alphas, int(trace[-1]), fri, log_t, log_blowup, queries)


def fibsq_cp_at(f0: int, f1: int, f2: int, x: int, alphas: Sequence[int], a_last: int, log_t: int) -> int:
    """CP(x) from f(x), f(gx), f(g^2 x) (the composition the prover commits)."""
    T = 1 << log_t
    f0, f1, f2, x, a_last = int(f0), int(f1), int(f2), int(x), int(a_last)
    g = pow(GENERATOR, (P - 1) >> log_t, P)
    glast, gprev = pow(g, T - 1, P), pow(g, T - 2, P)
    p0 = (f0 - 1) * pow(x - 1, P - 2, P)
    p1 = (f0 - a_last) * pow(x - glast, P - 2, P)
    p2 = (f2 - f1 * f1 - f0 * f0) * (x - gprev) * (x - glast) * pow(pow(x, T, P) - 1, P - 2, P)
    return (alphas[0] * p0 + alphas[1] * p1 + alphas[2] * p2) % P


def verify_fibsq(messages: Sequence[bytes], a_last: int, log_t: int, log_blowup: int, num_queries: int,
                 n_layers: int, offset: int = GENERATOR, channel_state: str = "", grinding_bits: int = 0) -> bool:
    """Verifier of prove_fibsq's transcript: replays the channel (trace root,
    alphas, FRI roots/betas/final, query indices), checks every trace path
    against the trace root, that layer 0 at each query equals the composition
    polynomial computed from the opened f(x), f(gx), f(g^2 x), and then every
    FRI check of verify_fri, the nonce of ``grinding_bits`` > 0 included."""
    L = log_t + log_blowup
    B, n = 1 << log_blowup, 1 << L
    a_last = int(a_last)
    state = {}

    def pre_commit(take, ch):
        r = take()
        if len(r) != 64:
            raise _Reject()
        state["root"] = bytes.fromhex(r.decode())
        ch.send(r)
        al = []
        for _ in range(3):
            a = ch.receive_random_field_element()
            if take() != a.to_bytes(8, "big"):
                raise _Reject()
            al.append(a)
        state["alphas"] = al

    def on_query(take, ch, idx):
        fs = []
        for j in range(3):
            vb, path = take(), take()
            ch.send(vb)
            ch.send(path)
            v = int.from_bytes(vb, "big")
            if len(vb) != 8 or v >= P or not _merkle_path_ok(v, idx + j * B, path, L, state["root"]):
                raise _Reject()
            fs.append(v)
        x = offset * pow(pow(GENERATOR, (P - 1) >> L, P), idx, P) % P
        return fibsq_cp_at(fs[0], fs[1], fs[2], x, state["alphas"], a_last, log_t)

    return _verify_transcript(messages, L, n_layers, num_queries, n - 2 * B - 1, offset, channel_state,
                              pre_commit, on_query, grinding_bits)


_CTX_CACHE = {}


def _default_ctx(log_n: int) -> Context:
    """The context of the reference-shaped calls without ``ctx``: over the
    default devices (Context.default: FRI_DEVICES, else every visible GPU),
    at least 2^log_n (2^12 minimum), one per size bound, kept."""
    key = max(log_n, 12)
    for k, c in _CTX_CACHE.items():
        if k >= key:
            return c
    c = Context.default(key)
    _CTX_CACHE[key] = c
    return c


# ---- Polynomial arithmetic (src/polynomial/ops.rs) --------------------------
def _trim(a: np.ndarray) -> np.ndarray:                                   # Polynomial::new (ops.rs:19-37)
    nz = np.flatnonzero(a)
    return a[: int(nz[-1]) + 1] if nz.size else a[:0]


def _log_for(n: int) -> int:
    return max(0, int(n - 1).bit_length())


def poly_add(a, b) -> np.ndarray:
    """a + b (Polynomial::add_assign, ops.rs:87-98), on the host, trimmed."""
    x, y = _u32(a).astype(np.uint64), _u32(b).astype(np.uint64)
    out = np.zeros(max(x.size, y.size), dtype=np.uint64)
    out[: x.size] = x
    out[: y.size] += y
    return _trim((out % P).astype(np.uint32))


def poly_sub(a, b) -> np.ndarray:
    """a - b (Polynomial::sub_assign, ops.rs:101-112), on the host, trimmed."""
    x, y = _u32(a).astype(np.uint64), _u32(b).astype(np.uint64)
    out = np.zeros(max(x.size, y.size), dtype=np.uint64)
    out[: x.size] = x
    out[: y.size] += P - y
    return _trim((out % P).astype(np.uint32))


def poly_scalar_mul(a, s: int) -> np.ndarray:
    """Polynomial::scalar_mul (ops.rs:194-198), on the host: like the reference
    it does not re-trim (s = 0 leaves len(a) zeros)."""
    if not 0 <= int(s) < P:
        raise FriError(FRI_EINVAL, "field element not canonical (>= p)")
    return ((_u32(a).astype(np.uint64) * np.uint64(int(s))) % np.uint64(P)).astype(np.uint32)


def poly_mul(a, b, ctx: Optional[Context] = None, force: Optional[str] = None) -> np.ndarray:
    """Polynomial::mul_assign (ops.rs:114-138) on the device."""
    ctx = ctx or _default_ctx(_log_for(len(a) + len(b)))
    return ctx.poly_mul(a, b, force=force)


def poly_div_rem(a, b, ctx: Optional[Context] = None):
    """Polynomial::div_rem (ops.rs:141-191) on the device: (q, r)."""
    ctx = ctx or _default_ctx(_log_for(len(a)) + 2)
    return ctx.poly_div_rem(a, b)


def poly_compose(p, q, ctx: Optional[Context] = None) -> np.ndarray:
    """Polynomial::compose (ops.rs:214-237) on the device: p(q(x))."""
    ctx = ctx or _default_ctx(_log_for(max(1, len(p)) * max(1, len(q))))
    return ctx.poly_compose(p, q)


# ---- src/polynomial/interpolation.rs ----------------------------------------
def gen_polynomial_from_roots(roots, ctx: Optional[Context] = None) -> np.ndarray:
    """gen_polynomial_from_roots (interpolation.rs:9-23) on the device:
    prod (x - r), n + 1 coefficients; the zero polynomial for no roots."""
    ctx = ctx or _default_ctx(_log_for(max(1, len(roots))))
    return ctx.poly_from_roots(roots)


def gen_lagrange_polynomials(xs, ctx: Optional[Context] = None) -> np.ndarray:
    """gen_lagrange_polynomials (interpolation.rs:46-78) on the device: the
    (n, n) array whose row i holds L_i's coefficients, untrimmed."""
    ctx = ctx or _default_ctx(_log_for(max(1, len(xs))))
    return ctx.lagrange_basis(xs)


gen_lagrange_polynomials_parallel = gen_lagrange_polynomials   # interpolation.rs:80-115: the same polynomials


def fri_commit(coeffs: Sequence[int], log_n: int, channel: Channel, offset: int = GENERATOR,
               ctx: Optional[Context] = None) -> FRIProof:
    """src/fri/fri_commit.rs:72-122 on the coset domain offset*<w_{2^log_n}>.

    Updates ``channel`` exactly as the reference does: proof gets
    root_hex bytes per layer, 8-byte BE beta per round, 8-byte BE final value;
    state ends as the device computed it."""
    ctx = ctx or _default_ctx(log_n)
    st = bytes.fromhex(channel.state) if channel.state else None
    res = ctx.commit(coeffs, log_n, offset, channel_state=st)
    return _mirror_commit(res, ctx, log_n, channel)


def fri_commit_pipelined(polys: Sequence[Sequence[int]], log_n: int, channels: Sequence[Channel],
                         offset: int = GENERATOR, ctx=None, depth: int = DEFAULT_LANES) -> List[FRIProof]:
    """fri_commit (fri_commit.rs:72-122) of many polynomials in a row, each
    with its own channel, pipelined from this one host thread
    (fri_commit_async / fri_commit_wait, ``depth`` commits in flight per
    context, each on a commit lane of its own: one context overlaps them).
    ``ctx`` is one Context or a list of them: with several, the commits are
    dealt round-robin and run concurrently, one stream each.
    Proof i equals fri_commit of polys[i] into channels[i]; on each context
    only its last proof's layers stay resident.  Without ``ctx`` the commits
    run on the default context; where that is a team (which takes no
    pipelined commits, fri_commit_async), on a one-device context of their
    own on the team's first device, kept per size bound."""
    if len(polys) != len(channels):
        raise FriError(FRI_EINVAL, "one channel per polynomial")
    if not 1 <= depth <= MAX_INFLIGHT:
        raise FriError(FRI_EINVAL, "depth must be 1..MAX_INFLIGHT")
    ctxs = list(ctx) if isinstance(ctx, (list, tuple)) else [ctx or _beside_team(_default_ctx(log_n), log_n, _PIPE_CTX)]
    if len({id(c) for c in ctxs}) != len(ctxs):
        raise FriError(FRI_EINVAL, "a context appears twice: pass each context once (depth sets the commits in flight)")
    gen = [c.commit_info()[0] for c in ctxs]     # every enqueued commit bumps its context's generation by one
    out: List[Optional[FRIProof]] = [None] * len(polys)
    pend = []

    def collect(i, j, ticket, g):
        out[i] = _mirror_commit(ctxs[j].commit_wait(ticket), ctxs[j], log_n, channels[i], generation=g)

    try:
        for i, (c, ch) in enumerate(zip(polys, channels)):
            j = i % len(ctxs)
            if len(pend) == depth * len(ctxs):
                collect(*pend.pop(0))
            st = bytes.fromhex(ch.state) if ch.state else None
            t = ctxs[j].commit_async(c, log_n, offset, channel_state=st)
            gen[j] += 1
            pend.append((i, j, t, gen[j]))
        while pend:
            collect(*pend.pop(0))
    finally:
        # a commit that failed (e.g. a coefficient >= p, reported at its wait)
        # must not leave the others' result slots pending on the contexts:
        # wait for every remaining ticket, discarding its result
        for _, j, t, _ in pend:
            try:
                ctxs[j].commit_wait(t)
            except FriError:
                pass
    return out


_BATCH_CTX = {}     # fri_commit_batch's one-device contexts beside a default team, by size bound
_PIPE_CTX = {}      # fri_commit_pipelined's


def _beside_team(ctx: Context, log_n: int, cache: dict) -> Context:
    """``ctx`` itself unless it is a team: then the one-device context of
    ``cache`` for 2^log_n (2^12 minimum) on the team's first device, created
    on first use and kept."""
    if ctx.n_ranks == 1:
        return ctx
    key = max(log_n, 12)
    if key not in cache:
        cache[key] = Context(ctx.device, key)
    return cache[key]


def _pack_batch(polys) -> tuple:
    """The members' coefficients as one (batch, d) uint32 array, d the longest
    member's length, shorter members padded with zeros (trailing zero
    coefficients do not change a commit).  Returns (array, d)."""
    rows = [_u32(p).reshape(-1) for p in polys]
    d = max((r.size for r in rows), default=0)
    c = np.zeros((len(rows), d), dtype=np.uint32)
    for b, r in enumerate(rows):
        c[b, : r.size] = r
    return c, d


def fri_commit_batch(polys: Sequence[Sequence[int]], log_n: int, channels: Sequence[Channel],
                     offset: int = GENERATOR, ctx: Optional[Context] = None) -> List[FRIProof]:
    """fri_commit (fri_commit.rs:72-122) of many small polynomials, each with
    its own channel, in ONE device call (fri_commit_batch: one workgroup per
    member; log_n <= BATCH_MAX_LOG_N).  Proof i equals fri_commit of polys[i]
    into channels[i] and remembers its member: its layers, trees and
    decommitments are served until the next commit on the context.  Members
    of different lengths are padded with zeros to the longest."""
    if len(polys) != len(channels):
        raise FriError(FRI_EINVAL, "one channel per polynomial")
    if len(polys) == 0:
        return []
    # batches run on one device: a context of their own beside a (default) team
    ctx = _beside_team(ctx or _default_ctx(log_n), log_n, _BATCH_CTX)
    states = [bytes.fromhex(ch.state) if ch.state else None for ch in channels]
    res = ctx.commit_batch(polys, log_n, offset, channel_states=states)
    gen = ctx.batch_info()[0]
    out = []
    for b, (r, ch) in enumerate(zip(res, channels)):
        proof = _mirror_commit(r, BatchMember(ctx, b), log_n, ch, generation=gen)
        proof.member = b
        out.append(proof)
    return out


def record_paths_len(log_n: int, trace_count: int, n_layers: int) -> int:
    """Bytes of the paths of one query record (fri_batch_query_round's) of a
    member with n_layers layers: trace_count paths of log_n digests, then layer
    k's two of log_n - k.  Its values are trace_count + 2 * n_layers words."""
    return trace_count * 32 * log_n + sum(64 * (log_n - k) for k in range(n_layers))


def batch_round_records(values: np.ndarray, paths: np.ndarray, paths_len: int, trace_count: int, n_layers: int,
                        log_n: int):
    """One member's record of Context.batch_query_round (its rows of values
    and paths, the bytes written) taken apart: ([(trace value, path)] *
    trace_count, decommit_query's tuples for the member's n_layers)."""
    tl = 32 * log_n
    if paths_len != record_paths_len(log_n, trace_count, n_layers):
        raise FriError(FRI_ESTATE, "the record does not hold this many layers (a skipped or failed member?)")
    raw = paths[:paths_len].tobytes()
    trace = [(int(values[j]), raw[j * tl:(j + 1) * tl]) for j in range(trace_count)]
    return trace, _openings(values, raw, n_layers, log_n, trace_count, trace_count * tl)


def query_phase_messages(indices, values: np.ndarray, paths: np.ndarray, n_layers: int, log_n: int,
                         trace_count: int, paths_len: Optional[int] = None) -> List[bytes]:
    """One member's rows of Context.batch_query_phase (its Q indices, (Q,
    stride) values and paths) as the messages of its query phase, in the
    transcript's order: per query be64(index), trace_count x (value, path),
    then per layer what _send_openings sends (a one-element layer's value
    once more first).  ``paths_len``: the bytes the call wrote per query, when
    batch_round_records is to check them against n_layers."""
    plen = record_paths_len(log_n, trace_count, n_layers) if paths_len is None else paths_len
    out: List[bytes] = []
    for q, index in enumerate(indices):
        out.append(int(index).to_bytes(8, "big"))
        trace, openings = batch_round_records(values[q], paths[q], plen, trace_count, n_layers, log_n)
        for v, path in trace:
            out += [v.to_bytes(8, "big"), path]
        for val, sval, path, spath in openings:
            if not path and not spath:
                out.append(val.to_bytes(8, "big"))
            out += [val.to_bytes(8, "big"), path, sval.to_bytes(8, "big"), spath]
    return out


def _device_query_phase(ctx: "Context", num_queries: int, max_index: int, fris: Sequence["FRIProof"],
                        channels: Sequence[Channel], log_n: int, trace_count: int, trace_stride: int):
    """The query phase of a batch through ONE fri_batch_query_phase: every
    channel takes over its member's messages and final state.  Returns the
    members' indices.  A member the device left out raises, as the round
    route's batch_round_records does."""
    if num_queries and any(not ch.state for ch in channels):
        raise FriError(FRI_ESTATE, "Channel state is not valid hex")       # channel.rs:65
    states = [bytes.fromhex(ch.state) if ch.state else None for ch in channels]
    idx, values, paths, lens, out = ctx.batch_query_phase(num_queries, max_index, states, trace_count=trace_count,
                                                          trace_stride=trace_stride,
                                                          max_layers=max(p.n_layers for p in fris))
    if num_queries == 0:
        return [[] for _ in fris]
    for b, (p, ch) in enumerate(zip(fris, channels)):
        ch.take_over_queries(query_phase_messages(idx[b], values[b], paths[b], p.n_layers, log_n, trace_count,
                                                  lens[b]), num_queries, out[b].hex())
    return [[int(i) for i in idx[b]] for b in range(len(fris))]


def decommit_fri_batch(num_queries: int, max_index: int, proofs: Sequence["FRIProof"],
                       channels: Sequence[Channel], device_queries: bool = False, grinding_bits: int = 0) -> None:
    """decommit_fri (fri_commit.rs:168-179) for every member of one batch
    (``proofs`` as fri_commit_batch or prove_fibsq_batch returned them, in
    member order): per round every channel draws its index, ONE
    fri_batch_query_round opens them all, and every channel absorbs its
    openings as decommit_fri_layers sends them.  ``device_queries=True``
    runs the whole phase, the channels' draws and sends included, in ONE
    fri_batch_query_phase instead (same transcripts and states; no host
    hashing).  Measured (profiles/prove_batch_device_queries.txt; log_t 7, 10, 13
    with 8 and 32 queries, blowup 8): the whole call is slower than the round
    route at B = 16 (0.47x to 0.71x) and faster from B = 64, the smallest
    measured size where it wins, at every shape and in both runs (1.1x to
    1.5x at 64, 1.9x to 2.5x at 256, up to 3.0x at 4096).
    ``grinding_bits`` > 0: every channel first grinds that many bits, on the
    device in ONE fri_grind_batch from GRIND_DEVICE_MIN_BITS up, by either
    route."""
    _check_grinding_bits(grinding_bits)
    if len(proofs) != len(channels):
        raise FriError(FRI_EINVAL, "one channel per proof")
    if len(proofs) == 0:
        return
    ctx, gen, log_n = proofs[0].ctx.ctx, proofs[0].generation, proofs[0].log_n
    if any(not isinstance(p.ctx, BatchMember) or p.ctx.ctx is not ctx or p.generation != gen or p.member != b
           for b, p in enumerate(proofs)):
        raise FriError(FRI_EINVAL, "proofs are not the members of one batch, in member order")
    g, members, ln = ctx.batch_info()
    if g != gen or members != len(proofs) or ln != log_n:
        raise FriError(FRI_ESTATE, "FRIProof layers were replaced by a later commit on the same context")
    _grind_batch(channels, grinding_bits, ctx)
    if device_queries:
        _device_query_phase(ctx, num_queries, max_index, proofs, channels, log_n, 0, 0)
        return
    for _ in range(num_queries):
        idx = [ch.receive_random_int(0, max_index, True) for ch in channels]
        values, paths, lens = ctx.batch_query_round(idx)
        for b, (p, ch) in enumerate(zip(proofs, channels)):
            _send_openings(batch_round_records(values[b], paths[b], lens[b], 0, p.n_layers, log_n)[1], ch)


def prove_fibsq_batch(a1s: Sequence[int], log_t: int, log_blowup: int, num_queries: int, channels: Sequence[Channel],
                      offset: int = GENERATOR, ctx: Optional[Context] = None,
                      device_queries: bool = False, grinding_bits: int = 0) -> List[StarkProof]:
    """prove_fibsq for many proofs of one shape, each with its own a1 and
    channel, in a fixed number of device calls: one fri_trace_commit_batch,
    one fri_fibsq_composition_commit_batch and one fri_batch_query_round per
    query round.  Member i's transcript (``channels[i].proof``) and state are
    what prove_fibsq(a1s[i], ...) into channels[i] gives.  A member whose
    trace violates the constraints raises FriError after the whole batch ran
    (the message names the member).  ``device_queries=True`` replaces the
    query rounds by ONE fri_batch_query_phase: three synchronising calls per
    batch, and the host hashes only the trace root and the alphas' draws.
    Measured (profiles/prove_batch_device_queries.txt; log_t 7, 10, 13
    with 8 and 32 queries, blowup 8): the whole call is slower than the round
    route at B = 16 (0.47x to 0.71x) and faster from B = 64, the smallest
    measured size where it wins, at every shape and in both runs (1.1x to
    1.5x at 64, 1.9x to 2.5x at 256, up to 3.0x at 4096).
    ``grinding_bits`` > 0: after the composition commit every channel grinds
    that many bits, on the device in ONE fri_grind_batch from
    GRIND_DEVICE_MIN_BITS up, by either route; the device route's query phase
    starts from the states that call returned."""
    _check_grinding_bits(grinding_bits)
    if len(a1s) != len(channels):
        raise FriError(FRI_EINVAL, "one channel per proof")
    if len(a1s) == 0:
        return []
    L = log_t + log_blowup
    B, n = 1 << log_blowup, 1 << L
    ctx = _beside_team(ctx or _default_ctx(L), L, _BATCH_CTX)     # batches run on one device
    traces = np.stack([fibsq_trace(a1, 1 << log_t) for a1 in a1s])
    roots = ctx.trace_commit_batch(traces, log_blowup, offset)
    alphas = []
    for root, ch in zip(roots, channels):
        ch.send(root.hex().encode())
        alphas.append([ch.receive_random_field_element() for _ in range(3)])
    res = ctx.fibsq_composition_commit_batch(log_t, log_blowup, traces[:, -1], alphas, offset,
                                             channel_states=[bytes.fromhex(ch.state) for ch in channels])
    gen = ctx.batch_info()[0]
    fris = []
    for b, (r, ch) in enumerate(zip(res, channels)):
        fri = _mirror_commit(r, BatchMember(ctx, b), L, ch, generation=gen)
        fri.member = b
        fris.append(fri)
    _grind_batch(channels, grinding_bits, ctx)
    queries = [[] for _ in a1s]
    if device_queries:
        queries = _device_query_phase(ctx, num_queries, n - 2 * B - 1, fris, channels, L, 3, B)
        num_queries = 0
    for _ in range(num_queries):
        idx = [ch.receive_random_int(0, n - 2 * B - 1, True) for ch in channels]
        values, paths, lens = ctx.batch_query_round(idx, trace_count=3, trace_stride=B)
        for b, (fri, ch) in enumerate(zip(fris, channels)):
            queries[b].append(idx[b])
            trace, openings = batch_round_records(values[b], paths[b], lens[b], 3, fri.n_layers, L)
            for v, path in trace:
                ch.send(v.to_bytes(8, "big"))
                ch.send(path)
            _send_openings(openings, ch)
    return [StarkProof(roots[b], alphas[b], int(traces[b, -1]), fris[b], log_t, log_blowup, queries[b])
            for b in range(len(a1s))]


# ---- batched verifier (fri_verify_batch) ------------------------------------
_HEXDIGITS = frozenset(b"0123456789abcdef")


@dataclass
class PackedTranscripts:
    """Transcripts of one shape in fri_verify_batch's record layout
    (fri_amd.h), as pack_transcripts leaves them.  ``reasons[b]`` is a host
    decision (VERIFY_MALFORMED) or 0; ``host[b]`` marks a member the existing
    host verifier decides (its root messages are not canonical lowercase hex,
    so they cannot be packed as raw bytes).  Both kinds hold zeros in the
    arrays and n_layers 1.  ``grinding_bits`` > 0: every member's message
    after the final value is its grinding nonce, in ``nonces``."""
    shape: VerifyShape
    chan: np.ndarray          # (batch, 36) uint8: fri_channel_state
    n_layers: np.ndarray      # (batch,) uint32
    a_last: Optional[np.ndarray]   # (batch,) uint32 when trace_count = 3
    head: np.ndarray          # (batch, head_stride) uint32
    indices: np.ndarray       # (batch, num_queries) uint64
    values: np.ndarray        # (batch, num_queries, values_stride) uint32
    paths: np.ndarray         # (batch, num_queries, paths_stride) uint8
    reasons: np.ndarray       # (batch,) uint32
    host: np.ndarray          # (batch,) bool
    nonces: Optional[np.ndarray] = None    # (batch,) uint64 (zeros without grinding bits)
    grinding_bits: int = 0

    @property
    def batch(self) -> int:
        return int(self.n_layers.size)

    def abi_args(self) -> tuple:
        """Context.verify_batch's arguments after ``self``, without verdict."""
        return (self.shape, self.batch, self.chan, self.n_layers, self.a_last, self.head, self.head.shape[1],
                self.indices, self.values, self.values.shape[2], self.paths, self.paths.shape[2])


def verify_record_strides(log_n: int, max_layers: int, trace_count: int) -> tuple:
    """(head words, values words, paths bytes) of one member's head and of one
    (member, query) record: the query record is fri_batch_query_round's."""
    return ((11 if trace_count else 0) + 9 * max_layers, trace_count + 2 * max_layers,
            record_paths_len(log_n, trace_count, max_layers))


def pack_transcripts(transcripts: Sequence[Sequence[bytes]], log_n: int, n_layers: Sequence[int], num_queries: int,
                     max_index: int, trace_count: int = 0, log_t: int = 0, log_blowup: int = 0,
                     a_last: Optional[Sequence[int]] = None, offset: int = GENERATOR,
                     channel_states: Optional[Sequence[str]] = None, grinding_bits: int = 0) -> PackedTranscripts:
    """Pure host code: the messages of verify_fri (trace_count 0) or
    verify_fibsq (trace_count 3) transcripts into fri_verify_batch's arrays.
    A member is decided here only where the host verifier certainly rejects
    it (VERIFY_MALFORMED in ``reasons``): a wrong message count for its
    n_layers, a message of the wrong length, a value, challenge or final value
    >= p, a one-element layer whose doubled value differs.  A member whose
    root messages are not canonical lowercase hex is left to the host verifier
    (``host``), as is the one case _verify_transcript does not settle by
    length, an FRI value that is not 8 bytes.  ``grinding_bits`` > 0: one
    more message per member, the nonce after the final value, which must be 8
    bytes (else VERIFY_MALFORMED) and goes into ``nonces``."""
    _check_grinding_bits(grinding_bits)
    B = len(transcripts)
    if len(n_layers) != B or (channel_states is not None and len(channel_states) != B) or \
            (trace_count and (a_last is None or len(a_last) != B)):
        raise FriError(FRI_EINVAL, "one n_layers, a_last and channel state per transcript")
    if trace_count not in (0, 3):
        raise FriError(FRI_EINVAL, "trace_count must be 0 or 3")
    L, Q, tc = log_n, num_queries, trace_count
    ok_nl = [nl for nl in n_layers if 1 <= nl <= L + 1]
    ML = max(ok_nl, default=1)
    hw, vw, pb = verify_record_strides(L, ML, tc)
    hb = 11 if tc else 0
    shape = VerifyShape(L, ML, Q, tc, log_t, log_blowup, offset % (1 << 32), max_index)
    pk = PackedTranscripts(shape, np.zeros((B, 36), np.uint8), np.ones(B, np.uint32),
                           np.zeros(B, np.uint32) if tc else None, np.zeros((B, hw), np.uint32),
                           np.zeros((B, Q), np.uint64), np.zeros((B, Q, vw), np.uint32),
                           np.zeros((B, Q, max(pb, 1)), np.uint8), np.zeros(B, np.uint32), np.zeros(B, bool),
                           np.zeros(B, np.uint64), grinding_bits)

    class _Malformed(Exception):
        pass

    class _Host(Exception):
        pass

    def u64(m: bytes, what_host: bool = False) -> int:
        if len(m) != 8:
            raise (_Host if what_host else _Malformed)()
        v = int.from_bytes(m, "big")
        if v >= P:
            raise _Malformed()
        return v

    def root_words(m: bytes):
        if len(m) != 64:
            raise _Malformed()
        if not all(c in _HEXDIGITS for c in m):
            raise _Host()
        return np.frombuffer(bytes.fromhex(m.decode()), dtype=">u4")

    for b, msgs in enumerate(transcripts):
        msgs, nl = list(msgs), n_layers[b]
        try:
            if not 1 <= nl <= L + 1:
                raise _Malformed()
            per_q = 1 + 2 * tc + sum(5 if L - k == 0 else 4 for k in range(nl))
            if len(msgs) != (4 if tc else 0) + 2 * nl + (1 if grinding_bits else 0) + Q * per_q:
                raise _Malformed()
            head, idxs, vals, pths = np.zeros(hw, np.uint32), [], np.zeros((Q, vw), np.uint32), []
            it = iter(msgs)
            if tc:
                head[0:8] = root_words(next(it))
                for j in range(3):
                    head[8 + j] = u64(next(it))
            for k in range(nl):
                head[hb + 8 * k:hb + 8 * k + 8] = root_words(next(it))
                if k < nl - 1:
                    head[hb + 8 * ML + k] = u64(next(it))
            fin = next(it)
            if Q == 0 and len(fin) == 8 and int.from_bytes(fin, "big") >= P:
                raise _Host()                 # no query ever compares it
            head[hb + 9 * ML - 1] = u64(fin)
            nonce = 0
            if grinding_bits:
                m = next(it)
                if len(m) != 8:
                    raise _Malformed()
                nonce = int.from_bytes(m, "big")
            for q in range(Q):
                m = next(it)
                if len(m) != 8:
                    raise _Malformed()
                idxs.append(int.from_bytes(m, "big"))
                rec = bytearray()
                for j in range(tc):
                    vals[q, j] = u64(next(it))
                    path = next(it)
                    if len(path) != 32 * L:
                        raise _Malformed()
                    rec += path
                for k in range(nl):
                    depth = L - k
                    extra = next(it) if depth == 0 else None
                    vb, path, sb, spath = next(it), next(it), next(it), next(it)
                    if extra is not None and extra != vb:
                        raise _Malformed()
                    if len(path) != 32 * depth or len(spath) != 32 * depth:
                        raise _Malformed()
                    vals[q, tc + 2 * k], vals[q, tc + 2 * k + 1] = u64(vb, True), u64(sb, True)
                    rec += path + spath
                pths.append(bytes(rec))
        except _Malformed:
            pk.reasons[b] = VERIFY_MALFORMED
            continue
        except _Host:
            pk.host[b] = True
            continue
        st = channel_states[b] if channel_states is not None else ""
        if st:
            pk.chan[b, :32] = np.frombuffer(bytes.fromhex(st), np.uint8)
            pk.chan[b, 32] = 1
        pk.n_layers[b] = nl
        if tc:
            pk.a_last[b] = int(a_last[b]) % P     # verify_fibsq reduces it too (fibsq_cp_at)
        pk.head[b] = head
        pk.nonces[b] = nonce
        pk.values[b] = vals
        for q in range(Q):
            pk.indices[b, q] = idxs[q]
            pk.paths[b, q, :len(pths[q])] = np.frombuffer(pths[q], np.uint8)
    return pk


def unpack_transcripts(pk: PackedTranscripts) -> List[Optional[List[bytes]]]:
    """pack_transcripts' inverse: every packed member's messages (None for a
    member decided on the host, whose record holds nothing)."""
    sh = pk.shape
    L, ML, Q, tc = sh.log_n, sh.max_layers, sh.num_queries, sh.trace_count
    hb = 11 if tc else 0
    out = []
    for b in range(pk.batch):
        if pk.reasons[b] or pk.host[b]:
            out.append(None)
            continue
        nl, head, msgs = int(pk.n_layers[b]), pk.head[b], []
        be = lambda v: int(v).to_bytes(8, "big")
        root = lambda w: w.astype(">u4").tobytes().hex().encode()
        if tc:
            msgs.append(root(head[0:8]))
            msgs += [be(head[8 + j]) for j in range(3)]
        for k in range(nl):
            msgs.append(root(head[hb + 8 * k:hb + 8 * k + 8]))
            if k < nl - 1:
                msgs.append(be(head[hb + 8 * ML + k]))
        msgs.append(be(head[hb + 9 * ML - 1]))
        if pk.grinding_bits:
            msgs.append(be(pk.nonces[b]))
        for q in range(Q):
            vals, raw = pk.values[b, q], pk.paths[b, q].tobytes()
            msgs.append(be(pk.indices[b, q]))
            for j in range(tc):
                msgs += [be(vals[j]), raw[32 * L * j:32 * L * (j + 1)]]
            off = 32 * L * tc
            for k in range(nl):
                pl = 32 * (L - k)
                if L - k == 0:
                    msgs.append(be(vals[tc + 2 * k]))
                msgs += [be(vals[tc + 2 * k]), raw[off:off + pl], be(vals[tc + 2 * k + 1]), raw[off + pl:off + 2 * pl]]
                off += 2 * pl
        out.append(msgs)
    return out


def _verify_packed(pk: PackedTranscripts, host_verify, ctx: Optional[Context], reasons: Optional[list]) -> List[bool]:
    """The masks of a packed batch: the host's decisions where the packer made
    one, ``host_verify(b)`` where it left the member to the host verifier, the
    device's for every other member (in calls of at most BATCH_MAX)."""
    mask = pk.reasons.copy()
    device = ~(pk.host | (pk.reasons != 0))
    if device.any():
        L = pk.shape.log_n
        ctx = _beside_team(ctx or _default_ctx(L), L, _BATCH_CTX)     # the verifier runs on one device
        args = pk.abi_args()
        for b0 in range(0, pk.batch, BATCH_MAX):
            b1 = min(pk.batch, b0 + BATCH_MAX)
            got = ctx.verify_batch(args[0], b1 - b0, pk.chan[b0:b1], pk.n_layers[b0:b1],
                                   pk.a_last[b0:b1] if pk.a_last is not None else None, pk.head[b0:b1], args[6],
                                   pk.indices[b0:b1], pk.values[b0:b1], args[9], pk.paths[b0:b1], args[11],
                                   grinding_bits=pk.grinding_bits, nonces=pk.nonces[b0:b1])
            mask[b0:b1] = np.where(device[b0:b1], got, mask[b0:b1])
    for b in np.flatnonzero(pk.host):
        mask[b] = 0 if host_verify(int(b)) else VERIFY_MALFORMED
    if reasons is not None:
        reasons[:] = [int(m) for m in mask]
    return [bool(m == 0) for m in mask]


def verify_fri_batch(transcripts: Sequence[Sequence[bytes]], log_n: int, n_layers: Sequence[int], num_queries: int,
                     max_index: int, offset: int = GENERATOR, channel_states: Optional[Sequence[str]] = None,
                     ctx: Optional[Context] = None, reasons: Optional[list] = None,
                     grinding_bits: int = 0) -> List[bool]:
    """verify_fri for many transcripts of one shape (log_n, num_queries,
    max_index, offset), member b with its own n_layers[b] and channel state,
    in one device call (fri_verify_batch).  Returns what a loop of verify_fri
    returns; ``reasons`` (a list) receives the VERIFY_* masks.
    ``grinding_bits`` > 0 (one value for the batch): every transcript carries
    its nonce after the final value (fri_verify_batch_pow, VERIFY_POW)."""
    _check_grinding_bits(grinding_bits)
    if len(n_layers) != len(transcripts) or (channel_states is not None and len(channel_states) != len(transcripts)):
        raise FriError(FRI_EINVAL, "one n_layers and channel state per transcript")
    if len(transcripts) == 0:
        if reasons is not None:
            reasons[:] = []
        return []
    pk = pack_transcripts(transcripts, log_n, n_layers, num_queries, max_index, offset=offset,
                          channel_states=channel_states, grinding_bits=grinding_bits)
    state = lambda b: channel_states[b] if channel_states is not None else ""
    return _verify_packed(pk, lambda b: verify_fri(transcripts[b], log_n, n_layers[b], num_queries, max_index, offset,
                                                   state(b), grinding_bits), ctx, reasons)


def verify_fibsq_batch(transcripts: Sequence[Sequence[bytes]], a_last: Sequence[int], log_t: int, log_blowup: int,
                       num_queries: int, n_layers: Sequence[int], offset: int = GENERATOR,
                       channel_states: Optional[Sequence[str]] = None, ctx: Optional[Context] = None,
                       reasons: Optional[list] = None, grinding_bits: int = 0) -> List[bool]:
    """verify_fibsq for many transcripts of one shape, member b with its own
    a_last[b], n_layers[b] and channel state, in one device call.  Returns what
    a loop of verify_fibsq returns; ``reasons`` receives the VERIFY_* masks.
    ``grinding_bits`` > 0: as verify_fri_batch's."""
    _check_grinding_bits(grinding_bits)
    B = len(transcripts)
    if len(a_last) != B or len(n_layers) != B or (channel_states is not None and len(channel_states) != B):
        raise FriError(FRI_EINVAL, "one a_last, n_layers and channel state per transcript")
    if B == 0:
        if reasons is not None:
            reasons[:] = []
        return []
    L = log_t + log_blowup
    a_last = [int(a) % P for a in a_last]     # verify_fibsq reduces it (FE / fibsq_cp_at)
    pk = pack_transcripts(transcripts, L, n_layers, num_queries, (1 << L) - 2 * (1 << log_blowup) - 1, 3, log_t,
                          log_blowup, a_last, offset, channel_states, grinding_bits)
    state = lambda b: channel_states[b] if channel_states is not None else ""
    return _verify_packed(pk, lambda b: verify_fibsq(transcripts[b], a_last[b], log_t, log_blowup, num_queries,
                                                     n_layers[b], offset, state(b), grinding_bits), ctx, reasons)


def fri_commit_sharded(coeffs: Sequence[int], log_n: int, channel: Channel, ctx: Context,
                       offset: int = GENERATOR) -> FRIProof:
    """fri_commit (fri_commit.rs:72-122) over the ranks attached to ``ctx``
    (one process per GPU, every rank passing the same coefficients and
    channel): coset-sharded on the devices, the same transcript on every rank.
    decommit_fri on the returned proof is collective (all ranks, same order)."""
    st = bytes.fromhex(channel.state) if channel.state else None
    res = ctx.commit_sharded(coeffs, log_n, offset, channel_state=st)
    proof = _mirror_commit(res, ctx, log_n, channel)
    proof.sharded = True
    return proof


def _mirror_commit(res: CommitResult, ctx: Context, log_n: int, channel: Channel,
                   generation: Optional[int] = None) -> FRIProof:
    """Append the messages the device commit sent (root hex per layer, beta
    per round, final value) to ``channel`` and take over its state."""
    roots = [bytes(res.roots[k]) for k in range(res.n_layers)]
    betas = [int(res.betas[r]) for r in range(res.n_rounds)]
    for k, root in enumerate(roots):
        channel.proof.append(root.hex().encode())
        channel.compressed_proof.append(root.hex().encode())
        if k < len(betas):
            channel.proof.append(betas[k].to_bytes(8, "big"))
    fv = int(res.final_value).to_bytes(8, "big")
    channel.proof.append(fv)
    channel.compressed_proof.append(fv)
    channel.state = bytes(res.channel_out.digest).hex() if res.channel_out.has_state else ""
    gen = ctx.commit_info()[0] if generation is None else generation
    return FRIProof(ctx, log_n, roots, betas, int(res.final_value), int(res.final_degree), gen)
