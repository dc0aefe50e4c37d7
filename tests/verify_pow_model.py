"""What fri_verify_batch_pow's verdict mask must be (fri_amd.h: the nonce is
sent after the final value, the state after that send must have grinding_bits
leading zero bits, "the replay goes on from that state whether it has them or
not").  CPU code over hashlib, numpy and the Python oracle; from the library
under test only the VERIFY_* constants.

The openings' classes do not depend on the channel, so they are
verify_mask_model's.  The channel is replayed here, in verify_mask_model's units
over fri_oracle.Channel, with the nonce sent as its 8 big-endian bytes after
the final value; the zero bits are grind_model's.  The replay gives
VERIFY_CHANNEL and VERIFY_POW and never stops early."""
import numpy as np

import fri_oracle as fo
import grind_model as gm
import verify_mask_model as vm
from fri_amd import VERIFY_CHANNEL, VERIFY_POW

P = fo.P


def replay_mask(shape, chan, n_layers, head, indices, values, paths, nonce, bits):
    """VERIFY_CHANNEL | VERIFY_POW of one member: every claimed alpha, beta
    and index against the replay, and the state after the nonce's send."""
    L, ML, Q, tc = int(shape.log_n), int(shape.max_layers), int(shape.num_queries), int(shape.trace_count)
    max_index = int(shape.max_index)
    nl, hb = int(n_layers), 11 if tc else 0
    hw, vw, pb = vm.record_strides(L, ML, tc)
    head = [int(w) for w in head[:hw]]
    root = lambda o: np.asarray(head[o:o + 8], dtype=">u4").tobytes()      # noqa: E731
    alphas = head[8:11] if tc else []
    betas = head[hb + 8 * ML:hb + 8 * ML + nl - 1]
    final = head[hb + 9 * ML - 1]
    mask = 0
    state = bytes(np.asarray(chan[:32], dtype=np.uint8)).hex() if int(chan[32]) else ""
    ch = fo.Channel(state=state)
    if tc:
        ch.send(root(0).hex().encode())
        for a in alphas:
            if ch.receive_random_field_element() != a:
                mask |= VERIFY_CHANNEL
    for k in range(nl):
        ch.send(root(hb + 8 * k).hex().encode())
        if k < nl - 1 and ch.receive_random_field_element() != betas[k]:
            mask |= VERIFY_CHANNEL
    ch.send(fo.fe_to_bytes(final))
    if bits:
        ch.send(int(nonce).to_bytes(8, "big"))
        if gm.zero_bits(ch.state) < bits:
            mask |= VERIFY_POW
    for q in range(Q):
        if ch.receive_random_int(0, max_index, True) != int(indices[q]):
            mask |= VERIFY_CHANNEL
        v = [int(w) for w in values[q][:vw]]
        pth = bytes(np.asarray(paths[q][:pb], dtype=np.uint8))
        off = 0
        for j in range(tc):
            ch.send(fo.fe_to_bytes(v[j]))
            ch.send(pth[off:off + 32 * L])
            off += 32 * L
        for k in range(nl):
            depth = L - k
            a, b = v[tc + 2 * k], v[tc + 2 * k + 1]
            if depth == 0:
                ch.send(fo.fe_to_bytes(a))
            ch.send(fo.fe_to_bytes(a))
            ch.send(pth[off:off + 32 * depth])
            ch.send(fo.fe_to_bytes(b))
            ch.send(pth[off + 32 * depth:off + 64 * depth])
            off += 64 * depth
    return mask


def member_mask(shape, chan, n_layers, a_last, head, indices, values, paths, nonce, bits):
    """One member's mask under `bits` grinding bits (0: no nonce message)."""
    opened = vm.member_mask(shape, chan, n_layers, a_last, head, indices, values, paths) & ~VERIFY_CHANNEL
    return opened | replay_mask(shape, chan, n_layers, head, indices, values, paths, nonce, bits)


def expected_masks(pk, bits=None):
    """The mask of every member of a PackedTranscripts, as a uint32 array;
    `bits` defaults to the bits it was packed with."""
    bits = int(pk.grinding_bits) if bits is None else bits
    B = int(pk.n_layers.size)
    return np.array([member_mask(pk.shape, pk.chan[b], pk.n_layers[b], pk.a_last[b] if pk.a_last is not None else 0,
                                 pk.head[b], pk.indices[b], pk.values[b], pk.paths[b], pk.nonces[b], bits)
                     for b in range(B)], dtype=np.uint32)
