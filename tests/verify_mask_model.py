"""What fri_verify_batch's verdict mask must be, check by check (fri_amd.h:
"Every check runs for every member: verdict[b] is the OR of the failed classes").
CPU code over hashlib, numpy and the Python oracle; from the library under test
only the VERIFY_* constants.  verify_fri / verify_fibsq stop at the first
mismatch and can only say accept or reject; this runs every check of every
class on a packed record and never stops early.

The model takes the arrays of a PackedTranscripts, not messages, so a record no
message can express (a claimed index with high bits set, a padded stride) has a
mask too.  It is defined for records whose words are all below p; it refuses
any other (ValueError), so that it cannot encode whatever the kernels happen to
do with them."""
import hashlib

import numpy as np

import fri_oracle as fo
from fri_amd import (VERIFY_CHANNEL, VERIFY_COMPOSITION, VERIFY_FINAL, VERIFY_FOLD, VERIFY_FRI_PATH,
                     VERIFY_TRACE_PATH)

P = fo.P


def record_strides(log_n, max_layers, trace_count):
    """(head words, values words, paths bytes) of fri_amd.h's record layout."""
    return ((11 if trace_count else 0) + 9 * max_layers, trace_count + 2 * max_layers,
            32 * log_n * trace_count + sum(64 * (log_n - k) for k in range(max_layers)))


def _reaches(value, pos, path, depth, root):
    """leaf = SHA256(be64(value)), then `depth` siblings, left/right by pos's bits."""
    h = hashlib.sha256(fo.fe_to_bytes(value)).digest()
    for lvl in range(depth):
        sib = path[32 * lvl:32 * lvl + 32]
        h = hashlib.sha256(sib + h if (pos >> lvl) & 1 else h + sib).digest()
    return h == root


def _composition(f0, f1, f2, x, alphas, a_last, log_t):
    """a0 (f-1)/(x-1) + a1 (f-A)/(x-g^(T-1)) + a2 (f(g^2 x) - f(gx)^2 - f^2) (x-g^(T-2))(x-g^(T-1))/(x^T-1)"""
    T = 1 << log_t
    g = fo.fe_pow(fo.GEN, (P - 1) >> log_t, P)
    glast, gprev = fo.fe_pow(g, T - 1, P), fo.fe_pow(g, T - 2, P)
    p0 = fo.fe_div(fo.fe_sub(f0, 1, P), fo.fe_sub(x, 1, P), P)
    p1 = fo.fe_div(fo.fe_sub(f0, a_last, P), fo.fe_sub(x, glast, P), P)
    num = fo.fe_sub(f2, fo.fe_add(fo.fe_mul(f1, f1, P), fo.fe_mul(f0, f0, P), P), P)
    z = fo.fe_mul(fo.fe_sub(x, gprev, P), fo.fe_sub(x, glast, P), P)
    p2 = fo.fe_div(fo.fe_mul(num, z, P), fo.fe_sub(fo.fe_pow(x, T, P), 1, P), P)
    terms = [fo.fe_mul(a, p, P) for a, p in zip(alphas, (p0, p1, p2))]
    return fo.fe_add(fo.fe_add(terms[0], terms[1], P), terms[2], P)


def member_mask(shape, chan, n_layers, a_last, head, indices, values, paths):
    """One member's mask.  chan: its 36 fri_channel_state bytes; head: its head
    words; indices (Q,), values (Q, >= record words), paths (Q, >= record bytes)."""
    L, ML, Q, tc = int(shape.log_n), int(shape.max_layers), int(shape.num_queries), int(shape.trace_count)
    log_t, lb, offset, max_index = int(shape.log_t), int(shape.log_blowup), int(shape.offset), int(shape.max_index)
    nl, hb = int(n_layers), 11 if tc else 0
    hw, vw, pb = record_strides(L, ML, tc)
    head = [int(w) for w in head[:hw]]
    root = lambda o: np.asarray(head[o:o + 8], dtype=">u4").tobytes()      # noqa: E731
    troot = root(0) if tc else None
    alphas = head[8:11] if tc else []
    roots = [root(hb + 8 * k) for k in range(nl)]
    betas = head[hb + 8 * ML:hb + 8 * ML + nl - 1]
    final = head[hb + 9 * ML - 1]
    vals = [[int(w) for w in values[q][:vw]] for q in range(Q)]
    pths = [bytes(np.asarray(paths[q][:pb], dtype=np.uint8)) for q in range(Q)]
    used = alphas + betas + [final] + [w for v in vals for w in v[:tc + 2 * nl]]
    if any(w >= P for w in used):
        raise ValueError("the mask model is defined for canonical words only")
    mask = 0

    # CHANNEL: replay a channel over what the record claims
    state = bytes(np.asarray(chan[:32], dtype=np.uint8)).hex() if int(chan[32]) else ""
    ch = fo.Channel(state=state)
    if tc:
        ch.send(troot.hex().encode())
        for a in alphas:
            if ch.receive_random_field_element() != a:
                mask |= VERIFY_CHANNEL
    for k in range(nl):
        ch.send(roots[k].hex().encode())
        if k < nl - 1 and ch.receive_random_field_element() != betas[k]:
            mask |= VERIFY_CHANNEL
    ch.send(fo.fe_to_bytes(final))
    for q in range(Q):
        if ch.receive_random_int(0, max_index, True) != int(indices[q]):
            mask |= VERIFY_CHANNEL
        off = 0
        for j in range(tc):
            ch.send(fo.fe_to_bytes(vals[q][j]))
            ch.send(pths[q][off:off + 32 * L])
            off += 32 * L
        for k in range(nl):
            depth = L - k
            v, sv = vals[q][tc + 2 * k], vals[q][tc + 2 * k + 1]
            if depth == 0:
                ch.send(fo.fe_to_bytes(v))
            ch.send(fo.fe_to_bytes(v))
            ch.send(pths[q][off:off + 32 * depth])
            ch.send(fo.fe_to_bytes(sv))
            ch.send(pths[q][off + 32 * depth:off + 64 * depth])
            off += 64 * depth

    # the openings, against the claimed challenges and indices
    for q in range(Q):
        index, v, pth = int(indices[q]), vals[q], pths[q]
        off = 0
        for j in range(tc):
            pos = (index + (j << lb)) % (1 << L)
            if not _reaches(v[j], pos, pth[off:off + 32 * L], L, troot):
                mask |= VERIFY_TRACE_PATH
            off += 32 * L
        for k in range(nl):
            depth = L - k
            m = 1 << depth
            i = index % m
            a, b = v[tc + 2 * k], v[tc + 2 * k + 1]
            if not _reaches(a, i, pth[off:off + 32 * depth], depth, roots[k]):
                mask |= VERIFY_FRI_PATH
            if not _reaches(b, (i + m // 2) % m, pth[off + 32 * depth:off + 64 * depth], depth, roots[k]):
                mask |= VERIFY_FRI_PATH
            off += 64 * depth
            if k >= 1:
                pm = 2 * m
                pi = index % pm
                lo, hi = v[tc + 2 * k - 2], v[tc + 2 * k - 1]
                if pi >= pm // 2:
                    lo, hi = hi, lo
                w = fo.fe_pow(fo.GEN, (P - 1) // pm, P)
                x = fo.fe_mul(fo.fe_pow(offset, 1 << (k - 1), P), fo.fe_pow(w, pi % (pm // 2), P), P)
                t = fo.fe_div(fo.fe_mul(betas[k - 1], fo.fe_sub(lo, hi, P), P), x, P)
                if fo.fe_div(fo.fe_add(fo.fe_add(lo, hi, P), t, P), 2, P) != a:
                    mask |= VERIFY_FOLD
            if k == nl - 1 and (a != final or b != final):
                mask |= VERIFY_FINAL
        if tc:
            w = fo.fe_pow(fo.GEN, (P - 1) >> L, P)
            x = fo.fe_mul(offset, fo.fe_pow(w, index % (1 << L), P), P)
            if _composition(v[0], v[1], v[2], x, alphas, int(a_last), log_t) != v[tc]:
                mask |= VERIFY_COMPOSITION
    return mask


def expected_masks(pk):
    """The mask of every member of a PackedTranscripts (any strides at or above
    the record's), as a uint32 array."""
    B = int(pk.n_layers.size)
    return np.array([member_mask(pk.shape, pk.chan[b], pk.n_layers[b], pk.a_last[b] if pk.a_last is not None else 0,
                                 pk.head[b], pk.indices[b], pk.values[b], pk.paths[b]) for b in range(B)],
                    dtype=np.uint32)
