"""The batches of the verdict-mask tests (test_verify_mask_model_host.py on the
CPU, test_gpu_verify_masks.py on the device): packed records built from oracle
transcripts and forgeries (verify_batch_cases.py) and from mutations of the
packed arrays that no message can express.  CPU code only; built once per
process."""
import dataclasses
import functools
import hashlib
import random

import numpy as np

import fri_amd
import verify_batch_cases as vc

P = vc.P
S1, S2 = hashlib.sha256(b"one").hexdigest(), hashlib.sha256(b"two").hexdigest()
MIXED = [5, 1, 64, 2, 16]                 # coefficients at log_n = 6: 4, 1, 7, 2 and 5 layers
COEFFS_OF_LAYERS = {1: 1, 2: 2, 3: 4, 4: 5, 5: 16, 6: 32, 7: 64}     # at log_n = 6


@dataclasses.dataclass
class Batch:
    pk: "fri_amd.PackedTranscripts"
    names: list                           # one label per member
    msgs: list = None                     # the messages that were packed, where the packer may decide a member
    nls: list = None                      # and their n_layers

    @property
    def device(self):
        """The members pack_transcripts left to the device."""
        return ~(self.pk.host | (self.pk.reasons != 0))


def pack_fibsq(msgs, a_last, nl, shape, offset=5, states=None):
    log_t, lb, q = shape
    L = log_t + lb
    return fri_amd.pack_transcripts(msgs, L, nl, q, (1 << L) - 2 * (1 << lb) - 1, 3, log_t, lb, a_last,
                                    offset=offset, channel_states=states)


def with_shape(pk, **fields):
    """pk under another shape (offset, max_index): the arrays are shared."""
    sh = fri_amd.VerifyShape.from_buffer_copy(pk.shape)
    for k, v in fields.items():
        setattr(sh, k, v)
    return dataclasses.replace(pk, shape=sh)


def select(pk, rows):
    """A batch of copies of pk's members `rows` (repeats allowed)."""
    rows = np.asarray(rows, dtype=np.intp)
    return dataclasses.replace(pk, chan=pk.chan[rows].copy(), n_layers=pk.n_layers[rows].copy(),
                               a_last=pk.a_last[rows].copy() if pk.a_last is not None else None,
                               head=pk.head[rows].copy(), indices=pk.indices[rows].copy(),
                               values=pk.values[rows].copy(), paths=pk.paths[rows].copy(),
                               reasons=pk.reasons[rows].copy(), host=pk.host[rows].copy())


def padded(pk, head_words=3, value_words=5, path_bytes=7):
    """pk re-laid with strides above the record's, the padding all 0xFF."""
    B, Q = pk.indices.shape
    head = np.full((B, pk.head.shape[1] + head_words), 0xFFFFFFFF, np.uint32)
    values = np.full((B, Q, pk.values.shape[2] + value_words), 0xFFFFFFFF, np.uint32)
    paths = np.full((B, Q, pk.paths.shape[2] + path_bytes), 0xFF, np.uint8)
    head[:, :pk.head.shape[1]] = pk.head
    values[:, :, :pk.values.shape[2]] = pk.values
    paths[:, :, :pk.paths.shape[2]] = pk.paths
    return dataclasses.replace(pk, head=head, values=values, paths=paths)


def host_accepts(pk, b, msgs=None, nl=None):
    """fri_amd.verify_fibsq / verify_fri on member b's unpacked messages (or
    on the messages it was packed from, for a member the packer decided)."""
    sh = pk.shape
    msgs = msgs if msgs is not None else fri_amd.unpack_transcripts(select(pk, [b]))[0]
    nl = int(pk.n_layers[b]) if nl is None else nl
    state = pk.chan[b, :32].tobytes().hex() if pk.chan[b, 32] else ""
    if sh.trace_count:
        return fri_amd.verify_fibsq(msgs, int(pk.a_last[b]), sh.log_t, sh.log_blowup, sh.num_queries,
                                    nl, sh.offset, state)
    return fri_amd.verify_fri(msgs, sh.log_n, nl, sh.num_queries, sh.max_index, sh.offset, state)


# ---- (a) every message flipped ----------------------------------------------
def _with_flips(msgs, log_n, nl, q, tc, label):
    cls = vc.message_classes(log_n, nl, q, tc)
    assert len(cls) == len(msgs)
    out, names = [list(msgs)], [label]
    for i, m in enumerate(msgs):
        if m:
            out.append(vc.flip(msgs, i))
            names.append("%s/%s@%d" % (label, cls[i], i))
    return out, names


@functools.lru_cache(maxsize=None)
def flipped_fibsq(shape):
    log_t, lb, q = shape
    msgs, a_last, nl = vc.fibsq_case(99, log_t, lb, q)
    batch, names = _with_flips(list(msgs), log_t + lb, nl, q, 3, "honest")
    nls = [nl] * len(batch)
    return Batch(pack_fibsq(batch, [a_last] * len(batch), nls, shape), names, batch, nls)


@functools.lru_cache(maxsize=None)
def flipped_fri_mixed():
    batch, names, nls = [], [], []
    for d in MIXED:
        msgs, nl = vc.fri_case(7 + d, d, 6, 2, 63)
        b, n = _with_flips(list(msgs), 6, nl, 2, 0, "coeffs%d" % d)
        batch += b
        names += n
        nls += [nl] * len(b)
    return Batch(fri_amd.pack_transcripts(batch, 6, nls, 2, 63), names, batch, nls)


HALVES_A1 = (3, 99, 31337)


@functools.lru_cache(maxsize=None)
def halves_batch(shape):
    """Accepted transcripts whose drawn indices the host test pins: at
    (4, 2, 4) both halves of every layer are opened, at (5, 3, 4) a1 = 31337
    opens only the high half of layers 0 and 1."""
    cases = [vc.fibsq_case(a1, *shape) for a1 in HALVES_A1]
    pk = pack_fibsq([list(c[0]) for c in cases], [c[1] for c in cases], [c[2] for c in cases], shape)
    return Batch(pk, ["a1 = %d" % a1 for a1 in HALVES_A1])


@functools.lru_cache(maxsize=None)
def path_word_batch():
    """An accepted (4, 2, 2) record with one path byte corrupted in the packed
    array, nothing re-derived: a trace path, a layer path, a sibling path."""
    msgs, a_last, nl = vc.fibsq_case(99, 4, 2, 2)
    pk = select(pack_fibsq([list(msgs)], [a_last], [nl], (4, 2, 2)), [0] * 4)
    L = 6
    pk.paths[1, 0, 32 * L + 5] ^= 0x80               # query 0, trace path 1
    pk.paths[2, 1, 3 * 32 * L + 64 * L + 3] ^= 1     # query 1, layer 1's path
    pk.paths[3, 0, 3 * 32 * L + 32 * L + 9] ^= 4     # query 0, layer 0's sibling path
    return Batch(pk, ["intact", "trace path", "layer path", "sibling path"])


# ---- (b) one layer wrong at a time ------------------------------------------
@functools.lru_cache(maxsize=None)
def layers_batch(shape, cp_seed=None):
    log_t, lb, q = shape
    nl = vc.forged_fibsq(log_t, lb, q, cp_seed=cp_seed)[2]
    kws = [("layer%d" % k, dict(tweak=vc.bump_layer(k))) for k in range(nl)]
    kws += [("high%d" % k, dict(tweak=vc.bump_layer(k, True))) for k in range(nl)]
    kws += [("final+1", dict(final_delta=1))]
    if cp_seed is None:
        kws += [("cp_seed", dict(cp_seed=3))]
    cases = [vc.forged_fibsq(log_t, lb, q, **dict(dict(cp_seed=cp_seed), **kw)) for _, kw in kws]
    pk = pack_fibsq([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], shape)
    return Batch(pk, [n for n, _ in kws])


# ---- (c) the composition, term by term --------------------------------------
@functools.lru_cache(maxsize=None)
def composition_batch():
    import fri_oracle as fo
    shape = (4, 2, 3)
    honest = vc.forged_fibsq(*shape)
    other_a_last = lambda fe, alphas, a_last: [int(v) for v in fo.fibsq_cp_evals_np(     # noqa: E731
        fe, shape[0], shape[1], fo.GEN, (a_last + 1) % P, alphas)]
    cases = [("honest", honest),
             ("alphas(1,0,2)", vc.forged_fibsq(*shape, cp_alphas=lambda a: [a[1], a[0], a[2]])),
             ("alphas(0,2,1)", vc.forged_fibsq(*shape, cp_alphas=lambda a: [a[0], a[2], a[1]])),
             ("a_last+1 in layer 0", vc.forged_fibsq(*shape, layer0=other_a_last)),
             ("verified with a_last+1", (honest[0], (honest[1] + 1) % P, honest[2]))]
    pk = pack_fibsq([c[0] for _, c in cases], [c[1] for _, c in cases], [c[2] for _, c in cases], shape)
    return Batch(pk, [n for n, _ in cases])


# ---- (d) offsets ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def offset_batch(kind, offset):
    """Honest transcripts made at `offset`, packed under it."""
    if kind == "fibsq":
        cases = [vc.fibsq_case(a1, 4, 2, 2, st, offset) for a1, st in ((3, ""), (99, S1))]
        pk = pack_fibsq([list(c[0]) for c in cases], [c[1] for c in cases], [c[2] for c in cases], (4, 2, 2),
                        offset=offset, states=["", S1])
    else:
        cases = [vc.fri_case(7 + d, d, 6, 2, 63, "", offset) for d in (64, 5)]
        pk = fri_amd.pack_transcripts([list(c[0]) for c in cases], 6, [c[1] for c in cases], 2, 63, offset=offset)
    return Batch(pk, ["%s offset %d #%d" % (kind, offset, i) for i in range(2)])


OFFSETS = [("fibsq", 7), ("fibsq", 25), ("fri", 1), ("fri", 7), ("fri", 25)]


# ---- (e) the index draw -----------------------------------------------------
MAX_INDICES = [0, 63, 1 << 31, (1 << 32) - 1]


@functools.lru_cache(maxsize=None)
def index_batch(max_index):
    msgs, nl = vc.fri_case(71, 64, 6, 4, max_index)
    return Batch(fri_amd.pack_transcripts([list(msgs)], 6, [nl], 4, max_index), ["max_index %d" % max_index])


@functools.lru_cache(maxsize=None)
def index_alias_batch(max_index):
    """An accepted record with one claimed index replaced by an alias of the
    same openings: + 2^log_n, + 2^32."""
    pk = select(index_batch(max_index).pk, [0] * 5)
    names = ["intact"]
    for b, (q, add) in enumerate(((0, 1 << 6), (3, 1 << 6), (1, 1 << 32), (2, (1 << 32) + (1 << 6))), 1):
        pk.indices[b, q] += np.uint64(add)
        names.append("index[%d] + %d" % (q, add))
    return Batch(pk, names)


# ---- (f) query counts -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def no_query_batch():
    msgs, nl = vc.fri_case(71, 64, 6, 0, 63)
    cls = vc.message_classes(6, nl, 0, 0)
    batch = [list(msgs), vc.flip(list(msgs), cls.index("beta"))]
    return Batch(fri_amd.pack_transcripts(batch, 6, [nl] * 2, 0, 63), ["honest", "beta flipped"])


@functools.lru_cache(maxsize=None)
def max_query_batch():
    Q = fri_amd.VERIFY_MAX_QUERIES
    msgs, nl = vc.fri_case(15, 8, 3, Q, 7)
    assert nl == 4                                   # the last layer has one element
    pk = select(fri_amd.pack_transcripts([list(msgs)], 3, [nl], Q, 7), [0, 0])
    pk.paths[1, Q - 1, 40] ^= 1                      # a path byte of the last query's record
    return Batch(pk, ["honest", "last query's path"])


# ---- (g) ragged waves and chunks --------------------------------------------
RAGGED_MEMBERS = 203


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """FRI-only at log_n = 6, n_layers cycling through a shuffled 1..7, the
    channel states mixed, every 5th member a forgery in rotation."""
    rng = random.Random(2024)
    order = []
    while len(order) < RAGGED_MEMBERS:
        seven = list(range(1, 8))
        rng.shuffle(seven)
        order += seven
    forge = 0
    batch, nls, states, names = [], [], [], []
    for b in range(RAGGED_MEMBERS):
        want_nl, st = order[b], ("", S1, S2)[b % 3]
        d = COEFFS_OF_LAYERS[want_nl]
        if b % 5 != 4:
            msgs, nl = vc.fri_case(1000 + b, d, 6, 2, 63, st)
            msgs, name = list(msgs), "honest"
        else:
            kind = forge % 9
            forge += 1
            if kind < 6:                             # a flipped message of one class, as in (a)
                msgs, nl = vc.fri_case(1000 + b, d, 6, 2, 63, st)
                cls = vc.message_classes(6, nl, 2, 0)
                want = ("root", "beta", "final", "index", "value", "path")[kind]
                at = [i for i, c in enumerate(cls) if c == want and msgs[i]]
                if not at:                           # one layer: no beta; its neighbour in the rotation
                    at = [i for i, c in enumerate(cls) if c == "final"]
                i = at[b % len(at)]
                msgs, name = vc.flip(list(msgs), i), "flip %s@%d" % (cls[i], i)
            else:                                    # a layer or the final value forged, as in (b)
                k = b % want_nl
                kw = (dict(tweak=vc.bump_layer(k)), dict(tweak=vc.bump_layer(k, True)), dict(final_delta=1))[kind - 6]
                msgs, nl = vc.forged_fri(1000 + b, d, 6, 2, 63, st, **kw)
                name = ("layer%d" % k, "high%d" % k, "final+1")[kind - 6]
        assert nl == want_nl
        batch.append(msgs)
        nls.append(nl)
        states.append(st)
        names.append("%s nl=%d" % (name, nl))
    return Batch(fri_amd.pack_transcripts(batch, 6, nls, 2, 63, channel_states=states), names, batch, nls)


# ---- (h) words >= p ---------------------------------------------------------
def malformed_batch():
    """An accepted (4, 2, 2) record and copies with one word set to p or to
    2^32 - 1, one per position class: (Batch, the mutated members)."""
    msgs, a_last, nl = vc.fibsq_case(99, 4, 2, 2)
    one = pack_fibsq([list(msgs)], [a_last], [nl], (4, 2, 2))
    ML = one.shape.max_layers
    assert nl == ML and nl >= 3
    spots = [("alpha%d" % j, "head", (8 + j,)) for j in range(3)]
    spots += [("beta%d" % k, "head", (11 + 8 * ML + k,)) for k in (0, nl - 2)]
    spots += [("final", "head", (11 + 9 * ML - 1,))]
    spots += [("trace value %d" % j, "values", (1, j)) for j in range(3)]
    spots += [("layer 0's value", "values", (0, 3)), ("layer 2's value", "values", (1, 3 + 4)),
              ("layer 1's sibling", "values", (0, 3 + 3)), ("last layer's sibling", "values", (1, 3 + 2 * nl - 1))]
    members = [(name, arr, at, word) for name, arr, at in spots for word in (P, (1 << 32) - 1)]
    pk = select(one, [0] * (2 + len(members)))
    names, bad = ["intact"], []
    for b, (name, arr, at, word) in enumerate(members, 1):
        getattr(pk, arr)[(b,) + at] = word
        names.append("%s = %d" % (name, word))
        bad.append(b)
    names.append("intact")
    return Batch(pk, names), bad


def spare_beta_batch():
    """The mixed FRI batch with p in every beta slot past n_layers - 1: not
    read, the members stay accepted."""
    cases = [vc.fri_case(7 + d, d, 6, 2, 63) for d in MIXED]
    pk = fri_amd.pack_transcripts([list(c[0]) for c in cases], 6, [c[1] for c in cases], 2, 63)
    ML = pk.shape.max_layers
    for b, nl in enumerate(pk.n_layers):
        pk.head[b, 8 * ML + int(nl) - 1:9 * ML - 1] = P
    return Batch(pk, ["coeffs%d" % d for d in MIXED])


# ---- all of it, for the host test that anchors the model --------------------
def model_batches():
    """(name, Batch) of every batch the device tests hand to the model."""
    yield "flipped (4,2,2)", flipped_fibsq((4, 2, 2))
    yield "flipped (2,1,1)", flipped_fibsq((2, 1, 1))
    yield "flipped FRI mixed", flipped_fri_mixed()
    yield "halves (4,2,4)", halves_batch((4, 2, 4))
    yield "halves (5,3,4)", halves_batch((5, 3, 4))
    yield "path words", path_word_batch()
    yield "layers (4,2,3)", layers_batch((4, 2, 3))
    yield "layers (2,1,2)", layers_batch((2, 1, 2))
    yield "layers (2,1,2) degree T", layers_batch((2, 1, 2), 3)
    yield "composition", composition_batch()
    for kind, off in OFFSETS:
        own = offset_batch(kind, off)
        yield "%s offset %d" % (kind, off), own
        yield "%s offset %d under 5" % (kind, off), Batch(with_shape(own.pk, offset=5), own.names)
    for mi in MAX_INDICES:
        yield "max_index %d" % mi, index_batch(mi)
    top = index_batch((1 << 32) - 1)
    yield "max_index 2^32-1 under 2^32-2", Batch(with_shape(top.pk, max_index=(1 << 32) - 2), top.names)
    yield "index aliases, 63", index_alias_batch(63)
    yield "index aliases, 2^32-1", index_alias_batch((1 << 32) - 1)
    yield "no queries", no_query_batch()
    yield "max queries", max_query_batch()
    yield "ragged", ragged_batch()
