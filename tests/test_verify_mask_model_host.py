"""The verdict-mask model (verify_mask_model.py) anchored on the CPU: on every
transcript the device tests hand to it (verify_mask_corpus.py) its mask is 0
exactly when fri_amd.verify_fibsq / verify_fri accept the unpacked messages;
the masks of the known forgeries are pinned; and the coverage the device tests
rely on (both halves of every layer, an all-high case, every class alone) is
asserted here, so a seed that stops providing it fails without a device."""
import functools

import verify_batch_cases as vc
import verify_mask_corpus as mc
from verify_mask_model import expected_masks

P = vc.P
CH, TP, CO, FP, FO, FI = 1, 2, 4, 8, 16, 32


@functools.lru_cache(maxsize=None)
def corpus():
    return {name: (batch, [int(m) for m in expected_masks(batch.pk)]) for name, batch in mc.model_batches()}


def test_bits_are_the_headers():
    import fri_amd
    assert (CH, TP, CO, FP, FO, FI) == (fri_amd.VERIFY_CHANNEL, fri_amd.VERIFY_TRACE_PATH, fri_amd.VERIFY_COMPOSITION,
                                        fri_amd.VERIFY_FRI_PATH, fri_amd.VERIFY_FOLD, fri_amd.VERIFY_FINAL)


def test_model_accepts_exactly_what_the_host_verifiers_accept():
    seen = 0
    for name, (batch, masks) in corpus().items():
        device = batch.device
        for b, m in enumerate(masks):
            if device[b]:
                assert (m == 0) == mc.host_accepts(batch.pk, b), (name, batch.names[b], m)
                seen += 1
    assert seen > 500
    # the members the packer decides are rejected by the host verifiers, on their messages
    decided = 0
    for batch in (mc.flipped_fibsq((4, 2, 2)), mc.flipped_fibsq((2, 1, 1)), mc.flipped_fri_mixed(),
                  mc.ragged_batch()):
        for b in range(batch.pk.batch):
            if not batch.device[b]:
                assert not mc.host_accepts(batch.pk, b, batch.msgs[b], batch.nls[b]), batch.names[b]
                decided += 1
    assert decided


def by_class(name):
    batch, masks = corpus()[name]
    out = {}
    for b, (label, m) in enumerate(zip(batch.names, masks)):
        if batch.device[b]:
            cls = label.split("/")[1].split("@")[0] if "/" in label else "honest"
            out.setdefault(cls, set()).add(m)
    return out


TABLE = {"honest": {0}, "alpha": {CH | CO}, "beta": {CH | FO}, "final": {CH | FI}, "index": {CH},
         "trace_value": {6, 7}, "trace_path": {2, 3}, "value": {24, 25, 28, 29, 40, 41, 56, 57}, "path": {8, 9},
         "root": {CH | FP, CH | TP | FP, CH | TP}}


def test_masks_of_the_flipped_messages():
    got = by_class("flipped (4,2,2)")
    assert set(got) == set(TABLE)
    for cls, masks in got.items():
        assert masks == TABLE[cls] if cls != "root" else masks <= TABLE[cls], (cls, masks)
    for cls, masks in by_class("flipped (2,1,1)").items():
        assert masks <= TABLE[cls], (cls, masks)
    fri = by_class("flipped FRI mixed")
    assert fri["honest"] == {0} and fri["index"] == {CH} and fri["beta"] == {CH | FO}
    assert fri["final"] == {CH | FI} and fri["path"] <= {8, 9} and fri["root"] == {CH | FP}
    assert fri["value"] <= TABLE["value"] - {28, 29}          # no composition without a trace


def test_masks_of_the_forgeries():
    batch, masks = corpus()["layers (4,2,3)"]
    named = dict(zip(batch.names, masks))
    nl = int(batch.pk.n_layers[0])
    assert nl == 6
    assert named["layer0"] == FO | CO and named["layer5"] == FO | FI
    for k in range(1, nl - 1):
        assert named["layer%d" % k] == FO and named["high%d" % k] == FO
    assert named["final+1"] == FI and named["cp_seed"] == CO
    # a one-element last layer, reached by a forged polynomial of degree T
    batch, masks = corpus()["layers (2,1,2) degree T"]
    named = dict(zip(batch.names, masks))
    nl = int(batch.pk.n_layers[0])
    assert nl == 3 + 1
    for k in range(1, nl - 1):
        assert named["layer%d" % k] == FO | CO
    assert named["layer%d" % (nl - 1)] == named["high%d" % (nl - 1)] == FO | FI | CO
    assert named["final+1"] == FI | CO
    batch, masks = corpus()["layers (2,1,2)"]
    named = dict(zip(batch.names, masks))
    for k in range(1, int(batch.pk.n_layers[0]) - 1):
        assert named["layer%d" % k] == FO
    assert named["cp_seed"] == CO and named["final+1"] == FI


def test_masks_of_the_composition_forgeries():
    batch, masks = corpus()["composition"]
    named = dict(zip(batch.names, masks))
    assert named == {"honest": 0, "alphas(1,0,2)": CO, "alphas(0,2,1)": CO, "a_last+1 in layer 0": CO | FO,
                     "verified with a_last+1": CO}


def test_masks_under_another_offset():
    for kind, off in mc.OFFSETS:
        assert corpus()["%s offset %d" % (kind, off)][1] == [0, 0]
        want = FO | CO if kind == "fibsq" else FO
        assert corpus()["%s offset %d under 5" % (kind, off)][1] == [want, want]
    # the table's own case: made at 5, verified under 7
    batch, _ = corpus()["flipped (4,2,2)"]
    assert list(expected_masks(mc.with_shape(mc.select(batch.pk, [0]), offset=7))) == [FO | CO]


def test_masks_of_the_index_draw():
    for mi in mc.MAX_INDICES:
        batch, masks = corpus()["max_index %d" % mi]
        assert masks == [0]
        assert all(int(i) <= mi for i in batch.pk.indices[0])
    # the draws above 2^31 leave the layer size far behind
    assert max(int(i) for i in corpus()["max_index %d" % ((1 << 32) - 1)][0].pk.indices[0]) >= 1 << 31
    assert corpus()["max_index 2^32-1 under 2^32-2"][1] == [CH]
    for name in ("index aliases, 63", "index aliases, 2^32-1"):
        assert corpus()[name][1] == [0, CH, CH, CH, CH]


def test_masks_of_the_query_counts():
    assert corpus()["no queries"][1] == [0, CH]
    assert corpus()["max queries"][1] == [0, FP]              # no draw follows the last query's record


def halves(indices, log_n, n_layers):
    """Per layer with at least two elements: the set of halves (0 low, 1 high) the indices open."""
    return [{int(i) % (1 << (log_n - k)) >= (1 << (log_n - k - 1)) for i in indices}
            for k in range(n_layers) if log_n - k >= 1]


def test_both_halves_of_every_layer_are_opened():
    batch, masks = corpus()["halves (4,2,4)"]
    assert masks == [0, 0, 0]
    idx = [[int(i) for i in row] for row in batch.pk.indices]
    assert idx == [[42, 16, 30, 18], [39, 16, 41, 48], [13, 2, 33, 19]]
    for b in (1, 2):
        assert all(h == {False, True} for h in halves(idx[b], 6, int(batch.pk.n_layers[b])))
    batch, masks = corpus()["halves (5,3,4)"]
    assert masks == [0, 0, 0]
    top = [int(i) for i in batch.pk.indices[2]]
    assert top == [195, 202, 214, 224]
    assert halves(top, 8, int(batch.pk.n_layers[2]))[:2] == [{True}, {True}]


def test_every_class_alone():
    seen = {m for _, masks in corpus().values() for m in masks}
    for alone in (CH, CO, FO, FI, CH | TP, CH | FP, FP):
        assert alone in seen
    # a corrupted path changes every later draw; in the last query's layer paths no draw follows
    assert corpus()["path words"][1] == [0, CH | TP, FP, CH | FP]


def test_ragged_batch_is_ragged():
    batch, masks = corpus()["ragged"]
    nl = [int(k) for k in batch.pk.n_layers[batch.device]]
    assert set(nl) == set(range(1, 8))
    # every wave of 64 holds every layer count, and so does every chunk the device test sets
    for b0 in range(0, batch.pk.batch - 63, 64):
        assert set(int(k) for k in batch.pk.n_layers[b0:b0 + 64]) == set(range(1, 8))
    assert [m != 0 for m in masks] == [b % 5 == 4 or not batch.device[b] for b in range(batch.pk.batch)]
    assert {int(c[32]) for c in batch.pk.chan} == {0, 1}
    assert len({m for m in masks}) >= 8


def test_model_refuses_words_above_p():
    import pytest
    batch, bad = mc.malformed_batch()
    assert list(expected_masks(mc.select(batch.pk, [0, batch.pk.batch - 1]))) == [0, 0]
    for b in bad:
        with pytest.raises(ValueError):
            expected_masks(mc.select(batch.pk, [b]))
    assert list(expected_masks(mc.with_shape(mc.spare_beta_batch().pk))) == [0] * 5


def test_padding_is_not_part_of_the_record():
    batch, masks = corpus()["ragged"]
    rows = list(range(0, 40))
    assert [int(m) for m in expected_masks(mc.padded(mc.select(batch.pk, rows)))] == masks[:40]
