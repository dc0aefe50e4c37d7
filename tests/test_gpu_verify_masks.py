"""fri_verify_batch's verdict masks, exact: "Every check runs for every member:
verdict[b] is the OR of the failed classes" (fri_amd.h).  Every expectation is
verify_mask_model.expected_masks over the same packed arrays the device gets
(the model itself is anchored on verify_fibsq / verify_fri by
test_verify_mask_model_host.py, which also pins the coverage these batches
provide: both halves of every layer, every class alone, ragged waves).  A
kernel that skips a check accepts, or reports fewer bits; equality sees both."""
import numpy as np
import pytest

import verify_mask_corpus as mc
from verify_mask_model import expected_masks

pytestmark = pytest.mark.gpu

P = mc.P


def device_masks(ctx, pk):
    return [int(m) for m in ctx.verify_batch(*pk.abi_args())]


def check(ctx, batch, pk=None):
    """The device's masks of the batch = the model's, member for member."""
    pk = batch.pk if pk is None else pk
    got, want = device_masks(ctx, pk), [int(m) for m in expected_masks(pk)]
    assert got == want, [(n, g, w) for n, g, w in zip(batch.names, got, want) if g != w]
    return want


# ---- (a) every flipped message ----------------------------------------------
@pytest.mark.parametrize("which", ["(4,2,2)", "(2,1,1)", "FRI mixed"])
def test_every_flipped_message_exact(ctx, which):
    import fri_amd
    batch = {"(4,2,2)": lambda: mc.flipped_fibsq((4, 2, 2)), "(2,1,1)": lambda: mc.flipped_fibsq((2, 1, 1)),
             "FRI mixed": mc.flipped_fri_mixed}[which]()
    pk, device = batch.pk, batch.device
    want = check(ctx, batch)                      # the blank records of host-decided members included
    assert all((w == 0) == ("/" not in n) for n, w in zip(batch.names, want))     # exactly the intact ones accepted
    # the mirrors: the packer's own decisions where it made one, the device's masks elsewhere
    reasons = []
    sh = pk.shape
    if sh.trace_count:
        ok = fri_amd.verify_fibsq_batch(batch.msgs, [int(pk.a_last[0])] * pk.batch, sh.log_t, sh.log_blowup,
                                        sh.num_queries, batch.nls, ctx=ctx, reasons=reasons)
    else:
        ok = fri_amd.verify_fri_batch(batch.msgs, sh.log_n, batch.nls, sh.num_queries, sh.max_index, ctx=ctx,
                                      reasons=reasons)
    assert reasons == [w if d else fri_amd.VERIFY_MALFORMED for w, d in zip(want, device)]
    assert ok == [r == 0 for r in reasons]


@pytest.mark.parametrize("shape", [(4, 2, 4), (5, 3, 4)])
def test_both_halves_of_the_fold(ctx, shape):
    """Accepted transcripts whose indices open the low and the high half of
    every layer, and (5, 3, 4) the high half only at layers 0 and 1."""
    assert check(ctx, mc.halves_batch(shape)) == [0, 0, 0]


def test_corrupted_path_words(ctx):
    import fri_amd
    V = fri_amd
    assert check(ctx, mc.path_word_batch()) == [0, V.VERIFY_CHANNEL | V.VERIFY_TRACE_PATH, V.VERIFY_FRI_PATH,
                                                V.VERIFY_CHANNEL | V.VERIFY_FRI_PATH]


# ---- (b) one layer wrong at a time ------------------------------------------
@pytest.mark.parametrize("shape,cp_seed", [((4, 2, 3), None), ((2, 1, 2), None), ((2, 1, 2), 3)])
def test_one_layer_wrong_at_a_time(ctx, shape, cp_seed):
    import fri_amd
    V = fri_amd
    batch = mc.layers_batch(shape, cp_seed)
    got = dict(zip(batch.names, check(ctx, batch)))
    nl = int(batch.pk.n_layers[0])
    assert nl == {((4, 2, 3), None): 6, ((2, 1, 2), None): 3, ((2, 1, 2), 3): 4}[shape, cp_seed]
    comp = V.VERIFY_COMPOSITION if cp_seed is not None else 0       # the forged polynomial is not the composition
    for k in range(1, nl - 1):
        assert got["layer%d" % k] == V.VERIFY_FOLD | comp
    assert got["layer%d" % (nl - 1)] == V.VERIFY_FOLD | V.VERIFY_FINAL | comp
    assert got["final+1"] == V.VERIFY_FINAL | comp
    if cp_seed is None:
        assert got["layer0"] == V.VERIFY_FOLD | V.VERIFY_COMPOSITION and got["cp_seed"] == V.VERIFY_COMPOSITION


# ---- (c) the composition, term by term --------------------------------------
def test_composition_term_by_term(ctx):
    import fri_amd
    C, F = fri_amd.VERIFY_COMPOSITION, fri_amd.VERIFY_FOLD
    assert check(ctx, mc.composition_batch()) == [0, C, C, C | F, C]


# ---- (d) offsets ------------------------------------------------------------
@pytest.mark.parametrize("kind,offset", mc.OFFSETS)
def test_offsets(ctx, kind, offset):
    import fri_amd
    batch = mc.offset_batch(kind, offset)
    assert batch.pk.shape.offset == offset
    assert check(ctx, batch) == [0, 0]
    wrong = fri_amd.VERIFY_FOLD | (fri_amd.VERIFY_COMPOSITION if kind == "fibsq" else 0)
    assert check(ctx, batch, mc.with_shape(batch.pk, offset=5)) == [wrong, wrong]


# ---- (e) the index draw -----------------------------------------------------
def test_index_draw_ranges(ctx):
    import fri_amd
    for mi in mc.MAX_INDICES:
        assert check(ctx, mc.index_batch(mi)) == [0]
    top = mc.index_batch((1 << 32) - 1)
    assert check(ctx, top, mc.with_shape(top.pk, max_index=(1 << 32) - 2)) == [fri_amd.VERIFY_CHANNEL]
    verdict = np.full(1, 0xDEADBEEF, dtype=np.uint32)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.verify_batch(*mc.with_shape(top.pk, max_index=1 << 32).abi_args(), verdict=verdict)
    assert e.value.code == fri_amd.FRI_EINVAL and list(verdict) == [0xDEADBEEF]


@pytest.mark.parametrize("max_index", [63, (1 << 32) - 1])
def test_index_aliases(ctx, max_index):
    """A claimed index replaced by one that opens the same positions: the
    draw differs and nothing else does."""
    import fri_amd
    assert check(ctx, mc.index_alias_batch(max_index)) == [0] + [fri_amd.VERIFY_CHANNEL] * 4


# ---- (f) query counts -------------------------------------------------------
def test_no_queries(ctx):
    import fri_amd
    assert check(ctx, mc.no_query_batch()) == [0, fri_amd.VERIFY_CHANNEL]


def test_most_queries(ctx):
    import fri_amd
    batch = mc.max_query_batch()
    assert batch.pk.shape.num_queries == fri_amd.VERIFY_MAX_QUERIES
    assert check(ctx, batch) == [0, fri_amd.VERIFY_FRI_PATH]


# ---- (g) ragged waves and chunks --------------------------------------------
def test_ragged_waves_and_chunks(ctx):
    batch = mc.ragged_batch()
    assert batch.pk.batch == mc.RAGGED_MEMBERS > 3 * 64
    want = check(ctx, batch)
    assert len(set(want)) >= 8
    try:
        for chunk in (1, 64, 65, 199):
            ctx.set_verify_chunk(chunk)
            assert device_masks(ctx, batch.pk) == want, chunk
    finally:
        ctx.set_verify_chunk(0)


# ---- (h) strides, the one-stream path, words >= p ----------------------------
def test_padded_strides(ctx):
    batch = mc.ragged_batch()
    pk = mc.padded(batch.pk)
    assert pk.head.shape[1] == batch.pk.head.shape[1] + 3 and pk.values.shape[2] == batch.pk.values.shape[2] + 5
    assert pk.paths.shape[2] == batch.pk.paths.shape[2] + 7
    want = [int(m) for m in expected_masks(batch.pk)]
    assert device_masks(ctx, pk) == want
    try:
        ctx.set_verify_chunk(64)                       # rows of a later chunk start at a padded offset
        assert device_masks(ctx, pk) == want
    finally:
        ctx.set_verify_chunk(0)


def test_one_stream_path(ctx, monkeypatch):
    import fri_amd
    batch = mc.ragged_batch()
    want = [int(m) for m in expected_masks(batch.pk)]
    c = fri_amd.Context(0, 14)
    try:
        c.set_profiling(True)
        c.set_verify_chunk(64)
        c.reset_profile()
        assert device_masks(c, batch.pk) == want
        chunks = (batch.pk.batch + 63) // 64
        assert c.profile("verify_chain")[1] == chunks and c.profile("verify_open")[1] == chunks
    finally:
        c.close()
    monkeypatch.setenv("FRI_VERIFY_SERIAL", "1")
    assert device_masks(ctx, batch.pk) == want


def test_words_not_below_p(ctx):
    import fri_amd
    batch, bad = mc.malformed_batch()
    got = device_masks(ctx, batch.pk)
    for b, (name, g) in enumerate(zip(batch.names, got)):
        if b in bad:
            assert g & fri_amd.VERIFY_MALFORMED, (name, g)
        else:
            assert g == 0, (name, g)
    # beta slots past n_layers - 1 are not read
    assert device_masks(ctx, mc.spare_beta_batch().pk) == [0] * 5
