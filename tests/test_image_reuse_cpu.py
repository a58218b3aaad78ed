"""CPU: the host side of image reuse -- generation.group_images, layers.PreparedBoxes(image_of_row=), the window plans of a
shared batch and of a session turn (generation.plan_windows / plan_shared_windows / plan_session_window), and the argument
checks of generate(images=EncodedImage..., share_images=), which must fail before the model is touched (the `_bare_lm`
pattern of tests/test_shared_prefix_cpu.py)."""
import pytest
import torch
import torch.nn as nn

from gpt4roi_amd.generation import (GenerationSession, SamplingConfig, group_images, plan_session_window,
                                    plan_shared_windows, plan_windows, same_pixels)
from gpt4roi_amd.layers import PreparedBoxes
from gpt4roi_amd.spi_llava import EncodedImage, SPILlavaMPTForCausalLM

BBOX, PATCH, START, END = 900, 901, 902, 903


def _enc(pixels, P=8):
    """An EncodedImage as encode_image leaves it, without the features (nothing here reads them)."""
    return EncodedImage(pixels=pixels.clone(), tokens=torch.zeros(P * P, 8), maps=[], affs=[], P=P, image_size=14 * P,
                        dtype=torch.bfloat16, tower=None, spi_stamp=(), proj_stamp=())


def _img(seed, S=28):
    return torch.randn(3, S, S, generator=torch.Generator().manual_seed(seed))


# ---- group_images ----------------------------------------------------------------------------------------------------
def test_group_images_keeps_the_order_of_first_appearance():
    a, b, c = _img(1), _img(2), _img(3)
    uniq, of_row = group_images([b, a, b.clone(), c, a.clone()])
    assert of_row == [0, 1, 0, 2, 1]
    assert len(uniq) == 3 and uniq[0] is b and uniq[1] is a and uniq[2] is c
    uniq, of_row = group_images(torch.stack([a, a, b, a]))                 # a [B, 3, S, S] tensor is its rows
    assert of_row == [0, 0, 1, 0] and len(uniq) == 2 and torch.equal(uniq[1], b)


def test_group_images_objects_against_tensors():
    a, b = _img(1), _img(2)
    ea, ea2, eb = _enc(a), _enc(a), _enc(b)
    assert group_images([ea, ea, eb])[1] == [0, 0, 1]                      # the same object is the same image
    uniq, of_row = group_images([ea, ea2])                                 # two encodings of equal pixels: one image
    assert of_row == [0, 0] and uniq == [ea]
    uniq, of_row = group_images([a, eb, ea, b])                            # a tensor row meets its encoding later:
    assert of_row == [0, 1, 0, 1] and uniq[0] is ea and uniq[1] is eb      # the group is served by the encoding
    uniq, of_row = group_images([ea, a[None], b])                          # [1, 3, S, S] pixels against the kept [3, S, S]
    assert of_row == [0, 0, 1] and uniq[0] is ea and uniq[1] is b
    assert not same_pixels(a, a.double()) and not same_pixels(a, _img(1, S=14)) and same_pixels(ea, a)


def test_group_images_batch_of_one_and_all_rows_distinct():
    a = _img(1)
    assert group_images([a]) == ([a], [0])
    e = _enc(a)
    assert group_images(e) == ([e], [0]) and group_images([e]) == ([e], [0])
    rows = [_img(s) for s in range(5)]
    uniq, of_row = group_images(rows)
    assert of_row == [0, 1, 2, 3, 4] and all(u is r for u, r in zip(uniq, rows))


def test_session_compares_an_encoding_by_its_pixels():
    a = _img(1)
    s = GenerationSession(cache_image=True)
    assert s.cache_image and not GenerationSession().cache_image
    s.image = _enc(a)
    assert s.same_image(a[None]) and s.same_image(s.image) and s.same_image(_enc(a))
    assert not s.same_image(_img(2)[None]) and not s.same_image(None)
    changed = a.clone()
    changed[0, 0, 0] += 1.0                                               # the encoding owns a copy: an in-place edit shows
    assert not s.same_image(changed)


# ---- PreparedBoxes(image_of_row=) ------------------------------------------------------------------------------------
def test_prepared_boxes_image_of_row():
    g = torch.Generator().manual_seed(0)
    boxes = [torch.rand(n, 4, generator=g) for n in (2, 0, 3, 1)]
    for dtype in (torch.bfloat16, torch.float16):
        plain = PreparedBoxes(boxes, 112, "cpu", dtype=dtype)
        same = PreparedBoxes(boxes, 112, "cpu", dtype=dtype, image_of_row=None)
        for name in ("rois5", "boxes_h16", "offsets"):                    # the default is today's table, exactly
            assert torch.equal(getattr(plain, name), getattr(same, name))
        assert plain.rois5[:, 0].tolist() == [0, 0, 2, 2, 2, 3] and plain.counts == same.counts == [2, 0, 3, 1]
        shared = PreparedBoxes(boxes, 112, "cpu", dtype=dtype, image_of_row=[0, 0, 1, 0])
        assert shared.rois5[:, 0].tolist() == [0, 0, 1, 1, 1, 0]          # the image of the row, not the row
        assert torch.equal(shared.rois5[:, 1:], plain.rois5[:, 1:]) and torch.equal(shared.boxes_h16, plain.boxes_h16)
        assert shared.counts == plain.counts and torch.equal(shared.offsets, plain.offsets) and shared.n == 6
        assert shared.offsets.tolist() == [0, 2, 2, 5, 6] and shared.num_imgs == 4
    for bad in ([0, 0, 1], [0, 0, 1, -1]):
        with pytest.raises(ValueError):
            PreparedBoxes(boxes, 112, "cpu", image_of_row=bad)


# ---- window plans ----------------------------------------------------------------------------------------------------
HEAD = [1, 20, START] + [PATCH] * 4 + [END, 21]                            # 9 positions, patch run at [3, 7)
ROW_A = HEAD + [BBOX, 30, BBOX, 31, 5]                                     # <bbox> at 9 and 11, 14 tokens
ROW_B = HEAD + [BBOX, 30, 40, 41, 42, BBOX, 5]                             # <bbox> at 9 and 14, 16 tokens
ROW_C = HEAD + [BBOX, 30, 50]                                              # <bbox> at 9, 12 tokens


def test_shared_window_plan_inside_the_patch_run():
    pre, suf = plan_shared_windows([ROW_A, ROW_B, ROW_C], 5, BBOX)
    assert (suf.lo, suf.hi, suf.W) == ([5, 5, 5], [14, 16, 12], 11)
    assert suf.region_from == suf.spi_skip == [0, 0, 0]                   # every box sits behind P: all go to the region head
    # the prefix holds no <bbox>: row 0's boxes are all "somebody else's", the region head does not run for it
    assert (pre.lo, pre.hi, pre.W) == ([0], [5], 5) and pre.region_from == pre.spi_skip == [2]


def test_shared_window_plan_right_after_a_bbox():
    pre, suf = plan_shared_windows([ROW_A, ROW_B, ROW_C], 10, BBOX)
    assert (suf.lo, suf.hi, suf.W) == ([10, 10, 10], [14, 16, 12], 6)
    assert suf.region_from == suf.spi_skip == [1, 1, 1]                   # box 0 belongs to the prefix
    assert (pre.lo, pre.hi) == ([0], [10]) and pre.region_from == pre.spi_skip == [0]      # it runs once, from row 0
    _, at = plan_shared_windows([ROW_A, ROW_B, ROW_C], 9, BBOX)           # P ON the <bbox>: it is the suffix's
    assert at.region_from == [0, 0, 0]


def test_shared_window_plan_with_an_empty_prefix():
    pre, suf = plan_shared_windows([ROW_A, ROW_C], 0, BBOX)
    assert (suf.lo, suf.hi, suf.W, suf.region_from, suf.spi_skip) == ([0, 0], [14, 12], 14, [0, 0], [0, 0])
    assert (pre.lo, pre.hi, pre.W) == ([0], [0], 1)                       # an empty window still has a stride of 1


def test_session_window_plan():
    T = len(ROW_B)
    last = plan_session_window(ROW_B, T - 1, BBOX)                        # L = T - 1: one position, both boxes behind it
    assert (last.lo, last.hi, last.W, last.region_from, last.spi_skip) == ([T - 1], [T], 1, [2], [2])
    mid = plan_session_window(ROW_B, 12, BBOX)                            # a follow-up that adds the second box
    assert (mid.lo, mid.hi, mid.W, mid.region_from) == ([12], [T], 4, [1])
    fresh = plan_session_window(ROW_B, 0, BBOX)                           # an empty session: the whole prompt
    assert (fresh.lo, fresh.hi, fresh.W, fresh.region_from) == ([0], [T], T, [0])


def test_window_plan_refuses_windows_outside_the_rows():
    for lo, hi in ((-1, 3), (5, 4), (0, 15), ([0, 0], [14, 13])):
        with pytest.raises(ValueError):
            plan_windows([ROW_A, ROW_C], lo, hi, BBOX)
    with pytest.raises(ValueError):
        plan_windows([ROW_A, ROW_C], [0], None, BBOX)
    per_row = plan_windows([ROW_A, ROW_C], [12, 3], [14, 3], BBOX)
    assert (per_row.W, per_row.region_from) == (2, [2, 0])


# ---- generate(): argument errors before the model is touched ---------------------------------------------------------
def _bare_lm():
    lm = SPILlavaMPTForCausalLM.__new__(SPILlavaMPTForCausalLM)
    nn.Module.__init__(lm)
    lm.config = type("Cfg", (), {})()
    lm.generation_config = SamplingConfig()
    return lm


IDS2 = torch.tensor([[1, 20, 21, 30, 31], [1, 20, 21, 40, 0]])
RIGHT = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 1, 0]])


@pytest.mark.parametrize("ids,kw", [
    (IDS2, dict(share_images=True, attention_mask=RIGHT)),                                   # no shared_prefix
    (IDS2, dict(share_images=True, shared_prefix=False, attention_mask=RIGHT)),
    (IDS2[:1], dict(share_images=True)),                                                     # batch 1, one sample
    (IDS2, dict(shared_prefix=True, attention_mask=RIGHT, images=[_enc(_img(1))])),          # one encoding, two rows
    (IDS2, dict(shared_prefix=True, attention_mask=RIGHT, images=[_enc(_img(1))] * 3)),
    (IDS2[:1], dict(images=[_enc(_img(1)), _enc(_img(2))])),                                 # two encodings, one row
    (IDS2, dict(shared_prefix=True, attention_mask=RIGHT,
                images=[_enc(_img(1), P=8), _enc(_img(2, S=56), P=4)])),                      # encoded at another size
    (IDS2, dict(shared_prefix=True, attention_mask=RIGHT, images=[_enc(_img(1), P=8), _img(2, S=56)])),
], ids=["no-shared-prefix", "shared-prefix-off", "batch-1", "short-list", "long-list", "list-for-one-row", "other-size",
        "other-size-tensor"])
def test_generate_validates_images_and_share_images_first(ids, kw):
    lm = _bare_lm()
    with pytest.raises(ValueError):
        lm.generate(ids, max_new_tokens=4, **kw)


def test_bot_refuses_share_images_without_share_prefix():
    from gpt4roi_amd.serve import ConversationBot
    bot = ConversationBot.__new__(ConversationBot)
    with pytest.raises(ValueError):
        bot.run_batch(["a"], [None], [[]], share_images=True)
