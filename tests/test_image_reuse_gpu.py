"""GPU: an image encoded once -- SPILlavaLlamaModel.encode_image / features_of / embed_window, generate(images=EncodedImage,
share_images=True), GenerationSession(cache_image=True), ConversationBot.run / run_batch on top of them.

The mini models of tests/test_session_gpu.py and tests/test_shared_prefix_gpu.py (image 112: P = 8, 64 patch tokens; ViT and
region module 512 wide, 2-layer decoder 512 wide, 4 heads x 128), 2 to 3 boxes per row, fp16 and bf16.
  * Everything the new path copies (text rows, patch rows) and everything it computes with the launches of the existing
    path at the same shapes (batch 1: tower, fuse, region head on the same boxes) is compared with `torch.equal`.
  * Region rows computed at ANOTHER row count than the row served alone (the boxes of several rows through one region-head
    call) may route their GEMMs differently, so no tolerance is fixed in advance: both paths are measured against the fp32
    restatement of the region module (oracle/spi_oracle.py, emulate=False, on the tower's own 16-bit level features), in
    max-norm over the region rows, and the shared path may be at most 1.25 x as far from it as the rows served alone --
    the margin tests/test_train_gpu.py gives this kind of comparison.  Both errors are printed."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import spi_oracle as S  # noqa: E402  (the checker; never the product path)

if torch.cuda.is_available():
    from gpt4roi_amd import synthetic as syn
    from gpt4roi_amd.generation import GenerationSession
    from gpt4roi_amd.llama import LlamaDecoder
    from gpt4roi_amd.spi_llava import EncodedImage, SPILlavaLlamaModel, SPILlavaMPTForCausalLM
    from gpt4roi_amd.vit import ClipVisionTower

DEV = "cuda"
HID, HEADS, INTER, LAYERS = 512, 4, 1408, 2
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
PROJ_SEED = 4
BOX = [[0.05, 0.1, 0.55, 0.85], [0.25, 0.03, 0.97, 0.66], [0.01, 0.02, 0.3, 0.45], [0.4, 0.5, 0.9, 0.95],
       [0.15, 0.2, 0.35, 0.7], [0.6, 0.05, 0.8, 0.4], [0.3, 0.3, 0.7, 0.6]]


def _mini_lm(dtype):
    ids = syn.token_ids(vocab_base=990)
    tower = ClipVisionTower(syn.vit_state(HID, 4 * HID, 12, 112, seed=8), heads=8, device=DEV, dtype=dtype)
    dec = LlamaDecoder(syn.llama_state(HID, INTER, LAYERS, ids.vocab, seed=9), heads=HEADS, max_positions=512, device=DEV,
                       dtype=dtype)
    model = SPILlavaLlamaModel(tower, dec, ids, embed_dims=HID)
    model.spi_module.load_state_dict(syn.spi_state(model.spi_module, 3))
    # the projector from a seeded generator: nn.Linear's default draws from torch's GLOBAL generator, whose state depends on
    # every test that ran before in the process -- the ids of a near-tied draw would then differ between a run of this file
    # alone and a run of the whole suite
    g = torch.Generator().manual_seed(PROJ_SEED)
    with torch.no_grad():
        pj = model.mm_projector
        pj.weight.copy_(torch.randn(pj.weight.shape, generator=g) / pj.weight.size(1) ** 0.5)
        pj.bias.copy_(torch.randn(pj.bias.shape, generator=g) * 0.05)
    return SPILlavaMPTForCausalLM(model), ids


def _image(seed, dtype):
    return torch.randn(1, 3, 112, 112, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _boxes(*which):
    return torch.tensor([BOX[i] for i in which], device=DEV)


def _head(ids):
    return [1, 20, 21, ids.im_start_token] + [ids.im_patch_token] * 64 + [ids.im_end_token, 22, 23]


class _Counters:
    """Counts the vision tower, the fuse rounds and the region head of a model, with the batch / RoI count of every call."""

    def __init__(self, model):
        self.tower, self.fuse, self.head = [], [], []
        tower, spi = model.vision_tower[0], model.spi_module
        t_fwd, f_fwd, r_fwd = tower.forward, spi.mlvl_fuse.forward, spi.roi_align.forward

        def tower_forward(images):
            self.tower.append(int(images.size(0)))
            return t_fwd(images)

        def fuse_forward(tokens, P, sizes):
            self.fuse.append(int(tokens[0].size(0)))
            return f_fwd(tokens, P, sizes)

        def head_forward(feats, rois, *a, **kw):
            self.head.append(int(rois.n) if hasattr(rois, "n") else sum(int(r.size(0)) for r in rois))
            return r_fwd(feats, rois, *a, **kw)
        tower.forward, spi.mlvl_fuse.forward, spi.roi_align.forward = tower_forward, fuse_forward, head_forward

    def take(self):
        got = (self.tower, self.fuse, self.head)
        self.tower, self.fuse, self.head = [], [], []
        return got


# ---- a. batch 1: the encoded path IS the existing one --------------------------------------------------------------------
@DTYPES
def test_batch_one_window_over_the_whole_prompt_equals_embed_inputs(dtype):
    lm, ids = _mini_lm(dtype)
    model = lm.model
    x, boxes = _image(6, dtype), [_boxes(0, 1, 2)]
    prompt = torch.tensor([_head(ids) + [ids.bbox_token, 24, 25, ids.bbox_token, 26, ids.bbox_token, 5]], device=DEV)
    with torch.no_grad():
        enc = model.encode_image(x[0])
        assert isinstance(enc, EncodedImage) and enc.P == 8 and enc.image_size == 112 and enc.dtype == dtype
        assert enc.tokens.shape == (64, HID) and [m.size(1) for m in enc.maps] == [64, 32, 16, 8]
        assert torch.equal(enc.pixels, x[0]) and enc.pixels.data_ptr() != x.data_ptr()
        assert enc.nbytes() >= 85 * 64 * HID * 2 + 64 * HID * 2
        assert model.encode_image(enc) is enc
        window = model.embed_window(prompt, enc, bboxes=boxes)
        st_window = model.last_status.clone()
        full = model.embed_inputs(prompt, x, boxes)
        assert window.shape == full.shape and torch.equal(window, full)           # the same launches at the same shapes
        assert torch.equal(st_window, model.last_status) and not st_window.any()
        assert torch.equal(model.embed_inputs(prompt, enc, boxes), full)          # embed_inputs takes the encoding too
        assert torch.equal(model.encode_image(x).tokens, enc.tokens)              # [1, 3, S, S] is the same image
    kw = dict(bboxes=boxes, do_sample=False, max_new_tokens=5, eos_token_id=-1)
    assert torch.equal(lm.generate(prompt, images=enc, **kw), lm.generate(prompt, images=x, **kw))
    assert enc.encodes == 1
    with pytest.raises(ValueError):                                               # a <bbox> of the window without features
        with torch.no_grad():
            model.embed_window(prompt, enc, bboxes=boxes, lo=0, hi=prompt.size(1), region_from=[1])
        model.check_status()
    assert model.last_status.tolist() == [32]


# ---- b. / c. four rows on one image --------------------------------------------------------------------------------------
def _four_rows(ids):
    """Four questions about one image: a common head up to and including the first `<bbox>` (one shared box), then different
    suffixes with 1 to 2 more boxes each.  -> (right-padded ids, mask, boxes per row, lengths)"""
    head = _head(ids) + [ids.bbox_token, 24]
    tails = [[25, ids.bbox_token, 26, 5], [30, 31, ids.bbox_token, 32, ids.bbox_token, 5], [40, ids.bbox_token, 41, 42, 5],
             [50, 51, 52, ids.bbox_token, 53, ids.bbox_token, 5]]
    boxes = [_boxes(0, 1), _boxes(0, 2, 3), _boxes(0, 4), _boxes(0, 5, 6)]
    rows = [head + t for t in tails]
    T = max(len(r) for r in rows)
    input_ids = torch.tensor([r + [0] * (T - len(r)) for r in rows], device=DEV)
    mask = torch.tensor([[1] * len(r) + [0] * (T - len(r)) for r in rows], device=DEV)
    return input_ids, mask, boxes, [len(r) for r in rows], len(head)


@DTYPES
def test_four_rows_on_one_image_are_the_rows_served_alone(dtype):
    lm, ids = _mini_lm(dtype)
    model, dec = lm.model, lm.model.llama
    x = _image(6, dtype)
    input_ids, mask, boxes, lens, P_want = _four_rows(ids)
    B = 4
    seen = {}
    decode = dec.decode_graph_batch

    def spy(inputs_embeds, *a, **kw):
        seen.update(suffix=inputs_embeds.clone(), prefix=kw["prefix_embeds"].clone(), P=kw["shared_prefix"])
        return decode(inputs_embeds, *a, **kw)
    dec.decode_graph_batch = spy
    counters = _Counters(model)
    images = x.expand(B, -1, -1, -1)
    kw = dict(images=images, bboxes=boxes, attention_mask=mask, do_sample=False, max_new_tokens=2, eos_token_id=-1,
              shared_prefix=True)
    lm.generate(input_ids, share_images=True, **kw)
    model.check_status()
    P = seen["P"]
    assert P == P_want == lm.last_shared_prefix                                   # inside the prompt, behind the first box
    assert seen["prefix"].shape == (1, P, HID) and seen["suffix"].shape == (B, max(lens) - P, HID)
    # c. the vision tower and the fuse rounds ran once, at batch 1; the region head once for the prefix (row 0's boxes)
    # and once for the 6 boxes of the four suffixes
    assert counters.take() == ([1], [1], [2, 6])
    del dec.decode_graph_batch
    lm.generate(input_ids, **kw)                                                  # the parent's path: batch 4
    assert counters.take() == ([B], [B], [10])
    # b. every row against the row served alone
    with torch.no_grad():
        _, mlvl = model.vision_tower[0].select(model.vision_tower[0].forward(x))
        feats = [f.float().cpu() for f in mlvl]
        oracle = S.MLVLROIQueryOracle(embed_dims=HID, P=8)
        oracle.roi_align.updims = torch.nn.Linear(1024, HID)
        oracle.load_state_dict({k: v.detach().float().cpu() for k, v in model.spi_module.state_dict().items()})
        want = oracle(feats, [torch.cat(boxes).float().cpu()], emulate=False)[0]      # fp32, every box of every row, once
    e_shared = e_alone = 0.0
    n0 = 0
    for b in range(B):
        n = lens[b]
        with torch.no_grad():
            alone = model.embed_inputs(input_ids[b:b + 1, :n].contiguous(), x, [boxes[b]])[0]
        got = torch.cat([seen["prefix"][0], seen["suffix"][b, :n - P]], 0)
        assert not seen["suffix"][b, n - P:].any()                                # zeros behind the row's window
        region = input_ids[b, :n] == ids.bbox_token
        assert int(region.sum()) == boxes[b].size(0)
        assert torch.equal(got[~region], alone[~region]), b                       # text and patch rows: copies of the same rows
        ref = want[n0:n0 + boxes[b].size(0)].to(DEV)
        n0 += boxes[b].size(0)
        e_shared = max(e_shared, float((got[region].float() - ref).abs().max()))
        e_alone = max(e_alone, float((alone[region].float() - ref).abs().max()))
    print(f"region rows vs the fp32 restatement, {dtype}: shared path {e_shared:.4e}, rows served alone {e_alone:.4e}")
    assert e_shared <= 1.25 * e_alone, (e_shared, e_alone)


# ---- c. sessions -----------------------------------------------------------------------------------------------------------
@DTYPES
def test_session_with_a_cached_image_runs_no_vision_on_a_follow_up(dtype):
    lm, ids = _mini_lm(dtype)
    model = lm.model
    x = _image(6, dtype)
    two, three = _boxes(0, 1), _boxes(0, 1, 2)
    first = _head(ids) + [ids.bbox_token, 24, 25, ids.bbox_token, 26, 5]
    windows = []
    embed_window = model.embed_window

    def spy(*a, **kw):
        out = embed_window(*a, **kw)
        windows.append(tuple(out.shape))
        return out
    model.embed_window = spy
    counters = _Counters(model)
    kw = dict(images=x, do_sample=False, max_new_tokens=6, return_new_tokens=True, eos_token_id=-1)

    def conversation(session):
        p1 = torch.tensor([first], device=DEV)
        new1 = lm.generate(p1, bboxes=[two], session=session, **kw)
        assert all(t < ids.im_patch_token for t in new1), new1
        p2 = torch.tensor([first + new1 + [5, 27, 28, 29, 5]], device=DEV)                 # a follow-up without a box
        c1 = counters.take()
        new2 = lm.generate(p2, bboxes=[two], session=session, **kw)
        stats2 = (session.reused, session.prefilled)
        c2 = counters.take()
        assert all(t < ids.im_patch_token for t in new2), new2
        p3 = torch.tensor([p2[0].tolist() + new2 + [5, 33, ids.bbox_token, 34, 5]], device=DEV)     # one that adds a box
        new3 = lm.generate(p3, bboxes=[three], session=session, **kw)
        return (new1, new2, new3), (c1, c2, counters.take()), stats2, (session.reused, session.prefilled), (p1, p2, p3)

    plain_ids, plain_counts, plain2, plain3, _ = conversation(GenerationSession())
    assert plain_counts == (([1], [1], [2]),) * 2 + (([1], [1], [3]),) and windows == []
    session = GenerationSession(cache_image=True)
    got_ids, counts, stats2, stats3, (p1, p2, p3) = conversation(session)
    assert isinstance(session.image, EncodedImage) and session.image.encodes == 1
    assert counts[0] == ([1], [1], [2])                                           # turn one encodes the picture
    assert counts[1] == ([], [], [])                                              # turn two: no ViT, no fuse, no region head
    assert counts[2] == ([], [], [1])                                             # turn three: the region head, for the new box only
    assert stats2 == plain2 and stats3 == plain3 and stats2[0] == len(first) + 5
    L2, L3 = stats2[0], stats3[0]
    assert windows == [(1, p1.size(1), HID), (1, p2.size(1) - L2, HID), (1, p3.size(1) - L3, HID)]      # W = T - L
    # turns one and two feed the decoder the rows the plain session feeds it (copies; turn one's boxes at the same count)
    assert got_ids[:2] == plain_ids[:2]
    # another picture: the entry is replaced, nothing of the cache is trusted
    lm.generate(p2, bboxes=[two], session=session, **dict(kw, images=_image(7, dtype)))
    assert counters.take() == ([1], [1], [2]) and session.reused == 0 and session.image.encodes == 1
    assert torch.equal(session.image.pixels, _image(7, dtype)[0])


# ---- d. the bot --------------------------------------------------------------------------------------------------------------
class _BotTok:
    """The word-level stub tokenizer of the serve tests (tests/test_session_gpu.py)."""

    def __init__(self, ids, model_max_length=2048):
        self.special = {"<im_patch>": ids.im_patch_token, "<bbox>": ids.bbox_token, "<point>": ids.point_token,
                        "<im_start>": ids.im_start_token, "<im_end>": ids.im_end_token}
        self.vocab = {"<pad>": 0, "<s>": 1, "###": 5}
        self.pad_token_id, self.model_max_length = 0, model_max_length

    def _ids(self, text):
        import re
        out = []
        for piece in re.split("(" + "|".join(re.escape(t) for t in self.special) + ")", text):
            if piece in self.special:
                out.append(self.special[piece])
            else:
                out += [self.vocab.setdefault(w, 10 + len(self.vocab)) for w in piece.split()]
        return out

    def __call__(self, text, return_tensors=None, padding=None, max_length=None, truncation=None):
        from types import SimpleNamespace
        if return_tensors is None:
            return SimpleNamespace(input_ids=self._ids(text))
        rows = [[1] + self._ids(t) for t in ([text] if isinstance(text, str) else text)]
        n = max(len(r) for r in rows)
        return SimpleNamespace(input_ids=torch.tensor([r + [0] * (n - len(r)) for r in rows], dtype=torch.int64))

    def batch_decode(self, ids, skip_special_tokens=True):
        inv = {v: k for k, v in self.vocab.items()}
        return [" ".join(inv.get(t, f"t{t}") for t in row if not (skip_special_tokens and t in self.special.values()))
                for row in ids.tolist()]


def _pictures(n):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 256, (300, 400, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(n)]


@DTYPES
def test_bot_turns_with_a_cached_image_answer_as_without_a_session(dtype):
    """The four turns of tests/test_session_gpu.py::test_bot_turns_with_a_session_answer_as_without: same image, a box added,
    another image."""
    from gpt4roi_amd.serve import ConversationBot
    lm, ids = _mini_lm(dtype)
    picture, other_picture = _pictures(2)
    two, three = [[20, 30, 220, 260], [100, 10, 390, 200]], [[20, 30, 220, 260], [100, 10, 390, 200], [5, 5, 120, 140]]
    turns = [("What is <region1> doing next to <region2> ?", picture, two),
             ("And what colour is <region2> ?", picture, []),
             ("Is <region3> behind <region1> ?", picture, three),
             ("What else is there ?", other_picture, [])]
    counters = _Counters(lm.model)

    def converse(session):
        bot, hist, answers, stats, counts = ConversationBot(lm, _BotTok(ids), image_size=112), [], [], [], []
        for text, pic, boxes in turns:
            ans, err, hist = bot.run(text, {"image": pic, "boxes": boxes}, hist, do_sample=False, max_new_tokens=8,
                                     session=session)
            assert err is None, err
            answers.append(ans)
            counts.append(counters.take())
            if session is not None:
                stats.append((session.reused, session.prefilled))
            if len(answers) == 3:
                third = copy.deepcopy(hist)
        return answers, third, hist, stats, counts

    plain_answers, plain_third, plain_hist, _, _ = converse(None)
    _, _, _, session_stats, _ = converse(GenerationSession())
    answers, third, hist, stats, counts = converse(GenerationSession(cache_image=True))
    print("answers:", answers, "(reused, prefilled) per turn:", stats, "tower / fuse / head calls per turn:", counts)
    assert answers == plain_answers

    def same_history(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x["sources"] == y["sources"] and x["region_name_set"] == y["region_name_set"]
            assert torch.equal(x["bboxes"], y["bboxes"])
    same_history(third, plain_third)
    same_history(hist, plain_hist)
    assert stats == session_stats and stats[1][0] > 0 and stats[3][0] == 0
    assert [c[:2] for c in counts] == [([1], [1]), ([], []), ([], []), ([1], [1])]     # the ViT runs for a new picture only
    assert counts[1][2] == []                                                          # turn two adds no box


@DTYPES
def test_bot_sampled_turn_draws_the_same_ids_with_a_cached_image(dtype):
    """ConversationBot.run(do_sample=True, seed=...) three times: without a session, with a plain session, with a
    cache_image=True session.
      * cached against the plain session is equal BY CONSTRUCTION, and asserted bit for bit at every link: the decoder is
        handed the same rows at the same positions (turn one: the launches of embed_inputs at the same shapes; turn two: a
        window of copied embedding rows), so its logits, the drawn ids and the recorded uniforms are the same numbers.
      * against the run without a session the ids and uniforms are those of tests/test_session_gpu.py::
        test_bot_sampled_turn_draws_the_same_ids_with_a_session (same picture, turns and seeds): a continued prefill agrees
        with a fresh one within 16-bit rounding, not bit for bit, and these seeds draw the same ids on both; that is the
        parent's property of a session, which a cached image inherits through the first point."""
    from gpt4roi_amd.serve import ConversationBot
    lm, ids = _mini_lm(dtype)
    picture = _pictures(1)[0]
    turns = [("What is <region1> doing next to <region2> ?", [[20, 30, 220, 260], [100, 10, 390, 200]], 31),
             ("And what colour is <region2> ?", [], 77)]
    dec = lm.model.llama
    ids_seen, fed = [], []
    generate, decode_graph = lm.generate, dec.decode_graph

    def recording_generate(input_ids, *a, **kw):
        out = generate(input_ids, *a, **kw)
        ids_seen.append(out[0, input_ids.size(1):].tolist())
        return out

    def recording_decode(inputs_embeds, *a, past_len=0, embeds_from=0, **kw):
        # what the decoder prefills: the rows behind past_len, wherever the caller's block starts
        fed.append((int(past_len), inputs_embeds[:, past_len - embeds_from:].clone()))
        return decode_graph(inputs_embeds, *a, past_len=past_len, embeds_from=embeds_from, **kw)
    lm.generate, dec.decode_graph = recording_generate, recording_decode

    def converse(session):
        del ids_seen[:], fed[:]
        bot, hist, answers, us = ConversationBot(lm, _BotTok(ids), image_size=112), [], [], []
        for text, boxes, seed in turns:
            ans, err, hist = bot.run(text, {"image": picture, "boxes": boxes}, hist, do_sample=True, temperature=0.2,
                                     max_new_tokens=8, seed=seed, session=session)
            assert err is None, err
            answers.append(ans)
            us.append(dec._dstate["u"][:len(ids_seen[-1])].cpu().clone())
        return answers, us, [list(r) for r in ids_seen], list(fed)

    none_answers, none_u, none_ids, _ = converse(None)
    plain = GenerationSession()
    plain_answers, plain_u, plain_ids, plain_fed = converse(plain)
    session = GenerationSession(cache_image=True)
    answers, us, got_ids, got_fed = converse(session)
    print("sampled answers:", answers, "plain session:", plain_answers, "no session:", none_answers, "reused", session.reused,
          "prefilled", session.prefilled)
    assert session.reused > 0 and isinstance(session.image, EncodedImage)
    assert (session.reused, session.prefilled) == (plain.reused, plain.prefilled)
    # the same rows into the decoder at the same cache length, hence the same ids and uniforms: bit for bit
    assert [L for L, _ in got_fed] == [L for L, _ in plain_fed] and got_fed[1][0] == session.reused
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(got_fed, plain_fed))
    assert got_ids == plain_ids and answers == plain_answers
    assert all(torch.equal(a, b) for a, b in zip(us, plain_u))
    # and those of a run without a session
    assert answers == none_answers and got_ids == none_ids
    assert all(torch.equal(a, b) for a, b in zip(us, none_u))


# ---- e. shared batches and n-best ----------------------------------------------------------------------------------------
def test_bot_run_batch_with_shared_images_answers_as_each_conversation_alone():
    """Three conversations about one picture and one about another (so P = 0: the rows share nothing but still decode
    together, as in tests/test_shared_prefix_gpu.py): greedy answers of run_batch(share_prefix=True, share_images=True) equal
    each conversation's run().  The questions and boxes were chosen so that the existing path, run_batch(share_prefix=True)
    without share_images, already equals run() for all four (asserted first: it is the premise, not the claim)."""
    from gpt4roi_amd.serve import ConversationBot
    lm, ids = _mini_lm(torch.bfloat16)
    bot = ConversationBot(lm, _BotTok(ids), image_size=112)
    pics = _pictures(2)
    images = [{"image": pics[0], "boxes": [[20, 30, 220, 260], [100, 10, 390, 200]]},
              {"image": pics[0], "boxes": [[5, 5, 120, 140], [60, 80, 300, 280]]},
              {"image": pics[1], "boxes": [[0, 0, 200, 150], [50, 60, 380, 290]]},
              {"image": pics[0], "boxes": [[150, 40, 390, 250], [10, 100, 180, 290], [200, 150, 320, 280]]}]
    texts = ["What is <region1> doing next to <region2> ?", "Which colour are <region1> and <region2> ?",
             "Where is <region1> sitting close to <region2> ?", "Is <region1> between <region2> and <region3> ?"]
    alone = [bot.run(t, im, [], do_sample=False, max_new_tokens=6)[0] for t, im in zip(texts, images)]
    counters = _Counters(lm.model)
    existing = [a for a, _, _ in bot.run_batch(texts, images, [[], [], [], []], do_sample=False, max_new_tokens=6,
                                               share_prefix=True)]
    assert counters.take()[:2] == ([4], [4])
    shared = bot.run_batch(texts, images, [[], [], [], []], do_sample=False, max_new_tokens=6, share_prefix=True,
                           share_images=True)
    assert all(e is None for _, e, _ in shared) and lm.last_shared_prefix == 0
    assert counters.take() == ([1, 1], [1, 1], [7, 2])              # two pictures, each once; the region head once per picture
    print("alone:", alone, "existing shared-prefix path:", existing, "with share_images:", [a for a, _, _ in shared])
    assert existing == alone, (alone, existing)                      # the premise: the existing shared-prefix path agrees
    assert [a for a, _, _ in shared] == alone, (shared, alone)
    with pytest.raises(ValueError):
        bot.run_batch(texts, images, [[], [], [], []], share_images=True)


def test_num_return_sequences_with_an_encoded_image_draws_the_same_rows():
    lm, ids = _mini_lm(torch.bfloat16)
    model, dec = lm.model, lm.model.llama
    x, boxes = _image(6, torch.bfloat16), [_boxes(0, 1)]
    prompt = torch.tensor([_head(ids) + [ids.bbox_token, 24, 25, ids.bbox_token, 26, 5]], device=DEV)
    n, N = 4, 8
    kw = dict(bboxes=boxes, do_sample=True, temperature=0.8, top_k=20, max_new_tokens=N, seed=4242, eos_token_id=-1,
              num_return_sequences=n, return_new_tokens=True)
    want = lm.generate(prompt, images=x, **kw)
    state = next(v for k, v in dec._bstate.items() if k[0] == n and k[1] == "shared" and k[-1] is True)
    want_u = state["u"][:, :N].clone()
    with torch.no_grad():
        enc = model.encode_image(x)
    counters = _Counters(model)
    got = lm.generate(prompt, images=enc, **kw)
    assert counters.take() == ([], [], [2])                         # no ViT, no fuse; the prompt's boxes once, not n times
    assert got == want and torch.equal(state["u"][:, :N], want_u) and lm.last_shared_prefix == prompt.size(1) - 1
    flagged = lm.generate(prompt, images=x, share_images=True, **kw)                  # pixels + the flag: encoded once
    assert counters.take() == ([1], [1], [2]) and flagged == want


# ---- f. staleness -----------------------------------------------------------------------------------------------------------
def test_a_written_weight_makes_the_encoding_stale_and_grad_mode_refuses_it():
    lm, ids = _mini_lm(torch.bfloat16)
    model = lm.model
    x = _image(6, torch.bfloat16)
    with torch.no_grad():
        enc = model.encode_image(x)
        old_maps = [m.clone() for m in enc.maps]
        assert model.features_of(enc)[0] is enc.tokens and enc.encodes == 1       # nothing moved: nothing is recomputed
        w = model.spi_module.mlvl_fuse.fuse_convs[2].conv.weight
        w[3, 5] *= 1.5                                                            # an in-place write, as an optimizer step makes
        tokens, maps, affs = model.features_of(enc)
        assert enc.encodes == 2
        fresh = model.encode_image(x)
        assert all(torch.equal(a, b) for a, b in zip(maps, fresh.maps)) and torch.equal(tokens, fresh.tokens)
        assert all(torch.equal(a, b) for a, b in zip(affs, fresh.affs))
        assert not all(torch.equal(a, b) for a, b in zip(maps, old_maps))         # and the write did change the pyramid
        model.mm_projector.bias.add_(0.25)                                        # the projector's stamp is watched too
        assert model.features_of(enc)[0] is not tokens and enc.encodes == 3
        assert torch.equal(enc.tokens, model.encode_image(x).tokens) and not torch.equal(enc.tokens, tokens)
    prompt = torch.tensor([_head(ids) + [24, 5]], device=DEV)
    assert any(p.requires_grad for p in model.spi_module.parameters())
    with torch.enable_grad():
        for call in (lambda: model.features_of(enc), lambda: model.embed_window(prompt, enc),
                     lambda: lm(input_ids=prompt, images=enc)):
            with pytest.raises(ValueError):
                call()
        for p in model.parameters():                                              # frozen weights: nothing wants a gradient
            p.requires_grad_(False)
        assert model.features_of(enc)[0] is enc.tokens
