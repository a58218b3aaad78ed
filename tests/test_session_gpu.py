"""GPU: conversation sessions -- a follow-up turn prefills only what the KV cache does not hold (LlamaDecoder.rewind /
decode_graph(past_len=), generate(session=), ConversationBot.run(session=)).

Tiny seeded models from gpt4roi_amd/synthetic.py (2 decoder layers, hidden 512, 4 heads x 128), fp16 and bf16.  The yardstick
is the fp32 oracle (oracle/transformer_oracle.py) run on the decoder's own 16-bit weights and the same embeddings:
  * logits of a continued prefill may be at most 1.25 x as far from the oracle as those of a fresh full prefill of the
    same sequence (this project's margin for "no worse than"), and the two agree within the sum of their errors;
  * greedy ids with and without the session are equal on seeds whose oracle top-2 logit gap, at every generated step,
    exceeds ten times the fresh path's measured logit error (an argmax can then not flip inside the error bars).  The
    seeds were picked with the oracle on the CPU; at most one may fail the gap condition with the error measured here,
    at least three must run.
Geometries: a 75-token prompt in a 256-row cache and a 530-token prompt in a 1024-row cache, each with the chunk's attention
on the prefill forward and on the split-key kernel (kernels.flash_attn_cont), whatever the routing rule picks by default."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import transformer_oracle as TO  # noqa: E402  (the checker; never the product path)

if torch.cuda.is_available():
    from gpt4roi_amd import synthetic as syn
    from gpt4roi_amd.generation import GenerationSession
    from gpt4roi_amd.llama import LlamaDecoder
    from gpt4roi_amd.spi_llava import SPILlavaLlamaModel, SPILlavaMPTForCausalLM
    from gpt4roi_amd.vit import ClipVisionTower

DEV = "cuda"
HID, HEADS, INTER, LAYERS, VOCAB = 512, 4, 1408, 2, 1000
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
# picked with the oracle on the CPU out of seeds 0..219: the four largest minimum top-2 gaps of turn two (0.33-0.45
# with the bf16 weights; the oracle's own bf16-emulating mode puts the logit error near 0.018), turn one's gaps > 0.12
GREEDY_SEEDS = (39, 201, 213, 216)
N1, N2, T0, TAIL = 3, 3, 75, 13           # greedy-id test: tokens of turn one / two, first prompt, new question


def _decoder(dtype, max_positions=256, seed=9):
    sd = syn.llama_state(HID, INTER, LAYERS, VOCAB, seed=seed)
    dec = LlamaDecoder(sd, heads=HEADS, max_positions=max_positions, device=DEV, dtype=dtype)
    w = {k: v.to(dtype).float().to(DEV) for k, v in sd.items()}       # the oracle computes in fp32 on the 16-bit weights
    return dec, w


def _embeds(n, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, n, HID, generator=g).to(dtype).to(DEV)


def _oracle_logits(w, embeds):
    h, _ = TO.llama_forward(w, embeds.float(), HEADS)
    return TO.lm_logits(w, h)[0]


def _check_continued(dec, w, full, L, what):
    """Cache rows [0, L) are in place: the logits of prefilling full[:, L:] there vs a fresh prefill of `full`, vs fp32."""
    dec.rewind(L)
    cont = dec.forward(full[:, L:], all_logits=True)[0].clone()
    assert dec.pos == full.size(1) == dec.rows_held
    dec.reset(1)
    fresh = dec.forward(full, all_logits=True)[0, L:].clone()
    want = _oracle_logits(w, full)[L:]
    e_cont, e_fresh = float((cont - want).abs().max()), float((fresh - want).abs().max())
    between = float((cont - fresh).abs().max())
    print(f"{what}: continued err {e_cont:.3e}, fresh err {e_fresh:.3e}, continued vs fresh {between:.3e}")
    assert e_cont <= 1.25 * e_fresh, (what, e_cont, e_fresh)
    assert between <= e_cont + e_fresh, (what, between, e_cont, e_fresh)


@DTYPES
@pytest.mark.parametrize("route", ["forward", "split-key"])
@pytest.mark.parametrize("t0,max_positions", [(75, 256), (530, 1024)])
def test_continued_prefill_matches_a_fresh_one(t0, max_positions, route, dtype, monkeypatch):
    from gpt4roi_amd import kernels as K
    monkeypatch.setattr(K, "CONT_ATTN_ROUTE", "always" if route == "split-key" else "never")
    assert K.cont_attn_wins(19, t0 + 24, HEADS) == (route == "split-key")
    dec, w = _decoder(dtype, max_positions)
    first = _embeds(t0, 100 + t0, dtype)
    ids = dec.decode_graph(first, 6)
    assert len(ids) == 6 and dec.rows_held == t0 + 5                  # the sixth token was never fed back
    tok = torch.tensor(ids, device=DEV)
    chunk = torch.cat([dec.embed[tok[5:]], _embeds(18, 200 + t0, dtype)[0]], 0)          # 19 rows
    full = torch.cat([first[0], dec.embed[tok[:5]], chunk], 0)[None].contiguous()
    _check_continued(dec, w, full, t0 + 5, f"chunk of 19 behind {t0 + 5} rows")
    # rewind INSIDE the cache, as when the new prompt's ids leave the cached ones early (tokenisation divergence)
    dec.reset(1)
    dec.decode_graph(first, 6)
    L = t0 - 10
    other = torch.cat([first[0, :L], _embeds(30, 300 + t0, dtype)[0]], 0)[None].contiguous()
    _check_continued(dec, w, other, L, f"rewind to {L} of {t0 + 5} rows, chunk of 30")


def test_rewind_and_past_len_refuse_what_the_cache_does_not_hold():
    dec, _ = _decoder(torch.bfloat16)
    first = _embeds(40, 1, torch.bfloat16)
    dec.decode_graph(first, 4)
    assert dec.rows_held == 43
    with pytest.raises(ValueError):
        dec.rewind(44)
    with pytest.raises(ValueError):
        dec.decode_graph(first, 2, past_len=40)                      # nothing left to prefill
    dec.reset(1)
    assert dec.rows_held == 0
    with pytest.raises(ValueError):
        dec.decode_graph(first, 2, past_len=10)                      # an emptied cache holds no prefix
    mask = torch.ones(2, 12, dtype=torch.bool, device=DEV)
    mask[0, :3] = False
    dec.reset(2)
    dec.forward(_embeds(24, 2, torch.bfloat16).view(2, 12, HID), all_logits=False, key_padding_mask=mask)
    with pytest.raises(ValueError):
        dec.rewind(5)                                                 # a ragged layout does not continue


def _second_turn(dec, seed, dtype):
    """Turn one on a seeded prompt, then the embeddings of turn two: prompt + the tokens turn one fed back + a question."""
    first = _embeds(T0, 1000 + seed, dtype)
    ids1 = dec.decode_graph(first, N1)
    tok = torch.tensor(ids1, device=DEV)
    full = torch.cat([first[0], dec.embed[tok], _embeds(TAIL, 2000 + seed, dtype)[0]], 0)[None].contiguous()
    return first, full, T0 + N1 - 1


@DTYPES
def test_greedy_and_sampled_ids_are_the_same_with_and_without_the_cache_prefix(dtype):
    dec, w = _decoder(dtype)
    ran, dropped = [], []
    for seed in GREEDY_SEEDS:
        first, full, L = _second_turn(dec, seed, dtype)
        assert dec.rows_held == L
        with_prefix = dec.decode_graph(full, N2, past_len=L)
        # the yardstick: oracle ids and logits, and the fresh path's logit error along the oracle's own sequence
        ids_o, trace = TO.greedy_decode(w, full.float(), lambda t: dec.embed[t.to(DEV)].float(), HEADS, N2)
        gap = min(float((lambda s: s[0] - s[1])(torch.topk(lg, 2).values)) for lg in trace)
        dec.reset(1)
        lg = dec.forward(full, all_logits=False)
        err = 0.0
        for s in range(N2):
            err = max(err, float((lg.view(-1) - trace[s]).abs().max()))
            lg = dec.forward(dec.embed[torch.tensor([[ids_o[s]]], device=DEV)].view(1, 1, -1), all_logits=False)
        print(f"seed {seed} {dtype}: oracle min top-2 gap {gap:.4f}, fresh logit error {err:.4f}")
        if not gap > 10.0 * err:
            dropped.append(seed)
            continue
        fresh = dec.decode_graph(full, N2)
        assert with_prefix == fresh == ids_o, (seed, with_prefix, fresh, ids_o)
        if not ran:                                                   # sampling: the same Philox stream on either path
            sampler = (0.2, 50, 1.0)
            sampled_fresh = dec.decode_graph(full, N2, sampler=sampler, seed=77)
            _second_turn(dec, seed, dtype)
            sampled_with = dec.decode_graph(full, N2, sampler=sampler, seed=77, past_len=L)
            assert sampled_with == sampled_fresh, (seed, sampled_with, sampled_fresh)
        ran.append(seed)
    assert len(dropped) <= 1 and len(ran) >= 3, (ran, dropped)


# ---- bot level -----------------------------------------------------------------------------------------------------
class _BotTok:
    """The word-level stub tokenizer of the serve tests (tests/test_generation_gpu.py): HF batch call for prompt.py, plain
    call + batch_decode for KeywordsStoppingCriteria; special tokens carry the model's configured ids."""

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


def _mini_lm(dtype):
    image = 112
    ids = syn.token_ids(vocab_base=990)
    tower = ClipVisionTower(syn.vit_state(HID, 4 * HID, 12, image, seed=8), heads=8, device=DEV, dtype=dtype)
    dec = LlamaDecoder(syn.llama_state(HID, INTER, LAYERS, ids.vocab, seed=9), heads=HEADS, max_positions=512, device=DEV,
                       dtype=dtype)
    model = SPILlavaLlamaModel(tower, dec, ids, embed_dims=HID)
    model.spi_module.load_state_dict(syn.spi_state(model.spi_module, 3))
    return SPILlavaMPTForCausalLM(model), ids


@DTYPES
def test_bot_turns_with_a_session_answer_as_without(dtype):
    from gpt4roi_amd.serve import ConversationBot
    lm, ids = _mini_lm(dtype)
    g = torch.Generator().manual_seed(5)
    picture = torch.randint(0, 256, (300, 400, 3), generator=g, dtype=torch.uint8).numpy()
    other_picture = torch.randint(0, 256, (300, 400, 3), generator=g, dtype=torch.uint8).numpy()
    two, three = [[20, 30, 220, 260], [100, 10, 390, 200]], [[20, 30, 220, 260], [100, 10, 390, 200], [5, 5, 120, 140]]
    turns = [("What is <region1> doing next to <region2> ?", picture, two),
             ("And what colour is <region2> ?", picture, []),
             ("Is <region3> behind <region1> ?", picture, three),
             ("What else is there ?", other_picture, [])]
    prompt_lens = []
    generate = lm.generate

    def recording_generate(input_ids, *a, **kw):
        prompt_lens.append(int(input_ids.size(1)))
        return generate(input_ids, *a, **kw)
    lm.generate = recording_generate

    def converse(session):
        bot, hist, answers, stats = ConversationBot(lm, _BotTok(ids), image_size=112), [], [], []
        for text, pic, boxes in turns:
            ans, err, hist = bot.run(text, {"image": pic, "boxes": boxes}, hist, do_sample=False, max_new_tokens=8,
                                     session=session)
            assert err is None, err
            answers.append(ans)
            if session is not None:
                stats.append((session.reused, session.prefilled, prompt_lens[-1]))
            if len(answers) == 3:
                third = copy.deepcopy(hist)
        return answers, third, hist, stats

    plain_answers, plain_third, plain_hist, _ = converse(None)
    session = GenerationSession()
    answers, third, hist, stats = converse(session)
    print("answers:", answers, "(reused, prefilled, prompt length) per turn:", stats)
    assert answers == plain_answers

    def same_history(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x["sources"] == y["sources"] and x["region_name_set"] == y["region_name_set"]
            assert torch.equal(x["bboxes"], y["bboxes"])
    same_history(third, plain_third)
    same_history(hist, plain_hist)
    assert stats[0][0] == 0 and stats[0][1] == stats[0][2]            # turn one: nothing to reuse
    for reused, prefilled, n in stats[1:3]:                           # turns two and three (three adds a box)
        assert reused > 0 and prefilled == n - reused
    # turn two keeps the whole first prompt.  Turn three keeps less, not more: from the second round on the reference
    # renders the stored conversation in place (serve.py, app.py), so round three wraps the first message in a second
    # "### Human: " and its ids leave the cached ones right behind the system header (tests/test_session_cpu.py pins that)
    assert stats[1][0] == stats[0][2]
    assert stats[3][0] == 0 and stats[3][1] == stats[3][2]            # another image: nothing may be trusted
    # somebody else's generate() on the same model empties the session's claim on the cache
    lm.generate = generate
    lm.generate(torch.tensor([[1, 20, 21, 22]], device=DEV), max_new_tokens=2)
    assert not session.valid_for(lm.model.llama)


@DTYPES
def test_bot_sampled_turn_draws_the_same_ids_with_a_session(dtype):
    """ConversationBot.run(do_sample=True, seed=...) with and without a session: the same Philox stream (its step counter
    starts at 0 every turn) over logits that agree within 16-bit rounding gives the same answers.  Turn two keeps the whole
    first prompt, so its draws run over a continued prefill."""
    from gpt4roi_amd.serve import ConversationBot
    lm, ids = _mini_lm(dtype)
    g = torch.Generator().manual_seed(5)
    picture = torch.randint(0, 256, (300, 400, 3), generator=g, dtype=torch.uint8).numpy()
    turns = [("What is <region1> doing next to <region2> ?", [[20, 30, 220, 260], [100, 10, 390, 200]], 31),
             ("And what colour is <region2> ?", [], 77)]

    def converse(session):
        bot, hist, answers = ConversationBot(lm, _BotTok(ids), image_size=112), [], []
        for text, boxes, seed in turns:
            ans, err, hist = bot.run(text, {"image": picture, "boxes": boxes}, hist, do_sample=True, temperature=0.2,
                                     max_new_tokens=8, seed=seed, session=session)
            assert err is None, err
            answers.append(ans)
        return answers

    plain = converse(None)
    session = GenerationSession()
    answers = converse(session)
    print("sampled answers:", answers, "plain:", plain, "reused", session.reused, "prefilled", session.prefilled)
    assert session.reused > 0
    assert answers == plain


@DTYPES
def test_append_only_prompts_keep_cached_box_rows_when_a_box_is_added(dtype):
    """generate(session=) under prompts that only append: turn two adds a third box behind the cached prefix, so the
    region module runs with three RoIs while the two cached `<bbox>` rows are trusted; ids equal those without a session."""
    lm, ids = _mini_lm(dtype)
    g = torch.Generator().manual_seed(6)
    image = torch.randn(1, 3, 112, 112, generator=g).to(dtype).to(DEV)
    two = torch.tensor([[0.05, 0.1, 0.55, 0.85], [0.25, 0.03, 0.97, 0.66]], device=DEV)
    three = torch.cat([two, torch.tensor([[0.01, 0.02, 0.3, 0.45]], device=DEV)], 0)
    first = [1, 20, 21, ids.im_start_token] + [ids.im_patch_token] * 64 + [ids.im_end_token, 22, 23, ids.bbox_token, 24,
                                                                          25, ids.bbox_token, 26, 5]
    p1 = torch.tensor([first], device=DEV)
    session = GenerationSession()
    new1 = lm.generate(p1, images=image, bboxes=[two], do_sample=False, max_new_tokens=6, session=session,
                       return_new_tokens=True, eos_token_id=-1)
    assert all(t < ids.im_patch_token for t in new1), new1          # a special id fed back would change the splice
    p2 = torch.tensor([first + new1 + [5, 27, 28, ids.bbox_token, 29, 5]], device=DEV)
    with_session = lm.generate(p2, images=image, bboxes=[three], do_sample=False, max_new_tokens=6, session=session,
                               return_new_tokens=True, eos_token_id=-1)
    print("reused", session.reused, "prefilled", session.prefilled, "ids", with_session)
    assert session.reused == len(first) + len(new1) - 1 and session.prefilled == p2.size(1) - session.reused
    plain = lm.generate(p2, images=image, bboxes=[three], do_sample=False, max_new_tokens=6, return_new_tokens=True,
                        eos_token_id=-1)
    assert with_session == plain
    # the first box moved: the cache is trusted only up to its `<bbox>` row
    moved = three.clone()
    moved[0, 0] += 0.02
    lm.generate(p1, images=image, bboxes=[two], do_sample=False, max_new_tokens=6, session=session, eos_token_id=-1)
    lm.generate(p2, images=image, bboxes=[moved], do_sample=False, max_new_tokens=6, session=session, eos_token_id=-1)
    assert session.reused == first.index(ids.bbox_token)
