"""CPU: the host side of conversation sessions (gpt4roi_amd/generation.py) -- the reuse plan as a pure function, the
session's bookkeeping against a stub decoder, and the refusal of a session next to a batch."""
from types import SimpleNamespace

import pytest
import torch

from gpt4roi_amd.generation import GenerationSession, plan_reuse

BBOX = 901
BOX_A, BOX_B, BOX_C = [0.1, 0.2, 0.5, 0.6], [0.3, 0.3, 0.9, 0.8], [0.0, 0.1, 0.2, 0.3]


def _plan(cached, new, same_image=True, cb=(), nb=(), max_positions=2048, max_new=64):
    return plan_reuse(cached, new, same_image, list(cb), list(nb), BBOX, max_positions, max_new)


def test_identical_prefix_plus_suffix():
    cached = [1, 7, 8, 9, 10, 11]
    assert _plan(cached, cached + [20, 21, 22]) == 6


def test_divergence_inside_the_old_answer():
    # the cleaned-up answer re-tokenises differently from the generated ids: the prefix ends where that shows
    cached = [1, 7, 8, 9, 50, 51, 52]
    new = [1, 7, 8, 9, 50, 60, 61, 20, 21]
    assert _plan(cached, new) == 5


def test_different_image_reuses_nothing():
    cached = [1, 7, 8, 9]
    assert _plan(cached, cached + [20], same_image=False) == 0


def test_second_box_changed_cuts_before_the_second_bbox():
    cached = [1, 7, BBOX, 8, 9, BBOX, 10, 11]
    new = cached + [20, 21]
    assert _plan(cached, new, cb=[BOX_A, BOX_B], nb=[BOX_A, BOX_C]) == 5
    assert _plan(cached, new, cb=[BOX_A, BOX_B], nb=[BOX_A, BOX_B]) == 8
    assert _plan(cached, new, cb=[BOX_A, BOX_B], nb=[BOX_C, BOX_B]) == 2
    # a box added behind the common prefix does not touch it; a box missing for a <bbox> inside it does
    assert _plan(cached, new + [BBOX], cb=[BOX_A, BOX_B], nb=[BOX_A, BOX_B, BOX_C]) == 8
    assert _plan(cached, new, cb=[BOX_A], nb=[BOX_A, BOX_B]) == 5


def test_new_ids_equal_to_the_cached_ids_leave_one_token_to_prefill():
    cached = [1, 7, 8, 9, 10]
    assert _plan(cached, list(cached)) == len(cached) - 1
    assert _plan(cached + [11, 12], cached) == len(cached) - 1       # the cache holds more than the new prompt


def test_a_prompt_that_would_overflow_the_cache_falls_back_to_a_full_prefill():
    cached = list(range(1, 101))
    assert _plan(cached, cached + [200], max_positions=128, max_new=27) == 100
    assert _plan(cached, cached + [200], max_positions=128, max_new=28) == 0


def test_empty_session_reuses_nothing():
    assert _plan([], [1, 2, 3]) == 0
    assert _plan([1, 2, 3], []) == 0


class _StubDecoder:
    """What a session reads of a LlamaDecoder: rows_held, cache_version, max_positions."""

    def __init__(self, max_positions=256):
        self.max_positions, self.rows_held, self.cache_version = max_positions, 0, 0

    def wrote(self, rows):                       # what decode_graph leaves behind
        self.rows_held, self.cache_version = rows, self.cache_version + 1

    def reset(self):
        self.rows_held, self.cache_version = 0, self.cache_version + 1


def _held_session(dec, image):
    s = GenerationSession()
    prompt, new = [1, 7, BBOX, 8, 9], [30, 31, 32]
    dec.wrote(len(prompt) + len(new) - 1)        # the last generated token was never fed back
    s.update(dec, prompt, new, image, [BOX_A], reused=0)
    return s, prompt, new


def test_session_keeps_what_the_cache_holds():
    dec, image = _StubDecoder(), torch.zeros(3, 4, 4)
    s, prompt, new = _held_session(dec, image)
    assert s.ids == prompt + new[:-1] and (s.reused, s.prefilled) == (0, len(prompt))
    nxt = prompt + new + [40, 41]
    assert s.plan(dec, nxt, image, [BOX_A], BBOX, 8) == len(prompt) + len(new) - 1
    assert s.plan(dec, nxt, image.clone(), [BOX_A], BBOX, 8) == len(prompt) + len(new) - 1     # equal pixels, other tensor
    assert s.plan(dec, nxt, image + 1, [BOX_A], BBOX, 8) == 0
    assert s.plan(dec, nxt, image, [BOX_B], BBOX, 8) == 2
    dec.wrote(len(nxt) + 3)
    s.update(dec, nxt, [50, 51, 52, 53], image, [BOX_A], reused=7)
    assert (s.reused, s.prefilled) == (7, len(nxt) - 7) and s.ids == nxt + [50, 51, 52]


def test_a_foreign_decoder_is_treated_as_empty():
    dec, other, image = _StubDecoder(), _StubDecoder(), torch.zeros(3, 4, 4)
    s, prompt, new = _held_session(dec, image)
    other.wrote(dec.rows_held)                   # same counters, another object
    assert s.plan(other, prompt + new + [40], image, [BOX_A], BBOX, 8) == 0
    assert s.plan(dec, prompt + new + [40], image, [BOX_A], BBOX, 8) > 0


def test_an_externally_reset_cache_is_treated_as_empty():
    dec, image = _StubDecoder(), torch.zeros(3, 4, 4)
    s, prompt, new = _held_session(dec, image)
    dec.reset()
    assert s.plan(dec, prompt + new + [40], image, [BOX_A], BBOX, 8) == 0
    s2, prompt, new = _held_session(dec, image)
    dec.wrote(dec.rows_held)                     # somebody else's generate() ran on this decoder in between
    assert s2.plan(dec, prompt + new + [40], image, [BOX_A], BBOX, 8) == 0


def test_generate_refuses_a_session_next_to_a_batch():
    from gpt4roi_amd.spi_llava import SPILlavaMPTForCausalLM
    lm = SPILlavaMPTForCausalLM.__new__(SPILlavaMPTForCausalLM)       # the check comes before anything touches the model
    with pytest.raises(ValueError, match="session"):
        SPILlavaMPTForCausalLM.generate(lm, torch.zeros((2, 5), dtype=torch.int64), session=GenerationSession())


class _WordTok:
    """Word-level stub tokenizer with the HF batch call prompt.py uses."""

    def __init__(self):
        self.vocab, self.pad_token_id, self.model_max_length = {}, 0, 2048

    def _ids(self, text):
        return [self.vocab.setdefault(w, 10 + len(self.vocab)) for w in
                text.replace("<", " <").replace(">", "> ").split()]

    def __call__(self, text, return_tensors=None, padding=None, max_length=None, truncation=None):
        if return_tensors is None:
            return SimpleNamespace(input_ids=self._ids(text))
        rows = [[1] + self._ids(t) for t in ([text] if isinstance(text, str) else text)]
        n = max(len(r) for r in rows)
        return SimpleNamespace(input_ids=torch.tensor([r + [0] * (n - len(r)) for r in rows], dtype=torch.int64))


def test_what_the_bot_prompts_of_three_rounds_share():
    """How much a session can keep under ConversationBot is decided by the reference's prompt assembly (app.py, mirrored by
    serve.py): round two re-sends round one's prompt unchanged and appends, so all of it is a common prefix; from then on
    the stored conversation is rendered in place, round three wraps the earlier messages in a second "### Human: " /
    "### Assistant: ", and its ids leave round two's right behind the system header.  A caller whose prompts only ever
    append (generate(session=) under its own history) keeps the whole conversation every round."""
    import numpy as np
    from gpt4roi_amd.serve import ConversationBot
    tok = _WordTok()
    bot = ConversationBot(None, tok, image_size=28, device="cpu")
    bot.preprocess_image = lambda image: torch.zeros(3, 28, 28)
    picture = np.zeros((30, 40, 3), np.uint8)
    rounds = [("What is <region1> ?", [[2, 3, 20, 26]]), ("And its colour ?", []), ("Why ?", [])]
    hist, prompts = [], []
    for text, boxes in rounds:
        image = {"image": picture, "boxes": boxes}
        err, text = bot.check_input(text, image, hist)
        assert err is None
        inputs, hist = bot.init_inputs(image, text, hist)
        prompts.append(inputs["input_ids"].tolist())
        hist[-1]["sources"]["conversations"].append({"from": "gpt", "value": "a b c"})
    boxes = [[0.05, 0.1, 0.5, 0.8667]]
    header = prompts[0].index(tok.vocab["Human:"]) + 1
    L2 = plan_reuse(prompts[0], prompts[1], True, boxes, boxes, -1, 2048, 8)
    L3 = plan_reuse(prompts[1], prompts[2], True, boxes, boxes, -1, 2048, 8)
    assert L2 == len(prompts[0])
    assert L3 == header and prompts[2][header:header + 2] == prompts[2][header - 2:header]


def test_routing_rule_of_the_continuation_attention_follows_its_table():
    """profiles/session_kernel_ab.txt (H = 32, D = 128, B = 1): WIN at Tk >= 32 Tq, no win elsewhere; unmeasured -> forward."""
    from gpt4roi_amd import kernels as K
    wins = {(8, 512), (16, 512), (8, 1024), (16, 1024), (32, 1024), (8, 2048), (16, 2048), (32, 2048), (64, 2048)}
    for Tk in (512, 1024, 2048):
        for Tq in (8, 16, 32, 64):
            assert K.cont_attn_wins(Tq, Tk, 32) == ((Tq, Tk) in wins), (Tq, Tk)
    assert not K.cont_attn_wins(8, 256, 32) and not K.cont_attn_wins(1, 2048, 32) and not K.cont_attn_wins(65, 4096, 32)
    assert not K.cont_attn_wins(8, 2048, 4) and not K.cont_attn_wins(8, 2048, 32, batch=2)
