"""GPU: batched sampling -- g4r_sample_rows_f32 (one draw per logits row, per-row temperature / top-k / top-p / seed) against
oracle/sampler_oracle.py draw for draw, the sampled and early-exiting LlamaDecoder.decode_graph_batch, generate() for B > 1
with do_sample and per-sequence stopping criteria (the call of gpt4roi/app.py:293-300 for several requests at once), and
ConversationBot.run_batch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampler_oracle as SO  # noqa: E402

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd import synthetic as syn
    from gpt4roi_amd.generation import SEED_STRIDE
    from gpt4roi_amd.llama import LlamaDecoder
    from gpt4roi_amd.spi_llava import KeywordsStoppingCriteria, SPILlavaLlamaModel, SPILlavaMPTForCausalLM
    from gpt4roi_amd.vit import ClipVisionTower

DEV = "cuda"

# (temperature, top_k, top_p) per row; temperature 0 = a greedy row
ROWS = [(0.0, 0, 1.0),            # greedy
        (0.2, 50, 1.0),           # the reference's serving setting
        (1.0, 0, 1.0),            # every token kept
        (1.3, 1024, 0.5),         # widest list + nucleus
        (1.0, 50, 1.0),           # all ties
        (1.0, 50, 0.9),           # a 12-way tie at the top with p < 1
        (0.7, 5, 1.0)]            # near-deterministic
SEEDS = [0x1234_5678_9ABC + 977 * b for b in range(len(ROWS))]


def _rows_logits(g, N):
    x = (torch.randn(len(ROWS), N, generator=g) * 3).float()
    x[4] = 0.25
    x[5, :12] = 7.5
    x[6, 17] = 50.0
    return x


def _params(rows, seeds):
    return (torch.tensor([r[0] for r in rows], dtype=torch.float32, device=DEV),
            torch.tensor([r[1] for r in rows], dtype=torch.int32, device=DEV),
            torch.tensor([r[2] for r in rows], dtype=torch.float32, device=DEV),
            torch.tensor(seeds, dtype=torch.int64, device=DEV))


def _batch_state(B, n=64):
    return dict(tok=torch.zeros(B, dtype=torch.int64, device=DEV), tok32=torch.zeros(B, dtype=torch.int32, device=DEV),
                out=torch.zeros((B, n), dtype=torch.int64, device=DEV), step=torch.zeros(1, dtype=torch.int32, device=DEV),
                pos=torch.zeros(1, dtype=torch.int32, device=DEV), u=torch.zeros((B, n), dtype=torch.float32, device=DEV))


def _check_draw(row, got, step, seed, T, k, p, u, tol=1e-6):
    """got == the oracle's draw, or u lies within `tol` of a CDF step of the kept set (float rounding decides there).
    -> True when the ids agree."""
    want = SO.sample(row, step, seed, T, k, p)
    if got == want:
        return True
    keep, e = SO.kept_and_weights(row, T, k, p)
    cdf = np.cumsum(e.astype(np.float64)) / e.astype(np.float64).sum()
    assert got in keep.tolist() and np.min(np.abs(cdf - u)) < tol, (step, got, want, u)
    return False


@pytest.mark.parametrize("N", [32006, 1000])
def test_sample_rows_matches_the_oracle_draw_for_draw(N):
    g = torch.Generator().manual_seed(N)
    B, n = len(ROWS), 24
    temp, topk, topp, seed = _params(ROWS, SEEDS)
    st = _batch_state(B)
    misses, drawn = [0] * B, []
    for s in range(n):
        x = _rows_logits(g, N)
        xd = x.to(DEV)
        nxt = K.sample_rows(xd, temp, topk, topp, seed, st["step"], u_out=st["u"])
        greedy = K.argmax_rows(xd)
        K.batch_advance(nxt, st["tok"], st["tok32"], st["out"], st["step"], st["pos"])
        ids, us = nxt.tolist(), st["u"][:, s].cpu().numpy()
        drawn.append(ids)
        assert ids[0] == int(greedy[0])                                 # the greedy row is argmax_rows' id
        for b in range(B):
            assert us[b] == SO.uniform(s, SEEDS[b]), (s, b)               # Philox pinned, bit for bit
            if b > 0:
                T, k, p = ROWS[b]
                misses[b] += not _check_draw(x[b].numpy(), ids[b], s, SEEDS[b], T, k, p, float(us[b]))
    assert int(st["step"]) == n and int(st["pos"]) == n                 # the kernel read the step, batch_advance moved it
    assert st["out"][:, :n].t().tolist() == drawn
    assert max(misses) <= 1, misses
    assert st["u"][:, n:].abs().sum().item() == 0                        # nothing written past the steps run


def test_sample_rows_are_independent_and_equal_the_batch_1_sampler():
    g = torch.Generator().manual_seed(3)
    N, B = 32006, len(ROWS)
    x = _rows_logits(g, N).to(DEV)
    step = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    temp, topk, topp, seed = _params(ROWS, SEEDS)
    u = torch.zeros((B, 8), dtype=torch.float32, device=DEV)
    ids = K.sample_rows(x, temp, topk, topp, seed, step, u_out=u)
    perm = [4, 0, 6, 2, 5, 1, 3]
    prm = torch.tensor(perm, device=DEV)
    u2 = torch.zeros((B, 8), dtype=torch.float32, device=DEV)
    ids2 = K.sample_rows(x[prm].contiguous(), temp[prm].contiguous(), topk[prm].contiguous(), topp[prm].contiguous(),
                         seed[prm].contiguous(), step, u_out=u2)
    assert torch.equal(ids2, ids[prm]) and torch.equal(u2, u[prm])
    # a strided row view (logits of a wider buffer) reads the same rows
    wide = torch.zeros((B, N + 64), dtype=torch.float32, device=DEV)
    wide[:, :N] = x
    assert torch.equal(K.sample_rows(wide[:, :N], temp, topk, topp, seed, step), ids)
    # B = 1 == the batch-1 kernel at the same step
    for b in range(1, B):
        one = K.sample_rows(x[b:b + 1], temp[b:b + 1], topk[b:b + 1], topp[b:b + 1], seed[b:b + 1], step,
                            u_out=u[b:b + 1])
        tok = torch.zeros((1, 1), dtype=torch.int64, device=DEV)
        out = torch.zeros(8, dtype=torch.int64, device=DEV)
        st1, pos = step.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
        u1 = torch.zeros(8, dtype=torch.float32, device=DEV)
        T, k, p = ROWS[b]
        K.sample_advance(x[b], tok, out, st1, pos, seed[b:b + 1].clone(), T, k, p, u_out=u1)
        assert int(one) == int(tok) == int(ids[b]) and float(u1[5]) == float(u[b, 5]), b
    assert int(step) == 5                                               # never advanced by the kernel


def _mini_lm():
    H, P, image = 512, 8, 112
    ids = syn.token_ids(vocab_base=990)
    tower = ClipVisionTower(syn.vit_state(H, 4 * H, 12, image, seed=8), heads=8, device=DEV)
    dec = LlamaDecoder(syn.llama_state(512, 1408, 2, ids.vocab, seed=9), heads=4, max_positions=256, device=DEV)
    model = SPILlavaLlamaModel(tower, dec, ids, embed_dims=H)
    model.spi_module.load_state_dict(syn.spi_state(model.spi_module, 3))
    g = torch.Generator().manual_seed(31)
    img = torch.randn(1, 3, image, image, generator=g).to(DEV)
    boxes = [syn.boxes(2, g).to(DEV)]
    prompt = syn.prompt_ids(ids, P, 2, g, sys_len=4, question_len=5, vocab_base=990)[None].to(DEV)
    return SPILlavaMPTForCausalLM(model), ids, prompt, img, boxes


DEC_ROWS = [(0.8, 20, 1.0), None, (1.2, 40, 0.9)]                   # one greedy row
DEC_SEEDS = [11, 2 ** 64 - 5, 424242]


def _record_logits(dec):
    """Wraps the decoder's batched token selection to keep a copy of every step's logits (eager steps only)."""
    rec = []
    orig = dec._advance_batch

    def spy(logits, st):
        rec.append(logits.float().cpu().clone())
        orig(logits, st)
    dec._advance_batch = spy
    return rec, lambda: delattr(dec, "_advance_batch")


def _check_rows(rec, got, seeds, rows, tol=1e-6):
    for b, r in enumerate(rows):
        for s, ids in enumerate(got[b]):
            row = rec[s][b].numpy()
            if r is None:
                assert ids == int(np.argmax(row)), (b, s)
            else:
                _check_draw(row, ids, s, seeds[b], r[0], r[1], r[2], float(SO.uniform(s, seeds[b])), tol)


@pytest.mark.parametrize("ragged", [False, True])
def test_sampled_decode_graph_batch(ragged):
    lm, ids, _, _, _ = _mini_lm()
    dec = lm.model.llama
    B, T, n = 3, 30, 10
    g = torch.Generator().manual_seed(17)
    tok = torch.randint(1, 900, (B, T), generator=g).to(DEV)
    mask = None
    if ragged:                                                          # left padding, as HF batch generation pads
        mask = torch.ones(B, T, dtype=torch.bool, device=DEV)
        mask[1, :7] = False
        mask[2, :3] = False
    with torch.no_grad():
        emb = K.gather_rows(dec.embed, tok.reshape(-1).to(torch.int32)).view(B, T, -1)
        # the eager loop first (no graph captured yet): on the logits it actually used, every draw is the oracle's
        rec, undo = _record_logits(dec)
        eager = dec.decode_graph_batch(emb, n, sampler=DEC_ROWS, seeds=DEC_SEEDS, key_padding_mask=mask, use_graph=False)
        undo()
        assert len(rec) == n and [len(r) for r in eager] == [n] * B
        _check_rows(rec, eager, DEC_SEEDS, DEC_ROWS)
        # the hipGraph loop draws the same ids, reproducibly
        got = dec.decode_graph_batch(emb, n, sampler=DEC_ROWS, seeds=DEC_SEEDS, key_padding_mask=mask)
        st = dec._bstate[(B, ragged, True)]
        assert st["graph"] is not None and got == eager
        assert dec.decode_graph_batch(emb, n, sampler=DEC_ROWS, seeds=DEC_SEEDS, key_padding_mask=mask) == got
        us = st["u"][:, :n].cpu().numpy()
        for b in range(B):
            assert all(us[b, s] == SO.uniform(s, DEC_SEEDS[b]) for s in range(n)), b
        # teacher-forced replay through the prefill path (dec.forward): its kernels round differently from the decode
        # step's, so a draw may move where u lies within 1e-3 of a CDF step of the replayed logits
        dec.reset(B)
        logits = dec.forward(emb, all_logits=False, key_padding_mask=mask)
        replay = []
        for s in range(n):
            replay.append(logits.view(B, -1).float().cpu())
            nxt = torch.tensor([got[b][s] for b in range(B)], device=DEV)
            logits = dec.forward(K.gather_rows(dec.embed, nxt.to(torch.int32)).view(B, 1, -1), all_logits=False)
        for b, r in enumerate(DEC_ROWS):
            for s in range(n):
                row = replay[s][b].numpy()
                if r is None:
                    assert row[got[b][s]] >= row.max() - 2e-2 * np.abs(row).max(), (b, s)
                else:
                    _check_draw(row, got[b][s], s, DEC_SEEDS[b], r[0], r[1], r[2], float(SO.uniform(s, DEC_SEEDS[b])),
                                tol=1e-3)
        # the greedy graph of the same batch is untouched by the sampled one
        greedy = dec.decode_graph_batch(emb, n, key_padding_mask=mask)
        assert greedy == dec.greedy_batch(emb, n, key_padding_mask=mask)
        # early exit: every row stops on its own, the loop ends long before max_new_tokens
        seen = []

        def on_tokens(b, new):
            seen.append((b, len(new)))
            return len(new) >= 3 + b
        cut = dec.decode_graph_batch(emb, 40, sampler=DEC_ROWS, seeds=DEC_SEEDS, key_padding_mask=mask, on_tokens=on_tokens,
                                     check_every=4)
        assert [len(r) for r in cut] == [3, 4, 5] and all(cut[b] == got[b][:3 + b] for b in range(B))
        assert dec.pos == T + 6 - 1                                     # tokens 1, 2 and one round of 4 replays
        assert sorted(seen) == sorted(set(seen))                        # each prefix shown once
        # an int seed expands to (s + b * SEED_STRIDE) mod 2^64
        dec.decode_graph_batch(emb, 4, sampler=DEC_ROWS, seeds=99, key_padding_mask=mask)
        us = dec._bstate[(B, ragged, True)]["u"][:, :4].cpu().numpy()
        for b in range(B):
            assert all(us[b, s] == SO.uniform(s, (99 + b * SEED_STRIDE) % 2 ** 64) for s in range(4)), b


class _Tok:
    """Two keywords, each a single token id; no text hit."""

    def __init__(self, kw):
        self.kw = kw

    def __call__(self, text):
        return SimpleNamespace(input_ids=[self.kw[text]])

    def batch_decode(self, ids, skip_special_tokens=True):
        return ["x" for _ in ids.tolist()]


def test_generate_batched_sampling_with_per_sequence_stopping():
    """generate(B = 2, do_sample=True, temperature=0.2, stopping_criteria=[KeywordsStoppingCriteria]) -- app.py's call for two
    requests at once: reproducible for a seed, each row cut at its own first criterion hit and padded, row 0's stream the
    batch-1 stream of the same seed; greedy without criteria unchanged."""
    lm, ids, prompt, img, boxes = _mini_lm()
    g = torch.Generator().manual_seed(77)
    prompt2 = syn.prompt_ids(ids, 8, 2, g, sys_len=4, question_len=5, vocab_base=990)[None].to(DEV)
    assert prompt2.shape == prompt.shape
    prompts = torch.cat([prompt, prompt2], 0)
    imgs = torch.cat([img, torch.randn(1, 3, 112, 112, generator=g).to(DEV)], 0)
    bxs = [boxes[0], syn.boxes(2, g).to(DEV)]
    T, n, seed = prompts.size(1), 16, 1234
    kw = dict(images=imgs, bboxes=bxs, do_sample=True, temperature=0.2, max_new_tokens=n, seed=seed)
    with torch.inference_mode():
        full = lm.generate(prompts, **kw)
        again = lm.generate(prompts, **kw)
    assert torch.equal(full, again) and full.shape == (2, T + n)       # no stop: both rows run to max_new_tokens
    rows = full[:, T:].tolist()
    stops = {"###": rows[0][3], "</s>": rows[1][6]}
    ends = [next(i for i, t in enumerate(r) if t in stops.values()) + 1 for r in rows]
    crit = KeywordsStoppingCriteria(list(stops), _Tok(stops), prompts)
    with torch.inference_mode():
        cut = lm.generate(prompts, stopping_criteria=[crit], pad_token_id=3, **kw)
    assert cut.shape == (2, T + max(ends)) and torch.equal(cut[:, :T], prompts)
    for b in range(2):
        assert cut[b, T:T + ends[b]].tolist() == rows[b][:ends[b]]
        assert all(int(t) == 3 for t in cut[b, T + ends[b]:])
    assert lm.model.llama.pos == T + max(ends) - 1                     # the decode stopped with the last row
    u_batch = lm.model.llama._bstate[(2, False, True)]["u"][0, :max(ends)].clone()
    # row 0 draws the batch-1 stream of the same seed
    with torch.inference_mode():
        lm.generate(prompt, images=img, bboxes=boxes, do_sample=True, temperature=0.2, max_new_tokens=n, seed=seed)
    u_one = lm.model.llama._dstate["u"][:max(ends)]
    assert torch.equal(u_batch, u_one)
    assert all(float(u_one[s]) == SO.uniform(s, seed) for s in range(max(ends)))
    # greedy, no criteria: the decoder-level batched greedy loop, as before
    with torch.no_grad():
        greedy = lm.generate(prompts, images=imgs, bboxes=bxs, do_sample=False, max_new_tokens=n)
        emb = lm.model.embed_inputs(prompts, imgs, bxs)
        want = lm.model.llama.greedy_batch(emb, n)
    assert greedy[:, T:].tolist() == want


class _BotTok:
    """Word-level tokenizer with both call styles the bot's collaborators use: HF batch call (prompt.py) and the plain
    call + batch_decode of KeywordsStoppingCriteria.  Special tokens carry the model's configured ids."""

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
        if return_tensors is None:
            return SimpleNamespace(input_ids=self._ids(text))
        rows = [[1] + self._ids(t) for t in ([text] if isinstance(text, str) else text)]
        n = max(len(r) for r in rows)
        return SimpleNamespace(input_ids=torch.tensor([r + [0] * (n - len(r)) for r in rows], dtype=torch.int64))

    def batch_decode(self, ids, skip_special_tokens=True):
        inv = {v: k for k, v in self.vocab.items()}
        return [" ".join(inv.get(t, f"t{t}") for t in row if not (skip_special_tokens and t in self.special.values()))
                for row in ids.tolist()]


def _clean(tok, new_ids):
    """The answer clean-up of ConversationBot.run on a list of new ids."""
    from gpt4roi_amd.serve import EMPTY_ANSWER, STOP_STR
    a = tok.batch_decode(torch.tensor([new_ids], dtype=torch.int64).reshape(1, -1))[0].strip()
    if a.endswith(STOP_STR):
        a = a[:-len(STOP_STR)]
    return a.strip() or EMPTY_ANSWER


def test_conversation_bot_run_batch():
    from gpt4roi_amd.serve import ConversationBot
    lm, ids, _, _, _ = _mini_lm()
    tok = _BotTok(ids)
    bot = ConversationBot(lm, tok, image_size=112)
    g = torch.Generator().manual_seed(5)
    pics = [torch.randint(0, 256, (300, 400, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(3)]
    images = [{"image": pics[0], "boxes": [[20, 30, 220, 260], [100, 10, 390, 200]]},
              {"image": pics[1], "boxes": [[0, 0, 200, 150], [50, 60, 380, 290]]},
              {"image": pics[2], "boxes": [[10, 10, 100, 100]]}]
    texts = ["What is <region1> doing next to <region2> ?", "Where is <region1> sitting close to <region2> ?",
             "What about <region1> and <region2> ?"]                    # the third mentions 2 regions, 1 box was drawn
    res = bot.run_batch(texts, images, [[], [], []], max_new_tokens=10, seeds=[3, 4, 5])
    res2 = bot.run_batch(texts, images, [[], [], []], max_new_tokens=10, seeds=[3, 4, 5])
    assert res[2][0] is None and "region" in res[2][1] and res[2][2] == []
    for (a, e, h), (a2, _, _) in zip(res[:2], res2[:2]):
        assert e is None and isinstance(a, str) and len(a) > 0 and a == a2
        conv = h[-1]["sources"]["conversations"]
        assert [t["from"] for t in conv] == ["human", "gpt"] and conv[1]["value"] == a.replace("Assistant: ", "")
        assert h[-1]["bboxes"].shape == (2, 4) and float(h[-1]["bboxes"].max()) <= 1.0
    assert lm.forward == lm.orig_forward                               # the partial binding was undone
    # second round: no new box, old regions mentioned again -> the boxes of round 1, a longer prompt
    hists = [res[0][2], res[1][2]]
    more = bot.run_batch(["And what colour is <region2> ?", "And <region1> ?"],
                         [{"image": pics[0], "boxes": []}, {"image": pics[1], "boxes": []}], hists, max_new_tokens=6,
                         seeds=[1, 2])
    for a, e, h in more:
        assert e is None and isinstance(a, str)
        assert len(h[-1]["sources"]["conversations"]) == 4 and h[-1]["bboxes"].shape == (2, 4)
    # greedy: the answers of generate() on the bot's own padded batch
    greedy = bot.run_batch(texts[:2], images[:2], [[], []], do_sample=False, max_new_tokens=8)
    results, rows, batch = bot.batch_inputs(texts[:2], images[:2], [[], []])
    assert rows == [0, 1] and results == [None, None]
    crit = KeywordsStoppingCriteria(["###"], tok, batch["input_ids"])
    with torch.no_grad():
        new = lm.generate(batch["input_ids"], images=batch["images"], bboxes=batch["bboxes"],
                          attention_mask=batch["attention_mask"], do_sample=False, max_new_tokens=8,
                          stopping_criteria=[crit], return_new_tokens=True)
    assert [a for a, _, _ in greedy] == [_clean(tok, r) for r in new]
    # equal-length prompts: the batch is dense, and each conversation answers as run() answers it alone
    assert bool(batch["attention_mask"].all())
    alone = [bot.run(texts[i], images[i], [], do_sample=False, max_new_tokens=8)[0] for i in range(2)]
    assert [a for a, _, _ in greedy] == alone
