"""GPU: shared-prefix batches -- LlamaDecoder.decode_graph_batch(shared_prefix=P), generate(shared_prefix=,
num_return_sequences=), ConversationBot.run_batch(share_prefix=True).

The tiny decoder of tests/test_session_gpu.py (2 layers, hidden 512, 4 heads x 128, vocabulary 1000), fp16 and bf16; the
yardstick is the fp32 oracle (oracle/transformer_oracle.py) on the decoder's own 16-bit weights, run on each row ALONE: the
shared path computes every row at its own positions, which is what a row gets when it is served alone.
  * step-0 logits of the shared batch may be at most 1.25 x as far from the oracle as those of decode_graph's fresh batch-1
    prefill of that row (this project's "no worse than" margin), and the two paths agree within the sum of their errors;
  * greedy ids: a row is compared only if its oracle top-2 logit gap, at every generated step, exceeds ten times the fresh
    path's measured logit error; compared rows equal the oracle's ids and the row served alone.  Inputs picked with the
    oracle on the CPU from 300 seeds (prefix randn(1, 70, 512) from manual_seed(5000 + seed), row b's suffix from
    manual_seed(7000 + 10 seed + b)): on each of the seeds below two of the three rows have oracle gaps >= 0.259 in both
    dtypes, the third's is below 0.13 and is expected to drop; of the 12 rows at least 6 must be compared (the oracle
    alone leaves 8 at 0.18 = 10 x the 0.018 logit error tests/test_session_gpu.py records for the bf16-emulating oracle).
Every assertion holds on either attention route of the decode step (kernels.SHARED_ATTN_ROUTE pinned to the shared-prefix
kernel and to the existing ragged kernel)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampler_oracle as SO  # noqa: E402  (the checkers; never the product path)
from oracle import transformer_oracle as TO  # noqa: E402

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd import synthetic as syn
    from gpt4roi_amd.generation import SEED_STRIDE, expand_seeds
    from gpt4roi_amd.llama import LlamaDecoder
    from gpt4roi_amd.spi_llava import SPILlavaLlamaModel, SPILlavaMPTForCausalLM
    from gpt4roi_amd.vit import ClipVisionTower

DEV = "cuda"
HID, HEADS, INTER, LAYERS, VOCAB = 512, 4, 1408, 2, 1000
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
ROUTES = pytest.mark.parametrize("route", ["always", "never"], ids=["shared-kernel", "ragged-kernel"])
SUFFIX = (5, 9, 13)
GREEDY_SEEDS = (177, 106, 171, 121)
N_NEW = 3


def _decoder(dtype, max_positions=256):
    sd = syn.llama_state(HID, INTER, LAYERS, VOCAB, seed=9)
    dec = LlamaDecoder(sd, heads=HEADS, max_positions=max_positions, device=DEV, dtype=dtype)
    w = {k: v.to(dtype).float().to(DEV) for k, v in sd.items()}       # the oracle computes in fp32 on the 16-bit weights
    return dec, w


def _randn(n, seed, dtype):
    return torch.randn(1, n, HID, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _batch(prefix, suffixes, dtype):
    """-> (the rows alone [1, P + n_b, C], the right-padded batch [B, T, C], its mask); the padding is ordinary noise."""
    rows = [torch.cat([prefix, s], 1).contiguous() for s in suffixes]
    T = max(r.size(1) for r in rows)
    batch = _randn(len(rows) * T, 31, dtype).view(len(rows), T, HID).clone()
    mask = torch.zeros(len(rows), T, dtype=torch.bool, device=DEV)
    for b, r in enumerate(rows):
        batch[b, :r.size(1)] = r[0]
        mask[b, :r.size(1)] = True
    return rows, batch, mask


def _oracle_last_logits(w, row):
    h, _ = TO.llama_forward(w, row.float(), HEADS)
    return TO.lm_logits(w, h[:, -1:])[0, 0]


@DTYPES
@ROUTES
@pytest.mark.parametrize("P,max_positions", [(70, 256), (530, 1024)])
def test_step0_logits_of_a_shared_prefix_batch(P, max_positions, route, dtype, monkeypatch):
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", route)
    dec, w = _decoder(dtype, max_positions)
    prefix = _randn(P, 400 + P, dtype)
    rows, batch, mask = _batch(prefix, [_randn(n, 500 + P + n, dtype) for n in SUFFIX], dtype)
    version = dec.cache_version
    ids = dec.decode_graph_batch(batch, 2, key_padding_mask=mask, shared_prefix=P)
    assert [len(r) for r in ids] == [2, 2, 2] and dec.rows_held == 0 and dec.cache_version > version
    assert dec.pos == P + max(SUFFIX) + 1
    shared = dec.shared_step0_logits.clone()
    assert dec._bstate[(3, "shared", route == "always", False)]["route"] == (route == "always")
    for b, row in enumerate(rows):
        want = _oracle_last_logits(w, row)
        dec.reset(1)
        fresh = dec.forward(row, all_logits=False).view(-1)
        e_shared, e_fresh = float((shared[b] - want).abs().max()), float((fresh - want).abs().max())
        between = float((shared[b] - fresh).abs().max())
        print(f"P={P} row {b} {dtype}: shared err {e_shared:.3e}, fresh err {e_fresh:.3e}, shared vs fresh {between:.3e}")
        assert e_shared <= 1.25 * e_fresh, (b, e_shared, e_fresh)
        assert between <= e_shared + e_fresh, (b, between, e_shared, e_fresh)
        assert ids[b][0] == int(shared[b].argmax())


@DTYPES
@ROUTES
def test_greedy_ids_of_a_shared_prefix_batch_are_those_of_each_row_alone(route, dtype, monkeypatch):
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", route)
    dec, w = _decoder(dtype)
    compared, dropped = [], []
    for seed in GREEDY_SEEDS:
        prefix = _randn(70, 5000 + seed, dtype)
        rows, batch, mask = _batch(prefix, [_randn(n, 7000 + 10 * seed + b, dtype) for b, n in enumerate(SUFFIX)], dtype)
        got = dec.decode_graph_batch(batch, N_NEW, key_padding_mask=mask, shared_prefix=70)
        for b, row in enumerate(rows):
            ids_o, trace = TO.greedy_decode(w, row.float(), lambda t: dec.embed[t.to(DEV)].float(), HEADS, N_NEW)
            gap = min(float((lambda s: s[0] - s[1])(torch.topk(lg, 2).values)) for lg in trace)
            dec.reset(1)
            lg = dec.forward(row, all_logits=False)
            err = 0.0
            for s in range(N_NEW):                                    # the fresh path's error along the oracle's sequence
                err = max(err, float((lg.view(-1) - trace[s]).abs().max()))
                lg = dec.forward(dec.embed[torch.tensor([[ids_o[s]]], device=DEV)].view(1, 1, -1), all_logits=False)
            print(f"seed {seed} row {b} {dtype} {route}: oracle min top-2 gap {gap:.4f}, fresh logit error {err:.4f}")
            if not gap > 10.0 * err:
                dropped.append((seed, b))
                continue
            alone = dec.decode_graph(row, N_NEW)
            assert got[b] == ids_o == alone, (seed, b, got[b], ids_o, alone)
            compared.append((seed, b))
    assert len(compared) >= 6, (compared, dropped)


def test_decoder_refuses_what_the_shared_path_does_not_take():
    dec, _ = _decoder(torch.bfloat16)
    prefix = _randn(20, 1, torch.bfloat16)
    rows, batch, mask = _batch(prefix, [_randn(n, 2 + n, torch.bfloat16) for n in (3, 6)], torch.bfloat16)
    dec.forward(rows[0], all_logits=False)
    version, kc = dec.cache_version, dec.kc.clone()
    left = mask.flip(1)
    for kw in (dict(key_padding_mask=left, shared_prefix=20),              # left-padded
               dict(key_padding_mask=mask, shared_prefix=23),              # row 0 has 23 tokens: nothing of its own left
               dict(key_padding_mask=mask, shared_prefix=20, own_positions=False),
               dict(key_padding_mask=mask[:, :5], shared_prefix=3)):
        with pytest.raises(ValueError):
            dec.decode_graph_batch(batch, 2, **kw)
    with pytest.raises(ValueError):
        dec.decode_graph_batch(batch, 240, key_padding_mask=mask, shared_prefix=20)     # does not fit the cache
    assert dec.cache_version == version and torch.equal(dec.kc, kc)        # refused before the cache was touched
    # P = 0 (an empty prefix at the rows' own positions) and no mask (all rows full) are taken
    assert [len(r) for r in dec.decode_graph_batch(batch, 2, key_padding_mask=mask, own_positions=True)] == [2, 2]
    assert [len(r) for r in dec.decode_graph_batch(batch[:, :22], 2, shared_prefix=20)] == [2, 2]


# ---- generate() and the bot ------------------------------------------------------------------------------------------
def _mini_lm(dtype=torch.bfloat16):
    ids = syn.token_ids(vocab_base=990)
    tower = ClipVisionTower(syn.vit_state(HID, 4 * HID, 12, 112, seed=8), heads=8, device=DEV, dtype=dtype)
    dec = LlamaDecoder(syn.llama_state(HID, INTER, LAYERS, ids.vocab, seed=9), heads=HEADS, max_positions=512, device=DEV,
                       dtype=dtype)
    model = SPILlavaLlamaModel(tower, dec, ids, embed_dims=HID)
    model.spi_module.load_state_dict(syn.spi_state(model.spi_module, 3))
    return SPILlavaMPTForCausalLM(model), ids


def _check_draw(row, got, step, seed, T, k, p, u, tol=1e-6):
    """got == the oracle's draw, or u lies within `tol` of a CDF step of the kept set (float rounding decides there)."""
    want = SO.sample(row, step, seed, T, k, p)
    if got != want:
        keep, e = SO.kept_and_weights(row, T, k, p)
        cdf = np.cumsum(e.astype(np.float64)) / e.astype(np.float64).sum()
        assert got in keep.tolist() and np.min(np.abs(cdf - u)) < tol, (step, got, want, u)


@ROUTES
def test_num_return_sequences_draws_n_rows_from_one_prompt(route, monkeypatch):
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", route)
    lm, ids = _mini_lm()
    dec = lm.model.llama
    g = torch.Generator().manual_seed(6)
    image = torch.randn(1, 3, 112, 112, generator=g).to(torch.bfloat16).to(DEV)
    boxes = [torch.tensor([[0.05, 0.1, 0.55, 0.85], [0.25, 0.03, 0.97, 0.66]], device=DEV)]
    prompt = torch.tensor([[1, 20, 21, ids.im_start_token] + [ids.im_patch_token] * 64 +
                           [ids.im_end_token, 22, 23, ids.bbox_token, 24, 25, ids.bbox_token, 26, 5]], device=DEV)
    T, n, N, seed, temp, k = prompt.size(1), 4, 8, 4242, 0.8, 20
    kw = dict(images=image, bboxes=boxes, do_sample=True, temperature=temp, top_k=k, max_new_tokens=N, seed=seed,
              eos_token_id=-1)
    seeds = expand_seeds(seed, n)
    # first the decoder with the loop on the host (no graph captured yet, so every step's logits can be kept): n rows of
    # the one prompt, P = T - 1; every id is the oracle's draw from that row's own logits with that row's Philox stream
    with torch.no_grad():
        emb = lm.model.embed_inputs(prompt, image, boxes).expand(n, -1, -1)
        rec, orig = [], dec._advance_batch

        def spy(logits, state):
            rec.append(logits.float().cpu().clone())
            orig(logits, state)
        dec._advance_batch = spy
        try:
            eager = dec.decode_graph_batch(emb, N, sampler=(temp, k, 1.0), seeds=seeds, shared_prefix=T - 1, use_graph=False,
                                           stop_ids={-1})
        finally:
            del dec._advance_batch
    st = dec._bstate[(n, "shared", route == "always", True)]
    assert st["graph"] is None and len(rec) == N and [len(r) for r in eager] == [N] * n
    us = st["u"][:, :N].cpu().numpy()
    for b in range(n):                                                    # distinct Philox streams, pinned bit for bit
        assert seeds[b] == (seed + b * SEED_STRIDE) % 2 ** 64
        assert all(us[b, s] == SO.uniform(s, seeds[b]) for s in range(N)), b
        for s in range(N):
            _check_draw(rec[s][b].numpy(), eager[b][s], s, seeds[b], temp, k, 1.0, float(us[b, s]))
    assert len({tuple(us[b].tolist()) for b in range(n)}) == n
    assert len({tuple(r) for r in eager}) > 1                             # and the rows are not n copies of one draw
    # generate(): the same ids through the captured graph, reproducibly, in both return forms
    out = lm.generate(prompt, num_return_sequences=n, pad_token_id=3, **kw)
    assert out.shape == (n, T + N) and all(torch.equal(out[b, :T], prompt[0]) for b in range(n))
    assert lm.last_shared_prefix == T - 1 and st["graph"] is not None
    new = lm.generate(prompt, num_return_sequences=n, return_new_tokens=True, **kw)
    assert isinstance(new, list) and len(new) == n and out[:, T:].tolist() == new == eager
    assert torch.equal(st["u"][:, :N].cpu(), torch.from_numpy(us))
    # n = 1 / None is the batch-1 call
    one = lm.generate(prompt, num_return_sequences=1, **kw)
    assert one.shape == (1, T + N) and torch.equal(one, lm.generate(prompt, **kw))


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


@ROUTES
def test_bot_run_batch_with_a_shared_prefix(route, monkeypatch):
    from gpt4roi_amd.serve import ConversationBot
    monkeypatch.setattr(K, "SHARED_ATTN_ROUTE", route)
    lm, ids = _mini_lm()
    bot = ConversationBot(lm, _BotTok(ids), image_size=112)
    g = torch.Generator().manual_seed(5)
    pics = [torch.randint(0, 256, (300, 400, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(2)]
    images = [{"image": pics[0], "boxes": [[20, 30, 220, 260], [100, 10, 390, 200]]},
              {"image": pics[0], "boxes": [[5, 5, 120, 140]]},
              {"image": pics[1], "boxes": [[0, 0, 200, 150], [50, 60, 380, 290]]}]
    texts = ["What is <region1> doing next to <region2> ?", "Which colour is <region1> ?",
             "Where is <region1> sitting close to <region2> ?"]
    calls = []
    generate = lm.generate

    def recording_generate(input_ids, *a, **kw):
        calls.append((kw.get("shared_prefix"), kw["attention_mask"].clone()))
        return generate(input_ids, *a, **kw)
    lm.generate = recording_generate
    res = bot.run_batch(texts, images, [[], [], []], max_new_tokens=8, seeds=[3, 4, 5], share_prefix=True)
    assert calls[-1][0] is True and lm.last_shared_prefix == 0           # another image in the batch: nothing is shared
    m = calls[-1][1]
    assert bool((m[:, :-1] >= m[:, 1:]).all()) and not bool(m.all())      # right-padded, and really padded
    two = bot.run_batch(texts[:2], images[:2], [[], []], max_new_tokens=8, seeds=[3, 4], share_prefix=True)
    P = lm.last_shared_prefix
    _, _, batch = bot.batch_inputs(texts[:2], images[:2], [[], []], pad_side="right")
    row0 = batch["input_ids"][0].tolist()
    assert P > row0.index(ids.im_end_token) and P <= row0.index(ids.bbox_token)     # header + image, up to the first box
    again = bot.run_batch(texts[:2], images[:2], [[], []], max_new_tokens=8, seeds=[3, 4], share_prefix=True)
    assert [a for a, _, _ in two] == [a for a, _, _ in again]
    for a, e, h in res + two:
        assert e is None and isinstance(a, str) and len(a) > 0
        conv = h[-1]["sources"]["conversations"]                          # the history update of run()
        assert [t["from"] for t in conv] == ["human", "gpt"] and conv[1]["value"] == a.replace("Assistant: ", "")
        assert h[-1]["bboxes"].dim() == 2 and float(h[-1]["bboxes"].max()) <= 1.0
    assert lm.forward == lm.orig_forward                                   # the partial binding was undone
    # the default stays the left-padded masked batch
    bot.run_batch(texts[:2], images[:2], [[], []], max_new_tokens=4, seeds=[3, 4])
    assert calls[-1][0] is None and lm.last_shared_prefix is None
