"""Generation glue of the region-feature path.

Mirrors what the reference's callers touch around `model.generate` (gpt4roi/app.py:285-301):
  * `KeywordsStoppingCriteria(keywords, tokenizer, input_ids)`      llava/model/utils.py:26-46
  * `prepare_inputs_for_generation(input_ids, past_key_values, ...)` llava/model/llava.py:263-283
  * the sampling defaults HF's `generate(do_sample=True, temperature=0.2)` runs with at the pinned transformers commit
    (GenerationConfig: top_k = 50, top_p = 1.0), executed by the device-side sampler g4r_sample_advance_f32.
Host-side logic only; the decode loop itself is LlamaDecoder.decode_graph (one hipGraph replay per token).
"""
from dataclasses import dataclass
from typing import Optional

import torch


class StoppingCriteria:
    """Call contract of transformers.StoppingCriteria: __call__(input_ids [B, T], scores) -> bool."""

    def __call__(self, input_ids, scores=None, **kwargs) -> bool:
        raise NotImplementedError


class KeywordsStoppingCriteria(StoppingCriteria):
    """Stops generation at a keyword -- the contract of llava/model/utils.py:26-46, which gpt4roi/app.py:289-300 builds with
    `['###']`: constructor `(keywords, tokenizer, input_ids)`; callable `(output_ids, scores) -> bool`.

    Behaviour kept from the reference, because callers (and HF's per-token calling convention) rely on it:
      * the first call arms the criterion (it only remembers how long the prompt was) and answers False;
      * afterwards a hit is EITHER the newest token being the id of a keyword that tokenises to exactly one id, OR the
        keyword text occurring in the decoded continuation (special tokens skipped);
      * only row 0 of the batch is looked at (the app is batch 1).
    Incremental use: `LlamaDecoder.decode_graph` shows it every prefix exactly once."""

    def __init__(self, keywords, tokenizer, input_ids):
        self.keywords = list(keywords)
        self.tokenizer = tokenizer
        self.input_ids = input_ids
        self.start_len = None                       # armed by the first call
        single_token_ids = []
        for word in self.keywords:
            ids = tokenizer(word).input_ids
            if isinstance(ids, list) and len(ids) == 1:
                single_token_ids.append(ids[0])
        self.keyword_ids = single_token_ids

    def _prompt_length(self):
        return self.input_ids.shape[1]

    def __call__(self, output_ids, scores=None, **kwargs) -> bool:
        if self.start_len is None:
            self.start_len = self._prompt_length()
            return False
        newest = output_ids[0, -1]
        if any(newest == kid for kid in self.keyword_ids):
            return True
        continuation = self.tokenizer.batch_decode(output_ids[:, self.start_len:], skip_special_tokens=True)[0]
        return any(word in continuation for word in self.keywords)


def prepare_inputs_for_generation(input_ids, past_key_values=None, attention_mask=None, inputs_embeds=None, **kwargs):
    """What HF `generate` asks the model for before every step (contract of llava/model/llava.py:263-283):
    with a KV cache only the newest token id is fed; `inputs_embeds` may replace the ids on the cache-less first step only;
    `images` is forwarded on every step (the vision branch ignores single-token calls, spi_llava.py:47-48)."""
    first_step = past_key_values is None
    if past_key_values:
        input_ids = input_ids[:, -1:]
    feed = {"inputs_embeds": inputs_embeds} if (inputs_embeds is not None and first_step) else {"input_ids": input_ids}
    feed["past_key_values"] = past_key_values
    feed["use_cache"] = kwargs.get("use_cache")
    feed["attention_mask"] = attention_mask
    feed["images"] = kwargs.get("images", None)
    return feed


@dataclass
class SamplingConfig:
    """do_sample / temperature / top_k / top_p as HF's GenerationConfig names them (defaults of the pinned release)."""
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    seed: Optional[int] = None

    def sampler(self):
        if not self.do_sample:
            return None
        if not self.temperature > 0:
            raise ValueError("`temperature` has to be a strictly positive float")
        if not 0 < self.top_p <= 1.0:
            raise ValueError("`top_p` has to be a float > 0 and <= 1")
        k = int(self.top_k or 0)
        if k < 0 or k > 1024:
            raise ValueError("`top_k` has to be in [0, 1024] (0 disables it) for the device-side sampler")
        if self.top_p < 1.0 and k == 0:
            raise NotImplementedError("top_p < 1 without top_k is not implemented on the device-side sampler")
        return (float(self.temperature), k, float(self.top_p))


SEED_STRIDE = 0x9E3779B97F4A7C15       # 2^64 / golden ratio: the seeds of the rows of a batch sampled with one int seed


def expand_seeds(seeds, B):
    """The B per-row Philox keys of a batched sampling call, as ints in [0, 2^64).  seeds = None: B seeds drawn from torch's
    generator (as batch-1 generate draws its one seed); an int s: row b gets (s + b * SEED_STRIDE) mod 2^64, so row 0 draws
    the stream of a batch-1 call with seed s; a list / tuple: one seed per row."""
    if seeds is None:
        return [int(x) for x in torch.randint(0, 2 ** 62, (B,)).tolist()]
    if isinstance(seeds, (list, tuple)):
        if len(seeds) != B:
            raise ValueError(f"{len(seeds)} seeds for a batch of {B} sequences")
        return [int(x) % 2 ** 64 for x in seeds]
    return [(int(seeds) + b * SEED_STRIDE) % 2 ** 64 for b in range(B)]


def row_samplers(sampler, B):
    """Per-row token selection of a batch: None (every row greedy), one (temperature, top_k, top_p) for every row, or a list
    of B entries, each None (greedy) or a tuple.  -> list of B entries."""
    if sampler is None or isinstance(sampler, tuple):
        rows = [sampler] * B
    else:
        rows = list(sampler)
        if len(rows) != B:
            raise ValueError(f"{len(rows)} samplers for a batch of {B} sequences")
    for r in rows:
        if r is not None and (len(r) != 3 or not r[0] > 0 or not 0 < r[2] <= 1.0 or not 0 <= int(r[1]) <= 1024
                              or (r[2] < 1.0 and int(r[1]) == 0)):
            raise ValueError(f"sampler {r!r}: (temperature > 0, top_k in [0, 1024], top_p in (0, 1]; top_p < 1 needs top_k)")
    return rows


def dense_or_mask(attention_mask):
    """Training batches: None when the mask is absent, all ones or RIGHT-padded (what the collator produces,
    data_modules.py:22-56) -- causal attention already hides the pad keys from every real row and the pad rows carry no
    loss (labels -100), so the dense kernels give the reference's logits on the real rows and its gradients; any other
    pattern (left padding, holes) is returned as a bool mask for the unpad -> varlen -> pad path the reference's
    flash-attention patch takes (llama_flash_attn_monkey_patch.py:60-85).  One small device->host read."""
    if attention_mask is None or attention_mask.dim() != 2:
        return None
    m = attention_mask.to(torch.bool)
    if m.size(1) <= 1 or bool((m[:, :-1] | ~m[:, 1:]).all()):
        return None
    return m


# ---- conversation sessions: a follow-up turn prefills only what the KV cache does not already hold -------------------
def plan_reuse(cached_ids, new_ids, same_image, cached_boxes, new_boxes, bbox_id, max_positions, max_new_tokens):
    """How many leading cache rows a new prompt may trust: -> L, the prompt is then prefilled from position L.

    cached_ids: the token ids whose K/V the cache holds, in row order; new_ids: the new prompt; cached_boxes / new_boxes:
    the box of every `<bbox>` token (id `bbox_id`) in order of appearance, as 4-number sequences.  L is
      * the longest common prefix of the ids -- nothing is assumed about how the earlier answer re-tokenises: the caller
        strips `###` / `Assistant:` from it (app.py:309-324) and the common prefix simply ends where that shows;
      * 0 if the image differs (every patch token's embedding depends on it);
      * cut to just before the first `<bbox>` position whose box differs (that row's embedding is the box's feature);
      * at most len(new_ids) - 1: at least one token is prefilled, so logits exist;
      * 0 if len(new_ids) + max_new_tokens does not fit the cache (the caller's full prefill then fails as it does today).
    Pure host function."""
    cached_ids, new_ids = list(cached_ids), list(new_ids)
    if not same_image or not cached_ids or not new_ids:
        return 0
    if len(new_ids) + int(max_new_tokens) > int(max_positions):
        return 0
    n = min(len(cached_ids), len(new_ids) - 1)
    L = 0
    while L < n and cached_ids[L] == new_ids[L]:
        L += 1
    cached_boxes = [] if cached_boxes is None else list(cached_boxes)
    new_boxes = [] if new_boxes is None else list(new_boxes)
    k = 0
    for p in range(L):
        if new_ids[p] != bbox_id:
            continue
        same = k < len(cached_boxes) and k < len(new_boxes) and \
            [float(x) for x in cached_boxes[k]] == [float(x) for x in new_boxes[k]]
        if not same:
            return p
        k += 1
    return L


def plan_shared_prefix(rows_ids, same_image, rows_boxes, bbox_id):
    """How many leading positions the rows of ONE batch share: -> P, the batch is then prefilled once over [0, P) and the
    rows decode against one copy of that prefix (LlamaDecoder.decode_graph_batch(shared_prefix=P)).  The sibling of
    `plan_reuse`, across the rows of a batch instead of the turns of a conversation.

    rows_ids: the real (unpadded) token ids of every row; same_image: every row's image equals row 0's; rows_boxes: per row,
    the box of every `<bbox>` token (id `bbox_id`) in order of appearance, as 4-number sequences (or None).  P is
      * the longest common prefix of all rows' ids;
      * 0 if the images differ (every patch token's embedding depends on the image);
      * cut to just before the first `<bbox>` position whose box differs, in any row, from row 0's box of the same ordinal
        (that position's embedding is the box's feature);
      * at most min_b n_b - 1: every row keeps at least one position of its own, so each has step-0 logits.
    Pure host function."""
    rows_ids = [list(r) for r in rows_ids]
    if not rows_ids or not same_image or any(len(r) == 0 for r in rows_ids):
        return 0
    first = rows_ids[0]
    P = min(len(r) for r in rows_ids) - 1
    for r in rows_ids[1:]:
        n = 0
        while n < P and r[n] == first[n]:
            n += 1
        P = n
    boxes = [[] if b is None else [[float(x) for x in box] for box in b] for b in (rows_boxes or [None] * len(rows_ids))]
    if len(boxes) != len(rows_ids):
        raise ValueError(f"{len(boxes)} box lists for {len(rows_ids)} rows")
    k = 0
    for p in range(P):
        if first[p] != bbox_id:
            continue
        if not all(k < len(b) and b[k] == boxes[0][k] for b in boxes):
            return p
        k += 1
    return P


# ---- encoded images: the vision path and the fused pyramid run once per picture, not per row or per turn ---------------
@dataclass(eq=False)
class EncodedImage:
    """What the model computes from ONE image and nothing else (the class lives here, beside the host functions that group
    and compare images; spi_llava re-exports it): made by SPILlavaLlamaModel.encode_image, read through
    SPILlavaLlamaModel.features_of (which re-encodes from `pixels` when a stamp no longer matches the model), accepted
    wherever generate() takes `images`.  Inference only.

    pixels [3, S, S]: a detached copy of the input.  tokens [n_patch, C]: the projected patch tokens the splice reads.
    maps / affs: the four raw maps of the fused pyramid ([1, H_l, H_l, E], H_l = 8P, 4P, 2P, P) and their deferred
    GroupNorm + ReLU affines ([1, 2, E] fp32) -- what RoIAlign pools any box from.  P: tokens per side; image_size = 14 P;
    dtype: the 16-bit storage type.  tower / spi_stamp / proj_stamp: the vision tower object and the parameter stamps
    (data pointer and version counter of every region-module / projector parameter) the features were computed with.
    The tower is watched by IDENTITY only (it is frozen and keeps 16-bit copies without version stamps): weights loaded
    in place into the same ClipVisionTower object leave an encoding stale without any sign -- encode again after that.

    Memory: the maps hold 85 P^2 positions of E 16-bit channels, 85 * P^2 * E * 2 bytes -- 100 MB for a 336^2 image at
    E = 1024 (P = 24), 25 MB at 224^2 -- plus n_patch * C * 2 bytes of patch tokens (4.7 MB at 336^2, C = 4096) and the
    fp32 pixels (1.4 MB).  Equality is identity (two encodings of equal pixels are two objects;
    generation.same_pixels compares the pixels)."""
    pixels: torch.Tensor
    tokens: torch.Tensor
    maps: list
    affs: list
    P: int
    image_size: int
    dtype: torch.dtype
    tower: object
    spi_stamp: tuple
    proj_stamp: tuple
    encodes: int = 1                                # how often the features were computed (1 + the re-encodes)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in [self.pixels, self.tokens] + list(self.maps) + list(self.affs))


def is_encoded(image):
    return isinstance(image, EncodedImage)


def _pixels(image):
    """The [3, S, S] pixel tensor a row shows: the tensor itself, or the copy an EncodedImage keeps."""
    x = image.pixels if is_encoded(image) else image
    return x[0] if x.dim() == 4 and x.size(0) == 1 else x


def same_pixels(a, b):
    """Two rows show one image iff they are the same EncodedImage object or their pixel tensors agree in shape, dtype,
    device and every value (`torch.equal`)."""
    if a is b:
        return True
    x, y = _pixels(a), _pixels(b)
    return x.shape == y.shape and x.dtype == y.dtype and x.device == y.device and bool(torch.equal(x, y))


def group_images(images):
    """The rows of a batch grouped by the image they show: -> (unique, image_of_row).  images: a [B, 3, S, S] tensor or a
    sequence of B entries, each a [3, S, S] pixel tensor or an EncodedImage; rows are equal as `same_pixels` says.
    unique lists one entry per distinct image in order of first appearance -- the EncodedImage of the group when any of its
    rows brought one (nothing is left to compute for it), else the first row's pixel tensor -- and image_of_row[b] indexes
    it.  Pure host function (one comparison per row and earlier distinct image)."""
    rows = [images] if is_encoded(images) else list(images)
    unique, image_of_row = [], []
    for r in rows:
        for u, have in enumerate(unique):
            if same_pixels(have, r):
                if is_encoded(r) and not is_encoded(have):
                    unique[u] = r
                image_of_row.append(u)
                break
        else:
            unique.append(r)
            image_of_row.append(len(unique) - 1)
    return unique, image_of_row


@dataclass
class WindowPlan:
    """What one windowed splice (SPILlavaLlamaModel.embed_window) is told, per row: positions [lo, hi) are written;
    region_from = the ordinal of the first box that goes through the region head = spi_skip, the number of leading `<bbox>`
    tokens the splice kernel finds no feature row for (both are the number of `<bbox>` tokens before lo).  W = the widest
    window (at least 1): the stride of the compact output."""
    lo: list
    hi: list
    region_from: list
    spi_skip: list
    W: int


def plan_windows(rows_ids, lo, hi, bbox_id):
    """rows_ids: the real (unpadded) ids of every row; lo / hi: one int for all rows or one per row, hi None = each row's
    length.  ValueError unless 0 <= lo <= hi <= len(row).  Pure host function."""
    rows_ids = [list(r) for r in rows_ids]
    B = len(rows_ids)
    lo = [int(x) for x in lo] if isinstance(lo, (list, tuple)) else [int(lo)] * B
    hi = [len(r) for r in rows_ids] if hi is None else \
        ([int(x) for x in hi] if isinstance(hi, (list, tuple)) else [int(hi)] * B)
    if len(lo) != B or len(hi) != B:
        raise ValueError(f"{len(lo)} / {len(hi)} window bounds for {B} rows")
    for r, a, z in zip(rows_ids, lo, hi):
        if not 0 <= a <= z <= len(r):
            raise ValueError(f"window [{a}, {z}) of a row of {len(r)} tokens")
    before = [sum(1 for t in r[:a] if t == bbox_id) for r, a in zip(rows_ids, lo)]
    return WindowPlan(lo, hi, before, list(before), max([1] + [z - a for a, z in zip(lo, hi)]))


def plan_shared_windows(rows_ids, P, bbox_id):
    """The two splices of a shared-prefix batch whose images are encoded once: -> (prefix, suffix).  prefix: ONE row, row 0,
    over [0, P); its region_from is 0 when a `<bbox>` lies before P (row 0's boxes then go through the region head, once for
    the whole batch) and the row's `<bbox>` count otherwise (no box is needed: the region head does not run).  suffix: every
    row over [P, n_b), region_from = the number of `<bbox>` tokens before P.
    Known redundancy: a window skips LEADING boxes only (the splice's count check is #<bbox> == spi_skip + #regions), so
    when a `<bbox>` lies before P the prefix call sends ALL of row 0's boxes through the region head, and those of them
    that sit at or behind P go through it a second time with the suffixes.  Correct, and one row's trailing boxes at
    most; the boxes before P still run once instead of B times."""
    rows_ids = [list(r) for r in rows_ids]
    suffix = plan_windows(rows_ids, P, None, bbox_id)
    prefix = plan_windows(rows_ids[:1], 0, P, bbox_id)
    if suffix.region_from[0] == 0:
        n0 = sum(1 for t in rows_ids[0] if t == bbox_id)
        prefix.region_from, prefix.spi_skip = [n0], [n0]
    return prefix, suffix


def plan_session_window(new_ids, L, bbox_id):
    """A session turn that keeps L cache rows splices only [L, T): the boxes whose `<bbox>` sits at or behind L go through
    the region head (none: it does not run)."""
    return plan_windows([list(new_ids)], L, None, bbox_id)


def right_padded_lengths(attention_mask, B, T):
    """The rows' real lengths of a RIGHT-padded [B, T] mask (None: all T) as a list of ints; ValueError for any other mask
    (left padding, holes, an empty row).  One small device->host read."""
    if attention_mask is None:
        return [int(T)] * int(B)
    if attention_mask.dim() != 2 or tuple(attention_mask.shape) != (B, T):
        raise ValueError(f"attention_mask must be [{B}, {T}], got {tuple(attention_mask.shape)}")
    rows = attention_mask.to(torch.bool).cpu().tolist()
    lens = [sum(r) for r in rows]
    if any(n == 0 or not all(r[:n]) for r, n in zip(rows, lens)):
        raise ValueError("shared_prefix needs a RIGHT-padded batch: each row's real tokens first, then the padding")
    return lens


def _batch_box_rows(bboxes, B):
    """The boxes of a batch as B lists of 4-float lists (bboxes: None, or the reference's list of B [n_b, 4] tensors)."""
    if bboxes is None:
        return [[] for _ in range(B)]
    if hasattr(bboxes, "boxes_h16") or len(bboxes) != B:
        raise ValueError(f"shared_prefix reads the boxes as a list of {B} [n, 4] tensors, one per row")
    return [[[float(x) for x in row] for row in b.detach().float().cpu().tolist()] for b in bboxes]


def _box_rows(bboxes):
    """The boxes of a batch-1 request as a list of 4-float lists (bboxes: None, or the reference's list of one [n, 4])."""
    if bboxes is None:
        return []
    if hasattr(bboxes, "boxes_h16"):                         # layers.PreparedBoxes: the rows the region module reads
        rows = bboxes.boxes_h16
    elif len(bboxes) == 0:
        return []
    else:
        rows = bboxes[0]
    return [[float(x) for x in row] for row in rows.detach().float().cpu().tolist()]


class GenerationSession:
    """What the KV cache of ONE decoder holds between the turns of ONE conversation, so that `generate(session=...)` can
    prefill only the tokens behind the longest prefix it may trust (`plan_reuse`).  The caller keeps one per conversation,
    next to the reference's `history_cache` (app.py), and hands it to every turn.

    ids / image / boxes: the token ids whose K/V the cache holds (truncated to the decoder's row count), the image tensor
    (with cache_image=True: its EncodedImage) and the per-`<bbox>` boxes they were computed with.  decoder / stamp: the decoder they live in and its `cache_version`
    when the session last wrote it -- a session that meets another decoder, or a cache somebody else has reset or written
    since, is treated as empty.  reused / prefilled: cache rows kept / prompt positions prefilled by the last call."""

    def __init__(self, cache_image=False):
        """cache_image: keep the conversation's picture as an EncodedImage (what generate() computed from it: projected
        patch tokens and the fused pyramid, about 105 MB at 336^2, see SPILlavaLlamaModel.encode_image) in place of the
        pixel copy.  A turn on the same image then runs no ViT and no fuse round, splices only the positions it prefills
        and runs the region head only for boxes whose `<bbox>` lies there.  One image per session: another image
        replaces the entry.  Default False: the session holds and does what it did before."""
        self.cache_image = bool(cache_image)
        self.clear()
        self.reused = 0
        self.prefilled = 0

    def clear(self):
        self.ids, self.image, self.boxes, self.decoder, self.stamp = [], None, [], None, None

    def valid_for(self, decoder):
        return (self.decoder is decoder and self.stamp is not None and self.stamp == getattr(decoder, "cache_version", None)
                and len(self.ids) > 0 and len(self.ids) <= getattr(decoder, "rows_held", 0))

    def same_image(self, image):
        """Pixels are compared with the session's own copy (an in-place change by the caller shows).  A turn without an
        image trusts nothing: a text-only conversation runs as without a session."""
        if self.image is None or image is None:
            return False
        if is_encoded(self.image) or is_encoded(image):
            return same_pixels(self.image, image)
        return self.image.shape == image.shape and self.image.dtype == image.dtype and \
            self.image.device == image.device and bool(torch.equal(self.image, image))

    def plan(self, decoder, new_ids, image, boxes, bbox_id, max_new_tokens):
        """-> L for this turn (0 for an empty / foreign / stale session)."""
        if not self.valid_for(decoder):
            return 0
        return plan_reuse(self.ids, new_ids, self.same_image(image), self.boxes, boxes, bbox_id, decoder.max_positions,
                          max_new_tokens)

    def update(self, decoder, prompt_ids, new_ids, image, boxes, reused):
        """After a decode: the cache holds the prompt and the generated tokens that were fed back (`decoder.rows_held`)."""
        prompt_ids = list(prompt_ids)
        self.ids = (prompt_ids + list(new_ids))[:int(decoder.rows_held)]
        if is_encoded(image):                                    # cache_image: the encoding (it owns a copy of the pixels)
            self.image = image
        elif image is None or not self.same_image(image):
            self.image = None if image is None else image.detach().clone()
        self.boxes = [list(b) for b in boxes]
        self.decoder, self.stamp = decoder, decoder.cache_version
        self.reused, self.prefilled = int(reused), len(prompt_ids) - int(reused)
