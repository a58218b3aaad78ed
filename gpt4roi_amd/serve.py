"""Headless conversation loop around the region-feature path: what `ConversationBot` of the reference's
demo does between the UI and the model, without the UI.

Mirrors gpt4roi/app.py:
  count_num_bboxes            :47-50    `<regionN>` mentions of a question
  ConversationBot.build_model :62-108   -> `ConversationBot.from_pretrained` (checkpoint.from_pretrained + bind_tokenizer)
  ConversationBot.init_inputs :110-188  boxes normalised by the image size, image -> 224^2 pixel tensor, first-round preamble,
                                        `<regionN>` -> `regionN <bbox>`, preprocess_multimodal + preprocess, box carry-over
  ConversationBot.check_input :190-239  number of `<regionN>` in the text vs boxes drawn this round; re-mentions of a known
                                        region lose their brackets
  ConversationBot.run         :243-328  KeywordsStoppingCriteria('###'), forward bound with partial(bboxes=...), sampling
                                        generate(temperature 0.2, <= 1024 new tokens), answer clean-up, history update
  ConversationBot.run_batch             the same round for several conversations in one left-padded batched generate()
Not mirrored: Gradio widgets, the box overlay drawing (`visualize`), chat-history HTML escaping.

The history cache has the reference's structure (a list whose last entry holds 'sources', 'region_name_set', 'bboxes') and
the same aliasing: from the second round on the stored conversation is the object the prompt functions rewrite in place,
so a third round sees the already rendered turns exactly like the reference does (pinned by tests/golden/bot_ref.json,
generated from the reference's own class).

Image step: the reference resizes with CLIPImageProcessor (bicubic, shortest edge 224, no crop) and then bilinearly to
224 x 224 (:125-136); here `kernels.image_preprocess` does normalise + bilinear resize to 224 x 224 in one launch from the
uint8 image.  `preprocess_image` can be replaced by the caller (e.g. with the HF processor) -- everything
after it only needs a float [3, S, S] tensor.
"""
import copy
import re
from functools import partial

import numpy as np
import torch

from .generation import KeywordsStoppingCriteria
from .prompt import preprocess, preprocess_multimodal

MULTIMODAL_CFG = dict(is_multimodal=True, sep_image_conv_front=False, image_token_len=256, image_aspect_ratio='square',
                      use_im_start_end=True)                       # app.py:33-39
PREAMBLE = "The <image> provides an overview of the picture.\n"     # app.py:141
STOP_STR = '###'
EMPTY_ANSWER = "There is internal error. Please click 'Clear All' and try again."     # app.py:316 (what the caller shows)


def count_num_bboxes(text):
    """-> (number of `<regionN>` mentions, the mentions)  (app.py:47-50)"""
    found = re.findall(r'<region\d+>', text)
    return len(found), found


def _mark_regions(text):
    """`<regionN>` / `<N>` -> `regionN <bbox>`, `<>` -> `<bbox>`  (app.py:148-150, 164-166)"""
    text = re.sub(r'<region(\d+)>', r'region\g<1> <bbox>', text)
    text = re.sub(r'\<(\d+)\>', r'region\g<1> <bbox>', text)
    return text.replace('<>', '<bbox>')


def _image_size(image):
    """(width, height) of a PIL image / HWC array / HWC tensor."""
    if hasattr(image, 'size') and not isinstance(image, (np.ndarray, torch.Tensor)):
        return image.size
    return int(image.shape[1]), int(image.shape[0])


class ConversationBot:
    def __init__(self, model, tokenizer, image_size=224, device='cuda', patch=14):
        self.model, self.tokenizer = model, tokenizer
        self.image_size, self.device, self.patch = image_size, device, patch

    @classmethod
    def from_pretrained(cls, model_name, tokenizer, vision_tower=None, device='cuda', **kw):
        """build_model (app.py:62-108): checkpoint directory -> model on the GPU, special tokens bound."""
        from .checkpoint import from_pretrained
        from .spi_llava import SPILlavaMPTForCausalLM
        model = from_pretrained(SPILlavaMPTForCausalLM, model_name, device=device, vision_tower=vision_tower,
                                tokenizer=tokenizer, **kw)
        return cls(model, tokenizer, device=device)

    # ---- image -----------------------------------------------------------------------------------------------------
    def preprocess_image(self, image):
        """uint8 RGB image (PIL / HWC array / HWC tensor) -> float [3, S, S] on the device, CLIP-normalised."""
        from . import kernels as K
        if not isinstance(image, torch.Tensor):
            arr = np.asarray(image.convert('RGB') if hasattr(image, 'convert') else image)
            image = torch.from_numpy(np.ascontiguousarray(arr))
        return K.image_preprocess(image.to(self.device), self.image_size)

    # ---- one round: host-side assembly ---------------------------------------------------------------------------
    def init_inputs(self, input_dict, question_str, history_cache):
        """-> (dict(input_ids, labels, sources, image, bboxes), history_cache)   (app.py:110-188)"""
        boxes = input_dict['boxes']
        have_boxes = len(boxes) > 0
        width, height = _image_size(input_dict['image'])
        if have_boxes:
            norm = np.array(boxes, dtype=np.float64) / np.array([width, height, width, height])
        image = self.preprocess_image(input_dict['image'])
        n_patch = (image.shape[1] // self.patch) * (image.shape[2] // self.patch)
        if not history_cache:
            question = PREAMBLE + question_str
            names = count_num_bboxes(question)[1]
            if have_boxes:
                question = _mark_regions(question)
            sources = {'conversations': [{'from': 'human', 'value': question}]}
            history_cache.append({'sources': copy.deepcopy(sources), 'region_name_set': set(names)})
        else:
            sources = history_cache[-1]['sources']           # the stored object itself: rewritten in place below
            sources['conversations'].append({'from': 'human', 'value': _mark_regions(question_str)})
        turns = preprocess_multimodal([sources['conversations']], MULTIMODAL_CFG, n_patch)
        rendered = copy.deepcopy(turns)
        enc = preprocess(turns, self.tokenizer)
        data = dict(input_ids=enc['input_ids'][0], labels=enc['labels'][0], sources=rendered, image=image)
        data['bboxes'] = torch.Tensor(norm) if have_boxes else history_cache[-1]['bboxes']
        history_cache[-1]['bboxes'] = copy.deepcopy(data['bboxes'])
        return data, history_cache

    def check_input(self, text, image, history_cache):
        """-> (error message or None, text with re-mentioned regions un-bracketed)   (app.py:190-239)"""
        if image is None:
            return 'No image: upload an image first.', text
        first = len(history_cache) == 0
        n_boxes = len(image['boxes'])
        if first:
            if n_boxes == 0:
                return 'No region of interest: draw at least one box on the image.', text
            drawn = n_boxes
        else:
            drawn = 0 if n_boxes == 0 else n_boxes - len(history_cache[-1]['bboxes'])
            known = copy.deepcopy(history_cache[-1]['region_name_set'])
            for name in count_num_bboxes(text)[1]:
                if name in known:
                    text = text.replace(name, name[1:-1])     # an old region is referred to by its plain name
                else:
                    known.add(name)
            history_cache[-1]['region_name_set'] = known
        mentioned = count_num_bboxes(text)[0]
        if mentioned != drawn:
            if mentioned == 0:
                return (f'The question {text!r} does not refer to the drawn boxes (use the <regionN> format).'), text
            return (f'The question {text!r} mentions {mentioned} <regionN>, but {drawn} boxes were drawn this round.'), text
        return None, text

    # ---- one round: model ------------------------------------------------------------------------------------------
    def run(self, text, image, history_cache, do_sample=True, temperature=0.2, max_new_tokens=1024, seed=None,
            session=None):
        """One question -> (answer text or None, error message or None, history_cache)   (app.py:243-328, no UI state).
        session: a generation.GenerationSession the caller keeps next to `history_cache`, one per conversation; with it a
        follow-up turn prefills only the tokens the KV cache does not hold yet (same answers, see generate); a
        GenerationSession(cache_image=True) also keeps the picture's encoding, so a follow-up on the same picture runs no
        vision tower and no fuse round."""
        error, text = self.check_input(text, image, history_cache)
        if error is not None:
            return None, error, history_cache
        text = text.strip()
        if not text:
            text = 'hello, world!'                           # app.py:256-258
        inputs, history_cache = self.init_inputs(image, text, history_cache)
        bboxes = inputs['bboxes']
        if bboxes is not None:
            bboxes = [bboxes.to(self.device)]
        input_ids = inputs['input_ids'].to(self.device)[None]
        criteria = KeywordsStoppingCriteria([STOP_STR], self.tokenizer, input_ids)
        model = self.model
        with torch.inference_mode():
            model.orig_forward = model.forward
            model.forward = partial(model.orig_forward, img_metas=[None], bboxes=bboxes)
            try:
                output_ids = model.generate(input_ids, images=inputs['image'][None].to(self.device), do_sample=do_sample,
                                            temperature=temperature, max_new_tokens=max_new_tokens,
                                            stopping_criteria=[criteria], seed=seed, session=session)
            finally:
                model.forward = model.orig_forward
        T = input_ids.shape[1]
        return self._answer(output_ids[:, T:], history_cache)

    def _answer(self, new_ids, history_cache):
        """New ids [1, n] -> (answer shown, None, history_cache): the clean-up and history update of app.py:309-328."""
        answer = self.tokenizer.batch_decode(new_ids, skip_special_tokens=True)[0].strip()
        if answer.endswith(STOP_STR):
            answer = answer[:-len(STOP_STR)]
        answer = answer.strip() or EMPTY_ANSWER
        shown = answer
        answer = answer.replace('Assistant: ', '').replace('Assistant:', '')
        history_cache[-1]['sources']['conversations'].append({'from': 'gpt', 'value': answer})
        return shown, None, history_cache

    def batch_inputs(self, texts, images, history_caches, pad_side="left"):
        """check_input + init_inputs for each conversation, then the batch: prompts LEFT-padded with the tokenizer's pad id
        (HF batch generation style; pad_side="right": right-padded, what generate(shared_prefix=True) takes) -> (results,
        rows, dict(input_ids [B, T], attention_mask [B, T], images [B, 3, S, S], bboxes list of B)).  results[i] is
        (None, error, history_caches[i]) for a conversation that fails its check, else None; rows lists the conversations
        in the batch, in order."""
        if pad_side not in ("left", "right"):
            raise ValueError(f"pad_side = {pad_side!r}: 'left' or 'right'")
        results, rows, ids, imgs, boxes = [None] * len(texts), [], [], [], []
        for i, (text, image, hist) in enumerate(zip(texts, images, history_caches)):
            error, text = self.check_input(text, image, hist)
            if error is not None:
                results[i] = (None, error, hist)
                continue
            text = text.strip() or 'hello, world!'           # app.py:256-258
            inputs, history_caches[i] = self.init_inputs(image, text, hist)
            rows.append(i)
            ids.append(inputs['input_ids'])
            imgs.append(inputs['image'])
            bb = inputs['bboxes']
            boxes.append(bb.to(self.device) if bb is not None else torch.zeros(0, 4, device=self.device))
        if not rows:
            return results, rows, None
        T = max(int(x.numel()) for x in ids)
        pad = self.tokenizer.pad_token_id
        input_ids = torch.full((len(rows), T), pad, dtype=torch.int64)
        mask = torch.zeros((len(rows), T), dtype=torch.int64)
        for r, x in enumerate(ids):
            lo = T - x.numel() if pad_side == "left" else 0
            input_ids[r, lo:lo + x.numel()] = x
            mask[r, lo:lo + x.numel()] = 1
        batch = dict(input_ids=input_ids.to(self.device), attention_mask=mask.to(self.device),
                     images=torch.stack([im.to(self.device) for im in imgs], 0), bboxes=boxes)
        return results, rows, batch

    def run_batch(self, texts, images, history_caches, do_sample=True, temperature=0.2, max_new_tokens=1024, seeds=None,
                  share_prefix=False, share_images=False):
        """Several conversations, one question each, answered by ONE batched generate(): -> list of
        (answer or None, error or None, history_cache), one per conversation.  Each conversation is checked and assembled
        as `run` does it; those that fail the check return their error and stay out of the batch.  The prompts are
        left-padded into one batch that decodes together (the weight stream of a step is shared), each sequence sampled
        with its own Philox stream and stopped by the '###' criterion on its own ids; the answers are cleaned up and
        appended to each history exactly as `run` does.  seeds: None (drawn), an int (expanded over the batch rows, see
        generate) or a list with one seed per conversation (a conversation then draws what `run(seed=...)` would draw on
        the same logits).  `run` stays the batch-1 path.
        share_prefix: the batch is built RIGHT-padded and generated with shared_prefix=True -- several questions about one
        image share the system header and the image tokens, which are then prefilled once and read once per decode step
        for the whole batch; every conversation is computed at its own positions, as `run` computes it.  Conversations
        about different images share nothing (P = 0) and still decode together.  Answers and histories as above.
        share_images (with share_prefix): generate(share_images=True) -- every distinct picture of the batch goes through the
        vision tower and the fuse rounds once, at batch 1, whatever the number of conversations about it."""
        if share_images and not share_prefix:
            raise ValueError("share_images=True goes with share_prefix=True")
        results, rows, batch = self.batch_inputs(texts, images, history_caches, pad_side="right" if share_prefix else "left")
        if not rows:
            return results
        if isinstance(seeds, (list, tuple)):
            if len(seeds) != len(texts):
                raise ValueError(f"{len(seeds)} seeds for {len(texts)} conversations")
            seeds = [seeds[i] for i in rows]
        input_ids = batch['input_ids']
        T = input_ids.size(1)
        # one '###' criterion for the batch: built on the padded prompts (T = its start length), generate() applies it to
        # every row on that row's own ids, so it acts for each conversation as run()'s criterion does for one
        criteria = KeywordsStoppingCriteria([STOP_STR], self.tokenizer, input_ids)
        model = self.model
        with torch.inference_mode():
            model.orig_forward = model.forward
            model.forward = partial(model.orig_forward, img_metas=[None] * len(rows), bboxes=batch['bboxes'])
            try:
                new = model.generate(input_ids, images=batch['images'], attention_mask=batch['attention_mask'],
                                     do_sample=do_sample, temperature=temperature, max_new_tokens=max_new_tokens,
                                     stopping_criteria=[criteria], seed=seeds, pad_token_id=self.tokenizer.pad_token_id,
                                     return_new_tokens=True,
                                     **(dict(shared_prefix=True, **(dict(share_images=True) if share_images else {}))
                                        if share_prefix and len(rows) > 1 else {}))
            finally:
                model.forward = model.orig_forward
        if len(rows) == 1:
            new = [new]
        for r, i in enumerate(rows):
            ids = torch.tensor([new[r]], dtype=torch.int64).reshape(1, -1)
            results[i] = self._answer(ids, history_caches[i])
        return results
