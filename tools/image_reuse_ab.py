#!/usr/bin/env python3
"""tools/image_reuse_ab.py -- what encoding an image once is worth (DESIGN.md "An image encoded once").

Synthetic 7 B decoder and CLIP-L/14 tower at the configs[1] geometry (336^2 image, 32 RoIs, 767-token prompt), one process,
eager calls (no hipGraph around the prefill), wall clock around generate(max_new_tokens=1) with a device synchronize on both
sides: the time to the first token.

  batch   B = 4 / 16 questions about ONE image (the 767-token prompt with its 32 boxes, then 32 question tokens of the
          row's own): generate(shared_prefix=True) with share_images off (every row through the ViT, the fuse rounds and the
          region head; a [B, T, C] splice) and on (one encoding, the prefix spliced once, the suffixes at batch B).
  turn    the second turn of a conversation (first prompt 767 tokens, 64 generated, a 32-token follow-up): a plain
          GenerationSession and GenerationSession(cache_image=True).
Each arm also runs once with a synchronising stopwatch around the embedding stage and around the splice kernel inside it,
so a saving can be split into vision (tower, fuse rounds, projector, region head) and splice.  Prints plain text; redirect
into profiles/.  Numbers of one box."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gpt4roi_amd import kernels as K  # noqa: E402

DEV = "cuda"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Stopwatch:
    """Synchronising timers around the embedding stage (encode_image / embed_inputs / embed_window, the outermost of them) and
    the splice kernels inside it: -> ms of the stage, ms of it spent in the splice."""

    def __init__(self, model):
        self.model, self.stage, self.splice, self.depth = model, 0.0, 0.0, 0
        self.saved = (model.embed_inputs, model.embed_window, K.splice_embed, K.splice_embed_window, model.encode_image)

    def _wrap(self, fn, outer):
        def run(*a, **kw):
            if outer and self.depth:
                return fn(*a, **kw)
            self.depth += outer
            t, out = timed(lambda: fn(*a, **kw))
            self.depth -= outer
            if outer:
                self.stage += t
            else:
                self.splice += t
            return out
        return run

    def __enter__(self):
        self.model.embed_inputs = self._wrap(self.saved[0], 1)
        self.model.embed_window = self._wrap(self.saved[1], 1)
        self.model.encode_image = self._wrap(self.saved[4], 1)
        K.splice_embed, K.splice_embed_window = self._wrap(self.saved[2], 0), self._wrap(self.saved[3], 0)
        return self

    def __exit__(self, *exc):
        del self.model.embed_inputs, self.model.embed_window, self.model.encode_image
        K.splice_embed, K.splice_embed_window = self.saved[2], self.saved[3]


def report(name, ts, extra=""):
    print(f"  {name:34s}: min {min(ts):8.2f}  median {statistics.median(ts):8.2f}  max {max(ts):8.2f}{extra}", flush=True)


def split(lm, fn):
    """one more run of `fn` under the stopwatch (the decoder's one-token call inside generate embeds nothing: T = 1 comes
    from the device-side loop, not from embed_inputs)"""
    with Stopwatch(lm.model) as sw:
        fn()
    return sw.stage, sw.splice


def summary(what, off, on, s_off, s_on):
    a, b = min(off), min(on)
    vis_off, vis_on = s_off[0] - s_off[1], s_on[0] - s_on[1]
    print(f"  {what}: {a:.2f} -> {b:.2f} ms, saves {a - b:.2f} ms ({a / b:.2f}x){'' if b < a else '  NOT FASTER'}; embedding "
          f"stage {s_off[0]:.2f} -> {s_on[0]:.2f} ms: vision (tower, fuse, projector, region head) {vis_off:.2f} -> {vis_on:.2f}, "
          f"splice {s_off[1]:.2f} -> {s_on[1]:.2f}", flush=True)


def batch_arm(lm, ids, args, dtype, B, reps):
    import bench
    image, boxes, prompt = bench.make_inputs(args, ids, DEV, 1, batch=1)
    g = torch.Generator().manual_seed(11 + B)
    tails = torch.randint(3, 32000, (B, 32), generator=g).to(DEV)
    input_ids = torch.cat([prompt.expand(B, -1), tails], 1).contiguous()
    images = image.to(dtype).expand(B, -1, -1, -1).contiguous()
    kw = dict(images=images, bboxes=[boxes[0]] * B, do_sample=False, max_new_tokens=1, eos_token_id=-1, shared_prefix=True,
              return_new_tokens=True)
    res, outs, splits = {}, {}, {}
    for name, flag in (("share_images off", False), ("share_images on", True)):
        call = lambda: lm.generate(input_ids, share_images=flag, **kw)     # noqa: E731
        call()                                                             # warms up every shape of the arm
        ts = []
        for _ in range(reps):
            t, outs[name] = timed(call)
            ts.append(t)
        res[name], splits[name] = ts, split(lm, call)
        report(f"B = {B:2d}, {name}", ts, f"  (P = {lm.last_shared_prefix} of {input_ids.size(1)} positions)")
    summary(f"B = {B:2d} time to first token", res["share_images off"], res["share_images on"], splits["share_images off"],
            splits["share_images on"])
    print(f"  B = {B:2d} first tokens equal on both arms: {outs['share_images off'] == outs['share_images on']}", flush=True)


def turn_arm(lm, ids, args, dtype, reps):
    import bench
    from gpt4roi_amd.generation import GenerationSession
    image, boxes, prompt = bench.make_inputs(args, ids, DEV, 1, batch=1)
    image = image.to(dtype)
    follow = torch.randint(3, 32000, (1, 32), generator=torch.Generator().manual_seed(7)).to(DEV)
    kw = dict(images=image, bboxes=boxes, do_sample=False, eos_token_id=-1)
    full = lm.generate(prompt, max_new_tokens=64, **kw)
    answer = full[:, prompt.size(1):].clone()
    answer[answer >= ids.im_patch_token] = 3           # a random-weight model may emit <im_patch> / <bbox>; fed back they
    prompt2 = torch.cat([prompt, answer, follow], 1)   # would break the splice (tools/session_bench.py does the same)
    res, outs, splits = {}, {}, {}
    for name, cached in (("plain session", False), ("cache_image=True", True)):
        ts = []
        for r in range(reps + 2):
            s = GenerationSession(cache_image=cached)
            lm.generate(prompt, max_new_tokens=64, session=s, **kw)        # the cache as the first turn leaves it
            call = lambda: lm.generate(prompt2, max_new_tokens=1, session=s, return_new_tokens=True, **kw)     # noqa: E731
            if r == reps + 1:
                splits[name] = split(lm, call)
            else:
                t, outs[name] = timed(call)
                ts.append(t)
        res[name] = ts[1:]                                                 # the first repetition warms up
        report(f"turn 2, {name}", res[name], f"  reused {s.reused} prefilled {s.prefilled}")
    summary("turn 2 time to first token", res["plain session"], res["cache_image=True"], splits["plain session"],
            splits["cache_image=True"])
    print(f"  turn 2 first token equal on both arms: {outs['plain session'] == outs['cache_image=True']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--llama-layers", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_reuse_ab: no GPU -- timings are taken on the device or not at all")
    import bench
    from gpt4roi_amd.spi_llava import SPILlavaMPTForCausalLM
    dtype = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    args = SimpleNamespace(image_size=336, rois=32, llama_layers=a.llama_layers, batch=1)
    model, ids = bench.build_model(args, DEV, 0, dtype=dtype)
    lm = SPILlavaMPTForCausalLM(model)
    print(f"# image reuse, configs[1] geometry (336^2, 32 RoIs, 767-token prompt), {a.llama_layers}-layer synthetic decoder, "
          f"{dtype}; ms, wall clock around generate(max_new_tokens=1) + synchronize, {a.reps} repetitions after a warm-up; one box")
    with torch.inference_mode():
        for B in (int(x) for x in a.batches.split(",")):
            batch_arm(lm, ids, args, dtype, B, a.reps)
        turn_arm(lm, ids, args, dtype, a.reps)
        enc = model.encode_image(bench.make_inputs(args, ids, DEV, 1, batch=1)[0].to(dtype))
        print(f"  one EncodedImage holds {enc.nbytes() / 2 ** 20:.1f} MiB", flush=True)


if __name__ == "__main__":
    main()
