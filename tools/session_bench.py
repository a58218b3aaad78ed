#!/usr/bin/env python3
"""tools/session_bench.py -- the two measurements behind conversation sessions (DESIGN.md "Conversation sessions").

  --kernel   A/B of the split-key continuation attention (csrc/attention_cont.hip) against the prefill forward
             (K.flash_attn, what the continuation chunk ran on before) on the same inputs, per hipGraph replay:
             Tq in {8, 16, 32, 64} x Tk in {512, 1024, 2048}, H = 32, D = 128, B = 1.  The forward is timed in several
             separately captured graphs; their spread is the bar a win has to clear.
  --turn     latency of the SECOND turn of a conversation at the configs[1] geometry (336^2 image, 32 RoIs, ~767-token
             first prompt, 64 new tokens, a 32-token follow-up), with and without a GenerationSession; also with one new
             token (vision + prefill + first token, no decode loop).  Wall clock around generate() with a device
             synchronize; the decode loop inside is the captured hipGraph either way.
Prints plain text; redirect into profiles/."""
import argparse
import math
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


def graph_us(fn, iters=20, warm=3, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(reps):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e3)
    return best


def kernel_ab(dtype):
    H, D, B = 32, 128, 1
    scale = 1.0 / math.sqrt(D)
    print(f"# split-key continuation attention vs the prefill forward, H={H} D={D} B={B} {dtype}, us per launch (hipGraph replay, "
          "best of 5 replays of 20 launches); forward: min..max over 4 separately captured graphs")
    print("#  Tq    Tk   forward(min..max)   cont(best split)   splits: us ...                      verdict")
    for Tk in (512, 1024, 2048):
        for Tq in (8, 16, 32, 64):
            g = torch.Generator(device="cpu").manual_seed(Tk + Tq)
            q = (torch.randn(B, Tq, H * D, generator=g) * 0.7).to(dtype).to(DEV)
            kc = (torch.randn(B, 2048, H * D, generator=g) * 0.7).to(dtype).to(DEV)
            vc = (torch.randn(B, 2048, H * D, generator=g) * 0.7).to(dtype).to(DEV)
            k, v = kc[:, :Tk], vc[:, :Tk]
            o = torch.empty_like(q)
            base = [graph_us(lambda: K.flash_attn(q, k, v, H, scale, True, out=o)) for _ in range(4)]
            res = {}
            for S in (2, 4, 8, 16):
                if S > -(-Tk // 64):
                    continue
                work = K.ContAttnWorkspace(H, D, DEV, splits=S, batch=B)
                res[S] = graph_us(lambda: K.flash_attn_cont(q, k, v, H, scale, work=work, out=o, splits=S))
            dflt = K.cont_splits(H, B, Tk)
            best = min(res, key=res.get)
            spread = max(base) - min(base)
            wins = res[dflt] < min(base) - spread
            print(f"  {Tq:4d} {Tk:5d}   {min(base):7.1f}..{max(base):7.1f}   {res[best]:7.1f} (S={best:2d})   "
                  + "  ".join(f"{S}: {us:6.1f}" for S, us in res.items())
                  + f"   default S={dflt}: {'WIN' if wins else 'no win'} ({min(base) / res[dflt]:.2f}x)", flush=True)


def turn_latency(dtype, reps):
    import bench
    from gpt4roi_amd.generation import GenerationSession
    from gpt4roi_amd.spi_llava import SPILlavaMPTForCausalLM
    args = SimpleNamespace(image_size=336, rois=32, llama_layers=32, batch=1)
    model, ids = bench.build_model(args, DEV, 0, dtype=dtype)
    lm = SPILlavaMPTForCausalLM(model)
    image, boxes, prompt = bench.make_inputs(args, ids, DEV, 1, batch=1)
    g = torch.Generator().manual_seed(7)
    follow = torch.randint(3, 32000, (1, 32), generator=g).to(DEV)
    print(f"# second turn of a conversation, configs[1] geometry, {dtype}: first prompt {prompt.size(1)} tokens, 64 new tokens, "
          f"follow-up of 32 tokens; ms, wall clock around generate() + synchronize (vision path, splice, the session's "
          f"image compare, prefill and decode loop), {reps} repetitions")

    def first_turn(session):
        return lm.generate(prompt, images=image, bboxes=boxes, do_sample=False, max_new_tokens=64, session=session,
                           eos_token_id=-1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.inference_mode():
        full = first_turn(None)
        answer = full[:, prompt.size(1):].clone()
        special = answer >= ids.im_patch_token                 # a random-weight model may emit <im_patch> / <bbox>: fed back
        answer[special] = 3                                    # they would break the splice; the common prefix ends there
        if bool(special.any()):
            print(f"  ({int(special.sum())} special ids among the 64 generated ones replaced in the follow-up prompt)")
        prompt2 = torch.cat([prompt, answer, follow], 1)
        for n_new in (64, 1):
            rows = {}
            for mode in ("no session", "session"):
                ts, outs = [], []
                for _ in range(reps + 1):
                    s = GenerationSession() if mode == "session" else None
                    first_turn(s)                                          # the cache as the first turn leaves it
                    t, out = timed(lambda: lm.generate(prompt2, images=image, bboxes=boxes, do_sample=False,
                                                       max_new_tokens=n_new, session=s, eos_token_id=-1))
                    ts.append(t)
                    outs.append(out)
                ts = ts[1:]                                                # the first repetition warms up
                rows[mode] = (ts, outs[-1], s)
                extra = f"  reused {s.reused} prefilled {s.prefilled}" if s is not None else ""
                print(f"  turn 2, {n_new:2d} new tokens, {mode:10s}: min {min(ts):8.2f}  median {statistics.median(ts):8.2f}  "
                      f"max {max(ts):8.2f}{extra}", flush=True)
            same = torch.equal(rows["session"][1], rows["no session"][1])
            a, b = min(rows["no session"][0]), min(rows["session"][0])
            print(f"  turn 2, {n_new:2d} new tokens: session saves {a - b:.2f} ms ({a / b:.2f}x); same ids: {same}", flush=True)
        t1 = [timed(lambda: first_turn(None))[0] for _ in range(reps)]
        print(f"  turn 1 (for scale), 64 new tokens: min {min(t1):8.2f}  median {statistics.median(t1):8.2f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--turn", action="store_true")
    ap.add_argument("--dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    if a.kernel:
        kernel_ab(dt)
    if a.turn:
        turn_latency(dt, a.reps)
