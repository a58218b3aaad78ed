"""tools/sample_batch_time.py -- cost of sampling in the batched decode: the hipGraph step of LlamaDecoder.decode_graph_batch on
full-width synthetic LLaMA-7B weights (fp16, the reference's serving dtype), greedy (argmax_rows + batch_advance) against
sampled (sample_rows at temperature 0.2, top-k 50 + batch_advance), and the g4r_sample_rows_f32 launch alone next to
g4r_argmax_rows_f32, at each batch size.
    python tools/sample_batch_time.py [--batches 1,8,16,32] [--tokens 64] [--prompt 128] [--rounds 2] [--out FILE]
Step time = (decode of tokens + 2 steps - decode of 2 steps) / tokens, best of `rounds` alternating greedy / sampled runs."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _launch_us(fn, n=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16,32")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd import synthetic as syn
    from gpt4roi_amd.llama import LlamaDecoder
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    dt = torch.float16
    l = syn.LLAMA_7B
    V = 32006
    batches = [int(x) for x in a.batches.split(",")]
    lsd = syn.llama_state(l["hidden"], l["inter"], 32, V, seed=1, device=dev, dtype=dt)
    dec = LlamaDecoder(lsd, heads=l["heads"], max_positions=-(-(a.prompt + a.tokens + 8) // 256) * 256, device=dev, dtype=dt,
                       max_batch=max(batches))
    del lsd
    sampler = (0.2, 50, 1.0)
    rows = []
    for B in batches:
        g = torch.Generator(device=dev).manual_seed(B)
        emb = (torch.randn(B, a.prompt, l["hidden"], device=dev, generator=g) * 0.02).to(dt)
        modes = {"greedy": dict(), "sampled": dict(sampler=sampler, seeds=7, check_every=a.tokens + 2)}
        for kw in modes.values():
            dec.decode_graph_batch(emb, a.tokens + 2, **kw)                  # warm-up + capture
        best = {m: [1e9, 1e9] for m in modes}
        for _ in range(a.rounds):
            for m, kw in modes.items():
                for i, n in enumerate((a.tokens + 2, 2)):
                    best[m][i] = min(best[m][i], _timed(lambda: dec.decode_graph_batch(emb, n, **kw)))
        step_ms = {m: (best[m][0] - best[m][1]) / a.tokens * 1e3 for m in modes}
        # the selection launches alone, on logits of the decode's shape
        logits = torch.randn(B, V, device=dev, generator=g) * 3
        temp = torch.full((B,), sampler[0], device=dev)
        topk = torch.full((B,), sampler[1], dtype=torch.int32, device=dev)
        topp = torch.full((B,), sampler[2], device=dev)
        seed = torch.arange(B, dtype=torch.int64, device=dev) + 11
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty(B, dtype=torch.int64, device=dev)
        us_sample = _launch_us(lambda: K.sample_rows(logits, temp, topk, topp, seed, step, out=out))
        us_argmax = _launch_us(lambda: K.argmax_rows(logits))
        r = dict(B=B, greedy_step_ms=round(step_ms["greedy"], 4), sampled_step_ms=round(step_ms["sampled"], 4),
                 sampled_minus_greedy_us=round((step_ms["sampled"] - step_ms["greedy"]) * 1e3, 1),
                 sample_rows_us=round(us_sample, 1), argmax_rows_us=round(us_argmax, 1), tokens=a.tokens,
                 prompt=a.prompt, dtype="fp16", sampler=list(sampler))
        rows.append(r)
        print(json.dumps(r), flush=True)
        dec._bstate = {}                                                  # graphs of this B hold its workspaces
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
