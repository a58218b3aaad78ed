"""tools/shared_prefix_ab.py -- A/B of the shared-prefix batched decode (LlamaDecoder.decode_graph_batch(shared_prefix=P),
csrc/attention_shared.hip) at LLaMA-7B shapes: B rows that share a prefix of P positions and own 167 more.

Two measurements, both in one process with the arms interleaved and every point repeated `--rounds` (>= 3) times:
  attention  the decode-attention launch alone: a captured graph of 32 launches (one per layer, each layer its own K/V cache,
             as in the decoder, so nothing is served from a cache the real step would not have) replayed `--replays` times
             between two device events -> us per launch.  Arms: the per-row ragged kernel (attn_decode) | the shared kernel.
  model      the whole step by hipGraph replay on a synthetic 7B decoder, (t(tokens + 2) - t(2)) / tokens -> ms per step, and
             the time to the first token t(1).  Arms: masked = today's batch (B full prefills, per-row attention) | ragged =
             the shared path with the attention pinned to the existing ragged kernel | shared = the shared path with the
             new kernel.  The time to the first token here is the DECODER's prefill (+ one token selection): the tool has no
             vision tower, and in generate() the vision path still runs per row in front of it on every arm.
A row of the table is one (B, P); `spread` is max - min over the rounds of an arm.  kernels.shared_attn_wins is derived from
the table: the new kernel is routed only where it beats the existing one by more than the larger spread at that point.
    python tools/shared_prefix_ab.py [--mode attention|model|both] [--batches 2,4,8,16,32] [--prefixes 64,256,600,1500]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OWN = 167
H, D, LAYERS = 32, 128, 32


def _stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 3), spread=round(xs[-1] - xs[0], 3), n=len(xs))


def attention_ab(K, dev, B, P, rounds, replays, dtype=torch.bfloat16):
    """us per launch of the two decode-attention kernels at (B, P): 32 layers' caches, graph replay, device events."""
    HD, n = H * D, P + OWN
    t_max = n + 8
    g = torch.Generator(device="cpu").manual_seed(B * 10007 + P)
    kc = torch.empty((LAYERS, B, t_max, HD), dtype=dtype, device=dev).normal_()
    vc = torch.empty_like(kc).normal_()
    kc[:, 1:, :P] = kc[:, :1, :P]
    vc[:, 1:, :P] = vc[:, :1, :P]
    qkv = torch.randn(B, 3 * HD, generator=g).to(dtype).to(dev)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(t_max, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = ang.cos().to(dev).contiguous(), ang.sin().to(dev).contiguous()
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    plen = torch.tensor([P], dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    w_old = K.DecodeAttnWorkspace(H, D, dev, splits=max(1, min(8, 512 // (H * B))), batch=B)
    w_new = K.SharedAttnWorkspace(H, D, dev, splits=K.shared_attn_splits(H, B), batch=B)
    out = torch.empty((B, HD), dtype=dtype, device=dev)

    def old():
        for li in range(LAYERS):
            K.attn_decode(None, kc[li], vc[li], H, scale, w_old, out=out, qkv=qkv, cos=cos, sin=sin, kv_lens_dev=lens)

    def new():
        for li in range(LAYERS):
            K.attn_decode_shared(qkv, kc[li], vc[li], H, scale, w_new, cos, sin, lens, plen, out=out)

    graphs, outs = {}, {}
    for name, fn in (("ragged", old), ("shared", new)):
        fn()                                                  # warm up (loads the code object)
        torch.cuda.synchronize()
        outs[name] = out.float().clone()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        graphs[name] = gr
    err = float((outs["ragged"] - outs["shared"]).abs().max())
    us = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, gr in graphs.items():                       # interleaved
            gr.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / (replays * LAYERS))
    return dict(B=B, P=P, keys=n + 1, us_per_launch={k: _stats(v) for k, v in us.items()}, max_abs_diff=round(err, 5),
                splits=dict(ragged=w_old.splits, shared=w_new.splits))


def model_ab(K, dec, dev, B, P, rounds, tokens):
    hidden = dec.hidden
    g = torch.Generator(device="cpu").manual_seed(B * 7919 + P)
    emb = (torch.randn(B, P + OWN, hidden, generator=g) * 0.02).to(dec.dtype).to(dev)
    emb[1:, :P] = emb[:1, :P]
    arms = {"masked": dict(), "ragged": dict(shared_prefix=P, route="never"), "shared": dict(shared_prefix=P, route="always")}
    step, ttft, ids = {k: [] for k in arms}, {k: [] for k in arms}, {}

    def call(kw, n):
        kw = dict(kw)
        K.SHARED_ATTN_ROUTE = kw.pop("route", "rule")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec.decode_graph_batch(emb, n, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for name, kw in arms.items():                             # warm up every shape and capture the graphs
        ids[name] = call(kw, tokens + 2)[1]
    for _ in range(rounds):
        for name, kw in arms.items():                         # interleaved
            t_long, t_two, t_one = call(kw, tokens + 2)[0], call(kw, 2)[0], call(kw, 1)[0]
            step[name].append((t_long - t_two) / tokens * 1e3)
            ttft[name].append(t_one * 1e3)
    K.SHARED_ATTN_ROUTE = "rule"
    return dict(B=B, P=P, prompt=P + OWN, ms_per_step={k: _stats(v) for k, v in step.items()},
                ms_to_first_token_decoder_only={k: _stats(v) for k, v in ttft.items()},
                ids_shared_equal_ragged=ids["shared"] == ids["ragged"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both", choices=["attention", "model", "both"])
    ap.add_argument("--batches", default="2,4,8,16,32")
    ap.add_argument("--prefixes", default="64,256,600,1500")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds: every point is repeated at least three times")
    if not torch.cuda.is_available():
        raise SystemExit("shared_prefix_ab: no GPU -- timings are taken on the device or not at all")
    from gpt4roi_amd import kernels as K
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    grid = [(B, P) for B in (int(x) for x in a.batches.split(",")) for P in (int(x) for x in a.prefixes.split(","))]

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.mode in ("attention", "both"):
        for B, P in grid:
            emit(dict(kind="attention", **attention_ab(K, dev, B, P, a.rounds, a.replays)))
            torch.cuda.empty_cache()
    if a.mode in ("model", "both"):
        from gpt4roi_amd import synthetic as syn
        from gpt4roi_amd.llama import LlamaDecoder
        l = syn.LLAMA_7B
        lsd = syn.llama_state(l["hidden"], l["inter"], LAYERS, 32006, seed=1, device=dev, dtype=torch.bfloat16)
        dec = LlamaDecoder(lsd, heads=l["heads"], max_positions=2048, device=dev)
        del lsd
        for B, P in grid:
            emit(dict(kind="model", **model_ab(K, dec, dev, B, P, a.rounds, a.tokens)))


if __name__ == "__main__":
    main()
