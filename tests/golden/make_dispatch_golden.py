"""tests/golden/make_dispatch_golden.py -- the launch sequence of kernels.gemm() over a sweep of shapes, traced WITHOUT a GPU,
written to tests/golden/gemm_dispatch.json.  The committed file was produced by this script at commit 8ecf09f ("Batched
generate() with sampling and per-sequence stopping criteria"), the last one whose gemm() took its routing decisions in a
ladder of its own; tests/test_dispatch_cpu.py replays the trace on the working tree and compares every case.

How: the operands are `meta` tensors (shapes and strides, no memory), `_lib.require_gpu` / `_stream` are stubbed, `_p` returns
the tensor's storage offset instead of its address and `_launch` records its arguments instead of calling the library.

Per shape (M, N, K) of the sweep, one line:
    [M, N, K, queries at BIG_TILE 34, queries at 24, crc, unique launch lists, which of them each variant ran]
  queries    "long_k_plan,small_m_split_plan,decode_split_plan,gemv_batch_wins": TILExSLICES or - (None), then 0 / 1
  variants   BIG_TILE (34, 24) x output (16-bit, fp32) x residual (without, with), in that nesting order: one digit each
  a launch   t<tile>:<n0>:<columns>:<K slices> (g4r_gemm_bf16_nt) or g:<n0>:<columns> (g4r_gemv_batch_bf16) for the weight rows
             [n0, n0 + columns); the tracer checks that bias / residual / out start at the same column (out at half of it
             under swiglu) and that M, K, the row strides, the activation and the fp32 flag are the call's
  crc        zlib.crc32 of the profiler tags (with shapes), flops and byte counts of the eight variants' launches
The `extra` cases (swiglu column splits, operands the weight-streaming kernel must refuse, explicit tile_cfg / splits /
workspace) are real CPU tensors where an address matters, and record every launch raw:
    <t|g>:M:N:K:tile:slices:fp32:act then a, w, out, bias, residual, workspace (- = absent) as storage offsets (meta
    tensors) or addresses modulo 64 (CPU tensors).

Run from the repository root:  python tests/golden/make_dispatch_golden.py
"""
import json
import os
import sys
import zlib
from contextlib import contextmanager

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gpt4roi_amd import _lib  # noqa: E402
from gpt4roi_amd import kernels as K  # noqa: E402

MS = (1, 2, 3, 4, 5, 8, 16, 32, 64, 65, 128, 577, 767, 1024, 1534, 2301, 3068, 4616, 5592, 6136, 9232, 12272)
NS = (256, 1024, 1280, 2816, 3072, 4096, 10246, 11008, 12288, 22016, 32006)
KS = (448, 512, 1000, 1024, 2048, 4000, 4096, 8192, 11008, 12288, 22016)
BIGS = (34, 24)
VARIANTS = [(big, fp32, res) for big in BIGS for fp32 in (False, True) for res in (False, True)]
BF = torch.bfloat16


@contextmanager
def traced(big=34):
    """gemm() with its GPU ends replaced: yields the list the launches are appended to."""
    log = []
    saved = (_lib.require_gpu, K._stream, K._p, K._launch, K.BIG_TILE, K.PROFILER.detail)
    _lib.require_gpu = lambda t: None
    K._stream = lambda t: 0
    K._p = lambda t: None if t is None else t.storage_offset() if t.device.type == "meta" else t.data_ptr() % 64
    K._launch = lambda name, args, tag=None, flops=0.0, nbytes=0.0, dt=None: log.append((name, args, tag, flops, nbytes))
    K.BIG_TILE, K.PROFILER.detail = big, True
    try:
        yield log
    finally:
        _lib.require_gpu, K._stream, K._p, K._launch, K.BIG_TILE, K.PROFILER.detail = saved


def fields(name, args):
    """-> dict of what a recorded launch was given, for either entry point"""
    if name == "g4r_gemm_bf16_nt":
        a, w, out, bias, res, ws, M, N, Kd, lda, ldw, ldo, ldr, act, fp32, splits, tile, _ = args
        return dict(kind="t", M=M, N=N, K=Kd, tile=tile, splits=splits, fp32=fp32, act=act, a=a, w=w, out=out, bias=bias,
                    res=res, ws=ws, lda=lda, ldw=ldw, ldo=ldo, ldr=ldr)
    assert name == "g4r_gemv_batch_bf16", name
    a, M, lda, gamma, _, w, out, ldo, bias, res, ldr, N, Kd, ldw, act, fp32, variant, _ = args
    assert gamma is None and variant == K.GEMV_BATCH_VARIANT
    return dict(kind="g", M=M, N=N, K=Kd, tile="", splits=1, fp32=fp32, act=act, a=a, w=w, out=out, bias=bias, res=res,
                ws=None, lda=lda, ldw=ldw, ldo=ldo, ldr=ldr)


def raw(name, args):
    f = fields(name, args)
    o = lambda v: "-" if v is None else str(v)
    return ":".join([f["kind"]] + [str(f[k]) for k in ("M", "N", "K", "tile", "splits", "fp32", "act")]
                    + [o(f[k]) for k in ("a", "w", "out", "bias", "res", "ws")])


def cols(name, args, M, N, Kd, fp32, res, act=None):
    """The launch as a column range of a gemm() call on contiguous operands [M,K] x [N,K] (+ bias [N], residual [M,N])."""
    f = fields(name, args)
    n_out = N // 2 if act == "swiglu" else N
    assert (f["M"], f["K"], f["lda"], f["ldw"], f["ldo"], f["a"]) == (M, Kd, Kd, Kd, n_out, 0), f
    assert f["act"] == K.ACT[act] and f["fp32"] == int(fp32) and f["w"] % Kd == 0
    n0 = f["w"] // Kd
    assert 0 <= n0 and n0 + f["N"] <= N and f["bias"] == n0 and f["out"] == (n0 // 2 if act == "swiglu" else n0)
    assert (f["res"], f["ldr"]) == ((n0, N) if res else (None, 0))
    assert (f["ws"] is None) == (f["splits"] == 1) and f["ws"] in (None, 0)
    return f"t{f['tile']}:{n0}:{f['N']}:{f['splits']}" if f["kind"] == "t" else f"g:{n0}:{f['N']}"


def run_meta(M, N, Kd, big, fp32, res, act=None):
    """gemm() without hints on contiguous meta operands -> ([launch strings], [(tag, flops, nbytes)])"""
    a = torch.empty((M, Kd), dtype=BF, device="meta")
    w = torch.empty((N, Kd), dtype=BF, device="meta")
    bias = torch.empty((N,), dtype=torch.float32, device="meta")
    r = out = None
    if res:
        # meta tensors all report address 0; where gemm() asks whether residual and out are one buffer (few rows), give it two
        r = torch.empty((M, N), dtype=BF, device="meta" if M > 16 else "cpu")
        if M <= 16:
            out = torch.empty((M, N // 2 if act == "swiglu" else N), dtype=torch.float32 if fp32 else BF)
    with traced(big) as log:
        K.gemm(a, w, bias=bias, residual=r, act=act, out=out, out_dtype=torch.float32 if fp32 else None)
    return [cols(n, args, M, N, Kd, fp32, res, act) for n, args, *_ in log], [list(rec[2:]) for rec in log]


def fmt_plan(p):
    return "-" if p is None else f"{p[0]}x{p[1]}"


def queries(M, N, Kd, big):
    saved, K.BIG_TILE = K.BIG_TILE, big
    try:
        return ",".join([fmt_plan(K.long_k_plan(M, N, Kd)), fmt_plan(K.small_m_split_plan(M, N, Kd)),
                         fmt_plan(K.decode_split_plan(M, N, Kd)), str(int(bool(K.gemv_batch_wins(M, N, Kd))))])
    finally:
        K.BIG_TILE = saved


def sweep_case(M, N, Kd):
    uniq, idx, prof = [], "", []
    for big, fp32, res in VARIANTS:
        launches, p = run_meta(M, N, Kd, big, fp32, res)
        s = " ".join(launches)
        if s not in uniq:
            uniq.append(s)
        idx += str(uniq.index(s))
        prof.append(p)
    crc = zlib.crc32(json.dumps(prof).encode())
    return [M, N, Kd, queries(M, N, Kd, 34), queries(M, N, Kd, 24), crc, uniq, idx]


def _cpu(shape, dtype=BF, offset=0, row_pad=0):
    """A real CPU tensor whose address is 64-byte aligned + 2 * offset bytes and whose rows are row_pad elements apart more
    than they are long."""
    rows, width = (shape[0], shape[1] + row_pad) if len(shape) == 2 else (1, shape[0])
    buf = torch.zeros(rows * width + 64, dtype=dtype)
    lead = (-buf.data_ptr() % 64) // buf.element_size()
    t = buf[lead + offset: lead + offset + rows * width]
    assert t.data_ptr() % 64 == (offset * buf.element_size()) % 64
    return t.view(rows, width)[:, :shape[1]] if len(shape) == 2 else t


def extra_cases():
    """-> [[name, [raw launches]]]"""
    out = []

    def rec(name, log):
        out.append([name, [raw(n, args) for n, args, *_ in log]])

    for big in BIGS:
        for M in (767, 3068, 12272):
            for fp32 in (False, True):
                launches, _ = run_meta(M, 22016, 4096, big, fp32, False, act="swiglu")
                out.append([f"swiglu {M}x22016x4096 big{big} fp32={int(fp32)}", launches])
    # few rows: what the weight-streaming kernel takes, and each operand property that sends the call on to the tiles
    for M, N, Kd in ((2, 256, 4096), (4, 512, 512), (3, 256, 8192)):
        for what in ("aligned", "a row stride K+4", "a row stride 0", "a address +2 bytes", "w address +2 bytes",
                     "w row stride K+4", "residual is out", "residual is not out"):
            a = _cpu((M, Kd), offset=1 if what.startswith("a address") else 0, row_pad=4 if what.startswith("a row stride K") else 0)
            if what == "a row stride 0":
                a = _cpu((1, Kd)).expand(M, Kd)
            w = _cpu((N, Kd), offset=1 if what.startswith("w address") else 0, row_pad=4 if what.startswith("w row") else 0)
            o = _cpu((M, N))
            r = o if what == "residual is out" else _cpu((M, N)) if what == "residual is not out" else None
            with traced() as log:
                K.gemm(a, w, residual=r, out=o)
            rec(f"few rows {M}x{N}x{Kd}: {what}", log)
    # explicit tile_cfg / splits / workspace: no planning
    def meta(*shape, dtype=BF):
        return torch.empty(shape, dtype=dtype, device="meta")
    for name, (M, N, Kd), kw in (
            ("tile_cfg=0 on a shape that splits columns", (767, 22016, 4096), dict(tile_cfg=0)),
            ("tile_cfg=7", (767, 4096, 11008), dict(tile_cfg=7)),
            ("splits=3", (767, 4096, 4096), dict(splits=3)),
            ("splits=2 on a shape that splits columns", (767, 22016, 4096), dict(splits=2)),
            ("tile_cfg=34 splits=2", (1534, 4096, 11008), dict(tile_cfg=34, splits=2)),
            ("tile_cfg=14 few rows", (4, 4096, 4096), dict(tile_cfg=14)),
            ("splits=2 few rows", (4, 4096, 4096), dict(splits=2)),
            ("workspace few rows", (4, 4096, 4096), dict(workspace=meta(5, 4, 4096, dtype=torch.float32)[1:])),
            ("workspace long K", (767, 4096, 11008), dict(workspace=meta(5, 767, 4096, dtype=torch.float32)[1:])),
            ("workspace on a shape that splits columns", (767, 22016, 4096),
             dict(workspace=meta(5, 767, 22016, dtype=torch.float32)[1:])),
            ("workspace splits=2 tile_cfg=0", (767, 4096, 4096),
             dict(workspace=meta(3, 767, 4096, dtype=torch.float32)[1:], splits=2, tile_cfg=0))):
        with traced() as log:
            K.gemm(meta(M, Kd), meta(N, Kd), bias=meta(N, dtype=torch.float32), residual=meta(M, N), **kw)
        rec(f"{name} {M}x{N}x{Kd}", log)
    return out


def trace_all():
    return dict(shapes=[sweep_case(M, N, Kd) for M in MS for N in NS for Kd in KS], extra=extra_cases())


def main():
    got = trace_all()
    plain = [len(c[6][int(c[7][i])].split(" ")) for c in got["shapes"] for i in (0, 2)]          # BIG_TILE 34, no residual
    print(f"plain sweep: {len(plain)} cases, {plain.count(1)} single-launch, {plain.count(2)} two-launch, "
          f"{len(plain) - plain.count(1) - plain.count(2)} other")
    path = os.path.join(HERE, "gemm_dispatch.json")
    with open(path, "w") as f:
        f.write('{"commit": "8ecf09f", "generator": "tests/golden/make_dispatch_golden.py",\n "shapes": [\n')
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in got["shapes"]))
        f.write('\n ],\n "extra": [\n')
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in got["extra"]))
        f.write("\n ]}\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(got['shapes'])} shapes x {len(VARIANTS)} variants, {len(got['extra'])} extra")


if __name__ == "__main__":
    main()
