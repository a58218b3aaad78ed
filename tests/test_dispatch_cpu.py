"""CPU: the tile / split dispatch of the production shapes (pure host logic in gpt4roi_amd/kernels.py).  Every decision below
was taken from an A/B measurement on MI355X (profiles/r02_gemm_tiles.md, r02_gemm_small_m.txt, r02_conv_k_order.jsonl,
r05_w4k64_epilogue.txt: tile 34 replaces the ring ping-pong tile 24 on the 256 x 256 shapes); this test pins them so that a heuristic edit for one shape cannot silently move another."""
import importlib.util
import json
import os

import pytest
import torch

from gpt4roi_amd import kernels as K


@pytest.mark.parametrize("M,N,Kd,tile,main", [
    (767, 12288, 4096, 34, None),      # LLaMA fused qkv: 144 one-wave-per-SIMD tiles (round 5: 82.6 us vs 95.5 on 192 x 256 ring tiles)
    (767, 22016, 4096, 0, 21760),      # gate|up: whole-wave column split, 255 tiles on the ring kernel + 256 columns
    (767, 32006, 4096, 0, 21760),      # lm_head
    (767, 4096, 4096, 7, None),        # o_proj: 128x128 x 8 waves, ring of 4
    (767, 256, 4096, 14, None),        # the gate|up remainder: 64x64 ring-4 (+ 2 K slices in gemm())
    (577, 3072, 1024, 14, None), (577, 1024, 1024, 14, None), (577, 4096, 1024, 13, None), (577, 1024, 4096, 14, None),  # ViT, batch 1
    (4616, 3072, 1024, 34, None), (4616, 1024, 4096, 0, None),                                                           # ViT, batch 8
    (12272, 12288, 4096, 34, None), (12272, 4096, 4096, 34, None), (12272, 22016, 4096, 34, 21760), (12272, 4096, 11008, 34, None),   # 16 merged requests (bench default): the one-wave-per-SIMD 256 x 256 tile (round 5) in whole waves
    (9232, 3072, 1024, 34, None), (9232, 4096, 1024, 34, None), (9232, 1024, 4096, 34, None),                                          # ViT, batch 16
    (8, 12288, 4096, 14, None), (8, 4096, 4096, 14, None), (8, 22016, 4096, 13, None), (16, 4096, 11008, 14, None),      # batched decode
])
def test_gemm_tile_dispatch(M, N, Kd, tile, main):
    assert K.pick_tile(M, N, Kd) == tile
    assert K.wave_split(M, N, Kd) == main


@pytest.mark.parametrize("M,N,Kd,want", [
    (5592, 1280, 11008, (34, 2)), (5592, 1280, 22016, (34, 2)), (5592, 1280, 12288, (34, 2)),   # training-batch column remainders
    (5592, 1280, 4096, None),          # K = 4096: the two-stage tile is as fast
    (767, 4096, 11008, None),          # down_proj at batch 1: long_k_plan's shape (48 tiles), not this one
    (767, 10246, 4096, None),          # lm_head remainder
    (5592, 2816, 11008, None),         # 242 tiles: a full wave on its own
])
def test_partial_wave_plan(M, N, Kd, want):
    assert K.partial_wave_plan(M, N, Kd) == want


@pytest.mark.parametrize("M,Cout,Kd,want", [
    (36864, 1024, 9216, (34, 1)),      # a 192^2 level on its own (the fuse rounds use conv3x3_mlvl: one launch for all levels)
    (2304, 1024, 9216, (4, 1)),
    (6272, 1024, 36864, (34, 2)),      # pconv, 32 RoIs: 100 tiles x 2 K slices
    (15288, 1024, 36864, (34, 1)),     # pconv, training batch (78 RoIs)
])
def test_conv_tile_dispatch(M, Cout, Kd, want):
    assert K.pick_conv_tile(M, Cout, Kd) == want


def test_mlvl_geometry_of_the_336_pyramid_is_three_full_waves():
    rows = sum(h * h for h in (192, 96, 48, 24))
    assert rows == 48960 and -(-rows // 256) * (1024 // 256) == 768 == 3 * 256
    for start in (192 * 192, 192 * 192 + 96 * 96, 192 * 192 + 96 * 96 + 48 * 48):
        assert start % 256 == 0                                   # level boundaries fall on tile boundaries at P = 24


def test_mlvl_maps_layout_is_level_major_with_contiguous_per_level_views():
    """kernels.MlvlMaps: the buffer conv3x3_mlvl reads / writes -- [level][b][y][x][C] in one allocation, each level a
    contiguous NHWC view at the row offset the kernel's level table assumes."""
    import torch
    m = K.MlvlMaps(2, [(6, 5), (3, 3), (2, 1)], 8, "cpu", dtype=torch.float32)
    rows = [2 * 6 * 5, 2 * 3 * 3, 2 * 2 * 1]
    assert m.flat.shape == (sum(rows), 8) and [tuple(v.shape) for v in m.levels] == [(2, 6, 5, 8), (2, 3, 3, 8), (2, 2, 1, 8)]
    off = 0
    for v, n in zip(m.levels, rows):
        assert v.is_contiguous() and v.data_ptr() == m.flat[off].data_ptr()
        off += n
    m.levels[1][1, 2, 0, 3] = 7.0                                 # level 1, image 1, y 2, x 0 -> flat row 60 + 9 + 6
    assert float(m.flat[60 + 9 + 6, 3]) == 7.0
    assert list(m._hw[0]) == [6, 3, 2] and list(m._hw[1]) == [5, 3, 1]


# ---- gemm(): one routing plan (kernels.gemm_plan), replayed against the launches recorded before it existed ----

@pytest.fixture(scope="module")
def tracer(golden_dir):
    """tests/golden/make_dispatch_golden.py: runs gemm() on meta / CPU operands with the launch recorded instead of issued"""
    spec = importlib.util.spec_from_file_location("make_dispatch_golden", os.path.join(golden_dir, "make_dispatch_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "gemm_dispatch.json")) as f:
        return json.load(f)


def _plan_strings(plan):
    return [f"g:{p.n0}:{p.n1 - p.n0}" if p.kernel == "gemv_batch" else f"t{p.tile}:{p.n0}:{p.n1 - p.n0}:{p.splits}" for p in plan]


def test_gemm_issues_the_recorded_launches_for_every_case(tracer, golden):
    """Every case of the golden sweep (2662 shapes x BIG_TILE 34 / 24 x 16-bit / fp32 output x without / with residual, the swiglu
    column splits, the operands the weight-streaming kernel refuses, the explicit tile_cfg / splits / workspace calls): the same
    entry points with the same sizes, column offsets, tiles, K slices, profiler tags, flops and byte counts, and the same
    answers of long_k_plan / small_m_split_plan / decode_split_plan / gemv_batch_wins."""
    got = tracer.trace_all()
    assert len(got["shapes"]) == len(golden["shapes"]) == len(tracer.MS) * len(tracer.NS) * len(tracer.KS)
    assert len(got["extra"]) == len(golden["extra"])
    for g, w in zip(got["shapes"] + got["extra"], golden["shapes"] + golden["extra"]):
        assert g == w
    plain = [len(c[6][int(c[7][i])].split(" ")) for c in golden["shapes"] for i in (0, 2)]
    assert (plain.count(1), plain.count(2)) == (5198, 126)


def test_the_plan_is_what_gemm_runs(tracer, golden, monkeypatch):
    """gemm_plan's launch list equals the launches recorded from gemm(), for every case of the sweep and for the extra cases
    that go through the planner."""
    for M, N, Kd, _, _, _, uniq, idx in golden["shapes"]:
        for (big, fp32, _), i in zip(tracer.VARIANTS, idx):
            monkeypatch.setattr(K, "BIG_TILE", big)
            assert " ".join(_plan_strings(K.gemm_plan(M, N, Kd, fp32_out=fp32, gemv_ok=True))) == uniq[int(i)], (M, N, Kd, big, fp32)
    n_extra = 0
    for name, launches in golden["extra"]:
        what, shape = name.split(" ")[0], [w for w in name.replace(":", "").split(" ") if w.count("x") == 2][0]
        M, N, Kd = (int(v) for v in shape.split("x"))
        if what == "swiglu":                         # (the activation does not enter the plan: the weight rows are what it splits)
            monkeypatch.setattr(K, "BIG_TILE", int(name.split("big")[1][:2]))
            assert _plan_strings(K.gemm_plan(M, N, Kd, fp32_out=name.endswith("fp32=1"), gemv_ok=True)) == launches, name
            n_extra += 1
        elif what == "few":
            monkeypatch.setattr(K, "BIG_TILE", 34)
            f = launches[0].split(":")
            plan = K.gemm_plan(M, N, Kd, fp32_out=False, gemv_ok=f[0] == "g")
            assert len(launches) == len(plan) == 1 and plan[0].kernel == ("gemv_batch" if f[0] == "g" else "tile")
            assert f[0] == "g" or (plan[0].tile, plan[0].splits) == (int(f[4]), int(f[5])), name
            n_extra += 1
    assert n_extra == 12 + 24


def test_the_look_ahead_queries_answer_as_before_on_every_shape(tracer, golden):
    """What llama.py (long_k_plan, decode_split_plan, gemv_batch_wins) and vit.py (small_m_split_plan) ask before they fuse a
    K-slice reduce with the next norm: the recorded answer for each of the 2662 shapes at both BIG_TILE values.  With the test
    above, no caller can be told anything but what gemm() runs."""
    for M, N, Kd, q34, q24, *_ in golden["shapes"]:
        assert (tracer.queries(M, N, Kd, 34), tracer.queries(M, N, Kd, 24)) == (q34, q24), (M, N, Kd)
    assert K.long_k_plan(767, 4096, 11008) == (34, 4) and K.long_k_plan(1534, 4096, 11008) is None     # two merged requests: not fused
    assert K.gemm_plan(1534, 4096, 11008)[0].rule == "partial_wave"
    assert K.small_m_split_plan(577, 1024, 4096) == (14, 2) and K.decode_split_plan(8, 4096, 11008) == (14, 4)


def test_gemv_batch_ok_refuses_operands_the_kernel_cannot_read():
    def t(rows, cols, width=None, offset=0):
        """bf16 [rows, cols] at a 64-byte aligned address + 2 * offset bytes, rows `width` elements apart"""
        width = width or cols
        buf = torch.zeros(rows * width + 64, dtype=torch.bfloat16)
        lead = (-buf.data_ptr() % 64) // 2 + offset
        return buf[lead:lead + rows * width].view(rows, width)[:, :cols]
    x, w, out = t(4, 4096), t(256, 4096), t(4, 256)
    assert K.gemv_batch_wins(4, 256, 4096)
    assert K.gemv_batch_ok(x, w) and K.gemv_batch_ok(x, w, residual=t(4, 256), out=out) and K.gemv_batch_ok(x, w, out=out)
    assert K.gemv_batch_ok(t(4, 4096, width=4104), w)                  # padded rows, still in 16-byte pieces
    assert not K.gemv_batch_ok(t(4, 4096, width=4100), w)              # odd row stride
    assert not K.gemv_batch_ok(x, t(256, 4096, width=4100))
    assert not K.gemv_batch_ok(t(1, 4096).expand(4, 4096), w)          # stride(0) < K
    assert not K.gemv_batch_ok(t(4, 4096, offset=1), w)                # address not a multiple of 16
    assert not K.gemv_batch_ok(t(4, 4096, offset=4), w)
    assert not K.gemv_batch_ok(x, t(256, 4096, offset=1))
    assert not K.gemv_batch_ok(x, w, residual=out, out=out)            # residual aliasing out
    assert not K.gemv_batch_ok(t(8, 4096), w)                          # a shape gemv_batch_wins does not name


def test_every_fp16_source_exists_and_a_misspelt_one_stops_the_build(monkeypatch):
    from gpt4roi_amd import build
    assert build.F16_SOURCES and all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.F16_SOURCES)
    monkeypatch.setattr(build, "F16_SOURCES", build.F16_SOURCES + ("gemm_no_such_family.hip",))
    with pytest.raises(RuntimeError, match="gemm_no_such_family.hip"):      # raised before any compile job starts
        build.build()
