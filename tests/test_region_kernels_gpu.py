"""GPU: the GroupNorm and shuffle kernels of the region-feature module -- groupnorm_affine / groupnorm_stats and the merged-level
affine (csrc/norm.hip, csrc/spi_backward.hip), gn_relu_bwd, upsample_coord, fuse_shuffle and fuse_shuffle_mlvl
(csrc/elementwise.hip), fuse_shuffle_bwd and fuse_shuffle_bwd_gather -- by value against the fp64 references of
tests/_region_ref.py, per element, in the units and under the bound measured there (tests/test_region_kernels_cpu.py shows on the
same inputs that eighteen wrong formulas exceed that bound by > 10x, that no backward case has a ReLU mask tie, and that the
tables reach every path of the launch code).

Every output a wrapper lets the caller supply (fuse_shuffle(out=), gn_relu_bwd(out=, dgamma, dbeta), the d_* maps of
fuse_shuffle_bwd, the MlvlMaps of fuse_shuffle_mlvl) is a view into a larger buffer whose guard elements must come back
untouched; the accumulated ones start from non-zero contents."""
import pytest
import torch

import _region_ref as R
from test_backward_rows_gpu import DEV, carve, guards_intact, sliced

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd._lib import HipKernelError

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])


def report(tag, errs):
    w = max(errs) if errs else 0.0
    print(f"{tag}: worst {w / R.BOUND:.3f} x BOUND ({w:.3f} units, bound {R.BOUND})")
    assert w <= R.BOUND, (tag, errs)


def dev(ts):
    return [None if t is None else t.to(DEV) for t in ts]


def guarded_maps(B, sizes, C, dtype=BF16):
    """A MlvlMaps whose stacked buffer is a guarded view."""
    m = K.MlvlMaps(B, sizes, C, DEV, dtype=dtype)
    buf, flat = carve(tuple(m.flat.shape), dtype)
    assert flat.is_contiguous() and flat.data_ptr() % 16 == 0
    m.flat, m.levels, off = flat, [], 0
    for h, w in m.sizes:
        m.levels.append(flat[off:off + B * h * w].view(B, h, w, C))
        off += B * h * w
    return buf, m


# ---------------------------------------------------------------------------------------------- GroupNorm affine and stats
@DTYPES
@pytest.mark.parametrize("C,G", R.GN_CG)
def test_groupnorm_affine_and_stats(C, G, dtype):
    errs = []
    for B, HW, Cc, Gg in R.GN_CASES:
        if (Cc, Gg) != (C, G):
            continue
        c = R.gn_case(B, HW, C, G, dtype)
        want = R.gn_ref(c["z"], c["gamma"], c["beta"], G)
        z, gamma, beta = dev([c["z"].view(B, HW, 1, C), c["gamma"], c["beta"]])
        aff = K.groupnorm_affine(z, gamma, beta, G, R.EPS)
        e = [R.worst(aff, *want["affine"])]
        if dtype == BF16:
            e.append(R.worst(K.groupnorm_stats(z, G, R.EPS), *want["stats"]))
        print(f"  groupnorm C {C} G {G} B {B} HW {HW}: " + " ".join(f"{x:.3f}" for x in e))
        errs += e
    report(f"groupnorm C {C} G {G} {dtype}", errs)


@pytest.mark.parametrize("B,C", R.MLVL_BC)
def test_groupnorm_affine_merged_levels(B, C):
    G, errs = R.GROUPS[C], []
    for sizes in R.MLVL_SIZES:
        cases = [R.gn_case(B, h * w, C, G, seed=l + 1) for l, (h, w) in enumerate(sizes)]
        gamma, beta = dev([cases[0]["gamma"], cases[0]["beta"]])
        z = K.MlvlMaps(B, sizes, C, DEV)
        for lv, c in zip(z.levels, cases):
            lv.copy_(c["z"].view(lv.shape))
        got = K.groupnorm_affine_mlvl(z, gamma, beta, G, R.EPS)
        assert len(got) == len(sizes)
        for l, c in enumerate(cases):
            errs.append(R.worst(got[l], *R.gn_ref(c["z"], cases[0]["gamma"], cases[0]["beta"], G)["affine"]))
            assert torch.equal(got[l], K.groupnorm_affine(z.levels[l], gamma, beta, G, R.EPS)), (sizes, l)
    report(f"groupnorm_affine_mlvl B {B} C {C}", errs)


# ---------------------------------------------------------------------------------------------- GroupNorm + ReLU backward
def _gn_relu_bwd(B, HW, C, from_kernels=False):
    G = R.GROUPS[C]
    c = R.bwd_case(B, HW, C)
    big = c["reps"] > 1
    d = R.expand(c, DEV if big else "cpu")                              # (the two tiled cases are referenced on the GPU)
    tile_ref = R.gn_ref(c["z"], c["gamma"], c["beta"], G)                # a tiled map has the moments of its tile
    affine, stats = tile_ref["affine"][0].float().to(DEV), tile_ref["stats"][0].float().to(DEV)
    z, dy = d["z"].to(DEV).view(B, HW, 1, C), d["dy"].to(DEV).view(B, HW, 1, C).contiguous()
    gamma = c["gamma"].to(DEV)
    if from_kernels:
        affine, stats = K.groupnorm_affine(z, gamma, c["beta"].to(DEV), G, R.EPS), K.groupnorm_stats(z, G, R.EPS)
        assert R.relu_ties(d["z"], affine.cpu()) == 0
    zb, dz = carve((B * HW, C), BF16)
    gb, dg = carve(C, F32, fill=c["dgamma0"])
    bb, db = carve(C, F32, fill=c["dbeta0"])
    out = dz.view(B, HW, 1, C)
    assert K.gn_relu_bwd(z, dy, affine, gamma, stats, dg, db, G, out=out) is out
    on = d["z"].device
    want = R.gn_bwd_ref(d["z"], d["dy"], affine.to(on), d["gamma"], stats.to(on), d["dgamma0"], d["dbeta0"], G)
    e = [R.worst(dz.view(B, HW, C), *want["dz"]), R.worst(dg, *want["dgamma"]), R.worst(db, *want["dbeta"])]
    assert guards_intact(zb, dz) and guards_intact(gb, dg) and guards_intact(bb, db)
    print(f"  gn_relu_bwd B {B} HW {HW} C {C}{' (kernel stats)' if from_kernels else ''}: dz {e[0]:.3f} dgamma {e[1]:.3f} dbeta {e[2]:.3f}")
    return e


@pytest.mark.parametrize("C", R.BWD_C)
def test_gn_relu_bwd(C):
    errs = []
    for B, HW in R.BWD_BHW:
        errs += _gn_relu_bwd(B, HW, C)
    errs += _gn_relu_bwd(3, 35, C, from_kernels=True)
    report(f"gn_relu_bwd C {C}", errs)


def test_gn_relu_bwd_above_the_grid_cap():
    report("gn_relu_bwd B %d HW %d C %d (above the grid cap)" % R.BWD_CAP, _gn_relu_bwd(*R.BWD_CAP))


# ---------------------------------------------------------------------------------------------- shuffle forward
@DTYPES
@pytest.mark.parametrize("B", R.SHUFFLE_B)
@pytest.mark.parametrize("C", R.SHUFFLE_C)
def test_fuse_shuffle(C, B, dtype):
    errs = []
    for geom in R.SHUFFLE_GEOMS:
        c = R.shuffle_case(B, C, geom, dtype)
        maps, affs = dev(c["maps"]), dev(c["affs"])
        for use in (False, True):
            a, ad = (c["affs"], affs) if use else ([None] * 3, [None] * 3)
            ob, out = carve((B * geom[0][0] * geom[0][1], C), dtype)
            o4 = out.view(maps[0].shape)
            assert K.fuse_shuffle(*maps, *ad, out=o4) is o4
            errs.append(R.worst(o4, *R.shuffle_ref(*c["maps"], a)["out"]))
            assert guards_intact(ob, out)
            assert torch.equal(K.fuse_shuffle(*maps, *ad), o4)
    report(f"fuse_shuffle C {C} B {B} {dtype}", errs)


@DTYPES
@pytest.mark.parametrize("B", R.SHUFFLE_B)
@pytest.mark.parametrize("C", R.SHUFFLE_C)
def test_fuse_shuffle_merged_levels(C, B, dtype):
    """Whole rounds of 4, 3, 2 and 1 levels with the reference's neighbour table, into a guarded MlvlMaps."""
    errs = []
    for sizes in R.ROUNDS:
        c = R.shuffle_case(B, C, sizes, dtype)
        maps, affs = dev(c["maps"]), dev(c["affs"])
        for use in (False, True):
            a, ad = (c["affs"], affs) if use else ([None] * len(sizes), [None] * len(sizes))
            ob, out = guarded_maps(B, sizes, C, dtype)
            K.fuse_shuffle_mlvl(maps, ad, R.lvl_list(len(sizes)), out)
            assert guards_intact(ob, out.flat)
            for (t, tp, dn), want in zip(R.lvl_list(len(sizes)), R.round_ref(c["maps"], a)):
                errs.append(R.worst(out.levels[t], *want))
                assert torch.equal(out.levels[t], K.fuse_shuffle(maps[t], maps[tp], maps[dn], ad[t], ad[tp], ad[dn])), (sizes, t)
    report(f"fuse_shuffle_mlvl C {C} B {B} {dtype}", errs)


# ---------------------------------------------------------------------------------------------- its transposes
def _scatter(dinp, dests0):
    """fuse_shuffle_bwd into three guarded destinations that start from dests0 (None: zeros) -> [(buffer, view4)]."""
    outs = []
    for d0 in dests0:
        B, h, w, C = d0.shape
        buf, v = carve((B * h * w, C), F32, fill=d0.reshape(-1, C))
        outs.append((buf, v, v.view(B, h, w, C)))
    K.fuse_shuffle_bwd(dinp, *(o[2] for o in outs))
    for buf, v, _ in outs:
        assert guards_intact(buf, v)
    return [o[2] for o in outs]


@pytest.mark.parametrize("B", R.SHUFFLE_B)
@pytest.mark.parametrize("C", R.SHUFFLE_C)
def test_fuse_shuffle_bwd_scatter(C, B):
    errs = []
    for geom in R.SHUFFLE_GEOMS:
        c = R.shuffle_case(B, C, geom)
        got = _scatter(c["dinps"][0].to(DEV), dev(c["d0"]))
        want = R.shuffle_bwd_ref(c["dinps"][0], geom[1], geom[2], c["d0"])
        errs += [R.worst(g, *want[k]) for g, k in zip(got, ("d_own", "d_top", "d_down"))]
    report(f"fuse_shuffle_bwd C {C} B {B}", errs)


@pytest.mark.parametrize("B", R.SHUFFLE_B)
@pytest.mark.parametrize("C", R.SHUFFLE_C)
def test_fuse_shuffle_bwd_gather(C, B):
    """Whole rounds: the gather of every source level is finite, the fp64 reference, the same bits twice, and what the scatter
    of every target level accumulates (under BOUND: the scatter adds in another order)."""
    errs, cross = [], []
    for sizes in R.ROUNDS:
        c = R.shuffle_case(B, C, sizes)
        dinps = dev(c["dinps"])
        want = R.round_bwd(c["dinps"])
        acc = [torch.zeros(B, h, w, C, dtype=F32, device=DEV) for h, w in sizes]
        for t, tp, dn in R.lvl_list(len(sizes)):
            K.fuse_shuffle_bwd(dinps[t], acc[t], acc[tp], acc[dn])
        for l in range(len(sizes)):
            got = K.fuse_shuffle_bwd_gather(l, dinps)
            assert got.dtype == F32 and got.shape == dinps[l].shape and bool(torch.isfinite(got).all())
            assert torch.equal(got, K.fuse_shuffle_bwd_gather(l, dinps))
            errs.append(R.worst(got, *want[l]))
            cross.append(R.worst(acc[l], got.double().cpu(), want[l][1]))
    report(f"fuse_shuffle_bwd_gather C {C} B {B}", errs)
    report(f"fuse_shuffle_bwd scatter against gather C {C} B {B}", cross)


def _big_dinp(h, w, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(1, h, w, C, generator=g, device=DEV).to(BF16)


def test_fuse_shuffle_bwd_gather_above_the_grid_cap():
    """Level 0 of a two-level round holds 4 200 000 work items; referenced on the GPU."""
    C = 64
    dinps = [_big_dinp(h, w, C, 11 + i) for i, (h, w) in enumerate(R.GATHER_BIG)]
    want = R.round_bwd(dinps)
    errs = []
    for l in range(2):
        got = K.fuse_shuffle_bwd_gather(l, dinps)
        assert bool(torch.isfinite(got).all())
        errs.append(R.worst(got, *want[l]))
    report("fuse_shuffle_bwd_gather (above the grid cap)", errs)


def test_fuse_shuffle_bwd_scatter_above_the_grid_cap():
    C = 64
    own, top, down = R.SCATTER_BIG
    dinp = _big_dinp(*own, C, 17)
    g = torch.Generator(device=DEV).manual_seed(18)
    d0 = [torch.randn(1, h, w, C, generator=g, device=DEV) for h, w in R.SCATTER_BIG]
    got = _scatter(dinp, d0)
    want = R.shuffle_bwd_ref(dinp, top, down, d0)
    report("fuse_shuffle_bwd (above the grid cap)", [R.worst(g_, *want[k]) for g_, k in zip(got, ("d_own", "d_top", "d_down"))])


# ---------------------------------------------------------------------------------------------- upsample + coordinates
@DTYPES
@pytest.mark.parametrize("C", R.UPSAMPLE_C)
def test_upsample_coord(C, dtype):
    errs, B = [], 2
    for hin, win, H, W in R.UPSAMPLE_GEOMS:
        c = R.upsample_case(B, hin, win, C, dtype)
        tok = c["hs"].to(DEV)[:, 1:, :C]                                # CLS row dropped, wider row stride
        assert tok.stride(1) == C + 8 and not tok.is_contiguous()
        for cpad in R.upsample_cpads(C):
            got = K.upsample_coord(tok, hin, win, H, W, cpad)
            assert got.shape == (B, H, W, cpad) and got.dtype == dtype
            errs.append(R.worst(got, *R.upsample_ref(c["tokens"], hin, win, H, W, cpad)["out"]))
            assert float(got[..., C + 2:].abs().max()) == 0.0           # pad channels: exactly 0
    report(f"upsample_coord C {C} {dtype}", errs)


# ---------------------------------------------------------------------------------------------- refusals
def test_entry_points_refuse_shapes_they_cannot_run():
    """C / 8 that does not divide 256, 4 channels per group, a shuffle C that is no multiple of 32, 5 levels: each is rejected
    by the entry point's shape check, before any launch, and the outputs the caller supplied are untouched."""
    def z(*shape, dtype=BF16):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    for C, G in ((72, 9), (64, 16)):
        x, g = z(1, 4, 1, C), z(C, dtype=F32)
        with pytest.raises(HipKernelError, match="groupnorm"):
            K.groupnorm_affine(x, g, g, G)
        with pytest.raises(HipKernelError, match="groupnorm_stats"):
            K.groupnorm_stats(x, G)
        zb, dz = carve((4, C), BF16)
        gb, dg = carve(C, F32, fill=1.5)
        bb, db = carve(C, F32, fill=2.5)
        with pytest.raises(HipKernelError, match="gn_relu_bwd"):
            K.gn_relu_bwd(x, z(1, 4, 1, C, dtype=F32), z(1, 2, C, dtype=F32), g, z(1, G, 2, dtype=F32), dg, db, G, out=dz.view(1, 4, 1, C))
        for buf, v in ((zb, dz), (gb, dg), (bb, db)):
            assert guards_intact(buf, v)
        assert bool((dg == 1.5).all()) and bool((db == 2.5).all()) and bool((dz == float(zb[0])).all())
        maps = K.MlvlMaps(1, [(2, 2)], C, DEV)
        with pytest.raises(HipKernelError, match="groupnorm_mlvl"):
            K.groupnorm_affine_mlvl(maps, g, g, G)
    m48 = z(1, 2, 3, 48)
    ob, out = carve((6, 48), BF16)
    with pytest.raises(HipKernelError, match="fuse_shuffle"):
        K.fuse_shuffle(m48, m48, m48, out=out.view(1, 2, 3, 48))
    assert guards_intact(ob, out) and bool((out == float(ob[0])).all())
    dests = [carve((6, 48), F32, fill=3.5) for _ in range(3)]
    with pytest.raises(HipKernelError, match="fuse_shuffle_bwd"):
        K.fuse_shuffle_bwd(m48, *(v.view(1, 2, 3, 48) for _, v in dests))
    assert all(guards_intact(b, v) and bool((v == 3.5).all()) for b, v in dests)
    with pytest.raises(HipKernelError, match="fuse_shuffle_bwd_gather"):
        K.fuse_shuffle_bwd_gather(0, [m48])
    sizes5 = [(2, 2)] * 5
    maps5 = [z(1, 2, 2, 64) for _ in sizes5]
    ob, out5 = guarded_maps(1, sizes5, 64)
    with pytest.raises(HipKernelError, match="fuse_shuffle_mlvl"):
        K.fuse_shuffle_mlvl(maps5, [None] * 5, R.lvl_list(5), out5)
    assert guards_intact(ob, out5.flat) and bool((out5.flat == float(ob[0])).all())
    with pytest.raises(HipKernelError, match="groupnorm_mlvl"):
        K.groupnorm_affine_mlvl(out5, z(64, dtype=F32), z(64, dtype=F32), 8)


def test_helpers_are_the_shared_ones():
    x = sliced(torch.zeros(3, 16, dtype=BF16))
    assert x.stride(0) == 32 and x.data_ptr() % 16 == 0
    buf, m = guarded_maps(2, [(3, 2), (1, 1)], 32)
    assert guards_intact(buf, m.flat) and m.levels[1].shape == (2, 1, 1, 32) and m.levels[1].data_ptr() == m.flat[12:].data_ptr()
    buf[0] = 0.0
    assert not guards_intact(buf, m.flat)
