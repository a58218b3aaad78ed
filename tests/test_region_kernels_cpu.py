"""CPU: would the comparison of tests/_region_ref.py notice a wrong GroupNorm / shuffle kernel of the region module?  The unit E
of its measure is measured again on fp32 torch restatements of every operation; the backward cases are free of ReLU mask ties; the
shape tables reach every path of the launch code (restated here in arithmetic); and one wrong restatement per plausible kernel
mistake exceeds the bound the GPU tests use by more than 10x on the very inputs tests/test_region_kernels_gpu.py runs.  The
mutants are evaluated in fp64, so all they differ by from the reference is their mistake."""
import pytest
import torch

import _region_ref as R

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


# ------------------------------------------------------------------------------------------ every case, once
def gn_eval(dtype, mutant=None, keys=None):
    w = 0.0
    for B, HW, C, G in R.GN_CASES:
        for zdt in (BF16, F16):
            c = R.gn_case(B, HW, C, G, zdt)
            want = R.gn_ref(c["z"], c["gamma"], c["beta"], G)
            w = max(w, R.worst_of(R.gn_formula(c["z"], c["gamma"], c["beta"], G, dtype=dtype, mutant=mutant), want, keys))
    return w


def gn_mlvl_eval(dtype, mutant=None):
    """The level maps of the merged-level cases (each level is one groupnorm of its own)."""
    w = 0.0
    for sizes in R.MLVL_SIZES:
        for B, C in R.MLVL_BC:
            for l, (h, wd) in enumerate(sizes):
                c = R.gn_case(B, h * wd, C, R.GROUPS[C], seed=l + 1)
                want = R.gn_ref(c["z"], c["gamma"], c["beta"], R.GROUPS[C])
                w = max(w, R.worst_of(R.gn_formula(c["z"], c["gamma"], c["beta"], R.GROUPS[C], dtype=dtype, mutant=mutant), want))
    return w


def _bwd_inputs(B, HW, C):
    c = R.bwd_case(B, HW, C)
    G = R.GROUPS[C]
    ref = R.gn_ref(c["z"], c["gamma"], c["beta"], G)
    return c, G, ref["affine"][0].float(), ref["stats"][0].float()


def bwd_eval(dtype, mutant=None, keys=None):
    w = 0.0
    for B, HW, C in R.BWD_CASES:
        c, G, affine, stats = _bwd_inputs(B, HW, C)                     # (the tile of a tiled case)
        want = R.gn_bwd_ref(c["z"], c["dy"], affine, c["gamma"], stats, c["dgamma0"], c["dbeta0"], G)
        got = R.gn_bwd_formula(c["z"], c["dy"], affine, c["gamma"], stats, c["dgamma0"], c["dbeta0"], G, dtype=dtype, mutant=mutant)
        w = max(w, R.worst_of(got, want, keys))
    return w


def _shuffle_cases():
    for C in R.SHUFFLE_C:
        for B in R.SHUFFLE_B:
            for geom in R.SHUFFLE_GEOMS:
                yield B, C, geom, (0, 1, 2)
            for sizes in R.ROUNDS:
                for t, tp, dn in R.lvl_list(len(sizes)):
                    yield B, C, sizes, (t, tp, dn)


def shuffle_eval(dtype, mutant=None):
    w = 0.0
    for B, C, sizes, idx in _shuffle_cases():
        for zdt in (BF16, F16):
            c = R.shuffle_case(B, C, sizes, zdt)
            m = [c["maps"][i] for i in idx]
            for affs in ((None, None, None), tuple(c["affs"][i] for i in idx)):
                w = max(w, R.worst_of(R.shuffle_formula(*m, affs, dtype=dtype, mutant=mutant), R.shuffle_ref(*m, affs)))
    return w


def shuffle_bwd_eval(dtype, mutant=None):
    w = 0.0
    for B, C, sizes, idx in _shuffle_cases():
        c = R.shuffle_case(B, C, sizes)
        args = (c["dinps"][idx[0]], sizes[idx[1]], sizes[idx[2]], tuple(c["d0"][i] for i in idx))
        w = max(w, R.worst_of(R.shuffle_bwd_formula(*args, dtype=dtype, mutant=mutant), R.shuffle_bwd_ref(*args)))
    for C in R.SHUFFLE_C:                                               # whole rounds, as the gather computes them
        for B in R.SHUFFLE_B:
            for sizes in R.ROUNDS:
                c = R.shuffle_case(B, C, sizes)
                want = R.round_bwd(c["dinps"])
                got = R.round_bwd(c["dinps"], R.shuffle_bwd_formula, dtype=dtype, mutant=mutant)
                w = max([w] + [R.worst(g, *wt) for g, wt in zip(got, want)])
    return w


def upsample_eval(dtype, mutant=None):
    w = 0.0
    for hin, win, H, W in R.UPSAMPLE_GEOMS:
        for C in R.UPSAMPLE_C:
            for cpad in R.upsample_cpads(C):
                for zdt in (BF16, F16):
                    tok = R.upsample_case(2, hin, win, C, zdt)["tokens"]
                    got = R.upsample_formula(tok, hin, win, H, W, cpad, dtype=dtype, mutant=mutant)
                    w = max(w, R.worst_of(got, R.upsample_ref(tok, hin, win, H, W, cpad)))
    return w


EVALS = dict(groupnorm=gn_eval, groupnorm_mlvl_levels=gn_mlvl_eval, gn_relu_bwd=bwd_eval, fuse_shuffle=shuffle_eval,
             fuse_shuffle_bwd=shuffle_bwd_eval, upsample_coord=upsample_eval)


# ------------------------------------------------------------------------------------------ the unit
def test_fp32_restatements_measure_the_unit():
    es = {name: f(F32) for name, f in EVALS.items()}
    es["gn_relu_bwd dgamma"], es["gn_relu_bwd dbeta"] = bwd_eval(F32, keys=["dgamma"]), bwd_eval(F32, keys=["dbeta"])
    for name, e in es.items():
        print(f"fp32 torch {name}: {e:.3f} units")
    e = max(es.values())
    print(f"E measured {e:.3f} (E = {R.E}, R = 2^-22, BOUND = {R.BOUND})")
    assert 0.25 < e <= R.E                  # (far below: the unit would be slack; above: _region_ref.E is stale)


def test_fp64_restatements_agree_with_the_references():
    """The hand-written formulas (the ones the mutants vary) and the references are two statements of the same operation: in
    fp64 they differ by the output's final rounding and the fp32 rounding of the stats they are given."""
    for name, f in EVALS.items():
        e = f(F64)
        print(f"fp64 formula {name}: {e:.3f} units")
        assert e <= 1.0, name


def test_references_are_the_torch_definitions():
    """gn_ref / gn_bwd_ref against F.group_norm and autograd through relu(F.group_norm) in fp64; the resampling matrices (that
    carry cond) against F.interpolate."""
    B, HW, C = 3, 35, 64
    c, G, affine, _ = _bwd_inputs(B, HW, C)
    z = c["z"].double().requires_grad_(True)
    gam, bet = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    y = torch.relu(torch.nn.functional.group_norm(z.permute(0, 2, 1), G, gam, bet, R.EPS)).permute(0, 2, 1)
    (y * c["dy"].double()).sum().backward()
    ref = R.gn_ref(c["z"], c["gamma"], c["beta"], G)
    a, s = ref["affine"][0][:, 0], ref["affine"][0][:, 1]
    assert float((torch.relu(a[:, None] * z.detach() + s[:, None]) - y.detach()).abs().max()) < 1e-11
    want = R.gn_bwd_ref(c["z"], c["dy"], affine, c["gamma"], ref["stats"][0], c["dgamma0"], c["dbeta0"], G)   # the fp64 stats
    assert float((want["dz"][0] - z.grad).abs().max()) < 1e-11
    assert float((want["dgamma"][0] - c["dgamma0"].double() - gam.grad).abs().max()) < 1e-10
    assert float((want["dbeta"][0] - c["dbeta0"].double() - bet.grad).abs().max()) < 1e-10
    g = torch.Generator().manual_seed(3)
    for hs, ws, H, W in ((3, 5, 6, 10), (3, 4, 5, 7), (9, 13, 5, 7), (1, 1, 2, 3), (2, 1, 4, 1), (3, 5, 1, 1), (1, 4, 3, 9)):
        x = torch.randn(2, hs, ws, 8, generator=g, dtype=F64)
        xm, xi = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        got, want = R._fwd(R.lerp_matrix(hs, H), R.lerp_matrix(ws, W), xm), R.resample_ref(xi, H, W)
        assert float((got - want).detach().abs().max()) < 1e-13
        d = torch.randn(got.shape, generator=g, dtype=F64)
        (got * d).sum().backward(), (want * d).sum().backward()
        assert float((xm.grad - xi.grad).abs().max()) < 1e-13
        assert float((xm.grad - R._bwd(R.lerp_matrix(hs, H), R.lerp_matrix(ws, W), d)).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------ ReLU ties
def test_backward_cases_have_no_relu_mask_ties():
    for B, HW, C in R.BWD_CASES:
        c, G, affine, _ = _bwd_inputs(B, HW, C)
        assert R.relu_ties(c["z"], affine) == 0, (B, HW, C)
        assert bool((c["z"] == 0).any()) and bool((c["gamma"] < 0).any()) and bool((c["gamma"] > 0).any())
        assert bool((c["dgamma0"] != 0).all()) and bool((c["dbeta0"] != 0).all())
        if B * G > 1:                                                   # the all-constant group: var = 0
            ref = R.gn_ref(c["z"], c["gamma"], c["beta"], G)["stats"][0]
            assert float(ref[B - 1, G - 1, 1]) == pytest.approx(R.EPS ** -0.5, rel=1e-12)
        tile = R.bwd_tile(B, HW, C)
        if tile:                                                        # the map is whole tiles: its moments are the tile's
            assert HW % tile == 0 and c["z"].size(1) == tile and c["reps"] * tile == HW
            full = R.expand(c, "cpu") if B * HW * C < 2 ** 22 else None
            if full is not None:
                fa = R.gn_ref(full["z"], c["gamma"], c["beta"], G)["affine"][0]
                assert float((fa - R.gn_ref(c["z"], c["gamma"], c["beta"], G)["affine"][0]).abs().max()) < 1e-9
                assert R.relu_ties(full["z"], fa.float()) == 0


def test_inputs_hold_what_the_issue_asks_for():
    c = R.gn_case(3, 63, 512, 64)
    mean, var, _, _ = R._moments(c["z"], 64)
    ratio = mean.abs() / var.sqrt().clamp_min(1e-30)
    assert bool((ratio[0] > 6).any()) and bool((ratio[0] < 0.3).any())       # offset groups and centred groups
    assert float(var[2, 63]) == 0.0 and bool((c["z"] == 0).any())


# ------------------------------------------------------------------------------------------ the tables reach every path
def test_layout_reaches_every_path():
    # groupnorm_affine / groupnorm_stats: ppb = max(32, ceil(HW / 256)), chunks = ceil(HW / ppb); plc = 256 / (C / 8)
    assert {256 // (C // 8) for _, _, C, _ in R.GN_CASES} == {32, 4, 2, 1}
    assert all(256 % (C // 8) == 0 and (C // G) % 8 == 0 for _, _, C, G in R.GN_CASES)
    hws = {HW for _, HW, _, _ in R.GN_CASES}
    chunks = {HW: -(-HW // R.gn_ppb(HW)) for HW in hws}
    assert chunks[1] == chunks[31] == chunks[32] == 1 and chunks[33] == 2 and 33 % 32 == 1 and chunks[63] == 2
    assert R.gn_ppb(2081) == 32 and chunks[2081] == 66 > 64 and 2081 % 32 == 1
    assert R.gn_ppb(8200) == 33 > 32 and chunks[8200] == 249 <= 256
    assert any(HW < 32 and 256 // (C // 8) == 32 for _, HW, C, _ in R.GN_CASES)          # most pixel lanes idle
    assert {B for B, _, _, _ in R.GN_CASES} == {1, 3} and {G for _, _, C, G in R.GN_CASES if C == 64} == {8, 1}
    # merged levels: 1..4 levels (the unused slots of the level table), a 2081-pixel level that is not first, 1x1 levels
    assert {len(s) for s in R.MLVL_SIZES} == {1, 2, 3, 4}
    assert any(h * w == 2081 and l > 0 for s in R.MLVL_SIZES for l, (h, w) in enumerate(s))
    assert any((1, 1) in s for s in R.MLVL_SIZES) and {c for _, c in R.MLVL_BC} == {64, 1024} and {b for b, _ in R.MLVL_BC} == {1, 2}
    # gn_relu_bwd: chunks = clamp(512 / B, 16, 256), ppb = max(32, ceil(HW / chunks)); a thread walks the pixels p0 + pl,
    # p0 + pl + plc, ... of its chunk: 4 at a time, then one at a time
    assert {256 // (C // 8) for _, _, C in R.BWD_CASES} == {32, 4, 1}
    rem = {C: set() for C in R.BWD_C}
    for B, HW, C in R.BWD_CASES:
        ppb, plc = R.bwd_ppb(B, HW), 256 // (C // 8)
        for p0 in range(0, HW, ppb):
            n = min(ppb, HW - p0)
            rem[C] |= {len(range(pl, n, plc)) % 4 for pl in range(plc)}
    assert rem[2048] == {0, 1, 2, 3} and rem[512] >= {0, 1, 2, 3}, rem
    assert 512 // 40 < 16 and R.bwd_ppb(40, 600) == 38 and R.bwd_ppb(1, 33) == 32 and -(-33 // 32) == 2
    B, HW, C = R.BWD_CAP
    assert R.GRID_CAP < B * HW * (C // 8) <= R.GRID_CAP + 256 and HW % R.BWD_CAP_TILE == 0
    assert R.bwd_ppb(B, HW) == 33 and -(-HW // 33) == 100                                # chunks > 64, ppb > 32 there too
    # shuffle: non-square resampling both up and down, non-integer ratios, a size-1 axis, both ends, 1..4 levels, the caps
    pairs = [(g[0], g[1]) for g in R.SHUFFLE_GEOMS] + [(g[0], g[2]) for g in R.SHUFFLE_GEOMS]
    ns = [(o, s) for o, s in pairs if o != s]
    assert any(o[0] > s[0] and o[1] > s[1] and o[0] != o[1] and s[0] != s[1] for o, s in ns)      # upsampled from a coarser map
    assert any(o[0] < s[0] and o[1] < s[1] and o[0] != o[1] and s[0] != s[1] for o, s in ns)      # downsampled from a finer one
    assert any((o[0] - 1) % max(s[0] - 1, 1) and (s[0] - 1) % max(o[0] - 1, 1) for o, s in ns)    # non-integer ratio
    assert any(o == (1, 1) for o, _ in pairs) and any(o[1] == 1 and o[0] > 1 and s[1] == 1 for o, s in ns)
    assert any(o == s for o, s in pairs[:len(R.SHUFFLE_GEOMS)]) and any(o == s for o, s in pairs[len(R.SHUFFLE_GEOMS):])
    assert {len(s) for s in R.ROUNDS} == {1, 2, 3, 4} and all(h != w for s in R.ROUNDS for h, w in s)
    assert any(1 in hw for s in R.ROUNDS for hw in s)
    (h, w), C = R.GATHER_BIG[0], 64
    assert R.GRID_CAP < h * w * (C // 8) < 2 * R.GRID_CAP and R.SCATTER_BIG[0] == (h, w)
    assert all(c % 32 == 0 for c in R.SHUFFLE_C)
    # upsample_coord: up, down to 1x1, from 1x1, identity, non-square; the coordinate vector next to C and further pad vectors
    assert any(hin != win and H != W for hin, win, H, W in R.UPSAMPLE_GEOMS)
    assert any((hin, win) == (1, 1) for hin, win, _, _ in R.UPSAMPLE_GEOMS) and any((H, W) == (1, 1) for _, _, H, W in R.UPSAMPLE_GEOMS)
    assert all(cp % 8 == 0 and cp >= C + 2 for C in R.UPSAMPLE_C for cp in R.upsample_cpads(C))
    assert any(cp > C + 8 for C in R.UPSAMPLE_C for cp in R.upsample_cpads(C))
    tok = R.upsample_case(2, 3, 5, 8)["tokens"]
    assert tok.stride(1) == 16 and tok.stride(0) == 16 * 16 and tok.storage_offset() == 16 and tok.stride(2) == 1


# ------------------------------------------------------------------------------------------ the mutants
MUTANTS = [
    ("groupnorm", gn_eval, "unbiased_variance"),
    ("groupnorm", gn_eval, "eps_outside_sqrt"),
    ("groupnorm", gn_eval, "shift_uses_neighbour_group"),
    ("groupnorm", gn_eval, "drops_last_pixel_of_ragged_chunk"),
    ("gn_relu_bwd", bwd_eval, "mask_from_z"),
    ("gn_relu_bwd", bwd_eval, "m2_dropped"),
    ("gn_relu_bwd", bwd_eval, "dgamma_overwrites"),
    ("fuse_shuffle", shuffle_eval, "align_corners_false"),
    ("fuse_shuffle", shuffle_eval, "xy_swapped"),
    ("fuse_shuffle", shuffle_eval, "offsets_swapped"),
    ("fuse_shuffle", shuffle_eval, "identity_on_resampled"),
    ("fuse_shuffle_bwd", shuffle_bwd_eval, "align_corners_false"),
    ("fuse_shuffle_bwd", shuffle_bwd_eval, "xy_swapped"),
    ("fuse_shuffle_bwd", shuffle_bwd_eval, "offsets_swapped"),
    ("upsample_coord", upsample_eval, "align_corners_false"),
    ("upsample_coord", upsample_eval, "xy_swapped"),
    ("upsample_coord", upsample_eval, "coords_swapped"),
    ("upsample_coord", upsample_eval, "pad_nonzero"),
]


@pytest.mark.parametrize("op,evaluate,mutant", MUTANTS, ids=[f"{m[0]}-{m[2]}" for m in MUTANTS])
def test_mutant_exceeds_the_bound_tenfold(op, evaluate, mutant):
    ratio = evaluate(F64, mutant) / R.BOUND
    print(f"mutant {op} {mutant}: {ratio:.3g} x BOUND")
    assert ratio > 10.0


def test_one_wrong_group_is_what_the_measure_protects():
    """max|got - want| / max|want| over the tensor, the measure of the older region-module tests, passes one wrong group out of
    64 and the dropped last pixel of a ragged chunk; this one does not."""
    B, HW, C, G = 3, 8200, 64, 8
    c = R.gn_case(B, HW, C, G)
    want = tuple(t[:1] for t in R.gn_ref(c["z"], c["gamma"], c["beta"], G)["affine"])     # (image 0: no all-constant group)
    got = R.gn_formula(c["z"], c["gamma"], c["beta"], G, dtype=F64, mutant="drops_last_pixel_of_ragged_chunk")["affine"][:1]
    assert float((got.double() - want[0]).abs().max() / want[0].abs().max()) < 1e-2
    assert R.worst(got, *want) > 10.0 * R.BOUND
    c = R.gn_case(2, 63, 512, 64)
    want = R.gn_ref(c["z"], c["gamma"], c["beta"], 64)["affine"]
    got = R.gn_formula(c["z"], c["gamma"], c["beta"], 64, dtype=F64)["affine"]
    got[1, 0, 8:16] *= 1.0 + 1e-3                                       # `a` of one group of the second image
    assert float((got.double() - want[0]).abs().max() / want[0].abs().max()) < 1e-2
    assert R.worst(got, *want) > 10.0 * R.BOUND
