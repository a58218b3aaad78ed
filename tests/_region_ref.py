"""fp64 references of the region-feature module's GroupNorm and shuffle kernels (csrc/norm.hip: gn_stats_nhwc, gn_finalize and
their merged-level variants; csrc/spi_backward.hip: gn_stats_partial / finalize, gn_relu_bwd reduce / apply, fuse_shuffle_bwd and
its gather; csrc/elementwise.hip: upsample_coord, fuse_shuffle, fuse_shuffle_mlvl), the inputs the two test files share
(tests/test_region_kernels_cpu.py, tests/test_region_kernels_gpu.py) and the shape tables.  A plain helper module: no fixtures.

The measure is the one of tests/_rows_ref.py (error / worst, R = 2^-22, FLOOR, per element, non-finite = inf), with fp16's ulp
2^-11 added there.  Every reference is written from the definition in fp64 on exactly the values the kernel receives and
returns (ref, cond) per output; it works on the device of its inputs (the cases above the grid cap are referenced on the GPU).

cond, per operation (the sum of the absolute values of the terms the fp64 formula adds to form ref):

    groupnorm      mean: E|x|.  var = E[x^2] - mean^2 as the kernels form it: cvar = E[x^2] + mean^2.  rstd = (var + eps)^-1/2:
                   crstd = rstd + rstd^3 cvar / 2 (its own roundings, and cvar carried through the derivative).  a = gamma rstd:
                   ca = |gamma| crstd.  s = beta - mean a: |beta| + |mean a| + |mean| ca + |a| E|x|.  The reference's var is the
                   two-pass one, so the all-constant group has var = 0 exactly and rstd = eps^-1/2.
    gn_relu_bwd    (mean and rstd are the fp32 `stats` the kernel is handed, a and s its `affine`: inputs, exact as they stand)
                   xhat = (z - mean) rstd is a difference: xhc = (|z| + |mean|) rstd stands for |xhat| wherever xhat is a
                   computed factor.  gd = gamma dy [a z + s > 0], m1 = mean_g(gd), m2 = mean_g(gd xhat):
                   dz: rstd (|gd| + mean_g|gd| + |xhat| mean_g(|gd| xhc) + xhc |m2|)     (m1 and m2 are sums: their cond is the
                   mean of the absolute terms; with |m1| and |m2| alone the fp32 restatement read 2.48 on the groups with
                   |mean| / std = 8, whose fp32-rounded mean shifts every xhat of the group the same way);
                   dgamma: |dgamma0| + sum |dyh| xhc;  dbeta: |dbeta0| + sum |dyh|.
    resampling     (fuse_shuffle, its two transposes, upsample_coord)  weight of source index j for target index i is the hat
                   function max(0, 1 - |src_i - j|), src_i = i (in - 1) / (out - 1): a difference of src_i and j, so each pair
                   within the hat's support carries (src_i + j) next to its |weight|:  cond = sum (|wy| |wx| + cwy |wx| +
                   |wy| cwx) |v|, cw = [|src - j| <= 1] (src + j), and cw = 0 where in == out, in == 1 or out == 1 (weights
                   exact).  With sum |w v| alone the fp32 restatements read 10.3 (fuse_shuffle), 15.5 (its transposes) and 4.6
                   (upsample_coord): where a weight is small, its own rounding is all the error there is.  A source with a deferred relu(a x + s) enters with |a x| + |s| (0 where a x + s is clearly negative).
                   The transposes add |what the destination held before|.
    coordinates    linspace(-1, 1, n)[i] = -1 + i step or 1 - (n - 1 - i) step: cond 2.  Pad channels: ref 0, cond 0.

ReLU ties.  The backward mask a z + s > 0 is evaluated in fp32 by the kernel and in fp64 here; BWD cases are generated from seeds
for which no element has |a z + s| < 2^-18 (|a z| + |s|) (relu_ties() == 0, asserted in the CPU test for every backward case),
so no element is masked out of a comparison.  The two cases too large to check element by element ((40, 600) and the case above
the grid cap) repeat a tile of 2 resp. 29 pixels along HW: mean, var and therefore every a z + s of the whole map are those
of the tile, which is checked (and is what the CPU readings run on).

The unit.  fp32 torch restatements (the *_formula functions with dtype=torch.float32, on the CPU) against the fp64 references:

    groupnorm affine + stats   GN_CASES: (C, G) (64, 8), (64, 1), (512, 64), (1024, 64), (2048, 64) x HW 1, 31, 32, 33, 63 x
                               B 1, 3; HW 2081, 8200 at C = 64; bf16 and fp16 input; the levels of MLVL_SIZES       0.643
                               (sums per chunk of ppb pixels in fp32, chunks and moments in fp64, as the kernels do: torch's
                               own fp32 sum over 8200 x 8 values read 8.3)
    gn_relu_bwd                BWD_CASES: C 64, 512, 2048 x (B, HW) (1, 1), (1, 33), (2, 63), (3, 35), (40, 2: the tile),
                               (1, 35); (5, 29: the tile) at C = 2048                    0.996  (dgamma 0.561, dbeta 0.422)
    fuse_shuffle               SHUFFLE_GEOMS and every target of ROUNDS x C 32, 64 x B 1, 2 x with / without affines x
                               bf16, fp16                                                                         0.996
    fuse_shuffle_bwd (+gather) the same geometries (destinations non-zero) and whole rounds                       0.230
    upsample_coord             UPSAMPLE_GEOMS x C 8, 64 x Cpad C + 8, 128 x bf16, fp16                             0.996

so E = 1.0 (a bf16 / fp16 output cannot read less: its final rounding is half an ulp = up to one unit), and the kernels get
BOUND = 4 E: rsqrt, reordered sums and atomics, as in _rows_ref.  test_region_kernels_cpu.py measures the readings again.

Mutants (wrong formulas evaluated in fp64; each exceeds BOUND by more than 10x on these inputs, the CPU test prints the ratios;
> 1e30 means a value where ref and cond are 0):  groupnorm unbiased_variance 3.9e4, eps_outside_sqrt 5.9e3,
shift_uses_neighbour_group (the mean of s taken with the group of the next 8-channel vector) 2.6e7,
drops_last_pixel_of_ragged_chunk 3.8e8;  gn_relu_bwd mask_from_z 4.8e9, m2_dropped 1.4e5, dgamma_overwrites 8.4e5;  fuse_shuffle
align_corners_false, xy_swapped, offsets_swapped (c + S <-> c - S), identity_on_resampled: all > 1e30 forward, the first three
> 1e30 backward too;  upsample_coord align_corners_false 1.2e5, xy_swapped 1.0e4, coords_swapped 5.2e5, pad_nonzero > 1e30.
"""
import torch
import torch.nn.functional as F

from _rows_ref import FLOOR, GRID_CAP, R, U_BF16, U_F16, U_F32, error, worst, worst_of  # noqa: F401  (the shared measure)

E = 1.0                          # measured 1.00 (module docstring)
BOUND = 4.0 * E
TIE = 2.0 ** -18                 # relative distance from 0 below which a ReLU mask may flip between fp32 and fp64
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
EPS = 1e-5

# ---- the shapes both files run ------------------------------------------------------------------------------------------
GN_CG = ((64, 8), (64, 1), (512, 64), (1024, 64), (2048, 64))
GN_HW_SMALL, GN_HW_LARGE, GN_B = (1, 31, 32, 33, 63), (2081, 8200), (1, 3)
GN_CASES = tuple((B, HW, C, G) for C, G in GN_CG for HW in GN_HW_SMALL for B in GN_B) + \
    tuple((B, HW, 64, G) for G in (8, 1) for HW in GN_HW_LARGE for B in GN_B)
GROUPS = {64: 8, 512: 64, 1024: 64, 2048: 64}
MLVL_SIZES = (((5, 7),), ((6, 4), (3, 2)), ((9, 5), (5, 3), (1, 1)), ((24, 24), (12, 12), (6, 6), (3, 3)),
              ((3, 3), (2081, 1), (5, 7), (1, 1)))
MLVL_BC = ((1, 64), (2, 64), (1, 1024), (2, 1024))

BWD_C = (64, 512, 2048)
BWD_BHW = ((1, 1), (1, 33), (2, 63), (3, 35), (40, 600), (1, 35))
BWD_TILE = {(40, 600): 2}                        # HW = 300 tiles of 2 pixels
# B * HW * C / 8 = 16384 * 256 + 256: one vector row above a single grid-stride pass of gn_relu_bwd_apply.  (16384 * 256 + 257
# is no multiple of C / 8 = 256; B * HW = 16385 = 5 * 29 * 113 is the first pixel count above the cap.)
BWD_CAP, BWD_CAP_TILE = (5, 3277, 2048), 29
BWD_CASES = tuple((B, HW, C) for C in BWD_C for B, HW in BWD_BHW) + (BWD_CAP,)
BWD_SEEDS = {(1, 33, 2048): 1, (2, 63, 2048): 3, (40, 600, 2048): 1, BWD_CAP: 47}   # where seed 0 has a ReLU tie

SHUFFLE_C, SHUFFLE_B = (32, 64), (1, 2)
# (own, top, down): every resampled pair non-square; non-integer ratios; 1x1 and Nx1 levels; both pyramid ends
SHUFFLE_GEOMS = (((6, 10), (3, 5), (12, 20)), ((5, 7), (3, 4), (9, 13)), ((1, 1), (1, 1), (2, 3)), ((4, 1), (2, 1), (8, 1)),
                 ((12, 20), (6, 10), (12, 20)), ((3, 5), (3, 5), (6, 10)))
ROUNDS = (((12, 20), (6, 10), (3, 5), (1, 2)), ((9, 13), (5, 7), (3, 4)), ((6, 4), (3, 2)), ((5, 7),))
GATHER_BIG = ((600, 875), (2, 3))                # B = 1, C = 64: 600 * 875 * 8 = 4 200 000 work items on level 0
SCATTER_BIG = ((600, 875), (2, 3), (5, 7))       # (own, top, down), the same count
UPSAMPLE_GEOMS = ((6, 6, 24, 24), (4, 6, 9, 14), (1, 1, 5, 3), (3, 5, 1, 1), (2, 2, 2, 2))
UPSAMPLE_C = (8, 64)


def upsample_cpads(C):
    return (C + 8, 128)


def gn_ppb(HW):
    return max(32, -(-HW // 256))


def bwd_ppb(B, HW):
    return max(32, -(-HW // min(256, max(16, 512 // B))))


def lvl_list(L):
    """(target, top, down) of every level: the coarser and the finer neighbour, or the level itself at the ends."""
    return [(l, min(l + 1, L - 1), max(l - 1, 0)) for l in range(L)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def gn_case(B, HW, C, G, dtype=BF16, seed=0):
    """z [B, HW, C] with per-group offsets (|mean| / std = 8 in every third group, 0 in the next, 0.5 in the third), exact
    zeros in the groups without an offset, one all-constant group (image B - 1, group G - 1, when there is more than one (image, group)); gamma of both
    signs; dy fp32; non-zero dgamma0 / dbeta0."""
    g = _gen(7919 * B + 31 * HW + C + G + 1000003 * seed)
    cpg = C // G
    std = 0.5 + torch.rand(B, 1, G, 1, generator=g)
    kind = (torch.arange(G) + (G == 1)) % 3                              # (a single group is a centred one)
    off = torch.tensor([8.0, 0.0, -0.5])[kind] * torch.tensor([1.0, -1.0])[(torch.arange(G) // 3) % 2]
    z = (torch.randn(B, HW, G, cpg, generator=g) + off.view(1, 1, G, 1)) * std
    z[(torch.rand(B, HW, G, cpg, generator=g) < 0.05) & (kind != 0).view(1, 1, G, 1)] = 0.0   # (a zero would widen an offset group)
    if B * G > 1:
        z[B - 1, :, G - 1, :] = 0.75
    z = z.reshape(B, HW, C)
    z[0, 0, C - cpg if G == 1 or B > 1 else cpg] = 0.0                   # one zero in every case: a centred group, or the constant one
    gamma = torch.randn(C, generator=g) * 0.8 + 0.3
    gamma[0], gamma[1] = -1.1, 0.9
    return dict(z=z.to(dtype), gamma=gamma, beta=torch.randn(C, generator=g) * 0.5, dy=torch.randn(B, HW, C, generator=g),
                dgamma0=torch.randn(C, generator=g), dbeta0=torch.randn(C, generator=g))


def bwd_tile(B, HW, C):
    return BWD_CAP_TILE if (B, HW, C) == BWD_CAP else BWD_TILE.get((B, HW))


def bwd_case(B, HW, C):
    """The gn_case of a backward shape; for the two tiled shapes the TILE ([B, tile, C]) and `reps`: expand() makes the map."""
    tile = bwd_tile(B, HW, C)
    c = gn_case(B, tile or HW, C, GROUPS[C], seed=BWD_SEEDS.get((B, HW, C), 0))
    c["reps"] = HW // tile if tile else 1
    assert (tile or HW) * c["reps"] == HW
    return c


def expand(c, device):
    """The full-size tensors of a (tiled) case on `device`: z repeated along HW, dy repeated with a factor per repeat."""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}
    reps = d.pop("reps", 1)
    if reps > 1:
        B, t, C = d["z"].shape
        d["z"] = d["z"].repeat(1, reps, 1)
        f = torch.cos(torch.arange(reps, device=device, dtype=F32))[None, :, None, None]
        d["dy"] = (d["dy"].view(B, 1, t, C) * f).reshape(B, reps * t, C)
    return d


def shuffle_case(B, C, sizes, dtype=BF16, seed=0):
    """Per level of `sizes`: a map in `dtype`, a deferred affine [B, 2, C] fp32 (a of both signs), a conv-input gradient
    (bf16) and what a gradient destination holds before the scatter (fp32)."""
    g = _gen(101 * B + C + 13 * sum(h * 31 + w for h, w in sizes) + seed)
    maps = [(torch.randn(B, h, w, C, generator=g) * 1.5 + 0.2).to(dtype) for h, w in sizes]
    affs = [torch.stack([torch.randn(B, C, generator=g) * 0.8 + 0.2, torch.randn(B, C, generator=g) * 0.5], 1).contiguous()
            for _ in sizes]
    dinps = [torch.randn(B, h, w, C, generator=g).to(BF16) for h, w in sizes]
    d0 = [torch.randn(B, h, w, C, generator=g) for h, w in sizes]
    return dict(maps=maps, affs=affs, dinps=dinps, d0=d0)


def upsample_case(B, hin, win, C, dtype=BF16, seed=0):
    """tokens [B, hin * win, C]: a view that drops a CLS row and 8 trailing columns of a wider buffer."""
    g = _gen(B + 7 * hin + 11 * win + C + seed)
    hs = (torch.randn(B, hin * win + 1, C + 8, generator=g) * 1.5).to(dtype)
    return dict(hs=hs, tokens=hs[:, 1:, :C])


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------
def _moments(z, G):
    B, HW, C = z.shape
    x = z.double().view(B, HW, G, C // G)
    mean = x.mean((1, 3))
    var = (x - mean[:, None, :, None]).pow(2).mean((1, 3))
    return mean, var, (x * x).mean((1, 3)), x.abs().mean((1, 3))


def gn_ref(z, gamma, beta, G, eps=EPS):
    """affine [B, 2, C] (a, s) and stats [B, G, 2] (mean, rstd)."""
    cpg = z.size(2) // G
    gamma, beta = gamma.double(), beta.double()
    mean, var, ex2, eabs = _moments(z, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    crstd = rstd + 0.5 * rstd.pow(3) * (ex2 + mean * mean)
    ge = lambda t: t.repeat_interleave(cpg, 1)                          # noqa: E731  [B, G] -> [B, C]
    a, ca = gamma * ge(rstd), gamma.abs() * ge(crstd)
    s = beta - ge(mean) * a
    cs = beta.abs() + (ge(mean) * a).abs() + ge(mean).abs() * ca + a.abs() * ge(eabs)
    return dict(affine=(torch.stack([a, s], 1), torch.stack([ca, cs], 1)),
                stats=(torch.stack([mean, rstd], -1), torch.stack([eabs, crstd], -1)))


def gn_formula(z, gamma, beta, G, eps=EPS, dtype=F32, mutant=None):
    B, HW, C = z.shape
    cpg = C // G
    n = HW * cpg
    # as the kernels do: sums per chunk of ppb pixels in `dtype`, the chunks and the moments in fp64, rounded to `dtype`
    ppb = gn_ppb(HW)
    chunks = -(-HW // ppb)
    x = torch.zeros(B, chunks * ppb, G, cpg, dtype=dtype, device=z.device)
    x[:, :HW] = z.to(dtype).view(B, HW, G, cpg)
    if mutant == "drops_last_pixel_of_ragged_chunk" and HW % ppb:
        x[:, HW - 1] = 0.0
    x = x.view(B, chunks, ppb, G, cpg)
    gamma, beta = gamma.to(dtype), beta.to(dtype)
    mean, ex2 = x.sum((2, 4)).double().sum(1) / n, (x * x).sum((2, 4)).double().sum(1) / n
    var = (ex2 - mean * mean).clamp_min(0.0)
    if mutant == "unbiased_variance":
        var = var * n / max(n - 1, 1)
    rstd = 1.0 / (torch.sqrt(var) + eps) if mutant == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    mean, rstd = mean.to(dtype), rstd.to(dtype)
    a = gamma * rstd.repeat_interleave(cpg, 1)
    gidx = torch.arange(C, device=z.device) // cpg
    if mutant == "shift_uses_neighbour_group":                          # channel -> group map off by one 8-channel vector
        gidx = ((torch.arange(C, device=z.device) + 8) // cpg) % G
    s = beta - mean[:, gidx] * a
    return dict(affine=torch.stack([a, s], 1).to(F32), stats=torch.stack([mean, rstd], -1).to(F32))


def relu_ties(z, affine):
    """Elements whose mask a z + s > 0 could differ between fp32 and fp64 (or that sit exactly at 0)."""
    az = affine[:, 0].double()[:, None, :] * z.double()
    s = affine[:, 1].double()[:, None, :]
    t = az + s
    return int(((t.abs() < TIE * (az.abs() + s.abs())) | (t == 0)).sum())


def gn_bwd_ref(z, dy, affine, gamma, stats, dgamma0, dbeta0, G):
    """y = relu(GN(z)), the closed form of csrc/spi_backward.hip in fp64 on exactly what the kernel is given: the mask from
    `affine`, mean and rstd from `stats` (with the fp64 stats of gn_ref this is autograd through relu(F.group_norm))."""
    B, HW, C = z.shape
    cpg = C // G
    x, dy, gamma = z.double(), dy.double(), gamma.double()
    ge = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]              # noqa: E731  [B, G] -> [B, 1, C]
    gm = lambda t: ge(t.view(B, HW, G, cpg).mean((1, 3)))               # noqa: E731  mean over the group, per element
    mu, rs = ge(stats[..., 0].double()), ge(stats[..., 1].double())
    mask = affine[:, 0].double()[:, None, :] * x + affine[:, 1].double()[:, None, :] > 0
    dyh = dy * mask
    xh, xhc = (x - mu) * rs, (x.abs() + mu.abs()) * rs
    gd = gamma * dyh
    m2 = gm(gd * xh)
    dz = rs * (gd - gm(gd) - xh * m2)
    cdz = rs * (gd.abs() + gm(gd.abs()) + xh.abs() * gm(gd.abs() * xhc) + xhc * m2.abs())
    return dict(dz=(dz, cdz),
                dgamma=(dgamma0.double() + (dyh * xh).sum((0, 1)), dgamma0.double().abs() + (dyh.abs() * xhc).sum((0, 1))),
                dbeta=(dbeta0.double() + dyh.sum((0, 1)), dbeta0.double().abs() + dyh.abs().sum((0, 1))))


def gn_bwd_formula(z, dy, affine, gamma, stats, dgamma0, dbeta0, G, dtype=F32, mutant=None):
    B, HW, C = z.shape
    cpg = C // G
    x, dy, gamma, affine, stats = (t.to(dtype) for t in (z, dy, gamma, affine, stats))
    ge = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]              # noqa: E731
    gm = lambda t: ge(t.view(B, HW, G, cpg).sum((1, 3)) / (HW * cpg))   # noqa: E731
    mu, rs = ge(stats[..., 0]), ge(stats[..., 1])
    mask = x > 0 if mutant == "mask_from_z" else affine[:, 0][:, None, :] * x + affine[:, 1][:, None, :] > 0
    dyh = dy * mask
    xh = (x - mu) * rs
    gd = gamma * dyh
    m2 = 0.0 if mutant == "m2_dropped" else gm(gd * xh)
    dz = rs * (gd - gm(gd) - xh * m2)
    dg0 = 0.0 if mutant == "dgamma_overwrites" else dgamma0.to(dtype)
    return dict(dz=dz.to(BF16), dgamma=(dg0 + (dyh * xh).sum((0, 1))).to(F32), dbeta=(dbeta0.to(dtype) + dyh.sum((0, 1))).to(F32))


# ---- align_corners=True bilinear resampling as matrices --------------------------------------------------------------------
def _src(n_in, n_out, dtype, align=True, device="cpu", count=None):
    """Source coordinate of each of `count` (default n_out) target indices on an axis resampled n_in -> n_out, in `dtype`."""
    dst = torch.arange(n_out if count is None else count, dtype=dtype, device=device)
    if not align:
        return ((dst + 0.5) * (torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)).to(device) - 0.5).clamp_min(0.0)
    if n_out <= 1:
        return torch.zeros_like(dst)
    return (torch.tensor(float(n_in - 1), dtype=dtype) / torch.tensor(float(n_out - 1), dtype=dtype)).to(device) * dst


def lerp_matrix(n_in, n_out, dtype=F64, align=True, pair=None, device="cpu"):
    """[n_out, n_in]: row i holds the two weights of target index i, computed in `dtype` the way lerp_ac does.  pair = (in,
    out) takes the scale from ANOTHER axis (the x / y swap mutant)."""
    src = _src(*(pair or (n_in, n_out)), dtype, align, device, count=n_out)
    i0 = src.floor().clamp(max=n_in - 1).long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    w1 = src - i0.to(dtype)
    M = torch.zeros(n_out, n_in, dtype=dtype, device=device)
    ar = torch.arange(n_out, device=device)
    M[ar, i0] += 1.0 - w1
    M[ar, i1] += w1
    return M


def lerp_cond(n_in, n_out, device="cpu"):
    """(|weights|, cw): cw[i, j] = src_i + j where j lies within the hat around src_i, 0 where the weights are exact."""
    M = lerp_matrix(n_in, n_out, device=device).abs()
    cw = torch.zeros_like(M)
    if n_in > 1 and n_out > 1 and n_in != n_out:
        src = _src(n_in, n_out, F64, device=device)[:, None]
        j = torch.arange(n_in, dtype=F64, device=device)[None]
        cw = ((src - j).abs() <= 1.0 + 1e-9) * (src + j)
    return M, cw


def _fwd(My, Mx, x):
    """[B, h, w, c] -> [B, H, W, c]: rows by My [H, h], then columns by Mx [W, w]."""
    B, h, w, c = x.shape
    t = torch.matmul(My, x.reshape(B, h, w * c)).view(B, My.size(0), w, c)
    return torch.matmul(Mx, t)


def _bwd(My, Mx, d):
    """The transpose of _fwd: [B, H, W, c] -> [B, h, w, c]."""
    B, H, W, c = d.shape
    t = torch.matmul(My.t(), d.reshape(B, H, W * c)).view(B, My.size(1), W, c)
    return torch.matmul(Mx.t(), t)


def _conds(op, cv, hs, ws, H, W):
    Ay, Cy = lerp_cond(hs, H, cv.device)
    Ax, Cx = lerp_cond(ws, W, cv.device)
    return op(Ay, Ax, cv) + op(Cy, Ax, cv) + op(Ay, Cx, cv)


def resample_ref(v, H, W):
    """v fp64 [B, h, w, c] -> ([B, H, W, c] by F.interpolate(bilinear, align_corners=True), differentiable)."""
    return F.interpolate(v.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


def _mats(hs, ws, H, W, dtype, mutant, device):
    align = mutant != "align_corners_false"
    if mutant == "xy_swapped":
        return lerp_matrix(hs, H, dtype, pair=(ws, W), device=device), lerp_matrix(ws, W, dtype, pair=(hs, H), device=device)
    return lerp_matrix(hs, H, dtype, align, device=device), lerp_matrix(ws, W, dtype, align, device=device)


def _parts(C, mutant=None):
    """(role, target channels, source channels) of the shuffle: layers.py _single_shuffle."""
    Rr, S = C // 2, C // 4
    top, down = slice(Rr + S, C), slice(Rr, Rr + S)
    if mutant == "offsets_swapped":
        top, down = down, top
    return (("own", slice(0, Rr), slice(0, Rr)), ("top", slice(Rr, Rr + S), top), ("down", slice(Rr + S, C), down))


def _aff(aff, sl, dtype):
    return aff[:, 0].to(dtype)[:, None, None, sl], aff[:, 1].to(dtype)[:, None, None, sl]


# ---- fuse_shuffle ---------------------------------------------------------------------------------------------------------
def shuffle_ref(own, top, down, affs=(None, None, None)):
    B, H, W, C = own.shape
    refs, conds = [], []
    for (_, _, sl), src, aff in zip(_parts(C), (own, top, down), affs):
        v = src.double()[..., sl]
        c = v.abs()
        if aff is not None:
            a, s = _aff(aff, sl, F64)
            t, c = a * v + s, (a * v).abs() + s.abs()
            v, c = t.clamp_min(0.0), c * (t > -TIE * c)
        refs.append(resample_ref(v, H, W))
        conds.append(c if src.shape[1:3] == (H, W) else _conds(_fwd, c, src.size(1), src.size(2), H, W))
    return dict(out=(torch.cat(refs, -1), torch.cat(conds, -1)))


def shuffle_formula(own, top, down, affs=(None, None, None), dtype=F32, mutant=None):
    B, H, W, C = own.shape
    outs = []
    for (_, _, sl), src, aff in zip(_parts(C, mutant), (own, top, down), affs):
        v = src.to(dtype)[..., sl]
        if aff is not None:
            a, s = _aff(aff, sl, dtype)
            v = (a * v + s).clamp_min(0.0)
        hs, ws = src.shape[1:3]
        if (hs, ws) == (H, W):
            outs.append(v)
        elif mutant == "identity_on_resampled":
            outs.append(v[:, torch.arange(H).clamp(max=hs - 1)][:, :, torch.arange(W).clamp(max=ws - 1)])
        else:
            outs.append(_fwd(*_mats(hs, ws, H, W, dtype, mutant, v.device), v))
    return dict(out=torch.cat(outs, -1).to(own.dtype))


def round_ref(maps, affs):
    return [shuffle_ref(maps[t], maps[tp], maps[dn], (affs[t], affs[tp], affs[dn]))["out"] for t, tp, dn in lvl_list(len(maps))]


# ---- its transpose: scatter (one target) and gather (one source of a whole round) ---------------------------------------------
def shuffle_bwd_ref(dinp, top_hw, down_hw, d0=(None, None, None)):
    """d_own, d_top, d_down [B, h, w, C] fp64: what the destination held (d0, fp32 or None = 0) plus fp64 autograd of the
    resampling of shuffle_ref, written as matrices (F.interpolate's own backward adds 10^7 fp64 atomics onto a 2 x 3 map)."""
    B, H, W, C = dinp.shape
    d = dinp.double()
    out = {}
    for (role, slt, sls), (hs, ws), z0 in zip(_parts(C), ((H, W), top_hw, down_hw), d0):
        part = d[..., slt]
        if (hs, ws) == (H, W):
            g, c = part, part.abs()
        else:
            xin = torch.zeros(B, hs, ws, part.size(3), dtype=F64, device=d.device, requires_grad=True)
            My, Mx = lerp_matrix(hs, H, device=d.device), lerp_matrix(ws, W, device=d.device)
            (_fwd(My, Mx, xin) * part).sum().backward()                 # (_fwd is F.interpolate: the CPU test compares the two)
            g, c = xin.grad, _conds(_bwd, part.abs(), hs, ws, H, W)
        ref = z0.double().clone() if z0 is not None else torch.zeros(B, hs, ws, C, dtype=F64, device=d.device)
        cond = ref.abs()
        ref[..., sls] += g
        cond[..., sls] += c
        out["d_" + role] = (ref, cond)
    return out


def shuffle_bwd_formula(dinp, top_hw, down_hw, d0=(None, None, None), dtype=F32, mutant=None):
    B, H, W, C = dinp.shape
    d = dinp.to(dtype)
    out = {}
    for (role, slt, sls), (hs, ws), z0 in zip(_parts(C, mutant), ((H, W), top_hw, down_hw), d0):
        part = d[..., slt]
        g = part if (hs, ws) == (H, W) else _bwd(*_mats(hs, ws, H, W, dtype, mutant, d.device), part)
        ref = z0.to(dtype).clone() if z0 is not None else torch.zeros(B, hs, ws, C, dtype=dtype, device=d.device)
        ref[..., sls] += g
        out["d_" + role] = ref.to(F32)
    return out


def round_bwd(dinps, one=shuffle_bwd_ref, **kw):
    """The gradient of every SOURCE level of a round, summed over the targets that read it (the reference's neighbour table):
    a list of (ref, cond) for one=shuffle_bwd_ref, of fp32 tensors for one=shuffle_bwd_formula."""
    L = len(dinps)
    acc = [None] * L

    def add(l, r):
        acc[l] = r if acc[l] is None else (tuple(x + y for x, y in zip(acc[l], r)) if isinstance(r, tuple) else acc[l] + r)

    for t, tp, dn in lvl_list(L):
        r = one(dinps[t], dinps[tp].shape[1:3], dinps[dn].shape[1:3], **kw)
        add(t, r["d_own"]), add(tp, r["d_top"]), add(dn, r["d_down"])
    return acc


# ---- upsample_coord ---------------------------------------------------------------------------------------------------------
def upsample_ref(tokens, hin, win, H, W, cpad):
    B, n, C = tokens.shape
    x = tokens.double().reshape(B, hin, win, C)
    ref = torch.zeros(B, H, W, cpad, dtype=F64, device=x.device)
    cond = torch.zeros_like(ref)
    ref[..., :C], cond[..., :C] = resample_ref(x, H, W), _conds(_fwd, x.abs(), hin, win, H, W)
    ref[..., C] = torch.linspace(-1, 1, W, dtype=F64, device=x.device)[None, None, :]
    ref[..., C + 1] = torch.linspace(-1, 1, H, dtype=F64, device=x.device)[None, :, None]
    cond[..., C:C + 2] = 2.0
    return dict(out=(ref, cond))


def upsample_formula(tokens, hin, win, H, W, cpad, dtype=F32, mutant=None):
    B, n, C = tokens.shape
    x = tokens.to(dtype).reshape(B, hin, win, C)
    out = torch.full((B, H, W, cpad), 2.0 ** -7 if mutant == "pad_nonzero" else 0.0, dtype=dtype)
    out[..., :C] = _fwd(*_mats(hin, win, H, W, dtype, mutant, x.device), x)
    cx, cy = (C + 1, C) if mutant == "coords_swapped" else (C, C + 1)
    out[..., cx] = torch.linspace(-1, 1, W, dtype=dtype)[None, None, :]
    out[..., cy] = torch.linspace(-1, 1, H, dtype=dtype)[None, :, None]
    return dict(out=out.to(tokens.dtype))
