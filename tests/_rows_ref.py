"""fp64 references of the backward row kernels (csrc/backward.hip: rmsnorm_bwd, layernorm_bwd, swiglu_il and its backward,
rope_qkv_bwd, cross_entropy, colsum), the inputs the two test files share and the measure they compare with
(tests/test_backward_rows_cpu.py, tests/test_backward_rows_gpu.py).  A plain helper module: no fixtures, no pytest settings.

The references.  Each one restates the operation from its definition in fp64 -- autograd through F.layer_norm, through the
RMSNorm formula, through F.silu(gate) * up, through oracle.transformer_oracle.apply_rope, and F.cross_entropy(reduction="sum",
ignore_index=-100) -- on exactly the bf16 / fp32 values the kernel receives.  They return (ref, cond) per output.

The measure.  Per element, no max over max:

    err = |got - ref| / (u_out * |ref| + R * cond + FLOOR)

u_out is one ulp of the output's storage (2^-8 bf16, 2^-24 fp32).  cond is the sum of the absolute values of the terms the
fp64 formula adds to form ref (its condition scale): an fp32 evaluation cannot do better than a few roundings of THOSE, however
small their sum.  dx of RMSNorm: rstd * (|gamma dy| + |xhat| |mean(gamma dy xhat)|) + |dres|; LayerNorm adds rstd * |mean(gamma
dy)| and, its xhat = (x - mean) rstd being a difference itself, takes (|x| + |mean|) rstd for |xhat|; dgamma, dbeta, colsum and the loss: |what the output held before| + sum over rows of |term|; dgate of SwiGLU:
|dy up| * (sigma + |g| sigma (1 - sigma)); rope: |a cos| + |b sin|; dlogits: (softmax + onehot) * |grad_scale|; the loss of one
row: |max| + |log sum exp(x - max)| + |x[label]|.  R = 2^-22, four fp32 roundings.  FLOOR = 2^-118 (3e-36) is absolute: an fp32
chain that forms sigma(g) through e^|g| saturates beyond |g| = 88.7, so silu(-90) * up = 7e-38 * up comes out as 0 in torch's
fp32 as in the kernels; nothing else in these tests is within 25 orders of magnitude of it.  A non-finite `got` counts as
infinite, and no element is left out: where ref and cond are both 0 (pad columns, ignored rows) anything but 0 reads > 1e30.

The unit.  An fp32 torch restatement of every operation (the `*_formula` functions below with dtype=torch.float32, run on the
CPU) was judged with this measure against the fp64 references on the inputs of this module:

    rmsnorm_bwd    NORM_SHAPES (rows 1, 8, 9, 37 x cols 8, 1024, 2048, 2056; rows 9, 37 x cols 4096, 8192),
                   with and without dres                                          0.996  (dgamma alone 0.78)
    layernorm_bwd  the same shapes, relu_in False and True                        0.996  (dgamma 0.95, dbeta 0.20)
    swiglu_il      SWIGLU_SHAPES (1, 4), (45, 352), (3, 11008), forward and backward    0.995
    rope_qkv_bwd   ROPE_CASES: D 64 and 128, pos0 0 and 5, 3 sequences of 7 rows, restarting and running positions    0.995
    cross_entropy  CE_SHAPES x rows 1 and 19 x CE_VARIANTS                        0.992  (loss alone 0.32)
    colsum         M 1, 255, 256, 257, 700 x N 1, 255, 257                        0.200

so E = 1.0 (test_backward_rows_cpu.py measures it again and asserts that it stays at or under E).  A bf16 output cannot read
less than this: its final rounding is half an ulp, which is up to 2^-8 of a value just above a power of two.  The fp32 outputs
reach the same unit with R = 2^-22 (LayerNorm's dgamma: 0.95), so R is not slack either.  The kernels are allowed
BOUND = 4 * E = 4 units: they use rsqrtf, __expf and __logf where torch rounds correctly, sum rows in another order, and
accumulate with atomics.

Every mutant of test_backward_rows_cpu.py exceeds BOUND by more than 10x on the same inputs; the ratios are printed there.
"""
import torch
import torch.nn.functional as F

from oracle.transformer_oracle import apply_rope, rope_tables

U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24
U_F16 = 2.0 ** -11                # (tests/_region_ref.py: the forward region kernels also run in fp16)
R = 2.0 ** -22
FLOOR = 2.0 ** -118
E = 1.0                          # measured 0.996 (module docstring); rounded up
BOUND = 4.0 * E                  # units of `error` a kernel may reach

GRID_CAP = 16384 * 256           # work items one pass of a grid-stride kernel covers (grid_for in csrc/backward.hip)
SLOT = 256 * 8                   # columns one register slot of the norm kernels holds; NORM_MAXV = 4 of them
BF16_MAX = 3.3895313892515355e38

# ---- the shapes both files run ----------------------------------------------------------------------------------------
NORM_COLS_SMALL, NORM_COLS_LARGE = (8, 1024, 2048, 2056), (4096, 8192)
NORM_SHAPES = tuple((r, c) for c in NORM_COLS_SMALL for r in (1, 8, 9, 37)) + tuple((r, c) for c in NORM_COLS_LARGE for r in (9, 37))
SWIGLU_SHAPES = ((1, 4), (45, 352), (3, 11008))
SWIGLU_BIG = (1025, 16388)       # T * F / 4 = 4 199 425 work items
ROPE_CASES = tuple((D, pos0) for D in (64, 128) for pos0 in (0, 5))
ROPE_B, ROPE_T, ROPE_HEADS = 3, 7, 3
CE_SHAPES = ((7, 8), (255, 256), (257, 320), (1003, 1024))
CE_ROWS = (1, 19)
CE_VARIANTS = ("plain", "all_ignored", "dominant", "shift+", "shift-")
CE_SHIFT = 1.0e4
COLSUM_M, COLSUM_N = (1, 255, 256, 257, 700), (1, 255, 257)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def norm_case(rows, cols, seed=0):
    """CPU tensors in the kernels' dtypes.  x has exact zeros, negative values and (rows > 1) one all-zero row."""
    g = _gen(1000 * rows + cols + seed)
    x = (torch.randn(rows, cols, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    x[torch.rand(rows, cols, generator=g) < 0.05] = 0.0
    x[0, 0], x[0, 1] = 0.0, -1.25
    if rows > 1:
        x[rows // 2] = 0.0
    return dict(x=x, gamma=1.0 + 0.3 * torch.randn(cols, generator=g),
                dy=torch.randn(rows, cols, generator=g).to(torch.bfloat16),
                dres=torch.randn(rows, cols, generator=g).to(torch.bfloat16),
                dgamma0=torch.randn(cols, generator=g), dbeta0=torch.randn(cols, generator=g))


SPECIAL_GATES = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0, BF16_MAX, -BF16_MAX)


def swiglu_case(T, Fd, seed=0):
    """gu [T, 2F] interleaved, dy [T, F].  The first gates hold +-0, +-20, +-90 and the largest finite bf16 of either sign
    (as many as fit, starting at another one per shape), with |up|, |dy| <= 1 there so every reference value stays finite."""
    g = _gen(7 * T + Fd + seed)
    gate, up = torch.randn(T, Fd, generator=g) * 2.0, torch.randn(T, Fd, generator=g)
    dy = torch.randn(T, Fd, generator=g)
    n = min(8, T * Fd)
    for i in range(n):
        gate.view(-1)[i] = SPECIAL_GATES[(i + Fd) % 8]
        up.view(-1)[i] = (1.0, -0.5)[i % 2]
        dy.view(-1)[i] = (-1.0, 1.0, 0.5)[i % 3]
    gu = torch.stack([gate, up], -1).reshape(T, 2 * Fd).to(torch.bfloat16)
    return dict(gu=gu, dy=dy.to(torch.bfloat16))


def rope_case(D, pos0, seed=0):
    """dq, dk, dv [B * T, heads * D] and tables long enough for running positions (pos0 + B * T)."""
    g = _gen(D + pos0 + seed)
    rows, HD = ROPE_B * ROPE_T, ROPE_HEADS * D
    cos, sin = rope_tables(pos0 + rows, D)
    d = [torch.randn(rows, HD, generator=g).to(torch.bfloat16) for _ in range(3)]
    return dict(dq=d[0], dk=d[1], dv=d[2], cos=cos.contiguous(), sin=sin.contiguous())


def ce_case(rows, N, variant="plain", seed=0):
    """logits fp32 [rows, N] on the grid of 2^-10 (so that +-1e4 shifts them exactly), labels int64, grad_scale, the loss
    the accumulator holds before the call."""
    g = _gen(31 * rows + N + seed)
    logits = (torch.randn(rows, N, generator=g) * 3.0 * 1024.0).round() / 1024.0
    labels = torch.randint(0, N, (rows,), generator=g)
    if rows >= 19:
        labels[3], labels[11] = -100, -1
        labels[5], labels[7] = N, 2 ** 40 + 3            # at and far above N: ignored, like a negative label
    if variant == "all_ignored":
        labels[:] = -100
    if variant == "dominant":
        logits[0, labels[0]] = 40.0                      # row 0 always carries a valid label
    if variant == "shift+":
        logits = logits + CE_SHIFT
    if variant == "shift-":
        logits = logits - CE_SHIFT
    n_valid = int(((labels >= 0) & (labels < N)).sum())
    return dict(logits=logits, labels=labels, gs=torch.tensor([1.0 / (n_valid + 2)]), loss0=torch.tensor([2.5]))


def colsum_case(M, N, seed=0):
    g = _gen(M * 1000 + N + seed)
    return dict(x=torch.randn(M, N, generator=g).to(torch.bfloat16), out0=torch.randn(N, generator=g))


# ---- the measure -----------------------------------------------------------------------------------------------------
def error(got, ref, cond, r=R):
    """Elementwise |got - ref| / (u_out |ref| + r cond + FLOOR), u_out from the dtype of `got`; non-finite -> inf."""
    u = {torch.bfloat16: U_BF16, torch.float32: U_F32, torch.float16: U_F16}[got.dtype]
    ref = ref.to(got.device)
    e = (got.detach().double() - ref).abs() / (u * ref.abs() + r * cond.to(got.device) + FLOOR)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def worst(got, ref, cond, r=R):
    assert got.shape == ref.shape == cond.shape, (got.shape, ref.shape, cond.shape)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(cond).all())
    return float(error(got, ref, cond, r).max()) if got.numel() else 0.0


def _d(t):
    return None if t is None else t.detach().double()


# ---- fp64 references: (ref, cond) per output ------------------------------------------------------------------------------
def rmsnorm_ref(x, gamma, dy, dres=None, dgamma0=None, eps=1e-6):
    x, gamma, dy, dres, dgamma0 = _d(x), _d(gamma), _d(dy), _d(dres), _d(dgamma0)
    xl, gl = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    y = xl * torch.rsqrt(xl.pow(2).mean(-1, keepdim=True) + eps) * gl
    (y * dy).sum().backward()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh, gd = x * rstd, gamma * dy
    dx = xl.grad + (dres if dres is not None else 0.0)
    cdx = rstd * (gd.abs() + xh.abs() * (gd * xh).mean(-1, keepdim=True).abs()) + (dres.abs() if dres is not None else 0.0)
    out = dict(dx=(dx, cdx))
    if dgamma0 is not None:
        out["dgamma"] = (dgamma0 + gl.grad, dgamma0.abs() + (dy * xh).abs().sum(0))
    return out


def layernorm_ref(x, gamma, dy, dgamma0=None, dbeta0=None, eps=1e-5, relu_in=False):
    x, gamma, dy, dgamma0, dbeta0 = _d(x), _d(gamma), _d(dy), _d(dgamma0), _d(dbeta0)
    cols = x.size(1)
    xl, gl, bl = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), torch.zeros_like(gamma).requires_grad_(True)
    y = F.layer_norm(F.relu(xl) if relu_in else xl, (cols,), gl, bl, eps)
    (y * dy).sum().backward()
    xr = x.clamp_min(0.0) if relu_in else x
    mean = xr.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xr - mean).pow(2).mean(-1, keepdim=True) + eps)
    xh, gd = (xr - mean) * rstd, gamma * dy
    xhc = (xr.abs() + mean.abs()) * rstd                 # xhat is itself a difference: its own condition scale
    cdx = rstd * (gd.abs() + gd.mean(-1, keepdim=True).abs() + xhc * (gd * xh).mean(-1, keepdim=True).abs())
    if relu_in:
        cdx = cdx * (x > 0)
    out = dict(dx=(xl.grad, cdx))
    if dgamma0 is not None:
        out["dgamma"] = (dgamma0 + gl.grad, dgamma0.abs() + (dy.abs() * xhc).sum(0))
    if dbeta0 is not None:
        out["dbeta"] = (dbeta0 + bl.grad, dbeta0.abs() + dy.abs().sum(0))
    return out


def swiglu_ref(gu, dy=None):
    """Works on the device of its inputs (the case above the grid cap is 33.6 M elements)."""
    T, F2 = gu.shape
    g, u = _d(gu[:, 0::2]).requires_grad_(True), _d(gu[:, 1::2]).requires_grad_(True)
    y = F.silu(g) * u
    out = dict(y=(y.detach(), y.detach().abs()))
    if dy is not None:
        dy = _d(dy)
        (y * dy).sum().backward()
        with torch.no_grad():
            sg = torch.sigmoid(g)
            cg = (dy * u).abs() * (sg + g.abs() * sg * (1.0 - sg))
            cu = (dy * g * sg).abs()
            out["dgu"] = (torch.stack([g.grad, u.grad], -1).reshape(T, F2), torch.stack([cg, cu], -1).reshape(T, F2))
    return out


def rope_ref(dq, dk, dv, cos, sin, heads, pos0, batch=1):
    """d(qkv) [rows, 3 * HD]: `batch` stacked sequences whose positions restart at pos0 (batch = 1: positions run on)."""
    rows, HD = dq.shape
    T, D = rows // batch, HD // heads
    c, s = _d(cos).cpu(), _d(sin).cpu()
    cf = torch.cat([c, c], -1)[pos0:pos0 + T].abs()[None, :, None, :]
    sf = torch.cat([s, s], -1)[pos0:pos0 + T].abs()[None, :, None, :]
    refs, conds = [], []
    for d in (dq, dk):
        d = _d(d).cpu().reshape(batch, T, HD)
        xin = torch.zeros(batch, T, HD, dtype=torch.float64, requires_grad=True)
        (apply_rope(xin, c, s, heads, pos0) * d).sum().backward()
        d4 = d.view(batch, T, heads, D)
        sw = torch.cat([d4[..., D // 2:], d4[..., :D // 2]], -1)
        refs.append(xin.grad.reshape(rows, HD))
        conds.append((d4.abs() * cf + sw.abs() * sf).reshape(rows, HD))
    refs.append(_d(dv).cpu())
    conds.append(_d(dv).cpu().abs())
    return dict(dqkv=(torch.cat(refs, 1), torch.cat(conds, 1)))


def ce_ref(logits, labels, gs, loss0, n_pad=None):
    """loss = loss0 + sum over the rows with a label in [0, N) (the kernel ignores every other label); dlogits [rows, n_pad]
    = d(sum loss) / d logits * gs, zero in the pad columns."""
    x, labels = _d(logits).cpu(), labels.cpu().clone()
    rows, N = x.shape
    n_pad = n_pad or N
    labels[(labels < 0) | (labels >= N)] = -100
    xl = x.clone().requires_grad_(True)
    loss = F.cross_entropy(xl, labels, ignore_index=-100, reduction="sum")
    loss.backward()
    gs, loss0 = float(_d(gs)), _d(loss0).cpu().reshape(1)
    valid = labels >= 0
    onehot = torch.zeros_like(x)
    onehot[valid, labels[valid]] = 1.0
    m = x.max(-1).values
    lse = torch.logsumexp(x, -1)
    xlab = (x * onehot).sum(-1)
    dl, cdl = torch.zeros(rows, n_pad, dtype=torch.float64), torch.zeros(rows, n_pad, dtype=torch.float64)
    dl[:, :N] = xl.grad * gs
    cdl[:, :N] = (torch.softmax(x, -1) + onehot) * abs(gs) * valid[:, None]
    closs = loss0.abs() + ((m.abs() + (lse - m).abs() + xlab.abs()) * valid).sum()
    return dict(loss=(loss0 + loss.detach(), closs), dlogits=(dl, cdl))


def colsum_ref(x, out0):
    x, out0 = _d(x), _d(out0)
    return dict(out=(out0 + x.sum(0), out0.abs() + x.abs().sum(0)))


# ---- torch restatements: dtype=float32 measures the unit, a mutant (in fp64) shows what the measure can see ----------------
def _t(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


def rmsnorm_formula(x, gamma, dy, dres, dgamma0, eps=1e-6, dtype=torch.float32, mutant=None):
    x, gamma, dy, dres, dgamma0 = (_t(t, dtype) for t in (x, gamma, dy, dres, dgamma0))
    rows, cols = x.shape
    rstd = torch.rsqrt((x * x).sum(-1, keepdim=True) / cols + eps)
    xh, gd = x * rstd, gamma * dy
    width = -(-cols // SLOT) * SLOT if mutant == "mean_over_padded_width" else cols
    dx = rstd * (gd - xh * ((gd * xh).sum(-1, keepdim=True) / width))
    if mutant == "no_mean_term":
        dx = rstd * gd
    if dres is not None:
        dx = dx + dres
    t = dy * (x if mutant == "dgamma_from_x" else xh)
    if mutant == "dgamma_drops_last_row_of_8":
        t = t.clone()
        t[7::8] = 0.0
    return dict(dx=dx.to(torch.bfloat16), dgamma=(dgamma0 + t.sum(0)).to(torch.float32))


def layernorm_formula(x, gamma, dy, dgamma0, dbeta0, eps=1e-5, relu_in=False, dtype=torch.float32, mutant=None):
    x, gamma, dy, dgamma0, dbeta0 = (_t(t, dtype) for t in (x, gamma, dy, dgamma0, dbeta0))
    xr = x.clamp_min(0.0) if relu_in and mutant != "relu_mask_on_output_only" else x
    mean = xr.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((xr - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh, gd = (xr - mean) * rstd, gamma * dy
    mg = gd.mean(-1, keepdim=True) if mutant != "no_mean_gdy_term" else 0.0
    dx = rstd * (gd - mg - xh * (gd * xh).mean(-1, keepdim=True))
    if relu_in:
        dx = dx * (~(x < 0) if mutant == "relu_mask_on_output_only" else (x > 0))
    return dict(dx=dx.to(torch.bfloat16), dgamma=(dgamma0 + (dy * xh).sum(0)).to(torch.float32),
                dbeta=(dbeta0 + dy.sum(0)).to(torch.float32))


def swiglu_formula(gu, dy, dtype=torch.float32, mutant=None):
    gu, dy = _t(gu, dtype), _t(dy, dtype)
    g, u = (gu[:, 1::2], gu[:, 0::2]) if mutant == "gate_up_swapped" else (gu[:, 0::2], gu[:, 1::2])
    sg = torch.sigmoid(g)
    dg = (dy * u * sg) * (1.0 + g * (1.0 - sg)) if mutant != "sigma_only" else dy * u * sg
    du = dy * (g * sg)
    pair = [du, dg] if mutant == "gate_up_swapped" else [dg, du]
    return dict(y=((g * sg) * u).to(torch.bfloat16), dgu=torch.stack(pair, -1).reshape(gu.shape).to(torch.bfloat16))


def rope_formula(dq, dk, dv, cos, sin, heads, pos0, batch=1, dtype=torch.float32, mutant=None):
    rows, HD = dq.shape
    T, D = rows // batch, HD // heads
    pos = pos0 + (torch.arange(rows) if mutant == "positions_do_not_restart" else torch.arange(rows) % T)
    c, s = _t(cos, dtype)[pos][:, None, :], _t(sin, dtype)[pos][:, None, :]
    if mutant == "forward_rotation":
        s = -s
    outs = []
    for d in (dq, dk):
        d = _t(d, dtype).view(rows, heads, D)
        a, b = d[..., :D // 2], d[..., D // 2:]
        outs.append(torch.cat([a * c + b * s, b * c - a * s], -1).reshape(rows, HD))
    outs.append(_t(dv, dtype))
    return dict(dqkv=torch.cat(outs, 1).to(torch.bfloat16))


CE_PREFILL = 7.0


def ce_formula(logits, labels, gs, loss0, n_pad=None, dtype=torch.float32, mutant=None):
    x, gs, loss0 = _t(logits, dtype), _t(gs, dtype), _t(loss0, dtype)
    rows, N = x.shape
    n_pad = n_pad or N
    valid = (labels >= 0) & (labels < N)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    ssum = e.sum(-1, keepdim=True)
    row_loss = (m + torch.log(ssum)).squeeze(-1) - x.gather(1, lab[:, None]).squeeze(-1)
    counted = valid if mutant != "ignored_row_contributes_loss" else torch.ones_like(valid)
    loss = loss0 + (row_loss * counted).sum().reshape(1)
    dl = torch.full((rows, n_pad), CE_PREFILL if mutant == "pad_columns_not_zeroed" else 0.0, dtype=dtype)
    onehot = torch.zeros(rows, n_pad + 1, dtype=dtype)
    onehot.scatter_(1, (lab + (1 if mutant == "onehot_at_label_plus_1" else 0))[:, None], 1.0)
    dl[:, :N] = (e / ssum - onehot[:, :N]) * (gs if mutant != "no_grad_scale" else 1.0)
    dl[~valid] = 0.0
    return dict(loss=loss.to(torch.float32), dlogits=dl.to(torch.bfloat16))


def colsum_formula(x, out0, dtype=torch.float32):
    return dict(out=(_t(out0, dtype) + _t(x, dtype).sum(0)).to(torch.float32))


def worst_of(got, want, keys=None):
    """max of `worst` over the outputs of a reference dict (name -> (ref, cond)) that `got` (name -> tensor) holds."""
    return max(worst(got[k], *want[k]) for k in (keys or want.keys()))
