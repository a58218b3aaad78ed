"""GPU: the two launches every training path ends in -- g4r_multi_sumsq and g4r_multi_adamw_f32 behind
kernels.MultiTensorAdamW -- the single-tensor g4r_adamw_f32 and the embedding gradient's g4r_scatter_add_rows_f32, by value
against fp64 restatements (tests/_optim_ref.py).  The error is taken on the UPDATE, in the units and under the bound derived
there; tests/test_optimizer_cpu.py shows on the same inputs that nine wrong update formulas exceed that bound by > 10x.

Every tensor the kernels write is cut out of a larger buffer with 64 guard elements on each side, which must come back
untouched.  The table mixes the chunk's edge sizes (1, 7, 4095, 4096, 4097, 8195, 3 * 4096, 20 000), bf16 and fp32 gradients,
tensors with and without a bf16 copy, an fp32 gradient that starts 4 bytes past a 16-byte boundary (scalar path of the sum
of squares) and fp32 gradients whose last chunk is 1 or 3 elements long."""
import math

import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K

DEV = "cuda"
PAD = 64
GUARD = {torch.float32: 12345.0, torch.bfloat16: 12288.0}      # (exact in bf16)
GRAD_OFFSET = (1, 0, 0, 0, 0, 0, 0, 0, 0)                      # tensor 0: fp32, 4097 elements, starts at element 1 of its buffer
COPIES = (True, False, True, False, True, False, True, False, True)


def carve(values, dtype=None, offset=0):
    """(buffer, view): `values` copied into a view that starts PAD + offset elements into a guard-filled buffer."""
    dtype = values.dtype if dtype is None else dtype
    n = values.numel()
    buf = torch.full((PAD + offset + n + PAD,), GUARD[dtype], dtype=dtype, device=DEV)
    view = buf[PAD + offset:PAD + offset + n]
    view.copy_(values.to(dtype))
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    g = GUARD[buf.dtype]
    return bool((buf[:lo] == g).all()) and bool((buf[lo + view.numel():] == g).all())


@pytest.fixture(scope="module")
def case():
    return R.make_case()


class Table:
    """A MultiTensorAdamW over guarded copies of p0: masters, both moments and the bf16 copies all lie between guards."""

    def __init__(self, p0, betas, wd=R.WD):
        z = [torch.zeros_like(p) for p in p0]
        self.p, self.m, self.v = ([carve(x) for x in xs] for xs in (p0, z, z))
        self.c = [carve(p, torch.bfloat16) if has else None for p, has in zip(p0, COPIES)]
        self.opt = K.MultiTensorAdamW([v for _, v in self.p], [c[1] if c else None for c in self.c], betas, R.EPS, wd,
                                      moments=([v for _, v in self.m], [v for _, v in self.v]))

    def state(self):
        return tuple([v.clone() for _, v in xs] for xs in (self.p, self.m, self.v))

    def check(self, before, grads, step, betas, max_norm, pre_scale, total_sq=None, wd=R.WD, tag=""):
        """p, m and v after a step against ref_step from the state before it; bf16 copies; guards."""
        want = R.ref_step(*before, grads, step, R.LR, betas, R.EPS, wd, max_norm, pre_scale, total_sq=total_sq)
        r = R.R0 + R.bias_term(betas, step)
        errs = [R.worst(b, a, w, r) for b, a, w in zip(before, self.state(), want[:3])]
        print(f"{tag} betas {betas} step {step} clip coefficient {want[3]['coef']:.3g}: "
              f"p {errs[0]:.2f} m {errs[1]:.2f} v {errs[2]:.2f} units (bound {R.BOUND})")
        assert max(errs) <= R.BOUND, (tag, step, errs)
        for (_, p), c in zip(self.p, self.c):
            if c is not None:
                assert torch.equal(c[1], p.to(torch.bfloat16))
        for buf, view in self.p + self.m + self.v + [c for c in self.c if c is not None]:
            assert guards_intact(buf, view)
        return want[3]


def device_grads(grads, flip=False):
    """Guarded device copies in the case's dtypes (flip: every dtype exchanged); tensor 0 keeps its 4-byte misalignment
    when it is fp32."""
    out = []
    for g, off in zip(grads, GRAD_OFFSET):
        dt = g.dtype if not flip else (torch.float32 if g.dtype == torch.bfloat16 else torch.bfloat16)
        out.append(carve(g, dt, off))
    return out


def test_gradient_layout_reaches_every_path(case):
    """The table really holds what the module docstring says (the sum of squares takes its float4 path only for a chunk whose
    length is a multiple of 4 at a 16-byte aligned address)."""
    _, grads = case
    dg = device_grads(grads[0])
    f32 = [(v, n) for (_, v), n in zip(dg, R.NUMELS) if v.dtype == torch.float32]
    assert any(v.data_ptr() % 16 == 4 and v.is_contiguous() for v, _ in f32)                   # scalar path: misaligned
    assert {n % R.CHUNK % 4 for v, n in f32 if v.data_ptr() % 16 == 0} >= {0, 1, 3}            # float4 and scalar last chunks
    assert any(v.dtype == torch.bfloat16 for _, v in dg) and 8 <= len(dg) <= 10
    assert set(R.NUMELS) == {1, 7, 4095, 4096, 4097, 8195, 3 * 4096, 20000}
    assert sum(COPIES) in (len(COPIES) // 2, len(COPIES) - len(COPIES) // 2)


def test_sum_of_squares(case):
    p0, grads = case
    t = Table(p0, R.BETAS[0])
    for flip in (False, True, False):                       # the pointer / dtype table is uploaded again when it changes
        dg = device_grads(grads[2], flip)
        views = [v for _, v in dg]
        got = t.opt.grad_norm_sq(views)
        assert got.dtype == torch.float64 and got.shape == (1,)
        first = got.clone()
        want = R.sumsq(views)                               # fp64 over the values as stored (bf16 or fp32)
        rel = abs(float(first) - want) / want
        print(f"sum of squares (dtypes exchanged: {flip}): {float(first):.17g} vs {want:.17g}, relative {rel:.2e}")
        assert rel <= 1e-12                                 # the squares are exact in fp64: only the order of the sum differs
        assert torch.equal(t.opt.grad_norm_sq(views), first)                       # fixed reduction order
        for (buf, v), g in zip(dg, grads[2]):
            assert guards_intact(buf, v) and torch.equal(v.cpu(), g.to(v.dtype))   # read only


@pytest.mark.parametrize("betas", R.BETAS)
def test_four_steps_against_the_fp64_step(case, betas):
    p0, grads = case
    t = Table(p0, betas)
    coefs = []
    for step in range(1, R.STEPS + 1):
        dg = device_grads(grads[step - 1])
        views = [v for _, v in dg]
        before = t.state()
        total = t.opt.step(views, R.LR, R.MAX_NORM, pre_scale=R.PRE_SCALE)
        info = t.check(before, views, step, betas, R.MAX_NORM, R.PRE_SCALE, tag="four steps")
        coefs.append(info["coef"])
        assert abs(float(total) - info["total_sq"]) <= 1e-12 * info["total_sq"]     # the UNCLIPPED, unscaled squared norm
        for (buf, v), g in zip(dg, grads[step - 1]):
            assert guards_intact(buf, v) and torch.equal(v.cpu(), g)
    assert coefs[0] < 1e-2 and coefs[2] < 1e-2 and coefs[1] == 1.0 and coefs[3] == 1.0    # clipping on, off, on, off


def test_pre_scale_no_clipping_and_supplied_norm(case):
    p0, grads = case
    betas = R.BETAS[0]
    # pre_scale = 1/8: a clipped step, then one below the clip threshold (where the scale reaches the moments unclipped)
    t = Table(p0, betas)
    for step, gs in ((1, grads[0]), (2, grads[1])):
        views = [v for _, v in device_grads(gs)]
        before = t.state()
        t.opt.step(views, R.LR, R.MAX_NORM, pre_scale=0.125)
        info = t.check(before, views, step, betas, R.MAX_NORM, 0.125, tag="pre_scale 1/8")
        assert (info["coef"] < 1.0) == (step == 1)
    # max_grad_norm=None: a gradient of norm 240 goes in unclipped
    t = Table(p0, betas)
    views = [v for _, v in device_grads(grads[0])]
    before = t.state()
    t.opt.step(views, R.LR, None)
    assert t.check(before, views, 1, betas, None, 1.0, tag="no clipping")["coef"] == 1.0
    assert math.sqrt(R.sumsq(views)) > 100 * R.MAX_NORM
    # total_sq supplied (the sharded optimizers' all-reduced sum): 9x the table's own -> a third of its own coefficient
    t = Table(p0, betas)
    own = R.sumsq(views)
    supplied = torch.tensor([9.0 * own], dtype=torch.float64, device=DEV)
    before = t.state()
    ret = t.opt.step(views, R.LR, R.MAX_NORM, total_sq=supplied)
    info = t.check(before, views, 1, betas, R.MAX_NORM, 1.0, total_sq=supplied, tag="supplied norm")
    assert ret is supplied and float(supplied) == 9.0 * own
    assert abs(info["coef"] * (3.0 * math.sqrt(own) + 1e-6) - R.MAX_NORM) < 1e-12


def test_checkpoint_round_trip_is_bit_exact(case):
    p0, grads = case
    betas = R.BETAS[0]
    dg = [[v for _, v in device_grads(g)] for g in grads[:3]]
    a = Table(p0, betas)
    for step in (0, 1):
        a.opt.step(dg[step], R.LR, R.MAX_NORM, pre_scale=R.PRE_SCALE)
    sd = a.opt.state_dict()
    b = Table([v.cpu() for _, v in a.p], betas)             # a fresh optimizer over copies of the parameters
    assert b.opt.steps == 0 and float(b.opt.exp_avg[2].abs().max()) == 0.0
    b.opt.load_state_dict(sd)
    assert b.opt.steps == 2
    a.opt.step(dg[2], R.LR, R.MAX_NORM, pre_scale=R.PRE_SCALE)
    b.opt.step(dg[2], R.LR, R.MAX_NORM, pre_scale=R.PRE_SCALE)
    for xa, xb in zip(a.state(), b.state()):
        assert all(torch.equal(u, w) for u, w in zip(xa, xb))
    for ca, cb in zip(a.c, b.c):
        assert ca is None or torch.equal(ca[1], cb[1])
    assert not torch.equal(a.p[2][1].cpu(), p0[2])


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_single_tensor_adamw_against_the_fp64_step(gdtype):
    """g4r_adamw_f32 (one tensor, grad_scale folded in, no clipping): three steps from zero moments, both gradient types."""
    n, betas, lr, wd = 4999, (0.9, 0.95), 2e-3, 0.1
    g = torch.Generator().manual_seed(3)
    p0 = (0.05 + 0.95 * torch.rand(n, generator=g)) * (2.0 * torch.randint(0, 2, (n,), generator=g) - 1.0)
    z = torch.zeros(n)
    (pb_, p), (mb_, m), (vb_, v), (cb_, c) = carve(p0), carve(z), carve(z), carve(p0, torch.bfloat16)
    for step in range(1, 4):
        gb_, gr = carve(torch.randn(n, generator=g) * (1.0, 1e-3, 1.0)[step - 1], gdtype)
        before = ([p.clone()], [m.clone()], [v.clone()])
        K.adamw(p, gr, m, v, step, lr, betas, R.EPS, wd, grad_scale=0.5, param_bf16=c)
        want = R.ref_step(*before, [gr], step, lr, betas, R.EPS, wd, None, 0.5)
        r = R.R0 + R.bias_term(betas, step)
        errs = [R.worst(b, [a], w, r) for b, a, w in zip(before, (p, m, v), want[:3])]
        print(f"single-tensor adamw {gdtype} step {step}: p {errs[0]:.2f} m {errs[1]:.2f} v {errs[2]:.2f} units (bound {R.BOUND})")
        assert max(errs) <= R.BOUND, errs
        assert torch.equal(c, p.to(torch.bfloat16))
        assert all(guards_intact(b, x) for b, x in ((pb_, p), (mb_, m), (vb_, v), (cb_, c), (gb_, gr)))


@pytest.mark.parametrize("C", [64, 520])
def test_scatter_add_rows_against_fp64_index_add(C):
    """out[idx[r]] += src[r] with fp32 atomics.  n = 1000 source rows into V = 50 table rows: row 7 is named 500 times, six
    rows 2..10 times, twenty rows ~18 times, 100 sources are skipped (-1), 23 rows are never named.  Source and table are
    row-strided views of wider tensors; the table is non-zero before the call.

    Tolerance.  An element of a row named `count` times is the result of `count` fp32 additions in an order the atomics
    choose.  Each addition rounds its result, a partial sum of magnitude at most S = |initial| + sum |terms|, by at most
    2^-24 * S; so any order ends within count * 2^-24 * S of the exact sum (the terms themselves, bf16 values, are exact
    in fp32)."""
    n, V = 1000, 50
    g = torch.Generator().manual_seed(C)
    perm = torch.randperm(n, generator=g)
    idx = torch.empty(n, dtype=torch.int64)
    idx[perm[:500]] = 7
    pos = 500
    for k, reps in enumerate((2, 3, 5, 10, 4, 9)):
        idx[perm[pos:pos + reps]] = 10 + k
        pos += reps
    idx[perm[pos:pos + 100]] = -1
    pos += 100
    idx[perm[pos:]] = torch.randint(20, 40, (n - pos,), generator=g)
    named = set(idx[idx >= 0].tolist())
    assert int((idx == -1).sum()) == 100 and int((idx == 7).sum()) == 500 and len(named) == 27
    wide_src = torch.randn(n, C + 24, generator=g).to(torch.bfloat16).to(DEV)
    src = wide_src[:, 8:8 + C]
    wide_out = torch.randn(V, C + 16, generator=g).to(DEV)
    out = wide_out[:, 8:8 + C]
    assert src.stride(0) == C + 24 and out.stride(0) == C + 16 and not out.is_contiguous()
    out0, wide0, src0 = out.clone(), wide_out.clone(), wide_src.clone()
    K.scatter_add_rows(src, idx.to(torch.int32).to(DEV), out)
    keep = idx >= 0
    s64 = src.double().cpu()[keep]
    want = out0.double().cpu().index_add_(0, idx[keep], s64)
    mag = out0.double().cpu().abs().index_add_(0, idx[keep], s64.abs())
    count = torch.bincount(idx[keep], minlength=V).double()[:, None]
    err = (out.double().cpu() - want).abs()
    tol = count * 2.0 ** -24 * mag
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"scatter_add_rows C={C}: worst error / tolerance {worst:.3f}; hot row max error {float(err[7].max()):.3e}")
    assert bool((err <= tol).all()), worst
    unnamed = [r for r in range(V) if r not in named]
    assert len(unnamed) == 23 and torch.equal(out[unnamed], out0[unnamed])          # (tolerance 0 there as well: count = 0)
    assert torch.equal(wide_out[:, :8], wide0[:, :8]) and torch.equal(wide_out[:, 8 + C:], wide0[:, 8 + C:])
    assert torch.equal(wide_src, src0)
    assert float((out[7] - out0[7]).abs().max()) > 1.0                               # the hot row did receive its 500 terms
