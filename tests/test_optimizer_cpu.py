"""CPU: would the optimizer comparison of tests/_optim_ref.py notice a wrong update?  The unit of `update_error` is measured on
torch's own fp32 step, an fp32 restatement of the kernels' formula must sit inside the bound the GPU tests use (and outside it
without the derived bias-correction term), and nine wrong restatements of the step must each exceed that bound by 10x on the
very inputs the GPU tests run (tests/test_optimizer_gpu.py takes `make_case` and the schedule from the same module)."""
import math

import numpy as np
import pytest
import torch

import _optim_ref as R


def _zeros(p0):
    return [torch.zeros_like(p) for p in p0]


def _scaled(grads, ps):
    return [g.float() * ps for g in grads]


# ------------------------------------------------------------------------------------------ the unit
def test_torch_fp32_step_measures_the_unit():
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False) in fp32 against ref_step from the same state, every step."""
    worst = 0.0
    for betas in R.BETAS:
        p0, grads = R.make_case()
        params = [torch.nn.Parameter(p.clone()) for p in p0]
        opt = torch.optim.AdamW(params, lr=R.LR, betas=betas, eps=R.EPS, weight_decay=R.WD, foreach=False)
        for step in range(1, R.STEPS + 1):
            before = [p.detach().clone() for p in params]
            m0 = [opt.state[p]["exp_avg"].clone() if opt.state[p] else torch.zeros_like(p) for p in params]
            v0 = [opt.state[p]["exp_avg_sq"].clone() if opt.state[p] else torch.zeros_like(p) for p in params]
            for p, g in zip(params, _scaled(grads[step - 1], R.PRE_SCALE)):
                p.grad = g
            torch.nn.utils.clip_grad_norm_(params, R.MAX_NORM, foreach=False)
            opt.step()
            pr, mr, vr, _ = R.ref_step(before, m0, v0, grads[step - 1], step, R.LR, betas, R.EPS, R.WD, R.MAX_NORM, R.PRE_SCALE)
            e = max(R.worst(before, [p.detach() for p in params], pr), R.worst(m0, [opt.state[p]["exp_avg"] for p in params], mr),
                    R.worst(v0, [opt.state[p]["exp_avg_sq"] for p in params], vr))
            print(f"torch fp32 betas {betas} step {step}: {e:.3f} units")
            worst = max(worst, e)
    print(f"e_torch = {worst:.3f} units (E_TORCH = {R.E_TORCH}, BOUND = {R.BOUND})")
    assert 0.25 < worst <= R.E_TORCH            # (far below: the unit would be slack; above: _optim_ref.E_TORCH is stale)


def _kernel_formula_fp32(p, m, v, grads, step, lr, betas, eps, wd, max_norm, pre_scale):
    """g4r_multi_adamw_f32's arithmetic in fp32 torch ops and numpy float32 scalars, operation for operation."""
    f = np.float32
    b1, b2 = f(betas[0]), f(betas[1])
    bc1, bc2 = f(1) - np.power(b1, f(step)), f(1) - np.power(b2, f(step))
    ib1, ib2 = f(1) / bc1, f(1) / bc2
    norm = f(math.sqrt(R.sumsq(grads))) * f(pre_scale)
    c = f(max_norm) / (norm + f(1e-6))
    gscale = f(pre_scale) * (c if c < f(1) else f(1))
    decay = f(1) - f(lr) * f(wd)
    po, mo, vo = [], [], []
    for pi, mi, vi, gi in zip(p, m, v, grads):
        gi = gi.float() * float(gscale)
        mi = mi * float(b1) + gi * float(f(1) - b1)
        vi = vi * float(b2) + gi * float(f(1) - b2) * gi
        pi = pi * float(decay) - (mi * float(ib1)) * float(f(lr)) / ((vi * float(ib2)).sqrt() + float(f(eps)))
        po.append(pi)
        mo.append(mi)
        vo.append(vi)
    return po, mo, vo


def test_fp32_restatement_of_the_kernel_formula_needs_the_derived_term():
    with_term, without = 0.0, 0.0
    for betas in R.BETAS:
        p0, grads = R.make_case()
        p, m, v = p0, _zeros(p0), _zeros(p0)
        for step in range(1, R.STEPS + 1):
            args = (grads[step - 1], step, R.LR, betas, R.EPS, R.WD, R.MAX_NORM, R.PRE_SCALE)
            got = _kernel_formula_fp32(p, m, v, *args)
            want = R.ref_step(p, m, v, *args)[:3]
            r = R.R0 + R.bias_term(betas, step)
            for b, a, w in zip((p, m, v), got, want):
                assert all(x.dtype == torch.float32 for x in a)
                with_term = max(with_term, R.worst(b, a, w, r))
                without = max(without, R.worst(b, a, w, R.R0))
            p, m, v = got
    print(f"fp32 kernel formula: {with_term:.2f} units with the bias-correction term ({with_term / R.BOUND:.2f} x BOUND), "
          f"{without:.2f} units without it ({without / R.BOUND:.2f} x BOUND)")
    assert with_term <= R.BOUND < without


# ------------------------------------------------------------------------------------------ mutants
MUTANTS = ("no_weight_decay", "l2_decay_in_gradient", "bias_correction_at_step_minus_1", "no_bias_correction",
           "clip_coefficient_not_clamped", "clipping_skipped", "eps_inside_sqrt", "norm_without_pre_scale", "beta2_on_exp_avg")


def mutant_step(kind, p, m, v, grads, step, lr, betas, eps, wd, max_norm, pre_scale):
    """ref_step with one thing wrong (kind None: nothing wrong, bit-equal to ref_step)."""
    assert kind is None or kind in MUTANTS
    p, m, v, g = (R._f64(x) for x in (p, m, v, grads))
    b1, b2 = betas
    norm = math.sqrt(R.sumsq(grads)) * (1.0 if kind == "norm_without_pre_scale" else pre_scale)
    coef = max_norm / (norm + 1e-6)
    if kind != "clip_coefficient_not_clamped":
        coef = min(1.0, coef)
    if kind == "clipping_skipped":
        coef = 1.0
    t = step - 1 if kind == "bias_correction_at_step_minus_1" else step
    bc1, bc2 = (1.0, 1.0) if kind == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    po, mo, vo = [], [], []
    for pi, mi, vi, gi in zip(p, m, v, g):
        gi = gi * (pre_scale * coef)
        if kind == "l2_decay_in_gradient":
            gi = gi + wd * pi
        mi = (b2 if kind == "beta2_on_exp_avg" else b1) * mi + (1.0 - (b2 if kind == "beta2_on_exp_avg" else b1)) * gi
        vi = b2 * vi + (1.0 - b2) * gi * gi
        decay = 1.0 if kind in ("no_weight_decay", "l2_decay_in_gradient") else 1.0 - lr * wd
        den = (vi / bc2 + eps).sqrt() if kind == "eps_inside_sqrt" else (vi / bc2).sqrt() + eps
        pi = pi * decay - lr * (mi / bc1) / den
        po.append(pi)
        mo.append(mi)
        vo.append(vi)
    return po, mo, vo


def _run_mutant(kind, betas):
    """The mutant plays the kernel: its fp32-stored state evolves over the four steps, and every step is compared with
    ref_step from the state before it, exactly as the GPU test does.  Returns per step the error of p in BOUNDs, and the
    worst over p, m and v.  (A step that leaves non-finite values is flagged; the run goes on from the reference's result.)"""
    p0, grads = R.make_case()
    p, m, v = p0, _zeros(p0), _zeros(p0)
    on_p, on_all = [], []
    for step in range(1, R.STEPS + 1):
        args = (grads[step - 1], step, R.LR, betas, R.EPS, R.WD, R.MAX_NORM, R.PRE_SCALE)
        got = mutant_step(kind, p, m, v, *args)
        want = R.ref_step(p, m, v, *args)[:3]
        r = R.R0 + R.bias_term(betas, step)
        e = [R.worst(b, a, w, r) for b, a, w in zip((p, m, v), got, want)]
        on_p.append(e[0] / R.BOUND)
        on_all.append(max(e) / R.BOUND)
        nxt = got if all(math.isfinite(x) for x in e) else want
        p, m, v = ([x.float() for x in xs] for xs in nxt)       # the kernel stores fp32
    return on_p, on_all


def test_unmutated_restatement_is_ref_step():
    p0, grads = R.make_case()
    args = (p0, _zeros(p0), _zeros(p0), grads[0], 1, R.LR, R.BETAS[0], R.EPS, R.WD, R.MAX_NORM, R.PRE_SCALE)
    for got, want in zip(mutant_step(None, *args), R.ref_step(*args)[:3]):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    for betas in R.BETAS:                       # stored in fp32 between the steps, the reference itself stays inside one unit
        assert max(_run_mutant(None, betas)[1]) * R.BOUND <= 1.0


@pytest.mark.parametrize("kind", MUTANTS)
def test_mutant_exceeds_the_gpu_bound_tenfold(kind):
    for betas in R.BETAS:
        on_p, on_all = _run_mutant(kind, betas)
        finite = max(x for x in on_p if math.isfinite(x))
        print(f"mutant {kind} betas {betas}: parameter update {max(on_p):.3g} x BOUND (worst finite step {finite:.3g}), "
              f"parameter and moments {max(on_all):.3g} x BOUND")
        assert finite >= 10.0, (kind, betas, on_p)


# ------------------------------------------------------------------------------------------ the reference itself
def test_ref_step_clip_cases():
    p0, grads = R.make_case()
    z = _zeros(p0)
    base = (p0, z, z, grads[0], 1, R.LR, R.BETAS[0], R.EPS, R.WD)
    own = R.sumsq(grads[0])
    info = R.ref_step(*base, 1.0, 0.5)[3]
    assert info["total_sq"] == own and info["coef"] == 1.0 / (math.sqrt(own) * 0.5 + 1e-6) < 1e-2
    assert R.ref_step(*base, None, 0.5)[3]["coef"] == 1.0 and R.ref_step(*base, 0, 0.5)[3]["coef"] == 1.0
    assert R.ref_step(*base, 1e6, 0.5)[3]["coef"] == 1.0                                  # clamped
    info = R.ref_step(*base, 1.0, 0.5, total_sq=torch.tensor([4.0 * own], dtype=torch.float64))[3]
    assert info["total_sq"] == own and info["coef"] == 1.0 / (math.sqrt(4.0 * own) * 0.5 + 1e-6)
    # against torch on one tensor, on the parameter (coarse: the fine comparison is test_torch_fp32_step_measures_the_unit)
    q = torch.nn.Parameter(p0[2].clone())
    q.grad = grads[0][2].float() * 0.5
    torch.nn.utils.clip_grad_norm_([q], 1.0)
    torch.optim.AdamW([q], lr=R.LR, betas=R.BETAS[0], eps=R.EPS, weight_decay=R.WD).step()
    want = R.ref_step([p0[2]], [z[2]], [z[2]], [grads[0][2]], 1, R.LR, R.BETAS[0], R.EPS, R.WD, 1.0, 0.5)[0][0]
    assert float((q.detach().double() - want).abs().max()) < 1e-6


def test_update_error_is_taken_on_the_update():
    before = torch.tensor([1.0, 1.0, 0.0, 3.0])
    ref = before.double() + torch.tensor([1e-3, 1e-3, 1e-3, 0.0], dtype=torch.float64)
    got = before.double() + torch.tensor([1.1e-3, 1e-3, float("nan"), 2.0 ** -22], dtype=torch.float64)
    e = R.update_error(before, got, ref)
    assert abs(float(e[0]) - 1e-4 / (R.R0 * 1e-3 + 2.0 ** -23)) < 1e-6 * float(e[0])       # 10 % of the update: ~830 units
    assert float(e[1]) == 0.0 and math.isinf(float(e[2])) and float(e[3]) == 1.0           # one ulp of 3.0 is 2^-22
    assert float(R.ulp32(torch.tensor([0.75]))) == 2.0 ** -24


def test_torch_slice_restatement_matches_ref_step():
    """The stand-in that tests/test_sharded_gloo.py and tests/test_fsdp_gloo.py inject for the fused kernels."""
    for betas in R.BETAS:
        p0, grads = R.make_case()
        p, m, v = [x.clone() for x in p0], _zeros(p0), _zeros(p0)
        for step in range(1, R.STEPS + 1):
            gs = grads[step - 1]
            total = torch.tensor([R.sumsq(gs)], dtype=torch.float64)
            want = R.ref_step(p, m, v, gs, step, R.LR, betas, R.EPS, R.WD, R.MAX_NORM, 1.0)[:3]
            before = [[x.clone() for x in xs] for xs in (p, m, v)]
            for pi, mi, vi, gi in zip(p, m, v, gs):
                R.torch_adamw_slice(pi, mi, vi, gi.float(), R.LR, step, betas, R.EPS, R.WD, total, R.MAX_NORM)
            for b, a, w in zip(before, (p, m, v), want):
                assert R.worst(b, a, w) <= R.BOUND
