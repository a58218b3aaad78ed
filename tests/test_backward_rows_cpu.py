"""CPU: would the comparison of tests/_rows_ref.py notice a wrong backward row kernel?  The unit E of its measure is measured
again on fp32 torch restatements of every operation, and one wrong restatement per plausible kernel mistake must exceed the
bound the GPU tests use by more than 10x, on the very inputs tests/test_backward_rows_gpu.py runs (both take them from
_rows_ref).  The mutants are evaluated in fp64, so all they differ by from the reference is their mistake."""
import pytest
import torch

import _rows_ref as R

F64 = torch.float64


# ------------------------------------------------------------------------------------------ every case, once
def _norm_cases():
    for rows, cols in R.NORM_SHAPES:
        yield (rows, cols), R.norm_case(rows, cols)


def rms_eval(dtype, mutant=None):
    w = 0.0
    for (rows, cols), c in _norm_cases():
        if mutant == "mean_over_padded_width" and cols % R.SLOT == 0:
            continue                                                  # (the padded width IS the width there)
        if mutant == "dgamma_drops_last_row_of_8" and rows < 8:
            continue
        want = R.rmsnorm_ref(c["x"], c["gamma"], c["dy"], c["dres"], c["dgamma0"])
        w = max(w, R.worst_of(R.rmsnorm_formula(c["x"], c["gamma"], c["dy"], c["dres"], c["dgamma0"], dtype=dtype, mutant=mutant), want))
        want = R.rmsnorm_ref(c["x"], c["gamma"], c["dy"])             # no dres: the cond loses its |dres| term
        got = R.rmsnorm_formula(c["x"], c["gamma"], c["dy"], None, c["dgamma0"], dtype=dtype, mutant=mutant)
        w = max(w, R.worst_of(got, want, ["dx"]))
    return w


def ln_eval(dtype, mutant=None, relu=(False, True)):
    w = 0.0
    for _, c in _norm_cases():
        for relu_in in relu:
            want = R.layernorm_ref(c["x"], c["gamma"], c["dy"], c["dgamma0"], c["dbeta0"], relu_in=relu_in)
            got = R.layernorm_formula(c["x"], c["gamma"], c["dy"], c["dgamma0"], c["dbeta0"], relu_in=relu_in, dtype=dtype, mutant=mutant)
            w = max(w, R.worst_of(got, want))
    return w


def swiglu_eval(dtype, mutant=None):
    w = 0.0
    for T, Fd in R.SWIGLU_SHAPES:
        c = R.swiglu_case(T, Fd)
        w = max(w, R.worst_of(R.swiglu_formula(c["gu"], c["dy"], dtype=dtype, mutant=mutant), R.swiglu_ref(c["gu"], c["dy"])))
    return w


def rope_eval(dtype, mutant=None):
    w = 0.0
    for D, pos0 in R.ROPE_CASES:
        c = R.rope_case(D, pos0)
        args = (c["dq"], c["dk"], c["dv"], c["cos"], c["sin"], R.ROPE_HEADS, pos0)
        for batch in (R.ROPE_B, 1):
            w = max(w, R.worst_of(R.rope_formula(*args, batch=batch, dtype=dtype, mutant=mutant), R.rope_ref(*args, batch=batch)))
    return w


def ce_eval(dtype, mutant=None):
    w = 0.0
    for N, n_pad in R.CE_SHAPES:
        for rows in R.CE_ROWS:
            for variant in R.CE_VARIANTS:
                c = R.ce_case(rows, N, variant)
                want = R.ce_ref(c["logits"], c["labels"], c["gs"], c["loss0"], n_pad)
                w = max(w, R.worst_of(R.ce_formula(c["logits"], c["labels"], c["gs"], c["loss0"], n_pad, dtype=dtype, mutant=mutant), want))
    return w


def colsum_eval(dtype):
    w = 0.0
    for M in R.COLSUM_M:
        for N in R.COLSUM_N:
            c = R.colsum_case(M, N)
            w = max(w, R.worst_of(R.colsum_formula(c["x"], c["out0"], dtype=dtype), R.colsum_ref(c["x"], c["out0"])))
    return w


EVALS = dict(rmsnorm_bwd=rms_eval, layernorm_bwd=ln_eval, swiglu_il=swiglu_eval, rope_qkv_bwd=rope_eval,
             cross_entropy=ce_eval, colsum=colsum_eval)


# ------------------------------------------------------------------------------------------ the unit
def test_fp32_restatements_measure_the_unit():
    es = {name: f(torch.float32) for name, f in EVALS.items()}
    for name, e in es.items():
        print(f"fp32 torch {name}: {e:.3f} units")
    e = max(es.values())
    print(f"E measured {e:.3f} (E = {R.E}, R = 2^-22, BOUND = {R.BOUND})")
    assert 0.25 < e <= R.E                  # (far below: the unit would be slack; above: _rows_ref.E is stale)


def test_fp64_restatements_agree_with_the_autograd_references():
    """The hand-written formulas (the ones the mutants vary) and the autograd references are two statements of the same
    operation: in fp64 they differ by the output's final rounding alone (half an ulp: up to one unit for bf16)."""
    for name, f in EVALS.items():
        e = f(F64)
        print(f"fp64 formula {name}: {e:.3f} units")
        assert e <= 1.0, name


def test_shifted_logits_have_the_reference_of_the_unshifted_ones():
    for N, n_pad in R.CE_SHAPES:
        c0 = R.ce_case(19, N)
        w0 = R.ce_ref(c0["logits"], c0["labels"], c0["gs"], torch.zeros(1), n_pad)
        for variant in ("shift+", "shift-"):
            c = R.ce_case(19, N, variant)
            assert torch.equal(c["logits"].double(), c0["logits"].double() + (R.CE_SHIFT if variant == "shift+" else -R.CE_SHIFT))
            w = R.ce_ref(c["logits"], c["labels"], c["gs"], torch.zeros(1), n_pad)
            assert float((w["loss"][0] - w0["loss"][0]).abs()) < 1e-9 * float(w0["loss"][0].abs())
            assert float((w["dlogits"][0] - w0["dlogits"][0]).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------ the mutants
MUTANTS = [
    ("rmsnorm_bwd", rms_eval, "no_mean_term"),
    ("rmsnorm_bwd", rms_eval, "mean_over_padded_width"),
    ("rmsnorm_bwd", rms_eval, "dgamma_from_x"),
    ("rmsnorm_bwd", rms_eval, "dgamma_drops_last_row_of_8"),
    ("layernorm_bwd", ln_eval, "no_mean_gdy_term"),
    ("layernorm_bwd", lambda dt, m: ln_eval(dt, m, relu=(True,)), "relu_mask_on_output_only"),
    ("swiglu_il", swiglu_eval, "sigma_only"),
    ("swiglu_il", swiglu_eval, "gate_up_swapped"),
    ("rope_qkv_bwd", rope_eval, "forward_rotation"),
    ("rope_qkv_bwd", rope_eval, "positions_do_not_restart"),
    ("cross_entropy", ce_eval, "no_grad_scale"),
    ("cross_entropy", ce_eval, "onehot_at_label_plus_1"),
    ("cross_entropy", ce_eval, "pad_columns_not_zeroed"),
    ("cross_entropy", ce_eval, "ignored_row_contributes_loss"),
]


@pytest.mark.parametrize("op,evaluate,mutant", MUTANTS, ids=[f"{m[0]}-{m[2]}" for m in MUTANTS])
def test_mutant_exceeds_the_bound_tenfold(op, evaluate, mutant):
    ratio = evaluate(F64, mutant) / R.BOUND
    print(f"mutant {op} {mutant}: {ratio:.3g} x BOUND")
    assert ratio > 10.0


def test_weakest_element_is_what_the_measure_protects():
    """max|got - want| / max|want|, the measure the older kernel tests use, passes a wrong pad column next to N in dlogits
    and a wrong tail column of dgamma; this one does not."""
    N, n_pad = R.CE_SHAPES[3]
    c = R.ce_case(19, N)
    want = R.ce_ref(c["logits"], c["labels"], c["gs"], c["loss0"], n_pad)["dlogits"]
    got = R.ce_formula(c["logits"], c["labels"], c["gs"], c["loss0"], n_pad, dtype=F64)["dlogits"]
    got[0, N] = 1e-4                                                    # the pad column next to N
    assert float((got.double() - want[0]).abs().max() / want[0].abs().max()) < 1e-2
    assert R.worst(got, *want) > 10.0 * R.BOUND
    c = R.norm_case(37, 2056)
    want = R.rmsnorm_ref(c["x"], c["gamma"], c["dy"], c["dres"], c["dgamma0"])["dgamma"]
    got = R.rmsnorm_formula(c["x"], c["gamma"], c["dy"], c["dres"], c["dgamma0"], dtype=F64)["dgamma"]
    got[-1] += 1e-3 * want[0].abs().max().float()                       # the last column of the partly filled slot
    assert float((got.double() - want[0]).abs().max() / want[0].abs().max()) < 1e-2
    assert R.worst(got, *want) > 10.0 * R.BOUND
