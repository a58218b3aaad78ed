"""GPU: the attention backward (csrc/attention_bwd.hip: Delta, dQ and dK/dV kernels) by value against the fp64 reference of
tests/_attn_bwd_ref.py, per element, in the units and under the bound measured there (tests/test_attention_bwd_cpu.py shows on
the same inputs that nineteen wrong formulas exceed that bound by > 10x).

Isolated: o = bf16(reference O) and lse = fp32(reference LSE * log2e), so the backward is judged alone, at every shape of
_attn_bwd_ref.CASES.  Chained: o and lse from K.flash_attn, the production chain, at six shapes.  Layouts: q and dO column
slices of a fused buffer, k and v slices of a longer cache, dq / dk / dv written through `out=` into guarded row-strided views
(carve, guards_intact, sliced of test_backward_rows_gpu), bit-equal to the dense call.  And the exactness claims of the kernel
file's header: two launches agree bit for bit, a batch element does not depend on its neighbours, rows with dO = 0 get dq = 0
exactly, masked scores whose exponential overflows leave everything finite."""
import pytest
import torch

import _attn_bwd_ref as A
from test_backward_rows_gpu import BF16, DEV, GUARD, POISON, carve, guards_intact

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd._lib import HipKernelError

F32 = torch.float32


def dev(c):
    return {n: t.to(DEV) if torch.is_tensor(t) else t for n, t in c.items()}


def report(tag, errs, bound=A.BOUND):
    """errs: name -> reading.  Printed before it is asserted."""
    w = max(errs.values())
    print(f"{tag}: worst {w / bound:.3f} x BOUND (" + " ".join(f"{n} {e:.3f}" for n, e in errs.items()) + f" units, bound {bound})")
    assert w <= bound, (tag, errs)


def backward(d, o, lse2, out=None):
    dq, dk, dv = K.flash_attn_bwd(d["q"], d["k"], d["v"], o, d["do"], lse2, d["heads"], d["scale"], d["causal"], out=out)
    return dict(dq=dq, dk=dk, dv=dv)


def exact_claims(key, d, got):
    """dO = 0 rows: dq exactly 0; the future-aligned head (and every other): finite."""
    B, H, D, Tq, Tk, causal = key
    rows = A.zero_do_rows(Tq)
    assert bool((got["dq"][:, rows] == 0).all())
    assert all(bool(torch.isfinite(t).all()) for t in got.values())


# ---------------------------------------------------------------------------------------------- the backward alone
@pytest.mark.parametrize("key", A.CASES, ids=A.case_id)
def test_backward_isolated(key):
    big = key in A.BIG_CASES
    c, ref = A.reference(key, DEV if big else "cpu")        # (the two large references are formed in fp64 on the device)
    d = dev(c)
    o, lse2 = A.kernel_inputs(ref)
    got = backward(d, o.to(DEV), lse2.to(DEV))
    assert all(t.is_contiguous() and t.dtype == BF16 for t in got.values())
    exact_claims(key, d, got)
    report(f"flash_attn_bwd isolated {A.case_id(key)}", A.worst_grads(got, ref))


# ---------------------------------------------------------------------------------------------- forward, then backward
@pytest.mark.parametrize("key", A.CHAINED_CASES, ids=A.case_id)
def test_backward_chained_to_the_forward(key):
    B, H, D, Tq, Tk, causal = key
    c, ref = A.reference(key)
    d = dev(c)
    lse2 = torch.empty((B, H, Tq), dtype=F32, device=DEV)
    o = K.flash_attn(d["q"], d["k"], d["v"], H, d["scale"], causal, lse=lse2)
    report(f"flash_attn LSE {A.case_id(key)}", dict(lse=A.worst(lse2, *ref["lse2"], r=A.LSE_R)), A.LSE_BOUND)
    got = backward(d, o, lse2)
    exact_claims(key, d, got)
    report(f"flash_attn_bwd chained {A.case_id(key)}", A.worst_grads(got, ref))


# ---------------------------------------------------------------------------------------------- strided inputs, out= views
@pytest.mark.parametrize("key", A.LAYOUT_CASES, ids=A.case_id)
def test_strided_inputs_and_out_views(key):
    B, H, D, Tq, Tk, causal = key
    C, maxT = H * D, Tk + 37
    c, ref = A.reference(key)
    d = dev(c)
    o, lse2 = (t.to(DEV) for t in A.kernel_inputs(ref))
    dense = backward(d, o, lse2)
    fused = torch.full((B, Tq, 3 * C), POISON, dtype=BF16, device=DEV)          # q | poison | dO, as a fused projection leaves them
    fused[:, :, :C], fused[:, :, 2 * C:] = d["q"], d["do"]
    caches = [torch.full((B, maxT, C), POISON, dtype=BF16, device=DEV) for _ in range(2)]
    caches[0][:, :Tk], caches[1][:, :Tk] = d["k"], d["v"]                       # the layout LlamaDecoder.backward passes
    s = dict(d, q=fused[:, :, :C], do=fused[:, :, 2 * C:], k=caches[0][:, :Tk], v=caches[1][:, :Tk])
    assert s["q"].stride(1) == 3 * C and s["k"].stride(0) == maxT * C and not s["k"].is_contiguous()
    if Tk == Tq:                                                # dq | dk | dv: the column slices of one guarded buffer
        buf, view = carve((B * Tq, 3 * C), BF16)
        v3 = view.view(B, Tq, 3 * C)
        bufs, outs = [(buf, view)], tuple(v3[:, :, i * C:(i + 1) * C] for i in range(3))
    else:                                                       # three guarded buffers whose rows are 8 elements apart
        bufs = [carve((B * T, C), BF16, ld=C + 8) for T in (Tq, Tk, Tk)]
        outs = tuple(view.view(B, T, C) for (_, view), T in zip(bufs, (Tq, Tk, Tk)))
    assert all(t.stride(1) > C for t in outs)
    got = backward(s, o, lse2, out=outs)
    assert all(got[n] is t for n, t in zip(("dq", "dk", "dv"), outs))
    assert all(guards_intact(buf, view) for buf, view in bufs)
    assert all(torch.equal(got[n], dense[n]) for n in dense)
    exact_claims(key, d, got)
    report(f"flash_attn_bwd layouts {A.case_id(key)}", A.worst_grads({n: t.contiguous() for n, t in got.items()}, ref))


# ---------------------------------------------------------------------------------------------- the header's exactness claims
@pytest.mark.parametrize("key", A.CHAINED_CASES, ids=A.case_id)
def test_two_launches_agree_bit_for_bit(key):
    """"Nothing is atomically accumulated: results are bit-reproducible.\""""
    c, ref = A.reference(key)
    d = dev(c)
    o, lse2 = (t.to(DEV) for t in A.kernel_inputs(ref))
    first, second = backward(d, o, lse2), backward(d, o, lse2)
    assert all(torch.equal(first[n], second[n]) for n in first)


@pytest.mark.parametrize("key", A.BATCH_CASES, ids=A.case_id)
def test_batch_element_equals_itself_run_alone(key):
    B = key[0]
    c, ref = A.reference(key)
    d = dev(c)
    o, lse2 = (t.to(DEV) for t in A.kernel_inputs(ref))
    whole = backward(d, o, lse2)
    for b in range(B):
        one = dict(d, **{n: d[n][b:b + 1] for n in ("q", "k", "v", "do")})
        alone = backward(one, o[b:b + 1], lse2[b:b + 1].contiguous())
        assert all(torch.equal(alone[n][0], whole[n][b]) for n in whole), b


# ---------------------------------------------------------------------------------------------- what the entry point refuses
def test_entry_point_refuses_before_any_launch():
    def call(heads, Tq, Tk, C, causal, q=None):
        z = lambda T: torch.zeros(1, T, C, dtype=BF16, device=DEV)  # noqa: E731
        outs = tuple(torch.full((1, T, C), GUARD[BF16], dtype=BF16, device=DEV) for T in (Tq, Tk, Tk))
        lse = torch.zeros(1, heads, Tq, dtype=F32, device=DEV)
        try:
            K.flash_attn_bwd(z(Tq) if q is None else q, z(Tk), z(Tk), z(Tq), z(Tq), lse, heads, 0.1, causal, out=outs)
        finally:
            torch.cuda.synchronize()
            assert all(bool((t == GUARD[BF16]).all()) for t in outs)            # nothing was launched
    with pytest.raises(HipKernelError, match="flash_attn_bwd: head_dim must be 64 or 128"):
        call(2, 8, 8, 2 * 96, True)
    with pytest.raises(HipKernelError, match="flash_attn_bwd: causal needs Tk >= Tq"):
        call(2, 9, 8, 128, True)
    wide = torch.zeros(1, 8, 128 + 4, dtype=BF16, device=DEV)
    assert wide[:, :, :128].stride(1) % 8 != 0
    with pytest.raises(HipKernelError, match="flash_attn_bwd: strides must keep 16-byte alignment"):
        call(2, 8, 8, 128, True, q=wide[:, :, :128])
