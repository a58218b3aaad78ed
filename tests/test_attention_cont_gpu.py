"""GPU: the split-key causal attention of a short query block against a long cache (csrc/attention_cont.hip,
kernels.flash_attn_cont) against fp32 torch softmax attention computed on the GPU from the same 16-bit inputs.

Tolerance: the one tests/test_kernels_gpu.py::test_flash_attention applies to the existing forward (2e-2 absolute + 2e-2
relative); in addition the new kernel's max error may be at most 1.25 x the existing flash_attn's max error against the
same reference on the same inputs (this project's margin for "no worse than").

Shapes: the smallest that reach every edge -- no past (Tk = Tq), a past that is no multiple of the 64-key tile, a last
split that is partial (Tk = 1000: 16 tiles, the last one cut) or empty (Tk = 1027: 17 tiles in runs of 3 leave splits 6, 7
without a tile; splits = 8 forced on 2 tiles), a query block that is not full, one wave (Tq <= 32) and two.  The cache is
longer than Tk and the rows beyond Tk hold large non-zero garbage, so a masking error shows instead of reading zeros."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K

DEV = "cuda"
SHAPES = [(1, 1), (2, 2), (17, 17), (64, 64), (3, 70), (17, 300), (64, 1000), (33, 1027)]
ATOL, RTOL = 2e-2, 2e-2            # tests/test_kernels_gpu.py::test_flash_attention


def _inputs(B, H, D, Tq, Tk, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t_max = Tk + 37
    q = torch.randn(B, Tq, H * D, generator=g).to(dtype).to(DEV)
    kc = torch.randn(B, t_max, H * D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(B, t_max, H * D, generator=g).to(dtype).to(DEV)
    kc[:, Tk:] *= 40.0                       # garbage behind the valid rows: would win every softmax it leaked into
    vc[:, Tk:] = vc[:, Tk:] * 40.0 + 100.0
    return q, kc, vc


def _ref(q, k, v, heads, scale):
    B, Tq, HD = q.shape
    Tk, D = k.size(1), HD // heads
    qh = q.float().view(B, Tq, heads, D).transpose(1, 2)
    kh = k.float().view(B, Tk, heads, D).transpose(1, 2)
    vh = v.float().view(B, Tk, heads, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale
    i = torch.arange(Tq, device=q.device)[:, None] + (Tk - Tq)
    j = torch.arange(Tk, device=q.device)[None, :]
    s = s.masked_fill(j > i, float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Tq, HD)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Tq,Tk", SHAPES)
def test_cont_attention_against_fp32_and_the_existing_forward(Tq, Tk, dtype):
    D = 128
    scale = 1.0 / math.sqrt(D)
    for H in (2, 5):
        for B in (1, 2):
            q, kc, vc = _inputs(B, H, D, Tq, Tk, dtype, seed=1000 * H + 10 * B + Tq)
            k, v = kc[:, :Tk], vc[:, :Tk]
            want = _ref(q, k, v, H, scale)
            tol = ATOL + RTOL * want.abs()
            base = K.flash_attn(q, k, v, H, scale, True)
            e_base = float((base.float() - want).abs().max())
            for splits in (None, 8):          # the default split count, and 8 (empty splits wherever Tk < 8 tiles)
                got = K.flash_attn_cont(q, k, v, H, scale, splits=splits)
                assert got.dtype == dtype and got.shape == q.shape
                err = (got.float() - want).abs()
                e = float(err.max())
                print(f"H={H} B={B} Tq={Tq} Tk={Tk} {dtype} splits={splits}: max err {e:.3e}, flash_attn {e_base:.3e}")
                assert bool(torch.isfinite(got.float()).all())
                assert bool((err <= tol).all()), (H, B, splits, e)
                assert e <= 1.25 * e_base, (H, B, splits, e, e_base)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cont_attention_head_dim_64(dtype):
    H, D, B, Tq, Tk = 3, 64, 2, 21, 333
    scale = 1.0 / math.sqrt(D)
    q, kc, vc = _inputs(B, H, D, Tq, Tk, dtype, seed=7)
    k, v = kc[:, :Tk], vc[:, :Tk]
    want = _ref(q, k, v, H, scale)
    got = K.flash_attn_cont(q, k, v, H, scale)
    err = (got.float() - want).abs()
    e_base = float((K.flash_attn(q, k, v, H, scale, True).float() - want).abs().max())
    assert bool((err <= ATOL + RTOL * want.abs()).all()), float(err.max())
    assert float(err.max()) <= 1.25 * e_base, (float(err.max()), e_base)


def test_cont_attention_repeat_launch_on_one_workspace_is_bit_equal():
    """Two launches back to back on the same workspace (and one of another shape in between): the workspace carries no
    state from call to call, so the results are bit-equal."""
    H, D, B = 5, 128, 2
    scale = 1.0 / math.sqrt(D)
    work = K.ContAttnWorkspace(H, D, DEV, splits=8, batch=B)
    q, kc, vc = _inputs(B, H, D, 33, 1027, torch.bfloat16, seed=3)
    k, v = kc[:, :1027], vc[:, :1027]
    first = K.flash_attn_cont(q, k, v, H, scale, work=work, splits=8)
    second = K.flash_attn_cont(q, k, v, H, scale, work=work, splits=8)
    assert torch.equal(first, second)
    q2, kc2, vc2 = _inputs(B, H, D, 64, 200, torch.bfloat16, seed=4)
    K.flash_attn_cont(q2, kc2[:, :200], vc2[:, :200], H, scale, work=work, splits=3)
    third = K.flash_attn_cont(q, k, v, H, scale, work=work, splits=8)
    assert torch.equal(first, third)


def test_cont_attention_refuses_what_it_does_not_cover():
    H, D = 2, 128
    q, kc, vc = _inputs(1, H, D, 65, 100, torch.bfloat16, seed=5)
    with pytest.raises(ValueError):
        K.flash_attn_cont(q, kc[:, :100], vc[:, :100], H, 0.1)                 # more than 64 query rows
    with pytest.raises(ValueError):
        K.flash_attn_cont(q[:, :8], kc[:, :4], vc[:, :4], H, 0.1)              # fewer keys than queries
    small = K.ContAttnWorkspace(H, D, DEV, splits=1, batch=1)
    from gpt4roi_amd._lib import HipKernelError
    with pytest.raises(HipKernelError):
        K.flash_attn_cont(q[:, :8], kc[:, :100], vc[:, :100], H, 0.1, work=small, splits=2)   # workspace too small
