"""GPU: the shared-prefix decode attention (csrc/attention_shared.hip, kernels.attn_decode_shared) by value.

One decode step for B sequences whose first P cache rows are the same tokens: row b attends keys [0, P) of cache slot 0,
keys [P, len_b) of its own slot and its own new key (RoPE at position len_b, appended at row len_b of slot b).

Inputs as tests/test_attention_cont_gpu.py builds them: seeded randn, caches longer than needed, the rows behind each
len_b hold x40 garbage (row len_b itself is overwritten by the append), and in the cache the kernel under test sees the slots
b >= 1 hold garbage in rows [0, P) as well, so a prefix read from the wrong slot shows.

Yardsticks, computed on clean caches that carry the prefix in every slot: fp32 torch softmax attention from the rotated
q / k that K.rope_qkv produces; e_decode = the max error of K.attn_decode(kv_lens_dev, rope_pos_dev=None); e_tiled = the
max error of K.flash_attn_cont per row with Tq = 1 (the existing kernel that, like the MFMA PV product here, rounds the
probabilities to 16 bits).  Asserted: finite; within 2e-2 + 2e-2 |want| (tests/test_kernels_gpu.py::test_flash_attention);
max error <= 1.25 x max(e_decode, e_tiled) (this project's "no worse than" margin); appended K/V rows bit-equal to the
existing kernel's.

Shapes, the smallest that reach every edge: D = 128 with H in {2, 5} and one D = 64 case; B in {1, 2, 5, 16, 17, 33} (row
groups of 16: one partial, one full, full + 1, two full + 1); P in {0, 1, 15, 16, 17, 64, 333, 1000} (edges of the 16-key
MFMA tiles and the 32-key step, partial and empty key splits); own lengths len_b - P mixed per row from {0, 1, 7, 70};
default splits and 8.  The cross product is thinned: every listed value appears in at least one case of each dtype."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd._lib import HipKernelError

DEV = "cuda"
ATOL, RTOL = 2e-2, 2e-2            # tests/test_kernels_gpu.py::test_flash_attention
OWN = (0, 1, 7, 70)
# (B, H, D, P, splits); own lengths cycle through OWN starting at a case-dependent offset
CASES = [
    (1, 2, 128, 0, None), (2, 5, 128, 1, None), (5, 2, 128, 15, 8), (16, 2, 128, 16, None), (17, 5, 128, 17, None),
    (33, 2, 128, 64, 8), (5, 5, 128, 333, None), (17, 2, 128, 1000, 8), (2, 2, 128, 1000, None), (16, 5, 128, 333, 8),
    (5, 3, 64, 333, None), (17, 3, 64, 17, 8),
]
DTYPES = [torch.bfloat16, torch.float16]
_tables = {}
_built = {}


def _cos_sin(D, rows):
    key = (D, rows)
    if key not in _tables:
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
        ang = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
        _tables[key] = (ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous())
    return _tables[key]


def _lens(B, P, shift):
    return [P + OWN[(b + shift) % 4] for b in range(B)]


def _build(B, H, D, P, dtype, seed, lens=None):
    """-> dict: qkv, the clean caches (prefix in every slot), the caches under test (prefix in slot 0 only), lengths, the
    fp32 yardstick and the outputs / appended rows / errors of the two existing kernels.  Built once per case."""
    key = (B, H, D, P, dtype, seed, tuple(lens) if lens else None)
    if key in _built:
        return _built[key]
    g = torch.Generator(device="cpu").manual_seed(seed)
    HD = H * D
    lens = lens or _lens(B, P, seed)
    t_max = max(lens) + 1 + 37
    qkv = torch.randn(B, 3 * HD, generator=g).to(dtype).to(DEV)
    kc = torch.randn(B, t_max, HD, generator=g).to(dtype).to(DEV)
    vc = torch.randn(B, t_max, HD, generator=g).to(dtype).to(DEV)
    kc[:, :P] = kc[:1, :P]
    vc[:, :P] = vc[:1, :P]
    for b, n in enumerate(lens):           # garbage behind the valid rows: would win every softmax it leaked into
        kc[b, n:] *= 40.0
        vc[b, n:] = vc[b, n:] * 40.0 + 100.0
    kd, vd = kc.clone(), vc.clone()        # what the kernel under test sees: the prefix lives in slot 0 only
    if B > 1 and P > 0:
        kd[1:, :P] *= 40.0
        vd[1:, :P] = vd[1:, :P] * 40.0 + 100.0
    cos, sin = _cos_sin(D, 1200)
    scale = 1.0 / math.sqrt(D)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    # yardstick: rotated q / k by rope_qkv into a clean copy, fp32 softmax attention per row
    kr, vr = kc.clone(), vc.clone()
    q = torch.empty(B, HD, dtype=dtype, device=DEV)
    want = torch.empty(B, HD, dtype=torch.float32, device=DEV)
    tiled = torch.empty(B, HD, dtype=dtype, device=DEV)
    for b, n in enumerate(lens):
        K.rope_qkv(qkv[b:b + 1], cos, sin, q[b:b + 1], kr[b], vr[b], H, D, n)
        qh = q[b].float().view(H, 1, D)
        kh = kr[b, :n + 1].float().view(n + 1, H, D).transpose(0, 1)
        vh = vr[b, :n + 1].float().view(n + 1, H, D).transpose(0, 1)
        want[b] = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).reshape(HD)
        tiled[b] = K.flash_attn_cont(q[b].view(1, 1, HD), kr[b:b + 1, :n + 1], vr[b:b + 1, :n + 1], H, scale).view(HD)
    ke, ve = kc.clone(), vc.clone()
    work = K.DecodeAttnWorkspace(H, D, DEV, splits=8, batch=B)
    dec = K.attn_decode(None, ke, ve, H, scale, work, qkv=qkv, cos=cos, sin=sin, kv_lens_dev=lens_dev, rope_pos_dev=None)
    torch.cuda.synchronize()
    r = dict(qkv=qkv, kd=kd, vd=vd, kc=kc, vc=vc, lens=lens, lens_dev=lens_dev, cos=cos, sin=sin, scale=scale, want=want,
             ke=ke, ve=ve, e_decode=float((dec.float() - want).abs().max()),
             e_tiled=float((tiled.float() - want).abs().max()),
             plen=torch.tensor([P], dtype=torch.int32, device=DEV))
    _built[key] = r
    return r


def _run(r, B, H, D, P, splits, work=None, host=True):
    k, v = r["kd"].clone(), r["vd"].clone()
    S = splits or K.shared_attn_splits(H, B)
    work = work or K.SharedAttnWorkspace(H, D, DEV, splits=S, batch=B)
    got = K.attn_decode_shared(r["qkv"], k, v, H, r["scale"], work, r["cos"], r["sin"], r["lens_dev"], r["plen"], splits=S,
                               prefix_len=P if host else None, kv_lens=r["lens"] if host else None)
    return got, k, v


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,H,D,P,splits", CASES)
def test_shared_attention_against_fp32_and_the_existing_kernels(B, H, D, P, splits, dtype):
    r = _build(B, H, D, P, dtype, seed=B + P)
    got, k, v = _run(r, B, H, D, P, splits)
    want = r["want"]
    err = (got.float() - want).abs()
    e, bound = float(err.max()), 1.25 * max(r["e_decode"], r["e_tiled"])
    print(f"B={B} H={H} D={D} P={P} splits={splits} {dtype}: max err {e:.3e}, attn_decode {r['e_decode']:.3e}, "
          f"flash_attn_cont {r['e_tiled']:.3e}")
    assert got.dtype == dtype and got.shape == (B, H * D)
    assert bool(torch.isfinite(got.float()).all())
    assert bool((err <= ATOL + RTOL * want.abs()).all()), e
    assert e <= bound, (e, r["e_decode"], r["e_tiled"])
    for b, n in enumerate(r["lens"]):      # the appended rows: the bits of the existing kernel; nothing else was written
        assert torch.equal(k[b, n], r["ke"][b, n]) and torch.equal(v[b, n], r["ve"][b, n]), b
    untouched = torch.ones(k.shape[:2], dtype=torch.bool, device=DEV)
    untouched[torch.arange(B, device=DEV), r["lens_dev"].long()] = False
    assert torch.equal(k[untouched], r["kd"][untouched]) and torch.equal(v[untouched], r["vd"][untouched])


def test_shared_attention_repeat_launch_on_one_workspace_is_bit_equal():
    """Two launches on one workspace, and one of another shape in between: the workspace carries no state."""
    B, H, D, P = 17, 5, 128, 333
    r = _build(B, H, D, P, torch.bfloat16, seed=B + P)
    work = K.SharedAttnWorkspace(H, D, DEV, splits=8, batch=B)
    first, _, _ = _run(r, B, H, D, P, 8, work=work)
    second, _, _ = _run(r, B, H, D, P, 8, work=work)
    assert torch.equal(first, second)
    r2 = _build(5, H, D, 15, torch.bfloat16, seed=20)
    _run(r2, 5, H, D, 15, 3, work=work)
    third, _, _ = _run(r, B, H, D, P, 8, work=work)
    assert torch.equal(first, third)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_shared_attention_row_does_not_depend_on_the_other_rows(dtype):
    """B = 17 against the same rows permuted and against row 3 alone, bit-equal at fixed splits."""
    B, H, D, P, S = 17, 2, 128, 333, 8
    r = _build(B, H, D, P, dtype, seed=B + P)
    full, _, _ = _run(r, B, H, D, P, S)

    def subset(rows):
        """The launch with `rows` (slot 0 keeps the prefix whichever row moves there)."""
        idx = torch.tensor(rows, device=DEV)
        k, v = r["kd"][idx].clone(), r["vd"][idx].clone()
        k[0, :P], v[0, :P] = r["kc"][0, :P], r["vc"][0, :P]
        lens = [r["lens"][i] for i in rows]
        work = K.SharedAttnWorkspace(H, D, DEV, splits=S, batch=len(rows))
        return K.attn_decode_shared(r["qkv"][idx].contiguous(), k, v, H, r["scale"], work, r["cos"], r["sin"],
                                    torch.tensor(lens, dtype=torch.int32, device=DEV), r["plen"], splits=S)

    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).tolist()
    got = subset(perm)
    assert torch.equal(got, full[torch.tensor(perm, device=DEV)])
    assert torch.equal(subset([3])[0], full[3])


def test_shared_attention_refusals():
    B, H, D, P = 2, 2, 128, 16
    r = _build(B, H, D, P, torch.bfloat16, seed=B + P)
    work = K.SharedAttnWorkspace(H, D, DEV, splits=2, batch=B)
    args = (H, r["scale"], work, r["cos"], r["sin"], r["lens_dev"], r["plen"])
    k, v = r["kd"].clone(), r["vd"].clone()
    with pytest.raises(HipKernelError):            # the prefix is longer than a sequence the host knows
        K.attn_decode_shared(r["qkv"], k, v, *args, prefix_len=P, kv_lens=[P - 1, P + 7])
    with pytest.raises(HipKernelError):            # a length beyond the cache
        K.attn_decode_shared(r["qkv"], k, v, *args, prefix_len=P, kv_lens=[P, k.size(1)])
    with pytest.raises(HipKernelError):            # workspace too small for 8 splits
        K.attn_decode_shared(r["qkv"], k, v, *args, splits=8)
    with pytest.raises(HipKernelError):            # more splits than the merge holds
        K.attn_decode_shared(r["qkv"], k, v, *args, splits=33)
    wide = torch.zeros(B, 3 * H * D + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(HipKernelError):            # projection rows that are not 16-byte aligned
        K.attn_decode_shared(wide[:, 4:4 + 3 * H * D], k, v, *args)
    with pytest.raises(HipKernelError):            # head_dim 32
        K.attn_decode_shared(r["qkv"], k, v, 8, r["scale"], work, r["cos"][:, :16].contiguous(),
                             r["sin"][:, :16].contiguous(), r["lens_dev"], r["plen"])
    assert torch.equal(k, r["kd"]) and torch.equal(v, r["vd"])      # a refused call writes nothing
    assert int(work.cnt.abs().sum()) == 0
