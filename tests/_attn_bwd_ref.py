"""fp64 reference of the attention backward (csrc/attention_bwd.hip: attn_delta_kernel, attn_bwd_dq_kernel,
attn_bwd_dkv_kernel), the inputs the two test files share and the measure they compare with
(tests/test_attention_bwd_cpu.py, tests/test_attention_bwd_gpu.py).  A plain helper module: no fixtures, no pytest settings.

The reference.  attn_bwd_ref restates O = softmax(Q K^T scale + mask) V in fp64 on exactly the bf16 values the kernel receives
and takes dq, dk, dv from autograd through it; key j is visible to query i where j <= i + (Tk - Tq) (causal) or everywhere.
It returns O, the natural-domain LSE, (ref, cond) per gradient and (ref, cond) of the log2-domain LSE the forward stores.

The measure is the one of tests/_rows_ref.py, per element, no max over max:

    err = |got - ref| / (U_BF16 * |ref| + r * cond + FLOOR)

cond is the sum of the absolute values of the terms the formula adds.  With P the probabilities, dP = dO V^T and
A_i = sum_d |dO_id O_id| (the terms of Delta_i):

    cond_dv = P^T |dO|        cond_dq = scale * (P * (|dP| + A)) |K|        cond_dk = scale * (P * (|dP| + A))^T |Q|

r = 2^-9 here, NOT the 2^-22 of the row kernels: the kernel stores P and dS = P (dP - Delta) scale as bf16 before the second
MFMAs and reads O as bf16 to form Delta.  Each of those is a rounding of half a bf16 ulp (2^-9) of a term cond counts.  They are
part of the operation's contract (it is what makes the second products bf16 MFMAs), not slack: an implementation that kept P
in fp32 would read far below one unit, one that rounded anything else to bf16 would read above the bound.  A non-finite `got`
reads infinite and no element is left out: a dq row whose dO is 0 has ref = cond = 0, so anything but 0 there reads > 1e30.

The unit.  attn_bwd_formula restates the kernel's arithmetic in torch on the CPU with its rounding points (S and dP from the
bf16 operands, P = exp2(S * scale * log2e - lse2), Delta from the bf16 O, P and dS rounded to bf16, outputs rounded to bf16);
it takes o and lse as arguments, as the kernel does: o = bf16(reference O), lse2 = fp32(reference LSE * log2e).  With
dtype=float32 it was judged with this measure against the fp64 reference on every case of CASES:

    causal Tq = Tk in 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257        D 64: 1.516   D 128: 1.368
    causal Tk - Tq in 1, 63, 64, 80 at Tq in 1, 70, 130                         D 64: 1.434   D 128: 1.639
    non-causal (33, 33), (130, 130), (130, 33), (33, 130), (65, 1)              D 64: 1.495   D 128: 1.518
    B = 3, H = 3: (64, 130, 130, causal), (128, 130, 33, non-causal)            1.529, 0.927
    second Delta pass: (32, 64, 128, 65, 65), (32, 128, 64, 65, 65), causal     1.700, 1.774
    production (1, 4, 128, 767, 767, causal)                                    1.448

(dq alone 0.90, dk alone 1.09; the worst is always dv) so E = 1.8 (test_attention_bwd_cpu.py measures it again and asserts
that it stays within (0.25 E, E]).  The same formula in fp64 -- only the bf16 roundings of O, P, dS and of the outputs left --
reads the same to three digits: the unit IS those roundings, and 2 is their ceiling for dv (every P of a column rounded the
same way by its full half ulp, 2^-9 cond, and the final rounding of a value just above a power of two, 2^-8 |ref|); the cases
with the most elements come closest.  The kernels are allowed BOUND = 4 * E = 7.2 units, the margin of the row and region
kernels, for the same things: MFMA accumulation order, exp2 by hardware, Delta summed in another order.  E is measured against
the reference, never against the GPU kernel.

The inputs (attn_case).  The heads differ on purpose so that every edge element carries weight the measure can see:
head 0 peaked (q * 6: LSE large, P near one-hot, dS nearly cancelled); head 1 diagonal-dominant (k[j] += 0.5 q[j - off]: P at
(i, i + off) is 0.1 or more even at T = 767, so a lost diagonal or a lost last key shows -- without it one key of hundreds sits
below the bf16 rounding allowance of the sum, which is a property of the sum, not of the measure); head 2 flat (plain randn);
head 3, causal shapes, future-aligned: for up to three rows i, k[i + off + 1] = 32 q[i], a MASKED key whose recomputed exp2
overflows to +inf, which the kernel's select must turn into an exact zero.  Heads beyond 4 repeat the kinds; the two cases of
the second Delta pass alternate peaked and flat only.  Everywhere: query rows Tq // 3 and 2 Tq // 3 have dO = 0 exactly, what
_attn_ragged_bwd feeds for pad rows (where Tq >= 3: with fewer rows nothing would be left to compare); key row Tk // 2 repeats
row Tk // 2 - 1; q holds three exact zeros and one -0.0.

The forward's LSE (chained tests) is judged with the row kernels' own r = 2^-22 and bound (4 units of _rows_ref): it is an fp32
chain -- cond = |max| + |log2 sum 2^(x - max)| + sum_j P_ij scale log2e sum_d |q_id k_jd|.

Every mutant of test_attention_bwd_cpu.py exceeds BOUND by more than 10x on the same inputs; the ratios are printed there.
"""
import functools
import math

import torch

from _rows_ref import FLOOR, U_BF16, error, worst, worst_of  # noqa: F401  (the measure, re-exported for the two test files)
from _rows_ref import BOUND as LSE_BOUND, R as LSE_R         # the forward's LSE: an fp32 chain, judged like the row kernels

R_ATTN = 2.0 ** -9               # half a bf16 ulp: P, dS and O are bf16 by contract (module docstring)
LOG2E = 1.4426950408889634
E = 1.8                          # measured 1.774 (module docstring); rounded up
BOUND = 4.0 * E                  # units of `error` the kernels may reach

TB = 64                          # rows of a streamed tile (keys for dQ, queries for dK/dV)
WAVE_ROWS = 32                   # rows one wave owns
DELTA_PASS = 8192 * 256          # work items one grid-stride pass of attn_delta_kernel covers


def wg_rows(D):
    """Rows (queries for dQ, keys for dK/dV) of one workgroup."""
    return 128 if D == 128 else 64


# ---- the cases both files run: (B, H, D, Tq, Tk, causal) -----------------------------------------------------------------
SQUARE_T = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257)
OFFSETS, OFFSET_TQ = (1, 63, 64, 80), (1, 70, 130)
NONCAUSAL = ((33, 33), (130, 130), (130, 33), (33, 130), (65, 1))
SQUARE_CASES = tuple((1, 4, D, T, T, True) for D in (64, 128) for T in SQUARE_T)
OFFSET_CASES = tuple((1, 4, D, Tq, Tq + off, True) for D in (64, 128) for Tq in OFFSET_TQ for off in OFFSETS)
NONCAUSAL_CASES = tuple((1, 4, D, Tq, Tk, False) for D in (64, 128) for Tq, Tk in NONCAUSAL)
BATCH_CASES = ((3, 3, 64, 130, 130, True), (3, 3, 128, 130, 33, False))
BIG_CASES = ((32, 64, 128, 65, 65, True), (32, 128, 64, 65, 65, True))       # second pass of attn_delta_kernel
PROD_CASE = (1, 4, 128, 767, 767, True)                                      # LLaMA prefill
SMALL_CASES = SQUARE_CASES + OFFSET_CASES + NONCAUSAL_CASES + BATCH_CASES
CASES = SMALL_CASES + BIG_CASES + (PROD_CASE,)
CHAINED_CASES = (PROD_CASE, (1, 4, 128, 129, 129, True), (1, 4, 64, 65, 65, True), (1, 4, 128, 70, 150, True),
                 (1, 4, 64, 130, 33, False), BATCH_CASES[0])
LAYOUT_CASES = tuple((2, 3, D, 70, Tk, True) for D in (64, 128) for Tk in (70, 150))
KINDS = ("peaked", "diagonal", "flat", "future")


def case_id(key):
    B, H, D, Tq, Tk, causal = key
    return f"B{B}-H{H}-D{D}-{Tq}x{Tk}-{'causal' if causal else 'full'}"


def head_kinds(key):
    B, H, D, Tq, Tk, causal = key
    if key in BIG_CASES:
        return tuple(KINDS[2 * (h % 2)] for h in range(H))
    return tuple("flat" if KINDS[h % 4] == "future" and not causal else KINDS[h % 4] for h in range(H))


def zero_do_rows(Tq):
    return sorted({Tq // 3, 2 * Tq // 3}) if Tq >= 3 else []


def future_pairs(Tq, Tk):
    """(i, j): masked key j = i + off + 1 aligned with query i (causal shapes)."""
    off = Tk - Tq
    return [(i, i + off + 1) for i in sorted({0, Tq // 2, Tq - 2}) if i >= 0 and i + off + 1 < Tk]


def attn_case(B, H, D, Tq, Tk, causal):
    """bf16 CPU tensors q, do [B, Tq, H * D], k, v [B, Tk, H * D] and the scale (module docstring: the head kinds, the dO = 0
    rows, the repeated key row, the zeros of q)."""
    key = (B, H, D, Tq, Tk, causal)
    g = torch.Generator().manual_seed(((B * 131 + H) * 131 + D) * 100003 + Tq * 1009 + Tk * 2 + int(causal))
    q, do = torch.randn(B, Tq, H, D, generator=g), torch.randn(B, Tq, H, D, generator=g)
    k, v = torch.randn(B, Tk, H, D, generator=g), torch.randn(B, Tk, H, D, generator=g)
    off = Tk - Tq
    kinds = head_kinds(key)
    j = torch.arange(max(off, 0), min(Tk, Tq + off))
    for h, kind in enumerate(kinds):
        if kind == "peaked":
            q[:, :, h] *= 6.0
        if kind == "diagonal":
            k[:, j, h] += 0.5 * q[:, j - off, h]
    q, k, v, do = (t.to(torch.bfloat16) for t in (q, k, v, do))
    if Tk >= 2:
        k[:, Tk // 2] = k[:, Tk // 2 - 1]
    q[0, 0, 0, 1], q[0, Tq // 2, H - 1, 5], q[0, Tq - 1, 0, D - 1], q[0, 0, 0, 2] = 0.0, 0.0, 0.0, -0.0
    for h, kind in enumerate(kinds):
        if kind == "future":
            for i, jj in future_pairs(Tq, Tk):
                k[:, jj, h] = 32.0 * q[:, i, h]                       # exact in bf16
    do[:, zero_do_rows(Tq)] = 0.0
    flat = lambda t: t.reshape(t.size(0), t.size(1), H * D).contiguous()  # noqa: E731
    return dict(q=flat(q), k=flat(k), v=flat(v), do=flat(do), heads=H, scale=1.0 / math.sqrt(D), causal=causal)


# ---- fp64 reference ------------------------------------------------------------------------------------------------------
def _split(t, heads, dtype):
    B, T, HD = t.shape
    return t.detach().to(dtype).view(B, T, heads, HD // heads).transpose(1, 2)      # [B, H, T, D]


def _merge(t):
    B, H, T, D = t.shape
    return t.transpose(1, 2).reshape(B, T, H * D)


def visible(Tq, Tk, causal, device="cpu", strict=False, off=None):
    off = Tk - Tq if off is None else off
    i, j = torch.arange(Tq, device=device)[:, None], torch.arange(Tk, device=device)[None, :]
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool, device=device)
    return j < i + off if strict else j <= i + off


def _ref_chunk(q, k, v, do, heads, scale, causal):
    f64 = torch.float64
    Q, K, V, G = (_split(t, heads, f64) for t in (q, k, v, do))
    Tq, Tk = Q.size(2), K.size(2)
    mask = visible(Tq, Tk, causal, q.device)
    Ql, Kl, Vl = (t.clone().requires_grad_(True) for t in (Q, K, V))
    S = (Ql @ Kl.transpose(-1, -2) * scale).masked_fill(~mask, float("-inf"))
    O = torch.softmax(S, -1) @ Vl
    (O * G).sum().backward()
    with torch.no_grad():
        S = S.detach()
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        O = O.detach()
        W = P * ((G @ V.transpose(-1, -2)).abs() + (G * O).abs().sum(-1, keepdim=True))
        m = S.max(-1).values
        qk = (Q.abs() @ K.abs().transpose(-1, -2)) * scale * LOG2E
        clse = (m.abs() + (lse - m).abs()) * LOG2E + (P * qk).sum(-1)
        return dict(o=_merge(O), lse=lse, lse2=(lse * LOG2E, clse),
                    dq=(_merge(Ql.grad), _merge(scale * (W @ K.abs()))),
                    dk=(_merge(Kl.grad), _merge(scale * (W.transpose(-1, -2) @ Q.abs()))),
                    dv=(_merge(Vl.grad), _merge(P.transpose(-1, -2) @ G.abs())))


def attn_bwd_ref(q, k, v, do, heads, scale, causal):
    """-> dict: o [B, Tq, H * D], lse [B, H, Tq] (natural domain), lse2 = (ref, cond) of the log2-domain LSE, and
    dq, dk, dv = (ref, cond), all fp64.  Works on the device of its inputs, eight batch elements at a time."""
    parts = [_ref_chunk(q[b:b + 8], k[b:b + 8], v[b:b + 8], do[b:b + 8], heads, scale, causal) for b in range(0, q.size(0), 8)]
    cat = lambda xs: torch.cat(list(xs))  # noqa: E731
    return {n: (cat(p[n][0] for p in parts), cat(p[n][1] for p in parts)) if isinstance(parts[0][n], tuple)
            else cat(p[n] for p in parts) for n in parts[0]}


@functools.lru_cache(maxsize=None)
def _reference_small(key):
    c = attn_case(*key)
    return c, attn_bwd_ref(c["q"], c["k"], c["v"], c["do"], c["heads"], c["scale"], c["causal"])


def reference(key, device="cpu"):
    """(case, reference) of a case key; computed once per key, except the two large cases of the second Delta pass, which are
    computed where asked (on `device`) and not kept."""
    if key not in BIG_CASES:
        return _reference_small(key)
    c = attn_case(*key)
    c = {n: t.to(device) if torch.is_tensor(t) else t for n, t in c.items()}
    return c, attn_bwd_ref(c["q"], c["k"], c["v"], c["do"], c["heads"], c["scale"], c["causal"])


def kernel_inputs(ref):
    """o and lse as the isolated kernel receives them: bf16(reference O), fp32(reference LSE in the log2 domain)."""
    return ref["o"].to(torch.bfloat16), (ref["lse"] * LOG2E).to(torch.float32)


def worst_grads(got, ref):
    """{dq, dk, dv: worst reading}; got: name -> bf16 tensor."""
    return {n: worst(got[n], *ref[n], r=R_ATTN) for n in ("dq", "dk", "dv")}


# ---- the kernel's arithmetic in torch: dtype=float32 measures the unit, a mutant (in fp64) shows what the measure can see ----
MUTANTS = ("strict_diagonal", "lse_natural", "no_delta", "delta_over_d_minus_8", "ds_without_scale",
           "dkv_drops_last_partial_q_tile", "dkv_drops_last_q_row", "dkv_counts_clamped_rows", "dq_counts_clamped_keys",
           "dq_drops_last_key_tile", "dq_drops_last_key", "dq_drops_first_key", "q_begin_rounded_up", "q_begin_ignores_offset",
           "lse_from_neighbour", "dk_columns_swapped", "v_from_next_head", "offset_ignored", "inf_multiplied")
# Not a mistake: a dK/dV workgroup that starts at kblock - off, not rounded down to a tile, skips only queries i < kblock - off,
# and those see no key of the block (i + off < kblock).  test_attention_bwd_cpu.py shows that it changes no bit.
NO_OP_MUTANTS = ("q_begin_unrounded",)


def mutant_applies(mutant, key):
    """False where the mistake changes nothing by construction (the CPU test skips those shapes)."""
    B, H, D, Tq, Tk, causal = key
    off = Tk - Tq
    if mutant in ("strict_diagonal", "q_begin_unrounded", "q_begin_rounded_up"):
        return causal
    if mutant in ("offset_ignored", "q_begin_ignores_offset"):
        return causal and off > 0 and (mutant == "offset_ignored" or Tk > wg_rows(D))
    if mutant == "inf_multiplied":
        return causal and "future" in head_kinds(key) and bool(future_pairs(Tq, Tk))
    if mutant in ("dkv_drops_last_partial_q_tile", "dkv_counts_clamped_rows"):
        return Tq % TB != 0
    if mutant == "dq_counts_clamped_keys":
        return not causal and Tk % TB != 0        # causal: the clamped keys lie beyond every query's diagonal
    if mutant == "lse_from_neighbour":
        return Tq >= 2
    if mutant == "v_from_next_head":
        return H >= 2
    return True


def _weights(mutant, D, Tq, Tk, causal, dtype):
    """How often each (query, key) pair is counted by the dQ kernel and by the dK/dV kernel: the visibility mask, which a
    tiling mistake zeroes (rows or keys dropped) or multiplies (clamped duplicates of the last row or key counted)."""
    off = Tk - Tq
    vis = visible(Tq, Tk, causal, strict=mutant == "strict_diagonal", off=0 if mutant == "offset_ignored" else None)
    wq, wkv = vis.to(dtype), vis.to(dtype)
    QB = KB = wg_rows(D)
    if mutant == "dkv_drops_last_partial_q_tile" and Tq % TB:
        wkv[Tq // TB * TB:] = 0
    if mutant == "dkv_drops_last_q_row":
        wkv[Tq - 1] = 0
    if mutant == "dkv_counts_clamped_rows" and Tq % TB:
        wkv[Tq - 1] *= 1 + TB - Tq % TB
    if mutant == "dq_counts_clamped_keys" and not causal and Tk % TB:
        wq[:, Tk - 1] *= 1 + TB - Tk % TB
    if mutant == "dq_drops_last_key_tile":
        for qb in range(0, Tq, QB):
            kend = min(Tk, qb + QB + off) if causal else Tk
            wq[qb:qb + QB, (kend - 1) // TB * TB:] = 0
    if mutant == "dq_drops_last_key":
        wq[:, Tk - 1] = 0
    if mutant == "dq_drops_first_key":
        wq[:, 0] = 0
    if mutant in ("q_begin_unrounded", "q_begin_rounded_up", "q_begin_ignores_offset") and causal:
        for kb in range(0, Tk, KB):
            first = max(kb - off, 0)                                  # first query that sees the first key of this block
            lo, hi = {"q_begin_unrounded": (first // TB * TB, first),  # starts at `first`: skips the rows of its tile before it
                      "q_begin_rounded_up": (0, -(-first // TB) * TB),
                      "q_begin_ignores_offset": (0, kb // TB * TB)}[mutant]
            wkv[lo:hi, kb:kb + KB] = 0
    return wq, wkv


def attn_bwd_formula(q, k, v, o, do, lse2, heads, scale, causal, dtype=torch.float32, mutant=None):
    """dq, dk, dv (bf16) as the kernels form them; lse2 fp32 [B, H, Tq], log2 domain."""
    assert mutant is None or mutant in MUTANTS + NO_OP_MUTANTS, mutant
    bf = torch.bfloat16
    Q, K, V, O, G = (_split(t.cpu(), heads, dtype) for t in (q, k, v, o, do))
    D, Tq, Tk = Q.size(3), Q.size(2), K.size(2)
    L = lse2.detach().cpu().to(dtype)
    if mutant == "lse_natural":
        L = L / LOG2E
    wq, wkv = _weights(mutant, D, Tq, Tk, causal, dtype)
    S = Q @ K.transpose(-1, -2)
    dP = G @ (V.roll(-1, 1) if mutant == "v_from_next_head" else V).transpose(-1, -2)
    sc2 = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).to(dtype)
    go = G * O
    delta = (go[..., :D - 8] if mutant == "delta_over_d_minus_8" else go).sum(-1)
    if mutant == "no_delta":
        delta = torch.zeros_like(delta)
    ds_scale = 1.0 if mutant == "ds_without_scale" else scale

    def side(L, w):
        x = S * sc2 - L[..., None]
        e = torch.where(x >= 128.0, torch.full_like(x, float("inf")), torch.exp2(x))   # the kernel's exp2 is an fp32 instruction
        P = e * (w != 0).to(dtype) if mutant == "inf_multiplied" else torch.where(w != 0, e, torch.zeros_like(e))
        dS = P * (dP - delta[..., None]) * ds_scale
        return P.to(bf).to(dtype) * w, dS.to(bf).to(dtype) * w       # every counted copy is the same rounded value

    _, dSq = side(L, wq)
    Lkv = L
    if mutant == "lse_from_neighbour" and Tq >= 2:
        r = min(TB + 1, Tq - 1)
        Lkv = L.clone()
        Lkv[..., r] = L[..., r - 1]
    Pk, dSk = side(Lkv, wkv)
    dq, dk, dv = dSq @ K, dSk.transpose(-1, -2) @ Q, Pk.transpose(-1, -2) @ G
    if mutant == "dk_columns_swapped":
        dk = dk.clone()
        dk[..., [3, 4]] = dk[..., [4, 3]]
    return dict(dq=_merge(dq).to(bf), dk=_merge(dk).to(bf), dv=_merge(dv).to(bf))
