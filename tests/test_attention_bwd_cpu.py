"""CPU: would the comparison of tests/_attn_bwd_ref.py notice a wrong attention backward?  The unit E of its measure is measured
again on the fp32 torch restatement of the kernels' arithmetic, and one wrong restatement per plausible kernel mistake must
exceed the bound the GPU tests use by more than 10x, on the very inputs tests/test_attention_bwd_gpu.py runs (both take them
from _attn_bwd_ref).  The mutants are evaluated in fp64 with the kernels' rounding points kept (bf16 O, P, dS and outputs, the
fp32 range of exp2), so all they differ by from the clean restatement is their mistake."""
import functools

import pytest
import torch

import _attn_bwd_ref as A

F32, F64 = torch.float32, torch.float64
MUTANT_CASES = A.SMALL_CASES + (A.PROD_CASE,)           # (the two cases of the second Delta pass hold no edge the others lack)


def formula(key, dtype, mutant=None):
    c, ref = A.reference(key)
    o, lse2 = A.kernel_inputs(ref)
    got = A.attn_bwd_formula(c["q"], c["k"], c["v"], o, c["do"], lse2, c["heads"], c["scale"], c["causal"], dtype=dtype, mutant=mutant)
    return got, ref


@functools.lru_cache(maxsize=None)
def clean_readings():
    """{key: (fp32 reading, fp64 reading or None)}, every case once."""
    out = {}
    for key in A.CASES:
        if key in A.BIG_CASES:                          # built and dropped: 2048 and 4096 problems of 65 x 65
            c, ref = A.reference(key)
            o, lse2 = A.kernel_inputs(ref)
            got = A.attn_bwd_formula(c["q"], c["k"], c["v"], o, c["do"], lse2, c["heads"], c["scale"], c["causal"], dtype=F32)
            out[key] = (A.worst_grads(got, ref), None)
        else:
            out[key] = tuple(A.worst_grads(*formula(key, dt)) for dt in (F32, F64))
    return out


# ------------------------------------------------------------------------------------------ the table reaches every path
def test_layout_reaches_every_path():
    assert len(set(A.CASES)) == len(A.CASES)
    sq = {D: {Tq for (_, _, d, Tq, Tk, c) in A.SQUARE_CASES if d == D and Tq == Tk and c} for D in (64, 128)}
    for D in (64, 128):
        W, T = A.wg_rows(D), sq[D]
        assert T == set(A.SQUARE_T)
        assert 1 in T                                                          # one lane of one wave
        assert {A.WAVE_ROWS - 1, A.WAVE_ROWS, A.WAVE_ROWS + 1} <= T            # the edge between two waves
        assert {A.TB - 1, A.TB, A.TB + 1} <= T                                 # the edge of a streamed tile
        assert {W - 1, W, W + 1} <= T                                          # the edge of a workgroup, at this width
        assert any(t // A.TB >= 3 and t % A.TB for t in T)                     # a ragged tile after three full ones (193)
        assert any(t > 2 * W and t % W for t in T)                             # a third, ragged workgroup (257)
    off_cases = {(D, Tq, Tk - Tq) for (_, _, D, Tq, Tk, c) in A.OFFSET_CASES}
    assert off_cases == {(D, Tq, off) for D in (64, 128) for Tq in (1, 70, 130) for off in (1, 63, 64, 80)}
    assert all(c for *_, c in A.OFFSET_CASES) and all(not c for *_, c in A.NONCAUSAL_CASES)
    for D in (64, 128):                                 # a dK/dV workgroup whose kblock - off lies inside a tile ...
        KB = A.wg_rows(D)
        firsts = {(kb - off) for (d, Tq, off) in off_cases if d == D for kb in range(0, Tq + off, KB) if 0 < kb - off < Tq}
        assert any(f % A.TB and f < A.TB for f in firsts)                      # ... of the first tile: q_begin rounds down to 0
        assert any(f % A.TB and f > A.TB for f in firsts)                      # ... of a later tile: q_begin rounds down to 64
        assert any(f % A.TB == 0 for f in firsts)                              # and one where it is a tile's first row
    nc = {(Tq, Tk) for (_, _, _, Tq, Tk, _) in A.NONCAUSAL_CASES}
    assert nc == {(33, 33), (130, 130), (130, 33), (33, 130), (65, 1)}
    assert any(Tk < Tq for Tq, Tk in nc) and any(Tk == 1 for _, Tk in nc) and any(Tq % A.TB and Tk % A.TB and Tq != Tk for Tq, Tk in nc)
    assert all(B == 3 and H == 3 for (B, H, *_) in A.BATCH_CASES) and {c for *_, c in A.BATCH_CASES} == {True, False}
    for B, H, D, Tq, Tk, causal in A.BIG_CASES:         # the second grid-stride pass of attn_delta_kernel, by arithmetic
        items = B * Tq * H * (D // 8)
        assert items == 2129920 and A.DELTA_PASS == 2097152 and A.DELTA_PASS < items < 2 * A.DELTA_PASS and causal
        assert set(A.head_kinds((B, H, D, Tq, Tk, causal))) == {"peaked", "flat"}
    assert {D for (_, _, D, *_) in A.BIG_CASES} == {64, 128}
    assert A.PROD_CASE == (1, 4, 128, 767, 767, True) and A.CASES.count(A.PROD_CASE) == 1
    for key in A.SQUARE_CASES + A.OFFSET_CASES + (A.PROD_CASE,):
        assert A.head_kinds(key) == ("peaked", "diagonal", "flat", "future")
    for key in A.NONCAUSAL_CASES:
        assert A.head_kinds(key) == ("peaked", "diagonal", "flat", "flat")
    assert len(A.CHAINED_CASES) == 6 and A.PROD_CASE in A.CHAINED_CASES and any(not c for *_, c in A.CHAINED_CASES)
    assert set(A.CHAINED_CASES) <= set(A.CASES)
    assert set(A.LAYOUT_CASES) == {(2, 3, D, 70, Tk, True) for D in (64, 128) for Tk in (70, 150)}


def test_inputs_hold_what_they_are_for():
    for key in A.SMALL_CASES + (A.PROD_CASE,):
        B, H, D, Tq, Tk, causal = key
        c, ref = A.reference(key)
        q4, k4 = c["q"].view(B, Tq, H, D), c["k"].view(B, Tk, H, D)
        rows = A.zero_do_rows(Tq)
        assert (len(rows) == 2 or Tq < 6) and Tq - 1 not in rows and bool((c["do"][:, rows] == 0).all())
        for n in ("dq",):                               # dO = 0 rows: reference and condition are exactly 0, so only 0 passes
            assert bool((ref[n][0][:, rows] == 0).all()) and bool((ref[n][1][:, rows] == 0).all())
        live = [i for i in range(Tq) if i not in rows]
        assert bool((c["do"][:, live] != 0).any(-1).all())
        if Tk >= 2:
            assert torch.equal(c["k"][:, Tk // 2], c["k"][:, Tk // 2 - 1])
        assert int((c["q"] == 0).sum()) >= 4 and int((torch.signbit(c["q"]) & (c["q"] == 0)).sum()) == 1
        kinds = A.head_kinds(key)
        lse2 = ref["lse"] * A.LOG2E
        P = torch.exp((q4.double().transpose(1, 2) @ k4.double().transpose(1, 2).transpose(-1, -2)) * c["scale"] - ref["lse"][..., None])
        P = P * A.visible(Tq, Tk, causal)
        if "future" in kinds:
            h = kinds.index("future")
            pairs = A.future_pairs(Tq, Tk)
            assert bool(pairs) == (Tq >= 2)
            for i, j in pairs:                          # masked, and the recomputed exponent is beyond the fp32 range
                assert j > i + (Tk - Tq)
                x = (q4[:, i, h].double() * k4[:, j, h].double()).sum(-1) * c["scale"] * A.LOG2E - lse2[:, h, i]
                assert bool((x > 128.0).all()), (key, i, j, x)
        if Tq >= 2 and min(Tq, Tk) > 1:                 # the diagonal of head 1 carries weight, the last key of the last row too
            h, off = kinds.index("diagonal"), Tk - Tq
            i = torch.arange(max(0, -off), Tq)
            diag = P[:, h, i, i + off]
            assert float(diag.median()) > 0.1, (key, float(diag.median()))
            assert float(P[:, h, Tq - 1, Tk - 1].min()) > 0.02, (key, float(P[:, h, Tq - 1, Tk - 1].min()))
        h = kinds.index("peaked")
        if Tq >= 31:                                    # most rows of head 0 put most of their weight on one key
            assert float(P[:, h].max(-1).values.median()) > 0.5 and float(ref["lse"][:, h].max()) > 10.0


# ------------------------------------------------------------------------------------------ the unit
GROUPS = (("causal Tq = Tk", A.SQUARE_CASES), ("causal Tk > Tq", A.OFFSET_CASES), ("non-causal", A.NONCAUSAL_CASES),
          ("B = 3, H = 3", A.BATCH_CASES), ("second Delta pass", A.BIG_CASES), ("production", (A.PROD_CASE,)))


def test_fp32_restatement_measures_the_unit():
    r = clean_readings()
    for name, keys in GROUPS:
        for D in (64, 128):
            ks = [k for k in keys if k[2] == D]
            if ks:
                print(f"fp32 torch {name} D {D}: " + " ".join(f"{n} {max(r[k][0][n] for k in ks):.3f}" for n in ("dq", "dk", "dv")))
    e = max(max(v[0].values()) for v in r.values())
    print(f"E measured {e:.3f} (E = {A.E}, r = 2^-9, BOUND = {A.BOUND})")
    assert 0.25 * A.E < e <= A.E                # (far below: the unit would be slack; above: _attn_bwd_ref.E is stale)


def test_fp64_restatement_reads_the_roundings_of_the_contract_alone():
    """The clean formula the mutants vary, in fp64: what is left is the bf16 rounding of O, P, dS and of the outputs, and
    that is the unit -- fp32 accumulation adds nothing visible to it."""
    r = clean_readings()
    e64 = max(max(v[1].values()) for v in r.values() if v[1] is not None)
    e32 = max(max(v[0].values()) for v in r.values() if v[1] is not None)
    print(f"fp64 formula {e64:.3f} units, fp32 {e32:.3f}")
    assert e64 <= A.E and abs(e64 - e32) < 0.05


# ------------------------------------------------------------------------------------------ the mutants
@functools.lru_cache(maxsize=None)
def mutant_ratios(mutant):
    out = {}
    for key in MUTANT_CASES:
        if A.mutant_applies(mutant, key):
            got, ref = formula(key, F64, mutant)
            out[key] = max(A.worst_grads(got, ref).values()) / A.BOUND
    return out


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutant_exceeds_the_bound_tenfold(mutant):
    r = mutant_ratios(mutant)
    best = max(r, key=r.get)
    print(f"mutant {mutant}: {r[best]:.3g} x BOUND at {A.case_id(best)}; over 10 x BOUND at {sum(v > 10.0 for v in r.values())} "
          f"of the {len(r)} shapes where it is a mistake")
    assert r[best] > 10.0


def test_every_required_mistake_has_a_mutant():
    required = {"strict_diagonal", "lse_natural", "no_delta", "delta_over_d_minus_8", "ds_without_scale",
                "dkv_drops_last_partial_q_tile", "dkv_drops_last_q_row", "dkv_counts_clamped_rows", "dq_counts_clamped_keys",
                "dq_drops_last_key_tile", "dq_drops_last_key", "dq_drops_first_key", "lse_from_neighbour", "dk_columns_swapped",
                "v_from_next_head", "offset_ignored", "inf_multiplied"}
    assert required <= set(A.MUTANTS) and {"q_begin_rounded_up", "q_begin_ignores_offset"} <= set(A.MUTANTS)
    assert A.NO_OP_MUTANTS == ("q_begin_unrounded",)


def test_an_unrounded_q_begin_is_no_mistake():
    """`q_begin` of the dK/dV kernel not rounded down to a tile: the rows it skips, floor64(kblock - off) .. kblock - off - 1,
    see no key of the block (i + off < kblock), so nothing changes -- by arithmetic on the mask and bit for bit in the formula.
    What CAN go wrong with q_begin is in MUTANTS: rounded up, and computed without the offset."""
    for key in A.SQUARE_CASES + A.OFFSET_CASES:
        B, H, D, Tq, Tk, causal = key
        off, KB = Tk - Tq, A.wg_rows(D)
        vis = A.visible(Tq, Tk, True)
        for kb in range(0, Tk, KB):
            first = max(kb - off, 0)
            assert not bool(vis[first // A.TB * A.TB:first, kb:kb + KB].any())
        got, _ = formula(key, F64, "q_begin_unrounded")
        clean, _ = formula(key, F64)
        assert all(torch.equal(got[n], clean[n]) for n in ("dq", "dk", "dv"))


def test_the_old_measure_passes_what_this_one_catches():
    """max|got - ref| / max|ref| < 3e-2 on unscaled randn, the measure and the inputs of test_train_gpu.py::
    test_flash_attention_backward, at its (1, 2, 128, 767, 767, causal): a dK/dV kernel that takes row 65's LSE from row 64 and
    a dQ kernel that drops the last key pass it, and one that ignores the last query row sits at its edge
    (printed).  With the inputs of this module, this measure reads each of them over 4 x BOUND at the production shape alone
    (the lost last key: 4.4 x there, 14 x at T = 128)."""
    g = torch.Generator().manual_seed(767)
    q, k, v, do = (torch.randn(1, 767, 256, generator=g).to(torch.bfloat16) for _ in range(4))
    ref = A.attn_bwd_ref(q, k, v, do, 2, 128 ** -0.5, True)
    o, lse2 = A.kernel_inputs(ref)
    for mutant in ("dkv_drops_last_q_row", "lse_from_neighbour", "dq_drops_last_key"):
        got = A.attn_bwd_formula(q, k, v, o, do, lse2, 2, 128 ** -0.5, True, dtype=F64, mutant=mutant)
        old = max(float((got[n].double() - ref[n][0]).abs().max() / ref[n][0].abs().max()) for n in ("dq", "dk", "dv"))
        new = mutant_ratios(mutant)[A.PROD_CASE]
        print(f"{mutant} at T = 767: old measure on flat inputs {old:.4f} (its bound: 0.03), this one {new:.3g} x BOUND")
        assert (old < 3e-2 or mutant == "dkv_drops_last_q_row") and new > 4.0
