"""GPU: the memory-bound kernels of csrc/backward.hip that every training step runs between its GEMMs -- rmsnorm_bwd,
layernorm_bwd, swiglu_il and its backward, rope_qkv_bwd, cross_entropy, transpose, colsum, relu_bwd, gather_rows -- by value
against the fp64 references of tests/_rows_ref.py, per element, in the units and under the bound measured there
(tests/test_backward_rows_cpu.py shows on the same inputs that fourteen wrong formulas exceed that bound by > 10x).  The three
kernels that only move values are compared with torch.equal.

Every tensor a kernel writes is a view into a larger buffer: 64 guard elements before and after it and, for a row-strided
output, guard elements between the end of each row and the start of the next.  The guards must come back untouched.  Inputs
are passed both dense and as column slices of wider buffers whose other columns hold 3e38.

The shapes are the smallest that reach each path: norm rows in register slot 0 alone (8, 1024, 2048 columns), in a partly
filled slot 1 (2056 = 257 vectors), in slots 0-1 (4096) and 0-3 (8192), with 1, 8, 9 and 37 rows for the 8-rows-per-workgroup
dgamma path and its ragged last workgroup; one case above the 16384 x 256 work items of a single grid-stride pass for swiglu_il,
swiglu_il_bwd, relu_bwd and gather_rows; the tile edges of transpose (63, 64, 65, 130) and of colsum (255, 256, 257)."""
import pytest
import torch

import _rows_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K
    from gpt4roi_amd._lib import HipKernelError

DEV = "cuda"
PAD = 64
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
GUARD = {F32: 12345.0, BF16: 12288.0, F16: 1234.0}             # (each exact in its type)
POISON = 3.0e38                                                   # what the columns next to a sliced input hold
BIG_N8 = R.GRID_CAP + 256 + 1                                     # relu_bwd: 8-element vectors, just above one pass
GATHER_BIG = (127101, 264)                                        # n * C / 8 = 4 194 333
NORM_VARIANTS = ((True, True, True), (False, False, False), (True, False, True), (False, True, False))   # (strided, dres, dgamma)


# ---------------------------------------------------------------------------------------------- guarded outputs, sliced inputs
def carve(shape, dtype, ld=None, fill=None):
    """(buffer, view): a 1-D [n] or 2-D [rows, cols] view with row stride ld >= cols, PAD guard elements before and after;
    the columns cols..ld of every row are guards too.  fill: a tensor or a number the view starts from."""
    rows, cols = (1, shape) if isinstance(shape, int) else shape
    ld = ld or cols
    buf = torch.full((PAD + rows * ld + PAD,), GUARD[dtype], dtype=dtype, device=DEV)
    view = buf[PAD:PAD + cols] if isinstance(shape, int) else buf[PAD:PAD + rows * ld].view(rows, ld)[:, :cols]
    if fill is not None:
        view.copy_(fill.to(dtype)) if torch.is_tensor(fill) else view.fill_(fill)
    return buf, view


def guards_intact(buf, view):
    b = buf.clone()
    torch.as_strided(b, view.shape, view.stride(), view.storage_offset()).fill_(GUARD[buf.dtype])
    return bool((b == GUARD[buf.dtype]).all())


def sliced(t, before=8, after=8):
    """`t` as a column slice of a wider buffer (row stride = cols + before + after) whose other columns hold POISON."""
    rows, cols = t.shape
    wide = torch.full((rows, before + cols + after), 6.0e4 if t.dtype == F16 else POISON, dtype=t.dtype, device=DEV)
    wide[:, before:before + cols] = t
    view = wide[:, before:before + cols]
    assert view.stride(0) > view.size(1) and torch.equal(view, t.to(DEV))
    return view


def dev(case):
    return {k: v.to(DEV) for k, v in case.items()}


def report(tag, errs):
    w = max(errs) if errs else 0.0
    print(f"{tag}: worst {w / R.BOUND:.3f} x BOUND ({w:.3f} units, bound {R.BOUND})")
    assert w <= R.BOUND, (tag, errs)


# ---------------------------------------------------------------------------------------------- the table reaches every path
def test_layout_reaches_every_path():
    cols = {c for _, c in R.NORM_SHAPES}
    rows = {r for r, _ in R.NORM_SHAPES}
    assert cols == {8, 1024, 2048, 2056, 4096, 8192} and rows == {1, 8, 9, 37}
    slots = {(c - 1) // R.SLOT for c in cols}                          # the highest register slot a row reaches
    assert slots >= {0, 1, 3} and any(c > 2 * R.SLOT + 8 for c in cols)   # 8192 fills slots 0..3, 4096 stops after slot 1
    assert any(c > R.SLOT and c % R.SLOT == 8 for c in cols)            # one vector in slot 1: a partly filled slot
    assert 8 in cols                                                    # 255 of 256 threads hold no column
    assert all(c <= 4 * R.SLOT and c % 8 == 0 for c in cols)
    for c in R.NORM_COLS_SMALL:
        assert {r for r, cc in R.NORM_SHAPES if cc == c} == {1, 8, 9, 37}
    for c in R.NORM_COLS_LARGE:
        assert {r for r, cc in R.NORM_SHAPES if cc == c} == {9, 37}
    assert any(r % 8 for r in rows if r > 8) and 8 in rows              # ragged and full last workgroup of the dgamma path
    assert any(v[0] for v in NORM_VARIANTS) and any(not v[0] for v in NORM_VARIANTS)
    x = sliced(torch.zeros(3, 16, dtype=BF16))
    assert x.stride(0) == 32 and x.size(1) == 16 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
    buf, view = carve((3, 16), BF16, ld=24)
    assert view.stride(0) == 24 and view.shape == (3, 16) and view.data_ptr() % 16 == 0 and guards_intact(buf, view)
    buf[PAD + 16] = 0.0                                                 # a guard between two rows
    assert not guards_intact(buf, view)
    # one grid-stride pass covers GRID_CAP work items; each of these needs a second one
    T, Fd = R.SWIGLU_BIG
    assert R.GRID_CAP < T * (Fd // 4) < 2 * R.GRID_CAP and Fd % 4 == 0  # swiglu_il and swiglu_il_bwd
    assert R.GRID_CAP < BIG_N8 < 2 * R.GRID_CAP                         # relu_bwd
    n, C = GATHER_BIG
    assert R.GRID_CAP < n * (C // 8) < 2 * R.GRID_CAP and C % 8 == 0    # gather_rows
    assert set(R.SWIGLU_SHAPES) == {(1, 4), (45, 352), (3, 11008)}
    assert {N for N, _ in R.CE_SHAPES} == {7, 255, 257, 1003} and min(N for N, _ in R.CE_SHAPES) < 256


# ---------------------------------------------------------------------------------------------- RMSNorm / LayerNorm backward
@pytest.mark.parametrize("rows,cols", R.NORM_SHAPES)
def test_rmsnorm_bwd(rows, cols):
    c = R.norm_case(rows, cols)
    d = dev(c)
    errs = []
    for strided, use_dres, use_dg in NORM_VARIANTS:
        x, dy, dres = ((sliced(d["x"]), sliced(d["dy"], 16, 0), sliced(d["dres"], 0, 24)) if strided
                       else (d["x"], d["dy"], d["dres"]))
        ob, out = carve((rows, cols), BF16, ld=cols + 8 if strided else cols)
        gb, dg = carve(cols, F32, fill=d["dgamma0"]) if use_dg else (None, None)
        got = K.rmsnorm_bwd(x, d["gamma"], dy, dres=dres if use_dres else None, dgamma=dg, out=out)
        assert got is out
        want = R.rmsnorm_ref(c["x"], c["gamma"], c["dy"], c["dres"] if use_dres else None, c["dgamma0"] if use_dg else None)
        errs.append(R.worst(out, *want["dx"]))
        assert guards_intact(ob, out)
        if use_dg:
            errs.append(R.worst(dg, *want["dgamma"]))                   # accumulated onto what dgamma held
            assert guards_intact(gb, dg)
        else:
            fresh = K.rmsnorm_bwd(x, d["gamma"], dy, dres=dres if use_dres else None)
            assert fresh.is_contiguous() and torch.equal(fresh, out)
    report(f"rmsnorm_bwd rows {rows} cols {cols}", errs)


@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("rows,cols", R.NORM_SHAPES)
def test_layernorm_bwd(rows, cols, relu_in):
    c = R.norm_case(rows, cols)
    d = dev(c)
    if relu_in:
        assert bool((c["x"] == 0).any()) and bool((c["x"] < 0).any()) and (rows == 1 or bool((c["x"] == 0).all(1).any()))
    errs = []
    # (strided, dgamma, dbeta, need_dx)
    for strided, use_dg, use_db, need_dx in ((True, True, True, True), (False, True, False, True), (True, False, True, True),
                                             (False, True, True, False), (False, False, False, True)):
        x, dy = (sliced(d["x"]), sliced(d["dy"], 16, 0)) if strided else (d["x"], d["dy"])
        ob, out = carve((rows, cols), BF16, ld=cols + 8 if strided else cols) if need_dx else (None, None)
        gb, dg = carve(cols, F32, fill=d["dgamma0"]) if use_dg else (None, None)
        bb, db = carve(cols, F32, fill=d["dbeta0"]) if use_db else (None, None)
        got = K.layernorm_bwd(x, d["gamma"], dy, dgamma=dg, dbeta=db, relu_in=relu_in, need_dx=need_dx, out=out)
        want = R.layernorm_ref(c["x"], c["gamma"], c["dy"], c["dgamma0"] if use_dg else None, c["dbeta0"] if use_db else None,
                               relu_in=relu_in)
        if need_dx:
            assert got is out
            errs.append(R.worst(out, *want["dx"]))
            assert guards_intact(ob, out)
        else:
            assert got is None
        if use_dg:
            errs.append(R.worst(dg, *want["dgamma"]))
            assert guards_intact(gb, dg)
        if use_db:
            errs.append(R.worst(db, *want["dbeta"]))
            assert guards_intact(bb, db)
        if not (use_dg or use_db):
            fresh = K.layernorm_bwd(x, d["gamma"], dy, relu_in=relu_in)
            assert fresh.is_contiguous() and torch.equal(fresh, out)
    report(f"layernorm_bwd rows {rows} cols {cols} relu_in {relu_in}", errs)


@pytest.mark.parametrize("cols", [8200, 12])
def test_norm_entry_points_reject_widths_they_cannot_hold(cols):
    """More than 4 slots of 2048 columns, or no whole 8-element vectors: the entry point refuses, nothing is launched."""
    x, dy = torch.zeros(2, cols, dtype=BF16, device=DEV), torch.zeros(2, cols, dtype=BF16, device=DEV)
    g = torch.ones(cols, device=DEV)
    with pytest.raises(HipKernelError, match="bad shape"):
        K.rmsnorm_bwd(x, g, dy)
    with pytest.raises(HipKernelError, match="bad shape"):
        K.layernorm_bwd(x, g, dy)


# ---------------------------------------------------------------------------------------------- SwiGLU
def _swiglu_check(T, Fd, d):
    want = R.swiglu_ref(d["gu"], d["dy"])                              # on the device
    yb, y = carve((T, Fd), BF16)
    gb, dgu = carve((T, 2 * Fd), BF16)
    assert K.swiglu_il(d["gu"], out=y) is y and K.swiglu_il_bwd(d["gu"], d["dy"], out=dgu) is dgu
    errs = [R.worst(y, *want["y"]), R.worst(dgu, *want["dgu"])]
    assert guards_intact(yb, y) and guards_intact(gb, dgu)
    return errs, y, dgu


@pytest.mark.parametrize("T,Fd", R.SWIGLU_SHAPES)
def test_swiglu_il_and_backward(T, Fd):
    c = R.swiglu_case(T, Fd)
    d = dev(c)
    errs, y, dgu = _swiglu_check(T, Fd, d)
    assert torch.equal(K.swiglu_il(d["gu"]), y) and torch.equal(K.swiglu_il_bwd(d["gu"], d["dy"]), dgu)
    report(f"swiglu_il T {T} F {Fd}", errs)


def test_swiglu_special_gates_are_all_run():
    """+-0, +-20, +-90 and the largest finite bf16 of either sign, by bit pattern, over the three small shapes."""
    bits = lambda t: set(t.contiguous().view(torch.int16).flatten().tolist())  # noqa: E731
    seen = set()
    for T, Fd in R.SWIGLU_SHAPES:
        seen |= bits(R.swiglu_case(T, Fd)["gu"][:, 0::2].flatten()[:8])
    assert seen >= bits(torch.tensor(R.SPECIAL_GATES).to(BF16)) and len(bits(torch.tensor(R.SPECIAL_GATES).to(BF16))) == 8
    assert float(torch.tensor(R.BF16_MAX).to(BF16)) == R.BF16_MAX


def test_swiglu_above_the_grid_cap():
    """T * F / 4 = 4 199 425 work items: the grid-stride step of both kernels runs (33.6 M gate / up values)."""
    T, Fd = R.SWIGLU_BIG
    g = torch.Generator(device=DEV).manual_seed(5)
    gu = (torch.randn(T, 2 * Fd, generator=g, device=DEV) * 2.0).to(BF16)
    dy = torch.randn(T, Fd, generator=g, device=DEV).to(BF16)
    small = dev(R.swiglu_case(1, 8))                                    # the special gates, in the first and in the LAST row
    gu[0, :16], dy[0, :8] = small["gu"][0], small["dy"][0]
    gu[-1, -16:], dy[-1, -8:] = small["gu"][0], small["dy"][0]
    errs, _, _ = _swiglu_check(T, Fd, dict(gu=gu, dy=dy))
    report(f"swiglu_il T {T} F {Fd} (above the grid cap)", errs)


# ---------------------------------------------------------------------------------------------- rope
@pytest.mark.parametrize("D,pos0", R.ROPE_CASES)
def test_rope_qkv_bwd(D, pos0):
    B, T, H = R.ROPE_B, R.ROPE_T, R.ROPE_HEADS
    rows, HD = B * T, H * D
    c = R.rope_case(D, pos0)
    d = dev(c)
    wide = torch.full((rows, 3 * HD + 24), POISON, dtype=BF16, device=DEV)      # dq, dk, dv: column slices of one buffer
    views = [wide[:, i * (HD + 8):i * (HD + 8) + HD] for i in range(3)]
    for v, k in zip(views, ("dq", "dk", "dv")):
        v.copy_(d[k])
    errs = []
    for period in (0, T):
        batch = B if period else 1
        span = pos0 + (period if period else rows)
        cos, sin = d["cos"][:span].contiguous(), d["sin"][:span].contiguous()   # tables exactly as long as the call reads
        want = R.rope_ref(c["dq"], c["dk"], c["dv"], c["cos"], c["sin"], H, pos0, batch=batch)["dqkv"]
        results = []
        for strided in (False, True):
            dq, dk, dv = views if strided else (d["dq"], d["dk"], d["dv"])
            ob, out = carve((rows, 3 * HD), BF16)
            assert K.rope_qkv_bwd(dq, dk, dv, cos, sin, H, D, pos0, out=out, period=period) is out
            errs.append(R.worst(out, *want))
            assert guards_intact(ob, out)
            assert torch.equal(out[:, 2 * HD:], d["dv"])                         # dv passes through unchanged
            fresh = K.rope_qkv_bwd(dq, dk, dv, cos, sin, H, D, pos0, period=period)
            assert fresh.is_contiguous() and torch.equal(fresh, out)
            results.append(out)
        assert torch.equal(results[0], results[1])
        if period:                                  # the batched entry == B calls of the single-sequence one, bit for bit
            parts = [K.rope_qkv_bwd(*(t[b * T:(b + 1) * T] for t in views), cos, sin, H, D, pos0) for b in range(B)]
            assert torch.equal(torch.cat(parts), results[0])
    report(f"rope_qkv_bwd D {D} pos0 {pos0}", errs)


# ---------------------------------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("rows", R.CE_ROWS)
@pytest.mark.parametrize("N,n_pad", R.CE_SHAPES)
def test_cross_entropy(N, n_pad, rows):
    errs = []
    for variant in R.CE_VARIANTS:
        c = R.ce_case(rows, N, variant)
        d = dev(c)
        want = R.ce_ref(c["logits"], c["labels"], c["gs"], c["loss0"], n_pad)
        if variant.startswith("shift"):                 # judged against the UNSHIFTED reference, on the cond of what it reads
            c0 = R.ce_case(rows, N)
            w0 = R.ce_ref(c0["logits"], c0["labels"], c0["gs"], c0["loss0"], n_pad)
            want = {k: (w0[k][0], want[k][1]) for k in want}
        if variant == "dominant":
            lab = int(c["labels"][0])
            assert rows == 19 or lab >= 0
            if 0 <= lab < N:                            # softmax 1 - tiny at the label: the gradient there is near 0
                assert 0 < abs(float(want["dlogits"][0][0, lab])) < 1e-6 * float(c["gs"])
        valid = (c["labels"] >= 0) & (c["labels"] < N)
        assert bool(valid.any()) != (variant == "all_ignored")
        for layout in ("dense", "sliced", "loss_only"):
            logits = d["logits"]
            if layout == "sliced":
                wide = torch.full((rows, N + 5), POISON, dtype=F32, device=DEV)
                wide[:, 3:3 + N] = d["logits"]
                logits = wide[:, 3:3 + N]
                assert logits.stride(0) > N
            lb, loss = carve(1, F32, fill=d["loss0"])                            # non-zero before the call: accumulated onto
            if layout == "loss_only":
                assert K.cross_entropy(logits, d["labels"], loss) is None
            else:
                db, dl = carve((rows, n_pad), BF16, ld=n_pad + 8 if layout == "sliced" else n_pad, fill=R.CE_PREFILL)
                assert (dl.stride(0) > n_pad) == (layout == "sliced")
                K.cross_entropy(logits, d["labels"], loss, d["gs"], dl, n_pad if layout == "dense" else None)
                errs.append(R.worst(dl, *want["dlogits"]))
                assert guards_intact(db, dl)
                assert float(dl[:, N:].abs().max() if n_pad > N else 0.0) == 0.0      # pad columns: exactly 0
                assert float(dl[~valid.to(DEV)].abs().max() if not bool(valid.all()) else 0.0) == 0.0   # ignored rows: exactly 0
            errs.append(R.worst(loss, *want["loss"]))
            assert guards_intact(lb, loss)
            if variant == "all_ignored":
                assert float(loss) == float(c["loss0"])
    report(f"cross_entropy rows {rows} N {N} n_pad {n_pad}", errs)


# ---------------------------------------------------------------------------------------------- the kernels that move values
EDGES = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("Rr", EDGES)
def test_transpose(Rr):
    g = torch.Generator().manual_seed(Rr)
    for C in EDGES:
        x = torch.randn(Rr, C, generator=g).to(BF16).to(DEV)
        for r_pad in (Rr, -(-Rr // 64) * 64, Rr + 130):
            want = torch.zeros(C, r_pad, dtype=BF16, device=DEV)
            want[:, :Rr] = x.t()
            got = K.transpose(x, r_pad)
            assert got.shape == (C, r_pad) and torch.equal(got, want)
            ob, out = carve((C, r_pad), BF16, ld=r_pad + 8, fill=5.0)
            assert K.transpose(sliced(x, 8, 3), r_pad, out=out) is out            # strided input, ld_out > r_pad
            assert torch.equal(out, want) and guards_intact(ob, out)
    assert K.transpose(x).shape == (C, Rr)


@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum(M):
    errs = []
    for N in R.COLSUM_N:
        c = R.colsum_case(M, N)
        d = dev(c)
        ob, out = carve(N, F32, fill=d["out0"])
        assert K.colsum(sliced(d["x"], 8, 5), out=out) is out                    # strided input, accumulated onto `out`
        errs.append(R.worst(out, *R.colsum_ref(c["x"], c["out0"])["out"]))
        assert guards_intact(ob, out)
        errs.append(R.worst(K.colsum(d["x"]), *R.colsum_ref(c["x"], torch.zeros(N))["out"]))
    report(f"colsum M {M}", errs)


def _relu_inputs(n, device):
    g = torch.Generator(device=device).manual_seed(n % 1000)
    y = torch.randn(n, generator=g, device=device).to(BF16)
    dy = torch.randn(n, generator=g, device=device).to(BF16)
    bits = torch.tensor([0x0000, -0x8000, 0x0001, -0x7FFF], dtype=torch.int16, device=device)   # +0, -0, +-2^-133
    for at in (0, n - 4):                               # in the first and in the last vector
        y.view(torch.int16)[at:at + 4] = bits
    return y, dy


@pytest.mark.parametrize("n", [8, 2048 + 8, 8 * BIG_N8])
def test_relu_bwd(n):
    y, dy = _relu_inputs(n, DEV)
    positive = y.view(torch.int16) > 0                  # sign clear and not zero, the smallest subnormal included (no NaN in y)
    want = torch.where(positive, dy, torch.zeros_like(dy))
    ob, out = carve(n, BF16)
    assert K.relu_bwd(y, dy, out=out) is out
    assert torch.equal(out, want) and guards_intact(ob, out)
    assert not bool(torch.signbit(out[~positive]).any())               # the zeros are +0
    if n < 10000:
        assert torch.equal(K.relu_bwd(y.view(-1, 8), dy.view(-1, 8)), want.view(-1, 8))


def _gather_check(src, idx, n_src, C, dtype, out_ld):
    want = src[idx.clamp(min=0).long()].clone()
    want[idx < 0] = 0
    ob, out = carve((idx.numel(), C), dtype, ld=out_ld, fill=5.0)
    assert K.gather_rows(src, idx, out=out) is out
    assert torch.equal(out, want) and guards_intact(ob, out)
    return want


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [8, 264])
def test_gather_rows(C, dtype):
    n_src = 70
    g = torch.Generator().manual_seed(C)
    src = torch.randn(n_src, C, generator=g).to(dtype).to(DEV)
    idx = torch.tensor([-1, 5, 5, 0, n_src - 1, -1, n_src - 1, 0, 33], dtype=torch.int32, device=DEV)
    want = _gather_check(sliced(src, 8, 16), idx, n_src, C, dtype, C + 8)        # strided source, strided out=
    got = K.gather_rows(src, idx)
    assert got.dtype == dtype and got.is_contiguous() and torch.equal(got, want)


def test_gather_rows_above_the_grid_cap():
    n, C = GATHER_BIG
    g = torch.Generator().manual_seed(9)
    src = torch.randn(300, C, generator=g).to(BF16).to(DEV)
    idx = torch.randint(-1, 300, (n,), generator=g).to(torch.int32).to(DEV)
    idx[0], idx[-1] = 299, 0
    _gather_check(src, idx, 300, C, BF16, C)


# ---------------------------------------------------------------------------------------------- the wrappers refuse what the
# kernels would read or write out of bounds (nothing is launched: each call raises before it reaches the library)
def _z(*shape, dtype=BF16):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def test_wrappers_check_shapes_and_strides_before_launching():
    x, g = _z(4, 64), _z(64, dtype=F32)
    cos = _z(16, 32, dtype=F32)
    q = _z(6, 128)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    one = _z(1, dtype=F32)
    idx = torch.zeros(3, dtype=torch.int32, device=DEV)
    bad = [
        (lambda: K.rmsnorm_bwd(_z(64, 4).t(), g, x), "rmsnorm_bwd: x must have unit inner stride"),
        (lambda: K.rmsnorm_bwd(x, g, _z(64, 4).t()), "rmsnorm_bwd: dy must have unit inner stride"),
        (lambda: K.rmsnorm_bwd(x, g, _z(3, 64)), r"rmsnorm_bwd: dy must be \[4, 64\]"),
        (lambda: K.rmsnorm_bwd(x, g, x, dres=_z(4, 56)), r"rmsnorm_bwd: dres must be \[4, 64\]"),
        (lambda: K.rmsnorm_bwd(x, g[:56], x), "rmsnorm_bwd: gamma must hold 64 contiguous values"),
        (lambda: K.rmsnorm_bwd(x, g, x, dgamma=_z(128, dtype=F32)[::2]), "rmsnorm_bwd: dgamma must hold 64 contiguous values"),
        (lambda: K.rmsnorm_bwd(x, g, x, out=_z(4, 56)), r"rmsnorm_bwd: out must be \[4, 64\]"),
        (lambda: K.rmsnorm_bwd(_z(4, 8, 8), g, x), "rmsnorm_bwd: x must be 2-D"),
        (lambda: K.layernorm_bwd(_z(64, 4).t(), g, x), "layernorm_bwd: x must have unit inner stride"),
        (lambda: K.layernorm_bwd(x, g, _z(4, 72)), r"layernorm_bwd: dy must be \[4, 64\]"),
        (lambda: K.layernorm_bwd(x, g[:8], x), "layernorm_bwd: gamma must hold 64 contiguous values"),
        (lambda: K.layernorm_bwd(x, g, x, dbeta=_z(63, dtype=F32)), "layernorm_bwd: dbeta must hold 64 contiguous values"),
        (lambda: K.layernorm_bwd(x, g, x, dgamma=_z(65, dtype=F32)), "layernorm_bwd: dgamma must hold 64 contiguous values"),
        (lambda: K.rope_qkv_bwd(_z(128, 6).t(), q, q, cos, cos, 2, 64), "rope_qkv_bwd: dq must have unit inner stride"),
        (lambda: K.rope_qkv_bwd(q, _z(5, 128), q, cos, cos, 2, 64), r"rope_qkv_bwd: dk must be \[6, 128\]"),
        (lambda: K.rope_qkv_bwd(q, q, _z(6, 64), cos, cos, 2, 64), r"rope_qkv_bwd: dv must be \[6, 128\]"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos, cos, 2, 32), r"rope_qkv_bwd: dq must be \[\*, 64\]"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos[:5], cos, 2, 64), "rope_qkv_bwd: cos holds 5 positions, the call reads up to position 6"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos, cos[:7], 2, 64, pos0=5, period=3), "rope_qkv_bwd: sin holds 7 positions, the call reads up to position 8"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos, cos[:, :16], 2, 64), r"rope_qkv_bwd: sin must be \[\*, 32\]"),
        (lambda: K.rope_qkv_bwd(q, q, q, _z(16, 64, dtype=F32)[:, :32], cos, 2, 64), "rope_qkv_bwd: cos must be dense"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos, cos, 2, 64, period=4), "rope_qkv_bwd: 6 rows are no whole number of sequences of period 4"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos, cos, 2, 64, out=_z(6, 392)[:, :384]), "rope_qkv_bwd: out must be dense"),
        (lambda: K.rope_qkv_bwd(q, q, q, cos, cos, 2, 64, out=_z(5, 384)), r"rope_qkv_bwd: out must be \[6, 384\]"),
        (lambda: K.cross_entropy(_z(8, 4, dtype=F32).t(), lab, one), "cross_entropy: logits must have unit inner stride"),
        (lambda: K.cross_entropy(_z(4, 8, dtype=F32), lab, _z(2, dtype=F32)), "cross_entropy: loss_sum must hold 1 contiguous values"),
        (lambda: K.cross_entropy(_z(4, 8, dtype=F32), lab, one, one, _z(3, 8)), r"cross_entropy: dlogits must be \[4, \*\]"),
        (lambda: K.cross_entropy(_z(4, 8, dtype=F32), lab, one, one, _z(8, 4).t()), "cross_entropy: dlogits must have unit inner stride"),
        (lambda: K.cross_entropy(_z(4, 8, dtype=F32), lab, one, one, _z(4, 8), 16), "cross_entropy: n_pad 16 must lie between N = 8 and the width of dlogits, 8"),
        (lambda: K.cross_entropy(_z(4, 8, dtype=F32), lab, one, one, _z(4, 7)), "cross_entropy: n_pad 7 must lie between N = 8"),
        (lambda: K.cross_entropy(_z(4, 8, dtype=F32), lab, one, None, _z(4, 8)), "cross_entropy: dlogits needs grad_scale"),
        (lambda: K.transpose(_z(64, 4).t()), "transpose: x must have unit inner stride"),
        (lambda: K.transpose(x, 3), "transpose: r_pad 3 is below the 4 rows of x"),
        (lambda: K.transpose(x, 8, out=_z(64, 4)), r"transpose: out must be \[64, >= 8\]"),
        (lambda: K.transpose(x, out=_z(63, 4)), r"transpose: out must be \[64, \*\]"),
        (lambda: K.transpose(x, out=_z(4, 64).t()), "transpose: out must have unit inner stride"),
        (lambda: K.colsum(_z(64, 4).t()), "colsum: x must have unit inner stride"),
        (lambda: K.colsum(x, out=_z(63, dtype=F32)), "colsum: out must hold 64 contiguous values"),
        (lambda: K.gather_rows(_z(64, 4).t(), idx), "gather_rows: src must have unit inner stride"),
        (lambda: K.gather_rows(x, idx, out=_z(2, 64)), r"gather_rows: out must be \[3, 64\]"),
        (lambda: K.gather_rows(x, idx, out=_z(64, 3).t()), "gather_rows: out must have unit inner stride"),
    ]
    for call, message in bad:
        with pytest.raises(ValueError, match=message):
            call()
