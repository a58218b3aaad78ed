"""GPU: kernels.splice_embed_window (g4r_splice_embed_window_bf16 / _f16) by value.

The kernel is a gather, so every comparison is `torch.equal`.  The restatement is built from `splice_embed`'s own full
output [B, T, C] (every `<bbox>` with its feature row, row b's patches from img[img_of_row[b]]): slot j of row b is position
lo_b + j of that output, zeros behind the window.  Shapes are the smallest at which each mechanism can break: T = 9 (less
than one wave), 300 and 515 (the 256-wide scan chunk crossed once and twice, a `<bbox>` placed on either side of a chunk
boundary); C = 8 (one 16-byte piece per row) and 264 (33 pieces: not a multiple of the block); n_patch 0, 4 and 64; one row
and three rows that share two images."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpt4roi_amd import kernels as K

DEV = "cuda"
V, PATCH, BBOX, IMS, IME = 100, 90, 91, 92, 93
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
GUARD = 4096


def _rnd(*shape, seed, dtype):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _bbox_positions(T, NP, b):
    """Where row b's `<bbox>` tokens sit, all behind <im_end> (position 2 + NP); rows differ in place and in number."""
    first = NP + 3
    if T == 9:
        return [7, 8] if NP else [3, 5, 7][:3 - (b % 2)]
    spots = [first + b, 255 + b, 256 + 2 * b, T - 2 - b]                   # both sides of the first chunk boundary
    if T > 512:
        spots.append(511 + b)                                             # and of the second
    spots = sorted(spots)
    return spots[:len(spots) - (b % 2)]


def _case(B, T, C, NP, dtype):
    g = torch.Generator().manual_seed(1000 + 7 * T + NP + B)
    ids = torch.randint(3, 80, (B, T), generator=g)
    if NP:
        ids[:, 1] = IMS
        ids[:, 2:2 + NP] = PATCH
        ids[:, 2 + NP] = IME
    spots = [_bbox_positions(T, NP, b) for b in range(B)]
    for b, s in enumerate(spots):
        ids[b, s] = BBOX
    ids = ids.to(DEV)
    U = 2 if B > 1 else 1
    img_of_row = [0, 0, 1][:B]
    embed = _rnd(V, C, seed=83, dtype=dtype)
    img = _rnd(U, NP, C, seed=84, dtype=dtype) if NP else None
    counts = [len(s) for s in spots]
    spi = _rnd(sum(counts), C, seed=85, dtype=dtype)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    rows_img = img[img_of_row].contiguous() if NP else None               # what splice_embed wants: one image per row
    full, st_full = K.splice_embed(ids, embed, rows_img, spi, torch.tensor(off, dtype=torch.int32, device=DEV), NP, PATCH,
                                   BBOX, IMS, IME)
    assert (st_full == 0).all()
    return dict(B=B, T=T, C=C, NP=NP, ids=ids, spots=spots, embed=embed, img=img, img_of_row=img_of_row, spi=spi, off=off,
                full=full, dtype=dtype)


def _window(c, lo, hi, skip, W=None):
    """Run the kernel into a buffer with a guard band -> (out [B, W, C], status); the band must come back untouched."""
    B, C = c["B"], c["C"]
    W = max([1] + [z - a for a, z in zip(lo, hi)]) if W is None else W
    # the rows of spi the kernel may read: row b's features from ordinal skip[b] on
    keep, off = [], [0]
    for b in range(B):
        n = max(0, len(c["spots"][b]) - skip[b])
        keep += list(range(c["off"][b] + skip[b], c["off"][b] + skip[b] + n))
        off.append(off[-1] + n)
    spi = c["spi"][keep].contiguous() if keep else None
    buf = torch.full((B * W * C + GUARD,), 7.0, dtype=c["dtype"], device=DEV)
    out = buf[:B * W * C].view(B, W, C)
    got, st = K.splice_embed_window(c["ids"], c["embed"], c["img"], c["img_of_row"], spi,
                                    torch.tensor(off, dtype=torch.int32, device=DEV), skip, lo, hi, W, c["NP"], PATCH, BBOX,
                                    IMS, IME, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[B * W * C:] == 7.0).all()), "the guard band behind `out` was written"
    return out, st


def _expect(c, lo, hi, W):
    want = torch.zeros((c["B"], W, c["C"]), dtype=c["dtype"], device=DEV)
    for b, (a, z) in enumerate(zip(lo, hi)):
        want[b, :z - a] = c["full"][b, a:z]
    return want


def _before(c, pos):
    """per row: the number of `<bbox>` tokens before position pos[b]"""
    return [sum(1 for s in c["spots"][b] if s < pos[b]) for b in range(c["B"])]


SHAPES = [(9, 0), (9, 4), (300, 0), (300, 4), (300, 64), (515, 0), (515, 4), (515, 64)]


@DTYPES
@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("T,NP", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_windows_equal_the_full_splice_where_they_overlap(B, T, NP, C, dtype):
    c = _case(B, T, C, NP, dtype)
    everything = ([0] * B, [T] * B)
    # [0, T): the sibling kernel bit for bit, status included (W = T: the compact layout IS the full one)
    out, st = _window(c, *everything, [0] * B)
    assert torch.equal(out, c["full"]) and (st == 0).all()
    windows = {
        "last position": ([T - 1] * B, [T] * B),
        "behind the first <bbox>": ([s[0] + 1 for s in c["spots"]], [T] * B),
        "behind the last <bbox>": ([s[-1] + 1 for s in c["spots"]], [T] * B),
        "empty": ([5] * B, [5] * B),
        "ends on a <bbox>": ([0] * B, [s[-1] for s in c["spots"]]),
    }
    if NP:
        windows["from the middle of the patch run"] = ([2 + NP // 2] * B, [T] * B)
        windows["inside the patch run"] = ([3] * B, [2 + NP] * B)
    if B == 3:                                      # one launch, three different windows: all, one position, nothing
        windows["mixed"] = ([0, T - 1, 4], [T, T, 4])
    for name, (lo, hi) in windows.items():
        skip = _before(c, lo)                       # spi_skip = the boxes before the window: 0, 1, ... or all of them
        out, st = _window(c, lo, hi, skip)
        W = out.size(1)
        assert W == max([1] + [z - a for a, z in zip(lo, hi)])
        assert torch.equal(out, _expect(c, lo, hi, W)), name
        assert (st == 0).all(), (name, st.tolist())
        for b, (a, z) in enumerate(zip(lo, hi)):    # (part of the comparison above; spelled out: zeros behind a row's window)
            assert not out[b, z - a:].any(), name
    # spi_skip in {0, 1, all} at ONE window that holds no <bbox> of rank below the skip
    lo = [s[-1] for s in c["spots"]]                # from the last <bbox> on
    for skip in (_before(c, lo), [0] * B):
        out, st = _window(c, lo, [T] * B, skip)
        assert torch.equal(out, _expect(c, lo, [T] * B, out.size(1))) and (st == 0).all(), skip
    # a stride wider than every window: the surplus slots are zeros too
    out, st = _window(c, [T - 1] * B, [T] * B, _before(c, [T - 1] * B), W=6)
    assert torch.equal(out, _expect(c, [T - 1] * B, [T] * B, 6)) and (st == 0).all()


@DTYPES
def test_rows_take_their_patches_from_the_image_they_name(dtype):
    c = _case(3, 300, 264, 64, dtype)
    assert c["img_of_row"] == [0, 0, 1]
    out, _ = _window(c, [0] * 3, [300] * 3, [0] * 3)
    assert torch.equal(out[0, 2:66], c["img"][0]) and torch.equal(out[1, 2:66], c["img"][0])
    assert torch.equal(out[2, 2:66], c["img"][1]) and not torch.equal(c["img"][0], c["img"][1])
    c["img_of_row"] = [1, 0, 1]
    out, _ = _window(c, [10] * 3, [40] * 3, [0] * 3)
    assert torch.equal(out[0], c["img"][1, 8:38]) and torch.equal(out[1], c["img"][0, 8:38])


def _status_case(dtype=torch.bfloat16):
    return _case(3, 300, 8, 4, dtype)


def test_status_is_that_of_the_full_splice_also_for_faults_outside_the_window():
    c = _status_case()
    T, NP = c["T"], c["NP"]
    faults = {
        "one <bbox> too many": (1, 200, BBOX, 2),
        "missing <im_end>": (0, 2 + NP, 7, 8),
        "missing <im_start>": (2, 1, 7, 4),
        "patch run broken": (1, 3, 7, 16 | 1),
        "a patch token too many": (0, 150, PATCH, 16 | 1),
    }
    off = torch.tensor(c["off"], dtype=torch.int32, device=DEV)
    good = c["ids"]
    for name, (b, pos, tok, bits) in faults.items():
        bad = good.clone()
        bad[b, pos] = tok
        c["ids"] = bad
        _, want = K.splice_embed(bad, c["embed"], c["img"][c["img_of_row"]].contiguous(), c["spi"], off, NP, PATCH, BBOX,
                                 IMS, IME)
        assert want[b].item() & bits == bits, (name, want.tolist())
        for lo, hi in (([0] * 3, [T] * 3), ([T - 1] * 3, [T] * 3), ([100] * 3, [100] * 3)):
            _, st = _window(c, lo, hi, [0] * 3)                           # skip 0: the same arithmetic as the full splice
            assert torch.equal(st, want), (name, lo, st.tolist(), want.tolist())
    c["ids"] = good


def test_status_counts_the_skipped_boxes_and_flags_a_box_without_features():
    c = _status_case()
    T, B = c["T"], 3
    n = [len(s) for s in c["spots"]]
    assert n == [4, 3, 4]
    lo = [s[1] + 1 for s in c["spots"]]                                   # behind the second <bbox>
    _, st = _window(c, lo, [T] * B, [2, 2, 2])
    assert st.tolist() == [0, 0, 0]
    # bit 2: #<bbox> != spi_skip + #regions -- _window hands over max(0, n_b - skip) feature rows, so shift the claim
    keep, spi = c["spots"], c["spi"]
    c["spots"] = [keep[0], keep[1] + [T - 20], keep[2]]                   # row 1 claims a region more than it has tokens
    c["off"], c["spi"] = [0, 4, 8, 12], _rnd(12, c["C"], seed=9, dtype=c["dtype"])
    _, st = _window(c, lo, [T] * B, [2, 2, 2])
    assert st.tolist() == [0, 2, 0]
    c["spots"], c["off"], c["spi"] = keep, [0, 4, 7, 11], spi
    _, st = _window(c, [T - 1] * B, [T] * B, [4, 4, 4])                    # row 1 has 3 tokens: 4 skipped + 0 regions != 3
    assert st.tolist() == [0, 2, 0]
    # bit 32: the window holds a <bbox> whose rank lies below spi_skip; that slot takes the token's embedding row
    lo32 = [s[1] for s in c["spots"]]                                     # ON the second <bbox>, yet two are skipped
    out, st = _window(c, lo32, [T] * B, [2, 2, 2])
    assert st.tolist() == [32, 32, 32]
    want = _expect(c, lo32, [T] * B, out.size(1))
    want[:, 0] = c["embed"][BBOX]
    assert torch.equal(out, want)
    _, st = _window(c, [0, lo32[1] + 1, 0], [T] * B, [0, 2, 1])           # only row 2 starts before a skipped box
    assert st.tolist() == [0, 0, 32]


def test_wrapper_checks_the_window_tables_on_the_host():
    c = _status_case()
    T, B = c["T"], 3
    z = [0] * B
    for kw in (dict(lo=[-1, 0, 0], hi=[T] * B), dict(lo=[5, 5, 5], hi=[4, 5, 5]), dict(lo=z, hi=[T + 1, T, T]),
               dict(lo=z, hi=[T] * B, W=T - 1), dict(lo=z, hi=[T] * B, W=0), dict(lo=z, hi=[T] * B, img_of_row=[0, 2, 0]),
               dict(lo=z, hi=[T] * B, skip=[0, -1, 0]), dict(lo=z[:2], hi=[T] * B)):
        with pytest.raises(ValueError):
            K.splice_embed_window(c["ids"], c["embed"], c["img"], kw.get("img_of_row", c["img_of_row"]), None, None,
                                  kw.get("skip", z), kw["lo"], kw["hi"], kw.get("W", T), c["NP"], PATCH, BBOX, IMS, IME)
