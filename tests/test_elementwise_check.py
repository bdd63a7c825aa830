"""Host self-test of tests/elementwise_check.py: the element-wise checks reject the subtle corruptions a whole-tensor
rel-L2 lets through, at the shapes and bounds (TAU) of tests/test_gpu_elementwise.py.  No GPU: CPU fp32 stands in for a
correct kernel, and CPU emulations of the bf16 operand splits stand in for broken ones.

Splitting into planes: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); "k planes" keeps only the cross terms
P_i(A) P_j(W) with i + j < k (the split engine runs k = 3).  Each corruption replaces part of a clean fp32 result:

    corruption (linear M = 66253, N = K = 256, as test_linear_row_stationary)    rel-L2    worst |err| / scale
    clean CPU fp32 A W^T                                                         2.9e-7    3.6e-7
    one 16 x 16 block on one bf16 plane                                          1.0e-5    6.5e-4
    one 16 x 16 block left at zero (a skipped tile)                              4.1e-3    0.26
    four rows x (1 + 1e-4)                                                       8.2e-7    3.3e-5
    the 77-row tail (the rows rowpanel leaves to the per-tile kernels), 2 planes 3.3e-7    2.03e-6
    rows 12-15 / 28-31 of every 128-row block, 2 planes                          1.1e-6    2.7e-6
    conv 1 x 64 x 64, C = 32: border ring x (1 + 1e-5)                           2.1e-6    4.3e-6
    (clean CPU fp32 conv: 1.2e-7 / 1.0e-7)

test_every_bound_rejects_its_corruptions maps every bound of TAU / ROW_TOL (calibrated on the MI355X, see
elementwise_check.py) to the corruptions above it rejects.  Recorded limits, not dropped cases:
  * the two-plane cases sit just above the fp32 forward bound 1.6e-6 (tail 2.03e-6, lane group 2.7e-6; the clean
    MI355X worst is 5.2e-7): they are rejected by the f32 / split "fwd" and "wgrad" bounds, not by the "slice" bounds
    (1e-5 .. 2e-5: the slice kernels recompute softmax weights, whose exp error alone reaches 9e-6 on the exact engine);
  * bf16 storage ("bf16s") computes on one bf16 plane by design and stores bf16: its "fwd" bound (2^-8 |ref| + 5e-3 scale)
    rejects a skipped tile and an unwritten element, not a one-plane block or a 1e-4 row scaling.
"""
import numpy as np
import pytest
import torch

from elementwise_check import TAU, check_products, check_rows, poisoned

M, N, K = 65536 + 128 * 5 + 77, 256, 256
TAU_FWD = max(TAU[("f32", "fwd")], TAU[("split", "fwd")])


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _planes(x):
    hi = _bf(x)
    mid = _bf(x - hi)
    lo = _bf(x - hi - mid)
    return hi, mid, lo


def _split_gemm(a, w, k):
    """a . w^T from the bf16 planes of both operands, cross terms with i + j < k, summed in fp64 (the MFMA's exact products
    and fp32-or-better accumulation)."""
    pa, pw = _planes(a), _planes(w)
    out = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64)
    for i in range(3):
        for j in range(3):
            if i + j < k:
                out += pa[i].double() @ pw[j].double().t()
    return out.float()


@pytest.fixture(scope="module")
def gemm():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    ref = a.double() @ w.double().t()
    scale = a.double().abs() @ w.double().abs().t()
    return a, w, a @ w.t(), ref, scale


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def _fails(got, ref, scale, label, **kw):
    with pytest.raises(AssertionError) as e:
        check_products(got, ref, scale, TAU_FWD, label=label, **kw)
    return str(e.value)


def test_clean_fp32_passes(gemm):
    a, w, clean, ref, scale = gemm
    worst = check_products(clean, ref, scale, TAU_FWD, label="clean")
    assert worst < TAU_FWD / 2, worst          # room between the CPU fp32 floor and the bound
    assert check_rows(clean, ref, 1e-5, label="clean rows") < 1e-5


def test_one_plane_block_fails(gemm):
    a, w, clean, ref, scale = gemm
    got = clean.clone()
    r0, c0 = 40000, 96
    got[r0:r0 + 16, c0:c0 + 16] = _split_gemm(a[r0:r0 + 16], w[c0:c0 + 16], 1)
    assert _rel(got, ref) < 2e-5               # passes the whole-tensor gradient bound
    msg = _fails(got, ref, scale, "one-plane block")
    assert "row 4" in msg and "16 distinct rows [40000 .. 40015]" in msg and "col " in msg


def test_scaled_rows_fail(gemm):
    a, w, clean, ref, scale = gemm
    got = clean.clone()
    rows = [7, 1000, 33333, 66000]
    got[rows] *= 1 + 1e-4
    assert _rel(got, ref) < 3e-6               # passes every whole-tensor bound of the suite
    msg = _fails(got, ref, scale, "scaled rows")
    assert "4 distinct rows [7 .. 66000]" in msg


def test_two_plane_tail_fails(gemm):
    a, w, clean, ref, scale = gemm
    got = clean.clone()
    t0 = M - M % 128
    got[t0:] = _split_gemm(a[t0:], w, 2)
    assert M - t0 == 77 and _rel(got, ref) < 3e-6
    worst = check_products(got, ref, scale, 1.0, label="tail")
    assert worst > TAU_FWD, f"2-plane tail: worst {worst:.3g} does not exceed tau {TAU_FWD:.3g}"
    msg = _fails(got, ref, scale, "2-plane tail")
    lo = int(msg.split("distinct rows [")[1].split(" ..")[0])
    assert lo >= t0, msg                       # every violating row is a tail row


def test_two_plane_lane_group_fails(gemm):
    a, w, clean, ref, scale = gemm
    got = clean.clone()
    r = torch.arange(M)
    rows = r[((r % 128 >= 12) & (r % 128 < 16)) | ((r % 128 >= 28) & (r % 128 < 32))]
    got[rows] = _split_gemm(a[rows], w, 2)
    assert _rel(got, ref) < 3e-6
    worst = check_products(got, ref, scale, 1.0, label="lanes")
    assert worst > TAU_FWD, f"2-plane lane group: worst {worst:.3g} does not exceed tau {TAU_FWD:.3g}"
    msg = _fails(got, ref, scale, "2-plane lane group")
    residues = msg.split("rows mod 32: ")[1].split("]")[0] + "]"
    assert set(eval(residues)) <= {12, 13, 14, 15, 28, 29, 30, 31}, msg


def _conv(x, w, H, W):
    B, Np, C = x.shape
    xp = torch.nn.functional.pad(x.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    out = 0
    for ky in range(3):
        for kx in range(3):
            out = out + xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    return out.reshape(B, Np, -1)


def test_conv_border_ring_fails():
    from oracle import transolver_oracle as orc
    B, H, W, C = 1, 64, 64, 32
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H * W, C, generator=g)
    w = torch.randn(2 * C, C, 3, 3, generator=g) * (9 * C) ** -0.5
    ref = orc.conv3x3(x.double(), w.double(), None, H, W)
    scale = orc.conv3x3(x.double().abs(), w.double().abs(), None, H, W)
    clean = _conv(x, w, H, W)
    assert check_products(clean, ref, scale, TAU_FWD, hw=(H, W), label="clean conv") < TAU_FWD / 2
    got = clean.clone().reshape(B, H, W, 2 * C)
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    got[:, ring] *= 1 + 1e-5
    got = got.reshape(B, H * W, 2 * C)
    assert _rel(got, ref) < 3e-6
    msg = _fails(got, ref, scale, "conv border", hw=(H, W))
    assert "on the border ring" in msg and " 0 interior" in msg, msg


def test_stale_element_fails_poisoned():
    def op(x):
        y = torch.empty_like(x)
        y.view(-1)[:] = x.view(-1) * 2
        return y

    x = torch.randn(300, 64)
    assert torch.equal(poisoned(op, x), x * 2)

    def stale(x):          # writes every element but one: that one keeps what the buffer held
        y = torch.empty_like(x)
        flat = y.view(-1)
        flat[:1234] = x.view(-1)[:1234] * 2
        flat[1235:] = x.view(-1)[1235:] * 2
        return y

    with pytest.raises(AssertionError, match=r"unwritten .* index \(19, 18\)"):
        poisoned(stale, x)

    calls = []

    def nondeterministic(x):
        calls.append(1)
        y = torch.empty_like(x)
        y.copy_(x)
        if len(calls) == 2:
            y[5, 5] += 1e-3
        return y

    with pytest.raises(AssertionError, match=r"differs between two runs in 1 elements"):
        poisoned(nondeterministic, x)

    def elsewhere(x):      # an output that does not come from a fresh buffer cannot be checked: refused, not passed
        return x

    with pytest.raises(AssertionError, match="vacuous"):
        poisoned(elsewhere, x)


def test_check_rows_names_the_row():
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(1000, 64, generator=g, dtype=torch.float64)
    got = ref.clone()
    got[300] *= 1 + 1e-4
    assert check_rows(ref.float(), ref, 1e-6, label="clean") < 1e-6
    with pytest.raises(AssertionError, match=r"1 of 1000 rows .* row 300 \(mod 16 = 12, mod 32 = 12, mod 128 = 44\)"):
        check_rows(got, ref, 1e-6, label="row")


# bound -> corruptions (names of _CORRUPTIONS) it must reject
_REJECTS = {
    ("f32", "fwd"): "block zero_block rows tail lanes", ("split", "fwd"): "block zero_block rows tail lanes",
    ("f32", "wgrad"): "block zero_block rows tail lanes", ("split", "wgrad"): "block zero_block rows tail lanes",
    ("bf16s", "wgrad"): "block zero_block rows tail lanes",
    ("f32", "slice"): "block zero_block rows", ("split", "slice"): "block zero_block rows",
    ("bf16s", "slice"): "block zero_block rows",
    ("bf16s", "fwd"): "zero_block",
}


def _corrupt(name, a, w, clean):
    got = clean.clone()
    r = torch.arange(M)
    if name == "block":
        got[40000:40016, 96:112] = _split_gemm(a[40000:40016], w[96:112], 1)
    elif name == "zero_block":
        got[40000:40016, 96:112] = 0.0
    elif name == "rows":
        got[[7, 1000, 33333, 66000]] *= 1 + 1e-4
    elif name == "tail":
        got[M - M % 128:] = _split_gemm(a[M - M % 128:], w, 2)
    elif name == "lanes":
        rows = r[((r % 128 >= 12) & (r % 128 < 16)) | ((r % 128 >= 28) & (r % 128 < 32))]
        got[rows] = _split_gemm(a[rows], w, 2)
    return got


def test_every_bound_rejects_its_corruptions(gemm):
    from elementwise_check import BF16_STORAGE_REL, ROW_TOL
    a, w, clean, ref, scale = gemm
    assert set(_REJECTS) == set(TAU)
    names = set(" ".join(_REJECTS.values()).split())
    for name in sorted(names):
        got = _corrupt(name, a, w, clean)
        worst = check_products(got, ref, scale, 1e30, label=name)
        for key, want in _REJECTS.items():
            if name not in want.split():
                continue
            rel_ref = BF16_STORAGE_REL if key[0] == "bf16s" and key[1] == "fwd" else 0.0
            with pytest.raises(AssertionError):
                check_products(got, ref, scale, TAU[key], rel_ref=rel_ref, label=f"{name} at {key}")
            assert rel_ref or worst > TAU[key], (name, key, worst)
    # per-row bounds: a row scaled by (1 + 1e-4) fails the fp32-accurate engines' row bound; a zeroed row fails all three
    got = clean.clone()
    got[33333] *= 1 + 1e-4
    for eng in ("f32", "split"):
        with pytest.raises(AssertionError, match="row 33333"):
            check_rows(got, ref, ROW_TOL[eng], label=eng)
    got[33333] = 0.0
    for eng in ROW_TOL:
        with pytest.raises(AssertionError, match="row 33333"):
            check_rows(got, ref, ROW_TOL[eng], label=eng)


# ---------------------------------------------------------------------------------------------- bf16 plane images
# to_planes / unplane / check_canonical_planes (the operand-planes route, tests/test_gpu_planes_elementwise.py).
def _wide(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, C, generator=g) * torch.exp(3 * torch.randn(rows, C, generator=g))


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("rows,C", [(37, 160), (5, 32), (64, 256)])
def test_planes_round_trip(rows, C, nt):
    from elementwise_check import check_canonical_planes, to_planes, unplane
    x = _wide(rows, C, rows + C)
    x[0, :4] = torch.tensor([0.0, -0.0, 1.0, -2.0 ** -100])
    img = to_planes(x, nt)
    assert img.dtype == torch.uint8 and img.numel() == rows * C * nt * 2
    planes, total = unplane(img, rows, C, nt)
    assert planes.shape == (nt, rows, C) and planes.dtype == torch.bfloat16
    if nt == 3:      # the split is exact, and every plane is at most half a bf16 ulp of the one above it
        assert torch.equal(total, x.double())
        p = planes.double().abs()
        assert bool((p[1] <= 2.0 ** -8 * p[0]).all()) and bool((p[2] <= 2.0 ** -8 * p[1]).all())
    else:
        assert torch.equal(total, x.bfloat16().double())
    assert torch.equal(check_canonical_planes(img, rows, C, nt, label="clean"), total)
    x[0, 1] = 0.0                        # the plane sum of a negative zero is +0: the check takes the sign from p0
    assert torch.equal(to_planes(unplane(to_planes(x, nt), rows, C, nt)[1].float(), nt), to_planes(x, nt))


@pytest.mark.parametrize("nt", [1, 3])
def test_planes_byte_offsets(nt):
    """element (row, c, plane q) at byte row (C/32) nt 64 + ((c >> 5) nt + q) 64 + (c & 31) 2: the kernels' formula"""
    from elementwise_check import to_planes
    rows, C = 11, 160
    x = _wide(rows, C, 3)
    img = to_planes(x, nt).view(torch.int16)           # 2-byte units
    r = x.clone()
    for q in range(nt):
        p = r.bfloat16()
        r = r - p.float()
        row, c = torch.meshgrid(torch.arange(rows), torch.arange(C), indexing="ij")
        off = row * (C // 32) * nt * 64 + ((c >> 5) * nt + q) * 64 + (c & 31) * 2
        assert torch.equal(img[off // 2], p.view(torch.int16)), q


def _canonical_fails(img, rows, C, nt, label):
    from elementwise_check import check_canonical_planes
    with pytest.raises(AssertionError) as e:
        check_canonical_planes(img, rows, C, nt, label=label)
    return str(e.value)


def test_canonical_planes_rejects_swapped_stale_and_misplaced():
    from elementwise_check import SENTINEL_BYTES, to_planes
    rows, C, nt = 40, 160, 3
    x = _wide(rows, C, 9)
    img = to_planes(x, nt)
    v = lambda t: t.view(rows, C // 32, nt, 64)        # [row][chunk][plane][64 bytes]
    # mid and lo swapped in one chunk of one row: same plane sum, so a value comparison cannot see it
    sw = img.clone()
    v(sw)[17, 3, 1], v(sw)[17, 3, 2] = v(img)[17, 3, 2], v(img)[17, 3, 1]
    msg = _canonical_fails(sw, rows, C, nt, "swapped")
    assert "row 17 (" in msg and "chunk 3 of 5" in msg and "planes [1, 2]" in msg and "1 distinct rows [17 .. 17]" in msg, msg
    lo, hi = (int(s) for s in msg.split("channels [")[1].split("]")[0].split(" .. "))
    assert 96 <= lo <= hi < 128, msg
    # ... everywhere
    sw = img.clone()
    v(sw)[:, :, 1], v(sw)[:, :, 2] = v(img)[:, :, 2], v(img)[:, :, 1]
    assert f"{rows} distinct rows" in _canonical_fails(sw, rows, C, nt, "all swapped")
    # mid written into the hi slot and hi into the mid slot
    sw = img.clone()
    v(sw)[5, 0, 0], v(sw)[5, 0, 1] = v(img)[5, 0, 1], v(img)[5, 0, 0]
    assert "row 5 (" in _canonical_fails(sw, rows, C, nt, "hi / mid")
    for byte in SENTINEL_BYTES:      # what `poisoned` leaves in an element no kernel wrote
        # one stale row
        st = img.clone()
        v(st)[23] = byte
        msg = _canonical_fails(st, rows, C, nt, "stale row")
        assert "row 23 (" in msg and "col 0 (" in msg and "channels [0 .. 159]" in msg and "1 distinct rows" in msg, msg
        # one stale plane of one chunk
        st = img.clone()
        v(st)[2, 4, 2] = byte
        msg = _canonical_fails(st, rows, C, nt, "stale plane")
        assert "row 2 (" in msg and "chunk 4 of 5" in msg, msg
        # a head's chunk written at the neighbouring head's offset: its own place keeps the sentinel
        mis = img.clone()
        v(mis)[31, 2] = v(img)[31, 1]
        v(mis)[31, 1] = byte
        msg = _canonical_fails(mis, rows, C, nt, "misplaced chunk")
        assert "row 31 (" in msg and "col 32 (" in msg and "chunk 1 of 5" in msg, msg
        # a quarter chunk (D = 8: four heads share a chunk) at the neighbouring head's offset, in every plane
        mis = img.clone()
        v(mis)[8, 0, :, 16:32] = v(img)[8, 0, :, 0:16]
        v(mis)[8, 0, :, 0:16] = byte
        msg = _canonical_fails(mis, rows, C, nt, "misplaced head")
        assert "row 8 (" in msg and "channels [0 .. 7]" in msg, msg
    # one plane: any finite bf16 is canonical, an unwritten (NaN-sentinel) one is not; the 0x71 sentinel is left to
    # `poisoned`, whose two runs differ in such an element
    img1 = to_planes(x, 1)
    st = img1.clone()
    st.view(rows, C // 32, 1, 64)[23] = SENTINEL_BYTES[0]
    assert "row 23 (" in _canonical_fails(st, rows, C, 1, "stale row, one plane")

    def stale_op(x):
        out = torch.empty(rows * C * 2, dtype=torch.uint8)
        out.copy_(to_planes(x, 1))
        out.view(rows, C * 2)[23] = torch.empty(C * 2, dtype=torch.uint8)      # never written
        return out.view(torch.bfloat16)

    with pytest.raises(AssertionError, match="unwritten|differs between two runs"):
        poisoned(stale_op, x)


def test_swapped_planes_fail_the_forward_bound():
    """A GEMM that reads an image with mid and lo swapped keeps hi w2 + lo w1 + ... and loses mid w1: at most 2^-16 per
    product.  Where the residuals of both operands have one sign (here: every value just below a bf16 tie) the lost terms
    add up and TAU[("split", "fwd")] fires.  With residuals of random sign they average out, to about 4e-6 / sqrt(K) of the
    scale: 5e-7 at a conv's K = 9 * 128 below, under the bound.  (On the MI355X the conv backward of chain case B, fed such
    an image from a scratch build, reached 1.9e-6 on the data gradient and 2.4e-6 on dwx against 1.6e-6 / 1e-6: it fires, but
    by too little to rely on.)  That is why the image itself is held to check_canonical_planes, which is exact."""
    from elementwise_check import to_planes, unplane
    rows, N, K = 64, 96, 9 * 32
    g = torch.Generator().manual_seed(4)

    def below_tie(*shape):      # 2^e (1 + k / 128 + f / 256), k < 16, f in [0.45, 0.5): mid = +f 2^(e - 8), > 1.6e-3 |x|
        e = torch.randint(-2, 2, shape, generator=g).float()
        k = torch.randint(0, 16, shape, generator=g).float()
        f = 0.45 + 0.05 * torch.rand(shape, generator=g)
        return (2.0 ** e * (1 + k / 128 + f / 256)).float()

    a, w = below_tie(rows, K), below_tie(N, K) / 16
    ref, scale = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    pw = _planes(w)

    def gemm_from(img):
        pa, _ = unplane(img, rows, K, 3)
        out = torch.zeros(rows, N, dtype=torch.float64)
        for i in range(3):
            for j in range(3):
                if i + j <= 2:
                    out += pa[i].double() @ pw[j].double().t()
        return out.float()

    img = to_planes(a, 3)
    tau = TAU[("split", "fwd")]
    assert check_products(gemm_from(img), ref, scale, tau, label="clean image") < tau / 2
    sw = img.clone()
    v, v0 = sw.view(rows, K // 32, 3, 64), img.view(rows, K // 32, 3, 64)
    v[:, :, 1], v[:, :, 2] = v0[:, :, 2], v0[:, :, 1]
    assert torch.equal(unplane(sw, rows, K, 3)[1], unplane(img, rows, K, 3)[1])      # same plane sums
    worst = check_products(gemm_from(sw), ref, scale, 1.0, label="swapped image")
    print(f"swapped image, residuals of one sign: worst |err| / scale {worst:.3g}")
    with pytest.raises(AssertionError, match="swapped image"):
        check_products(gemm_from(sw), ref, scale, tau, label="swapped image")
    # residuals of random sign at a conv's depth (K = 9 * 128): the same swap stays below the bound, and the image check
    # is what rejects it
    K2 = 9 * 128
    a2 = torch.randn(rows, K2, generator=g)
    w2 = torch.randn(N, K2, generator=g) * K2 ** -0.5
    ref2, scale2 = a2.double() @ w2.double().t(), a2.double().abs() @ w2.double().abs().t()
    sw2 = to_planes(a2, 3)
    v = sw2.view(rows, K2 // 32, 3, 64)
    v[:, :, 1], v[:, :, 2] = v[:, :, 2].clone(), v[:, :, 1].clone()
    pa, pw2 = unplane(sw2, rows, K2, 3)[0], _planes(w2)
    out = sum(pa[i].double() @ pw2[j].double().t() for i in range(3) for j in range(3) if i + j <= 2).float()
    worst = check_products(out, ref2, scale2, 1.0, label="random signs")
    print(f"swapped image, residuals of random sign, K = {K2}: worst |err| / scale {worst:.3g}")
    assert worst < tau
    _canonical_fails(sw2, rows, K2, 3, "swapped image, random signs")
