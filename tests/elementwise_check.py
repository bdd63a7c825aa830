"""Element-wise checks of stage kernels against an fp64 reference (helper module of the suite, not a conftest).

A whole-tensor rel-L2 averages a wrong tile, a wrong lane group or a wrong border ring away.  These checks bound every
element instead:

* `check_products(got, ref, scale, tau)`: |got - ref| <= tau * scale (+ rel_ref * |ref| + abs_floor) for every element,
  where `scale` is the same operation evaluated in fp64 on absolute values (|A| |W|^T for a linear, the conv of |x| with
  |w|, sum_n w_nm |x_n| for the slice scatter, ...): the bound an fp32-accurate sum of products meets whatever the
  cancellation in that element.
* `check_rows(got, ref, tol)`: the largest rel-L2 over rows, for stages that are not sums of products (LayerNorm,
  softmax-normalised outputs, token attention, the slice backward's point gradients).
* `poisoned(fn, *args)`: runs an op twice with every `torch.empty` / `torch.empty_like` buffer it allocates pre-filled
  with a sentinel (all-ones bytes = NaN in fp32 and bf16, then 0x71 bytes = 1.2e30), asserts that every output tensor
  lives in such a buffer, that both results are finite and that they are bit-identical: an element a kernel never
  writes, or writes differently from run to run, fails.
* `to_planes` / `unplane` / `check_canonical_planes`: the bf16 plane images of the operand-planes route
  (tests/test_gpu_planes_elementwise.py), built and taken apart in plain torch, and the exact condition that an image
  is the canonical hi / mid / lo split of the value it holds.

The failure messages name the worst element with its row modulo 16 / 32 / 128, its column modulo 64 / 128, the count of
violating elements, the residues mod 32 of the violating rows and, for convs (`hw=(H, W)`), the pixel and whether it
is on the border ring: a tile, lane-group or border pattern is readable from the message alone.

TAU: the per-element bounds of the GPU suite (tests/test_gpu_elementwise.py), per engine and per family ("fwd": the
contraction is a layer width, "wgrad": the contraction runs over the rows of a batch).  Calibration on the MI355X and
the corruptions these values reject: see the docstrings of test_gpu_elementwise.py and test_elementwise_check.py.
"""
from __future__ import annotations

import contextlib

import torch

TAU = {      # MI355X worst |got - ref| / scale over tests/test_gpu_elementwise.py in the comment; bound <= 4x that
    ("f32", "fwd"): 1.6e-6,     # 5.2e-7  linear M=32895 N=1024 K=128 pre-activation (exact fp32 kernel)
    ("split", "fwd"): 1.6e-6,   # 5.2e-7  the same case on the row-stationary kernel and with it switched off
    ("bf16s", "fwd"): 5e-3,     # 1.3e-3  linear M=32968 N=192 K=96 data gradient (one bf16 term: weights rounded)
    ("f32", "wgrad"): 1e-6,     # 2.6e-7  linear M=200 N=64 K=64 weight gradient
    ("split", "wgrad"): 1e-6,   # 2.6e-7  the same case
    ("bf16s", "wgrad"): 3e-7,   # 7.9e-8  conv 1x12x20 C=64 dwx (bf16 values, exact products, fp32 sums)
    ("f32", "slice"): 2e-5,     # 9.1e-6  slice B=2 N=4113 heads=8 D=32 M=64 dfx_mid (softmax weights recomputed)
    ("split", "slice"): 1e-5,   # 4.6e-6  slice B=1 N=4100 heads=8 D=16 M=128 dfx_mid
    ("bf16s", "slice"): 1.2e-5,  # 5.7e-6  slice B=1 N=4100 heads=8 D=16 M=128 scatter S
}
ROW_TOL = {"f32": 1.9e-5,       # 4.9e-6  slice B=2 N=4113 heads=8 D=32 M=64 dn (token attention backward)
           "split": 9e-6,       # 2.3e-6  slice B=1 N=4100 heads=8 D=16 M=128 dn
           "bf16s": 9e-3}       # 2.4e-3  LayerNorm rows=300 C=64 forward (bf16 output)
BF16_STORAGE_REL = 2.0 ** -8          # bf16-stored outputs: rounding of the stored value (2^-9) plus the kernel's own
ROW_MODS = (16, 32, 128)
COL_MODS = (64, 128)


def _d(t):
    return torch.as_tensor(t).detach().to(torch.float64)


def _unravel(flat, shape):
    idx = []
    for s in reversed(shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))


def _where_row(row, hw):
    s = f"row {row} (" + ", ".join(f"mod {m} = {row % m}" for m in ROW_MODS) + ")"
    if hw is not None:
        H, W = hw
        b, n = divmod(row, H * W)
        y, x = divmod(n, W)
        ring = y in (0, H - 1) or x in (0, W - 1)
        s += f", image {b} pixel (y={y}, x={x}) {'on the border ring' if ring else 'interior'}"
    return s


def _where(row, col, hw):
    return _where_row(row, hw) + f", col {col} (" + ", ".join(f"mod {m} = {col % m}" for m in COL_MODS) + ")"


def _row_summary(rows, hw):
    """Residues of the violating rows: which lane groups / tiles / border pixels are involved."""
    rows = torch.unique(rows)
    out = [f"{rows.numel()} distinct rows [{int(rows.min())} .. {int(rows.max())}]",
           f"rows mod 32: {sorted(set((rows % 32).tolist()))}"]
    if hw is not None:
        H, W = hw
        n = rows % (H * W)
        y, x = n // W, n % W
        ring = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
        out.append(f"{int(ring.sum())} of them on the border ring, {int((~ring).sum())} interior")
    return "; ".join(out)


def check_products(got, ref, scale, tau, *, abs_floor=0.0, rel_ref=0.0, hw=None, label=""):
    """Assert |got - ref| <= tau * scale + rel_ref * |ref| + abs_floor element by element; returns the worst
    (|got - ref| - rel_ref |ref| - abs_floor) / scale, the number the calibration records.  Tensors are viewed as
    [rows, last dim]; hw = (H, W): rows are pixels of [B, H*W] images (conv outputs and data gradients)."""
    g = _d(got)
    r, s = _d(ref).to(g.device), _d(scale).to(g.device)      # computed where `got` lives
    assert g.shape == r.shape == s.shape, (label, tuple(g.shape), tuple(r.shape), tuple(s.shape))
    shape = tuple(g.shape)
    err = (g - r).abs()
    excess = err - rel_ref * r.abs() - abs_floor
    ratio = excess / s.clamp_min(1e-300)
    ratio = torch.where(torch.isnan(g), torch.full_like(ratio, float("inf")), ratio)    # NaN compares false: count it
    bad = ratio > tau
    worst = float(ratio.max()) if ratio.numel() else 0.0
    nbad = int(bad.sum())
    if nbad:
        flat = int(ratio.reshape(-1).argmax())
        cols = shape[-1] if len(shape) else 1
        row, col = divmod(flat, cols)
        badrows = bad.reshape(-1, cols).any(1).nonzero().flatten()
        raise AssertionError(
            f"{label}: {nbad} of {g.numel()} elements exceed |got - ref| <= {tau:.3g} * scale"
            f"{f' + {rel_ref:.3g} |ref|' if rel_ref else ''}{f' + {abs_floor:.3g}' if abs_floor else ''}; "
            f"worst at index {_unravel(flat, shape)}: {_where(row, col, hw)}: got {float(g.reshape(-1)[flat]):.9g}, "
            f"ref {float(r.reshape(-1)[flat]):.9g}, scale {float(s.reshape(-1)[flat]):.4g}, "
            f"|err| / scale = {worst:.3g}; violating {_row_summary(badrows, hw)}")
    return worst


def check_rows(got, ref, tol, *, hw=None, label=""):
    """Assert that every row ([rows, last dim] view) has rel-L2 <= tol against ref; returns the worst row's rel-L2."""
    g = _d(got)
    r = _d(ref).to(g.device)
    assert g.shape == r.shape, (label, tuple(g.shape), tuple(r.shape))
    cols = g.shape[-1]
    g, r = g.reshape(-1, cols), r.reshape(-1, cols)
    rel = (g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-300)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
    worst = float(rel.max()) if rel.numel() else 0.0
    bad = rel > tol
    if bool(bad.any()):
        row = int(rel.argmax())
        where = _where_row(row, hw)
        raise AssertionError(
            f"{label}: {int(bad.sum())} of {rel.numel()} rows exceed rel-L2 {tol:.3g}; worst {where}: rel-L2 "
            f"{worst:.3g}; violating {_row_summary(bad.nonzero().flatten(), hw)}")
    return worst


# ---------------------------------------------------------------------------------------------- bf16 plane images
# The operand-planes route hands a [rows, C] fp32 tensor on as a byte image [row][C / 32][nt][32] bf16 (nt = 3: the exact
# split p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), round-to-nearest-even; nt = 1: bf16(x)): element
# (row, c, plane q) sits at byte row * (C / 32) * nt * 64 + ((c >> 5) * nt + q) * 64 + (c & 31) * 2.
def to_planes(x, nt):
    """fp32 [rows, C] -> flat uint8 plane image (plain torch, CPU or GPU)."""
    x = torch.as_tensor(x).detach().to(torch.float32)
    rows, C = x.shape
    assert C % 32 == 0 and nt in (1, 3), (C, nt)
    planes, r = [], x
    for q in range(nt):
        p = r.bfloat16()
        planes.append(p.view(rows, C // 32, 32))
        if q + 1 < nt:
            r = r - p.float()            # exact in fp32
    return torch.stack(planes, 2).contiguous().view(torch.uint8).reshape(-1)


def unplane(img, rows, C, nt):
    """(planes [nt, rows, C] bf16, their fp64 sum [rows, C]) of a plane image."""
    assert img.numel() * img.element_size() == rows * C * nt * 2, (img.numel(), rows, C, nt)
    p = img.reshape(-1).view(torch.bfloat16).view(rows, C // 32, nt, 32).permute(2, 0, 1, 3).reshape(nt, rows, C)
    return p, p.double().sum(0)


def check_canonical_planes(img, rows, C, nt, *, label=""):
    """Assert that the image is the canonical split of the value it holds: every plane finite and, for nt = 3,
    to_planes(p0 + p1 + p2) == img bit for bit (the sum of a canonical split is an fp32 number, and the split of that
    number is unique).  Exact, no tolerance: swapped planes, a plane in the wrong slot and a stale plane fail, and the
    message names rows, channels and planes.  nt = 1: any finite bf16 is its own split, so finiteness only.  Returns
    the fp64 sum [rows, C]."""
    planes, total = unplane(img, rows, C, nt)
    bad = ~torch.isfinite(planes.float())                                        # [nt, rows, C]
    what = "not finite (never written?)"
    if not bool(bad.any()) and nt > 1:
        x = total.float()
        x = torch.where(x == 0, planes[0].float(), x)                           # keeps the sign of a zero
        want, _ = unplane(to_planes(x, nt), rows, C, nt)
        bad = planes.view(torch.int16) != want.view(torch.int16)
        what = "not the canonical split of their own sum"
    if bool(bad.any()):
        elem = bad.any(0)                                                        # [rows, C]
        badrows = elem.any(1).nonzero().flatten()
        row = int(badrows[0])
        cols = elem[row].nonzero().flatten()
        col = int(cols[0])
        held = ", ".join(f"p{q} = {float(planes[q, row, col]):.9g}" for q in range(nt))
        raise AssertionError(
            f"{label}: {int(elem.sum())} of {rows * C} elements of the {nt}-plane image are {what} (planes "
            f"{sorted(set(bad.any(2).any(1).nonzero().flatten().tolist()))}); first at {_where(row, col, None)}, 32-channel "
            f"chunk {col >> 5} of {C // 32}: {held}; channels [{int(cols.min())} .. {int(cols.max())}] of that row; violating "
            f"{_row_summary(badrows, None)}")
    return total


# ---------------------------------------------------------------------------------------------- poisoned outputs
SENTINEL_BYTES = (0xFF, 0x71)         # all-ones: NaN in fp32 and bf16; 0x71717171: 1.2e30 (fp32), 0x7171: 1.2e30 (bf16)


@contextlib.contextmanager
def _sentinel_allocations(byte):
    """Inside: every torch.empty / torch.empty_like buffer is filled with `byte` before the caller sees it.  Yields the
    list of (data_ptr, nbytes) of those buffers."""
    made = []
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        st = t.untyped_storage()
        if st.nbytes():
            st.fill_(byte)
        made.append((st.data_ptr(), st.nbytes()))
        return t

    def empty(*a, **k):
        return fill(real_empty(*a, **k))

    def empty_like(*a, **k):
        return fill(real_like(*a, **k))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield made
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def _tensors(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    if isinstance(out, dict):
        return [t for o in out.values() for t in _tensors(o)]
    return []


def poisoned(fn, *args, **kwargs):
    """fn(*args, **kwargs) with its fresh buffers pre-filled with NaN, then with 1.2e30: every output tensor must lie in
    a sentinel-filled buffer, be finite and be bit-identical between the two runs.  Returns the first run's result."""
    results = []
    for byte in SENTINEL_BYTES:
        with _sentinel_allocations(byte) as made:
            out = fn(*args, **kwargs)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        ts = _tensors(out)
        assert ts, "poisoned(): the op returned no tensor"
        for i, t in enumerate(ts):
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
            assert any(p <= lo and hi <= p + n for p, n in made), \
                f"poisoned(): output {i} ({tuple(t.shape)}) does not lie in a sentinel-filled buffer: the check would be vacuous"
        results.append((out, ts))
    (out0, t0), (_, t1) = results
    for i, (a, b) in enumerate(zip(t0, t1)):
        nonfinite = ~torch.isfinite(a)
        if bool(nonfinite.any()):
            flat = int(nonfinite.reshape(-1).nonzero()[0])
            raise AssertionError(f"poisoned(): output {i} ({tuple(a.shape)}) keeps {int(nonfinite.sum())} unwritten "
                                 f"(NaN-sentinel) elements; first at index {_unravel(flat, tuple(a.shape))}")
        if not torch.equal(a, b):
            diff = (a != b)
            flat = int(diff.reshape(-1).nonzero()[0])
            raise AssertionError(f"poisoned(): output {i} ({tuple(a.shape)}) differs between two runs in "
                                 f"{int(diff.sum())} elements (unwritten, or not deterministic); first at index "
                                 f"{_unravel(flat, tuple(a.shape))}")
    return out0
