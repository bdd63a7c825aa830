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
* `check_abs_rel(got, ref, a, r)`, `adamw_reference`, `exact_sum_probes` / `decode_probe_sum`, `flat_where`: the flat
  streaming kernels of the step tail (tests/test_gpu_step_tail_elementwise.py): |got - ref| <= a + r |ref| per element with
  a message that names the grid-stride trip or the scalar tail, the fp64 statement of one AdamW step with its scales, and
  sums of powers of two that must come out exact and say which term was dropped or doubled when they do not.

The failure messages name the worst element with its row modulo 16 / 32 / 128, its column modulo 64 / 128, the count of
violating elements, the residues mod 32 of the violating rows and, for convs (`hw=(H, W)`), the pixel and whether it
is on the border ring: a tile, lane-group or border pattern is readable from the message alone.

TAU: the per-element bounds of the GPU suite (tests/test_gpu_elementwise.py), per engine and per family ("fwd": the
contraction is a layer width, "wgrad": the contraction runs over the rows of a batch).  Calibration on the MI355X and
the corruptions these values reject: see the docstrings of test_gpu_elementwise.py and test_elementwise_check.py.
"""
from __future__ import annotations

import contextlib
import math

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


# ---------------------------------------------------------------------------------------------- the step tail
# The flat streaming kernels of the step tail (sum of squares, AdamW): 256 threads x one float4 = 1024 floats per workgroup
# sweep, a grid of min(ceil(n / 1024), 2048) workgroups that strides over the float4 body in "trips" of grid * 1024 floats,
# and a scalar tail of n % 4 floats done by workgroup 0 (csrc/pa2d_optim.hip: stream_blocks, adamw_body).
SWEEP, MAX_BLOCKS = 1024, 2048
FLAT_MODS = (4, 256, 1024)
EPS32 = 2.0 ** -24          # half an ulp of 1: one fp32 rounding
ULP32 = 2.0 ** -23          # the floor of every yardstick-derived bound


def stream_grid(n):
    return max(1, min(-(-n // SWEEP), MAX_BLOCKS))


def stream_trips(n, grid=None, vec=4):
    grid = stream_grid(n) if grid is None else grid
    return -(-(n // vec) // (grid * 256))


def flat_where(i, n, grid=None, vec=4):
    """Which part of a flat streaming launch over n floats handles element i: the trip, workgroup and thread of the
    body (256 threads x `vec` floats per workgroup sweep, `grid` workgroups per trip), or the scalar tail of n % vec
    floats.  vec = 1: the element-per-thread kernels (act_bwd, rel_l2_bwd), which have no tail."""
    grid = stream_grid(n) if grid is None else grid
    nv = n // vec
    s = f"index {i} (" + ", ".join(f"mod {m} = {i % m}" for m in FLAT_MODS) + "): "
    if i >= vec * nv:
        return s + f"scalar tail, element {i - vec * nv} of {n % vec} (workgroup 0)"
    trip, r = divmod(i // vec, grid * 256)
    return s + (f"{'float4 ' if vec == 4 else ''}body, trip {trip} of {stream_trips(n, grid, vec)}, workgroup {r // 256} of "
                f"{grid}, thread {r % 256}" + (f", component {i % vec}" if vec > 1 else ""))


def _flat_summary(idx, n, grid, vec):
    """Where the violating elements of a flat launch sit: tail / trips / residues."""
    out = [f"indices [{int(idx.min())} .. {int(idx.max())}]"]
    if n is not None:
        grid = stream_grid(n) if grid is None else grid
        body = idx[idx < vec * (n // vec)]
        out.append(f"{int((idx >= vec * (n // vec)).sum())} in the scalar tail")
        trips = sorted(set(((body // vec) // (grid * 256)).tolist()))
        out.append(f"{body.numel()} in the body, trips {trips[:8]}")
    for m in FLAT_MODS:
        res = sorted(set((idx % m).tolist()))
        out.append(f"mod {m}: {res if len(res) <= 8 else f'{len(res)} residues'}")
    return "; ".join(out)


def check_abs_rel(got, ref, a, r, label="", *, n_flat=None, grid=None, vec=4):
    """Assert |got - ref| <= a + r |ref| element by element (a, r: numbers or tensors of got's shape; a = tau * scale and
    r = 0 gives a check_products-style bound).  Returns the worst |got - ref| / (a + r |ref|): the fraction of the bound
    in use.  The tensors are read as flat; n_flat = n: they are the n floats of one flat streaming launch (grid, vec: see
    flat_where), and the message names the trip or the tail of the worst element and of all violating ones."""
    g = _d(got).reshape(-1)
    rr = _d(ref).to(g.device).reshape(-1)
    assert g.shape == rr.shape, (label, tuple(g.shape), tuple(rr.shape))
    if g.numel() == 0:
        return 0.0
    a = torch.as_tensor(a, dtype=torch.float64, device=g.device).expand_as(_d(got)).reshape(-1) if torch.is_tensor(a) else a
    r = torch.as_tensor(r, dtype=torch.float64, device=g.device).expand_as(_d(got)).reshape(-1) if torch.is_tensor(r) else r
    bound = (a + r * rr.abs()) * torch.ones_like(g)
    err = (g - rr).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))     # 0 <= 0 holds
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))     # NaN compares false: count it
    worst = float(ratio.max())
    bad = ratio > 1.0
    nbad = int(bad.sum())
    if nbad:
        i = int(ratio.argmax())
        idx = bad.nonzero().flatten()
        where = flat_where(i, n_flat, grid, vec) if n_flat is not None else \
            f"index {i} (" + ", ".join(f"mod {m} = {i % m}" for m in FLAT_MODS) + ")"
        raise AssertionError(
            f"{label}: {nbad} of {g.numel()} elements exceed |got - ref| <= a + r |ref|; worst at {where}: got "
            f"{float(g[i]):.9g}, ref {float(rr[i]):.9g}, bound {float(bound[i]):.4g}, |err| / bound = {worst:.3g}; violating "
            f"{_flat_summary(idx, n_flat, grid, vec)}")
    return worst


def adamw_reference(p, g, m, v, lr, beta1, beta2, eps, wd, step, gnorm_sq=None, max_norm=0.0, dtype=torch.float64):
    """One AdamW step as csrc/pa2d_optim.hip's adamw_body states it (torch.optim.AdamW with the clip coefficient
    min(1, max_norm / (sqrt(gnorm_sq) + 1e-6)) applied to the gradient), on copies of the given state in `dtype`; the
    hyper-parameters are Python floats (fp64), never a rounded coefficient row.  Returns (p, m, v) and the scales
    (|p0| + step (beta1 |m0| + (1 - beta1) |g'|) / (sqrt(v) / sqrt(bias2) + eps), |m0| + |g'|, v0 + g'^2) one step's
    rounding is measured against.  dtype=torch.float32 is the
    yardstick: the same statement with every tensor operation rounded to fp32."""
    p, g, m, v = (torch.as_tensor(t).detach().to(dtype) for t in (p, g, m, v))
    coef = 1.0
    if gnorm_sq is not None and max_norm > 0.0:
        coef = min(1.0, max_norm / (math.sqrt(float(gnorm_sq)) + 1e-6))
    gc = g * coef
    bias1, bias2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    m1 = m + (1.0 - beta1) * (gc - m)
    v1 = beta2 * v + (1.0 - beta2) * gc * gc
    upd = (lr / bias1) * m1 / (v1.sqrt() / math.sqrt(bias2) + eps)
    p1 = p * (1.0 - lr * wd) - upd
    # the update on absolute values: where beta1 m0 and (1 - beta1) g' cancel in m1, the update keeps their rounding
    upd_abs = (lr / bias1) * (beta1 * m.abs() + (1.0 - beta1) * gc.abs()) / (v1.sqrt() / math.sqrt(bias2) + eps)
    return (p1, m1, v1), (p.abs() + upd_abs, m.abs() + gc.abs(), v + gc * gc)


def exact_sum_probes(n, positions):
    """fp32 [n], zero except 2^j at positions[j] (at most 12 distinct positions): the squares are 4^j, every subset sum of
    them (and of doubled ones) is below 2^24 and so exact in fp32, and a sum of squares must equal sum_j 4^j bit for bit
    in any order."""
    assert len(positions) <= 12 and len(set(positions)) == len(positions) and all(0 <= q < n for q in positions), positions
    x = torch.zeros(n, dtype=torch.float32)
    for j, q in enumerate(positions):
        x[q] = 2.0 ** j
    return x


def decode_probe_sum(got, positions, n=None, grid=None):
    """Reads a sum of squares of exact_sum_probes(n, positions) digit by digit in base 4: digit j is how often probe j
    was counted.  Returns (is exact, text naming every probe counted 0, 2 or 3 times and where it sits)."""
    want = sum(4 ** j for j in range(len(positions)))
    got = float(got)
    if got == want:
        return True, "exact"
    if not (math.isfinite(got) and got == int(got) and 0 <= got < 4 ** (len(positions) + 1)):
        return False, f"got {got!r}, want {want}: not a sum of the probes' squares"
    k, notes = int(got), []
    for j, q in enumerate(positions):
        d = (k >> (2 * j)) & 3
        if d != 1:
            what = {0: "dropped", 2: "counted twice", 3: "counted three times"}[d]
            notes.append(f"probe 2^{j} {what} at " + (flat_where(q, n, grid) if n is not None else f"index {q}"))
    if k >> (2 * len(positions)):
        notes.append(f"and {k >> (2 * len(positions))} x 4^{len(positions)} more than all probes hold")
    return False, f"got {k}, want {want}: " + "; ".join(notes)
