"""The decoded, strided relative-L2 kernels (csrc/pa2d_rel_l2_affine.hip, functional.rel_l2_affine,
FusedTestLoss.rel_decoded) against float64, element by element.

Cases: B in {1, 3} x L in {1, 5, 1023, 1025, 4099} (a single lane; a tail that is no multiple of 4; just under and just over
the 1024 elements of one workgroup pass, i.e. one and two workgroups per sample; five workgroups) x target contiguous or
read with element stride 3 x a device mean / std or none x the base of `pred` and of the target's storage one float past a
16-byte boundary or ON it, outputs in NaN- and 1.2e30-prefilled buffers.  `dpred` is a fresh allocation, so it is aligned:
with the aligned base `pred`, a unit-stride target and `dpred` agree in phase and the backward's float4 path runs, with its
head and tail wherever odd L puts the rows of samples 1 and 2 off the boundary (this is what every training call runs); with
the misaligned base they disagree and the backward takes the scalar loop, while the forward peels a head of 3.  A last test
puts `pred` and a unit-stride target at DIFFERENT phases (both ways round): the scalar loop of both kernels.

Bound (policy of tests/elementwise_check.py: |got - ref| <= tau * scale with `scale` the operation on absolute values).
With u = 2^-24, o = pred std + mean, y = y_n std + mean, d = o - y, A_b = || |o| + |y| ||:
  * a decoded value is one fma (<= u relative), the subtraction another u: |delta d_i| <= 2u (|o_i| + |y_i|), so
    |delta ||d|| | <= 2u A;
  * a sum of squares is a product (u) and at most 4 adds in a lane (L <= 4099 over ceil(L / 1024) workgroups of 256 lanes
    x 4 elements) + 6 in the wave + 2 in the block, 13u on the sum = 6.5u on its root, for both norms 13u; the partial
    sums of the workgroups are added in double;
  * two square roots and the division: <= 2u each, 6u.
  ratio: |err| <= 21u A / ||y||.  dpred_i = s d_i with s = gout std / (||d|| ||y||): |err_i| <= |s| (2u (|o_i| + |y_i|)
  + |d_i| (2u A / ||d|| + 20u)) <= 22u |s| ((|o_i| + |y_i|) + |d_i| A / ||d||).
TAU = 24u covers both with the scales `A / ||y||` and `|s| ((|o| + |y|) + |d| A / ||d||)`."""
import numpy as np
import pytest
import torch

from elementwise_check import check_products, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 24 * 2.0 ** -24
BS = (1, 3)
LS = (1, 5, 1023, 1025, 4099)
STRIDES = (1, 3)
NORMS = ((0.02, 0.01), None)


def _stats(norm):
    if norm is None:
        return None, None
    return torch.tensor([norm[0]], device=DEV), torch.tensor([norm[1]], device=DEV)


_DATA = {}


def data(B, L, stride, offset=1, y_offset=None):
    """(pred [B, L], target view [B, L] with element stride `stride`, gout [B]); pred's storage starts `offset` floats past
    a 16-byte boundary, the target's `y_offset` (default: the same).  Seeded (the values depend on the shape alone), made
    once per case."""
    y_offset = offset if y_offset is None else y_offset
    key = (B, L, stride, offset, y_offset)
    if key not in _DATA:
        rng = np.random.default_rng(100 * L + 10 * B + stride)
        y = rng.standard_normal((B, L)).astype(np.float32)
        p = (y + 0.1 * rng.standard_normal((B, L))).astype(np.float32)
        pbuf = torch.zeros(B * L + offset, device=DEV)
        pbuf[offset:] = torch.from_numpy(p).reshape(-1).to(DEV)
        ybuf = torch.full((B * L * stride + y_offset,), 7.0, device=DEV)   # the gaps hold 7: read by mistake, it shows
        yv = ybuf[y_offset:].view(B, L, stride)[..., 0]
        yv.copy_(torch.from_numpy(y).to(DEV))
        gout = torch.from_numpy(rng.uniform(0.5, 2.0, B).astype(np.float32)).to(DEV)
        _DATA[key] = (pbuf[offset:].view(B, L), yv, gout)
        assert _DATA[key][0].data_ptr() % 16 == 4 * offset and yv.data_ptr() % 16 == 4 * y_offset
        assert yv.stride() == (L * stride, stride)
    return _DATA[key]


def reference64(pred, y, gout, norm):
    """(ratio, dpred, scale of ratio, scale of dpred) in float64."""
    p, t, g = pred.double(), y.double(), gout.double()
    mu, sd = (0.0, 1.0) if norm is None else (float(np.float32(norm[0])), float(np.float32(norm[1])))
    o, yy = p * sd + mu, t * sd + mu
    d = o - yy
    dn, yn = d.norm(dim=1), yy.norm(dim=1)
    A = (o.abs() + yy.abs()).norm(dim=1)
    s = (g * sd / (dn * yn))[:, None]
    return dn / yn, s * d, A / yn, s.abs() * ((o.abs() + yy.abs()) + d.abs() * (A / dn)[:, None])


def _check(B, L, stride, norm, offset, y_offset=None):
    from transformerbasednavierstokesolver_amd import ops
    pred, y, gout = data(B, L, stride, offset, y_offset)
    mean, std = _stats(norm)
    dn, yn, ratio = poisoned(ops.rel_l2_affine_fwd, pred, y, mean, std)
    dpred = poisoned(ops.rel_l2_affine_bwd, pred, y, mean, std, dn, yn, gout)
    assert dpred.data_ptr() % 16 == 0
    want, gwant, scale, gscale = reference64(pred, y, gout, norm)
    label = f"B={B} L={L} stride={stride} norm={norm} offset={offset}/{offset if y_offset is None else y_offset}"
    w = check_products(ratio, want, scale, TAU, label=label + " ratio")
    gw = check_products(dpred, gwant, gscale, TAU, label=label + " dpred")
    print(f"{label}: worst |err| / scale: ratio {w:.2e}, dpred {gw:.2e} (bound {TAU:.2e})")


@pytest.mark.parametrize("offset", (1, 0), ids=("misaligned", "aligned"))
@pytest.mark.parametrize("norm", NORMS, ids=("normaliser", "identity"))
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
def test_ratios_and_gradient_element_by_element(B, L, stride, norm, offset):
    _check(B, L, stride, norm, offset)


@pytest.mark.parametrize("offsets", ((0, 1), (1, 0), (0, 2)), ids=("pred-aligned", "target-aligned", "half-way"))
@pytest.mark.parametrize("L", (5, 1025))
def test_prediction_and_target_at_different_phases(L, offsets):
    """Unit-stride `pred` and target whose 16-byte boundaries fall on different elements: no float4 access fits both, so
    both kernels take the scalar loop (B = 3, odd L: every row at its own pair of phases)."""
    _check(3, L, 1, NORMS[0], *offsets)


def test_autograd_runs_the_same_kernels_and_reads_a_time_slice_in_place():
    """FusedTestLoss.rel_decoded on yy[..., t:t+1] of [B, N, 4, T] (the plasticity target): the bits of the kernels called
    on that view, a gradient to pred only, and no copy of the target (the kernel is handed the view itself)."""
    from transformerbasednavierstokesolver_amd import ops
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss, TestLoss
    B, N, T, t = 3, 37, 5, 2
    g = torch.Generator(device=DEV).manual_seed(3)
    yy = torch.randn(B, N, 4, T, device=DEV, generator=g)
    pred = (yy[..., t] + 0.1 * torch.randn(B, N, 4, device=DEV, generator=g)).requires_grad_(True)
    target = yy[..., t:t + 1]
    assert ops.uniform_strides(target) == (T, N * 4 * T)
    calls = []
    real = ops.rel_l2_affine_fwd
    ops.rel_l2_affine_fwd = lambda p, y, *a: calls.append(y) or real(p, y, *a)
    try:
        loss = FusedTestLoss(size_average=False).rel_decoded(pred.reshape(B, -1), target)
    finally:
        ops.rel_l2_affine_fwd = real
    loss.backward()
    assert len(calls) == 1 and calls[0].data_ptr() == target.data_ptr() and calls[0].stride() == target.stride()
    p2 = pred.detach().reshape(B, -1)
    dn, yn, ratio = ops.rel_l2_affine_fwd(p2, target)
    assert torch.equal(loss.detach(), ratio.sum())
    assert torch.equal(pred.grad.reshape(B, -1), ops.rel_l2_affine_bwd(p2, target, None, None, dn, yn, torch.ones(B, device=DEV)))
    # the reshaped copy goes through the 16-byte path, which adds in another order: the same values to rounding
    copy = target.reshape(B, -1).contiguous()
    assert float(((ops.rel_l2_affine_fwd(p2, copy)[2] - ratio) / ratio).abs().max()) <= 1e-6
    p64 = pred.detach().double().requires_grad_(True)
    want = TestLoss(size_average=False)(p64.reshape(B, -1), target.double().reshape(B, -1))
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * float(want.detach())
    assert float((pred.grad.double() - p64.grad).norm() / p64.grad.norm()) <= 5e-6


@pytest.mark.parametrize("offset", (1, 0), ids=("misaligned", "aligned"))
def test_equal_prediction_and_target_give_zeros_never_nan(offset):
    """`pred` is a copy of the target at the same phase: aligned, the backward's float4 path writes the zeros."""
    from transformerbasednavierstokesolver_amd import ops
    _, y, gout = data(3, 1025, 1, offset)
    mean, std = _stats(NORMS[0])
    buf = torch.zeros(y.numel() + offset, device=DEV)
    buf[offset:] = y.reshape(-1)
    same = buf[offset:].view_as(y)
    assert same.data_ptr() != y.data_ptr() and same.data_ptr() % 16 == 4 * offset
    dn, yn, ratio = poisoned(ops.rel_l2_affine_fwd, same, y, mean, std)
    assert torch.equal(ratio, torch.zeros_like(ratio)) and torch.equal(dn, torch.zeros_like(dn))
    dpred = poisoned(ops.rel_l2_affine_bwd, same, y, mean, std, dn, yn, gout)
    assert torch.equal(dpred, torch.zeros_like(dpred))


def test_empty_batch_and_empty_rows_touch_nothing():
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    poison = torch.full((8,), 1.2e30, device=DEV)
    out = [poison.clone() for _ in range(4)]
    x = torch.ones(8, device=DEV)
    ws = torch.zeros(2 * 3 * _lib.REL_L2_AFFINE_SPLIT, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for B, L in ((0, 5), (3, 0)):
        assert lib.pa2d_rel_l2_affine_fwd(x.data_ptr(), x.data_ptr(), 1, L, 0, 0, out[0].data_ptr(), out[1].data_ptr(),
                                          out[2].data_ptr(), ws.data_ptr(), ws.numel() * 4, B, L, stream) == 0
        assert lib.pa2d_rel_l2_affine_bwd(x.data_ptr(), x.data_ptr(), 1, L, 0, 0, out[0].data_ptr(), out[1].data_ptr(),
                                          x.data_ptr(), out[3].data_ptr(), B, L, stream) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, poison) for o in out)
    # a mean without a std is a contract violation, and a workspace that is too small is refused before any launch
    assert lib.pa2d_rel_l2_affine_fwd(x.data_ptr(), x.data_ptr(), 1, 4, x.data_ptr(), 0, out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel() * 4, 2, 4, stream) == 1001
    assert lib.pa2d_rel_l2_affine_fwd(x.data_ptr(), x.data_ptr(), 1, 4, 0, 0, out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr(), ws.data_ptr(), 16, 2, 4, stream) == 1003


def test_empty_batch_through_the_loss_object():
    """B = 0 through FusedTestLoss.rel_decoded and autograd: a zero loss, an empty gradient, nothing raised."""
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss
    pred = torch.empty(0, 5, device=DEV, requires_grad=True)
    loss = FusedTestLoss(size_average=False).rel_decoded(pred, torch.empty(0, 5, device=DEV))
    loss.backward()
    assert float(loss.detach()) == 0.0 and pred.grad.shape == (0, 5)


def test_unfusable_inputs_take_the_torch_path():
    """A float64 target, a target that asks for a gradient and a per-feature normaliser keep torch's arithmetic."""
    from transformerbasednavierstokesolver_amd import ops
    from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss, TestLoss

    class Norm:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def decode(self, x):
            return x * self.std + self.mean

    pred, y, _ = data(3, 5, 1)
    fused, plain = FusedTestLoss(size_average=False), TestLoss(size_average=False)
    real = ops.rel_l2_affine_fwd

    def refuse(*a):
        raise AssertionError("the kernel ran")

    ops.rel_l2_affine_fwd = refuse
    try:
        n64 = Norm(torch.tensor([[0.02]], device=DEV, dtype=torch.float64), torch.tensor([[0.01]], device=DEV, dtype=torch.float64))
        got = fused.rel_decoded(pred, y.double(), n64)
        assert got.dtype == torch.float64 and torch.equal(got, plain.rel_decoded(pred, y.double(), n64))
        wide = Norm(torch.zeros(1, 5, device=DEV), torch.ones(1, 5, device=DEV))
        assert torch.equal(fused.rel_decoded(pred, y, wide), plain.rel_decoded(pred, y, wide))
        yg = y.clone().requires_grad_(True)
        fused.rel_decoded(pred, yg).backward()
        assert yg.grad is not None and float(yg.grad.abs().max()) > 0
    finally:
        ops.rel_l2_affine_fwd = real
