"""The broadcast embedding add (csrc/pa2d_embed_bias.hip, functional.embed_bias, TransolverBase._embed).

Cases: B = 3 x N in {1, 37, 300} x C in {8, 64, 256} (2, 16 and 64 float4 columns: 128, 16 and 4 row lanes per workgroup;
N = 300 with C = 64 / 256 makes 2 / 5 row chunks per sample) x placeholder alone, time vector alone, both.
Forward: bit-equal to `(h + placeholder[None, None, :]) + tvec[:, None, :]`.  Backward: dtvec[b, c] = sum_n dz[b, n, c] and
dplaceholder[c] = sum_b dtvec[b, c] against float64, element by element, |got - ref| <= TAU * sum |dz| (the policy of
tests/elementwise_check.py).  With u = 2^-24 an fp32 sum of depth k is within k u of the exact one relative to the sum of
absolute values; here a lane adds at most ceil(ceil(N / chunks) / row lanes) <= 15 rows (N = 300, C = 256: 60 rows over 4
lanes), the row lanes are added pairwise (<= 7 levels, 128 lanes), the chunks and the samples in double with one rounding
each: <= 15 + 7 + 2 = 24u, TAU = 24u."""
import pytest
import torch

from elementwise_check import check_products, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 24 * 2.0 ** -24
B = 3
NS = (1, 37, 300)
CS = (8, 64, 256)
ADDENDS = ("placeholder", "tvec", "both")

_DATA = {}


def data(N, C):
    if (N, C) not in _DATA:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + C)
        _DATA[(N, C)] = tuple(torch.randn(*s, device=DEV, generator=g) for s in ((B, N, C), (C,), (B, C), (B, N, C)))
    return _DATA[(N, C)]


def torch_expression(h, p, t):
    z = h if p is None else h + p[None, None, :]
    return z if t is None else z + t[:, None, :]


@pytest.mark.parametrize("which", ADDENDS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", NS)
def test_forward_bits_and_backward_column_sums(N, C, which):
    from transformerbasednavierstokesolver_amd import ops
    h, p, t, dz = data(N, C)
    p = p if which in ("placeholder", "both") else None
    t = t if which in ("tvec", "both") else None
    z = poisoned(ops.embed_bias_fwd, h, p, t)
    assert torch.equal(z, torch_expression(h, p, t))
    dp, dt = poisoned(ops.embed_bias_bwd, dz, p is not None, t is not None)
    assert (dp is None) == (p is None) and (dt is None) == (t is None)
    d64, label = dz.double(), f"N={N} C={C} {which}"
    if dt is not None:
        w = check_products(dt, d64.sum(1), d64.abs().sum(1), TAU, label=label + " dtvec")
        print(f"{label} dtvec: worst |err| / scale {w:.2e} (bound {TAU:.2e})")
    if dp is not None:
        w = check_products(dp, d64.sum((0, 1)), d64.abs().sum((0, 1)), TAU, label=label + " dplaceholder")
        print(f"{label} dplaceholder: worst |err| / scale {w:.2e} (bound {TAU:.2e})")
    if which == "both":
        assert torch.equal(dp, dt.double().sum(0).float())           # the sum of dtvec over b, as documented


def test_autograd_hands_dz_on_and_matches_the_torch_expression():
    from transformerbasednavierstokesolver_amd import functional as Fn
    h, p, t, dz = data(37, 64)
    leaves = [x.clone().requires_grad_(True) for x in (h, p, t)]
    z = Fn.embed_bias(*leaves)
    z.backward(dz)
    ref = [x.clone().double().requires_grad_(True) for x in (h, p, t)]
    torch_expression(*ref).backward(dz.double())
    assert torch.equal(z.detach(), torch_expression(h, p, t)) and torch.equal(leaves[0].grad, dz)
    for got, want in zip(leaves[1:], ref[1:]):
        assert float((got.grad.double() - want.grad).norm() / want.grad.norm()) <= 1e-6
    # an addend that asks for no gradient gets none, and no reduction runs for it
    z = Fn.embed_bias(leaves[0], p, None)
    (gh,) = torch.autograd.grad(z, leaves[0], dz)
    assert torch.equal(gh, dz)


def test_upstream_gradient_at_an_odd_offset():
    """A contiguous dz that is a view one float past a 16-byte boundary: the backward reduces an aligned copy (the kernel
    reads 16 bytes at a time) instead of raising; the same bits as for the aligned tensor."""
    from transformerbasednavierstokesolver_amd import functional as Fn, ops
    h, p, t, dz = data(37, 64)
    buf = torch.zeros(dz.numel() + 1, device=DEV)
    buf[1:] = dz.reshape(-1)
    odd = buf[1:].view_as(dz)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    leaves = [x.clone().requires_grad_(True) for x in (h, p, t)]
    Fn.embed_bias(*leaves).backward(odd)
    dp, dt = ops.embed_bias_bwd(dz, True, True)
    assert torch.equal(leaves[1].grad, dp) and torch.equal(leaves[2].grad, dt) and torch.equal(leaves[0].grad, dz)


def test_in_place_over_the_input():
    from transformerbasednavierstokesolver_amd import ops
    h, p, t, _ = data(37, 64)
    buf = h.clone()
    out = ops.embed_bias_fwd(buf, p, t, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, torch_expression(h, p, t))


def test_width_that_is_no_multiple_of_four_is_refused_and_the_model_takes_the_torch_route():
    from transformerbasednavierstokesolver_amd import _lib, functional as Fn, ops
    lib = _lib.load()
    x = torch.zeros(64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pa2d_embed_bias_fwd(x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), 1, 2, 6, stream) == 1002
    assert lib.pa2d_embed_bias_bwd(x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), 256, 1, 2, 6, stream) == 1002
    assert lib.pa2d_embed_bias_fwd(x.data_ptr() + 4, 0, 0, x.data_ptr(), 1, 2, 8, stream) == 1001      # 16-byte contract
    g = torch.Generator(device=DEV).manual_seed(5)
    h, p, t = (torch.randn(*s, device=DEV, generator=g) for s in ((B, 5, 6), (6,), (B, 6)))
    real = ops.embed_bias_fwd

    def refuse(*a, **k):
        raise AssertionError("the kernel ran")

    ops.embed_bias_fwd = refuse
    try:
        assert not ops.embed_bias_supported(h, p, t)
        assert torch.equal(Fn.embed_bias(h, p, t), torch_expression(h, p, t))
    finally:
        ops.embed_bias_fwd = real


def test_model_embedding_goes_through_the_kernel_and_keeps_its_bits():
    """Transolver_Structured_Mesh_2D with Time_Input: forward(x, None, T=T) makes ONE embed_bias call (placeholder and
    time vector together), forward(x, None) one with the placeholder alone, forward(x, fx) none (no addend); the
    embedding equals the torch expression bit for bit."""
    from transformerbasednavierstokesolver_amd import ops
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh_2D import Model
    torch.manual_seed(0)
    kw = dict(space_dim=2, n_layers=1, n_hidden=32, n_head=4, Time_Input=True, out_dim=1, slice_num=8, H=6, W=5)
    m0, m1 = Model(fun_dim=0, **kw).to(DEV), Model(fun_dim=1, **kw).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    x, fx = torch.rand(2, 30, 2, device=DEV, generator=g), torch.randn(2, 30, 1, device=DEV, generator=g)
    T = torch.tensor([[0.25], [0.75]], device=DEV)
    calls = []
    real = ops.embed_bias_fwd
    ops.embed_bias_fwd = lambda h, p=None, t=None, out=None: calls.append((p is not None, t is not None)) or real(h, p, t, out)
    try:
        with torch.no_grad():
            m1(x, fx)
            assert calls == []
            m0(x, None, T=T)
            m0(x, None)
            assert calls == [(True, True), (True, False)]
            z = m1._embed(x, fx, always_placeholder=False, T=T)
            assert calls[-1] == (False, True)
            h = m1.preprocess(torch.cat((x, fx), -1))
            want = h + m1._time_vector(T)[:, None, :]
            assert torch.equal(z, want)
            z0 = m0._embed(x, None, always_placeholder=False, T=T)
            assert torch.equal(z0, (m0.preprocess(x) + m0.placeholder[None, None, :]) + m0._time_vector(T)[:, None, :])
    finally:
        ops.embed_bias_fwd = real
