"""The halo conv's 16x16x32 consumers read their LDS fragments ahead of use (conv_halo_kernel<3, float, 1, true>);
PA2D_CONV_AHEAD=0 selects the reference loop (conv_halo_ref_kernel).  Both issue the same MFMAs per accumulator in the
same order, so forward outputs and data gradients are bit-equal; every case runs with PA2D_CONV_HALO=force.

Shapes (B, H, W, C); the data gradient has 2C input channels, so twice the chunks:
  (1, 8, 32, 32)    one chunk, nine stages, no halo swap, one exact 8 x 32 tile
  (1, 9, 33, 64)    one swap in the forward, three in the backward; tiles ragged in both directions
  (2, 17, 40, 96)   odd chunk count; stage count no multiple of 4; 192 output channels: a ragged channel tile; two images
  (1, 21, 17, 128)  a shape of test_conv_halo_both_mfma_shapes
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from elementwise_check import poisoned
from test_gpu_stages import BWD_TOL, FWD_TOL, _check_conv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 8, 32, 32), (1, 9, 33, 64), (2, 17, 40, 96), (1, 21, 17, 128)]


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _inputs(B, H, W, C, seed):
    rng = np.random.default_rng(seed)
    s = (9 * C) ** -0.5
    return dict(xn=_r(rng, B, H * W, C), wx=_r(rng, C, C, 3, 3, scale=s), wf=_r(rng, C, C, 3, 3, scale=s),
                bx=0.1 * _r(rng, C), bf=0.1 * _r(rng, C), dout=_r(rng, B, H * W, 2 * C))


def _run(t, H, W, wrap=lambda fn, *a, **k: fn(*a, **k)):
    from transformerbasednavierstokesolver_amd import ops
    g = {k: v.to(DEV) for k, v in t.items()}
    out = wrap(ops.conv3x3x2_fwd, g["xn"], g["wx"], g["bx"], g["wf"], g["bf"], H, W, engine="split")
    dxn = wrap(ops.conv3x3x2_bwd, g["dout"], g["xn"], g["wx"], g["wf"], H, W, engine="split")[0]
    return out, dxn


def _oracle(t, H, W):
    from oracle import transolver_oracle as orc
    xd, wxd, wfd, bxd, bfd = (t[k].double() for k in ("xn", "wx", "wf", "bx", "bf"))
    xd.requires_grad_(True)
    out = torch.cat([orc.conv3x3(xd, wxd, bxd, H, W), orc.conv3x3(xd, wfd, bfd, H, W)], -1)
    out.backward(t["dout"].double())
    return out.detach(), xd.grad


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_ahead_and_reference_consumers_are_bit_equal(kernel_env, B, H, W, C):
    t = _inputs(B, H, W, C, B * H + W + C)
    got = {}
    for arm in ("0", None):                                   # None: the default, the read-ahead loop
        # PA2D_CONV_MFMA unset: the 16x16x32 consumers, the only ones with two loops (on 32x32x16 both arms are one kernel)
        kernel_env(PA2D_CONV_HALO="force", PA2D_CONV_MFMA=None, PA2D_CONV_AHEAD=arm)
        _check_conv(DEV, B, H, W, C, "split", FWD_TOL, BWD_TOL)
        got[arm] = _run(t, H, W)
    for name, a, b in zip(("out", "dxn"), got["0"], got[None]):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ between the two loops"


def test_second_run_after_poisoned_buffers_matches_the_oracle(kernel_env):
    """(1, 9, 33, 64) twice in one process with different inputs, every fresh buffer of the calls (outputs, plane images,
    weight packs) pre-filled with NaN and then with 1.2e30: outputs finite, identical under both fills, and the second
    input's result within the fp32 tolerances of its own fp64 oracle.  A fragment read issued across a halo swap would
    multiply another chunk's activations with this chunk's weights and miss the tolerance by orders of magnitude."""
    B, H, W, C = 1, 9, 33, 64
    kernel_env(PA2D_CONV_HALO="force", PA2D_CONV_MFMA=None, PA2D_CONV_AHEAD=None)
    first, second = _inputs(B, H, W, C, 11), _inputs(B, H, W, C, 12)
    out1, dxn1 = _run(first, H, W, wrap=poisoned)
    out2, dxn2 = _run(second, H, W, wrap=poisoned)
    out_o, dxn_o = _oracle(second, H, W)
    assert torch.isfinite(out2).all() and torch.isfinite(dxn2).all()
    assert rel_l2(out2, out_o) < FWD_TOL and rel_l2(dxn2, dxn_o) < BWD_TOL
    assert not torch.equal(out1, out2)
