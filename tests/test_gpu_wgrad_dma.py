"""The 256 x 256 conv weight gradient (gemm_mc_planes_big_kernel, 16x16x32 form) with its LDS slots filled by
buffer_load ... lds (PA2D_MC_DMA) and with the six split terms of an accumulator issued back to back (PA2D_MC_CHAIN).

Both arms keep the per-accumulator order of the register-staged kernel, so conv3x3x2_bwd_planes on the split engine must
return the same bits under PA2D_MC_DMA=0 PA2D_MC_CHAIN=0, PA2D_MC_DMA=1 PA2D_MC_CHAIN=0 and PA2D_MC_DMA=1 PA2D_MC_CHAIN=1:
torch.equal on dwx, dwf and the data gradient, no tolerance.  Every arm runs through `poisoned` (slabs and gradient buffers
pre-filled with NaN, then 1.2e30: a slot or a 16-byte piece the DMA never wrote, or wrote late, shows as a surviving
sentinel, a run-to-run difference or a difference between arms), and the library's default arm meets the per-element
fp64 bounds of elementwise_check.TAU as the other weight-gradient tests apply them.

Shapes (B, H, W, C); all take the 256 x 256 route (Mi = 2C >= 256, C % 32 == 0, B*H*W >= 512):
  (1, 24, 24, 128)  576 rows: an even number of 16-row chunks
  (1, 20, 27, 128)  540 rows: a ragged last chunk and a half-empty 32-row step
  (2, 32, 32, 256)  two i-tiles, split boundaries inside a sample
  (3, 17, 33, 128)  image rows narrower and wider than a 32-pixel run: tap shifts cross row ends and sample ends
"""
import numpy as np
import pytest
import torch

from elementwise_check import TAU, check_products, poisoned, to_planes, unplane
from test_gpu_elementwise import DEV, _conv_refs, _r

pytestmark = pytest.mark.gpu
BASE = dict(PA2D_MC_DMA="0", PA2D_MC_CHAIN="0")
ARMS = [dict(PA2D_MC_DMA="1", PA2D_MC_CHAIN="0"), dict(PA2D_MC_DMA="1", PA2D_MC_CHAIN="1")]
DEFAULT = dict(PA2D_MC_DMA=None, PA2D_MC_CHAIN=None)


@pytest.mark.parametrize("B,H,W,C", [(1, 24, 24, 128), (1, 20, 27, 128), (2, 32, 32, 256), (3, 17, 33, 128)])
def test_conv_weight_gradient_dma_and_chain_arms(kernel_env, B, H, W, C):
    from transformerbasednavierstokesolver_amd import ops
    N, rows = H * W, B * H * W
    assert 2 * C >= 256 and C % 32 == 0 and rows >= 512      # the 256 x 256 route
    assert ops.conv_planes_mask(B, H, W, C, "split") == 7
    rng = np.random.default_rng(B * H + W + C)
    ximg, dimg = to_planes(_r(rng, rows, C), 3), to_planes(_r(rng, rows, 2 * C), 3)
    wx, wf = _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5), _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5)
    bx, bf = 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    tag = f"conv planes wgrad B={B} H={H} W={W} C={C}"

    def run(env):
        kernel_env(**env)
        return poisoned(ops.conv3x3x2_bwd_planes, dimg, ximg, wx, wf, B, H, W, "split")

    base = run(BASE)
    for env in ARMS:
        for got, want, name in zip(run(env), base, ("data gradient", "dwx", "dwf")):
            assert torch.equal(got, want), \
                f"{tag} {env}: {name} differs from PA2D_MC_DMA=0 PA2D_MC_CHAIN=0 in {int((got != want).sum())} elements"

    dxn, dwx, dwf = run(DEFAULT)
    xs, ds = unplane(ximg, rows, C, 3)[1].view(B, N, C), unplane(dimg, rows, 2 * C, 3)[1].view(B, N, 2 * C)
    (_, dx_r, dwx_r, _, dwf_r, _), (_, dx_s, dwx_s, _, dwf_s, _) = _conv_refs(
        xs, wx.double(), bx.double(), wf.double(), bf.double(), ds, H, W)
    for got, ref, sc, name in ((dwx, dwx_r, dwx_s, "dwx"), (dwf, dwf_r, dwf_s, "dwf")):
        v = check_products(got.reshape(C, -1), ref.reshape(C, -1), sc.reshape(C, -1), TAU[("split", "wgrad")],
                           label=f"{tag} default arm {name} [co, ci*9+tap]")
        print(f"{tag} default arm {name}: worst |err| / scale {v:.3e}")
    check_products(dxn, dx_r, dx_s, TAU[("split", "fwd")], hw=(H, W), label=f"{tag} default arm data gradient")
    for got, want in zip((dxn, dwx, dwf), base):
        assert torch.equal(got, want)
