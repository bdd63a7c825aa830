"""The split engine's weight-gradient kernels on both MFMA shapes (PA2D_MC_MFMA=32: v_mfma_f32_32x32x16_bf16 on 16-row
K-steps; PA2D_MC_MFMA=16: v_mfma_f32_16x16x32_bf16 on 32-row K-steps read from two of three 16-row LDS slots).

Every case runs once per PA2D_MC_MFMA value and asserts, per arm: whole-tensor rel-L2 against fp64 under BWD_TOL of
test_gpu_stages.py, the per-element bound TAU[("split", "wgrad")] on poisoned outputs exactly as test_gpu_elementwise.py
checks it, and then that the two arms agree to fp32 rounding (rel-L2 < 1e-6, the bound of test_conv_halo_both_mfma_shapes).

Shapes (pa2d_gemm_mc_planes.hip: plan_mc_planes_big, plan_mc, mc_f32src_applies):
  conv (B, H, W, C), Mi = 2C rows x Nj = 9C columns of 256 x 256 tiles, K = B*H*W pixel rows in 16-row chunks
    (1, 24, 24, 128)  36 chunks -> 4 splits of 9: every split ends on a half-empty 32-row step; 1152 columns: ragged tile
    (2, 24, 24, 192)  ragged tiles in both directions, taps that change inside a column tile
    (1, 40, 30, 128)  75 chunks (odd); W = 30: pixel rows wrap inside a K-step
    (2, 64, 64, 256)  the bench's channel geometry
  linear (M, N, K), dW [N, K] on 128 x 128 tiles when M >= 2048 and N, K > 64
    (200, 64, 64)     the calibrated worst case of the wgrad family
    (1029, 256, 256)  an odd chunk count and a 5-row tail
    (4096, 256, 128)  fp32-source planes kernel, 32 splits of 8 chunks
    (2600, 256, 192)  fp32-source planes kernel: 163 chunks -> splits of 11 (odd: half-empty last step), the last split 9
                      chunks with an 8-row tail, ragged column tile (192 = 128 + 64)
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from elementwise_check import TAU, check_products, poisoned
from test_gpu_stages import BWD_TOL, FWD_TOL, _check_conv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARMS = ("32", "16")
ARM_TOL = 1e-6
TAU_W = TAU[("split", "wgrad")]


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("B,H,W,C", [(1, 24, 24, 128), (2, 24, 24, 192), (1, 40, 30, 128), (2, 64, 64, 256)])
def test_conv_weight_gradient_both_mfma_shapes(kernel_env, B, H, W, C):
    from transformerbasednavierstokesolver_amd import ops
    from test_gpu_elementwise import _conv_refs
    rng = np.random.default_rng(B * H + W + C)
    x, dout = _r(rng, B, H * W, C), _r(rng, B, H * W, 2 * C)
    wx, wf = _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5), _r(rng, C, C, 3, 3, scale=(9 * C) ** -0.5)
    bx, bf = 0.1 * _r(rng, C), 0.1 * _r(rng, C)
    ref, scale = _conv_refs(x.double(), wx.double(), bx.double(), wf.double(), bf.double(), dout.double(), H, W)
    (_, _, dwx_r, dbx_r, dwf_r, dbf_r), (_, _, dwx_s, dbx_s, dwf_s, dbf_s) = ref, scale
    got = {}
    for arm in ARMS:
        kernel_env(PA2D_MC_MFMA=arm)
        _check_conv(DEV, B, H, W, C, "split", FWD_TOL, BWD_TOL)
        _, dwx, dbx, dwf, dbf = poisoned(ops.conv3x3x2_bwd, dout, x, wx, wf, H, W, engine="split")
        tag = f"[split] conv B={B} H={H} W={W} C={C} PA2D_MC_MFMA={arm}"
        for g, r, s, name in ((dwx, dwx_r, dwx_s, "dwx"), (dwf, dwf_r, dwf_s, "dwf")):
            v = check_products(g.reshape(C, -1), r.reshape(C, -1), s.reshape(C, -1), TAU_W, label=f"{tag} {name} [co, ci*9+tap]")
            print(f"{tag} {name}: worst |err| / scale {v:.3e}, rel-L2 {rel_l2(g, r):.3e}")
            assert rel_l2(g, r) < BWD_TOL
        check_products(dbx, dbx_r, dbx_s, TAU_W, label=tag + " dbx")
        check_products(dbf, dbf_r, dbf_s, TAU_W, label=tag + " dbf")
        got[arm] = (dwx, dwf)
    for a, b, name in zip(got["16"], got["32"], ("dwx", "dwf")):
        d = rel_l2(a, b)
        print(f"conv B={B} H={H} W={W} C={C} {name}: 16 vs 32 rel-L2 {d:.3e}")
        assert d < ARM_TOL


@pytest.mark.parametrize("M,N,K", [(200, 64, 64), (1029, 256, 256), (4096, 256, 128), (2600, 256, 192)])
def test_linear_weight_gradient_both_mfma_shapes(kernel_env, M, N, K):
    from transformerbasednavierstokesolver_amd import ops
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    x, dy = _r(rng, M, K), _r(rng, M, N)
    xd, dyd = x.double(), dy.double()
    dw_r, dw_s = dyd.t() @ xd, dyd.abs().t() @ xd.abs()
    db_r, db_s = dyd.sum(0), dyd.abs().sum(0)
    got = {}
    for arm in ARMS:
        kernel_env(PA2D_MC_MFMA=arm)
        dw, db = poisoned(ops.linear_bwd_weight, dy, x, engine="split")
        tag = f"[split] linear M={M} N={N} K={K} PA2D_MC_MFMA={arm}"
        vw = check_products(dw, dw_r, dw_s, TAU_W, label=tag + " weight gradient")
        vb = check_products(db, db_r, db_s, TAU_W, label=tag + " bias gradient")
        print(f"{tag}: worst |err| / scale dw {vw:.3e} db {vb:.3e}, rel-L2 dw {rel_l2(dw, dw_r):.3e} db {rel_l2(db, db_r):.3e}")
        assert rel_l2(dw, dw_r) < BWD_TOL and rel_l2(db, db_r) < BWD_TOL
        got[arm] = (dw, db)
    for a, b, name in zip(got["16"], got["32"], ("dw", "db")):
        d = rel_l2(a, b)
        print(f"linear M={M} N={N} K={K} {name}: 16 vs 32 rel-L2 {d:.3e}")
        assert d < ARM_TOL


@pytest.mark.parametrize("B,H,W,C", [(1, 24, 24, 128), (1, 40, 30, 128)])
def test_small_tile_conv_weight_gradient_with_mfma16_selected(kernel_env, B, H, W, C):
    """PA2D_MC_BIG=off sends the conv weight gradient to the 128 x 128 planes kernel, which stays on 32x32x16 whatever
    PA2D_MC_MFMA says: the selection must not disturb it."""
    kernel_env(PA2D_MC_BIG="off", PA2D_MC_MFMA="16")
    _check_conv(DEV, B, H, W, C, "split", FWD_TOL, BWD_TOL)
