"""Physics-Attention for structured 2-D meshes, MI355X-native.

Same constructor, parameter names/shapes and `forward(x[B,N,C]) -> [B,N,C]` as the reference class
of the same name (model/Physics_Attention.py:60-119), but the forward/backward run as a handful of
hand-written HIP kernels (libpa2d): one implicit-GEMM for both 3x3 projections on the NHWC tensor
(no permute copies), MFMA slice-softmax-scatter, an in-LDS token attention, a de-slice that
recomputes the slice weights, and an MFMA GEMM for to_out with bias/residual epilogue.
The nn.Conv2d / nn.Linear sub-modules are parameter containers only (identical state_dict keys and
default initialisation); their own forward is never called.
"""
import torch
import torch.nn as nn

from .. import functional as Fn
from ._core import pad_contraction


class Physics_Attention_Structured_Mesh_2D(nn.Module):
    fused_tail_capable = True      # BlockBase.fused_route: de-slice .. to_out are the stages ops.block_tail_fwd fuses

    def __init__(self, dim, heads=8, dim_head=64, dropout=0., slice_num=64, H=101, W=31, kernel=3):
        super().__init__()
        inner_dim = dim_head * heads
        if kernel != 3:
            raise NotImplementedError("the HIP path implements the 3x3 projection used by every reference script")
        if inner_dim != dim:
            raise NotImplementedError("HIP path needs heads*dim_head == dim (true for every reference model)")
        self.dim_head = dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.softmax = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.temperature = nn.Parameter(torch.ones([1, heads, 1, 1]) * 0.5)
        self.H = H
        self.W = W
        self.engine = None      # GEMM engine (None = pa2d_default_engine()); TransolverBase.set_engine sets it

        self.in_project_x = nn.Conv2d(dim, inner_dim, kernel, 1, kernel // 2)
        self.in_project_fx = nn.Conv2d(dim, inner_dim, kernel, 1, kernel // 2)
        self.in_project_slice = nn.Linear(dim_head, slice_num)
        torch.nn.init.orthogonal_(self.in_project_slice.weight)
        self.to_q = nn.Linear(dim_head, dim_head, bias=False)
        self.to_k = nn.Linear(dim_head, dim_head, bias=False)
        self.to_v = nn.Linear(dim_head, dim_head, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))

    def attention_parameters(self):
        return (self.temperature, self.in_project_x.weight, self.in_project_x.bias, self.in_project_fx.weight,
                self.in_project_fx.bias, self.in_project_slice.weight, self.in_project_slice.bias,
                self.to_q.weight, self.to_k.weight, self.to_v.weight, self.to_out[0].weight, self.to_out[0].bias)

    def forward(self, x, residual=None):
        """x: [B, N=H*W, C].  `residual` (extension): added in the to_out epilogue (block uses it)."""
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("dropout > 0 is not implemented in the HIP path (every reference script "
                                      "uses --dropout 0.0); refusing to silently ignore it")
        B, N, C = x.shape
        if N != self.H * self.W:
            raise RuntimeError(f"shape '[{B}, {self.H}, {self.W}, {C}]' is invalid for input of size {x.numel()}")
        return Fn.physics_attention(x, residual, self.H, self.W, self.heads, self.attention_parameters(),
                                    engine=self.engine)


class Physics_Attention_Structured_Mesh_3D(nn.Module):
    """Physics-Attention for structured 3-D meshes: the reference class of the same name (model/Physics_Attention.py,
    Physics_Attention_Structured_Mesh_3D) with the same constructor, parameter names and shapes (`in_project_x.weight`
    [C, C, 3, 3, 3]) and `forward(x[B,N,C]) -> [B,N,C]`, N = H*W*D with point n = (h*W + w)*D + d.  Both Conv3d
    projections run as one 27-tap implicit GEMM of libpa2d (pa2d_conv3x3x3x2_*); slice, token attention, de-slice and
    to_out are the kernels of the 2-D class.  The nn.Conv3d / nn.Linear sub-modules are parameter containers only."""
    fused_tail_capable = True

    def __init__(self, dim, heads=8, dim_head=64, dropout=0., slice_num=32, H=32, W=32, D=32, kernel=3):
        super().__init__()
        inner_dim = dim_head * heads
        if kernel != 3:
            raise NotImplementedError("the HIP path implements the 3x3x3 projection of the reference")
        if inner_dim != dim:
            raise NotImplementedError("HIP path needs heads*dim_head == dim (true for every reference model)")
        self.dim_head = dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.softmax = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.temperature = nn.Parameter(torch.ones([1, heads, 1, 1]) * 0.5)
        self.H = H
        self.W = W
        self.D = D
        self.engine = None      # GEMM engine (None = pa2d_default_engine()); TransolverBase.set_engine sets it

        self.in_project_x = nn.Conv3d(dim, inner_dim, kernel, 1, kernel // 2)
        self.in_project_fx = nn.Conv3d(dim, inner_dim, kernel, 1, kernel // 2)
        self.in_project_slice = nn.Linear(dim_head, slice_num)
        torch.nn.init.orthogonal_(self.in_project_slice.weight)
        self.to_q = nn.Linear(dim_head, dim_head, bias=False)
        self.to_k = nn.Linear(dim_head, dim_head, bias=False)
        self.to_v = nn.Linear(dim_head, dim_head, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))

    @property
    def mesh_w(self):
        """The geometry argument `W` of the functional layer: (width, depth) selects the 3x3x3 conv."""
        return (self.W, self.D)

    def attention_parameters(self):
        return (self.temperature, self.in_project_x.weight, self.in_project_x.bias, self.in_project_fx.weight,
                self.in_project_fx.bias, self.in_project_slice.weight, self.in_project_slice.bias,
                self.to_q.weight, self.to_k.weight, self.to_v.weight, self.to_out[0].weight, self.to_out[0].bias)

    def forward(self, x, residual=None):
        """x: [B, N=H*W*D, C].  `residual` (extension): added in the to_out epilogue (block uses it)."""
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("dropout > 0 is not implemented in the HIP path; refusing to silently ignore it")
        B, N, C = x.shape
        if N != self.H * self.W * self.D:
            raise RuntimeError(f"shape '[{B}, {self.H}, {self.W}, {self.D}, {C}]' is invalid for input of size {x.numel()}")
        return Fn.physics_attention(x, residual, self.H, self.mesh_w, self.heads, self.attention_parameters(),
                                    engine=self.engine)


class Physics_Attention_Structured_Mesh_2D_Auto_Encoder(nn.Module):
    """The auto-encoder attention of the reference (model/Physics_Attention.py,
    Physics_Attention_Structured_Mesh_2D_Auto_Encoder): the 2-D structured attention plus `project_slice`
    (Linear(M, M)) and the cached slice weights.  Same constructor, parameter names and order, `forward` /
    `encode(x, cache_slice)` / `reconstruct_fx(code)` / `decode(code)`.

    State: `slice_weights` is None until `encode(..., cache_slice=True)` stores the softmax slice weights [B,heads,N,M]
    there; `reconstruct_fx` replaces it by project_slice(slice_weights) (a new tensor, never written in place), and
    `decode` de-slices with whatever it holds.  `forward` is the plain 2-D attention (project_slice takes no part)."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0., slice_num=64, H=101, W=31, kernel=3):
        super().__init__()
        inner_dim = dim_head * heads
        if kernel != 3:
            raise NotImplementedError("the HIP path implements the 3x3 projection used by every reference script")
        if inner_dim != dim:
            raise NotImplementedError("HIP path needs heads*dim_head == dim (true for every reference model)")
        self.dim_head = dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.softmax = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.temperature = nn.Parameter(torch.ones([1, heads, 1, 1]) * 0.5)
        self.H = H
        self.W = W
        self.slice_weights = None
        self.engine = None

        self.in_project_x = nn.Conv2d(dim, inner_dim, kernel, 1, kernel // 2)
        self.in_project_fx = nn.Conv2d(dim, inner_dim, kernel, 1, kernel // 2)
        self.in_project_slice = nn.Linear(dim_head, slice_num)
        torch.nn.init.orthogonal_(self.in_project_slice.weight)
        self.to_q = nn.Linear(dim_head, dim_head, bias=False)
        self.to_k = nn.Linear(dim_head, dim_head, bias=False)
        self.to_v = nn.Linear(dim_head, dim_head, bias=False)
        self.project_slice = nn.Linear(slice_num, slice_num)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))

    def attention_parameters(self):
        return (self.temperature, self.in_project_x.weight, self.in_project_x.bias, self.in_project_fx.weight,
                self.in_project_fx.bias, self.in_project_slice.weight, self.in_project_slice.bias,
                self.to_q.weight, self.to_k.weight, self.to_v.weight, self.to_out[0].weight, self.to_out[0].bias)

    def encoder_parameters(self):
        """The parameters of `encode`, in functional.ENC_KEYS order."""
        return self.attention_parameters()[:10]

    def _check(self, x):
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("dropout > 0 is not implemented in the HIP path; refusing to silently ignore it")
        B, N, C = x.shape
        if N != self.H * self.W:
            raise RuntimeError(f"shape '[{B}, {self.H}, {self.W}, {C}]' is invalid for input of size {x.numel()}")

    def forward(self, x, residual=None):
        """x: [B, N=H*W, C].  `residual` (extension): added in the to_out epilogue (block uses it)."""
        self._check(x)
        return Fn.physics_attention(x, residual, self.H, self.W, self.heads, self.attention_parameters(),
                                    engine=self.engine)

    def encode(self, x, cache_slice=False):
        """out_slice_token [B, heads, M, D]; with cache_slice the softmax slice weights go to `slice_weights`."""
        self._check(x)
        code, x_mid = Fn.attention_encode(x, self.H, self.W, self.heads, self.encoder_parameters(), engine=self.engine)
        if cache_slice:
            self.slice_weights = Fn.slice_weights(x_mid, self.temperature, self.in_project_slice.weight,
                                                  self.in_project_slice.bias)
        return code

    def project_cached(self):
        """slice_weights <- project_slice(slice_weights) (a new tensor); returns it."""
        sw = self.slice_weights
        if sw is None:
            raise RuntimeError("decode before encode: no slice weights are cached (call encode(..., cache_slice=True) "
                               "or set them first)")
        p = self.project_slice
        x, w = pad_contraction(sw, p.weight)
        self.slice_weights = Fn.linear(x, w, p.bias, None, engine=self.engine)
        return self.slice_weights

    def reconstruct_fx(self, code):
        w = self.project_cached()
        return Fn.linear(Fn.deslice_weights(code, w), self.to_out[0].weight, self.to_out[0].bias, None, engine=self.engine)

    def decode(self, code):
        if self.slice_weights is None:
            raise RuntimeError("decode before encode: no slice weights are cached")
        y = Fn.deslice_weights(code, self.slice_weights)
        return Fn.linear(y, self.to_out[0].weight, self.to_out[0].bias, None, engine=self.engine)
