"""Transolver for structured 3-D meshes — the drop-in for the reference module of the same name:
`Model` keeps its 16 keyword parameters and defaults (model/Transolver_Structured_Mesh_3D.py), `__name__`,
`use_checkpoint`, `forward(x, fx, T=None)` and the state_dict; the arithmetic runs on libpa2d.  The blocks differ from
the 2-D family only in the attention module (Conv3d projections: the 27-tap implicit GEMM); shared pieces (MLP, block,
init, embedding) are in `_core.py`.  bf16 storage (engine 'bf16s') is not implemented for this family and is refused."""
import numpy as np
import torch
import torch.utils.checkpoint as checkpoint

from ._core import ACTIVATION, MLP, BlockBase, TransolverBase  # noqa: F401  (MLP/ACTIVATION re-exported like the reference)
from .Physics_Attention import Physics_Attention_Structured_Mesh_3D


class Transolver_block(BlockBase):
    serves_dropout = True          # BlockBase.forward: training-mode dropout runs on the HIP kernels

    def __init__(self, num_heads, hidden_dim, dropout, act='gelu', mlp_ratio=4, last_layer=False, out_dim=1,
                 slice_num=32, H=32, W=32, D=32):
        super().__init__()
        attn = Physics_Attention_Structured_Mesh_3D(hidden_dim, heads=num_heads, dim_head=hidden_dim // num_heads,
                                                    dropout=dropout, slice_num=slice_num, H=H, W=W, D=D)
        self._assemble(attn, hidden_dim, act, mlp_ratio, last_layer, out_dim)


def _refuse_bf16_storage(engine):
    from .. import ops
    if engine is not None and ops.resolve_engine(engine) == ops.ENGINE_BF16S:
        raise NotImplementedError("bf16 storage (engine 'bf16s') is not implemented for the 3-D structured mesh")


class Model(TransolverBase):
    def __init__(self, space_dim=1, n_layers=5, n_hidden=256, dropout=0.0, n_head=8, Time_Input=False, act='gelu',
                 mlp_ratio=1, fun_dim=1, out_dim=1, slice_num=32, ref=8, unified_pos=False, H=32, W=32, D=32):
        super().__init__()
        self.__name__ = 'Transolver_3D'
        # reference attribute: run every block under torch.utils.checkpoint (activations recomputed in the backward)
        self.use_checkpoint = False
        self.H, self.W, self.D, self.ref, self.unified_pos, self.space_dim = H, W, D, ref, unified_pos, space_dim
        if unified_pos:
            # non-persistent buffer: follows .cuda()/.to() and stays out of the state_dict, like the reference's plain
            # attribute (whose get_grid hard-codes .cuda())
            self.register_buffer("pos", self.get_grid(), persistent=False)

        def make_block(is_last):
            return Transolver_block(num_heads=n_head, hidden_dim=n_hidden, dropout=dropout, act=act,
                                    mlp_ratio=mlp_ratio, last_layer=is_last, out_dim=out_dim, slice_num=slice_num,
                                    H=H, W=W, D=D)

        self._assemble(make_block, fun_dim + (ref ** 3 if unified_pos else space_dim), n_layers, n_hidden,
                       Time_Input, act)

    def get_grid(self, batchsize=1):
        """[batchsize, H, W, D, ref^3]: Euclidean distance of mesh point (i/(H-1), j/(W-1), k/(D-1)) to the lattice
        point (a/(ref-1), b/(ref-1), c/(ref-1)), feature index (a*ref + b)*ref + c; linspace in float64, arithmetic in
        float32."""
        axis = lambda n: torch.tensor(np.linspace(0, 1, n), dtype=torch.float)
        gx, gy, gz, lat = axis(self.H), axis(self.W), axis(self.D), axis(self.ref)
        dx2 = (gx[:, None] - lat[None, :]) ** 2           # H, ref
        dy2 = (gy[:, None] - lat[None, :]) ** 2           # W, ref
        dz2 = (gz[:, None] - lat[None, :]) ** 2           # D, ref
        pos = torch.sqrt(dx2[:, None, None, :, None, None] + dy2[None, :, None, None, :, None]
                         + dz2[None, None, :, None, None, :])
        pos = pos.reshape(1, self.H, self.W, self.D, self.ref ** 3)
        return pos.repeat(batchsize, 1, 1, 1, 1).contiguous()

    def set_engine(self, engine):
        _refuse_bf16_storage(engine)
        return super().set_engine(engine)

    def _run_blocks(self, z):
        if not self.use_checkpoint:
            return super()._run_blocks(z)
        # re-entrant form: the blocks' autograd nodes keep their saved tensors on ctx (not save_for_backward), which the
        # saved-tensor hooks of the non-re-entrant form never see; here the forward runs without a graph and is redone
        # inside the backward, so the activations of a block really are freed in between
        if any(block.training_dropout() > 0 for block in self.blocks):
            # the recomputation would reserve NEW draws: the gradient would belong to other masks than the loss
            raise NotImplementedError("use_checkpoint with training-mode dropout > 0 is not implemented: the package's dropout "
                                      "generator is not rewound for the recomputation; refusing to mix two sets of masks")
        for block in self.blocks:
            z = checkpoint.checkpoint(block, z, use_reentrant=True)
        return z

    def forward(self, x, fx, T=None):
        _refuse_bf16_storage(self.engine)
        if self.unified_pos:      # the coordinates in `x` are ignored (only the batch size is used)
            x = self.pos.expand(x.shape[0], -1, -1, -1, -1).reshape(x.shape[0], self.H * self.W * self.D, self.ref ** 3)
        z = self._embed(x, fx, always_placeholder=False, T=T)
        return self._run_blocks(z)
