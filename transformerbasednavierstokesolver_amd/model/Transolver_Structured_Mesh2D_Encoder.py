"""Transolver auto-encoder on structured 2-D meshes — the drop-in for the reference module of the same name
(model/Transolver_Structured_Mesh2D_Encoder.py, trained by auto_encoder.py and loaded frozen by SequenSolver.py,
SequenSolverMerged.py and LearnSlice.py).  `Model` keeps the reference's 15 keyword parameters and defaults,
`__name__ = 'Transolver_2D'`, the state_dict (the 2-D family's plus `blocks.i.Attn.project_slice.{weight,bias}`) and the
stateful interface `encode` / `decode` / `get_attention_slice` / `set_attention_slice`.

The non-last blocks are the 2-D block (project_slice takes no part and gets no gradient).  The last block has no residual
from its input:  code = Attn.encode(ln_1(fx)) caches the slice weights sw;  decode(code) replaces them by
P(sw) = project_slice(sw), then fx = 2 to_out(deslice(code, P(sw))) (the reference adds reconstruct_fx(code) and
Attn.decode(code), the same term twice), fx += mlp(ln_2(fx)), out = mlp2(ln_3(fx)).  Every `decode` projects the cached
weights again, so two calls use P(P(sw)).  bf16 storage (engine 'bf16s') is not implemented for this family and is
refused."""

from .. import functional as Fn
from ._core import ACTIVATION, HEAD_KERNEL_MAX_OUT, MLP, BlockBase, TransolverBase  # noqa: F401  (re-exported like the reference)
from .Physics_Attention import Physics_Attention_Structured_Mesh_2D_Auto_Encoder
from .Transolver_Structured_Mesh_2D import Model as _Model2D


def _refuse_bf16_storage(engine):
    from .. import ops
    if engine is not None and ops.resolve_engine(engine) == ops.ENGINE_BF16S:
        raise NotImplementedError("bf16 storage (engine 'bf16s') is not implemented for the auto-encoder family")


class Transolver_Encoder_block(BlockBase):
    def __init__(self, num_heads, hidden_dim, dropout, act='gelu', mlp_ratio=4, last_layer=False, out_dim=1,
                 slice_num=32, H=85, W=85):
        super().__init__()
        attn = Physics_Attention_Structured_Mesh_2D_Auto_Encoder(hidden_dim, heads=num_heads,
                                                                 dim_head=hidden_dim // num_heads, dropout=dropout,
                                                                 slice_num=slice_num, H=H, W=W)
        self._assemble(attn, hidden_dim, act, mlp_ratio, last_layer, out_dim)

    def forward(self, fx):
        if self.last_layer:
            return self.decode(self.encode(fx))
        return super().forward(fx)

    def encode(self, fx):
        if not self.last_layer:
            return super().forward(fx)
        return self.Attn.encode(Fn.layer_norm(fx, self.ln_1.weight, self.ln_1.bias), cache_slice=True)

    def decode(self, code):
        if not self.last_layer:
            print("the model has to be the last layer")      # the reference's message; it returns None too
            return None
        attn, mlp = self.Attn, self.mlp
        if attn.training and attn.dropout.p > 0:
            raise NotImplementedError("dropout > 0 is not implemented in the HIP path; refusing to ignore it")
        w = attn.project_cached()
        fx = Fn.to_out_twice(Fn.deslice_weights(code, w), attn.to_out[0].weight, attn.to_out[0].bias, engine=self.engine)
        pre, post = mlp.linear_pre[0], mlp.linear_post
        if mlp.linears or pre.weight.shape[1] % 4:
            fx = mlp(Fn.layer_norm(fx, self.ln_2.weight, self.ln_2.bias), residual=fx)
        else:
            fx = Fn.mlp_branch(fx, self.ln_2.weight, self.ln_2.bias, mlp.act_name, pre.weight, pre.bias,
                               post.weight, post.bias, engine=self.engine)
        z = Fn.layer_norm(fx, self.ln_3.weight, self.ln_3.bias)
        if self.mlp2.out_features <= HEAD_KERNEL_MAX_OUT:
            return Fn.head(z, self.mlp2.weight, self.mlp2.bias)
        return Fn.linear(z, self.mlp2.weight, self.mlp2.bias, None, engine=self.engine)


class Model(TransolverBase):
    def __init__(self, space_dim=1, n_layers=5, n_hidden=256, dropout=0.0, n_head=8, Time_Input=False, act='gelu',
                 mlp_ratio=1, fun_dim=1, out_dim=1, slice_num=32, ref=8, unified_pos=False, H=85, W=85):
        super().__init__()
        self.__name__ = 'Transolver_2D'
        self.H, self.W, self.ref, self.unified_pos, self.space_dim = H, W, ref, unified_pos, space_dim
        if unified_pos:
            # non-persistent buffer: follows .cuda()/.to() and stays out of the state_dict, like the reference's plain
            # attribute (whose get_grid hard-codes .cuda())
            self.register_buffer("pos", self.get_grid(), persistent=False)

        def make_block(is_last):
            return Transolver_Encoder_block(num_heads=n_head, hidden_dim=n_hidden, dropout=dropout, act=act,
                                            mlp_ratio=mlp_ratio, last_layer=is_last, out_dim=out_dim,
                                            slice_num=slice_num, H=H, W=W)

        self._assemble(make_block, fun_dim + (ref * ref if unified_pos else space_dim), n_layers, n_hidden,
                       Time_Input, act)

    get_grid = _Model2D.get_grid

    def set_engine(self, engine):
        _refuse_bf16_storage(engine)
        return super().set_engine(engine)

    def _embed_input(self, x, fx, T=None):
        _refuse_bf16_storage(self.engine)
        if self.unified_pos:      # the coordinates in `x` are ignored (only the batch size is used)
            x = self.pos.expand(x.shape[0], -1, -1, -1).reshape(x.shape[0], self.H * self.W, self.ref ** 2)
        return self._embed(x, fx, always_placeholder=False, T=T)

    def forward(self, x, fx, T=None):
        z = self._embed_input(x, fx, T)
        return self._run_blocks(z)

    def encode(self, x, fx):
        """The code [B, heads, M, D] of the last block; caches its slice weights (embedding without T, as the
        reference)."""
        z = self._embed_input(x, fx)
        for block in self.blocks:
            z = block.encode(z)
        return z

    def decode(self, code):
        _refuse_bf16_storage(self.engine)
        return self.blocks[-1].decode(code)

    def get_attention_slice(self):
        return self.blocks[-1].Attn.slice_weights

    def get_attention_code(self):
        return self.blocks[-1].Attn.code      # never set, as in the reference: AttributeError

    def set_attention_slice(self, slice):
        self.blocks[-1].Attn.slice_weights = slice
