"""Shared building blocks of the MI355X Transolver models.

The reference keeps one copy of MLP / block / Model per mesh family (model/Transolver_*.py); here the
families differ only in the attention module handed to `TransolverBase._assemble`, so everything else
lives once in this file.  Attribute names (`preprocess`, `time_fc`, `blocks.i.{ln_1,Attn,ln_2,mlp,ln_3,
mlp2}`, `placeholder`) are the reference's, because they ARE the state_dict contract."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as Fn
from .Embedding import timestep_embedding

# activation names accepted by the reference's ACTIVATION table (model/Transolver_Structured_Mesh_2D.py:9-10);
# its 'leaky_relu' entry is an nn.Module instance instead of a class and cannot be constructed there either
ACTIVATION = {'gelu': nn.GELU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid, 'relu': nn.ReLU,
              'softplus': nn.Softplus, 'ELU': nn.ELU, 'silu': nn.SiLU}
HEAD_KERNEL_MAX_OUT = 8        # widest output the dedicated head kernel handles


def pad_contraction(x, w):
    """libpa2d GEMMs load 16 bytes at a time: zero-pad the contraction length to a multiple of 4."""
    rem = w.shape[1] % 4
    if rem:
        x, w = F.pad(x, (0, 4 - rem)), F.pad(w, (0, 4 - rem))
    return x, w


class MLP(nn.Module):
    """Linear -> act -> [hidden Linear -> act (+ skip)] x n_layers -> Linear (reference MLP, :13-38).
    The activation modules inside the Sequentials are parameter-free markers; the arithmetic runs in
    the GEMM epilogues of libpa2d."""

    def __init__(self, n_input, n_hidden, n_output, n_layers=1, act='gelu', res=True):
        super().__init__()
        if act not in ACTIVATION:
            raise NotImplementedError
        self.act_name, self.res = act, res
        self.engine = None              # GEMM engine of this module's kernels (None = pa2d_default_engine())
        self.n_input, self.n_hidden, self.n_output, self.n_layers = n_input, n_hidden, n_output, n_layers
        make = ACTIVATION[act]
        self.linear_pre = nn.Sequential(nn.Linear(n_input, n_hidden), make())
        self.linear_post = nn.Linear(n_hidden, n_output)
        self.linears = nn.ModuleList(nn.Sequential(nn.Linear(n_hidden, n_hidden), make()) for _ in range(n_layers))

    def forward(self, x, residual=None):
        first, last = self.linear_pre[0], self.linear_post
        x, w_first = pad_contraction(x, first.weight)
        if not self.linears:            # the only shape the Transolver blocks use: one fused pair of GEMMs
            return Fn.mlp(x, residual, self.act_name, w_first, first.bias, last.weight, last.bias, engine=self.engine)
        h = Fn.linear(x, w_first, first.bias, self.act_name, engine=self.engine)
        for hidden in self.linears:
            y = Fn.linear(h, hidden[0].weight, hidden[0].bias, self.act_name, engine=self.engine)
            h = y + h if self.res else y
        out = Fn.linear(h, last.weight, last.bias, None, engine=self.engine)
        return out if residual is None else out + residual


class BlockBase(nn.Module):
    """pre-LN residual block: fx += Attn(LN1 fx); fx += MLP(LN2 fx); last block: head(LN3 fx)."""

    # training-mode dropout p > 0 (on the attention matrix and after to_out) is served by the blocks that
    # declare it: the 2-D, 3-D and irregular Transolver_block.  Every other block keeps refusing it.
    serves_dropout = False

    def training_dropout(self):
        """p of the attention's dropout while it applies (the attention is in training mode), else 0."""
        attn = self.Attn
        return float(attn.dropout.p) if attn.training else 0.0

    def _assemble(self, attn, hidden_dim, act, mlp_ratio, last_layer, out_dim):
        self.last_layer = last_layer
        self.engine = None
        self.fused_tail = False         # TransolverBase.set_fused_tail: no-grad forwards take ops.block_tail_fwd
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.Attn = attn
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = MLP(hidden_dim, hidden_dim * mlp_ratio, hidden_dim, n_layers=0, res=False, act=act)
        if last_layer:
            self.ln_3 = nn.LayerNorm(hidden_dim)
            self.mlp2 = nn.Linear(hidden_dim, out_dim)

    def fused_route(self, fx):
        """True when this call takes the fused tail (ops.block_tail_fwd): the flag is on, the block is in eval mode and no
        autograd graph is being recorded, storage is fp32, the block is the plain 2-D / 3-D / irregular block with an
        n_layers = 0 MLP, and the library has the shape.  Everything else is today's route, bit for bit."""
        from .. import ops
        attn, mlp = self.Attn, self.mlp
        if not self.fused_tail or torch.is_grad_enabled() or fx.dtype != torch.float32 or fx.dim() != 3:
            return False
        if self.training_dropout() > 0:         # the tail has no dropout: such a call takes the served route or raises
            return False
        if self.training or self.engine == ops.ENGINE_BF16S or len(mlp.linears):
            return False
        if not getattr(attn, "fused_tail_capable", False):      # the plain 2-D, 3-D and irregular attention declare it
            return False
        C = fx.shape[-1]
        if C % attn.heads or mlp.linear_pre[0].weight.shape[1] != C:
            return False
        return ops.block_tail_supported(C, attn.heads, C // attn.heads, attn.in_project_slice.weight.shape[0],
                                        mlp.n_hidden, mlp.act_name, self.engine)

    def forward_fused(self, fx, xn=None, next_ln=None):
        """The fused route: conv, slice scatter, token attention, tail.  xn = ln_1(fx) from the previous block's tail
        (None: made here); next_ln: the next block's ln_1.  Returns (fx', LN(fx')) with LN = ln_3 on the last block,
        next_ln otherwise (None without one)."""
        attn, mlp = self.Attn, self.mlp
        if xn is None:
            xn = Fn.layer_norm(fx, self.ln_1.weight, self.ln_1.bias)
        ln = self.ln_3 if self.last_layer else next_ln
        pre, post = mlp.linear_pre[0], mlp.linear_post
        P = dict(zip(Fn.ATTN_KEYS, attn.attention_parameters()))
        return Fn.block_tail(fx, xn, P, getattr(attn, "H", None), getattr(attn, "mesh_w", getattr(attn, "W", None)),
                             attn.heads, self.ln_2.weight, self.ln_2.bias, mlp.act_name, pre.weight, pre.bias, post.weight,
                             post.bias, None if ln is None else ln.weight, None if ln is None else ln.bias,
                             engine=self.engine)

    def head(self, z):
        """mlp2 on z = ln_3(fx)."""
        if self.mlp2.out_features <= HEAD_KERNEL_MAX_OUT:
            return Fn.head(z, self.mlp2.weight, self.mlp2.bias)          # fp32 out, whatever the storage type
        return Fn.linear(z, self.mlp2.weight, self.mlp2.bias, None, engine=self.engine).float()

    def forward(self, fx):
        attn, mlp = self.Attn, self.mlp
        if self.fused_tail and self.fused_route(fx):
            fx, z = self.forward_fused(fx)
            return self.head(z) if self.last_layer else fx
        p = self.training_dropout()
        if p > 0:
            from .. import ops
            if not self.serves_dropout:
                raise NotImplementedError("dropout > 0 is not implemented in the HIP path for this block; refusing to ignore it")
            if fx.dtype != torch.float32 or self.engine == ops.ENGINE_BF16S:
                raise NotImplementedError("dropout > 0 is served for fp32 storage only; refusing to ignore it under bf16 storage")
            ops.dropout_constants(p)            # p = 1 has no finite scale: ValueError before any kernel runs
        # each residual branch (LayerNorm -> sub-layer -> + fx) is one autograd node
        # mesh geometry: H, and W (2-D) or (W, D) (3-D attention's `mesh_w`); the irregular mesh has neither
        fx = Fn.attn_branch(fx, self.ln_1.weight, self.ln_1.bias, getattr(attn, "H", None),
                            getattr(attn, "mesh_w", getattr(attn, "W", None)), attn.heads, attn.attention_parameters(),
                            engine=self.engine, dropout=p or None)
        pre, post = mlp.linear_pre[0], mlp.linear_post
        if mlp.linears or pre.weight.shape[1] % 4:      # generic MLP shapes keep the unfused route
            fx = mlp(Fn.layer_norm(fx, self.ln_2.weight, self.ln_2.bias), residual=fx)
        else:
            fx = Fn.mlp_branch(fx, self.ln_2.weight, self.ln_2.bias, mlp.act_name, pre.weight, pre.bias,
                               post.weight, post.bias, engine=self.engine)
        if not self.last_layer:
            return fx
        return self.head(Fn.layer_norm(fx, self.ln_3.weight, self.ln_3.bias))


class TransolverBase(nn.Module):
    def _assemble(self, make_block, in_features, n_layers, n_hidden, Time_Input, act):
        self.Time_Input, self.n_hidden = Time_Input, n_hidden
        self.engine = None
        self.fused_tail = False         # set_fused_tail
        self.preprocess = MLP(in_features, n_hidden * 2, n_hidden, n_layers=0, res=False, act=act)
        if Time_Input:
            self.time_fc = nn.Sequential(nn.Linear(n_hidden, n_hidden), nn.SiLU(), nn.Linear(n_hidden, n_hidden))
        self.blocks = nn.ModuleList(make_block(i == n_layers - 1) for i in range(n_layers))
        self.initialize_weights()
        # created after the init pass, uniform in [0, 1/C) like the reference (…_2D.py:167)
        self.placeholder = nn.Parameter(torch.rand(n_hidden, dtype=torch.float) / n_hidden)

    def initialize_weights(self):
        self.apply(self._init_weights)

    def _init_weights(self, m):
        """Linear: trunc_normal(std .02) / zero bias; LayerNorm: 1 / 0; Conv2d keeps PyTorch's default."""
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, (nn.LayerNorm, nn.BatchNorm1d)):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def _embed(self, x, fx, always_placeholder, T=None):
        """preprocess(x [, fx]) + placeholder (without fx, or always for the irregular mesh) + time_fc(embedding of T):
        the two broadcast adds are ONE launch (Fn.embed_bias), in the order h + placeholder, then + time vector."""
        h = self.preprocess(x if fx is None else torch.cat((x, fx), -1))
        placeholder = self.placeholder if (fx is None or always_placeholder) else None
        return Fn.embed_bias(h, placeholder, None if T is None else self._time_vector(T))

    def _time_vector(self, T):
        """T: [B,1] -> [B, C].  The reference repeats the embedding over the N points before `time_fc`
        (…_2D.py:212-215); that is the same per-point linear map, so it is applied once and broadcast."""
        fc = self.time_fc
        emb = timestep_embedding(T, self.n_hidden)
        tvec = Fn.mlp(emb, None, 'silu', fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias, engine=self.engine)
        return tvec.reshape(T.shape[0], self.n_hidden)

    def set_engine(self, engine):
        """Select the GEMM engine ("f32" | "split" | "bf16" | 0 | 1 | 2 | None = environment default) for every
        kernel of THIS model; other models in the process keep theirs (the library holds no engine state)."""
        from .. import ops
        eng = None if engine is None else ops.resolve_engine(engine)
        for m in self.modules():
            if hasattr(m, "engine"):
                m.engine = eng
        return self

    def set_fused_tail(self, flag=True):
        """Opt in to (or out of) the fused block tail for no-grad forwards of THIS model: each block then runs conv,
        slice scatter, token attention and ONE launch for de-slice .. next LayerNorm (ops.block_tail_fwd).  Training,
        bf16 storage, generic MLPs and shapes outside the kernel keep the default route; so do models whose blocks are
        not the plain Transolver block (the flag is accepted and has no effect).  Default: off."""
        self.fused_tail = bool(flag)
        for m in self.modules():
            if isinstance(m, (BlockBase, TransolverBase)):
                m.fused_tail = bool(flag)
        return self

    def _run_blocks(self, z):
        from .. import ops
        blocks = list(self.blocks)
        if self.fused_tail and blocks and all(
                isinstance(b, BlockBase) and b.fused_tail and b.fused_route(z) for b in blocks) and blocks[-1].last_layer:
            # each tail hands (fx, ln_1 of the next block) on: ln_1 runs once, in front of the first block
            xn = None
            for i, block in enumerate(blocks):
                z, xn = block.forward_fused(z, xn, blocks[i + 1].ln_1 if i + 1 < len(blocks) else None)
            return blocks[-1].head(xn)
        if self.engine == ops.ENGINE_BF16S:
            # bf16 storage: from here on every activation, saved tensor and inter-kernel gradient is bf16 (the cast is
            # the one fp32 -> bf16 boundary; its autograd node casts the gradient back for the fp32 input embedding)
            z = z.to(torch.bfloat16)
        for block in self.blocks:
            z = block(z)
        return z
