"""SequenSolver, merged form — the latent sequence model that predicts the code of the next frame AND its slice weights;
the drop-in for the reference's top-level SequenSolverMerged.py (class SequenSolver), the variant its newest training
loop runs (`SequenSolver(..., layers=8, sequential_head=16)`).

  1. the last T frames go through the frozen encoder: each frame becomes one token of width dim = M*C;
  2. a sinusoidal positional encoding is added to the tokens (forward only: `get_code` does not add it, as in the reference);
  3. `layers` weight-tied pre-LN blocks: tokens += attention(ln_1 tokens), tokens += mlp(ln_2 tokens).  The attention is
     causal and split into `sequential_head` groups: the [T, dim] LayerNorm output of a sample is reshaped AS CONTIGUOUS
     MEMORY to [sequential_head, T, seq_dim], so group g holds the pseudo-rows g*T .. g*T+T-1 of seq_dim floats, pseudo-row
     p being chunk p % sequential_head of real token p // sequential_head; one bias-free Linear(seq_dim, seq_dim) each
     for q, k, v is shared by all groups, and scale = dim ** -0.5 (the whole token width).  One launch of
     pa2d_head_seq_attn_* per call where seq_dim <= 64, else three linears and the causal pa2d_seq_attn_*
     (functional.head_seq_attention);
  4. the last token is the code [B, 1, M, C];
  5. the slice weights are always predicted: `forward_slice(spatial_pos, fx, code)`, the code-conditioned conv predictor
     that SliceLearner.VorticitySliceLearner runs (one implementation: SliceLearner.code_conditioned_slice_weights) over
     this module's own `preprocess`, `in_project_x`, `in_project_slice` and `temperature`.  use_gt=True only encodes y as
     well, which leaves the encoder's cached slice weights as y's; its own result is overwritten, as in the reference;
  6. output = mlp2(ln_3(einsum("bhgc,bhng->bhnc", code, slice_weights))).

The constructor keeps the reference's names, order and defaults; `encoder_config` (keyword-only) is the one extension, as
in SequenSolver.py.  The state_dict has the reference's keys and shapes as saved on a GPU: `temperature` stays 0.5 (there
`nn.Parameter(...).cuda()` is a plain tensor, in no state_dict and no optimizer; here a non-persistent buffer), and the
causal mask is a kernel argument, not a tensor.  The reference hard-codes 64 + T = 74 point features; here it is 64 + T.
The reference reshapes with the constructor's B; here the actual batch is used.  Every arithmetic step goes through
functional.py; torch only slices, reshapes, owns memory and adds the constant positional table to the frozen encoder's
tokens."""
import os

import torch
import torch.nn as nn

from . import functional as Fn
from . import ops
from .SequenSolver import REFERENCE_ENCODER, encode_table, fold_calls
from .SliceLearner import code_conditioned_slice_weights
from .model import Transolver_Structured_Mesh2D_Encoder
from .model._core import ACTIVATION, MLP  # noqa: F401  (the reference module defines both names)

SLICE_HIDDEN = 256          # n_hidden of the slice predictor (hard-coded in the reference)
SLICE_POS_FEATURES = 64     # ref * ref unified_pos distances per point


def positional_table(num_tokens, embed_dim):
    """pe [num_tokens, embed_dim] in fp32 on the host, written as the reference's add_positional_encoding writes it."""
    pos = torch.arange(num_tokens, dtype=torch.float).unsqueeze(1)
    div_term = 10000 ** (torch.arange(0, embed_dim, 2).float() / embed_dim)
    pe = torch.zeros(num_tokens, embed_dim)
    pe[:, 0::2] = torch.sin(pos / div_term)
    pe[:, 1::2] = torch.cos(pos / div_term)
    return pe


class SequenSolver(nn.Module):

    def __init__(self, transolver_path, T, W, H, M, C, B, sequential_head=1, mlp_ratio=4, layers=5, act='gelu', dropout=0.,
                 *, encoder_config=None):
        super().__init__()
        self.T, self.W, self.H, self.M, self.C = T, W, H, M, C
        self.N = H * W
        self.B = B
        self.dim = M * C
        self.scale = self.dim ** -0.5
        self.Head = 1
        self.layers = layers
        self.sequential_head = sequential_head
        self.engine = None
        self.fused = None                 # None: the fused head attention where it serves seq_dim; False: the unfused route
        self.batched_encoding = True      # the T (+1) frames of a call go through the encoder as ONE batch

        if sequential_head < 1 or self.dim % sequential_head:
            raise ValueError(f"sequential_head = {sequential_head} must divide dim = M*C = {self.dim}")
        self.seq_dim = self.dim // sequential_head
        if self.seq_dim % 4:
            raise NotImplementedError(f"seq_dim = dim // sequential_head = {self.seq_dim}: the attention kernels serve "
                                      "seq_dim % 4 == 0")
        if not 1 <= T <= ops.HEAD_SEQ_ATTN_MAX_T:
            raise NotImplementedError(f"the sequence attention kernels serve 1 <= T <= {ops.HEAD_SEQ_ATTN_MAX_T}; got T = {T}")
        if self.dim > ops.SEQ_ATTN_MAX_DIM or self.dim % 4:
            raise NotImplementedError(f"dim = M*C = {self.dim}: LayerNorm and the sequence attention kernel serve "
                                      f"dim % 4 == 0 up to {ops.SEQ_ATTN_MAX_DIM}")
        cfg = dict(REFERENCE_ENCODER if encoder_config is None else encoder_config)
        self.encoder = Transolver_Structured_Mesh2D_Encoder.Model(**cfg)
        enc_h, enc_w, enc_m = self.encoder.H, self.encoder.W, self.encoder.blocks[-1].Attn.in_project_slice.out_features
        enc_heads, enc_c = self.encoder.blocks[-1].Attn.heads, self.encoder.blocks[-1].Attn.dim_head
        if (enc_h, enc_w) != (H, W):
            raise ValueError(f"H x W = {H} x {W} does not match the encoder's mesh {enc_h} x {enc_w}")
        if enc_heads != self.Head:
            raise ValueError(f"the encoder has {enc_heads} heads; SequenSolver reads its code as one head of M x C")
        if (enc_m, enc_c) != (M, C):
            raise ValueError(f"M x C = {M} x {C} does not match the encoder's code {enc_m} slices x {enc_c} channels")
        if transolver_path is not None:
            sd = transolver_path
            if isinstance(sd, (str, os.PathLike)):
                sd = torch.load(sd, weights_only=True, map_location="cpu")
            self.encoder.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
        self.encoder.eval()
        for param in self.encoder.parameters():
            param.requires_grad = False

        self.to_q = nn.Linear(self.seq_dim, self.seq_dim, bias=False)
        self.to_k = nn.Linear(self.seq_dim, self.seq_dim, bias=False)
        self.to_v = nn.Linear(self.seq_dim, self.seq_dim, bias=False)
        self.softmax_attention = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)

        # non-persistent buffers: they follow .cuda() / .to() and stay out of the state_dict, like the reference's plain
        # tensor attributes (its `temperature` is one of them on a GPU: nn.Parameter(...).cuda())
        self.register_buffer("slice_weights", torch.zeros(B, 1, self.N, self.M), persistent=False)
        self.register_buffer("pe", positional_table(T, self.dim), persistent=False)
        self.slice_weights_t = 0
        self.code = None

        self.ln_1 = nn.LayerNorm(self.dim)
        self.ln_2 = nn.LayerNorm(self.dim)
        self.mlp = MLP(self.dim, self.dim * mlp_ratio, self.dim, n_layers=0, res=False, act=act)

        self.fundemental = SLICE_POS_FEATURES + T                        # the reference hard-codes 74 = 64 + 10
        self.preprocess = MLP(self.fundemental, SLICE_HIDDEN * 2, SLICE_HIDDEN, n_layers=0, res=False, act=act)
        self.in_project_x = nn.Conv2d(SLICE_HIDDEN, SLICE_HIDDEN, 3, 1, 1)
        self.softmax_vort = nn.Softmax(dim=-1)
        self.concatenated = SLICE_HIDDEN + self.dim
        self.in_project_slice = MLP(self.concatenated, self.concatenated // 2, self.M)
        self.register_buffer("temperature", torch.ones([1, 1, 1, 1]) * 0.5, persistent=False)

        self.ln_3 = nn.LayerNorm(self.C)
        self.mlp2 = nn.Linear(self.C, 1)

    # ---- engine
    def set_fused_tail(self, flag=True):
        """Accepted for interface parity with the Transolver models (harness.rollout(fused_tail=...)); this model has no
        block tail of that shape, so the flag has no effect."""
        self.fused_tail = bool(flag)
        return self

    def set_engine(self, engine):
        """GEMM engine of the encoder and of this model's dense layers and conv ("f32" | "split" | "bf16" | None =
        default); bf16 storage ('bf16s') is refused.  The attention, z-score and slice-weight stages are exact fp32 on
        every engine."""
        self.encoder.set_engine(engine)          # refuses 'bf16s'
        self.engine = None if engine is None else ops.resolve_engine(engine)
        for m in (self.mlp, self.preprocess, self.in_project_slice):
            m.engine = self.engine
        return self

    def train(self, mode=True):
        super().train(mode)
        self.encoder.eval()                      # the encoder is frozen and stays in eval()
        return self

    def _refuse(self, what="the merged SequenSolver"):
        if ops.resolve_engine(self.engine) == ops.ENGINE_BF16S:
            raise NotImplementedError(f"bf16 storage (engine 'bf16s') is not implemented for {what}")
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("dropout > 0 is not implemented in the HIP path; refusing to ignore it")

    # ---- encoding
    def _encode_frames(self, spatial_pos, frames):
        """frames: list of [B, N, 1] -> (tokens [B, Head, len(frames), dim], slice weights of the LAST frame [B, 1, N, M]).
        The encoder's cached slice weights are left as the last frame's, as a frame-by-frame loop leaves them."""
        B = frames[0].shape[0]
        with torch.no_grad():
            if self.batched_encoding and len(frames) > 1:
                n = len(frames)
                code = self.encoder.encode(spatial_pos.repeat(n, *([1] * (spatial_pos.dim() - 1))), torch.cat(frames, 0))
                sw = self.encoder.get_attention_slice()[-B:].contiguous()
                self.encoder.set_attention_slice(sw)
                tokens = code.reshape(n, B, self.Head, self.dim).permute(1, 2, 0, 3).contiguous()
            else:
                codes = [self.encoder.encode(spatial_pos, f).reshape(B, self.Head, 1, self.dim) for f in frames]
                sw = self.encoder.get_attention_slice()
                tokens = torch.cat(codes, 2)
        return tokens, sw

    def _blocks(self, tokens):
        mlp = self.mlp
        pre, post = mlp.linear_pre[0], mlp.linear_post
        for _ in range(self.layers):
            tokens = self.attention(Fn.layer_norm(tokens, self.ln_1.weight, self.ln_1.bias), residual=tokens)
            tokens = Fn.mlp_branch(tokens, self.ln_2.weight, self.ln_2.bias, mlp.act_name, pre.weight, pre.bias,
                                   post.weight, post.bias, engine=self.engine)
        return tokens

    def _code(self, tokens):
        B = tokens.shape[0]
        return tokens[:, :, -1:, ].reshape(B, self.Head, self.M, self.C).contiguous()

    def forward(self, spatial_pos, fx, y, use_gt=True):
        """spatial_pos [B, N, 64] the unified_pos distances, fx [B, N, T] the last T frames, y [B, N, 1] the next frame
        (encoded with use_gt=True only; the decoding slice weights are always the predicted ones) -> [B, N, 1]."""
        self._refuse()
        frames = [fx[:, :, i:i + 1] for i in range(self.T)]
        if use_gt:      # y last, so that the encoder's cached slice weights are y's; the result is overwritten below
            tokens, sw = self._encode_frames(spatial_pos, frames + [y])
            tokens = tokens[:, :, :self.T].contiguous()
            self.slice_weights = sw
        else:
            tokens, _ = self._encode_frames(spatial_pos, frames)
        with torch.no_grad():       # the tokens come from the frozen encoder
            tokens = self.add_positional_encoding(tokens)
        tokens = self._blocks(tokens)
        code = self._code(tokens)
        self.code = code
        self.slice_weights = self.forward_slice(spatial_pos, fx, code)
        decoded = self.decode(code)
        return Fn.head(Fn.layer_norm(decoded, self.ln_3.weight, self.ln_3.bias), self.mlp2.weight, self.mlp2.bias)

    def forward_windows(self, spatial_pos, seq, use_gt=True):
        """The n = seq.shape[-1] - T teacher-forced calls of a training iteration in folded batches: seq [B, N, T + n] holds
        TRUE frames, and column k of the result [B, N, n] is what forward(spatial_pos, seq[..., k:k+T],
        seq[..., k+T:k+T+1], use_gt) returns.  Every frame is encoded ONCE (use_gt=True: all T + n, so that the encoder's
        cached slice weights end as the last target's; else T + n - 1); call k's tokens are frames k .. k+T-1 of that
        table plus the positional table; the blocks run on n*B sequences and forward_slice on n*B windows with one set of
        z-score statistics per call (groups = n).  `code`, `slice_weights` and the encoder's cached slice weights are left
        as the last call's.  n is cut into several folded calls where a folded tensor would pass the 4 GiB extent."""
        self._refuse()
        B, T = seq.shape[0], self.T
        n = seq.shape[-1] - T
        if n < 1:
            raise ValueError(f"forward_windows needs seq [B, N, T + n] with n >= 1; got {tuple(seq.shape)} at T = {T}")
        nframes = T + n if use_gt else T + n - 1
        tokens = encode_table(self, spatial_pos, seq, nframes)                         # [B, Head, nframes, dim]
        ratio = self.mlp.linear_pre[0].weight.shape[0] / self.dim
        group = fold_calls(n, B, self.N, T, max(2 * SLICE_HIDDEN, self.concatenated // 2), int(ratio * self.dim))
        outs = []
        for k0 in range(0, n, group):
            g = min(group, n - k0)
            with torch.no_grad():       # the tokens come from the frozen encoder
                win = torch.cat([tokens[:, :, k:k + T] for k in range(k0, k0 + g)], 0)   # [g*B, Head, T, dim], call-major
                win = self.add_positional_encoding(win)
                fxw = torch.cat([seq[..., k:k + T] for k in range(k0, k0 + g)], 0)       # [g*B, N, T]
                pos = spatial_pos.repeat(g, *([1] * (spatial_pos.dim() - 1)))
            code = self._code(self._blocks(win))
            sw = self.forward_slice(pos, fxw, code, groups=g)
            decoded = Fn.deslice_weights(code, sw)
            out = Fn.head(Fn.layer_norm(decoded, self.ln_3.weight, self.ln_3.bias), self.mlp2.weight, self.mlp2.bias)
            outs.append(out.reshape(g, B, self.N))
        self.code, self.slice_weights = code[-B:], sw[-B:]
        out = outs[0] if len(outs) == 1 else torch.cat(outs, 0)
        return out.permute(1, 2, 0)

    def forward_slice(self, x, fx, code, groups=1):
        """x [B, N, 64], fx [B, N, T], code [B, 1, M, C] -> slice weights [B, 1, N, M].  `groups` > 1: the batch is that
        many folded calls of B / groups samples, each z-scored on its own (SliceLearner.code_conditioned_slice_weights)."""
        self._refuse()
        if fx is None:
            raise ValueError("forward_slice needs fx: the reference's fx=None path reads a placeholder it never creates")
        if x.shape[-1] + fx.shape[-1] != self.fundemental:
            raise ValueError(f"forward_slice takes {SLICE_POS_FEATURES} positional features and T = {self.T} frames per "
                             f"point; got {x.shape[-1]} and {fx.shape[-1]}")
        folded = {} if groups == 1 else dict(groups=groups)      # an unfolded call is made exactly as it always was
        return code_conditioned_slice_weights(x, fx, code, self.preprocess, self.in_project_x, self.in_project_slice,
                                              self.temperature, self.H, self.W, self.M, self.C, self.engine, **folded)

    def get_code(self, spatial_pos, fx, y):
        """The code without the positional encoding, as the reference's get_code."""
        self._refuse()
        tokens, _ = self._encode_frames(spatial_pos, [fx[:, :, i:i + 1] for i in range(self.T)])
        return self._code(self._blocks(tokens))

    def get_last_slice_weight(self, spatial_pos, fx):
        with torch.no_grad():
            self.encoder.encode(spatial_pos, fx[:, :, -1:])
        return self.encoder.get_attention_slice()

    def add_positional_encoding(self, tokens):
        """tokens [B, Head, T, dim] + the fp32 sinusoidal table (the same fp32 values whatever the tokens' dtype)."""
        n, d = tokens.shape[-2:]
        pe = self.pe if tuple(self.pe.shape) == (n, d) else positional_table(n, d).to(tokens.device)
        return tokens + pe

    def attention(self, tokens, residual=None):
        """Causal head attention among the T tokens: tokens [B, Head, T, dim] -> the same shape.  `residual` (extension):
        added in the kernel's epilogue (the blocks use it)."""
        self._refuse()
        shp = tokens.shape
        flat = (-1, shp[-2], shp[-1])
        res = None if residual is None else residual.reshape(flat)
        out = Fn.head_seq_attention(tokens.reshape(flat), self.to_q.weight, self.to_k.weight, self.to_v.weight,
                                    self.sequential_head, self.scale, res=res, causal=True, engine=self.engine,
                                    fused=self.fused)
        return out.reshape(shp)

    def decode(self, code):
        return Fn.deslice_weights(code, self.slice_weights)

    def z_score_normalization(self, x):
        return Fn.zscore(x)

    def freeze_attention(self):
        frozen = (self.to_q, self.to_k, self.to_v, self.mlp, self.ln_1, self.ln_2)
        for m in frozen + (self.softmax_attention,):
            m.eval()
        for m in frozen:
            for param in m.parameters():
                param.requires_grad = False
