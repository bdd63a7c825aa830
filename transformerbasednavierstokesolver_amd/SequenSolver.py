"""SequenSolver — the latent sequence model over the codes of the frozen structured 2-D auto-encoder; the drop-in for the
reference's top-level SequenSolver.py (class SequenSolver, :45-388).

  1. the last T frames go through the frozen encoder: each frame becomes one token of width dim = M*C;
  2. `layers` weight-tied pre-LN blocks run over the T tokens: tokens += attention(ln_1 tokens) (single-head attention
     among the T tokens, pa2d_seq_attn_*), tokens += mlp(ln_2 tokens) (dim -> mlp_ratio*dim -> dim);
  3. the last token is the code [B, 1, M, C] of the next frame;
  4. the code is de-sliced with slice weights [B, 1, N, M]: with use_gt=True the encoder's weights of the true next frame,
     with use_gt=False predicted from the code and the point coordinates by `weight_projection` and a softmax over M
     (pa2d_code_slice_weights_*, the P = 2 case of LearnSlice's stage: the reference's loop over the N points and its
     [B, N, M, C+2] tensor do not exist here);
  5. output = mlp2(ln_3(.)).

The constructor keeps the reference's names, order and defaults; `encoder_config` (keyword-only) is the one extension: the
reference hard-codes its encoder (8 layers, n_hidden=32, 1 head, 16 slices, 64 x 64, unified_pos=1, fun_dim=1), which stays
the default.  The state_dict has the reference's keys and shapes: `slice_projection` and `temporal_slice_projection` are
created and never used (no gradient), `token_to_slice_list` (a plain list of N unused layers, not in the state_dict) is
not built.  Every arithmetic step goes through functional.py; torch only slices, reshapes and owns memory.
`solve_with_slice_learner` runs the default mode of the reference's (a trained LearnSlice.get_slice_weight on the code) without
its prints and plots."""
import os

import torch
import torch.nn as nn

from . import functional as Fn
from . import ops
from .LearnSlice import LearnSlice
from .folding import _fold_group, fold_calls, groups, joined, windows
from .model import Transolver_Structured_Mesh2D_Encoder
from .model._core import ACTIVATION, MLP  # noqa: F401  (the reference module defines both names)

REFERENCE_ENCODER = dict(space_dim=2, n_layers=8, n_hidden=32, dropout=0.0, n_head=1, slice_num=16, Time_Input=False,
                         fun_dim=1, out_dim=1, unified_pos=1, H=64, W=64)
WEIGHT_PROJECTION_HIDDEN = 64


def load_frozen(source, build, *, strict, device=None, freeze=True):
    """A checkpoint into a module that is then left in eval() with (`freeze`) no trainable parameter.  `source`: a
    checkpoint file, a state_dict, None (nothing is loaded) or a module, which is returned untouched: the caller's own.
    `build()` gives the module to load into; `device`: where it is moved after loading."""
    if isinstance(source, nn.Module):
        return source
    module = build()
    if source is not None:
        if isinstance(source, (str, os.PathLike)):
            source = torch.load(source, weights_only=True, map_location="cpu")
        module.load_state_dict({k: torch.as_tensor(v) for k, v in source.items()}, strict=strict)
    if device is not None:
        module = module.to(device)
    module.eval()
    if freeze:
        for param in module.parameters():
            param.requires_grad = False
    return module


def encode_table(model, spatial_pos, seq, nframes, want_slices=False):
    """The first `nframes` frames of seq [B, N, >= nframes] through the frozen encoder ONCE, as one frame-major batch (cut
    only where a folded encoder tensor would pass the 4 GiB extent): tokens [B, Head, nframes, dim] and, with
    `want_slices`, every frame's slice weights [nframes*B, 1, N, M] in frame-major order.  The encoder's cached slice
    weights are left as the last frame's [B, 1, N, M], as a frame-by-frame loop leaves them."""
    B, N = seq.shape[0], seq.shape[1]
    with torch.no_grad():
        frames = seq[..., :nframes].permute(2, 0, 1).reshape(nframes * B, N, 1)
        codes, slices = [], []
        for f0, f in groups(nframes, _fold_group(model.encoder, B, N, nframes)):
            pos = spatial_pos.repeat(f, *([1] * (spatial_pos.dim() - 1)))
            code = model.encoder.encode(pos, frames[f0 * B:(f0 + f) * B])
            codes.append(code.reshape(f, B, model.Head, model.dim))
            sw = model.encoder.get_attention_slice()
            if want_slices:
                slices.append(sw)
        model.encoder.set_attention_slice(sw[-B:].contiguous())
        tokens = joined(codes).permute(1, 2, 0, 3).contiguous()
    if not want_slices:
        return tokens
    return tokens, joined(slices)


class _LatentSequence(nn.Module):
    """What SequenSolver.SequenSolver and SequenSolverMerged.SequenSolver share.  Registration order is behaviour (the
    state_dict's key order, the parameter order of an optimizer's bucket, the order construction draws from the RNG) and
    the two interleave shared and own members differently, so a constructor calls the `_build_*` steps in its own order."""
    WHAT = None                # _refuse's default subject
    ENGINE_MODULES = ()        # the dense sub-modules that carry an `engine`

    def _set_geometry(self, T, W, H, M, C, B, layers):
        self.T, self.W, self.H, self.M, self.C = T, W, H, M, C
        self.N = H * W
        self.B = B
        self.dim = M * C
        self.scale = self.dim ** -0.5
        self.Head = 1
        self.layers = layers
        self.engine = None
        self.batched_encoding = True      # the T (+1) frames of a call go through the encoder as ONE batch

    def _build_encoder(self, encoder_config):
        cfg = dict(REFERENCE_ENCODER if encoder_config is None else encoder_config)
        self.encoder = Transolver_Structured_Mesh2D_Encoder.Model(**cfg)
        H, W, M, C = self.H, self.W, self.M, self.C
        enc_h, enc_w, enc_m = self.encoder.H, self.encoder.W, self.encoder.blocks[-1].Attn.in_project_slice.out_features
        enc_heads, enc_c = self.encoder.blocks[-1].Attn.heads, self.encoder.blocks[-1].Attn.dim_head
        if (enc_h, enc_w) != (H, W):
            raise ValueError(f"H x W = {H} x {W} does not match the encoder's mesh {enc_h} x {enc_w}")
        if enc_heads != self.Head:
            raise ValueError(f"the encoder has {enc_heads} heads; SequenSolver reads its code as one head of M x C")
        if (enc_m, enc_c) != (M, C):
            raise ValueError(f"M x C = {M} x {C} does not match the encoder's code {enc_m} slices x {enc_c} channels")

    def _refuse_dim(self):
        if self.dim > ops.SEQ_ATTN_MAX_DIM or self.dim % 4:
            raise NotImplementedError(f"dim = M*C = {self.dim}: LayerNorm and the sequence attention kernel serve "
                                      f"dim % 4 == 0 up to {ops.SEQ_ATTN_MAX_DIM}")

    def _build_attention(self, transolver_path, width, dropout):
        """The encoder's checkpoint, loaded and frozen; q / k / v of `width`; the non-persistent `slice_weights` buffer,
        which follows .cuda() / .to() and stays out of the state_dict, like the reference's plain tensor attribute."""
        load_frozen(transolver_path, lambda: self.encoder, strict=False)
        self.to_q = nn.Linear(width, width, bias=False)
        self.to_k = nn.Linear(width, width, bias=False)
        self.to_v = nn.Linear(width, width, bias=False)
        self.softmax_attention = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.register_buffer("slice_weights", torch.zeros(self.B, 1, self.N, self.M), persistent=False)
        self.slice_weights_t = 0
        self.code = None

    def _build_blocks(self, mlp_ratio, act):
        self.ln_1 = nn.LayerNorm(self.dim)
        self.ln_2 = nn.LayerNorm(self.dim)
        self.mlp = MLP(self.dim, self.dim * mlp_ratio, self.dim, n_layers=0, res=False, act=act)

    def _build_readout(self):
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
        default); bf16 storage ('bf16s') is refused, as for the encoder family.  The attention, z-score and slice-weight
        stages are exact fp32 on every engine."""
        self.encoder.set_engine(engine)          # refuses 'bf16s'
        self.engine = None if engine is None else ops.resolve_engine(engine)
        for name in self.ENGINE_MODULES:
            getattr(self, name).engine = self.engine
        return self

    def train(self, mode=True):
        super().train(mode)
        self.encoder.eval()                      # the encoder is frozen and stays in eval()
        return self

    def _refuse(self, what=None):
        if ops.resolve_engine(self.engine) == ops.ENGINE_BF16S:
            raise NotImplementedError(f"bf16 storage (engine 'bf16s') is not implemented for {what or self.WHAT}")
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

    def _encode_window(self, spatial_pos, fx, y=None):
        """The T frames of fx [B, N, T] -> (tokens [B, Head, T, dim], slice weights of the last frame encoded).  With y
        [B, N, 1] the target is encoded with them, last, so that the encoder's cached slice weights (and the ones
        returned) are y's."""
        frames = [fx[:, :, i:i + 1] for i in range(self.T)]
        if y is None:
            return self._encode_frames(spatial_pos, frames)
        tokens, sw = self._encode_frames(spatial_pos, frames + [y])
        return tokens[:, :, :self.T].contiguous(), sw

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

    def _window_count(self, seq, who):
        n = seq.shape[-1] - self.T
        if n < 1:
            raise ValueError(f"{who} needs seq [B, N, T + n] with n >= 1; got {tuple(seq.shape)} at T = {self.T}")
        return n

    def _token_width(self):
        """The widest per-token row of the blocks: the MLP's hidden layer."""
        return int(self.mlp.linear_pre[0].weight.shape[0] / self.dim * self.dim)

    def get_code(self, spatial_pos, fx, y):
        self._refuse()
        tokens, _ = self._encode_window(spatial_pos, fx)
        return self._code(self._blocks(tokens))

    def get_last_slice_weight(self, spatial_pos, fx):
        with torch.no_grad():
            self.encoder.encode(spatial_pos, fx[:, :, -1:])
        return self.encoder.get_attention_slice()

    def decode(self, code):
        return Fn.deslice_weights(code, self.slice_weights)

    def readout(self, code, slice_weights):
        """mlp2(ln_3(code de-sliced with slice_weights)): code [B, 1, M, C], slice_weights [B, 1, N, M] -> [B, N, 1]."""
        decoded = Fn.deslice_weights(code, slice_weights)
        return Fn.head(Fn.layer_norm(decoded, self.ln_3.weight, self.ln_3.bias), self.mlp2.weight, self.mlp2.bias)

    def freeze_attention(self):
        frozen = (self.to_q, self.to_k, self.to_v, self.mlp, self.ln_1, self.ln_2)
        for m in frozen + (self.softmax_attention,):
            m.eval()
        for m in frozen:
            for param in m.parameters():
                param.requires_grad = False


class SequenSolver(_LatentSequence):
    WHAT = "SequenSolver"
    ENGINE_MODULES = ("mlp", "weight_projection", "temporal_slice_projection")

    def __init__(self, transolver_path, T, W, H, M, C, B, mlp_ratio=4, layers=5, act='gelu', dropout=0., *,
                 encoder_config=None):
        super().__init__()
        self._set_geometry(T, W, H, M, C, B, layers)
        self._build_encoder(encoder_config)
        if not 1 <= T <= ops.SEQ_ATTN_MAX_T:
            raise NotImplementedError(f"the sequence attention kernel serves 1 <= T <= {ops.SEQ_ATTN_MAX_T}; got T = {T}")
        self._refuse_dim()
        self._build_attention(transolver_path, self.dim, dropout)
        self.slice_projection = nn.Linear(self.M, self.M)                           # never used (reference :93)
        self.temporal_slice_projection = MLP(self.T, self.T * mlp_ratio, 1)         # never used (reference :95)
        self.learned_slice_weights = None      # what solve_with_slice_learner's LearnSlice predicted last
        self.weight_projection = MLP(self.C + 2, WEIGHT_PROJECTION_HIDDEN, 1)
        self.softmax_slice = nn.Softmax(dim=-1)
        self._build_blocks(mlp_ratio, act)
        self._build_readout()

    def forward(self, spatial_pos, fx, y, use_gt=True):
        """spatial_pos [B, N, 2] point coordinates, fx [B, N, T] the last T frames, y [B, N, 1] the next frame (read with
        use_gt=True only) -> [B, N, 1]."""
        self._refuse()
        # use_gt: the target's slice weights, encoded with the T frames, last, so that they are the cached ones
        tokens, sw = self._encode_window(spatial_pos, fx, y if use_gt else None)
        self.code = code = self._code(self._blocks(tokens))
        self.slice_weights = sw if use_gt else self._predicted_slice_weights(code, spatial_pos)
        return self.readout(code, self.slice_weights)

    def _predicted_slice_weights(self, code, spatial_pos):
        if spatial_pos.dim() != 3 or spatial_pos.shape[-1] != 2:
            raise ValueError("use_gt=False predicts the slice weights from the two point coordinates: spatial_pos "
                             f"must be [B, N, 2]; got {tuple(spatial_pos.shape)}")
        wp = self.weight_projection
        return Fn.code_slice_weights(code.reshape(code.shape[0], self.M, self.C), spatial_pos,
                                     wp.linear_pre[0].weight, wp.linear_pre[0].bias,
                                     wp.linears[0][0].weight, wp.linears[0][0].bias,
                                     wp.linear_post.weight, wp.linear_post.bias)

    def forward_windows(self, spatial_pos, seq, use_gt=True):
        """The n = seq.shape[-1] - T teacher-forced calls of a training iteration in folded batches: seq [B, N, T + n] holds
        TRUE frames, and column k of the result [B, N, n] is what forward(spatial_pos, seq[..., k:k+T],
        seq[..., k+T:k+T+1], use_gt) returns.  Every frame is encoded ONCE (use_gt=True: all T + n, and call k decodes
        with the cached slice weights of frame T + k, a contiguous block of the encoder's output; else T + n - 1 and the
        code -> slice-weight stage on the folded batch); call k's tokens are frames k .. k+T-1 of that table and the blocks
        run on n*B sequences.  `code`, `slice_weights` and the encoder's cached slice weights are left as the last call's.
        n is cut into several folded calls where a folded tensor would pass the 4 GiB extent.  This model has no conv
        slice predictor (the merged model's 512-float hidden layer): its widest per-point rows are the slice weights (M),
        the point features (C + 2) and weight_projection's hidden layer, its widest per-token row the blocks' mlp_ratio*dim."""
        self._refuse()
        B, T = seq.shape[0], self.T
        n = self._window_count(seq, "forward_windows")
        if use_gt:
            tokens, slices = encode_table(self, spatial_pos, seq, T + n, want_slices=True)
        else:
            tokens = encode_table(self, spatial_pos, seq, T + n - 1)
        outs = []
        for k0, g in groups(n, self._calls_per_fold(n, B)):
            code = self._code(self._blocks(windows(tokens, k0, g, T, 2)))               # on [g*B, Head, T, dim], call-major
            if use_gt:
                sw = slices[(T + k0) * B:(T + k0 + g) * B]
            else:
                sw = self._predicted_slice_weights(code, spatial_pos.repeat(g, 1, 1))
            outs.append(self.readout(code, sw).reshape(g, B, self.N))
        self.code, self.slice_weights = code[-B:], sw[-B:]
        return joined(outs).permute(1, 2, 0)

    def _calls_per_fold(self, n, B):
        return fold_calls(n, B, self.N, self.T, max(self.M, self.C + 2, WEIGHT_PROJECTION_HIDDEN), self._token_width())

    def code_windows(self, spatial_pos, seq):
        """Everything the slice trainers take from this frozen model for the n = seq.shape[-1] - T teacher-forced calls of
        an iteration, computed ONCE: seq [B, N, T + n] holds TRUE frames.  One `encode_table(..., T + n, want_slices=True)`
        pass encodes every frame once, and the blocks run on the folded windows (cut by `fold_calls`, as
        `forward_windows`); all under no_grad and ops.weights_frozen().  Returns

          codes  [n, B, 1, M, C]   codes[k] is what get_code(spatial_pos, seq[..., k:k+T], .) returns;
          slices [(T + n) * B, 1, N, M]   the encoder's slice weights of every frame, frame-major: frame f is the block
                                   slices[f*B:(f+1)*B].

        Call k reads its code codes[k], its target (the slice weights of frame T + k) and its previous slice (frame
        T + k - 1: what get_last_slice_weight gives on window k).  The encoder's cached slice weights are left as the eager
        loops' last call leaves them (the last window's last frame, T + n - 2); `code` and `slice_weights`, which those
        loops never write, are not touched."""
        self._refuse()
        B, T = seq.shape[0], self.T
        n = self._window_count(seq, "code_windows")
        with torch.no_grad(), ops.weights_frozen():
            tokens, slices = encode_table(self, spatial_pos, seq, T + n, want_slices=True)
            codes = []
            for k0, g in groups(n, self._calls_per_fold(n, B)):
                code = self._code(self._blocks(windows(tokens, k0, g, T, 2)))           # on [g*B, Head, T, dim], call-major
                codes.append(code.reshape(g, B, self.Head, self.M, self.C))
            self.encoder.set_attention_slice(slices[(T + n - 2) * B:(T + n - 1) * B].contiguous())
        return joined(codes), slices

    def solve_with_slice_learner(self, slice_learner_path, spatial_pos, fx, y, unified_pos=0, use_vorticity=0,
                                 use_previous_slice=False, learn_from_vort=False, use_code_for_vorticity=False, *,
                                 decode_with_learned=False):
        """Reference SequenSolver.py:182-291 without its prints and plots: the code of the next frame, the slice weights
        that a trained LearnSlice predicts from it (kept in `learned_slice_weights` [B, 1, N, M]), and the output decoded
        with the encoder's weights of the true frame y (left in `slice_weights`), as the reference's line 239 does.
        `slice_learner_path`: a checkpoint file, a state_dict or a LearnSlice instance.  `decode_with_learned=True`
        (extension) decodes with the learned weights instead.  spatial_pos is what the slice learner was trained on
        ([B, N, 2], or [B, N, 64] with unified_pos); any B."""
        self._refuse("solve_with_slice_learner (SequenSolver and LearnSlice keep fp32 activations)")
        if use_previous_slice or learn_from_vort:
            raise NotImplementedError("solve_with_slice_learner serves the default mode (LearnSlice.get_slice_weight); "
                                      "use_previous_slice needs LearnSlice.forward_previous_slice and learn_from_vort "
                                      "LearnSlice.forward_from_vorticity, which are not built")
        # a module built here is frozen, as the reference's; the caller's own is left as it is
        learner = load_frozen(slice_learner_path, lambda: LearnSlice(
            unified_pos=unified_pos, use_vorticity=use_vorticity, use_code_for_vorticity=use_code_for_vorticity,
            C=self.C, M=self.M, T=self.T), strict=True, device=fx.device)
        tokens, sw_gt = self._encode_window(spatial_pos, fx, y)              # y last: its slice weights are the cached ones
        self.code = code = self._code(self._blocks(tokens))
        self.learned_slice_weights = learner.get_slice_weight(code, spatial_pos, fx, use_vorticity)
        self.slice_weights = self.learned_slice_weights if decode_with_learned else sw_gt
        return self.readout(code, self.slice_weights)

    def attention(self, tokens, residual=None):
        """Attention among the T tokens: tokens [B, Head, T, dim] -> the same shape.  `residual` (extension): added in
        the kernel's epilogue (the blocks use it)."""
        self._refuse()
        shp = tokens.shape
        q = Fn.linear(tokens, self.to_q.weight, None, None, engine=self.engine)
        k = Fn.linear(tokens, self.to_k.weight, None, None, engine=self.engine)
        v = Fn.linear(tokens, self.to_v.weight, None, None, engine=self.engine)
        flat = (-1, shp[-2], shp[-1])
        res = None if residual is None else residual.reshape(flat)
        return Fn.seq_attention(q.reshape(flat), k.reshape(flat), v.reshape(flat), self.scale, res=res).reshape(shp)
