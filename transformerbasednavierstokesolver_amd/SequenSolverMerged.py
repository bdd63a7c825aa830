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
import torch
import torch.nn as nn

from . import functional as Fn
from . import ops
from .SequenSolver import _LatentSequence, encode_table
from .SliceLearner import code_conditioned_slice_weights
from .folding import fold_calls, groups, joined, windows
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


class SequenSolver(_LatentSequence):
    WHAT = "the merged SequenSolver"
    ENGINE_MODULES = ("mlp", "preprocess", "in_project_slice")

    def __init__(self, transolver_path, T, W, H, M, C, B, sequential_head=1, mlp_ratio=4, layers=5, act='gelu', dropout=0.,
                 *, encoder_config=None):
        super().__init__()
        self._set_geometry(T, W, H, M, C, B, layers)
        self.sequential_head = sequential_head
        self.fused = None                 # None: the fused head attention where it serves seq_dim; False: the unfused route
        if sequential_head < 1 or self.dim % sequential_head:
            raise ValueError(f"sequential_head = {sequential_head} must divide dim = M*C = {self.dim}")
        self.seq_dim = self.dim // sequential_head
        if self.seq_dim % 4:
            raise NotImplementedError(f"seq_dim = dim // sequential_head = {self.seq_dim}: the attention kernels serve "
                                      "seq_dim % 4 == 0")
        if not 1 <= T <= ops.HEAD_SEQ_ATTN_MAX_T:
            raise NotImplementedError(f"the sequence attention kernels serve 1 <= T <= {ops.HEAD_SEQ_ATTN_MAX_T}; got T = {T}")
        self._refuse_dim()
        self._build_encoder(encoder_config)
        self._build_attention(transolver_path, self.seq_dim, dropout)
        # non-persistent, like `slice_weights`: the reference's plain tensor attributes (its `temperature` is one of them
        # on a GPU: nn.Parameter(...).cuda())
        self.register_buffer("pe", positional_table(T, self.dim), persistent=False)
        self._build_blocks(mlp_ratio, act)

        self.fundemental = SLICE_POS_FEATURES + T                        # the reference hard-codes 74 = 64 + 10
        self.preprocess = MLP(self.fundemental, SLICE_HIDDEN * 2, SLICE_HIDDEN, n_layers=0, res=False, act=act)
        self.in_project_x = nn.Conv2d(SLICE_HIDDEN, SLICE_HIDDEN, 3, 1, 1)
        self.softmax_vort = nn.Softmax(dim=-1)
        self.concatenated = SLICE_HIDDEN + self.dim
        self.in_project_slice = MLP(self.concatenated, self.concatenated // 2, self.M)
        self.register_buffer("temperature", torch.ones([1, 1, 1, 1]) * 0.5, persistent=False)
        self._build_readout()

    def forward(self, spatial_pos, fx, y, use_gt=True):
        """spatial_pos [B, N, 64] the unified_pos distances, fx [B, N, T] the last T frames, y [B, N, 1] the next frame
        (encoded with use_gt=True only; the decoding slice weights are always the predicted ones) -> [B, N, 1]."""
        self._refuse()
        # use_gt: y is encoded last, so that the encoder's cached slice weights are y's; they are not used here
        tokens, _ = self._encode_window(spatial_pos, fx, y if use_gt else None)
        with torch.no_grad():       # the tokens come from the frozen encoder
            tokens = self.add_positional_encoding(tokens)
        self.code = code = self._code(self._blocks(tokens))
        self.slice_weights = self.forward_slice(spatial_pos, fx, code)
        return self.readout(code, self.slice_weights)

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
        n = self._window_count(seq, "forward_windows")
        nframes = T + n if use_gt else T + n - 1
        tokens = encode_table(self, spatial_pos, seq, nframes)                         # [B, Head, nframes, dim]
        group = fold_calls(n, B, self.N, T, max(2 * SLICE_HIDDEN, self.concatenated // 2), self._token_width())
        outs = []
        for k0, g in groups(n, group):
            with torch.no_grad():       # the tokens come from the frozen encoder
                win = self.add_positional_encoding(windows(tokens, k0, g, T, 2))         # [g*B, Head, T, dim], call-major
                fxw = windows(seq, k0, g, T)                                             # [g*B, N, T]
                pos = spatial_pos.repeat(g, *([1] * (spatial_pos.dim() - 1)))
            code = self._code(self._blocks(win))
            sw = self.forward_slice(pos, fxw, code, groups=g)
            outs.append(self.readout(code, sw).reshape(g, B, self.N))
        self.code, self.slice_weights = code[-B:], sw[-B:]
        return joined(outs).permute(1, 2, 0)

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
        return super().get_code(spatial_pos, fx, y)

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

    def z_score_normalization(self, x):
        return Fn.zscore(x)
