"""Folding teacher-forced calls into one batch: how many calls fit (the 4 GiB extent of a buffer descriptor) and the loop
that cuts n calls into such groups.  Imports neither harness nor a model module; both read it."""
import torch

from . import ops

# widest per-row tensor any kernel addresses through a 32-bit buffer descriptor must stay below 4 GiB
FOLD_MAX_BYTES = 2 ** 32 - 4096


def model_engine(model):
    """The resolved GEMM engine id of a (possibly SOL-wrapped) Transolver."""
    inner = getattr(model, "transolver_model", model)
    return ops.resolve_engine(getattr(inner, "engine", None))


def _fold_group(model, bsz, npoints, ncalls):
    """How many teacher-forced calls fit in ONE folded model call: the widest activation row ([x_mid | fx_mid] =
    2C, the preprocess hidden 2C, or the MLP hidden r*C floats) times the folded row count must stay under the
    4 GiB extent of a buffer descriptor (libpa2d returns PA2D_ERR_UNSUPPORTED beyond it)."""
    inner = getattr(model, "transolver_model", model)
    C = inner.n_hidden
    r = max((blk.mlp.linear_pre[0].weight.shape[0] for blk in inner.blocks), default=C) / C
    width = int(max(2, r) * C)
    row_bytes = 4 * width
    eng = model_engine(model)
    if eng == ops.ENGINE_SPLIT:      # split engine: the 2C-wide conv gradient travels as 3 bf16 planes
        row_bytes = max(row_bytes, 6 * 2 * C)
    elif eng == ops.ENGINE_BF16S:    # bf16 storage: block activations are 2 bytes wide, the fp32 input embedding (2C) is not
        row_bytes = max(2 * width, 4 * 2 * C)
    rows = FOLD_MAX_BYTES // row_bytes
    return max(1, min(ncalls, rows // max(1, bsz * npoints)))


def fold_calls(ncalls, B, N, T, point_width, token_width):
    """How many teacher-forced calls fit in ONE folded call (the rule of _fold_group): the widest per-point tensor
    (`point_width` floats on calls*B*N rows) and the widest per-token tensor (`token_width` floats on calls*B*T rows) must
    stay under the 4 GiB extent of a buffer descriptor."""
    per_call = max(4 * point_width * B * N, 4 * token_width * B * T, 1)
    return max(1, min(ncalls, FOLD_MAX_BYTES // per_call))


def _slice_fold_group(model, ncalls, bsz, npoints):
    """How many calls of a slice predictor fit in ONE folded forward: its widest per-point row (the previous-slice
    predictor's 4 (M + M C) hidden layer; the conv predictors' preprocess hidden 2 n_hidden or first-layer input) times
    the folded row count stays under the 4 GiB extent of a buffer descriptor (fold_calls)."""
    if hasattr(model, "weight_projection_form_slice"):
        width = model.weight_projection_form_slice.n_hidden
    else:
        width = max(2 * model.n_hidden, getattr(model, "concatenated", model.n_hidden))
    return fold_calls(ncalls, bsz, npoints, 1, width, 1)


def groups(n, group):
    """(k0, g): calls k0 .. k0+g-1 of n, `group` at a time and the remainder last."""
    for k0 in range(0, n, group):
        yield k0, min(group, n - k0)


def windows(t, k0, g, T, dim=-1):
    """Windows k0 .. k0+g-1 of width T along dimension `dim` of t, concatenated call-major along dimension 0."""
    return torch.cat([t.narrow(dim, k, T) for k in range(k0, k0 + g)], 0)


def joined(pieces):
    """The groups' results along dimension 0: one piece as it is, several concatenated."""
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces, 0)
