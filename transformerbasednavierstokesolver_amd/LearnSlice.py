"""LearnSlice — slice weights learned from the code and what is known about a mesh point; the drop-in for the part of the
reference's top-level LearnSlice.py (class LearnSlice, :41-153) that its shipped checkpoints (`sequential_checkpoints/
slice_*.pt`) hold: `weight_projection = MLP(C + P, 64, 1)` with one hidden layer and a softmax over the M slices,

    w[n, :] = softmax_m(weight_projection(cat(code[m, :], feat[n, :])))

where feat is P wide: the two point coordinates (P = 2) or the 64 `unified_pos` distances to the 8 x 8 reference grid
(P = 64), plus the last T frames when `use_vorticity` is set (P = 12 / 74).  The reference calls the MLP once per point in a
Python loop; here all B * N * M rows are ONE kernel launch (functional.point_slice_weights, pa2d_point_slice_weights_*), and
`harness.learnslice_train_step` restates the trainer (:477-526) with one forward and one backward launch per step.

The constructor keeps the reference's three parameters; C, M and T (keyword-only; the reference hard-codes 32, 16 and 10)
are the extension.  Only `weight_projection` is built, so the state_dict is its six tensors and every shipped checkpoint
loads with strict=True (the reference's other sub-modules are freshly initialised in every checkpoint-less use and belong
to the methods that raise below).  The reference's get_slice_weight reads sample 0 only; here every sample of the batch
uses its own code and features, which is the same at B = 1."""
import torch
import torch.nn as nn

from . import functional as Fn
from .model._core import ACTIVATION, MLP  # noqa: F401  (the reference module defines both names)

WEIGHT_PROJECTION_HIDDEN = 64
UNIFIED_POS_WIDTH = 64      # the 8 x 8 reference grid of get_grid() (:230-248)


class LearnSlice(nn.Module):

    def __init__(self, unified_pos=0, use_vorticity=0, use_code_for_vorticity=False, *, C=32, M=16, T=10):
        super().__init__()
        self.C, self.M, self.T = C, M, T
        self.unified_pos = unified_pos
        self.use_vorticity = use_vorticity
        self.use_code_for_vorticity = use_code_for_vorticity
        self.pos = (UNIFIED_POS_WIDTH if unified_pos else 2) + (T if use_vorticity else 0)      # reference :52-59
        self.weight_projection = MLP(self.C + self.pos, WEIGHT_PROJECTION_HIDDEN, 1)

    def _params(self):
        wp = self.weight_projection
        return (wp.linear_pre[0].weight, wp.linear_pre[0].bias, wp.linears[0][0].weight, wp.linears[0][0].bias,
                wp.linear_post.weight, wp.linear_post.bias)

    def _weights(self, code, feat):
        """code [B, M, C], feat [B, N, P] -> [B, 1, N, M]."""
        if code.shape[-1] != self.C or feat.shape[-1] != self.pos:
            raise ValueError(f"this LearnSlice takes a code of C = {self.C} channels and P = {self.pos} features per point "
                             f"(unified_pos={self.unified_pos}, use_vorticity={self.use_vorticity}); got "
                             f"{tuple(code.shape)} and {tuple(feat.shape)}")
        return Fn.point_slice_weights(code, feat, *self._params())

    def forward(self, code, spatial_pos):
        """The reference's per-point call: code [M, C], spatial_pos [1, P] -> w [1, M] (M from `code`)."""
        return self._weights(code[None], spatial_pos[None]).reshape(1, code.shape[0])

    def get_slice_weight(self, tokens, spatial_pos, fx, use_vorticity=0):
        """tokens [B, 1, M, C] (the code), spatial_pos [B, N, P0], fx [B, N, T] (read with use_vorticity only)
        -> slice weights [B, 1, N, M]; with use_vorticity the point features are cat(spatial_pos, fx)."""
        B, _, M, C = tokens.shape
        feat = torch.cat((spatial_pos, fx), -1) if use_vorticity else spatial_pos
        return self._weights(tokens.reshape(B, M, C), feat)

    # ---- the reference's other predictors: no shipped checkpoint holds their weights
    def forward_all(self, concatenated):
        raise NotImplementedError("forward_all takes the concatenated [N, M, C+P] tensor, which this package never forms: "
                                  "use get_slice_weight(tokens, spatial_pos, fx)")

    def forward_previous_slice(self, prev_slice_weight, token):
        raise NotImplementedError("forward_previous_slice needs weight_projection_form_slice = MLP(M + M*C, 4 (M + M*C), M) "
                                  "(2112 wide at the reference's shape), which is not built: no shipped checkpoint holds it")

    def forward_from_vorticity(self, x, fx, code=None):
        raise NotImplementedError("forward_from_vorticity needs the conv slice predictor (preprocess, in_project_x, "
                                  "in_project_slice, temperature), which is not built: no shipped checkpoint holds it")

    def forward_from_vorticity_seperate(self, x, fx, code):
        raise NotImplementedError("forward_from_vorticity_seperate needs the per-slice conv predictor (preprocess_seperate, "
                                  "in_project_x_seperate, in_project_slice_seperate), which is not built: no shipped "
                                  "checkpoint holds it")
