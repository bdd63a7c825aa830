"""Plain-torch restatement of the reference's conv slice predictors (SliceLearner.py, class SliceLearner;
LearnSlice.forward_from_vorticity, LearnSlice.py:155-193, which SequenSolverMerged.SequenSolver.forward_slice repeats line for
line), in whatever dtype its inputs have (helper module of the suite, not a conftest): the three stages on their own, the two
forwards from a state_dict, the seeded weights and inputs that tools/make_golden_slicepredictor.py and the tests both draw,
and access to tests/golden/G12_slicepredictor.npz.  Test infrastructure only."""
from __future__ import annotations

import json

import numpy as np
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------- stages
def conv3x3(z, w, b, H, W):
    """Conv2d(C, C, 3, 1, 1) on the [B, N, C] tensor viewed as [B, H, W, C]."""
    B, N, C = z.shape
    img = z.reshape(B, H, W, C).permute(0, 3, 1, 2)
    return F.conv2d(img, w, b, padding=1).permute(0, 2, 3, 1).reshape(B, N, w.shape[0])


def zscore(x):
    """z_score_normalization (LearnSlice.py:189-193): mean and population std over the WHOLE tensor."""
    return (x - torch.mean(x)) / (torch.std(x, unbiased=False) + 1e-8)


def zscore_backward(dy, y, sigma, eps=1e-8):
    """The closed form the HIP stage evaluates, for the check against autograd of `zscore`."""
    se = sigma + eps
    return (dy - dy.mean() - y * (dy * y).mean() * se / sigma) / se


def wide_slice_weights(x, ws, bs, temperature, clamp=True):
    t = torch.clamp(temperature, min=0.1, max=5) if clamp else temperature
    return torch.softmax((x @ ws.t() + bs) / t.reshape(()), dim=-1)


def mlp(x, sd, prefix, hidden_layers):
    """The reference's MLP with gelu: n_layers = hidden_layers (0 or 1), res=True on the hidden layer."""
    h = F.gelu(x @ sd[prefix + "linear_pre.0.weight"].t() + sd[prefix + "linear_pre.0.bias"])
    for i in range(hidden_layers):
        h = F.gelu(h @ sd[prefix + f"linears.{i}.0.weight"].t() + sd[prefix + f"linears.{i}.0.bias"]) + h
    return h @ sd[prefix + "linear_post.weight"].t() + sd[prefix + "linear_post.bias"]


# ---------------------------------------------------------------------------------------------- the two forwards
def slice_learner(sd, x, fx, H, W, pos=None):
    """SliceLearner.forward: x [B, N, space_dim] (or pos [1, N, ref^2] with unified_pos), fx [B, N, fun_dim] or None."""
    if pos is not None:
        x = pos.expand(x.shape[0], -1, -1)
    if fx is not None:
        z = mlp(torch.cat((x, fx), -1), sd, "preprocess.", 0)
    else:
        z = mlp(x, sd, "preprocess.", 0) + sd["placeholder"][None, None, :]
    x_mid = conv3x3(z, sd["in_project_x.weight"], sd["in_project_x.bias"], H, W)
    sw = wide_slice_weights(x_mid, sd["in_project_slice.weight"], sd["in_project_slice.bias"], sd["temperature"])
    return sw[:, None]


def vorticity_learner(sd, x, fx, code, H, W):
    """forward_from_vorticity: x [B, N, 64 | 2], fx [B, N, T], code [B, 1, M, C] or None -> [B, 1, N, M]."""
    z = mlp(torch.cat((x, fx), -1), sd, "preprocess.", 0)
    x_mid = conv3x3(z, sd["in_project_x.weight"], sd["in_project_x.bias"], H, W)
    B, N, _ = x_mid.shape
    if code is not None:
        c = zscore(code.reshape(B, 1, -1)).expand(-1, N, -1)
        x_mid = torch.cat((zscore(x_mid), c), -1)
    logits = mlp(x_mid, sd, "in_project_slice.", 1)
    t = torch.clamp(sd["temperature"], min=0.1, max=5).reshape(())
    return torch.softmax(logits / t, dim=-1)[:, None]


# ---------------------------------------------------------------------------------------------- shapes and seeded weights
def _mlp_shapes(prefix, n_in, n_hidden, n_out, hidden_layers):
    s = [(prefix + "linear_pre.0.weight", (n_hidden, n_in)), (prefix + "linear_pre.0.bias", (n_hidden,)),
         (prefix + "linear_post.weight", (n_out, n_hidden)), (prefix + "linear_post.bias", (n_out,))]
    for i in range(hidden_layers):
        s += [(prefix + f"linears.{i}.0.weight", (n_hidden, n_hidden)), (prefix + f"linears.{i}.0.bias", (n_hidden,))]
    return s


def slice_learner_shapes(space_dim=1, n_hidden=256, Time_Input=False, fun_dim=1, ref=8, unified_pos=False, slice_num=32):
    """[(key, shape)] in the order of the reference's state_dict."""
    s = [("temperature", (1, 1, 1, 1)), ("placeholder", (n_hidden,))]
    s += _mlp_shapes("preprocess.", fun_dim + (ref * ref if unified_pos else space_dim), 2 * n_hidden, n_hidden, 0)
    if Time_Input:
        s += [("time_fc.0.weight", (n_hidden, n_hidden)), ("time_fc.0.bias", (n_hidden,)),
              ("time_fc.2.weight", (n_hidden, n_hidden)), ("time_fc.2.bias", (n_hidden,))]
    s += [("in_project_x.weight", (n_hidden, n_hidden, 3, 3)), ("in_project_x.bias", (n_hidden,)),
          ("in_project_slice.weight", (slice_num, n_hidden)), ("in_project_slice.bias", (slice_num,))]
    return s


def vorticity_shapes(unified_pos=1, use_code=True, C=32, M=16, T=10, n_hidden=256):
    """[(key, shape)] of the predictor part of the reference's LearnSlice, in state_dict order."""
    cat = n_hidden + (M * C if use_code else 0)
    s = [("temperature", (1, 1, 1, 1))]
    s += _mlp_shapes("preprocess.", T + (64 if unified_pos else 2), 2 * n_hidden, n_hidden, 0)
    s += [("in_project_x.weight", (n_hidden, n_hidden, 3, 3)), ("in_project_x.bias", (n_hidden,))]
    s += _mlp_shapes("in_project_slice.", cat, cat // 2, M, 1)
    return s


LAST_LAYER = ("in_project_slice.weight", "in_project_slice.linear_post.weight")


def draw_state(shapes, seed, last_gain=1.0):
    """Seeded float32 weights for [(key, shape)], drawn key by key in the given order: weights normal with std
    1.5 / sqrt(fan_in) (the last layer times `last_gain`: sharp slice weights show errors that flat ones hide), biases normal
    with std 0.1, the placeholder uniform in [0, 1/n), the temperature 0.5."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in shapes:
        if key == "temperature":
            a = np.full(shape, 0.5)
        elif key == "placeholder":
            a = rng.random(shape) / shape[0]
        elif key.endswith("bias"):
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) * (1.5 / np.sqrt(np.prod(shape[1:])))
            if key in LAST_LAYER:
                a = a * last_gain
        sd[key] = a.astype(np.float32)
    return sd


def state_sum(sd):
    return float(sum(np.sum(a, dtype=np.float64) for a in sd.values()))


def to_torch(sd, dtype, requires_grad=False):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(requires_grad) for k, v in sd.items()}


def draw_inputs(seed, B, N, n_x, n_fx, M, C):
    """(x [B, N, n_x] uniform, fx [B, N, n_fx] normal, code [B, 1, M, C] normal * 2 + 0.3, dsw [B, 1, N, M] normal,
    target [B, 1, N, M]: a softmax of 2 * normals), float32 except the float64 target."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, N, n_x)).astype(np.float32)
    fx = rng.standard_normal((B, N, n_fx)).astype(np.float32)
    code = (2.0 * rng.standard_normal((B, 1, M, C)) + 0.3).astype(np.float32)
    dsw = rng.standard_normal((B, 1, N, M)).astype(np.float32)
    target = torch.softmax(torch.from_numpy(2.0 * rng.standard_normal((B, 1, N, M))), dim=-1).numpy()
    return x, fx, code, dsw, target


def input_sums(arrays):
    return np.array([np.sum(a, dtype=np.float64) for a in arrays])


# ---------------------------------------------------------------------------------------------- G12 fixture access
SMALL = dict(space_dim=2, n_hidden=32, Time_Input=True, fun_dim=3, ref=8, unified_pos=False, H=6, W=5, slice_num=12)
SMALL_B, SMALL_SEED, SMALL_GAIN = 2, 71, 0.4
VORT = dict(unified_pos=1, C=32, M=16, T=10, H=64, W=64, n_hidden=256)
VORT_CASES = {"code": dict(use_code=True, seed=72, last_gain=0.5), "nocode": dict(use_code=False, seed=73, last_gain=0.5)}
STRIDE, GRAD_SAMPLES = 7, 257


def small_case():
    """(state_dict, x, fx, dsw) of the small SliceLearner case, float32 arrays."""
    shp = slice_learner_shapes(**{k: v for k, v in SMALL.items() if k not in ("H", "W")})
    sd = draw_state(shp, SMALL_SEED, SMALL_GAIN)
    x, fx, _, dsw, _ = draw_inputs(SMALL_SEED + 100, SMALL_B, SMALL["H"] * SMALL["W"], SMALL["space_dim"], SMALL["fun_dim"],
                                   SMALL["slice_num"], 1)
    return sd, x, fx, dsw


def vort_case(name):
    """(state_dict, x, fx, code or None, target) of a forward_from_vorticity case at the reference's fixed shape."""
    cfg = VORT_CASES[name]
    shp = vorticity_shapes(VORT["unified_pos"], cfg["use_code"], VORT["C"], VORT["M"], VORT["T"], VORT["n_hidden"])
    sd = draw_state(shp, cfg["seed"], cfg["last_gain"])
    x, fx, code, _, target = draw_inputs(cfg["seed"] + 100, 1, VORT["H"] * VORT["W"], 64, VORT["T"], VORT["M"], VORT["C"])
    return sd, x, fx, (code if cfg["use_code"] else None), target


def check_sums(g, key, sd, arrays):
    """The regenerated weights and inputs are the generator's: compared by their sums."""
    np.testing.assert_allclose(state_sum(sd), float(g[key + ".state_sum"]), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(input_sums([a for a in arrays if a is not None]), g[key + ".input_sums"], rtol=1e-12, atol=1e-12)


def grad_sample(a):
    """(norm, every k-th element) of a gradient: what G12 stores of the large ones."""
    f = np.asarray(a, dtype=np.float64).ravel()
    k = max(1, f.size // GRAD_SAMPLES)
    return float(np.linalg.norm(f)), f[::k].copy()


def key_list(g, name):
    return [(k, tuple(s)) for k, s in json.loads(str(g[name]))]


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a.reshape(-1) - b.reshape(-1)).norm() / b.norm().clamp_min(1e-300))
