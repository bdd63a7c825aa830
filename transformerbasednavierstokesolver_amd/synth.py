"""Build-owned deterministic generators: model weights and Navier-Stokes-like fields.

The reference ships no datasets (its `data/` is git-ignored) and does not seed anything, so
parity is defined on identical weights + inputs.  Everything here is a pure
function of (config, seed) through `numpy.random.default_rng`, so the GPU box can regenerate the
exact tensors the golden fixtures were captured on without access to the reference.

State-dict layout follows the reference contract (key names / shapes of
model/Transolver_Structured_Mesh_2D.py:122-181 and model/Physics_Attention.py:62-86).
"""
from __future__ import annotations

import numpy as np

__all__ = ["darcy_batch", "DARCY_CONFIG", "make_config", "state_dict_spec", "synth_state_dict", "synth_state_dict_from_spec",
           "synth_ns_fields", "ns_batch",
           "meshgrid_pos", "NS_CONFIG", "NS_SMALL_CONFIG", "TINY_CONFIG", "mesh_field_arrays", "elas_arrays", "plas_input",
           "plas_output_sample"]


def make_config(space_dim=2, n_layers=8, n_hidden=256, n_head=8, mlp_ratio=1, fun_dim=10, out_dim=1,
                slice_num=64, ref=8, unified_pos=1, H=64, W=64, Time_Input=False, act="gelu",
                dropout=0.0):
    return dict(space_dim=space_dim, n_layers=n_layers, n_hidden=n_hidden, n_head=n_head,
                mlp_ratio=mlp_ratio, fun_dim=fun_dim, out_dim=out_dim, slice_num=slice_num, ref=ref,
                unified_pos=int(unified_pos), H=H, W=W, Time_Input=bool(Time_Input), act=act,
                dropout=dropout)


# BASELINE.json configs[1]: NS 64x64, 8 layers, C=256, 8 heads, M=64 slices.
NS_CONFIG = make_config()
# Size of the checkpoints the reference ships (checkpoints/ep400_sim100.pt): C=64, M=32.
NS_SMALL_CONFIG = make_config(n_hidden=64, slice_num=32)
# Tiny parity case (non-square grid, D=8, M=12 not a multiple of 16, out_dim 2).
TINY_CONFIG = make_config(n_layers=2, n_hidden=32, n_head=4, fun_dim=3, out_dim=2, slice_num=12,
                          ref=3, unified_pos=1, H=6, W=5, mlp_ratio=2)


def in_features(cfg):
    return cfg["fun_dim"] + (cfg["ref"] ** 2 if cfg["unified_pos"] else cfg["space_dim"])


def state_dict_spec(cfg):
    """Ordered (key, shape, kind) triples of the reference Model.state_dict()."""
    C, L, h = cfg["n_hidden"], cfg["n_layers"], cfg["n_head"]
    D, M, r = C // h, cfg["slice_num"], cfg["mlp_ratio"]
    spec = [("placeholder", (C,), "placeholder"),
            ("preprocess.linear_pre.0.weight", (2 * C, in_features(cfg)), "lin_w"),
            ("preprocess.linear_pre.0.bias", (2 * C,), "bias"),
            ("preprocess.linear_post.weight", (C, 2 * C), "lin_w"),
            ("preprocess.linear_post.bias", (C,), "bias")]
    if cfg["Time_Input"]:
        spec += [("time_fc.0.weight", (C, C), "lin_w"), ("time_fc.0.bias", (C,), "bias"),
                 ("time_fc.2.weight", (C, C), "lin_w"), ("time_fc.2.bias", (C,), "bias")]
    for i in range(L):
        p = f"blocks.{i}."
        spec += [(p + "ln_1.weight", (C,), "ln_w"), (p + "ln_1.bias", (C,), "bias"),
                 (p + "Attn.temperature", (1, h, 1, 1), "temperature"),
                 (p + "Attn.in_project_x.weight", (C, C, 3, 3), "conv_w"),
                 (p + "Attn.in_project_x.bias", (C,), "bias"),
                 (p + "Attn.in_project_fx.weight", (C, C, 3, 3), "conv_w"),
                 (p + "Attn.in_project_fx.bias", (C,), "bias"),
                 (p + "Attn.in_project_slice.weight", (M, D), "slice_w"),
                 (p + "Attn.in_project_slice.bias", (M,), "bias"),
                 (p + "Attn.to_q.weight", (D, D), "qk_w"),
                 (p + "Attn.to_k.weight", (D, D), "qk_w"),
                 (p + "Attn.to_v.weight", (D, D), "lin_w"),
                 (p + "Attn.to_out.0.weight", (C, C), "lin_w"),
                 (p + "Attn.to_out.0.bias", (C,), "bias"),
                 (p + "ln_2.weight", (C,), "ln_w"), (p + "ln_2.bias", (C,), "bias"),
                 (p + "mlp.linear_pre.0.weight", (r * C, C), "lin_w"),
                 (p + "mlp.linear_pre.0.bias", (r * C,), "bias"),
                 (p + "mlp.linear_post.weight", (C, r * C), "lin_w"),
                 (p + "mlp.linear_post.bias", (C,), "bias")]
        if i == L - 1:
            spec += [(p + "ln_3.weight", (C,), "ln_w"), (p + "ln_3.bias", (C,), "bias"),
                     (p + "mlp2.weight", (cfg["out_dim"], C), "lin_w"),
                     (p + "mlp2.bias", (cfg["out_dim"],), "bias")]
    return spec


def irregular_state_dict_spec(cfg):
    """state_dict of model/Transolver_Irregular_Mesh.Model: same keys, Linear [C,C] projections."""
    out = []
    for key, shape, kind in state_dict_spec(cfg):
        if kind == "conv_w":
            out.append((key, shape[:2], "lin_w"))
        else:
            out.append((key, shape, kind))
    return out


def synth_irregular_state_dict(cfg, seed=0):
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape, kind in irregular_state_dict_spec(cfg):
        if kind in ("lin_w",):
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        elif kind == "qk_w":
            v = rng.standard_normal(shape) * (1.5 / np.sqrt(shape[1]))
        elif kind == "slice_w":
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        elif kind == "bias":
            v = 0.1 * rng.standard_normal(shape)
        elif kind == "ln_w":
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif kind == "temperature":          # NOT clamped in this family: include values outside [0.1, 5]
            v = np.resize(np.array([0.06, 0.5, 6.0, 0.25, 1.5, 0.8, 0.3, 1.1]), shape[1]).reshape(shape)
        else:
            v = rng.uniform(0.0, 1.0, size=shape) / shape[0]
        sd[key] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def synth_state_dict(cfg, seed=0, wild_temperature=False):
    """Deterministic fp32 weights (numpy) with O(1) activations through the whole stack.

    Scales are chosen so that the slice softmax and the token attention are far from uniform
    (the reference's trunc_normal(0.02) init leaves to_q/to_k gradients ~1e-9), which
    makes parity tests discriminating.  `wild_temperature` puts some heads outside [0.1, 5] to
    pin the clamp mask of Physics_Attention.py:98-99.
    """
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape, kind in state_dict_spec(cfg):
        if kind == "lin_w":
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        elif kind == "qk_w":
            v = rng.standard_normal(shape) * (1.5 / np.sqrt(shape[1]))
        elif kind == "slice_w":
            v = rng.standard_normal(shape) * (1.0 / np.sqrt(shape[1]))
        elif kind == "conv_w":
            v = rng.standard_normal(shape) / np.sqrt(9.0 * shape[1])
        elif kind == "bias":
            v = 0.1 * rng.standard_normal(shape)
        elif kind == "ln_w":
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif kind == "temperature":
            if wild_temperature:
                pool = np.array([0.03, 0.5, 7.0, 0.25, 1.5, 0.1, 5.0, 0.8])
                v = np.resize(pool, shape[1]).reshape(shape)
            else:
                v = rng.uniform(0.3, 1.2, size=shape)
        elif kind == "placeholder":
            v = rng.uniform(0.0, 1.0, size=shape) / shape[0]
        else:  # pragma: no cover
            raise KeyError(kind)
        out[key] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def spec_kind(key, shape):
    """Kind (as in state_dict_spec) of a state_dict entry of any Transolver family, from its name and shape."""
    if key.endswith("temperature"):
        return "temperature"
    if key == "placeholder":
        return "placeholder"
    if key.endswith(".bias"):
        return "bias"
    if ".ln_" in key or key.startswith("ln_"):      # top-level LayerNorms (SequenSolver) as well as a block's
        return "ln_w"
    if key.endswith(("to_q.weight", "to_k.weight")):
        return "qk_w"
    if key.endswith("in_project_slice.weight"):
        return "slice_w"
    return "conv_w" if len(shape) > 2 else "lin_w"


def synth_state_dict_from_spec(spec, seed=0, wild_temperature=False):
    """synth_state_dict for an explicit [(key, shape), ...] list (e.g. a model's state_dict order): the same kinds and
    scales, a conv weight [C_out, C_in, k...] scaled by 1/sqrt(C_in * taps) whatever its number of kernel axes."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in spec:
        shape = tuple(int(s) for s in shape)
        kind = spec_kind(key, shape)
        if kind == "lin_w":
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        elif kind == "qk_w":
            v = rng.standard_normal(shape) * (1.5 / np.sqrt(shape[1]))
        elif kind == "slice_w":
            v = rng.standard_normal(shape) * (1.0 / np.sqrt(shape[1]))
        elif kind == "conv_w":
            v = rng.standard_normal(shape) / np.sqrt(float(np.prod(shape[1:])))
        elif kind == "bias":
            v = 0.1 * rng.standard_normal(shape)
        elif kind == "ln_w":
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif kind == "temperature":
            if wild_temperature:
                pool = np.array([0.03, 0.5, 7.0, 0.25, 1.5, 0.1, 5.0, 0.8])
                v = np.resize(pool, shape[1]).reshape(shape)
            else:
                v = rng.uniform(0.3, 1.2, size=shape)
        else:
            v = rng.uniform(0.0, 1.0, size=shape) / shape[0]
        out[key] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def synth_ns_fields(S, H=64, W=64, T=20, seed=0):
    """[S,H,W,T] fp32 vorticity-like trajectories: low-passed Gaussian noise whose
    Fourier modes rotate (advection) and decay slowly from frame to frame; unit std overall."""
    rng = np.random.default_rng(seed)
    ky = np.fft.fftfreq(H, d=1.0 / H)[:, None]
    kx = np.fft.fftfreq(W, d=1.0 / W)[None, :]
    k2 = ky ** 2 + kx ** 2
    amp = (1.0 + k2 / 16.0) ** -1.25
    out = np.empty((S, H, W, T), dtype=np.float32)
    for s in range(S):
        spec = np.fft.fft2(rng.standard_normal((H, W))) * amp
        vel = rng.uniform(-1.5, 1.5, size=2)
        phase = np.exp(-2j * np.pi * (ky * vel[0] / H + kx * vel[1] / W))
        decay = np.exp(-1e-3 * k2)
        for t in range(T):
            out[s, :, :, t] = np.real(np.fft.ifft2(spec))
            spec = spec * phase * decay
    out /= out.std()
    return out


def meshgrid_pos(S, H, W):
    """Driver-side plain position input, exp_ns.py:88-94 convention ('xy' meshgrid: the first
    coordinate varies along image columns)."""
    x = np.linspace(0, 1, W)
    y = np.linspace(0, 1, H)
    xx, yy = np.meshgrid(x, y)
    pos = np.stack([xx.ravel(), yy.ravel()], axis=-1).astype(np.float32)
    return np.array(np.broadcast_to(pos[None], (S, H * W, 2)))   # writable copy


def ns_batch(S, H=64, W=64, T_in=10, T=10, seed=0):
    """(pos [S,N,2], a [S,N,T_in], u [S,N,T]) with the exp_ns.py:64-80 split of a trajectory."""
    f = synth_ns_fields(S, H, W, T_in + T, seed)
    a = np.ascontiguousarray(f[..., :T_in].reshape(S, H * W, T_in))
    u = np.ascontiguousarray(f[..., T_in:].reshape(S, H * W, T))
    return meshgrid_pos(S, H, W), a, u


# BASELINE.json configs[4]: Darcy 421x421 structured mesh, 8 layers, C=128, 8 heads, M=128 slices
# (exp_darcy.py:118-130 constructor arguments: fun_dim=1, out_dim=1, unified_pos + ref 8 as scripts/Transolver_Darcy.sh).
DARCY_CONFIG = make_config(n_layers=8, n_hidden=128, n_head=8, slice_num=128, fun_dim=1, out_dim=1, H=421, W=421)


def darcy_batch(S, s=421, seed=0):
    """(pos [S,N,2], coeff [S,N], sol [S,N]) shaped like exp_darcy.py:76-83: `coeff` a piecewise-constant {3, 12}
    permeability field (thresholded low-passed noise, as the FNO Darcy set), `sol` a smooth O(1e-2) field standing
    in for the pressure solution (values only need the right shape and smoothness; throughput is value-independent)."""
    rng = np.random.default_rng(seed)
    k = np.fft.fftfreq(s, d=1.0 / s)
    k2 = k[:, None] ** 2 + k[None, :] ** 2
    coeff = np.empty((S, s * s), dtype=np.float32)
    sol = np.empty((S, s * s), dtype=np.float32)
    for i in range(S):
        g = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((s, s))) * (1.0 + k2 / 9.0) ** -1.0))
        coeff[i] = np.where(g > 0, 12.0, 3.0).ravel()
        u = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((s, s))) * (1.0 + k2 / 4.0) ** -1.5))
        sol[i] = (0.01 * u / u.std() + 0.02).ravel()
    return meshgrid_pos(S, s, s), coeff, sol


# ------------------------------------------------------------------ stand-ins for the airfoil / pipe / elas / plas files
def mesh_field_arrays(n, h, w, channels, channel, seed):
    """(X, Y [n, h, w], Q [n, channels, h, w]) float32 shaped like NACA_Cylinder_{X,Y,Q}.npy (221 x 51, target channel 4) and
    Pipe_{X,Y,Q}.npy (129 x 129, target channel 0): a smoothly deformed mesh per sample and a smooth O(1) field with a
    non-zero mean on it in `channel`; the other channels hold other fields, so a wrong channel shows."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    a = rng.uniform(0.6, 1.4, (n, 1, 1)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, (n, 1, 1)).astype(np.float32)
    ph = rng.uniform(0, 2 * np.pi, (n, 1, 1)).astype(np.float32)
    two_pi = np.float32(2 * np.pi)
    X = i[None] * a + b * np.sin(two_pi * j)[None]
    Y = j[None] * (2 - a) + b * np.cos(two_pi * i)[None]
    q = np.sin(two_pi * (X * a + Y) + ph) + 0.5 * np.cos(two_pi * (X - Y) * a) + 0.7
    Q = np.empty((n, channels, h, w), dtype=np.float32)
    for c in range(channels):
        Q[:, c] = q if c == channel else np.float32(c + 1) - q
    return X.astype(np.float32), Y.astype(np.float32), Q


def elas_arrays(samples, points, seed):
    """(sigma [points, samples], XY [points, 2, samples]) float32 shaped like Random_UnitCell_{sigma,XY}_10.npy: scattered
    points in the unit square and a smooth stress-like field O(100) on them."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 1, (points, 2, samples))
    a = rng.uniform(0.5, 2.0, (1, samples))
    ph = rng.uniform(0, 2 * np.pi, (1, samples))
    sigma = 150.0 + 80.0 * np.sin(2 * np.pi * a * xy[:, 0] + ph) * np.cos(2 * np.pi * xy[:, 1]) + 30.0 * xy[:, 0] * a
    return sigma.astype(np.float32), xy.astype(np.float32)


def plas_input(samples, seed, s1=101):
    """'input' of plas_N987_T20.mat: [samples, s1] float32 die profiles."""
    rng = np.random.default_rng(seed)
    s = np.linspace(0, 1, s1)[None]
    a, ph = rng.uniform(0.5, 1.5, (samples, 1)), rng.uniform(0, 2 * np.pi, (samples, 1))
    return (a * np.sin(2 * np.pi * s + ph) + 0.5 * a + s).astype(np.float32)


def plas_output_sample(index, seed, s1=101, s2=31, T=20):
    """One sample of 'output' of plas_N987_T20.mat: [s1, s2, T, 4] float32 (mesh position and displacement growing with
    time), a pure function of (seed, index) so that a few samples can be made without the other 980."""
    rng = np.random.default_rng([seed, index])
    i, j, t = np.meshgrid(np.linspace(0, 1, s1), np.linspace(0, 1, s2), np.linspace(0, 1, T), indexing="ij")
    a, b, ph = rng.uniform(0.5, 1.5), rng.uniform(-0.3, 0.3), rng.uniform(0, 2 * np.pi)
    du = a * t * np.sin(np.pi * i + ph) * (1 - j)
    dv = b * t * np.cos(np.pi * j) * i
    return np.stack([50.0 * i + du, 15.0 * j + dv, du, dv], axis=-1).astype(np.float32)


def velocity_fields(S, H=64, W=64, frames=20, seed=0):
    """[S, H, W, 2 * frames] fp32: a seeded, divergence-free (vel_x, vel_y) sequence standing in for the PhiFlow arrays of
    ns_velocity.py (ns_50_20.npy: frame t is the column pair (2 t, 2 t + 1), vel_x first).  The vorticity w of
    `synth_ns_fields` gives the stream function psi with -lap psi = w (spectral, the mean mode dropped) and the velocity
    (d psi / dy, -d psi / dx), whose spectral divergence is zero mode by mode; unit std overall."""
    w = synth_ns_fields(S, H, W, frames, seed).astype(np.float64)
    ky = 2.0 * np.pi * np.fft.fftfreq(H, d=1.0 / H)[:, None]
    kx = 2.0 * np.pi * np.fft.fftfreq(W, d=1.0 / W)[None, :]
    k2 = ky ** 2 + kx ** 2
    k2[0, 0] = 1.0
    psi = np.fft.fft2(w, axes=(1, 2)) / k2[None, :, :, None]
    psi[:, 0, 0, :] = 0.0
    if H % 2 == 0:                       # the Nyquist rows / columns have no real derivative: dropped
        psi[:, H // 2, :, :] = 0.0
    if W % 2 == 0:
        psi[:, :, W // 2, :] = 0.0
    vx =np.real(np.fft.ifft2(1j * ky[None, :, :, None] * psi, axes=(1, 2)))
    vy = np.real(np.fft.ifft2(-1j * kx[None, :, :, None] * psi, axes=(1, 2)))
    out = np.stack((vx, vy), axis=-1).reshape(S, H, W, 2 * frames)
    return (out / out.std()).astype(np.float32)
