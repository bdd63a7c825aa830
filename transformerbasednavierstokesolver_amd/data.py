"""Data ingress either side of the hot path.

* `load_ns_mat` / `split_ns_trajectories`   the `.mat` -> (a, u) slicing of exp_ns.py:64-80
* `load_darcy_mat` / `darcy_from_mats` / `split_darcy`   exp_darcy.py:76-99 (coeff/sol fields + UnitTransformer encoding)
* `load_airfoil_npy` / `load_pipe_npy` / `load_elas_npy` / `load_plas_mat` (and their `*_from_arrays` / `plas_from_mat`)
                                            the `.npy` / `.mat` slicing and UnitTransformer encoding of exp_airfoil.py:50-79,
                                            exp_pipe.py:52-91, exp_elas.py:54-72, exp_plas.py:105-137
* `grid_positions`                          the driver-side position input (exp_ns.py:88-94)
* `ResidentDataset`                         the whole split kept in HBM and batched by device-side index
                                            selection: replaces TensorDataset + DataLoader(num_workers=0) +
                                            per-batch `.cuda()` (exp_ns.py:96-99,195); one NS split at 64x64
                                            is 1200 x 4096 x 20 x 4 B = 393 MB, nothing against 288 GB
* `simulate_ns_vorticity`                   torch.fft pseudo-spectral 2-D Navier-Stokes (vorticity form,
                                            FNO forcing) standing in for the PhiFlow data-generation notebook.
                                            PARITY UNPINNED: the notebook's generator (PhiFlow + an external
                                            repo) cannot run here; this is a utility, tested on invariants only.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .utils.normalizer import UnitTransformer


def _downsampled(field, r, h):
    return field[:, ::r, ::r][:, :h, :h]


def split_ns_trajectories(u, ntrain, ntest, T_in=10, T=10, r=1):
    """u: [S, 64, 64, >=T_in+T].  First `ntrain` trajectories train, LAST `ntest` test; inputs are frames
    [0, T_in), targets frames [T_in, T_in+T); spatial stride r; points flattened row-major."""
    u = np.asarray(u)
    h = int(((u.shape[1] - 1) / r) + 1)

    def cut(block, t0, t1):
        x = _downsampled(block[..., t0:t1], r, h)
        return torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1, x.shape[-1])))

    tr, te = u[:ntrain], u[-ntest:]
    return dict(h=h, train_a=cut(tr, 0, T_in), train_u=cut(tr, T_in, T_in + T),
                test_a=cut(te, 0, T_in), test_u=cut(te, T_in, T_in + T))


def split_ns_all_frames(u, ntrain, ntest):
    """The split the auto-encoder trains on (auto_encoder.py:81-88): u [S, H, W, F] -> train [ntrain*F, H*W, 1] of the
    first `ntrain` trajectories and test [ntest*F, H*W, 1] of the LAST `ntest`.  As in the script, [n, H*W, F] is RESHAPED
    to [n*F, H*W, 1] (no transpose): sample i*F + j is the j-th run of H*W consecutive values of trajectory i's
    point-major, frame-minor memory."""
    u = np.asarray(u)

    def frames(block):
        flat = block.reshape(block.shape[0], -1, block.shape[-1])
        return torch.from_numpy(np.ascontiguousarray(flat.reshape(flat.shape[0] * flat.shape[-1], flat.shape[1], 1)))

    return dict(h=u.shape[1], train=frames(u[:ntrain]), test=frames(u[-ntest:]))


def load_ns_mat(path, ntrain, ntest, T_in=10, T=10, r=1, key="u"):
    import scipy.io as scio
    return split_ns_trajectories(scio.loadmat(path)[key], ntrain, ntest, T_in, T, r)


def split_darcy(coeff, sol, n, r=1):
    """[S, 421, 421] fields -> ([n, s*s] float32 coefficient, [n, s*s] solution, s)"""
    s = int(((coeff.shape[1] - 1) / r) + 1)
    x = torch.from_numpy(np.ascontiguousarray(_downsampled(np.asarray(coeff)[:n], r, s).reshape(n, -1))).float()
    y = torch.from_numpy(np.ascontiguousarray(_downsampled(np.asarray(sol)[:n], r, s).reshape(n, -1)))
    return x, y, s


def darcy_from_mats(tr, te, ntrain, ntest, r=1):
    """exp_darcy.py:77-98 on the two loaded `.mat` dicts ('coeff', 'sol'): encoded train/test inputs, the encoded train
    target, the RAW test target, the two normalisers (fitted on the TRAIN split), s and dx = 1/s."""
    x_train, y_train, s = split_darcy(tr["coeff"], tr["sol"], ntrain, r)
    x_test, y_test, _ = split_darcy(te["coeff"], te["sol"], ntest, r)
    xn, yn = UnitTransformer(x_train), UnitTransformer(y_train)
    return dict(s=s, dx=1.0 / s, x_normalizer=xn, y_normalizer=yn, x_train=xn.encode(x_train),
                y_train=yn.encode(y_train), x_test=xn.encode(x_test), y_test=y_test)


def load_darcy_mat(train_path, test_path, ntrain, ntest, r=1):
    """Returns encoded train/test tensors, the two normalisers (fitted on the TRAIN split), s and dx = 1/s."""
    import scipy.io as scio
    return darcy_from_mats(scio.loadmat(train_path), scio.loadmat(test_path), ntrain, ntest, r)


def grid_positions(h, w=None):
    """[1, h*w, 2] float32; 'xy' meshgrid, i.e. the FIRST coordinate varies along image columns."""
    w = h if w is None else w
    xx, yy = np.meshgrid(np.linspace(0, 1, w), np.linspace(0, 1, h))
    return torch.tensor(np.c_[xx.ravel(), yy.ravel()], dtype=torch.float).unsqueeze(0)


def unified_positions(h, w=None, ref=8):
    """[1, h*w, ref*ref] float32: the `unified_pos` point input that the SequenSolver scripts' train() builds with their
    get_grid(): the Euclidean distance of mesh point (i/(h-1), j/(w-1)) to the lattice point (k/(ref-1), l/(ref-1)),
    feature index k*ref + l; linspace in float64, arithmetic in float32 (SliceLearner.get_grid is the same table)."""
    w = h if w is None else w
    axis = lambda n: torch.tensor(np.linspace(0, 1, n), dtype=torch.float)
    rows, cols, lat = axis(h), axis(w), axis(ref)
    dr2 = (rows[:, None] - lat[None, :]) ** 2
    dc2 = (cols[:, None] - lat[None, :]) ** 2
    return torch.sqrt(dr2[:, None, :, None] + dc2[None, :, None, :]).reshape(1, h * w, ref * ref).contiguous()


class ResidentDataset:
    """Tensors with a common leading sample dimension, resident on one device."""

    def __init__(self, *tensors, device=None):
        n = tensors[0].shape[0]
        if any(t.shape[0] != n for t in tensors):
            raise ValueError("all tensors need the same number of samples")
        self.tensors = [t.to(device).contiguous() if device is not None else t.contiguous() for t in tensors]

    def __len__(self):
        return self.tensors[0].shape[0]

    def shard(self, rank, world_size):
        """contiguous equal shards (drops the remainder, like DistributedSampler(drop_last=True))"""
        n = len(self) // world_size
        return ResidentDataset(*[t[rank * n:(rank + 1) * n] for t in self.tensors])

    def batches(self, batch_size, shuffle=False, generator=None, drop_last=False, order=None):
        """`order`: an index tensor (or sequence) that overrides `shuffle`: the samples are taken in exactly this order,
        the short last batch included (a recorded permutation replayed, harness.fit_*'s `epoch_orders`)."""
        n, dev = len(self), self.tensors[0].device
        if order is not None:
            order = torch.as_tensor(order, dtype=torch.long).to(dev)
            n = order.numel()
        else:
            order = torch.randperm(n, device=dev, generator=generator) if shuffle else torch.arange(n, device=dev)
        for i in range(0, n, batch_size):
            idx = order[i:i + batch_size]
            if drop_last and idx.numel() < batch_size:
                return
            yield tuple(t.index_select(0, idx) for t in self.tensors)


@torch.no_grad()
def simulate_ns_vorticity(w0, visc=1e-5, T=20.0, dt=1e-3, record=20, forcing=True):
    """Pseudo-spectral 2-D Navier-Stokes in vorticity form on the periodic unit square:
    w_t + u.grad(w) = visc * lap(w) + f,  f = 0.1 (sin 2pi(x+y) + cos 2pi(x+y)),  Crank-Nicolson for the
    viscous term, explicit advection, 2/3 de-aliasing.  w0: [S, n, n].  Returns [S, n, n, record]."""
    S, n, _ = w0.shape
    dev, dt64 = w0.device, torch.float64
    k = torch.fft.fftfreq(n, d=1.0 / n, device=dev).to(dt64)
    ky, kx = k.reshape(n, 1).expand(n, n), k.reshape(1, n).expand(n, n)
    lap = 4 * math.pi ** 2 * (kx ** 2 + ky ** 2)
    lap_safe = lap.clone()
    lap_safe[0, 0] = 1.0
    dealias = ((kx.abs() <= n / 3) & (ky.abs() <= n / 3)).to(dt64)
    grid = torch.linspace(0, 1, n + 1, device=dev, dtype=dt64)[:-1]
    xs, ys = grid.reshape(1, n), grid.reshape(n, 1)
    f_h = torch.fft.fft2(0.1 * (torch.sin(2 * math.pi * (xs + ys)) + torch.cos(2 * math.pi * (xs + ys)))) if forcing else 0.0
    w_h = torch.fft.fft2(w0.to(dt64))
    steps = int(round(T / dt))
    every = max(1, steps // record)
    out = torch.empty(S, n, n, record, dtype=torch.float32, device=dev)
    rec = 0
    for it in range(steps):
        psi_h = w_h / lap_safe
        u = torch.fft.ifft2(2j * math.pi * ky * psi_h).real          # u =  d psi / dy
        v = torch.fft.ifft2(-2j * math.pi * kx * psi_h).real         # v = -d psi / dx
        wx = torch.fft.ifft2(2j * math.pi * kx * w_h).real
        wy = torch.fft.ifft2(2j * math.pi * ky * w_h).real
        adv_h = torch.fft.fft2(u * wx + v * wy) * dealias
        w_h = (w_h * (1.0 - 0.5 * dt * visc * lap) + dt * (f_h - adv_h)) / (1.0 + 0.5 * dt * visc * lap)
        if (it + 1) % every == 0 and rec < record:
            out[..., rec] = torch.fft.ifft2(w_h).real.float()
            rec += 1
    return out


# ------------------------------------------------------------------ the airfoil / pipe / elasticity / plasticity sets
def _mesh_size(full, r):
    return int(((full - 1) / r) + 1)


def split_mesh_fields(X, Y, q, train, test, r1=1, r2=1):
    """exp_airfoil.py:62-79 / exp_pipe.py:65-81 on loaded arrays: X, Y, q [S, H, W]; `train` / `test`: slices of the
    sample axis.  Returns (x_train [n, s1*s2, 2], y_train [n, s1*s2], x_test, y_test, s1, s2), float32, strided by
    (r1, r2) and cut to s1 x s2 = (H-1)/r1+1 x (W-1)/r2+1 points, flattened row-major."""
    xy = torch.stack([torch.tensor(np.asarray(X), dtype=torch.float), torch.tensor(np.asarray(Y), dtype=torch.float)], dim=-1)
    q = torch.tensor(np.asarray(q), dtype=torch.float)
    s1, s2 = _mesh_size(xy.shape[1], r1), _mesh_size(xy.shape[2], r2)
    cut = lambda t, sl: t[sl, ::r1, ::r2][:, :s1, :s2]
    x_train, x_test = cut(xy, train), cut(xy, test)
    y_train, y_test = cut(q, train), cut(q, test)
    return (x_train.reshape(x_train.shape[0], -1, 2), y_train.reshape(y_train.shape[0], -1),
            x_test.reshape(x_test.shape[0], -1, 2), y_test.reshape(y_test.shape[0], -1), s1, s2)


def airfoil_from_arrays(X, Y, Q, ntrain=1000, ntest=200, r1=1, r2=1):
    """exp_airfoil.py:62-79 on the loaded arrays (X, Y [S, 221, 51], Q [S, >= 5, 221, 51]): the target is channel 4 of Q; the
    mesh is strided by (r1, r2); train = the first `ntrain` samples, test = samples ntrain .. ntrain + ntest.  No
    normaliser: x and y are raw.  Returns x_train [n, N, 2], y_train [n, N], x_test, y_test, x_normalizer = y_normalizer =
    None, s1, s2."""
    x_train, y_train, x_test, y_test, s1, s2 = split_mesh_fields(X, Y, np.asarray(Q)[:, 4], slice(0, ntrain),
                                                                 slice(ntrain, ntrain + ntest), r1, r2)
    return dict(x_train=x_train, y_train=y_train, x_test=x_test, y_test=y_test, x_normalizer=None, y_normalizer=None,
                s1=s1, s2=s2)


def load_airfoil_npy(path, ntrain=1000, ntest=200, r1=1, r2=1):
    """exp_airfoil.py:50-79: NACA_Cylinder_{X,Y,Q}.npy under `path`, see `airfoil_from_arrays`."""
    X, Y, Q = (np.load(os.path.join(path, f"NACA_Cylinder_{k}.npy")) for k in "XYQ")
    return airfoil_from_arrays(X, Y, Q, ntrain, ntest, r1, r2)


PIPE_SAMPLES = 1200      # exp_pipe.py:58: the script's `N`; train / test are taken from the first N samples


def pipe_from_arrays(X, Y, Q, ntrain=1000, ntest=200, r1=1, r2=1):
    """exp_pipe.py:65-91 on the loaded arrays (X, Y [S, 129, 129], Q [S, >= 1, 129, 129]): the target is channel 0 of Q; the
    mesh is strided by (r1, r2); train = the first `ntrain`, test = the LAST `ntest` of the first N = 1200 samples.
    UnitTransformer on x (per coordinate) and on y (one mean / std), both fitted on the train split; x_train, x_test and
    y_train are encoded, y_test stays RAW."""
    n = PIPE_SAMPLES
    x_train, y_train, x_test, y_test, s1, s2 = split_mesh_fields(np.asarray(X)[:n], np.asarray(Y)[:n], np.asarray(Q)[:n, 0],
                                                                 slice(0, ntrain), slice(-ntest, None), r1, r2)
    xn, yn = UnitTransformer(x_train), UnitTransformer(y_train)
    return dict(x_train=xn.encode(x_train), y_train=yn.encode(y_train), x_test=xn.encode(x_test), y_test=y_test,
                x_normalizer=xn, y_normalizer=yn, s1=s1, s2=s2)


def load_pipe_npy(path, ntrain=1000, ntest=200, r1=1, r2=1):
    """exp_pipe.py:52-91: Pipe_{X,Y,Q}.npy under `path`, see `pipe_from_arrays`."""
    X, Y, Q = (np.load(os.path.join(path, f"Pipe_{k}.npy")) for k in "XYQ")
    return pipe_from_arrays(X, Y, Q, ntrain, ntest, r1, r2)


def elas_from_arrays(sigma, xy, ntrain=1000, ntest=200):
    """exp_elas.py:57-72 on the loaded arrays: sigma [N, S] -> [S, N], xy [N, 2, S] -> [S, N, 2]; train = the first
    `ntrain` samples, test = the LAST `ntest`; UnitTransformer on y only (fitted on the train split): y_train is encoded,
    y_test RAW, the point coordinates raw."""
    s = torch.tensor(np.asarray(sigma), dtype=torch.float).permute(1, 0)
    p = torch.tensor(np.asarray(xy), dtype=torch.float).permute(2, 0, 1)
    y_train = s[:ntrain]
    yn = UnitTransformer(y_train)
    return dict(x_train=p[:ntrain], y_train=yn.encode(y_train), x_test=p[-ntest:], y_test=s[-ntest:], x_normalizer=None,
                y_normalizer=yn, s1=None, s2=None)


ELAS_FILES = ("elasticity/Meshes/Random_UnitCell_sigma_10.npy", "elasticity/Meshes/Random_UnitCell_XY_10.npy")


def load_elas_npy(path, ntrain=1000, ntest=200):
    """exp_elas.py:54-72: <path>/elasticity/Meshes/Random_UnitCell_{sigma,XY}_10.npy, see `elas_from_arrays`."""
    return elas_from_arrays(np.load(os.path.join(path, ELAS_FILES[0])), np.load(os.path.join(path, ELAS_FILES[1])),
                            ntrain, ntest)


PLAS_MESH, PLAS_T, PLAS_DEFORMATION = (101, 31), 20, 4


def plas_from_mat(mat, ntrain=900, ntest=80):
    """exp_plas.py:105-137 on the loaded `.mat` dict: 'input' [S, 101] (the die profile) is repeated along the 31 mesh
    columns -> x [n, N, 1]; 'output' [S, 101, 31, T = 20, 4] is transposed to [..., 4, T] -> y [n, N, 4, T]; train = the
    first `ntrain`, test = the LAST `ntest`.  UnitTransformer on x only (fitted on the train split); y is raw.
    `pos` [1, N, 2] is the script's np.meshgrid(linspace(0, 1, 101), linspace(0, 1, 31)) raveled: ITS point order runs
    along the 101-axis fastest, while x and y are flattened with the 31-axis fastest; kept as the script has it.
    `t` [T] = linspace(0, 1, T)."""
    s1, s2 = PLAS_MESH
    inp = torch.tensor(np.asarray(mat["input"]), dtype=torch.float)
    out = torch.tensor(np.asarray(mat["output"]), dtype=torch.float).transpose(-2, -1)
    T = out.shape[-1]
    grow = lambda a: a[:, :s1].reshape(a.shape[0], s1, 1).repeat(1, 1, s2).reshape(a.shape[0], -1, 1)
    x_train, x_test = grow(inp[:ntrain]), grow(inp[-ntest:])
    y_train = out[:ntrain, :s1, :s2].reshape(ntrain, -1, PLAS_DEFORMATION, T)
    y_test = out[-ntest:, :s1, :s2].reshape(ntest, -1, PLAS_DEFORMATION, T)
    xn = UnitTransformer(x_train)
    return dict(x_train=xn.encode(x_train), y_train=y_train, x_test=xn.encode(x_test), y_test=y_test, x_normalizer=xn,
                y_normalizer=None, pos=grid_positions(s2, s1), t=torch.tensor(np.linspace(0, 1, T), dtype=torch.float),
                s1=s1, s2=s2, T=T)


def load_plas_mat(path, ntrain=900, ntest=80):
    """exp_plas.py:105: plas_N987_T20.mat ('input', 'output'), see `plas_from_mat`."""
    import scipy.io as scio
    return plas_from_mat(scio.loadmat(path), ntrain, ntest)


# ------------------------------------------------------------------------------ ns_velocity.py and its two siblings
VELOCITY_SIDE = 64      # ns_velocity.py:64: the crop size comes from this constant, not from the array


def split_velocity(arr, ntrain, ntest, T_in=10, T=10, r=1):
    """ns_velocity.py:63-97 (the same lines in ns_velocity_unrolling.py and ns_unrolling2_with_t.py) on the loaded array
    [S, H, W, >= T_in + T], whose columns interleave (vel_x, vel_y) per frame: h = int((64 - 1) / r + 1), spatial stride r,
    the [:h, :h] crop, points flattened row-major; the first `ntrain` samples train, the LAST `ntest` test; inputs are
    columns [0, T_in), targets [T_in, T_in + T).  Returns (h, train, test): ResidentDatasets of (pos, a, u) on the CPU,
    pos = grid_positions(h) repeated per sample."""
    arr = np.asarray(arr)
    h = int(((VELOCITY_SIDE - 1) / r) + 1)

    def cut(block, c0, c1):
        x = block[:, ::r, ::r, c0:c1][:, :h, :h, :]
        return torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1, x.shape[-1])))

    pos = grid_positions(h)
    sets = []
    for block, n in ((arr[:ntrain], ntrain), (arr[-ntest:], ntest)):
        sets.append(ResidentDataset(pos.repeat(n, 1, 1), cut(block, 0, T_in), cut(block, T_in, T_in + T)))
    return h, sets[0], sets[1]


def load_velocity_npy(path, ntrain, ntest, T_in=10, T=10, r=1):
    """`split_velocity` of the `.npy` file at `path` (the scripts' ns_50_20.npy / ns_20_20.npy)."""
    return split_velocity(np.load(path), ntrain, ntest, T_in, T, r)
