"""Host side of the time-folded latent-sequence iteration: the grouped z-score's symbols and refusals, the `groups` argument
of functional.zscore, the call sequence of `forward_windows` (both SequenSolver classes) and of the epoch loops
`fit_autoencoder` / `fit_sequensolver`, all through recording stand-ins: no GPU is touched."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

from test_benchmarks_host import _header_arity
from test_sequensolver_merged_host import TINY_ENCODER

NEW_SYMBOLS = ("pa2d_zscore_grouped_workspace", "pa2d_zscore_grouped_fwd", "pa2d_zscore_grouped_bwd", "pa2d_act_fwd")
ARG, UNSUP = 1001, 1002


# ---------------------------------------------------------------------------------------------- the C interface
@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_arity(name):
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    res, args = _lib.SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert res is (ctypes.c_size_t if name.endswith("workspace") else ctypes.c_int)
    assert len(args) == _header_arity(name)


def test_grouped_zscore_refusals_return_before_any_launch():
    """All pointers are NULL: every call below must return from its checks."""
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    f, b = lib.pa2d_zscore_grouped_fwd, lib.pa2d_zscore_grouped_bwd
    # fwd(x, ldx, y, stats, ws, ws_bytes, groups, rows_per_group, C, stream)
    assert f(0, 8, 0, 0, 0, 0, 2, 5, 6, 0) == UNSUP                  # C % 4 != 0
    assert f(0, 8, 0, 0, 0, 0, 0, 5, 8, 0) == ARG                    # groups < 1
    assert f(0, 4, 0, 0, 0, 0, 2, 5, 8, 0) == ARG                    # pitch < C
    assert f(0, 10, 0, 0, 0, 0, 2, 5, 8, 0) == ARG                   # pitch % 4 != 0
    assert f(0, 8, 0, 0, 0, 0, 70000, 5, 8, 0) == UNSUP              # more groups than a grid axis holds
    assert f(0, 256, 0, 0, 0, 0, 10, 1 << 19, 256, 0) == UNSUP       # 5 GiB over ALL groups (one group: 512 MiB)
    assert f(0, 256, 0, 0, 0, 0, 1, 1 << 19, 256, 0) == ARG          # that one group alone is in range: NULL operands
    assert f(0, 8, 0, 0, 0, 0, 3, 0, 8, 0) == 0                      # groups * rows_per_group = 0: a no-op
    assert f(0, 8, 0, 0, 0, 0, 2, 5, 8, 0) == ARG                    # NULL operands
    # bwd(dy, lddy, y, stats, dx, lddx, ws, ws_bytes, groups, rows_per_group, C, stream)
    assert b(0, 8, 0, 0, 0, 8, 0, 0, 2, 5, 6, 0) == UNSUP
    assert b(0, 8, 0, 0, 0, 8, 0, 0, 0, 5, 8, 0) == ARG
    assert b(0, 8, 0, 0, 0, 4, 0, 0, 2, 5, 8, 0) == ARG              # lddx < C
    assert b(0, 8, 0, 0, 0, 8, 0, 0, 3, 0, 8, 0) == 0
    assert b(0, 8, 0, 0, 0, 8, 0, 0, 2, 5, 8, 0) == ARG
    assert lib.pa2d_act_fwd(0, 0, 0, 1, 0) == 0 and lib.pa2d_act_fwd(0, 0, 5, 1, 0) == ARG


def test_grouped_workspace_is_groups_times_the_ungrouped_one_and_monotone():
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    ws, one = lib.pa2d_zscore_grouped_workspace, lib.pa2d_zscore_workspace
    for C in (4, 64, 256):
        prev = 0
        for rows in (1, 5, 70, 4099, 40000, 400000):
            assert ws(1, rows, C) == one(rows, C) and ws(7, rows, C) == 7 * one(rows, C)
            assert ws(3, rows, C) >= prev
            prev = ws(3, rows, C)
        assert [ws(g, 70, C) for g in (1, 2, 5, 10)] == sorted(ws(g, 70, C) for g in (1, 2, 5, 10))
    assert ws(0, 70, 64) == 0 and ws(2, 0, 64) == 0 and ws(2, 70, 6) == 0


def test_zscore_rejects_groups_that_do_not_divide_the_leading_dimension():
    from transformerbasednavierstokesolver_amd import functional as Fn
    x = torch.zeros(6, 5, 8)
    for bad in (4, 0, -1, 7):
        with pytest.raises(ValueError, match="groups"):
            Fn.zscore(x, groups=bad)
    with pytest.raises(ValueError, match="groups"):
        Fn.zscore(torch.zeros(8), groups=2)


def test_slice_predictor_rejects_groups_that_do_not_divide_the_batch(monkeypatch):
    from transformerbasednavierstokesolver_amd import SliceLearner as SL, functional as Fn
    v = SL.VorticitySliceLearner(C=16, M=8, T=3, H=8, W=8, n_hidden=32)
    monkeypatch.setattr(Fn, "conv3x3", lambda z, H, W, w, b, engine=None: z)
    preprocess = lambda t: torch.zeros(t.shape[0], t.shape[1], 32)
    with pytest.raises(ValueError, match="groups = 2 must divide the batch of 3"):
        SL.code_conditioned_slice_weights(torch.zeros(3, 64, 64), torch.zeros(3, 64, 3), torch.zeros(3, 1, 8, 16), preprocess,
                                          v.in_project_x, v.in_project_slice, v.temperature, 8, 8, 8, 16, None, groups=2)


# ---------------------------------------------------------------------------------------------- forward_windows
def _recording_encoder(m, calls):
    """encoder.encode stand-in: sample i of a call gets the code value 10 * frame + b (frame-major batches of B), and the
    cached slice weights hold the same number."""
    def encode(pos, frames):
        calls.append((tuple(pos.shape), tuple(frames.shape)))
        nB = frames.shape[0]
        val = frames[:, 0, 0]                                   # the frames carry their own label, see _labelled_seq
        m.encoder.set_attention_slice(val.reshape(nB, 1, 1, 1).expand(nB, 1, m.N, m.M).clone())
        return val.reshape(nB, 1, 1, 1).expand(nB, 1, m.M, m.C).clone()
    m.encoder.encode = encode


def _labelled_seq(B, N, F):
    """seq [B, N, F] whose frame f of sample b is the constant 10 * f + b."""
    f = torch.arange(F, dtype=torch.float32).reshape(1, 1, F)
    b = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1)
    return (10 * f + b).expand(B, N, F).clone()


def _stub_stages(monkeypatch, Fn):
    """de-slice -> the code's first value on every point; LayerNorm and the head pass it on."""
    monkeypatch.setattr(Fn, "deslice_weights", lambda code, sw: code[:, 0, 0, :1].reshape(-1, 1, 1).expand(-1, sw.shape[2], 4))
    monkeypatch.setattr(Fn, "layer_norm", lambda x, w, b: x)
    monkeypatch.setattr(Fn, "head", lambda x, w, b: x[..., :1])


@pytest.mark.parametrize("use_gt", [True, False])
def test_merged_forward_windows_call_sequence(monkeypatch, use_gt):
    from transformerbasednavierstokesolver_amd import SequenSolverMerged as SM, functional as Fn
    B, T, n = 2, 3, 4
    m = SM.SequenSolver(None, T=T, W=8, H=8, M=8, C=16, B=B, sequential_head=8, layers=2, encoder_config=TINY_ENCODER)
    m.pe.zero_()
    calls, seen = [], []
    _recording_encoder(m, calls)
    m._blocks = lambda tokens: tokens

    def spy(x, fx, code, preprocess, in_project_x, in_project_slice, temperature, H, W, M, C, engine, groups=1):
        seen.append((tuple(x.shape), fx.clone(), code.clone(), groups))
        return torch.zeros(x.shape[0], 1, H * W, M) + code[:, 0, 0, 0].reshape(-1, 1, 1, 1)

    monkeypatch.setattr(SM, "code_conditioned_slice_weights", spy)
    _stub_stages(monkeypatch, Fn)
    seq = _labelled_seq(B, 64, T + n)
    out = m.forward_windows(torch.zeros(B, 64, 64), seq, use_gt=use_gt)
    nframes = T + n if use_gt else T + n - 1
    assert calls == [((nframes * B, 64, 64), (nframes * B, 64, 1))]               # ONE encoder call, frame-major
    assert len(seen) == 1 and seen[0][0] == (n * B, 64, 64) and seen[0][3] == n    # groups = n reaches the z-scores
    fxw, code = seen[0][1], seen[0][2]
    for k in range(n):
        for b in range(B):
            assert torch.equal(fxw[k * B + b], seq[b, :, k:k + T])                 # call-major windows of true frames
            assert float(code[k * B + b, 0, 0, 0]) == 10 * (k + T - 1) + b         # the last token of window k
            assert float(out[b, 0, k]) == 10 * (k + T - 1) + b
    assert tuple(out.shape) == (B, 64, n)
    # what the eager loop leaves: the last call's code and slice weights, the encoder's cache at the last encoded frame
    assert tuple(m.code.shape) == (B, 1, 8, 16) and float(m.code[1, 0, 0, 0]) == 10 * (n + T - 2) + 1
    assert tuple(m.slice_weights.shape) == (B, 1, 64, 8)
    cached = m.encoder.get_attention_slice()
    assert tuple(cached.shape) == (B, 1, 64, 8) and float(cached[0, 0, 0, 0]) == 10 * (nframes - 1)
    with pytest.raises(ValueError, match="n >= 1"):
        m.forward_windows(torch.zeros(B, 64, 64), seq[..., :T], use_gt=use_gt)


@pytest.mark.parametrize("use_gt", [True, False])
def test_plain_forward_windows_call_sequence(monkeypatch, use_gt):
    from test_gpu_sequensolver import TINY_ENCODER as PLAIN_ENCODER
    from transformerbasednavierstokesolver_amd import SequenSolver as S, functional as Fn
    B, T, n = 3, 2, 3
    m = S.SequenSolver(None, T=T, W=5, H=6, M=8, C=16, B=B, layers=2, encoder_config=PLAIN_ENCODER)
    calls, predicted = [], []
    _recording_encoder(m, calls)
    m._blocks = lambda tokens: tokens
    monkeypatch.setattr(Fn, "code_slice_weights", lambda code, pos, *p: predicted.append((tuple(code.shape), tuple(pos.shape)))
                        or torch.full((code.shape[0], 1, 30, 8), -1.0))
    used = []
    monkeypatch.setattr(Fn, "deslice_weights", lambda code, sw: used.append(sw.clone())
                        or code[:, 0, 0, :1].reshape(-1, 1, 1).expand(-1, 30, 4))
    monkeypatch.setattr(Fn, "layer_norm", lambda x, w, b: x)
    monkeypatch.setattr(Fn, "head", lambda x, w, b: x[..., :1])
    seq = _labelled_seq(B, 30, T + n)
    out = m.forward_windows(torch.zeros(B, 30, 2), seq, use_gt=use_gt)
    nframes = T + n if use_gt else T + n - 1
    assert calls == [((nframes * B, 30, 2), (nframes * B, 30, 1))]
    assert tuple(out.shape) == (B, 30, n) and len(used) == 1
    for k in range(n):
        for b in range(B):
            assert float(out[b, 0, k]) == 10 * (k + T - 1) + b
            # use_gt: call k decodes with the cached slice weights of its TARGET frame T + k
            assert float(used[0][k * B + b, 0, 0, 0]) == (10 * (T + k) + b if use_gt else -1.0)
    assert predicted == ([] if use_gt else [((n * B, 8, 16), (n * B, 30, 2))])
    assert float(m.encoder.get_attention_slice()[0, 0, 0, 0]) == 10 * (nframes - 1)


def test_fold_calls_cuts_at_the_descriptor_extent():
    from transformerbasednavierstokesolver_amd.SequenSolver import fold_calls
    assert fold_calls(10, 1, 4096, 10, 512, 2048) == 10                     # the reference shape folds whole
    assert fold_calls(10, 64, 4096, 10, 512, 2048) == 7                     # 512 MiB per call: 7 fit under 4 GiB
    assert fold_calls(10, 1024, 4096, 10, 512, 2048) == 1                   # never below one call


# ---------------------------------------------------------------------------------------------- the epoch loops
class _Stub(nn.Module):
    def __init__(self, merged):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.T, self.freezes, self.modes = 10, [], []
        if merged:
            self.sequential_head = 16

    def freeze_attention(self):
        self.freezes.append(len(self.modes))

    def train(self, mode=True):
        self.modes.append(mode)
        return super().train(mode)

    def forward(self, x, fx=None):
        return fx * 0.5


@pytest.mark.parametrize("variant", ["plain", "merged"])
def test_fit_sequensolver_call_sequence_divisors_and_saves(monkeypatch, variant):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.data import ResidentDataset
    model = _Stub(variant == "merged")
    steps, rolls, saves = [], [], []

    def train_step(m, opt, sched, x, fx, yy, use_gt=True, max_grad_norm=None, grad_sync=None, fold_time=False):
        steps.append((len(m.freezes), use_gt, fold_time, tuple(x.shape), float(fx[0, 0, 0])))
        return torch.tensor(3.0), torch.tensor(5.0)

    def rollout(m, x, fx, yy, use_gt=True):
        rolls.append(use_gt)
        k = float(fx[0, 0, 0])
        return yy * 2, torch.tensor(7.0 + k), torch.tensor(11.0 + k)

    monkeypatch.setattr(harness, "sequensolver_train_step", train_step)
    monkeypatch.setattr(harness, "sequensolver_rollout", rollout)
    monkeypatch.setattr(harness, "_save_state", lambda module, path: saves.append(path))
    ntrain, ntest, epochs = 4, 3, 8
    train = ResidentDataset(torch.arange(ntrain).float().reshape(-1, 1, 1).expand(-1, 6, 10), torch.ones(ntrain, 6, 10))
    test = ResidentDataset(torch.arange(ntest).float().reshape(-1, 1, 1).expand(-1, 6, 10), torch.ones(ntest, 6, 10))
    orders = [list(range(ntrain))[::-1]] * epochs
    hist = harness.fit_sequensolver(model, None, None, torch.zeros(1, 6, 2), train, test, epochs=epochs, fold_time=True,
                                    epoch_orders=orders, save_path="ckpt.pt")
    assert len(hist) == epochs and len(steps) == epochs * ntrain and saves == ["ckpt.pt"]      # saved once, at the end
    assert [s[4] for s in steps[:ntrain]] == [3.0, 2.0, 1.0, 0.0]                               # the recorded order, B = 1
    assert all(s[2] is True and s[3] == (1, 6, 2) for s in steps)
    assert rolls == [True] * (epochs * ntest)                       # the test pass: use_gt=True, prediction feedback
    if variant == "plain":
        assert all(s[1] is True for s in steps)                     # `use_gt = False` of the script is never passed on
        # freeze_attention() at the start of every epoch from ep > 5 on, after model.train()
        assert [s[0] for s in steps[::ntrain]] == [0, 0, 0, 0, 0, 0, 1, 2]
        last = float(ntest - 1)                                     # both test metrics are the LAST batch's alone
        want = dict(train_step=3.0 * ntrain / ntrain / 10, train_full=5.0 * ntrain / ntrain,
                    test_step=(7.0 + last) / ntest / 10, test_full=(11.0 + last) / ntest)
    else:
        assert all(s[1] is False for s in steps) and model.freezes == []
        ksum = sum(range(ntest))
        want = dict(train_step=3.0 / 10, train_full=5.0, test_step=(7.0 * ntest + ksum) / ntest / 10,
                    test_full=(11.0 * ntest + ksum) / ntest, test_first=float(ntest) / ntest)   # ||2 - 1|| / ||1|| per sample
    assert hist[0].keys() == want.keys()
    for k, v in want.items():
        assert hist[-1][k] == pytest.approx(v, rel=1e-12), k
    with pytest.raises(TypeError, match="unexpected"):
        harness.fit_sequensolver(model, None, None, torch.zeros(1, 6, 2), train, test, epochs=1, freeze_at=3)


def test_fit_autoencoder_divisors_and_save_cadence(monkeypatch):
    from transformerbasednavierstokesolver_amd import data, harness
    import numpy as np
    u = np.arange(5 * 4 * 4 * 20, dtype=np.float32).reshape(5, 4, 4, 20) + 1.0
    d = data.split_ns_all_frames(u, ntrain=3, ntest=2)
    # the script's reshape, no transpose: [n, N, F] -> [n * F, N, 1] of the same memory
    assert tuple(d["train"].shape) == (60, 16, 1) and tuple(d["test"].shape) == (40, 16, 1) and d["h"] == 4
    assert torch.equal(d["train"].reshape(3, -1), torch.from_numpy(u[:3].reshape(3, -1)))
    assert torch.equal(d["test"].reshape(2, -1), torch.from_numpy(u[-2:].reshape(2, -1)))
    seen, saves = [], []

    def step(m, opt, sched, x, fx, max_grad_norm=None, grad_sync=None):
        seen.append((tuple(x.shape), tuple(fx.shape)))
        return torch.tensor(2.0)

    monkeypatch.setattr(harness, "autoencoder_train_step", step)
    monkeypatch.setattr(harness, "_save_state", lambda module, path: saves.append(path))
    model = _Stub(False)
    hist = harness.fit_autoencoder(model, None, None, d, epochs=102, batch_size=8, ntrain=3, ntest=2, save_name="enc")
    assert seen[:8] == [((8, 16, 2), (8, 16, 1))] * 7 + [((4, 16, 2), (4, 16, 1))]      # 60 frames: the short batch is kept
    # train: 8 batches of 2.0; test: model returns fx / 2, so every one of the 40 frames has rel-L2 0.5
    assert hist[0] == dict(train_step=pytest.approx(16.0 / 3 / 10), test_step=pytest.approx(20.0 / 2 / 10))
    path = os.path.join("sequential_checkpoints", "enc.pt")
    assert saves == [path] * 3                                                            # ep 0, ep 100 and the end


def test_frozen_parameters_leave_the_active_ranges():
    from transformerbasednavierstokesolver_amd.ddp import FlatGradSync
    ps = [nn.Parameter(torch.zeros(n)) for n in (4, 6, 8, 3)]
    sync = FlatGradSync(ps)
    sync.touched = [True] * 4
    assert sync.active_ranges() == [(0, sync.total)]
    ps[1].requires_grad = False
    assert sync.offsets == [0, 4, 12, 20] and sync.total == 24          # slots are padded to 4 floats
    assert sync.active_ranges() == [(0, 4), (12, 24)]
    ps[3].requires_grad = False
    assert sync.active_ranges() == [(0, 4), (12, 20)]


def test_train_drivers_are_untouched():
    from transformerbasednavierstokesolver_amd import train, train_sequence
    assert train.DRIVERS == ("ns", "unrolled", "darcy", "airfoil", "pipe", "elas", "plas")
    assert train_sequence.DRIVERS == ("autoencoder", "sequensolver", "sequensolver_merged")


# ---------------------------------------------------------------------------------------------- the command line
# auto_encoder.py:13-31, flag by flag: (option string, type, default)
AUTO_ENCODER_FLAGS = [
    ("--lr", float, 1e-3), ("--epochs", int, 30), ("--weight_decay", float, 1e-5), ("--model", str, "Transolver_2D"),
    ("--n-hidden", int, 64), ("--n-layers", int, 3), ("--n-heads", int, 4), ("--batch-size", int, 8), ("--gpu", str, "0"),
    ("--max_grad_norm", float, None), ("--downsample", int, 1), ("--mlp_ratio", int, 1), ("--dropout", float, 0.0),
    ("--unified_pos", int, 0), ("--ref", int, 8), ("--slice_num", int, 32), ("--eval", int, 0),
    ("--save_name", str, "ns_2d_UniPDE"), ("--data_path", str, "/data/fno"),
]
# SequenSolverMerged.py:530-533
MERGED_FLAGS = [("--eval", int, 1), ("--epochs", int, 10), ("--save_name", str, "buff"), ("--sim_num", int, 10)]
# SequenSolver.py has no parser: train()'s hard-coded epochs, save_name, ntrain (:471-476) and __main__'s train(eval=True)
PLAIN_FLAGS = [("--eval", int, 1), ("--epochs", int, 10), ("--save_name", str, "tokenizer_ep10_sim10_2"), ("--sim_num", int, 10)]


def _table(parser):
    return [(a.option_strings[0], a.type, a.default) for a in parser._actions if a.dest != "help"]


@pytest.mark.parametrize("driver,flags,ntest", [("autoencoder", AUTO_ENCODER_FLAGS, 20), ("sequensolver_merged", MERGED_FLAGS, 10),
                                                ("sequensolver", PLAIN_FLAGS, 2)])
def test_train_sequence_parser_defaults_equal_the_scripts(driver, flags, ntest):
    from transformerbasednavierstokesolver_amd import train_sequence as ts
    table = _table(ts.build_parser(driver))
    assert table[:len(flags)] == flags                                  # the script's own flags first, in its order
    added = {name: (typ, default) for name, typ, default in table[len(flags):]}
    assert added["--ntest"] == (int, ntest) and added["--engine"] == (str, None) and added["--driver"][1] == driver
    assert "--data_path" in dict((n, 0) for n, _, _ in table)
    args = ts.parse_args(["--driver", driver])
    assert args.driver == driver and args.ntest == ntest
    if driver == "autoencoder":
        assert added["--ntrain"] == (int, 100) and not hasattr(args, "fold_time")
    else:
        assert added["--transolver_path"] == (str, os.path.join("sequential_checkpoints", "encoder_ep20_head_1.pt"))
        # folded by default: the folded median lies outside the eager range at both measured shapes
        assert added["--fold_time"] == (int, 1) and args.fold_time == 1
        assert ("--slice_learner_path" in added) == (driver == "sequensolver")
    with pytest.raises(SystemExit):
        ts.parse_args([])                                               # --driver is required
    assert (ts.LR, ts.WEIGHT_DECAY, ts.BATCH_SIZE, ts.T_IN, ts.T_OUT, ts.LAYERS, ts.SEQUENTIAL_HEAD) == (1e-3, 1e-5, 1, 10, 10, 8, 16)
    assert ts.GEOMETRY == dict(H=64, W=64, M=16, C=32)


def test_train_sequence_hands_the_flags_to_the_loops(monkeypatch, tmp_path):
    """--driver sequensolver_merged end to end on the host, with the model, the device and the loop replaced by recorders."""
    import numpy as np
    import scipy.io as scio
    from transformerbasednavierstokesolver_amd import SequenSolverMerged, cli, harness, train_sequence as ts
    u = np.random.default_rng(0).standard_normal((5, 64, 64, 20)).astype(np.float32)
    scio.savemat(str(tmp_path / "NavierStokes_V1e-5_N1200_T20.mat"), {"u": u})
    seen = {}

    class Model(_Stub):
        def __init__(self, path, **kw):
            super().__init__(True)
            seen["model"] = (path, kw)

    def fit(model, opt, sched, pos, train_set, test_set, **kw):
        seen["fit"] = (tuple(pos.shape), len(train_set), len(test_set), kw)
        return []

    monkeypatch.setattr(SequenSolverMerged, "SequenSolver", Model)
    monkeypatch.setattr(cli, "device", lambda args: torch.device("cpu"))
    monkeypatch.setattr(cli, "optim", lambda model, *a, **k: (type("O", (), {"sync": None})(), None))
    monkeypatch.setattr(harness, "fit_sequensolver", fit)
    ts.main(["--driver", "sequensolver_merged", "--eval", "0", "--sim_num", "3", "--ntest", "2", "--epochs", "4",
             "--data_path", str(tmp_path), "--transolver_path", "enc.pt", "--save_name", "run"])
    assert seen["model"] == ("enc.pt", dict(T=10, B=1, layers=8, sequential_head=16, H=64, W=64, M=16, C=32))
    pos_shape, ntrain, ntest, kw = seen["fit"]
    assert (pos_shape, ntrain, ntest) == ((1, 4096, 64), 3, 2)
    assert kw["epochs"] == 4 and kw["variant"] == "merged" and kw["fold_time"] is True and kw["batch_size"] == 1
    assert kw["save_path"] == os.path.join("./sequential_checkpoints", "run.pt") and kw["Tin"] == 10


def test_unified_positions_are_the_slice_learners_table():
    from transformerbasednavierstokesolver_amd import data
    from transformerbasednavierstokesolver_amd.SliceLearner import SliceLearner
    import sequensolver_merged_restatement as RM
    pos = data.unified_positions(8, 8)
    assert tuple(pos.shape) == (1, 64, 64) and pos.dtype == torch.float32
    sl = SliceLearner(unified_pos=True, H=8, W=8, n_hidden=32)
    assert torch.equal(pos, sl.get_grid().reshape(1, 64, 64))
    assert float((pos - torch.from_numpy(RM.unified_positions(8, 8))).abs().max()) < 1e-6
