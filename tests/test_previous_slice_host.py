"""Host side of the slice-learner trainers: the symbols and refusals of pa2d_prev_slice_entry_*, the state_dict and the
column split of `PreviousSliceLearner`, the fixture G23 against the float64 restatement, and the call sequences of
`SequenSolver.code_windows`, the folded steps, `fit_slice_learner` and the `train_slices.py` flag table, all through
recording stand-ins: no GPU is touched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
import previous_slice_restatement as R
from test_benchmarks_host import _header_arity
from test_gpu_sequensolver import TINY_ENCODER
from test_sequence_fold_host import _labelled_seq, _recording_encoder

NEW_SYMBOLS = ("pa2d_prev_slice_entry_workspace", "pa2d_prev_slice_entry_fwd", "pa2d_prev_slice_entry_bwd")
ARG, UNSUP, WS = 1001, 1002, 1003
G23 = os.path.join(GOLDEN, "G23_previous_slice.npz")


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


def test_entry_refusals_return_before_any_launch():
    """All pointers are NULL (or a made-up aligned address that is never read): every call returns from its checks."""
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    f, b, ws = lib.pa2d_prev_slice_entry_fwd, lib.pa2d_prev_slice_entry_bwd, lib.pa2d_prev_slice_entry_workspace
    # fwd(sw, wsw, tb, h0, B, N, M, H, act, stream)
    assert f(0, 0, 0, 0, 2, 5, 65, 8, 1, 0) == UNSUP                     # M = 65
    assert f(0, 0, 0, 0, 2, 5, 0, 8, 1, 0) == ARG                        # M = 0
    assert f(0, 0, 0, 0, 2, 5, 16, 6, 1, 0) == UNSUP                     # H % 4 != 0
    assert f(0, 0, 0, 0, 2, 5, 16, 8, 9, 0) == ARG                       # no such activation
    assert f(0, 0, 0, 0, -1, 5, 16, 8, 1, 0) == ARG
    assert f(0, 0, 0, 0, 125, 4096, 16, 2112, 1, 0) == UNSUP             # h0 = 4.03 GiB: past the buffer addressing
    assert f(0, 0, 0, 0, 124, 4096, 16, 2112, 1, 0) == ARG               # just under it: NULL operands
    assert f(0, 0, 0, 0, 1 << 20, 64, 64, 8, 1, 0) == UNSUP              # sw = 16 GiB
    assert f(0, 0, 0, 0, 0, 5, 16, 8, 1, 0) == 0 and f(0, 0, 0, 0, 2, 0, 16, 8, 1, 0) == 0      # empty: a no-op
    assert f(0, 0, 0, 0, 2, 5, 16, 8, 1, 0) == ARG                       # NULL operands
    assert f(16, 16, 24, 16, 2, 5, 16, 8, 1, 0) == ARG                   # tb not 16-byte aligned
    # bwd(dh0, sw, wsw, tb, dwsw, dtb, ws, ws_bytes, B, N, M, H, act, stream)
    assert b(0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 65, 8, 1, 0) == UNSUP
    assert b(0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 16, 6, 1, 0) == UNSUP
    assert b(0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 16, 8, 1, 0) == ARG
    assert b(0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 16, 8, 1, 0) == ARG           # even an empty problem needs its two outputs
    assert b(16, 16, 16, 16, 16, 16, 16, ws(2, 5, 16, 8) - 1, 2, 5, 16, 8, 1, 0) == WS
    # one record per (sample, chunk of 128 rows): H M floats of dWsw and H of dtb
    assert ws(2, 5, 16, 8) == 4 * 2 * 1 * (8 * 16 + 8) and ws(3, 130, 4, 64) == 4 * 3 * 2 * (64 * 4 + 64)
    assert ws(1, 4096, 16, 2112) == 4 * 32 * (2112 * 16 + 2112)
    assert ws(0, 5, 16, 8) == 0 and ws(2, 0, 16, 8) == 0


def test_wrappers_refuse_on_the_host():
    from transformerbasednavierstokesolver_amd import functional as Fn, ops
    sw, wsw, tb = torch.rand(2, 5, 4), torch.randn(8, 4), torch.randn(2, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.prev_slice_entry_fwd(sw, wsw, tb, "gelu")                   # no CPU path
    with pytest.raises(ValueError, match="no gradient flows to `sw`"):
        Fn.prev_slice_entry(sw.clone().requires_grad_(True), wsw, tb, "gelu")
    assert ops.PREV_SLICE_MAX_M == 64


# ---------------------------------------------------------------------------------------------- the module
def test_state_dict_is_the_references_weight_projection_form_slice():
    from transformerbasednavierstokesolver_amd.SliceLearner import FUSED_ENTRY_DEFAULT, PreviousSliceLearner
    m = PreviousSliceLearner()
    want = R.previous_slice_shapes(32, 16)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert dict(want)[R.PREFIX + "linear_pre.0.weight"] == (2112, 528) and dict(want)[R.PREFIX + "linear_post.weight"] == (16, 2112)
    g = np.load(G23)                                                      # the keys and shapes the reference's module has
    assert [str(k) for k in g["keys"]] == [k for k, _ in want]
    assert [tuple(s) for s in json.loads(str(g["shapes"]))] == [s for _, s in want]
    assert m.fused_entry is FUSED_ENTRY_DEFAULT and m.weight_projection_form_slice.res and m.weight_projection_form_slice.act_name == "gelu"
    # a reference LearnSlice state_dict (which holds many more modules) loads with strict=False and no missing key
    sd = dict(m.state_dict(), **{"weight_projection.linear_post.bias": torch.zeros(1), "temperature": torch.ones(1, 1, 1, 1)})
    res = m.load_state_dict(sd, strict=False)
    assert not res.missing_keys and sorted(res.unexpected_keys) == ["temperature", "weight_projection.linear_post.bias"]
    with pytest.raises(NotImplementedError, match="bf16"):
        m.set_engine("bf16s")
    # default initialisation, as the reference: PyTorch's uniform(+-1/sqrt(fan_in)), not the Transolver trunc_normal(0.02)
    w = m.weight_projection_form_slice.linear_pre[0].weight.detach()
    assert float(w.abs().max()) <= 528 ** -0.5 and float(w.std()) > 0.02


def _cpu_stages(monkeypatch, Fn, seen):
    """functional.linear and functional.prev_slice_entry in plain torch on the CPU, recording their operands."""
    import torch.nn.functional as F

    def linear(x, w, b, act, engine=None):
        seen.append(("linear", tuple(x.shape), tuple(w.shape), act))
        y = x @ w.t() + (0 if b is None else b)
        return F.gelu(y) if act == "gelu" else y

    def entry(sw, wsw, tb, act, fused=True, engine=None):
        seen.append(("entry", tuple(sw.shape), tuple(wsw.shape), tuple(tb.shape), act, fused))
        return F.gelu(sw @ wsw.t() + tb[:, None, :])

    monkeypatch.setattr(Fn, "linear", linear)
    monkeypatch.setattr(Fn, "prev_slice_entry", entry)


@pytest.mark.parametrize("B,N,M,C", [(1, 7, 4, 3), (3, 5, 8, 2), (2, 9, 3, 3)])
def test_column_split_equals_the_explicit_concatenation(monkeypatch, B, N, M, C):
    """float64 torch on the CPU: the module's split (first M columns on the slice weights, the rest on the token flattened
    in (m, c) order, one row per sample) against the reference's lines on the [B, 1, N, M + M C] concatenation.  (2, 9, 3, 3):
    M C = 9 is no multiple of 4, so the row GEMM's operands are zero-padded."""
    from transformerbasednavierstokesolver_amd import SliceLearner as SL, functional as Fn
    torch.manual_seed(5)
    m = SL.PreviousSliceLearner(C=C, M=M).double()
    seen = []
    _cpu_stages(monkeypatch, Fn, seen)
    prev = torch.softmax(torch.randn(B, 1, N, M, dtype=torch.float64), -1)
    token = torch.randn(B, 1, M, C, dtype=torch.float64)
    got = m(prev, token)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    want = R.forward_previous_slice(sd, prev, token)
    assert tuple(got.shape) == (B, 1, N, M)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((R.forward_split(sd, prev, token) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    H, K = 4 * (M + M * C), M * C + (-M * C) % 4
    assert seen == [("linear", (B, K), (H, K), None), ("entry", (B, N, M), (H, M), (B, H), "gelu", SL.FUSED_ENTRY_DEFAULT),
                    ("linear", (B, N, H), (H, H), "gelu"), ("linear", (B, N, H), (M, H), None)]
    # a token whose samples are swapped gives another result: the per-sample row is per sample
    if B > 1:
        assert float((m(prev, token.flip(0)) - want).abs().max()) > 1e-6
    with pytest.raises(ValueError, match="previous slice weights"):
        m(prev[..., :-1], token)
    with pytest.raises(ValueError, match="token"):
        m(prev, token[:, :, :-1])


def test_restatement_meets_the_fixture():
    """The float64 restatement (concatenation and split) at the reference's shape against the reference's own run, with the
    weights regenerated from their seeds and verified by the recorded sums."""
    import torch.nn.functional as F
    g = np.load(G23)
    sd, prev, token, target = R.draw_g23()
    np.testing.assert_allclose([np.sum(sd[str(k)], dtype=np.float64) for k in g["keys"]], g["sums"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose([np.sum(a, dtype=np.float64) for a in (prev, token, target)], g["input_sums"], rtol=1e-12)
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    stride, rows = int(g["point_stride"]), int(g["row_stride"])
    for fn in (R.forward_previous_slice, R.forward_split):
        for p in P.values():
            p.grad = None
        out = fn(P, torch.from_numpy(prev).double(), torch.from_numpy(token).double())
        assert R.rel(out.detach()[0, 0, ::stride], g["out.f64"]) <= 1e-12
        assert abs(float(out.detach().norm()) - float(g["out.norm"])) <= 1e-12 * float(g["out.norm"])
        loss = F.mse_loss(out, torch.from_numpy(target).double())
        assert abs(float(loss) - float(g["loss.f64"])) <= 1e-12 * float(g["loss.f64"])
        loss.backward()
        for k in [str(s) for s in g["whole_keys"]]:
            assert R.rel(P[k].grad, g["grad." + k]) <= 1e-11, k
        for k in [str(s) for s in g["row_keys"]]:
            assert R.rel(P[k].grad[::rows], g["grad." + k]) <= 1e-11, k
            assert abs(float(P[k].grad.norm()) - float(g["grad." + k + ".norm"])) <= 1e-11 * float(g["grad." + k + ".norm"])
    # the fixture's own float32 run deviates by what float32 does, not more
    assert R.rel(g["out.f32"], g["out.f64"]) < 1e-5 and 0 < float(g["fp32_self_error.out"]) < 1e-5


# ---------------------------------------------------------------------------------------------- code_windows
def _tiny_solver(Bsz=2, T=2):
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    m = SequenSolver(None, T=T, W=5, H=6, M=8, C=16, B=Bsz, layers=2, encoder_config=TINY_ENCODER)
    calls = []
    _recording_encoder(m, calls)
    m._blocks = lambda tokens: tokens
    return m, calls


def test_code_windows_encodes_every_frame_once():
    Bsz, T, n = 2, 2, 3
    m, calls = _tiny_solver(Bsz, T)
    m.code, marker = "untouched", m.slice_weights
    seq = _labelled_seq(Bsz, 30, T + n)
    codes, slices = m.code_windows(torch.zeros(Bsz, 30, 2), seq)
    assert calls == [(((T + n) * Bsz, 30, 2), ((T + n) * Bsz, 30, 1))]            # ONE encoder call, frame-major
    assert tuple(codes.shape) == (n, Bsz, 1, 8, 16) and tuple(slices.shape) == ((T + n) * Bsz, 1, 30, 8)
    for k in range(n):
        for b in range(Bsz):
            assert float(codes[k, b, 0, 0, 0]) == 10 * (k + T - 1) + b              # the last token of window k
    for f in range(T + n):
        for b in range(Bsz):
            assert float(slices[f * Bsz + b, 0, 0, 0]) == 10 * f + b               # frame f is block f of the table
    # what the eager loops leave: the encoder's cache at the last window's last frame; code / slice_weights untouched
    cached = m.encoder.get_attention_slice()
    assert tuple(cached.shape) == (Bsz, 1, 30, 8) and float(cached[1, 0, 0, 0]) == 10 * (T + n - 2) + 1
    assert m.code == "untouched" and m.slice_weights is marker
    with pytest.raises(ValueError, match="n >= 1"):
        m.code_windows(torch.zeros(Bsz, 30, 2), seq[..., :T])


def test_code_windows_cuts_the_fold(monkeypatch):
    from transformerbasednavierstokesolver_amd import SequenSolver as S
    m, _ = _tiny_solver(2, 2)
    sizes, blocks = [], []
    monkeypatch.setattr(S, "fold_calls", lambda n, *a: sizes.append(n) or 2)
    m._blocks = lambda tokens: blocks.append(tokens.shape[0]) or tokens
    codes, _ = m.code_windows(torch.zeros(2, 30, 2), _labelled_seq(2, 30, 5))
    assert sizes == [3] and blocks == [4, 2] and tuple(codes.shape) == (3, 2, 1, 8, 16)
    assert [float(codes[k, 1, 0, 0, 0]) for k in range(3)] == [11.0, 21.0, 31.0]


# ---------------------------------------------------------------------------------------------- the folded steps
class _Recorder(nn.Module):
    """A slice learner that records what each call hands it and returns w * (its first argument's label)."""

    def __init__(self, kind):
        super().__init__()
        self.w = nn.Parameter(torch.ones(1))
        self.seen = []
        if kind == "previous":
            self.weight_projection_form_slice = nn.Module()
            self.weight_projection_form_slice.n_hidden = 544
        elif kind == "vorticity":
            self.in_project_x, self.use_code_for_vorticity, self.n_hidden, self.concatenated = nn.Identity(), True, 32, 160
        else:
            self.weight_projection, self.use_vorticity = nn.Identity(), 1

    def forward(self, a, b, code=None):
        return self.forward_folded(a, b, code, 1)

    def forward_folded(self, a, b, code=None, groups=1):
        self.seen.append(("forward", a.detach().clone(), b.detach().clone(), None if code is None else code.detach().clone(), groups))
        n = a.shape[0]
        return self.w * torch.ones(n, 1, 30, 8)

    def get_slice_weight(self, code, x, fx, use_vorticity=0):
        self.seen.append(("get_slice_weight", code.detach().clone(), fx.detach().clone(), use_vorticity))
        return self.w * torch.ones(code.shape[0], 1, 30, 8)


def _folded_step(monkeypatch, kind):
    from transformerbasednavierstokesolver_amd import functional as Fn, harness
    Bsz, T, n = 2, 2, 3
    solver, calls = _tiny_solver(Bsz, T)
    model = _Recorder(kind)
    targets = []
    monkeypatch.setattr(Fn, "slice_mse", lambda sw, target: targets.append(target.detach().clone()) or ((sw - target) ** 2).mean(-1).sum())
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    steps = []
    opt.register_step_post_hook(lambda *a: steps.append(len(targets)))
    seq = _labelled_seq(Bsz, 30, T + n)
    fn = {"previous": harness.previous_slice_train_step, "vorticity": harness.slice_predictor_train_step}.get(kind)
    if fn is None:
        out = harness.learnslice_train_step(model, opt, None, solver, torch.zeros(Bsz, 30, 2), seq[..., :T], seq[..., T:], 1, fold_time=True)
    else:
        out = fn(model, opt, None, solver, torch.zeros(Bsz, 30, 2), seq[..., :T], seq[..., T:], fold_time=True)
    assert calls == [(((T + n) * Bsz, 30, 2), ((T + n) * Bsz, 30, 1))]            # every frame encoded once, whatever the kind
    return model, targets, steps, out, seq, (Bsz, T, n)


def test_folded_previous_step_pairs_each_call_with_its_frames(monkeypatch):
    model, targets, steps, loss, seq, (Bsz, T, n) = _folded_step(monkeypatch, "previous")
    assert len(model.seen) == 1 and steps == [n]                                   # ONE forward on n*B samples, one step
    _, prev, code, _, _ = model.seen[0]
    assert tuple(prev.shape) == (n * Bsz, 1, 30, 8) and tuple(code.shape) == (n * Bsz, 1, 8, 16)
    for k in range(n):
        assert tuple(targets[k].shape) == (Bsz, 1, 30, 8)
        for b in range(Bsz):
            assert float(targets[k][b, 0, 0, 0]) == 10 * (T + k) + b               # target: frame T + k
            assert float(prev[k * Bsz + b, 0, 0, 0]) == 10 * (T + k - 1) + b       # previous slice: frame T + k - 1
            assert float(code[k * Bsz + b, 0, 0, 0]) == 10 * (T + k - 1) + b       # code of window k (identity blocks: its last token)
    want = sum(((1.0 - (10.0 * (T + k) + b)) ** 2) * 30 for k in range(n) for b in range(Bsz)) / (Bsz * 30)
    assert float(loss) == pytest.approx(want, rel=1e-6)                            # the terms summed, each / (B N)


def test_folded_vorticity_step_is_one_call_major_forward_with_per_call_groups(monkeypatch):
    model, targets, steps, _, seq, (Bsz, T, n) = _folded_step(monkeypatch, "vorticity")
    assert len(model.seen) == 1 and steps == [n]
    _, x, wins, code, groups = model.seen[0]
    assert groups == n and tuple(x.shape) == (n * Bsz, 30, 2)
    for k in range(n):
        for b in range(Bsz):
            assert torch.equal(wins[k * Bsz + b], seq[b, :, k:k + T])              # call-major windows of true frames
            assert float(code[k * Bsz + b, 0, 0, 0]) == 10 * (T + k - 1) + b
            assert float(targets[k][b, 0, 0, 0]) == 10 * (T + k) + b


def test_folded_learnslice_step_keeps_one_optimizer_step_per_frame(monkeypatch):
    model, targets, steps, losses, seq, (Bsz, T, n) = _folded_step(monkeypatch, "learnslice")
    assert len(losses) == n and steps == [1, 2, 3]                                  # a step after every frame's loss
    assert [s[0] for s in model.seen] == ["get_slice_weight"] * n
    for k, (_, code, fx, use_vorticity) in enumerate(model.seen):
        assert use_vorticity == 1 and torch.equal(fx, seq[..., k:k + T])           # window k's point features
        for b in range(Bsz):
            assert float(code[b, 0, 0, 0]) == 10 * (T + k - 1) + b and float(targets[k][b, 0, 0, 0]) == 10 * (T + k) + b


def test_folded_steps_refuse_a_window_of_another_length():
    from transformerbasednavierstokesolver_amd import harness
    solver, _ = _tiny_solver(2, 2)
    seq = _labelled_seq(2, 30, 6)
    with pytest.raises(ValueError, match="reads T = 2"):
        harness.previous_slice_train_step(_Recorder("previous"), None, None, solver, torch.zeros(2, 30, 2), seq[..., :3], seq[..., 3:],
                                          fold_time=True)


# ---------------------------------------------------------------------------------------------- the epoch loop
@pytest.mark.parametrize("kind", ["learnslice", "vorticity", "previous"])
def test_fit_slice_learner_call_sequence_divisors_and_saves(monkeypatch, kind):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.data import ResidentDataset
    model, solver = _Recorder(kind), _Recorder("previous")
    steps, tests, saves = [], [], []

    def ls_step(m, opt, sched, ss, x, fx, yy, use_vorticity, max_grad_norm=None, grad_sync=None, fold_time=False):
        steps.append(("learnslice", use_vorticity, fold_time, tuple(x.shape), float(fx[0, 0, 0])))
        return [torch.tensor(1.0)] * yy.shape[-1]

    def sp_step(m, opt, sched, ss, x, fx, yy, max_grad_norm=None, grad_sync=None, fold_time=False):
        steps.append(("vorticity", None, fold_time, tuple(x.shape), float(fx[0, 0, 0])))
        return torch.tensor(3.0)

    def pv_step(m, opt, sched, ss, x, fx, yy, max_grad_norm=None, grad_sync=None, fold_time=False):
        steps.append(("previous", None, fold_time, tuple(x.shape), float(fx[0, 0, 0])))
        return torch.tensor(5.0)

    def test_loss(k, m, ss, x, fx, yy, use_vorticity=0):
        tests.append((k, m.training, use_vorticity))
        return torch.tensor(20.0)

    monkeypatch.setattr(harness, "learnslice_train_step", ls_step)
    monkeypatch.setattr(harness, "slice_predictor_train_step", sp_step)
    monkeypatch.setattr(harness, "previous_slice_train_step", pv_step)
    monkeypatch.setattr(harness, "slice_learner_test_loss", test_loss)
    monkeypatch.setattr(harness, "_save_state", lambda module, path: saves.append((module is model, path)))
    ntrain, ntest, epochs, Tout = 4, 3, 2, 10
    train = ResidentDataset(torch.arange(ntrain).float().reshape(-1, 1, 1).expand(-1, 6, 10), torch.ones(ntrain, 6, Tout))
    test = ResidentDataset(torch.arange(ntest).float().reshape(-1, 1, 1).expand(-1, 6, 10), torch.ones(ntest, 6, Tout))
    hist = harness.fit_slice_learner(model, None, None, solver, torch.zeros(1, 6, 2), train, test, epochs=epochs, fold_time=True,
                                     epoch_orders=[list(range(ntrain))[::-1]] * epochs, save_path="ckpt.pt")
    assert harness.slice_learner_kind(model) == kind                               # the default kind: by the model's class
    assert len(steps) == epochs * ntrain and all(s[0] == kind and s[2] is True and s[3] == (1, 6, 2) for s in steps)
    assert [s[4] for s in steps[:ntrain]] == [3.0, 2.0, 1.0, 0.0]                  # the recorded order, batch size 1
    assert tests == [(kind, False, 1 if kind == "learnslice" else 0)] * (epochs * ntest)      # eval mode; the model's own flag
    assert saves == [(True, "ckpt.pt")] * (epochs + 1)                             # after every epoch, as the scripts; and the end
    want = {"learnslice": dict(train=(Tout * 1.0 / Tout) * ntrain / ntrain, test=(20.0 / Tout) * ntest / ntrain),   # / len(TRAIN loader)
            "vorticity": dict(train=3.0 * ntrain, test=20.0 * ntest / ntest),
            "previous": dict(train=5.0 * ntrain, test=20.0 * ntest)}[kind]
    assert hist[0].keys() == want.keys()
    for k, v in want.items():
        assert hist[-1][k] == pytest.approx(v, rel=1e-12), k
    with pytest.raises(ValueError, match="kind"):
        harness.fit_slice_learner(model, None, None, solver, torch.zeros(1, 6, 2), train, test, epochs=1, kind="other")
    with pytest.raises(TypeError, match="none of the slice learners"):
        harness.slice_learner_kind(nn.Linear(2, 2))


def test_previous_test_pass_never_slides_its_window(monkeypatch):
    """The script's test loop of train_from_previous does not update fx: code and previous slice are the first window's on
    every frame, only the target changes."""
    from transformerbasednavierstokesolver_amd import functional as Fn, harness
    Bsz, T, n = 2, 2, 3
    solver, calls = _tiny_solver(Bsz, T)
    model = _Recorder("previous")
    targets = []
    monkeypatch.setattr(Fn, "slice_mse", lambda sw, target: targets.append(target.detach().clone()) or ((sw - target) ** 2).mean(-1).sum())
    seq = _labelled_seq(Bsz, 30, T + n)
    harness.slice_learner_test_loss("previous", model, solver, torch.zeros(Bsz, 30, 2), seq[..., :T], seq[..., T:])
    assert len(model.seen) == 1
    _, prev, code, _, _ = model.seen[0]
    assert float(prev[1, 0, 0, 0]) == 10 * (T - 1) + 1 and float(code[1, 0, 0, 0]) == 10 * (T - 1) + 1
    assert [float(t[0, 0, 0, 0]) for t in targets] == [10.0 * (T + k) for k in range(n)]


# ---------------------------------------------------------------------------------------------- the command line
def _table(parser):
    return {a.option_strings[0]: (a.type, a.default) for a in parser._actions if a.dest != "help"}


@pytest.mark.parametrize("driver,epochs,ntrain,save_name", [("learnslice", 1, 10, "buff"), ("vorticity", 5, 10, "buff"),
                                                            ("previous", 50, 50, "slice_ep5_sim50_unified_vort")])
def test_train_slices_flag_defaults_are_the_scripts_constants(driver, epochs, ntrain, save_name):
    from transformerbasednavierstokesolver_amd import train_sequence, train_slices as tsl
    t = _table(tsl.build_parser(driver))
    assert t["--epochs"] == (int, epochs) and t["--ntrain"] == (int, ntrain) and t["--ntest"] == (int, 10)
    assert t["--lr"] == (float, 1e-3) and t["--weight_decay"] == (float, 1e-5) and t["--save_name"] == (str, save_name)
    assert t["--unified_pos"] == (int, 1) and t["--use_vorticity"] == (int, 1) and t["--use_code_for_vorticity"] == (int, 1)
    assert t["--eval"] == (int, 1)
    assert t["--encoder_path"] == (str, os.path.join("sequential_checkpoints", "encoder_ep20_head_1.pt"))
    assert t["--sequensolver_path"] == (str, os.path.join("sequential_checkpoints", "tokenizer_ep10_sim10_2.pt"))
    assert t["--fold_time"] == (int, tsl.FOLD_TIME_DEFAULT[driver]) and t["--engine"] == (str, None)
    args = tsl.parse_args(["--driver", driver])
    assert args.driver == driver and args.epochs == epochs
    with pytest.raises(SystemExit):
        tsl.parse_args([])                                              # --driver is required
    assert tsl.DRIVERS == ("learnslice", "vorticity", "previous")
    assert train_sequence.DRIVERS == ("autoencoder", "sequensolver", "sequensolver_merged")      # untouched
    kinds = {"learnslice": "LearnSlice", "vorticity": "VorticitySliceLearner", "previous": "PreviousSliceLearner"}
    assert type(tsl.build_learner(args)).__name__ == kinds[driver]


def test_train_slices_hands_the_flags_to_the_loop(monkeypatch, tmp_path):
    import scipy.io as scio
    from transformerbasednavierstokesolver_amd import cli, harness, train_slices as tsl
    u = np.random.default_rng(0).standard_normal((6, 64, 64, 20)).astype(np.float32)
    scio.savemat(str(tmp_path / "NavierStokes_V1e-5_N1200_T20.mat"), {"u": u})
    seen = {}

    def fit(model, opt, sched, solver, pos, train_set, test_set, **kw):
        seen["fit"] = (type(model).__name__, solver, tuple(pos.shape), len(train_set), len(test_set), kw)
        return []

    monkeypatch.setattr(tsl, "build_sequen_solver", lambda args, dev: seen.setdefault("solver", (args.encoder_path, args.sequensolver_path)))
    monkeypatch.setattr(cli, "device", lambda args: torch.device("cpu"))
    monkeypatch.setattr(cli, "optim", lambda model, lr, wd, epochs, steps, clip=None:
                        seen.setdefault("optim", (lr, wd, epochs, steps)) and (type("O", (), {"sync": None})(), None))
    monkeypatch.setattr(harness, "fit_slice_learner", fit)
    tsl.main(["--driver", "previous", "--eval", "0", "--ntrain", "3", "--ntest", "2", "--epochs", "4", "--data_path", str(tmp_path),
              "--encoder_path", "enc.pt", "--sequensolver_path", "seq.pt", "--save_name", "run", "--fold_time", "1"])
    assert seen["solver"] == ("enc.pt", "seq.pt") and seen["optim"] == (1e-3, 1e-5, 4, 3)
    name, solver, pos_shape, ntrain, ntest, kw = seen["fit"]
    assert (name, solver, pos_shape, ntrain, ntest) == ("PreviousSliceLearner", ("enc.pt", "seq.pt"), (1, 4096, 64), 3, 2)
    assert kw["epochs"] == 4 and kw["kind"] == "previous" and kw["fold_time"] is True and kw["batch_size"] == 1
    assert kw["save_path"] == os.path.join("./sequential_checkpoints", "run.pt")
    # learnslice: the schedule steps once per frame
    seen.clear()
    tsl.main(["--driver", "learnslice", "--eval", "0", "--ntrain", "3", "--ntest", "2", "--data_path", str(tmp_path)])
    assert seen["optim"] == (1e-3, 1e-5, 1, 30) and seen["fit"][0] == "LearnSlice" and seen["fit"][5]["use_vorticity"] == 1


def test_wrapper_words_the_grid_refusal():
    """More (sample, row chunk) units than one launch's grid holds: the C side returns PA2D_ERR_UNSUPPORTED; the wrapper holds
    the same two constants and says why before it gets there (its message: tests/test_gpu_prev_slice_entry.py)."""
    from transformerbasednavierstokesolver_amd import _lib, ops
    B, N, M, H = 262141, 1, 1, 4
    assert _lib.load().pa2d_prev_slice_entry_fwd(16, 16, 16, 16, B, N, M, H, 1, 0) == UNSUP
    assert _lib.load().pa2d_prev_slice_entry_fwd(0, 0, 0, 0, B - 1, N, M, H, 1, 0) == ARG            # one fewer: only NULL is wrong
    assert ops.PREV_SLICE_MAX_UNITS == 262140 and ops.PREV_SLICE_FWD_ROWS == 64
