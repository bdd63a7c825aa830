"""The order of the calls that every harness.*_train_step makes around its optimizer step, without a GPU.  All eight
end in the one tail harness._apply_step; what their docstrings promise is recorded here on a stub optimizer, a stub
scheduler, a `grad_sync` callable, the patched torch.nn.utils.clip_grad_norm_ and Tensor.backward, with a forward
pre-hook on the model:

  * zero_grad before backward, at the place of each driver relative to its model calls (before the call in the Darcy
    and static steps, after it everywhere else), with the set_to_none that each driver hands the optimizer;
  * grad_sync before the clip before optimizer.step() before scheduler.step();
  * the clip only when a threshold is given, over the parameters each driver clips (all of them, or the trainable ones);
  * learnslice_train_step: one optimizer step per frame; plas_train_step: one per time step and no scheduler;
    every other function: exactly one optimizer step.

train / Darcy / static / plas steps run the fp64 oracle modules of the driver tests (two frames or time steps); the four
steps whose models exist on the GPU only run two-layer stand-ins with the same call signatures and one frozen parameter."""
import pytest
import torch

import benchmark_restatement as br
import driver_restatement as dr
from transformerbasednavierstokesolver_amd import data, harness

B, N, T_IN, FRAMES, M = 2, 5, 3, 2, 4
ZERO, ZERO_FALSE = "zero_grad()", "zero_grad(set_to_none=False)"
TAIL = ["backward", "sync", "clip", "step", "sched"]


class _Optimizer:
    def __init__(self, log):
        self.log = log

    def zero_grad(self, **kw):
        self.log.append("zero_grad(%s)" % ", ".join(f"{k}={v}" for k, v in kw.items()))

    def step(self):
        self.log.append("step")


class _Scheduler:
    def __init__(self, log):
        self.log = log

    def step(self):
        self.log.append("sched")


class _Window(torch.nn.Module):
    """Stand-in for the auto-encoder (model(x, fx=fx) -> fx's shape), the sequence models (model(x, fx, y, use_gt=) ->
    [B, N, 1]) and the slice predictors (get_slice_weight(code, x, fx, use_vorticity=) / model(x, fx) -> [B, 1, N, M])."""

    def __init__(self, out):
        super().__init__()
        self.lin = torch.nn.Linear(T_IN, out)
        self.frozen = torch.nn.Linear(1, 1).requires_grad_(False)

    def forward(self, x, fx, y=None, use_gt=True):
        return self.lin(fx)

    def get_slice_weight(self, code, x, fx, use_vorticity):
        return self(x, fx)[:, None]


class _SlicePredictor(_Window):
    def forward(self, x, fx):
        return self.lin(fx)[:, None]


class _FrozenSolver:
    """What the LearnSlice loops read of the frozen sequence model: encoder.encode / get_attention_slice and get_code."""

    def __init__(self):
        self.encoder = self

    def encode(self, x, y):
        self.y = y

    def get_attention_slice(self):
        return self.y.expand(-1, -1, M)[:, None].softmax(-1)

    def get_code(self, x, fx, y):
        return fx.mean(1, keepdim=True)[:, None]


@pytest.fixture
def rec(monkeypatch):
    """(log, optimizer, scheduler, grad_sync, clipped): `clipped` collects the parameter list of every clip call."""
    log, clipped = [], []
    real = torch.Tensor.backward
    monkeypatch.setattr(torch.Tensor, "backward", lambda t, *a, **k: (log.append("backward"), real(t, *a, **k))[1])
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda ps, thr: (log.append("clip"), clipped.append(list(ps)))[0])
    monkeypatch.setattr(harness.Fn, "slice_mse", lambda sw, target: ((sw - target) ** 2).mean(-1).sum())
    return log, _Optimizer(log), _Scheduler(log), lambda: log.append("sync"), clipped


def _window_batch():
    g = torch.Generator().manual_seed(3)
    return torch.rand(B, N, 2, generator=g), torch.rand(B, N, T_IN, generator=g), torch.rand(B, N, FRAMES, generator=g)


def _ns(opt, sched, sync, thr):
    model = dr.OracleModel(dr.model_config("ns_clip"), dr.weights("ns_clip"))
    x, fx, yy = next(dr.ns_datasets("ns_clip")[0].batches(B))
    return model, lambda: harness.train_step(model, opt, sched, x, fx, yy[..., :FRAMES], max_grad_norm=thr, grad_sync=sync)


def _darcy(opt, sched, sync, thr):
    model, d = dr.OracleModel(dr.model_config("darcy"), dr.weights("darcy")), dr.darcy_data("darcy")
    x = data.grid_positions(d["s"]).expand(B, -1, -1)
    return model, lambda: harness.darcy_train_step(model, opt, sched, x, d["x_train"][:B], d["y_train"][:B], d["y_normalizer"],
                                                   d["dx"], d["s"], max_grad_norm=thr, grad_sync=sync)


def _static(opt, sched, sync, thr):
    model, d = br.oracle_model("elas"), br.load_data("elas")
    return model, lambda: harness.static_train_step(model, opt, sched, d["x_train"][:B], d["y_train"][:B], d["y_normalizer"],
                                                    max_grad_norm=thr, grad_sync=sync)


def _plas(opt, sched, sync, thr):
    model, d = br.oracle_model("plas"), br.load_data("plas")
    x, tim = d["pos"].expand(B, -1, -1), d["t"][:FRAMES].expand(B, -1)
    return model, lambda: harness.plas_train_step(model, opt, x, d["x_train"][:B], tim, d["y_train"][:B, ..., :FRAMES],
                                                  max_grad_norm=thr, grad_sync=sync)


def _autoencoder(opt, sched, sync, thr):
    model, (x, fx, _) = _Window(T_IN), _window_batch()
    return model, lambda: harness.autoencoder_train_step(model, opt, sched, x, fx, max_grad_norm=thr, grad_sync=sync)


def _sequensolver(opt, sched, sync, thr):
    model, (x, fx, yy) = _Window(1), _window_batch()
    return model, lambda: harness.sequensolver_train_step(model, opt, sched, x, fx, yy, max_grad_norm=thr, grad_sync=sync)


def _learnslice(opt, sched, sync, thr):
    model, (x, fx, yy) = _Window(M), _window_batch()
    return model, lambda: harness.learnslice_train_step(model, opt, sched, _FrozenSolver(), x, fx, yy, False,
                                                        max_grad_norm=thr, grad_sync=sync)


def _slice_predictor(opt, sched, sync, thr):
    model, (x, fx, yy) = _SlicePredictor(M), _window_batch()
    return model, lambda: harness.slice_predictor_train_step(model, opt, sched, _FrozenSolver(), x, fx, yy,
                                                             max_grad_norm=thr, grad_sync=sync)


# name: (setup, the calls up to and including zero_grad, clips the trainable parameters only, tails per call)
STEPS = {
    "train_step": (_ns, ["forward"] * FRAMES + [ZERO_FALSE], False, 1),
    "darcy_train_step": (_darcy, [ZERO_FALSE, "forward"], False, 1),
    "static_train_step": (_static, [ZERO_FALSE, "forward"], False, 1),
    "plas_train_step": (_plas, ["forward", ZERO_FALSE], False, FRAMES),
    "autoencoder_train_step": (_autoencoder, ["forward", ZERO], False, 1),
    "sequensolver_train_step": (_sequensolver, ["forward"] * FRAMES + [ZERO], True, 1),
    "learnslice_train_step": (_learnslice, ["forward", ZERO], True, FRAMES),
    "slice_predictor_train_step": (_slice_predictor, ["forward"] * FRAMES + [ZERO], True, 1),
}


@pytest.mark.parametrize("threshold", [None, 0.1])
@pytest.mark.parametrize("name", list(STEPS))
def test_train_step_call_order(name, threshold, rec):
    log, opt, sched, sync, clipped = rec
    setup, head, trainable_only, repeats = STEPS[name]
    model, call = setup(opt, sched, sync, threshold)
    model.register_forward_pre_hook(lambda *_: log.append("forward"))
    call()
    tail = [e for e in TAIL if (e != "clip" or threshold is not None) and (e != "sched" or name != "plas_train_step")]
    assert log == (head + tail) * repeats, name
    assert log.count("step") == repeats
    want = [p for p in model.parameters() if p.requires_grad or not trainable_only]
    assert len(clipped) == (0 if threshold is None else repeats)
    assert all(len(c) == len(want) and all(a is b for a, b in zip(c, want)) for c in clipped)
    if trainable_only:
        assert len(want) < len(list(model.parameters()))            # the stand-in has a frozen parameter to leave out
