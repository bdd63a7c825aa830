"""Callers of the hot path, restated for the MI355X build.

The reference's driver scripts run argparse at import and keep their work in main(); these functions reproduce
their loops, iteration by iteration and (fit_*) epoch by epoch, pinned by fixtures that the drivers' own main()
made (tests/golden/G14-G16, tools/make_golden_drivers.py):

  train_iteration / train_step  exp_ns.py:191-218   (T/step teacher-forced model calls, summed rel-L2,
                                                    one backward, AdamW(wd=1e-5) + OneCycleLR step)
  rollout                       exp_ns.py:225-241, ns_vorticity_unrolling.py:264-286
                                (prediction-feedback loop, no grad)
  GraphedRollout                the same step captured once in a hipGraph (static buffers; the
                                `torch.cat` window shift becomes an in-place roll)
  GraphedCallStep               a whole one-call iteration (exp_darcy / exp_airfoil / exp_pipe / exp_elas / one time step
                                of exp_plas) with its optimizer step in one hipGraph: fit_darcy / fit_static / fit_plas
                                with graphed=True
  unrolled_train_iteration      ns_vorticity_unrolling.py:225-244 (look-ahead windows through the SOL
  / LookAheadCurriculum         wrapper, BPTT through n chained calls) and :216-223 (curriculum)
  central_diff / darcy_loss     exp_darcy.py:59-68, 209-234 (decode, rel-L2 + 0.1 x derivative loss,
  / darcy_train_step            clip, step) — the large-N single-call iteration
  static_train_step             exp_airfoil.py:187-199, exp_pipe.py:204-221, exp_elas.py:163-176 (one model(x, None) call, rel-L2
                                of the decoded prediction and target)
  plas_train_step               exp_plas.py:242-253 (per batch T time-conditioned calls, each with its own optimizer step)
  fit_ns / fit_unrolled         exp_ns.py:184-257, ns_vorticity_unrolling.py:204-329, exp_darcy.py:205-268, exp_airfoil.py:
  / fit_darcy / fit_static      182-226, exp_pipe.py:199-249, exp_elas.py:158-204, exp_plas.py:233-292: the epoch loops (shuffled
  / fit_plas                    batches, per-epoch test pass, the drivers' metric normalisation, checkpoints).  Each is its
                                setup, a per-batch closure and a metrics function around the one loop `_fit`; a loop with a
                                graph mode picks replay or eager per batch through `_graphed_or_eager`
  evaluate_ns / _darcy          the test pass of a loop alone, normalised like the loop's metrics
  / _static / _plas
  autoencoder_train_step        auto_encoder.py:166-181 (the auto-encoder reconstructs its own input fx)
  sequensolver_train_step       SequenSolver.py:572-606 (Tout teacher-forced calls of the latent sequence model, window slid
  / sequensolver_rollout        with the true frame, summed rel-L2, one backward, step) and :613-630 (prediction feedback)
                                (fold_time=True: the Tout calls as ONE model.forward_windows call, every frame encoded once)
  fit_autoencoder               auto_encoder.py:160-210, SequenSolver.py:572-640, SequenSolverMerged.py:454-523: the epoch
  / fit_sequensolver            loops of the latent-sequence family on `_fit`, with the scripts' own metric divisors
  learnslice_train_step         LearnSlice.py:477-526 (slice weights from the frozen model's code: one optimizer step per frame)
  slice_predictor_train_step    LearnSlice.py:929-962 and :861-913 (the conv slice predictors: Tout summed terms and one step;
  / slice_predictor_rollout     the prediction-feedback evaluation)
  fit_velocity                  ns_velocity.py:192-273, ns_velocity_unrolling.py:202-313, ns_unrolling2_with_t.py:200-313: the
  / fit_velocity_unrolled       epoch loops on PhiFlow velocity data (one prediction = a (vel_x, vel_y) pair, step = 2), with
  / fit_unrolled_t              graphed=True one whole-iteration hipGraph per look-ahead value (end of this file)
  scored_rollout                their prediction-feedback test pass with one fused launch after each model call (window shift,
  / GraphedScoredRollout        kept prediction, the step's score) and one after the last; the whole of it in ONE hipGraph

Every *_train_step, the SOL loops and GraphedTrainStep end in `_apply_step`: [grad_sync], [clip], optimizer.step(),
[scheduler.step()].  zero_grad and backward stay in each function, because their place differs and is kept as the drivers have
it: the Darcy, static and plasticity steps zero with set_to_none=False outside any `ops.weights_frozen()` scope (before the
model call; plas after it), the others zero after the forward and inside the scope (the NS time-stepping family through the one
`_eager_iteration`: train_step with its `set_to_none` argument, fit_unrolled with the optimizer's default, the velocity loops
with set_to_none=False; the rest with the optimizer's default); the sequence-model and slice steps clip the trainable
parameters only, the others all of them.  The NS time-stepping drivers (exp_ns, ns_vorticity_unrolling and the three velocity
scripts) are one family: one teacher-forced loop, one prediction-feedback test pass, one windowed SOL loop and one SOL epoch
loop, switched by `fused` (see `_step_loss`); the four Graphed* classes capture through `_warm_capture` and guard their
parameter pointers with `_ParamPointers`.
"""
from __future__ import annotations

import os

import torch

from . import functional as Fn
from . import ops
from .folding import FOLD_MAX_BYTES, _fold_group, _slice_fold_group, groups, joined, model_engine, windows  # noqa: F401
from .model.Transolver_Structured_Mesh_2D import Model
from .utils.testloss import TestLoss


def build_model(cfg, state_dict=None, device="cuda", engine=None):
    """`engine`: GEMM engine of this model ("f32" | "split" | "bf16"; None = PA2D_GEMM / the split default)."""
    m = _build_model(cfg, state_dict, device)
    return m.set_engine(engine) if engine is not None else m


def _build_model(cfg, state_dict, device):
    m = Model(space_dim=cfg["space_dim"], n_layers=cfg["n_layers"], n_hidden=cfg["n_hidden"],
              dropout=cfg.get("dropout", 0.0), n_head=cfg["n_head"], Time_Input=cfg["Time_Input"],
              act=cfg.get("act", "gelu"), mlp_ratio=cfg["mlp_ratio"], fun_dim=cfg["fun_dim"],
              out_dim=cfg["out_dim"], slice_num=cfg["slice_num"], ref=cfg["ref"],
              unified_pos=cfg["unified_pos"], H=cfg["H"], W=cfg["W"])
    if state_dict is not None:
        m.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()}, strict=True)
    return m.to(device)


def train_iteration(model, x, fx, yy, step=1, loss_fn=None, fold_time=False):
    """Forward part of one exp_ns mini-batch.  Returns (loss [graph attached], full_loss, pred).

    `fold_time`: the loop below is teacher-forced — the input window of call t is built from GROUND
    TRUTH frames only (exp_ns.py:205), so the T/step model calls do not depend on each other.  Folded,
    they run as ONE call on a batch of (T/step)*B windows: the same per-window outputs, the same summed
    loss and (up to fp32 summation order inside the weight-gradient reductions) the same gradients, with
    1/(T/step) of the launches, no per-call gradient accumulation and full tiles at the reference's small
    batch sizes.  Not applicable to the prediction-feedback rollout.
    With training-mode dropout the folded call draws ONE larger mask per layer for all its windows where the loop draws one
    per call: both are valid dropout, from different stretches of the generator, so the two routes are not bit-equal then."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    bsz = x.shape[0]
    if fold_time:
        return _train_iteration_folded(model, x, fx, yy, step, loss_fn)
    loss, preds = _teacher_forced(model, x, fx, yy, step, loss_fn, False)
    pred = torch.cat(preds, -1)
    with torch.no_grad():
        full = loss_fn(pred.reshape(bsz, -1), yy.reshape(bsz, -1))
    return loss, full, pred


def _batch_sum_rel(loss_fn):
    """True where `loss_fn` is the scripts' loss: a `TestLoss` (or FusedTestLoss) with p = 2 that sums over the batch."""
    return isinstance(loss_fn, TestLoss) and loss_fn.p == 2 and loss_fn.reduction and not loss_fn.size_average


def _step_loss(loss_fn, im, yy, col, fused, calls=None):
    """The loss of one model call against the columns [col, col + k) of yy, k = im.shape[-1]; the value (detached, a device
    tensor) is appended to `calls` where that is a list.  `fused` is THE switch for "on the window kernels" of the NS
    time-stepping family: False (exp_ns, ns_vorticity_unrolling: fit_ns, evaluate_ns, train_step, GraphedTrainStep,
    fit_unrolled) is always `loss_fn` on the reshaped copies, as the scripts have it; True (the velocity loops) is
    functional.rel_l2_window, the target read in place, where k > 1 with fp32 GPU tensors and the p = 2 batch-sum `rel`, and
    the same `loss_fn` call otherwise.  At k = 1 the two are the same code; at k > 1 they differ in the last bits.
    The target columns are counted by the prediction's width k, where the scripts count by `step`: the same wherever the
    model's out_dim equals step, as in every script and fixture (with another out_dim the scripts' own reshape fails)."""
    bsz, k = im.shape[0], im.shape[-1]
    if (fused and 1 < k <= ops.WINDOW_MAX_K and _batch_sum_rel(loss_fn) and not yy.requires_grad
            and all(t.is_cuda and t.dtype == torch.float32 for t in (im, yy))):
        v = Fn.rel_l2_window(im, yy, col, k).sum()
    else:
        v = loss_fn(im.reshape(bsz, -1), yy[..., col:col + k].reshape(bsz, -1))
    if calls is not None:
        calls.append(v.detach())
    return v


def _full_loss(loss_fn, preds, yy, calls=None):
    bsz = yy.shape[0]
    with torch.no_grad():
        v = loss_fn(torch.cat(preds, -1).reshape(bsz, -1), yy.reshape(bsz, -1))
    if calls is not None:
        calls.append(v)
    return v


def _teacher_forced(model, x, fx, yy, step, loss_fn, fused, calls=None):
    """The teacher-forced loop of exp_ns.py:199-211 and ns_velocity.py:204-225: T / step model calls, the input window of
    each built from GROUND TRUTH columns only.  Returns (summed per-call loss, the per-call predictions), graphs attached."""
    loss, preds = 0, []
    for t in range(0, yy.shape[-1], step):
        im = model(x, fx=fx)
        loss = loss + _step_loss(loss_fn, im, yy, t, fused, calls)
        preds.append(im)
        fx = torch.cat((fx[..., step:], yy[..., t:t + step]), dim=-1)
    return loss, preds


def _train_iteration_folded(model, x, fx, yy, step, loss_fn):
    T, bsz, F = yy.shape[-1], x.shape[0], fx.shape[-1]
    nt = len(range(0, T, step))
    seq = torch.cat((fx, yy), dim=-1)                                     # frames the windows slide over
    loss, outs = 0, []
    for t0, g in groups(nt, _fold_group(model, bsz, x.shape[1], nt)):     # normally ONE group
        wins = torch.stack([seq[..., t * step:t * step + F] for t in range(t0, t0 + g)], 0)       # [g,B,N,F]
        im = model(x.repeat(g, 1, 1), fx=wins.reshape(g * bsz, *fx.shape[1:]))                    # [g*B,N,step]
        im = im.reshape(g, bsz, *im.shape[1:])
        for k in range(g):                    # per-call loss terms, so any reduction mode of loss_fn carries over
            t = t0 + k
            y = yy[..., t * step:(t + 1) * step]
            loss = loss + loss_fn(im[k].reshape(bsz, -1), y.reshape(bsz, -1))
        outs.append(im)
    im = joined(outs)
    pred = im.permute(1, 2, 0, 3).reshape(bsz, im.shape[2], -1)
    with torch.no_grad():
        full = loss_fn(pred.reshape(bsz, -1), yy.reshape(bsz, -1))
    return loss, full, pred


def _apply_step(optimizer, scheduler, params, max_grad_norm, grad_sync):
    """The tail of every eager iteration, after its backward: [grad_sync()], [clip_grad_norm_ of `params`, any iterable,
    read only when a threshold is given], optimizer.step(), [scheduler.step()].  zero_grad and backward stay with the
    caller: where they stand relative to the forward and to an `ops.weights_frozen()` scope differs per driver."""
    if grad_sync is not None:
        grad_sync()
    if max_grad_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()


def train_step(model, optimizer, scheduler, x, fx, yy, step=1, max_grad_norm=None, grad_sync=None,
               set_to_none=False, loss_fn=None, fold_time=False):
    """One full exp_ns.py:191-218 iteration.  `grad_sync` (DDP): callable run between backward and
    the optimizer step (all-reduce SUM of the flat gradient bucket).  With `optim.FusedAdamW` pass
    `grad_sync=optimizer.sync` (same bucket) and put the clip threshold in the optimizer instead of
    `max_grad_norm`."""
    return _eager_iteration(model, optimizer, scheduler, lambda: train_iteration(model, x, fx, yy, step, loss_fn, fold_time)[:2],
                            max_grad_norm, grad_sync, dict(set_to_none=set_to_none))


def _eager_iteration(module, optimizer, scheduler, forward, max_grad_norm, grad_sync, zero_grad_kw):
    """The eager iteration of train_step, fit_unrolled and the velocity loops: forward() -> loss parts (the first is
    differentiated), optimizer.zero_grad(**zero_grad_kw) and the backward inside ONE `ops.weights_frozen()` scope (no
    parameter moves between the first model call and the end of backward); then `_apply_step` on the module's parameters.
    Returns the detached parts."""
    with ops.weights_frozen():
        parts = forward()
        optimizer.zero_grad(**zero_grad_kw)
        parts[0].backward()
    _apply_step(optimizer, scheduler, module.parameters(), max_grad_norm, grad_sync)
    return tuple(p.detach() for p in parts)


class _fused_tail_set:
    """`with _fused_tail_set(model, flag):` the model's fused-tail switch (TransolverBase.set_fused_tail) is `flag` inside
    and what it was afterwards; flag None leaves the model as it is."""

    def __init__(self, model, flag):
        self.model, self.flag = model, flag

    def __enter__(self):
        if self.flag is not None:
            self.before = bool(getattr(self.model, "fused_tail", False))
            self.model.set_fused_tail(self.flag)

    def __exit__(self, *exc):
        if self.flag is not None:
            self.model.set_fused_tail(self.before)
        return False


@torch.no_grad()
def rollout(model, x, fx, nsteps, step=1, fused_tail=None):
    """fused_tail: None = the model as it is; True / False = the model's fused block tail (set_fused_tail) on / off for
    this call, restored afterwards."""
    frames = []
    with _fused_tail_set(model, fused_tail), ops.weights_frozen():
        for _ in range(nsteps):
            im = model(x, fx=fx)
            frames.append(im)
            fx = torch.cat((fx[..., step:], im), dim=-1)
    return torch.cat(frames, -1)


def _warm_capture(body, warmup, between=None, before_run=None):
    """The capture of every Graphed* class: `warmup` runs of body() on a side stream that waits for the current one (they
    set kernel attributes and warm the allocator), the current stream waits for the side stream, `between()` where given
    (state that the warm-up moved is put back), then ONE more run inside torch.cuda.graph.  `before_run()`, where given,
    runs ahead of every one of those runs and outside the capture (the optimizer's host half).  Returns (graph, what the
    captured run returned)."""
    current, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(current)
    with torch.cuda.stream(side):
        for _ in range(warmup):
            if before_run is not None:
                before_run()
            body()
    current.wait_stream(side)
    if between is not None:
        between()
    if before_run is not None:
        before_run()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    return graph, out


class _ParamPointers:
    """Captured launches hold raw parameter pointers: anything that re-seats parameter storage afterwards (an optimizer
    that flattens the parameters, .to(), load with assign=True) invalidates the graph.  Records the pointers of `model`'s
    parameters; check() raises RuntimeError "parameter storage moved since this `what` was captured`advice`"."""

    def __init__(self, model, what, advice):
        self.model, self.what, self.advice = model, what, advice
        self.ptrs = [p.data_ptr() for p in model.parameters()]

    def check(self):
        if [p.data_ptr() for p in self.model.parameters()] != self.ptrs:
            raise RuntimeError(f"parameter storage moved since this {self.what} was captured{self.advice}")


class _RolloutGraph:
    """What GraphedRollout and GraphedScoredRollout share: warm-up and capture under no_grad, with the model's fused block
    tail set as asked, inside one `ops.weights_frozen()` scope that is kept: the conv weight packs are made during the
    warm-up and only REFERENCED by the captured launches, and `_ready()` refreshes them in place before a replay, so later
    weight updates (training between rollouts) are seen."""

    def _capture(self, model, body, warmup, fused_tail, between=None):
        self.model = model
        with _fused_tail_set(model, fused_tail), ops.weights_frozen() as self.packs, torch.no_grad():
            self.graph, out = _warm_capture(body, warmup, between)
        self._ptrs = _ParamPointers(model, "rollout graph", " (e.g. FusedAdamW / FlatGradSync built afterwards, or .to()); "
                                    "build the optimizer first or re-capture")
        return out

    def _ready(self, buffers, batch):
        """Before a replay: the pointer check, the batch copied into the static buffers (None keeps one), the packs."""
        self._ptrs.check()
        for buf, t in zip(buffers, batch):
            if t is not None:
                buf.copy_(t)
        self.packs.refresh()


class GraphedRollout(_RolloutGraph):
    """One autoregressive step (model call + window shift) captured in a hipGraph and replayed.

    Static buffers: `x`, the input window `fx` [B,N,fun_dim] and the output `im`.  The window shift
    `fx = cat(fx[..., step:], im)` is done in place inside the graph, so shapes and pointers never
    change.  Replays are bit-identical to the eager loop (same kernels, same order).
    fused_tail: None = the model as it is; True / False = the model's fused block tail on / off for the capture (the
    captured step keeps that route; the model's own flag is restored when the constructor returns)."""

    def __init__(self, model, x, fx, step=1, warmup=2, fused_tail=None):
        self.step, self.x, self.fx = step, x.clone(), fx.clone()
        self._capture(model, self._step_eager, warmup, fused_tail, between=lambda: self.fx.copy_(fx))
        self.fx.copy_(fx)

    def _step_eager(self):
        self.im = self.model(self.x, fx=self.fx)
        k = self.im.shape[-1]
        shifted = self.fx[..., self.step:].clone()
        self.fx[..., :-k].copy_(shifted[..., :self.fx.shape[-1] - k])
        self.fx[..., -k:].copy_(self.im)

    @torch.no_grad()
    def run(self, fx0, nsteps):
        self._ready((self.fx,), (fx0,))
        frames = []
        for _ in range(nsteps):
            self.graph.replay()
            frames.append(self.im.clone())
        return torch.cat(frames, -1)


def training_dropout(model):
    """Largest dropout probability that applies in a call of `model` as it stands: over its nn.Dropout members in training
    mode (0.0 without one).  Host-side, no GPU."""
    return max((float(m.p) for m in model.modules() if isinstance(m, torch.nn.Dropout) and m.training), default=0.0)


def _refuse_graphed_dropout(model, who):
    """The dropout kernels take the draw's (seed, offset) as launch constants, which a capture bakes in: every replay would
    reuse one mask.  First check of every graph-capturing step, before anything touches the GPU."""
    if training_dropout(model) > 0:
        raise NotImplementedError(f"{who}: a model with training-mode dropout p > 0 cannot be captured (every replay would "
                                  "draw the same mask); run the eager step, or set dropout=0")


class GraphedTrainStep:
    """exp_ns iteration with the launch-bound part captured in ONE hipGraph.

    At the reference's batch sizes (2-8) an iteration is ~14 000 kernel launches and the host cannot
    issue them as fast as the GPU retires them.  Captured once, replayed per iteration: zeroing the flat
    gradient bucket, the T/step teacher-forced model calls, the summed rel-L2 loss and the whole backward
    pass (static input buffers; every intermediate lives in the graph's private pool).  The gradient
    all-reduce, `optimizer.step()` and `scheduler.step()` stay eager because the OneCycle lr / beta1 are
    host scalars that change every iteration (2-3 launches).  Needs `optim.FusedAdamW` (gradients must be
    views of one persistent flat buffer).  Replays run the same kernels in the same order as the eager
    path, so results are bit-identical to `train_step`."""

    def __init__(self, model, optimizer, scheduler, x, fx, yy, step=1, loss_fn=None, warmup=3, fold_time=False):
        from .optim import FusedAdamW
        _refuse_graphed_dropout(model, "GraphedTrainStep")
        self.fold_time = fold_time
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError("GraphedTrainStep needs optim.FusedAdamW (persistent flat gradient bucket)")
        self.model, self.opt, self.sched, self.step_size, self.loss_fn = model, optimizer, scheduler, step, loss_fn
        self.x, self.fx, self.yy = x.clone(), fx.clone(), yy.clone()
        snap = [p.detach().clone() for p in model.parameters()]

        def restore():                                     # warm-up must not move the weights
            for p, q in zip(model.parameters(), snap):
                p.data.copy_(q)
        self.graph, (self.loss, self.full) = _warm_capture(self._fwd_bwd, warmup, between=restore)

    def _fwd_bwd(self):
        with ops.weights_frozen():      # inside the capture: each layer's weights are packed once per replay
            self.opt.zero_grad()
            loss, full, _ = train_iteration(self.model, self.x, self.fx, self.yy, self.step_size, self.loss_fn,
                                            self.fold_time)
            loss.backward()
        return loss.detach(), full

    def __call__(self, x, fx, yy):
        self.x.copy_(x)
        self.fx.copy_(fx)
        self.yy.copy_(yy)
        self.graph.replay()
        _apply_step(self.opt, self.sched, (), None, self.opt.sync)      # all-reduce(SUM) of the flat bucket when world_size > 1
        return self.loss, self.full


def _graphed_refusals(who, optimizer, max_grad_norm, one_rank=True):
    """What every graphed loop asks for before it captures anything (also on a machine without a GPU).  `one_rank=False`:
    fit_ns, whose GraphedTrainStep leaves the all-reduce and the optimizer step outside the capture and so serves several ranks."""
    from .optim import FusedAdamW
    if max_grad_norm is not None:
        raise ValueError(f"{who}(graphed=True) clips inside optim.FusedAdamW: build it with max_grad_norm=... and pass "
                         "max_grad_norm=None here (a replayed batch would otherwise go unclipped)")
    if not isinstance(optimizer, FusedAdamW):
        raise TypeError(f"{who}(graphed=True) needs optim.FusedAdamW (persistent flat gradient bucket, staged step)")
    import torch.distributed as dist
    if one_rank and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"{who}(graphed=True): the gradient all-reduce is not captured; run one rank, or eager")


class GraphedCallStep:
    """A WHOLE one-call iteration in one hipGraph: zero-grad, one model call, the loss, the backward and the optimizer
    step (`FusedAdamW.step_staged`: the gradient norm and the AdamW launches, which read the step's coefficients from the
    device row `optimizer.coef`).  Unlike GraphedTrainStep there is NO `ops.weights_frozen()` scope around the model call
    and the backward, as there is none in darcy_train_step / static_train_step / plas_train_step: with one call per
    iteration every weight pack is used once, so making the packs ahead only adds launches (measured on the MI355X, Darcy
    85 x 85 at batch 4: 6.43 ms with the scope against 6.25 ms without), and without it the capture holds
    exactly the launches of the eager step.

    `static`: the iteration's input buffers, owned by this object (pointers and strides never change).  `body(model,
    *static)` makes the model call and returns the loss parts, the first of which is differentiated; the parts come back
    from every call as (static) device tensors.  One call = copy the batch into the static buffers (None keeps a buffer
    as it is), `optimizer.stage_step()` (host: counts the step and queues the row of the CURRENT lr / beta1 behind the
    previous replay), ONE replay, `scheduler.step()` (host arithmetic) where a scheduler is given.  No host
    synchronisation.  The replay runs the kernels of the eager iteration in the same order on the same values: the
    results are equal bit for bit, PROVIDED the static buffers show the loss kernels the strides and the 16-byte phase
    of the eager batch (they choose vector or scalar summation from those): buffers are made by `clone()` of a batch.

    The warm-up (side stream) takes real optimizer steps; parameters, both moments and `steps` are put back after it.
    The parameters that received a gradient differ per driver (`placeholder` does without `fx`), so the optimizer's
    active ranges are recorded at capture: every call compares them and raises RuntimeError if they have changed, and
    likewise if parameter storage moved (GraphedRollout's check)."""

    def __init__(self, model, optimizer, scheduler, static, body, warmup=2):
        _refuse_graphed_dropout(model, "GraphedCallStep")
        _graphed_refusals("GraphedCallStep", optimizer, None)
        self.model, self.opt, self.sched, self.static, self.body = model, optimizer, scheduler, list(static), body
        opt = optimizer
        snap = [t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq)]
        steps = opt.steps

        def between():                        # the warm-up has marked the touched parameters
            self._restore(snap, steps)
            self.ranges = opt.sync.active_ranges()
        # stage_step before every run: also a valid row for the capture's own (never executed) launches to point at
        self.graph, self.out = _warm_capture(self._iteration, warmup, between=between, before_run=opt.stage_step)
        self._restore(snap, steps)
        opt.sync.release_untouched()          # what step() leaves behind; a replay changes no Python state
        self._ptrs = _ParamPointers(model, "iteration", "; re-capture")

    def _restore(self, snap, steps):
        opt = self.opt
        with torch.no_grad():
            for t, q in zip((opt.flat_p, opt.exp_avg, opt.exp_avg_sq), snap):
                t.copy_(q)
        opt.steps = steps

    def _iteration(self):
        self.opt.zero_grad()
        parts = self.body(self.model, *self.static)
        parts[0].backward()
        self.opt.step_staged()
        return tuple(p.detach() for p in parts)

    def __call__(self, *batch):
        if self.opt.sync.active_ranges() != self.ranges:
            raise RuntimeError("the set of parameters with a gradient changed since this iteration was captured (its "
                               "AdamW launches cover the ranges of then); re-capture")
        self._ptrs.check()
        with torch.no_grad():
            for buf, t in zip(self.static, batch):
                if t is not None:
                    buf.copy_(t)
        self.opt.stage_step()
        self.graph.replay()
        if self.sched is not None:
            self.sched.step()
        return self.out


def _capturable_model(model, who):
    if getattr(model, "unified_pos", False) and not hasattr(model, "pos"):
        raise NotImplementedError(f"{who}(graphed=True): the irregular-mesh model with unified_pos builds its lattice from "
                                  "host memory in every call, which a capture cannot hold")


def _darcy_body(y_normalizer, dx, s):
    def body(model, x, fx, y):
        out = model(x, fx=fx.unsqueeze(-1)).squeeze(-1)
        if not _darcy_fusable(out, y, y_normalizer, s):
            raise ValueError("fit_darcy(graphed=True) needs the fused Darcy loss (fp32 CUDA tensors, a scalar fp32 "
                             "normaliser, s <= 2048); this batch would take the torch path")
        return darcy_loss(out, y, y_normalizer, dx, s, fused=True)
    return body


def _static_body(loss_fn, y_normalizer):
    def body(model, x, y):
        return (_rel_decoded(loss_fn, model(x, None).squeeze(-1), y, y_normalizer),)
    return body


def _plas_body(loss_fn):
    """static = (x, fx, tim [B, 1], yy [B, N, 4, T]): the target is COLUMN 0 of yy, a stride-T view like the eager
    yy[..., t:t+1] (a contiguous copy would take the loss kernels' vector path and other last bits)."""
    def body(model, x, fx, tim, yy):
        bsz = x.shape[0]
        im = model(x, fx, T=tim)
        return (_rel_decoded(loss_fn, im.reshape(bsz, -1), yy[..., 0:1], None),)
    return body


# ------------------------------------------------------------------------------ unrolled look-ahead training
def _windowed_iteration(sol_model, x, fx, yy, look_ahead, step, starts, loss_fn, fused, calls=None):
    """The windowed loop of the three SOL scripts: at every window start t of `starts` (the script's own range), `look_ahead`
    chained calls through the SOL wrapper, scored against yy[..., t + offset - step:t + offset], offset = step * look_ahead;
    the window then advances by `starts.step` GROUND-TRUTH columns.  `starts` None: the single window at 0, which never
    advances and whose loss is returned as it is.  Returns the summed loss (graph attached)."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    sol_model.n = look_ahead
    offset = step * look_ahead
    if starts is None:
        return _step_loss(loss_fn, sol_model(x, fx), yy, offset - step, fused, calls)
    loss = 0
    for t in starts:
        loss = loss + _step_loss(loss_fn, sol_model(x, fx), yy, t + offset - step, fused, calls)
        fx = torch.cat((fx[..., starts.step:], yy[..., t:t + starts.step]), dim=-1)
    return loss


def unrolled_train_iteration(sol_model, x, fx, yy, look_ahead, step=1, loss_fn=None):
    """One mini-batch of ns_vorticity_unrolling.py:225-244.  `sol_model.n` chained calls per window;
    the window then advances by `look_ahead` GROUND-TRUTH frames.  Returns the loss (graph attached)."""
    return _windowed_iteration(sol_model, x, fx, yy, look_ahead, step, range(0, yy.shape[-1] - look_ahead + 1, look_ahead),
                               loss_fn, False)


def unrolled_window_iteration(sol_model, x, fx, yy, look_ahead, step=2, loss_fn=None, calls=None):
    """One mini-batch of ns_velocity_unrolling.py:220-227: ONE window, `look_ahead` chained calls through the SOL wrapper,
    scored against yy[..., offset - step:offset], offset = step * look_ahead.  Returns the loss (graph attached)."""
    return _windowed_iteration(sol_model, x, fx, yy, look_ahead, step, None, loss_fn, True, calls)


def unrolled_t_iteration(sol_model, x, fx, yy, look_ahead, step=2, loss_fn=None, calls=None):
    """One mini-batch of ns_unrolling2_with_t.py:219-229: every window t in range(0, T - offset + step, step) is scored
    against yy[..., t + offset - step:t + offset] after `look_ahead` chained calls, and the window then advances by `step`
    GROUND-TRUTH columns.  Returns the summed loss (graph attached)."""
    return _windowed_iteration(sol_model, x, fx, yy, look_ahead, step, range(0, yy.shape[-1] - step * look_ahead + step, step),
                               loss_fn, True, calls)


class LookAheadCurriculum:
    """look_ahead doubles (capped) whenever `ep % thresh == 0 and ep >= thresh`, after which the
    threshold halves (ns_vorticity_unrolling.py:205-223)."""

    def __init__(self, epochs, look_ahead=1, max_look_ahead=10):
        self.look_ahead, self.max_look_ahead, self.thresh = look_ahead, max_look_ahead, epochs / 2

    def update(self, ep):
        if ep % self.thresh == 0 and ep >= self.thresh and self.look_ahead <= self.max_look_ahead:
            self.look_ahead = min(self.look_ahead * 2, self.max_look_ahead)
            self.thresh /= 2
        return self.look_ahead


# ------------------------------------------------------------------------------ Darcy iteration
def central_diff(x, h, resolution):
    """x: [B, res*res, C]; zero-padded central differences along image x / y (exp_darcy.py:59-68)."""
    B, N, C = x.shape
    img = torch.nn.functional.pad(x.reshape(B, resolution, resolution, C), (0, 0, 1, 1, 1, 1))
    gx = (img[:, 1:-1, 2:, :] - img[:, 1:-1, :-2, :]) / (2 * h)
    gy = (img[:, 2:, 1:-1, :] - img[:, :-2, 1:-1, :]) / (2 * h)
    return gx, gy


def darcy_loss(out, y, y_normalizer, dx, s, loss_fn=None, fused=False):
    """out, y: [B, N] normalised prediction / target.  Returns (loss, l2loss, deriv_loss) with
    loss = l2 + 0.1 * (rel-L2 of d/dx + rel-L2 of d/dy), prediction border zeroed first.

    `fused=True`: fp32 CUDA tensors with a scalar fp32 normaliser go through the libpa2d Darcy-loss kernels
    (functional.DarcyLossFn: one stencil kernel each way instead of ~25 + ~40 elementwise launches; the normaliser's
    mean / std are read on the device; `loss_fn` is not consulted).  Anything else takes the torch path below with
    `loss_fn`: the float64 target a real `.mat` gives (it promotes the loss to float64, as in the reference), an image
    wider than 2048 pixels, or a target / normaliser that requires a gradient (the kernels give one to `out` only)."""
    if fused and _darcy_fusable(out, y, y_normalizer, s):
        return Fn.darcy_loss(out, y, y_normalizer.mean, y_normalizer.std, dx, s)
    loss_fn = loss_fn or TestLoss(size_average=False)
    out = y_normalizer.decode(out)
    y = y_normalizer.decode(y)
    l2 = loss_fn(out, y)
    B = out.shape[0]
    img = out.reshape(B, s, s)
    inner = torch.zeros_like(img)
    inner[:, 1:-1, 1:-1] = img[:, 1:-1, 1:-1]
    gtx, gty = central_diff(y.unsqueeze(-1), dx, s)
    px, py = central_diff(inner.reshape(B, s * s, 1), dx, s)
    deriv = loss_fn(px, gtx) + loss_fn(py, gty)
    return 0.1 * deriv + l2, l2, deriv


DARCY_FUSED_MAX_S, DARCY_FUSED_MAX_B = 2048, 65535      # what pa2d_darcy_loss_* serve (one image row per LDS tile; grid.y)


def _darcy_fusable(out, y, y_normalizer, s):
    """fp32 CUDA [B, s*s] tensors with a one-element fp32 normaliser, within the kernels' sizes, and a target that asks
    for no gradient (the kernels give none to y)."""
    mean, std = y_normalizer.mean, y_normalizer.std
    ts = (out, y, mean, std)
    return (all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ts)
            and out.dim() == 2 and out.shape == y.shape and mean.numel() == 1 and std.numel() == 1
            and s <= DARCY_FUSED_MAX_S and out.shape[0] <= DARCY_FUSED_MAX_B
            and not (y.requires_grad or mean.requires_grad or std.requires_grad))


def darcy_train_step(model, optimizer, scheduler, x, fx, y, y_normalizer, dx, s, max_grad_norm=None,
                     grad_sync=None, fused=False, loss_fn=None):
    """exp_darcy.py:209-234: ONE model call per iteration (fun_dim = 1).  `fused`, `loss_fn`: see darcy_loss."""
    optimizer.zero_grad(set_to_none=False)
    out = model(x, fx=fx.unsqueeze(-1)).squeeze(-1)
    loss, l2, deriv = darcy_loss(out, y, y_normalizer, dx, s, loss_fn=loss_fn, fused=fused)
    loss.backward()
    _apply_step(optimizer, scheduler, model.parameters(), max_grad_norm, grad_sync)
    return loss.detach(), l2.detach(), deriv.detach()


def autoencoder_train_step(model, optimizer, scheduler, x, fx, max_grad_norm=None, grad_sync=None):
    """One auto_encoder.py:166-181 iteration of the structured 2-D auto-encoder (model/Transolver_Structured_Mesh2D_Encoder):
    TestLoss(size_average=False) of model(x, fx) against fx itself, zero_grad, backward, [grad_sync], [clip], step,
    [scheduler].  With `optim.FusedAdamW` pass `grad_sync=optimizer.sync` and put the clip threshold in the optimizer.
    Returns the detached loss."""
    bsz = x.shape[0]
    with ops.weights_frozen():
        im = model(x, fx=fx)
        loss = TestLoss(size_average=False)(im.reshape(bsz, -1), fx.reshape(bsz, -1))
        optimizer.zero_grad()
        loss.backward()
    _apply_step(optimizer, scheduler, model.parameters(), max_grad_norm, grad_sync)
    return loss.detach()


def sequensolver_train_step(model, optimizer, scheduler, x, fx, yy, use_gt=True, max_grad_norm=None, grad_sync=None,
                            fold_time=False):
    """One SequenSolver.py:581-606 iteration of the latent sequence model (SequenSolver.SequenSolver): Tout = yy.shape[-1]
    teacher-forced calls model(x, fx, y, use_gt) on the window fx [B, N, T], which slides on with the TRUE frame y; the
    TestLoss(size_average=False) terms are summed, then zero_grad, one backward, [grad_sync], [clip], step, [scheduler].
    The reference hard-codes use_gt=True in this loop and switches to freeze_attention() from epoch 6 on; parameters
    without requires_grad (the frozen encoder, whatever freeze_attention() froze) are in neither `optim.FusedAdamW` nor its
    gradient bucket.  With FusedAdamW pass `grad_sync=optimizer.sync` and put the clip threshold in the optimizer.
    The merged model (SequenSolverMerged.SequenSolver) has the same call signature and the same loop in its reference
    file, which runs it with use_gt=False (x is then the 64-wide unified encoding [B, N, 64]).
    `fold_time`: the windows hold ground truth only, so the Tout calls do not depend on each other; True makes ONE
    `model.forward_windows(x, cat(fx, yy), use_gt)` call (every frame encoded once, the blocks and the slice predictor on
    Tout*B folded samples, per-call z-score statistics), the same per-call loss terms summed in call order and the same
    full loss.  Teacher forcing only: `sequensolver_rollout` feeds predictions back and cannot fold.
    Returns (summed step loss [detached], full loss of the Tout predictions against yy)."""
    loss_fn = TestLoss(size_average=False)
    bsz = x.shape[0]
    with ops.weights_frozen():
        loss, preds = 0, []
        if fold_time:
            pred = model.forward_windows(x, torch.cat((fx, yy), dim=-1), use_gt=use_gt)      # [B, N, Tout]
            for t in range(yy.shape[-1]):
                loss = loss + loss_fn(pred[..., t].reshape(bsz, -1), yy[..., t].reshape(bsz, -1))
        else:
            for t in range(yy.shape[-1]):
                y = yy[..., t:t + 1]
                im = model(x, fx, y, use_gt=use_gt)
                loss = loss + loss_fn(im.reshape(bsz, -1), y.reshape(bsz, -1))
                preds.append(im)
                fx = torch.cat((fx[..., 1:], y), dim=-1)             # the ground truth enters the window
            pred = torch.cat(preds, -1)
        with torch.no_grad():
            full = loss_fn(pred.reshape(bsz, -1), yy.reshape(bsz, -1))
        optimizer.zero_grad()
        loss.backward()
    _apply_step(optimizer, scheduler, _trainable(model), max_grad_norm, grad_sync)
    return loss.detach(), full


def _trainable(model):
    """The parameters that an optimizer of `model` steps and a clip reads: the ones with requires_grad."""
    return (p for p in model.parameters() if p.requires_grad)


def _target_slices(sequen_solver, x, y):
    """The frozen encoder's slice weights [B, 1, N, M] of the true frame y [B, N, 1] (left as its cached ones)."""
    with torch.no_grad():
        sequen_solver.encoder.encode(x, y)
        return sequen_solver.encoder.get_attention_slice()


def _fold_table(sequen_solver, x, fx, yy):
    """The frozen sequence model's part of a teacher-forced slice-trainer iteration, computed once
    (`SequenSolver.code_windows` on the T + Tout true frames): (seq [B, N, T + Tout], codes [Tout, B, 1, M, C],
    slices [(T + Tout) * B, 1, N, M] frame-major).  Call k: code codes[k], target frame T + k, previous slice frame
    T + k - 1, window seq[..., k:k+T]."""
    if fx.shape[-1] != sequen_solver.T:
        raise ValueError(f"the window holds {fx.shape[-1]} frames; the sequence model reads T = {sequen_solver.T}")
    seq = torch.cat((fx, yy), dim=-1)
    codes, slices = sequen_solver.code_windows(x, seq)
    return seq, codes, slices


def learnslice_train_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, use_vorticity, max_grad_norm=None,
                          grad_sync=None, fold_time=False):
    """The LearnSlice.py:477-526 loop over one batch: for each of the Tout = yy.shape[-1] output frames y, the target is
    the frozen encoder's slice weights of y, the code comes from `sequen_solver.get_code` on the window fx [B, N, T]
    (no gradient: the sequence model is frozen), the loss is functional.slice_mse of
    model.get_slice_weight(code, x, fx, use_vorticity) against the target (the reference's sum over the points of
    F.mse_loss), then zero_grad, backward, [grad_sync], [clip], step, [scheduler]: ONE optimizer step PER FRAME, and the
    window slides on with the true frame.  The reference makes N calls of the MLP per step; here a step is one forward and
    one backward launch.  Works with torch.optim.AdamW and with `optim.FusedAdamW` (pass `grad_sync=optimizer.sync`).
    `fold_time=True`: targets and codes of all Tout frames come from ONE `sequen_solver.code_windows` call (every frame
    encoded once); the optimizer still steps once per frame, on window k = cat(fx, yy)[..., k:k+T].
    Returns the list of the Tout detached step losses."""
    losses = []

    def step(code, window, target):
        loss = Fn.slice_mse(model.get_slice_weight(code, x, window, use_vorticity=use_vorticity), target)
        optimizer.zero_grad()
        loss.backward()
        _apply_step(optimizer, scheduler, _trainable(model), max_grad_norm, grad_sync)
        losses.append(loss.detach())

    with ops.weights_frozen():            # the sequence model's weights; LearnSlice's go through no packed GEMM
        if fold_time:
            T, B = fx.shape[-1], x.shape[0]
            seq, codes, slices = _fold_table(sequen_solver, x, fx, yy)
            for k in range(yy.shape[-1]):
                step(codes[k], seq[..., k:k + T], slices[(T + k) * B:(T + k + 1) * B])
        else:
            for t in range(yy.shape[-1]):
                y = yy[..., t:t + 1]
                target = _target_slices(sequen_solver, x, y)
                with torch.no_grad():
                    code = sequen_solver.get_code(x, fx, y)
                step(code, fx, target)
                fx = torch.cat((fx[..., 1:], y), dim=-1)             # the ground truth enters the window
    return losses


def _conv_slices(model, x, fx, code, groups=None):
    """The slice weights of a conv slice predictor.  The code-conditioned predictor (SliceLearner.VorticitySliceLearner
    built with use_code_for_vorticity) reads the code; SliceLearner gets none.  `groups`: the batch is that many folded
    calls, call-major (`forward_folded`: the z-scores stay per call)."""
    if not hasattr(model, "use_code_for_vorticity"):
        return model(x, fx)
    code = code if model.use_code_for_vorticity else None
    return model(x, fx, code) if groups is None else model.forward_folded(x, fx, code, groups=groups)


def _predict_slices(model, sequen_solver, x, fx):
    """(slice weights [B, 1, N, M] of a conv slice predictor, code [B, 1, M, C] of the frozen sequence model)."""
    with torch.no_grad():
        code = sequen_solver.get_code(x, fx, None)
    return _conv_slices(model, x, fx, code), code


def _folded_terms(pred, target, ncalls):
    """sum over the calls, in call order, of F.mse_loss(pred of call k, target of call k): pred, target [ncalls*B, 1, N, M]
    call-major."""
    B = pred.shape[0] // ncalls
    loss = 0
    for k in range(ncalls):
        loss = loss + Fn.slice_mse(pred[k * B:(k + 1) * B], target[k * B:(k + 1) * B]) / (B * pred.shape[2])
    return loss


def slice_predictor_train_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, max_grad_norm=None, grad_sync=None,
                               fold_time=False):
    """One LearnSlice.py:929-962 iteration (train_from_vorticity) of a conv slice predictor (SliceLearner.SliceLearner or
    SliceLearner.VorticitySliceLearner): for each of the Tout = yy.shape[-1] output frames y, the target is the frozen
    encoder's slice weights of y, the code comes from `sequen_solver.get_code` on the window fx [B, N, T] (no gradient), the
    term is F.mse_loss(model's slice weights, target) (the mean over ALL elements: functional.slice_mse scaled by 1 / (B N)),
    and the window slides on with the true frame; the Tout terms are summed, then zero_grad, ONE backward, [grad_sync],
    [clip], step, [scheduler].  Works with torch.optim.AdamW and with `optim.FusedAdamW` (pass `grad_sync=optimizer.sync`).
    `fold_time=True`: the windows hold ground truth only, so everything frozen comes from ONE `sequen_solver.code_windows`
    call and the predictor runs ONE forward on the Tout*B folded samples, call-major (cut where a folded tensor would pass
    the 4 GiB extent); the code-conditioned predictor's z-scores stay per call (`groups`).  The same terms, summed in call
    order.  Returns the detached summed loss."""
    def eager(fx, y):
        return _predict_slices(model, sequen_solver, x, fx)[0]

    def folded(seq, code, slices, k0, g):
        wins = windows(seq, k0, g, fx.shape[-1])                                               # [g*B, N, T], call-major
        return _conv_slices(model, x.repeat(g, *([1] * (x.dim() - 1))), wins, code, groups=g)

    return _summed_slice_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, max_grad_norm, grad_sync, fold_time,
                              eager, folded)


def previous_slice_train_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, max_grad_norm=None, grad_sync=None,
                              fold_time=False):
    """One LearnSlice.py:722-755 iteration (train_from_previous) of SliceLearner.PreviousSliceLearner: for each of the
    Tout = yy.shape[-1] output frames y, the target is the frozen encoder's slice weights of y, the code comes from
    `sequen_solver.get_code` on the window fx [B, N, T], the previous slice is the encoder's slice weights of the window's
    LAST frame (`get_last_slice_weight`), the term is F.mse_loss(model(previous slice, code), target) (functional.slice_mse
    scaled by 1 / (B N)), and the window slides on with the true frame; the Tout terms are summed, then zero_grad, ONE
    backward, [grad_sync], [clip], step, [scheduler].
    `fold_time=True`: targets, codes and previous slices come from ONE `sequen_solver.code_windows` call (previous slice of
    call k = frame T + k - 1 of its table) and the predictor runs ONE forward on the Tout*B folded samples, call-major; the
    same terms, summed in call order.  Returns the detached summed loss."""
    T, B = fx.shape[-1], x.shape[0]

    def eager(fx, y):
        with torch.no_grad():
            code = sequen_solver.get_code(x, fx, y)
            prev = sequen_solver.get_last_slice_weight(x, fx)
        return model(prev, code)

    def folded(seq, code, slices, k0, g):
        return model(slices[(T - 1 + k0) * B:(T - 1 + k0 + g) * B], code)

    return _summed_slice_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, max_grad_norm, grad_sync, fold_time,
                              eager, folded)


def _summed_slice_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, max_grad_norm, grad_sync, fold_time, eager,
                       folded):
    """The frame of slice_predictor_train_step and previous_slice_train_step: the Tout F.mse_loss terms against the frozen
    encoder's slice weights of each true frame, summed in call order, zero_grad, ONE backward, `_apply_step` on the
    trainable parameters.  `eager(fx, y)`: the prediction of one call on the window fx, which then slides on with y;
    `folded(seq, code, slices, k0, g)`: the prediction of calls k0 .. k0+g-1 on `_fold_table`'s seq and slices and their
    codes [g*B, 1, M, C], call-major."""
    loss = 0
    with ops.weights_frozen():
        if fold_time:
            T, B, n = fx.shape[-1], x.shape[0], yy.shape[-1]
            seq, codes, slices = _fold_table(sequen_solver, x, fx, yy)
            for k0, g in groups(n, _slice_fold_group(model, n, B, x.shape[1])):
                pred = folded(seq, codes[k0:k0 + g].reshape(g * B, *codes.shape[2:]), slices, k0, g)
                loss = loss + _folded_terms(pred, slices[(T + k0) * B:(T + k0 + g) * B], g)
        else:
            for t in range(yy.shape[-1]):
                y = yy[..., t:t + 1]
                target = _target_slices(sequen_solver, x, y)
                pred = eager(fx, y)
                loss = loss + Fn.slice_mse(pred, target) / (pred.shape[0] * pred.shape[2])
                fx = torch.cat((fx[..., 1:], y), dim=-1)             # the ground truth enters the window
        optimizer.zero_grad()
        loss.backward()
    _apply_step(optimizer, scheduler, _trainable(model), max_grad_norm, grad_sync)
    return loss.detach()


def _decode_step(sequen_solver, slice_weights, code):
    """The rollouts' feedback: decode `code` with `slice_weights` (left in sequen_solver.slice_weights) and apply
    mlp2(ln_3(.)) -> [B, N, 1]."""
    sequen_solver.slice_weights = slice_weights.contiguous()
    return sequen_solver.readout(code, sequen_solver.slice_weights)


@torch.no_grad()
def previous_slice_rollout(model, sequen_solver, x, fx, nsteps):
    """The evaluation loop of train_from_previous (LearnSlice.py:663-706) without its prints and plots: every step takes the
    code of the frozen sequence model on the window fx [B, N, T], the encoder's slice weights of the window's last frame,
    the predictor's RAW output for them, decodes the code with THAT output (set as sequen_solver.slice_weights), applies
    mlp2(ln_3(.)) and feeds the prediction back into the window.  No ground truth is used.  Returns [B, N, nsteps]."""
    preds = []
    with ops.weights_frozen():
        for _ in range(nsteps):
            code = sequen_solver.get_code(x, fx, None)
            prev = sequen_solver.get_last_slice_weight(x, fx)
            pred = _decode_step(sequen_solver, model(prev, code), code)
            preds.append(pred)
            fx = torch.cat((fx[..., 1:], pred), dim=-1)
    return torch.cat(preds, -1)


@torch.no_grad()
def slice_predictor_rollout(model, sequen_solver, x, fx, nsteps):
    """The evaluation loop of train_from_vorticity (LearnSlice.py:861-913) without its prints and plots: every step takes
    the code of the frozen sequence model on the window fx [B, N, T], the slice weights that the predictor makes of the
    window (and the code), decodes the code with THOSE weights, applies mlp2(ln_3(.)) and feeds the prediction back into
    the window.  No ground truth is used.  Returns the predictions [B, N, nsteps]."""
    preds = []
    with ops.weights_frozen():
        for _ in range(nsteps):
            sw, code = _predict_slices(model, sequen_solver, x, fx)
            pred = _decode_step(sequen_solver, sw, code)
            preds.append(pred)
            fx = torch.cat((fx[..., 1:], pred), dim=-1)
    return torch.cat(preds, -1)


@torch.no_grad()
def sequensolver_rollout(model, x, fx, yy, use_gt=True):
    """SequenSolver.py:613-630: Tout = yy.shape[-1] calls with the PREDICTION fed back into the window (y still supplies
    the slice weights when use_gt=True).  Also the two evaluation loops of SequenSolverMerged.py on its model: the one
    inside train() passes use_gt=True, train(eval=True) use_gt=False; either way that model decodes with predicted slice
    weights.  Returns (pred [B, N, Tout], summed step loss, full loss)."""
    loss_fn = TestLoss(size_average=False)
    bsz = x.shape[0]
    loss, preds = 0, []
    with ops.weights_frozen():
        for t in range(yy.shape[-1]):
            y = yy[..., t:t + 1]
            im = model(x, fx, y, use_gt=use_gt)
            loss = loss + loss_fn(im.reshape(bsz, -1), y.reshape(bsz, -1))
            preds.append(im)
            fx = torch.cat((fx[..., 1:], im), dim=-1)
    pred = torch.cat(preds, -1)
    return pred, loss, loss_fn(pred.reshape(bsz, -1), yy.reshape(bsz, -1))


@torch.no_grad()
def learned_slice_rollout(model, learner, x, fx, yy, unified_pos=1, use_vorticity=1):
    """SequenSolver.py:553-568: Tout = yy.shape[-1] prediction-feedback calls of `model.solve_with_slice_learner` with the
    LearnSlice module `learner` (the caller's one instance: the script builds and loads it once per frame).  Returns the
    full rel-L2 of the batch."""
    bsz, preds = fx.shape[0], []
    with ops.weights_frozen():
        for t in range(yy.shape[-1]):
            im = model.solve_with_slice_learner(learner, x, fx, yy[..., t:t + 1], unified_pos=unified_pos,
                                                use_vorticity=use_vorticity)
            preds.append(im)
            fx = torch.cat((fx[..., 1:], im), dim=-1)
    return TestLoss(size_average=False)(torch.cat(preds, -1).reshape(bsz, -1), yy.reshape(bsz, -1))


# ------------------------------------------------------------------------------ epoch loops of the reference drivers
def _device_of(model):
    return next(model.parameters()).device


def _positions_cache(pos1):
    """positions(bsz): the mesh `pos1` [1, N, 2] as ONE contiguous [bsz, N, 2] copy per batch size (full and short batch),
    not one per sample."""
    pos = {}

    def positions(bsz):
        if bsz not in pos:
            pos[bsz] = pos1.expand(bsz, -1, -1).contiguous()
        return pos[bsz]

    return positions


def _epoch_batches(dataset, batch_size, ep, epoch_orders, generator):
    """Shuffled batches with the short last batch kept (DataLoader(shuffle=True), drop_last=False); `epoch_orders[ep]`
    replays a recorded permutation instead."""
    if epoch_orders is not None:
        return dataset.batches(batch_size, order=epoch_orders[ep])
    return dataset.batches(batch_size, shuffle=True, generator=generator)


def _save_state(module, save_path):
    """torch.save of the state_dict (CPU tensors, the reference's key names: loads strict=True into its Model)."""
    folder = os.path.dirname(save_path)
    if folder:
        os.makedirs(folder, exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in module.state_dict().items()}, save_path)


def _fit(model, *, epochs, n_acc, batches, train_batch, test_pass, metrics, on_epoch, save_path, save_every, save_module=None,
         per_epoch=None):
    """The epoch loop that the fit_* drivers share.  Each epoch: model.train(); a zeroed float64 accumulator `acc` [n_acc]
    on the model's device; `train_batch(batch, acc)` for every batch of `batches(ep)`; `per_epoch()` where given (a
    scheduler stepped per epoch); model.eval(); `test_pass(acc)`; ONE acc.tolist(), the epoch's only host synchronisation;
    `metrics(a)` makes the epoch's dict of that list; `on_epoch(ep, dict)`; `save_module` (default: the model) is saved
    when ep % save_every == 0, and once more after the last epoch.  Returns the list of the dicts."""
    dev = _device_of(model)
    save_module = model if save_module is None else save_module
    history = []
    for ep in range(epochs):
        model.train()
        acc = torch.zeros(n_acc, dtype=torch.float64, device=dev)
        for batch in batches(ep):
            train_batch(batch, acc)
        if per_epoch is not None:
            per_epoch()
        model.eval()
        test_pass(acc)
        history.append(metrics(acc.tolist()))
        if on_epoch is not None:
            on_epoch(ep, history[-1])
        if save_path is not None and ep % save_every == 0:
            _save_state(save_module, save_path)
    if save_path is not None:
        _save_state(save_module, save_path)
    return history


def _evaluate(model, n_acc, test_pass, metrics):
    """The test half of one `_fit` epoch alone: a zeroed float64 accumulator [n_acc] on the model's device, model.eval(),
    `test_pass(acc)`, ONE acc.tolist(), `metrics(a)`.  What every evaluate_* returns."""
    acc = torch.zeros(n_acc, dtype=torch.float64, device=_device_of(model))
    model.eval()
    test_pass(acc)
    return metrics(acc.tolist())


# the test half of each family's epoch dict: fit_X and evaluate_X both read it (`a`: the accumulator of X's test pass)
_ns_test_metrics = lambda a, ntest, calls: dict(test_step=a[2] / ntest / calls, test_full=a[3] / ntest)
_plas_test_metrics = lambda a, ntest, T: dict(test_step=a[1] / ntest / T, test_full=a[2] / ntest)
_rel_err = lambda total, ntest: dict(rel_err=total / ntest)                     # darcy and the static drivers


def _graphed_or_eager(graphed, batch_size, build, replay, eager):
    """run(*batch, key=None) of a loop with a graph mode.  A full batch (batch[0].shape[0] == batch_size) of a graphed loop
    goes to `replay(graph, *batch)`, where `graph = build(*batch)` is made of the first full batch with that `key` (one
    graph per key: the look-ahead of the SOL loops; the other loops have the one key None); every other batch, and every
    batch of an eager loop, goes to `eager(*batch)`.  A key that is given is handed on to the three as their last argument."""
    graphs = {}

    def run(*batch, key=None):
        args = batch if key is None else batch + (key,)
        if not (graphed and batch[0].shape[0] == batch_size):
            return eager(*args)
        if key not in graphs:
            graphs[key] = build(*args)
        return replay(graphs[key], *args)

    return run


@torch.no_grad()
def _rollout_test_pass(model, test, batch_size, T, step, loss_fn, acc, full, fused, calls=None, graphed=False, graphs=None):
    """The prediction-feedback test pass of the NS scripts (exp_ns.py:225-241, ns_vorticity_unrolling.py:264-286,
    ns_velocity.py:238-254): acc[2] += the summed step losses, acc[3] += the loss of the whole trajectory (full); every
    value also goes to `calls` where that is a list.  With `fused` (the velocity loops) and where
    `scored_rollout_supported` says so it runs on `scored_rollout` (graphed: full batches replay one GraphedScoredRollout,
    kept in the caller's dict `graphs`); otherwise the torch loop, whose step losses follow `_step_loss(fused)`."""
    for x, fx, yy in test.batches(batch_size):
        yy = yy[..., :T]
        if fused and scored_rollout_supported(model, x, fx, yy, step, loss_fn):
            if graphed and x.shape[0] == batch_size:
                if "rollout" not in graphs:
                    graphs["rollout"] = GraphedScoredRollout(model, x, fx, yy, step)
                step_ratio, full_ratio, _ = graphs["rollout"].run(x, fx, yy)
            else:
                step_ratio, full_ratio, _ = scored_rollout(model, x, fx, yy, step)
            per_step = step_ratio.sum(1)
            acc[2] += per_step.sum()
            if calls is not None:
                calls.extend(per_step.unbind(0))
            if full:
                total = full_ratio.sum()
                acc[3] += total
                if calls is not None:
                    calls.append(total)
            continue
        loss, preds = 0, []
        with ops.weights_frozen():
            for t in range(0, T, step):
                im = model(x, fx=fx)
                loss = loss + _step_loss(loss_fn, im, yy, t, fused, calls)
                preds.append(im)
                fx = torch.cat((fx[..., step:], im), dim=-1)
        acc[2] += loss
        if full:
            acc[3] += _full_loss(loss_fn, preds, yy, calls)


def evaluate_ns(model, test, batch_size, T=10, step=1, loss_fn=None):
    """The test pass alone (exp_ns.py:137-183 without the plots): {'test_step', 'test_full'} normalised like fit_ns."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    return _evaluate(model, 4, lambda acc: _rollout_test_pass(model, test, batch_size, T, step, loss_fn, acc, True, False),
                     lambda a: _ns_test_metrics(a, len(test), T / step))


@torch.no_grad()
def _darcy_test_pass(model, test, batch_size, positions, y_normalizer, loss_fn, acc):
    """exp_darcy.py:243-254: the prediction is decoded, the target is the raw solution; acc[2] += summed rel-L2."""
    for fx, y in test.batches(batch_size):
        out = model(positions(fx.shape[0]), fx=fx.unsqueeze(-1)).squeeze(-1)
        acc[2] += loss_fn(y_normalizer.decode(out), y)


def _darcy_setup(model, data, want_train=True):
    """(device, y-normaliser ON the device, train set or None, test set, positions(bsz)).  The caller's normaliser is left
    where it is: a shallow copy is moved."""
    import copy
    from .data import ResidentDataset, grid_positions
    dev = _device_of(model)
    yn = copy.copy(data["y_normalizer"]).to(dev)
    train = ResidentDataset(data["x_train"], data["y_train"], device=dev) if want_train else None
    test = ResidentDataset(data["x_test"], data["y_test"], device=dev)
    return dev, yn, train, test, _positions_cache(grid_positions(data["s"]).to(dev))


def evaluate_darcy(model, data, batch_size, loss_fn=None):
    """The test pass alone (exp_darcy.py:154-203 without the plots): {'rel_err'} = summed rel-L2 / ntest."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    _, yn, _, test, positions = _darcy_setup(model, data, want_train=False)
    return _evaluate(model, 3, lambda acc: _darcy_test_pass(model, test, batch_size, positions, yn, loss_fn, acc),
                     lambda a: _rel_err(a[2], len(test)))


def fit_ns(model, optimizer, scheduler, train, test, *, epochs, batch_size, T=10, step=1, max_grad_norm=None, loss_fn=None,
           epoch_orders=None, generator=None, save_path=None, save_every=100, graphed=False, grad_sync=None, on_epoch=None):
    """The epoch loop of exp_ns.main() (exp_ns.py:184-257).  `train` / `test`: data.ResidentDataset of (x [n, N, 2],
    fx [n, N, T_in], yy [n, N, >= T]) on the model's device (any device: a CPU module goes through the same loop).

    Each epoch: model.train(); shuffled batches, the short last batch kept; per batch the teacher-forced iteration
    `train_step` (T/step model calls, summed rel-L2, zero_grad, backward, [grad_sync], [clip], optimizer.step(),
    scheduler.step()); then model.eval() and the prediction-feedback test pass under no_grad.  The caller builds the
    scheduler (the reference: OneCycleLR(max_lr=lr, epochs=epochs, steps_per_epoch=ceil(ntrain / batch_size))).

    Returns one dict per epoch with the metrics the reference prints, unrounded (exp_ns.py:243-246):
    train_step = sum / ntrain / (T / step), train_full = sum / ntrain, test_step = sum / ntest / (T / step),
    test_full = sum / ntest.  The sums are accumulated on the device: ONE host synchronisation per epoch.

    `epoch_orders[ep]`: the sample order of epoch ep (a recorded permutation); otherwise a fresh permutation from
    `generator`.  `save_path`: the state_dict is written when ep % save_every == 0 and after the last epoch.
    `graphed=True` (CUDA, optim.FusedAdamW): full batches replay one GraphedTrainStep (bit-identical to the eager
    iteration); the short last batch runs eagerly.  `grad_sync` is passed through to the eager iteration; a replayed batch
    calls the optimizer's own `sync` (the same bucket), and clips through the optimizer only: `max_grad_norm` together
    with `graphed=True` raises.
    `on_epoch(ep, metrics)`: called after every epoch's synchronisation (progress lines of a command line)."""
    if graphed:
        _graphed_refusals("fit_ns", optimizer, max_grad_norm, one_rank=False)
    loss_fn = loss_fn or TestLoss(size_average=False)
    run = _graphed_or_eager(
        graphed, batch_size,
        lambda x, fx, yy: GraphedTrainStep(model, optimizer, scheduler, x, fx, yy, step=step, loss_fn=loss_fn),
        lambda graph, x, fx, yy: graph(x, fx, yy),
        lambda x, fx, yy: train_step(model, optimizer, scheduler, x, fx, yy, step=step, max_grad_norm=max_grad_norm,
                                     grad_sync=grad_sync, loss_fn=loss_fn))
    return _fit_teacher_forced(model, train, test, run, False, None, False, epochs=epochs, batch_size=batch_size, T=T,
                               step=step, loss_fn=loss_fn, epoch_orders=epoch_orders, generator=generator,
                               save_path=save_path, save_every=save_every, on_epoch=on_epoch)


def _fit_teacher_forced(model, train, test, run, fused, calls, graphed, *, epochs, batch_size, T, step, loss_fn, epoch_orders,
                        generator, save_path, save_every, on_epoch):
    """The frame of fit_ns and fit_velocity, which differ in `fused`, in the graph class behind `run` and in whether
    `calls` is threaded through: run(x, fx, yy[..., :T]) -> (step loss, full loss) per batch, the prediction-feedback test
    pass (with `graphed`: on one GraphedScoredRollout), the four metrics of exp_ns.py:243-246."""
    ntrain, ntest, ncalls, graphs = len(train), len(test), T / step, {}

    def train_batch(batch, acc):
        x, fx, yy = batch
        loss, full = run(x, fx, yy[..., :T])
        acc[0] += loss
        acc[1] += full

    return _fit(model, epochs=epochs, n_acc=4, batches=lambda ep: _epoch_batches(train, batch_size, ep, epoch_orders, generator),
                train_batch=train_batch,
                test_pass=lambda acc: _rollout_test_pass(model, test, batch_size, T, step, loss_fn, acc, True, fused, calls,
                                                         graphed, graphs),
                metrics=lambda a: dict(train_step=a[0] / ntrain / ncalls, train_full=a[1] / ntrain,
                                       **_ns_test_metrics(a, ntest, ncalls)),
                on_epoch=on_epoch, save_path=save_path, save_every=save_every)


def fit_unrolled(sol_model, optimizer, scheduler, train, test, *, epochs, batch_size, T=10, step=1, look_ahead=1,
                 max_look_ahead=10, loss_fn=None, epoch_orders=None, generator=None, save_path=None, save_every=100,
                 grad_sync=None, on_epoch=None):
    """The epoch loop of ns_vorticity_unrolling.main() (ns_vorticity_unrolling.py:204-329) on the SOL wrapper
    (model/SOL_Transolver_Structured_Mesh_2D).  The look-ahead follows `LookAheadCurriculum` (it doubles, capped at
    `max_look_ahead`, when ep % thresh == 0 and ep >= thresh; thresh = epochs / 2 is a float that then halves); per
    batch `unrolled_train_iteration` (BPTT through the chained calls), zero_grad, backward, [grad_sync], step,
    scheduler.step(): this loop never clips.  The test pass (:264-286) runs the inner `transolver_model` with
    prediction feedback and keeps the step loss only.

    Returns one dict per epoch: train_step = the RAW epoch sum (what :257 prints), test_step = sum / ntest / (T / step),
    look_ahead = the epoch's look-ahead.  One host synchronisation per epoch.  Saves
    `sol_model.transolver_model.state_dict()` (ep % save_every == 0 and after the last epoch).  No graph mode."""
    return _fit_sol("fit_unrolled", sol_model, optimizer, scheduler, train, test,
                    LookAheadCurriculum(epochs, look_ahead, max_look_ahead),
                    lambda sol, x, fx, yy, la, step, loss_fn, vals: unrolled_train_iteration(sol, x, fx, yy, la, step, loss_fn),
                    accumulate=True, fused=False, zero_grad_kw={}, epochs=epochs, batch_size=batch_size, T=T, step=step,
                    loss_fn=loss_fn, epoch_orders=epoch_orders, generator=generator, save_path=save_path,
                    save_every=save_every, graphed=False, grad_sync=grad_sync, on_epoch=on_epoch, calls=None)


def fit_darcy(model, optimizer, scheduler, data, *, epochs, batch_size, max_grad_norm=None, loss_fn=None,
              epoch_orders=None, generator=None, save_path=None, save_every=100, fused=True, grad_sync=None,
              on_epoch=None, graphed=False):
    """The epoch loop of exp_darcy.main() (exp_darcy.py:205-268).  `data`: the dict `data.load_darcy_mat` returns
    (encoded x_train / y_train / x_test, the RAW y_test, both normalisers, s, dx); everything is moved to the model's
    device, the positions are `data.grid_positions(s)`.

    Per batch `darcy_train_step` (zero_grad, one model call, `darcy_loss`, backward, [grad_sync], [clip], step,
    scheduler.step()), with the fused Darcy-loss kernels where they apply (`fused=True`: fp32 CUDA tensors; a float64
    target or a CPU module keeps the torch path, which calls `loss_fn`).  Test pass (always `loss_fn`): the prediction is DECODED, the target is the raw solution (never
    encoded), rel-L2 summed.  Returns one dict per epoch: reg = sum of the derivative losses / ntrain, train_loss = sum
    of the l2 losses / ntrain, rel_err = sum / ntest.  One host synchronisation per epoch.

    Quirk of the reference kept OUT of this function: exp_darcy builds its OneCycleLR with epochs=500 whatever
    --epochs says (its module global `epochs`), so a shorter run never leaves the warm-up.  The caller builds the
    scheduler; pass OneCycleLR(..., epochs=500, ...) to reproduce the reference, or the real count not to.

    `graphed=True` (CUDA, optim.FusedAdamW, one rank, the fused loss): full batches replay ONE GraphedCallStep, the whole
    iteration with the optimizer step, bit-identical to the eager one; the short last batch runs eagerly on the same
    moments, step count and scheduler.  Clips through the optimizer only: `max_grad_norm` together with it raises."""
    if graphed:
        _graphed_refusals("fit_darcy", optimizer, max_grad_norm)
        _capturable_model(model, "fit_darcy")
        if not fused:
            raise ValueError("fit_darcy(graphed=True) captures the fused Darcy loss: leave fused=True")
    test_loss = loss_fn or TestLoss(size_average=False)
    _, yn, train, test, positions = _darcy_setup(model, data)
    s, dx = data["s"], data["dx"]
    ntrain, ntest = len(train), len(test)
    run = _graphed_or_eager(
        graphed, batch_size,
        lambda fx, y: GraphedCallStep(model, optimizer, scheduler, (positions(batch_size), fx.clone(), y.clone()),
                                      _darcy_body(yn, dx, s)),
        lambda graph, fx, y: graph(None, fx, y),
        lambda fx, y: darcy_train_step(model, optimizer, scheduler, positions(fx.shape[0]), fx, y, yn, dx, s,
                                       max_grad_norm=max_grad_norm, grad_sync=grad_sync, fused=fused, loss_fn=loss_fn))

    def train_batch(batch, acc):
        _, l2, deriv = run(*batch)
        acc[0] += l2
        acc[1] += deriv

    return _fit(model, epochs=epochs, n_acc=3, batches=lambda ep: _epoch_batches(train, batch_size, ep, epoch_orders, generator),
                train_batch=train_batch, test_pass=lambda acc: _darcy_test_pass(model, test, batch_size, positions, yn, test_loss, acc),
                metrics=lambda a: dict(reg=a[1] / ntrain, train_loss=a[0] / ntrain, **_rel_err(a[2], ntest)),
                on_epoch=on_epoch, save_path=save_path, save_every=save_every)


# ------------------------------------------------------------------ exp_airfoil / exp_pipe / exp_elas: one call per batch
def _rel_decoded(loss_fn, out, y, y_normalizer):
    """The training loss of the static drivers: rel-L2 of the decoded prediction against the decoded target.  A loss
    object with `rel_decoded` (utils.testloss.TestLoss; FusedTestLoss runs it on the decoded rel-L2 kernels, with the
    normaliser read on the device) is asked for it; any other callable gets the two decoded tensors."""
    if hasattr(loss_fn, "rel_decoded"):
        return loss_fn.rel_decoded(out, y, y_normalizer)
    if y_normalizer is None:
        return loss_fn(out, y)
    return loss_fn(y_normalizer.decode(out), y_normalizer.decode(y))


def static_train_step(model, optimizer, scheduler, x, y, y_normalizer=None, max_grad_norm=None, grad_sync=None,
                      loss_fn=None):
    """exp_airfoil.py:187-199 / exp_pipe.py:204-221 / exp_elas.py:163-176: zero_grad, ONE call model(x, None) (fun_dim = 0:
    the placeholder path), the rel-L2 of the decoded prediction and target (raw without a normaliser), backward,
    [grad_sync], [clip], step, [scheduler] (pass None where the schedule is stepped per epoch).  Returns the detached
    loss."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    optimizer.zero_grad(set_to_none=False)
    out = model(x, None).squeeze(-1)
    loss = _rel_decoded(loss_fn, out, y, y_normalizer)
    loss.backward()
    _apply_step(optimizer, scheduler, model.parameters(), max_grad_norm, grad_sync)
    return loss.detach()


@torch.no_grad()
def _static_test_pass(model, test, batch_size, y_normalizer, loss_fn, acc):
    """exp_pipe.py:229-235: the prediction is decoded (where there is a normaliser), the target is RAW; acc[1] += rel-L2."""
    for x, y in test.batches(batch_size):
        out = model(x, None).squeeze(-1)
        acc[1] += loss_fn(out if y_normalizer is None else y_normalizer.decode(out), y)


def _static_setup(model, data, want_train=True):
    import copy
    from .data import ResidentDataset
    dev = _device_of(model)
    yn = data.get("y_normalizer")
    yn = None if yn is None else copy.copy(yn).to(dev)        # the caller's normaliser stays where it is
    train = ResidentDataset(data["x_train"], data["y_train"], device=dev) if want_train else None
    return dev, yn, train, ResidentDataset(data["x_test"], data["y_test"], device=dev)


def evaluate_static(model, data, batch_size, loss_fn=None):
    """The test pass alone (the `eval` branch of the three scripts without the plots): {'rel_err'} = summed rel-L2 / ntest."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    _, yn, _, test = _static_setup(model, data, want_train=False)
    return _evaluate(model, 2, lambda acc: _static_test_pass(model, test, batch_size, yn, loss_fn, acc),
                     lambda a: _rel_err(a[1], len(test)))


def fit_static(model, optimizer, scheduler, data, *, epochs, batch_size, max_grad_norm=None, loss_fn=None,
               epoch_orders=None, generator=None, save_path=None, save_every=100, scheduler_per_epoch=False, grad_sync=None,
               on_epoch=None, graphed=False):
    """The epoch loop of exp_airfoil.main() (:182-226), exp_pipe.main() (:199-249) and exp_elas.main() (:158-204).  `data`:
    the dict of `data.load_airfoil_npy` / `load_pipe_npy` / `load_elas_npy` (x_train [n, N, 2], y_train [n, N], x_test, the
    RAW y_test, y_normalizer or None); everything is moved to the model's device.

    Per batch `static_train_step`: one model(x, None) call and the rel-L2 loss.  What the three scripts do differently
    follows from `data["y_normalizer"]` and one flag, and is kept:
      * airfoil (no normaliser): raw loss, raw test metric;
      * pipe: the training loss decodes prediction AND target; the test pass decodes the prediction, its target is raw;
      * elas: as pipe, and the scheduler is stepped once per EPOCH (exp_elas.py:177): `scheduler_per_epoch=True`.
    The caller builds the scheduler.  exp_airfoil / exp_pipe: OneCycleLR(max_lr=lr, epochs=epochs, steps_per_epoch=
    ceil(ntrain / batch_size)).  exp_elas.py:102 builds CosineAnnealingLR(T_max=epochs) from an UNDEFINED global `epochs`
    and raises as shipped; this project's command line passes CosineAnnealingLR(T_max=args.epochs), the evident intent.

    `loss_fn`: a TestLoss(size_average=False)-like object; utils.testloss.FusedTestLoss runs the training loss on the
    decoded rel-L2 kernels.  Returns one dict per epoch: train_loss = sum / ntrain, rel_err = sum / ntest.  Accumulators
    stay on the device: ONE host synchronisation per epoch.  `epoch_orders`, `generator`, `save_path` / `save_every`,
    `grad_sync`, `on_epoch`: as fit_ns.  `graphed`: as fit_darcy (the loss inside the capture is `_rel_decoded` with the
    normaliser or none; a per-epoch scheduler stays outside it)."""
    if graphed:
        _graphed_refusals("fit_static", optimizer, max_grad_norm)
        _capturable_model(model, "fit_static")
    loss_fn = loss_fn or TestLoss(size_average=False)
    _, yn, train, test = _static_setup(model, data)
    ntrain, ntest = len(train), len(test)
    batch_sched = None if scheduler_per_epoch else scheduler
    run = _graphed_or_eager(
        graphed, batch_size,
        lambda x, y: GraphedCallStep(model, optimizer, batch_sched, (x.clone(), y.clone()), _static_body(loss_fn, yn)),
        lambda graph, x, y: graph(x, y)[0],
        lambda x, y: static_train_step(model, optimizer, batch_sched, x, y, yn, max_grad_norm=max_grad_norm,
                                       grad_sync=grad_sync, loss_fn=loss_fn))

    def train_batch(batch, acc):
        acc[0] += run(*batch)

    return _fit(model, epochs=epochs, n_acc=2, batches=lambda ep: _epoch_batches(train, batch_size, ep, epoch_orders, generator),
                train_batch=train_batch, test_pass=lambda acc: _static_test_pass(model, test, batch_size, yn, loss_fn, acc),
                metrics=lambda a: dict(train_loss=a[0] / ntrain, **_rel_err(a[1], ntest)),
                on_epoch=on_epoch, save_path=save_path, save_every=save_every,
                per_epoch=scheduler.step if scheduler_per_epoch and scheduler is not None else None)


# ------------------------------------------------------------------ exp_plas: T time-conditioned calls and steps per batch
def plas_train_step(model, optimizer, x, fx, tim, yy, max_grad_norm=None, grad_sync=None, loss_fn=None):
    """exp_plas.py:242-253 on one batch: for every t < T = yy.shape[-1]: ONE call model(x, fx, T=tim[:, t:t+1]), the raw
    rel-L2 of the [B, N * 4] prediction against yy[..., t:t+1] (read in place through its strides by the fused loss),
    zero_grad, backward, [grad_sync], [clip], optimizer.step(): T optimizer steps.  The scheduler is the caller's (once
    per batch).  Returns the detached sum of the T step losses."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    bsz = x.shape[0]
    total = 0
    for t in range(yy.shape[-1]):
        im = model(x, fx, T=tim[:, t:t + 1].reshape(bsz, 1))
        loss = _rel_decoded(loss_fn, im.reshape(bsz, -1), yy[..., t:t + 1], None)
        total = total + loss.detach()
        optimizer.zero_grad(set_to_none=False)
        loss.backward()
        _apply_step(optimizer, None, model.parameters(), max_grad_norm, grad_sync)
    return total


@torch.no_grad()
def _plas_test_pass(model, test, batch_size, positions, t, loss_fn, acc):
    """exp_plas.py:260-277: acc[1] += the T step losses, acc[2] += the loss of the whole [B, N * 4 * T] trajectory."""
    for fx, yy in test.batches(batch_size):
        bsz = fx.shape[0]
        x, tim = positions(bsz), t.expand(bsz, -1)
        loss, preds = 0, []
        with ops.weights_frozen():
            for k in range(yy.shape[-1]):
                im = model(x, fx, T=tim[:, k:k + 1].reshape(bsz, 1))
                loss = loss + _rel_decoded(loss_fn, im.reshape(bsz, -1), yy[..., k:k + 1], None)
                preds.append(im.unsqueeze(-1))
        acc[1] += loss
        acc[2] += loss_fn(torch.cat(preds, -1).reshape(bsz, -1), yy.reshape(bsz, -1))


def _plas_setup(model, data, want_train=True):
    from .data import ResidentDataset
    dev = _device_of(model)
    train = ResidentDataset(data["x_train"], data["y_train"], device=dev) if want_train else None
    test = ResidentDataset(data["x_test"], data["y_test"], device=dev)
    return dev, train, test, _positions_cache(data["pos"].to(dev)), data["t"].to(dev)


def evaluate_plas(model, data, batch_size, loss_fn=None):
    """The test pass alone (exp_plas.py:168-231 without the plots): {'test_step', 'test_full'} normalised like fit_plas."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    _, _, test, positions, t = _plas_setup(model, data, want_train=False)
    return _evaluate(model, 3, lambda acc: _plas_test_pass(model, test, batch_size, positions, t, loss_fn, acc),
                     lambda a: _plas_test_metrics(a, len(test), t.numel()))


def fit_plas(model, optimizer, scheduler, data, *, epochs, batch_size, max_grad_norm=None, loss_fn=None, epoch_orders=None,
             time_orders=None, generator=None, save_path=None, save_every=100, grad_sync=None, on_epoch=None,
             graphed=False):
    """The epoch loop of exp_plas.main() (exp_plas.py:233-292).  `data`: the dict of `data.load_plas_mat` (encoded x_train
    [n, N, 1], y_train [n, N, 4, T], x_test, y_test, pos [1, N, 2], t [T]); everything is moved to the model's device.

    The train collate (`random_collate_fn`, :51-85) permutes the T timesteps of every sample on its own: `time_orders[ep]`
    [ntrain, T] replays recorded permutations, row i for the i-th sample IN THE EPOCH'S ORDER; otherwise they are drawn
    from `generator`.  Per batch `plas_train_step` (T model calls with T optimizer steps), then scheduler.step() ONCE
    (:255; the caller builds OneCycleLR(max_lr=lr, epochs=epochs, steps_per_epoch=ceil(ntrain / batch_size))).  The test
    pass runs the timesteps in order and keeps the summed step losses and the loss of the whole trajectory.

    Returns one dict per epoch: train_step = sum / ntrain / T, test_step = sum / ntest / T, test_full = sum / ntest
    (:279-282).  One host synchronisation per epoch; `epoch_orders`, `save_path` / `save_every`, `grad_sync`, `on_epoch`:
    as fit_ns.

    `graphed=True` (requirements as fit_darcy): a full batch is T replays of ONE GraphedCallStep (model call with the
    time input, raw rel-L2, backward, optimizer step).  The window fx is written once per batch; between replays only
    the static time vector [B, 1] and column 0 of the static [B, N, 4, T] target are rewritten.  The scheduler steps once
    per batch, as in the eager loop; short batches run eagerly."""
    if graphed:
        _graphed_refusals("fit_plas", optimizer, max_grad_norm)
        _capturable_model(model, "fit_plas")
    loss_fn = loss_fn or TestLoss(size_average=False)
    dev, train, test, positions, t = _plas_setup(model, data)
    ntrain, ntest, T = len(train), len(test), t.numel()

    def batches(ep):       # (fx, yy, perm [B, T]): a batch's time permutations are drawn right after the batch itself
        seen = 0
        for fx, yy in _epoch_batches(train, batch_size, ep, epoch_orders, generator):
            bsz = fx.shape[0]
            if time_orders is not None:
                perm = torch.as_tensor(time_orders[ep], dtype=torch.long)[seen:seen + bsz].to(dev)
            else:
                gdev = dev if generator is None else generator.device
                perm = torch.rand(bsz, T, generator=generator, device=gdev).argsort(dim=1).to(dev)
            seen += bsz
            yield fx, yy, perm

    def replay(graph, fx, tim, yy):
        graph.static[1].copy_(fx)                                            # the window: once per batch
        total = 0
        for k in range(T):
            graph.static[3][..., 0].copy_(yy[..., k])                        # the target column and the time: per replay
            total = total + graph(None, None, tim[:, k:k + 1], None)[0]
        return total

    run = _graphed_or_eager(
        graphed, batch_size,
        lambda fx, tim, yy: GraphedCallStep(model, optimizer, None, (positions(batch_size), fx.clone(), tim[:, :1].clone(), yy.clone()),
                                            _plas_body(loss_fn)),
        replay,
        lambda fx, tim, yy: plas_train_step(model, optimizer, positions(fx.shape[0]), fx, tim, yy, max_grad_norm=max_grad_norm,
                                            grad_sync=grad_sync, loss_fn=loss_fn))

    def train_batch(batch, acc):
        fx, yy, perm = batch
        tim = t[perm]                                                            # [B, T]
        yy = yy.gather(-1, perm[:, None, None, :].expand_as(yy))                 # u[..., permuted_indices] per sample
        acc[0] += run(fx, tim, yy)
        if scheduler is not None:
            scheduler.step()

    return _fit(model, epochs=epochs, n_acc=3, batches=batches, train_batch=train_batch,
                test_pass=lambda acc: _plas_test_pass(model, test, batch_size, positions, t, loss_fn, acc),
                metrics=lambda a: dict(train_step=a[0] / ntrain / T, **_plas_test_metrics(a, ntest, T)),
                on_epoch=on_epoch, save_path=save_path, save_every=save_every)


# ------------------------------------------------------------------------------ latent-sequence family: epoch loops
def _autoencoder_test(model, data):
    """test_pass(acc, batch_size) of the auto-encoder, and positions(bsz): acc[1] += TestLoss(size_average=False) of
    model(x, fx) against fx itself, over `data["test"]` under no_grad (auto_encoder.py:188-197)."""
    from .data import ResidentDataset, grid_positions
    dev = _device_of(model)
    test = ResidentDataset(data["test"], device=dev)
    positions = _positions_cache(grid_positions(data["h"]).to(dev))
    loss_fn = TestLoss(size_average=False)

    @torch.no_grad()
    def test_pass(acc, batch_size):
        for fx, in test.batches(batch_size):
            bsz = fx.shape[0]
            acc[1] += loss_fn(model(positions(bsz), fx=fx).reshape(bsz, -1), fx.reshape(bsz, -1))

    return test_pass, positions


def evaluate_autoencoder(model, data, batch_size, ntest):
    """The test pass of fit_autoencoder alone (auto_encoder.py:135-158 without the plots): {'test_l2'} = summed loss / ntest,
    where `ntest` counts TRAJECTORIES, not frames, as the script divides."""
    test_pass, _ = _autoencoder_test(model, data)
    return _evaluate(model, 2, lambda acc: test_pass(acc, batch_size), lambda a: dict(test_l2=a[1] / ntest))


def fit_autoencoder(model, optimizer, scheduler, data, *, epochs, batch_size, ntrain, ntest, T=10, step=1, max_grad_norm=None,
                    epoch_orders=None, generator=None, save_path=None, save_name=None, save_every=100, grad_sync=None,
                    on_epoch=None):
    """The epoch loop of auto_encoder.main() (auto_encoder.py:160-210) on `data` = data.split_ns_all_frames(...): every
    frame of every trajectory is one sample [n*F, N, 1], and the loss of a batch is TestLoss(size_average=False) of
    model(x, fx) against the input fx itself (`autoencoder_train_step`); the test pass is the same loss under no_grad.

    Returns one dict per epoch with the script's metrics, unrounded and with ITS divisors (auto_encoder.py:199):
    train_step = sum / ntrain / (T / step), test_step = sum / ntest / (T / step), where ntrain / ntest count TRAJECTORIES
    (the script's globals), not frames.  One host synchronisation per epoch.  The state_dict is written when
    ep % save_every == 0 (the script: 100) and after the last epoch, to `save_path`, or, as the script names it, to
    sequential_checkpoints/<save_name>.pt.  `epoch_orders`, `generator`, `grad_sync`, `on_epoch` as fit_ns."""
    from .data import ResidentDataset
    if save_path is None and save_name is not None:
        save_path = os.path.join("sequential_checkpoints", save_name + ".pt")
    train = ResidentDataset(data["train"], device=_device_of(model))
    test_pass, positions = _autoencoder_test(model, data)
    calls = T / step

    def train_batch(batch, acc):
        fx, = batch
        acc[0] += autoencoder_train_step(model, optimizer, scheduler, positions(fx.shape[0]), fx, max_grad_norm=max_grad_norm,
                                         grad_sync=grad_sync)

    return _fit(model, epochs=epochs, n_acc=2, batches=lambda ep: _epoch_batches(train, batch_size, ep, epoch_orders, generator),
                train_batch=train_batch, test_pass=lambda acc: test_pass(acc, batch_size),
                metrics=lambda a: dict(train_step=a[0] / ntrain / calls, test_step=a[1] / ntest / calls),
                on_epoch=on_epoch, save_path=save_path, save_every=save_every)


# what the two reference files' train() loops differ in
SEQUENSOLVER_LOOPS = {
    # SequenSolver.py:572-640.  `if ep > 5: model.freeze_attention(); use_gt = False` sets a flag the calls never read: they
    # pass use_gt=True throughout.  `test_l2_step += ...` and `test_l2_full = ...` (:629-630) stand AFTER the loop over the
    # test batches, so both metrics are the LAST test batch's alone.
    "plain": dict(train_use_gt=True, freeze_after=5, last_test_batch_only=True, first_frame=False),
    # SequenSolverMerged.py:454-523: no freeze, both test sums accumulated, and the loss of the first predicted frame
    "merged": dict(train_use_gt=False, freeze_after=None, last_test_batch_only=False, first_frame=True),
}


def fit_sequensolver(model, optimizer, scheduler, pos, train, test, *, epochs, batch_size=1, variant=None, Tin=None,
                     fold_time=False, max_grad_norm=None, epoch_orders=None, generator=None, save_path=None, save_every=None,
                     grad_sync=None, on_epoch=None, **loop):
    """The epoch loop of the reference's SequenSolver.py / SequenSolverMerged.py train().  `pos` [1, N, P]: the point input of
    every sample (the coordinates, or the 64 unified distances); `train` / `test`: data.ResidentDataset of (fx [n, N, Tin],
    yy [n, N, Tout]) on the model's device.  `variant` "plain" | "merged" picks SEQUENSOLVER_LOOPS (default: by the model's
    class); single entries can be overridden by keyword.

    Each epoch: model.train(); from ep > freeze_after on, model.freeze_attention() (the frozen tensors then stop moving
    with torch.optim.AdamW, whose zero_grad leaves them without a gradient, and with optim.FusedAdamW, whose active ranges
    leave out parameters that no longer require a gradient); shuffled batches through `sequensolver_train_step(use_gt=
    train_use_gt, fold_time=fold_time)`; model.eval() and `sequensolver_rollout(use_gt=True)` (prediction feedback) on
    every test batch.

    Returns one dict per epoch, divided as the scripts divide: train_step = sum / ntrain / Tin, train_full = sum / ntrain,
    test_step = sum / ntest / Tin, test_full = sum / ntest (+ test_first = the first predicted frame's loss / ntest with
    first_frame).  With last_test_batch_only the two test sums are the last test batch's alone, as the plain script
    computes them.  One host synchronisation per epoch.  The scripts save once, after the last epoch: `save_every` None
    does that; `epoch_orders`, `generator`, `grad_sync`, `on_epoch`, `save_path` as fit_ns."""
    if variant is None:
        variant = "merged" if hasattr(model, "sequential_head") else "plain"
    unknown = set(loop) - set(SEQUENSOLVER_LOOPS[variant])
    if unknown:
        raise TypeError(f"fit_sequensolver got unexpected keywords {sorted(unknown)}")
    cfg = dict(SEQUENSOLVER_LOOPS[variant], **loop)
    ntrain, ntest = len(train), len(test)
    Tin = model.T if Tin is None else Tin
    positions = _positions_cache(pos.to(_device_of(model)))
    loss_fn = TestLoss(size_average=False)

    def batches(ep):
        if cfg["freeze_after"] is not None and ep > cfg["freeze_after"]:
            model.freeze_attention()
        return _epoch_batches(train, batch_size, ep, epoch_orders, generator)

    def train_batch(batch, acc):
        fx, yy = batch
        loss, full = sequensolver_train_step(model, optimizer, scheduler, positions(fx.shape[0]), fx, yy,
                                             use_gt=cfg["train_use_gt"], max_grad_norm=max_grad_norm, grad_sync=grad_sync,
                                             fold_time=fold_time)
        acc[0] += loss
        acc[1] += full

    @torch.no_grad()
    def test_pass(acc):
        last = None
        for fx, yy in test.batches(batch_size):
            bsz = fx.shape[0]
            pred, loss, full = sequensolver_rollout(model, positions(bsz), fx, yy, use_gt=True)
            last = (loss, full)
            if not cfg["last_test_batch_only"]:
                acc[2] += loss
                acc[3] += full
            if cfg["first_frame"]:
                acc[4] += loss_fn(pred[..., 0].reshape(bsz, -1), yy[..., 0].reshape(bsz, -1))
        if cfg["last_test_batch_only"] and last is not None:
            acc[2] += last[0]
            acc[3] += last[1]

    def metrics(a):
        m = dict(train_step=a[0] / ntrain / Tin, train_full=a[1] / ntrain, test_step=a[2] / ntest / Tin,
                 test_full=a[3] / ntest)
        if cfg["first_frame"]:
            m["test_first"] = a[4] / ntest
        return m

    history = _fit(model, epochs=epochs, n_acc=5, batches=batches, train_batch=train_batch, test_pass=test_pass,
                   metrics=metrics, on_epoch=on_epoch, save_path=save_path if save_every is not None else None,
                   save_every=save_every)
    if save_path is not None and save_every is None:
        _save_state(model, save_path)
    return history


def evaluate_sequensolver(model, pos, test, ntest, batch_size=1, slice_learner=None):
    """train(eval=True) of the two scripts without the prints and plots: {'test_full'} = the summed full rel-L2 of every
    test batch's prediction-feedback rollout / `ntest` (the caller's count).  The merged model (SequenSolverMerged.py) is
    given no `slice_learner` and runs `sequensolver_rollout(use_gt=False)`; the plain one (SequenSolver.py:541-570) is
    given its LearnSlice module and runs `learned_slice_rollout`."""
    positions = _positions_cache(pos.to(_device_of(model)))

    def test_pass(acc):
        for fx, yy in test.batches(batch_size):
            x = positions(fx.shape[0])
            if slice_learner is None:
                acc[0] += sequensolver_rollout(model, x, fx, yy, use_gt=False)[2]
            else:
                acc[0] += learned_slice_rollout(model, slice_learner, x, fx, yy)

    return _evaluate(model, 1, test_pass, lambda a: dict(test_full=a[0] / ntest))


# ------------------------------------------------------------------------------ slice learners: epoch loops
SLICE_LEARNER_KINDS = ("learnslice", "vorticity", "previous")


def slice_learner_kind(model):
    """The trainer a slice learner belongs to, by its class: LearnSlice.LearnSlice -> "learnslice" (train, :472-588),
    SliceLearner.SliceLearner / VorticitySliceLearner -> "vorticity" (train_from_vorticity, :924-1006),
    SliceLearner.PreviousSliceLearner -> "previous" (train_from_previous, :717-793)."""
    if hasattr(model, "weight_projection_form_slice"):
        return "previous"
    if hasattr(model, "in_project_x"):
        return "vorticity"
    if hasattr(model, "weight_projection"):
        return "learnslice"
    raise TypeError(f"{type(model).__name__} is none of the slice learners (LearnSlice, SliceLearner, VorticitySliceLearner, "
                    "PreviousSliceLearner)")


@torch.no_grad()
def slice_learner_test_loss(kind, model, sequen_solver, x, fx, yy, use_vorticity=0):
    """The loss of ONE test batch as the `kind`'s script computes it inside its epoch loop, summed over the Tout frames
    (the caller divides).  Every frame: the target is the encoder's slice weights of the true frame y, the code comes from
    the window.
      "learnslice" (:544-586): functional.slice_mse of get_slice_weight; the code is decoded with the TARGET slice
                   weights and the prediction enters the window.
      "vorticity"  (:975-1004): F.mse_loss of the predictor's slice weights; the code is decoded with the PREDICTED
                   weights and the prediction enters the window.
      "previous"   (:768-791): F.mse_loss of the predictor's raw output; the window NEVER slides (the script does not update
                   fx in this loop), so code and previous slice are the first window's on every frame and only the target
                   changes: both are computed once."""
    loss = 0
    with ops.weights_frozen():
        code = prev = None
        for t in range(yy.shape[-1]):
            y = yy[..., t:t + 1]
            target = _target_slices(sequen_solver, x, y)
            if kind == "previous":
                if code is None:
                    code = sequen_solver.get_code(x, fx, y)
                    prev = sequen_solver.get_last_slice_weight(x, fx)
                    new_slice = model(prev, code)
                loss = loss + Fn.slice_mse(new_slice, target) / (new_slice.shape[0] * new_slice.shape[2])
                continue
            if kind == "learnslice":
                code = sequen_solver.get_code(x, fx, y)
                loss = loss + Fn.slice_mse(model.get_slice_weight(code, x, fx, use_vorticity=use_vorticity), target)
                used = target
            elif kind == "vorticity":
                used, code = _predict_slices(model, sequen_solver, x, fx)
                loss = loss + Fn.slice_mse(used, target) / (used.shape[0] * used.shape[2])
            else:
                raise ValueError(f"kind must be one of {SLICE_LEARNER_KINDS}; got {kind!r}")
            fx = torch.cat((fx[..., 1:], _decode_step(sequen_solver, used, code)), dim=-1)
    return loss


def fit_slice_learner(model, optimizer, scheduler, sequen_solver, pos, train, test, *, epochs, batch_size=1, kind=None,
                      fold_time=False, use_vorticity=None, max_grad_norm=None, epoch_orders=None, generator=None,
                      save_path=None, save_every=1, grad_sync=None, on_epoch=None):
    """The epoch loops of the reference's three slice trainers in LearnSlice.py, on the frozen `sequen_solver`.  `pos`
    [1, N, P]: the point input of every sample; `train` / `test`: data.ResidentDataset of (fx [n, N, Tin], yy [n, N, Tout])
    on the model's device.  `kind` "learnslice" | "vorticity" | "previous" picks the loop (default: by the model's class,
    `slice_learner_kind`); `use_vorticity` (learnslice only) defaults to the model's own flag.

    Each epoch: model.train(); shuffled batches through `learnslice_train_step` / `slice_predictor_train_step` /
    `previous_slice_train_step` with `fold_time`; model.eval(); `slice_learner_test_loss` on every test batch.  Returns one
    dict per epoch (train, test), each script's own figures with ITS divisors and quirks:
      learnslice  train = sum over batches of (sum of the Tout step losses / Tout) / len(train batches);
                  test = sum over test batches of (loss / Tout) / len(TRAIN batches): the script divides its test sum by
                  len(train_loader) (:587).  The scheduler steps once per frame, inside the step function.
      vorticity   train = the sum of the batch losses, undivided (:955-963); test = sum / len(test batches) (:1006).
      previous    train = the sum of the batch losses, undivided (:750-756); test = the sum, undivided (:791-793), of a test
                  pass whose window never slides.
    One host synchronisation per epoch.  The scripts save after every epoch: `save_every` = 1 does that (and `_fit` writes
    once more after the last epoch); `epoch_orders`, `generator`, `grad_sync`, `on_epoch`, `save_path` as fit_ns."""
    kind = slice_learner_kind(model) if kind is None else kind
    if kind not in SLICE_LEARNER_KINDS:
        raise ValueError(f"kind must be one of {SLICE_LEARNER_KINDS}; got {kind!r}")
    if use_vorticity is None:
        use_vorticity = getattr(model, "use_vorticity", 0)
    sequen_solver.eval()
    positions = _positions_cache(pos.to(_device_of(model)))
    ntrain_batches = -(-len(train) // batch_size)
    ntest_batches = -(-len(test) // batch_size)
    common = dict(max_grad_norm=max_grad_norm, grad_sync=grad_sync, fold_time=fold_time)

    def train_batch(batch, acc):
        fx, yy = batch
        x = positions(fx.shape[0])
        if kind == "learnslice":
            losses = learnslice_train_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, use_vorticity, **common)
            acc[0] += torch.stack(losses).sum() / yy.shape[-1]
        elif kind == "vorticity":
            acc[0] += slice_predictor_train_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, **common)
        else:
            acc[0] += previous_slice_train_step(model, optimizer, scheduler, sequen_solver, x, fx, yy, **common)

    def test_pass(acc):
        for fx, yy in test.batches(batch_size):
            loss = slice_learner_test_loss(kind, model, sequen_solver, positions(fx.shape[0]), fx, yy, use_vorticity)
            acc[1] += loss / yy.shape[-1] if kind == "learnslice" else loss

    def metrics(a):
        if kind == "learnslice":
            return dict(train=a[0] / ntrain_batches, test=a[1] / ntrain_batches)
        if kind == "vorticity":
            return dict(train=a[0], test=a[1] / ntest_batches)
        return dict(train=a[0], test=a[1])

    return _fit(model, epochs=epochs, n_acc=2, batches=lambda ep: _epoch_batches(train, batch_size, ep, epoch_orders, generator),
                train_batch=train_batch, test_pass=test_pass, metrics=metrics, on_epoch=on_epoch, save_path=save_path,
                save_every=save_every)


def evaluate_slice_learner(kind, model, sequen_solver, pos, test, use_vorticity=0, batch_size=1):
    """train(eval=True) of LearnSlice.py's three trainers on a loaded `model`, per test batch:
      learnslice           {'test_slice'}: sum of `slice_learner_test_loss` / Tout, / len(test) (it has no rollout of its own);
      vorticity, previous  {'test_full'}: sum of the full rel-L2 of the kind's prediction-feedback rollout
                           (`slice_predictor_rollout` / `previous_slice_rollout`), / len(test)."""
    if kind not in SLICE_LEARNER_KINDS:
        raise ValueError(f"kind must be one of {SLICE_LEARNER_KINDS}; got {kind!r}")
    positions = _positions_cache(pos.to(_device_of(model)))
    loss_fn = TestLoss(size_average=False)
    rollout = slice_predictor_rollout if kind == "vorticity" else previous_slice_rollout

    def test_pass(acc):
        for fx, yy in test.batches(batch_size):
            bsz, x = fx.shape[0], positions(fx.shape[0])
            if kind == "learnslice":
                acc[0] += slice_learner_test_loss(kind, model, sequen_solver, x, fx, yy, use_vorticity) / yy.shape[-1]
            else:
                acc[0] += loss_fn(rollout(model, sequen_solver, x, fx, yy.shape[-1]).reshape(bsz, -1), yy.reshape(bsz, -1))

    return _evaluate(model, 1, test_pass,
                     lambda a: {"test_slice" if kind == "learnslice" else "test_full": a[0] / len(test)})


# ------------------------------------------------------------------------------ velocity-field trainers
# ns_velocity.py, ns_velocity_unrolling.py, ns_unrolling2_with_t.py: the exp_ns / SOL-wrapper loops on PhiFlow velocity data,
# where one prediction is a (vel_x, vel_y) pair: out_dim = step = 2, so a step's target yy[..., t:t+step] is a
# two-dimensional strided view.  They are ONE family with exp_ns / ns_vorticity_unrolling and run the same functions:
# `_teacher_forced` (train_iteration, velocity_iteration), `_rollout_test_pass`, `_windowed_iteration` (the three
# unrolled_* iterations), `_fit_sol` (fit_unrolled, fit_velocity_unrolled, fit_unrolled_t), `_fit_teacher_forced` (fit_ns,
# fit_velocity), `_eager_iteration` and `_graphed_or_eager`.  The velocity loops pass fused=True, the older ones False:
#   * `_step_loss(fused=True)`: the per-call loss; with step > 1, fp32 GPU tensors and the p = 2 batch-sum `rel` it is
#     functional.rel_l2_window (the target read in place), otherwise `loss_fn` on the reshaped copies, as the scripts do;
#   * `scored_rollout` / `GraphedScoredRollout`: the prediction-feedback test pass with ONE launch after each model call
#     (window shift, prediction kept, step scored) and one after the last, no host synchronisation;
#   * `_ScopedCallStep`: a whole iteration (chained calls, windows, summed loss, backward, staged AdamW) in one hipGraph,
#     one per look-ahead value (the key of `_graphed_or_eager`).
def scored_rollout_supported(model, x, fx, yy, step, loss_fn=None):
    """True where `scored_rollout` serves the prediction-feedback test pass: the model on the GPU, fp32 tensors, a window of
    at most ops.WINDOW_MAX_F columns, 1 <= step <= ops.WINDOW_MAX_K dividing T, and (where given) the p = 2 batch-sum `rel`."""
    return ((loss_fn is None or _batch_sum_rel(loss_fn)) and _device_of(model).type == "cuda"
            and all(t.is_cuda and t.dtype == torch.float32 for t in (x, fx, yy)) and fx.dim() == 3 and yy.dim() == 3
            and 1 <= step <= min(ops.WINDOW_MAX_K, fx.shape[-1]) and fx.shape[-1] <= ops.WINDOW_MAX_F
            and yy.shape[-1] % step == 0 and yy.shape[-1] > 0)


def _scored_steps(model, x, win, yy, step, record, traj):
    """The T / step model calls of a scored rollout on the window `win` (shifted in place), each followed by one
    pa2d_rollout_tail launch; then the one pa2d_rollout_score launch."""
    for s in range(yy.shape[-1] // step):
        im = model(x, fx=win)
        if im.shape[-1] != step:
            raise ValueError(f"scored_rollout: the model predicts {im.shape[-1]} columns per call, step is {step}")
        ops.rollout_tail(im.contiguous(), win, traj, s * step, yy, s * step, record, s)
    return ops.rollout_score(record, win.shape[1])


@torch.no_grad()
def scored_rollout(model, x, fx, yy, step, keep_pred=False):
    """The prediction-feedback rollout of the test passes (ns_velocity.py:238-254) with its scores, on the GPU: T / step
    model calls under `ops.weights_frozen()`, each followed by ONE launch that shifts the input window, appends the
    prediction, keeps it (keep_pred) and adds the step's partial sums to a record; one more launch reduces the record.
    Returns (step_ratio [S, B], full_ratio [B], pred [B, N, T] or None), device tensors, no host synchronisation:
    step_ratio[s, b] = ||pred_s - y_s|| / ||y_s||, full_ratio[b] = the relative L2 of the whole predicted trajectory (the
    steps' columns partition it, so the concatenated prediction is not needed for it).  `fx` is left as it is."""
    if not scored_rollout_supported(model, x, fx, yy, step):
        raise ValueError("scored_rollout needs a model on the GPU, fp32 GPU tensors x, fx [B, N, F <= "
                         f"{ops.WINDOW_MAX_F}], yy [B, N, T] and 1 <= step <= {ops.WINDOW_MAX_K} dividing T")
    B, N, _ = fx.shape
    win = fx.clone(memory_format=torch.contiguous_format)
    record = ops.rollout_record(yy.shape[-1] // step, B, fx)
    traj = torch.empty(B, N, yy.shape[-1], dtype=torch.float32, device=fx.device) if keep_pred else None
    with ops.weights_frozen():
        step_ratio, full_ratio = _scored_steps(model, x, win, yy, step, record, traj)
    return step_ratio, full_ratio, traj


class GraphedScoredRollout(_RolloutGraph):
    """The WHOLE scored rollout (every model call, every tail launch and the score) in ONE hipGraph with static buffers
    (x, the initial window, the target, the window the steps shift, the record, the trajectory).  `run(x, fx, yy)` copies
    a batch in, refreshes the weight packs the captured launches point at (GraphedRollout's scheme, with its check that
    parameter storage has not moved) and replays once.  It returns `scored_rollout`'s triple, bit for bit (the same
    kernels in the same order on the same values); the tensors are the graph's own and hold until the next run."""

    def __init__(self, model, x, fx, yy, step, keep_pred=False, warmup=2, fused_tail=None):
        if not scored_rollout_supported(model, x, fx, yy, step):
            raise ValueError("GraphedScoredRollout: what scored_rollout needs")
        self.step = step
        self.x, self.fx, self.yy = x.clone(), fx.clone(memory_format=torch.contiguous_format), yy.clone()
        B, N, _ = fx.shape
        self.win = torch.empty_like(self.fx)
        self.record = ops.rollout_record(yy.shape[-1] // step, B, fx)
        self.traj = torch.empty(B, N, yy.shape[-1], dtype=torch.float32, device=fx.device) if keep_pred else None
        self.out = self._capture(model, self._body, warmup, fused_tail)

    def _body(self):
        self.win.copy_(self.fx)
        return _scored_steps(self.model, self.x, self.win, self.yy, self.step, self.record, self.traj)

    @torch.no_grad()
    def run(self, x, fx, yy):
        self._ready((self.x, self.fx, self.yy), (x, fx, yy))
        self.graph.replay()
        return self.out[0], self.out[1], self.traj


class _ScopedCallStep(GraphedCallStep):
    """GraphedCallStep for an iteration of SEVERAL model calls: zero-grad, the body and the backward sit in one
    `ops.weights_frozen()` scope inside the capture (each layer's weights are packed once per replay, as in
    GraphedTrainStep and in the eager iterations below); the staged optimizer step follows outside the scope."""

    def _iteration(self):
        with ops.weights_frozen():
            self.opt.zero_grad()
            parts = self.body(self.model, *self.static)
            parts[0].backward()
        self.opt.step_staged()
        return tuple(p.detach() for p in parts)


class StepCurriculum:
    """look_ahead += 1 whenever `ep % period == 0 and ep >= period and look_ahead <= max_look_ahead`
    (ns_velocity_unrolling.py:210-214 with period 40, ns_unrolling2_with_t.py:208-212 with period 10): the look-ahead can
    reach max_look_ahead + 1."""

    def __init__(self, period, look_ahead=1, max_look_ahead=4):
        self.period, self.look_ahead, self.max_look_ahead = period, look_ahead, max_look_ahead

    def update(self, ep):
        if ep % self.period == 0 and ep >= self.period and self.look_ahead <= self.max_look_ahead:
            self.look_ahead += 1
        return self.look_ahead


def velocity_iteration(model, x, fx, yy, step=2, loss_fn=None, calls=None):
    """Forward part of one ns_velocity.py:204-225 mini-batch (exp_ns's teacher-forced iteration with step columns per
    call).  Returns (loss [graph attached], full loss)."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    loss, preds = _teacher_forced(model, x, fx, yy, step, loss_fn, True, calls)
    return loss, _full_loss(loss_fn, preds, yy, calls)


def _velocity_runner(module, optimizer, scheduler, batch_size, graphed, max_grad_norm, grad_sync, calls, forward, nparts,
                     zero_grad_kw):
    """run(key, x, fx, yy) -> the `nparts` detached loss parts of one iteration `forward(key, x, fx, yy, calls)`.  Eager:
    the iteration as the scripts run it.  graphed: a full batch replays the `_ScopedCallStep` of `key` (the look-ahead),
    captured when the curriculum first reaches that key; the short last batch runs eagerly.  A replay's per-call loss
    values are copied to `calls` (the graph's own tensors are overwritten by the next replay)."""
    def build(x, fx, yy, key):
        def body(_, sx, sfx, syy):
            vals = []                        # a fresh list per run: the body runs in every warm-up and again in the capture
            return forward(key, sx, sfx, syy, vals) + tuple(vals)
        return _ScopedCallStep(module, optimizer, scheduler, (x.clone(), fx.clone(), yy.clone()), body)

    def replay(graph, x, fx, yy, key):
        out = graph(x, fx, yy)
        if calls is not None:
            calls.extend(v.clone() for v in out[nparts:])
        return out[:nparts]

    run = _graphed_or_eager(
        graphed, batch_size, build, replay,
        lambda x, fx, yy, key: _eager_iteration(module, optimizer, scheduler, lambda: forward(key, x, fx, yy, calls),
                                                max_grad_norm, grad_sync, zero_grad_kw))
    return lambda key, x, fx, yy: run(x, fx, yy, key=key)


def evaluate_velocity(model, test, batch_size, T=10, step=2, loss_fn=None, full=True, calls=None, graphed=False):
    """The test pass alone: {'test_step'} (and {'test_full'} with full) normalised like the loops' metrics."""
    loss_fn = loss_fn or TestLoss(size_average=False)
    graphs = {}
    m = _evaluate(model, 4, lambda acc: _rollout_test_pass(model, test, batch_size, T, step, loss_fn, acc, full, True, calls,
                                                           graphed, graphs),
                  lambda a: _ns_test_metrics(a, len(test), T / step))
    return m if full else dict(test_step=m["test_step"])


def _velocity_setup(who, module, optimizer, max_grad_norm, graphed):
    if graphed:
        _refuse_graphed_dropout(module, who)
        _graphed_refusals(who, optimizer, max_grad_norm)
        _capturable_model(module, who)


def fit_velocity(model, optimizer, scheduler, train, test, *, epochs, batch_size, T=10, step=2, max_grad_norm=None,
                 loss_fn=None, epoch_orders=None, generator=None, save_path=None, save_every=100, graphed=False,
                 grad_sync=None, on_epoch=None, calls=None):
    """The epoch loop of ns_velocity.main() (ns_velocity.py:192-273): exp_ns's loop on velocity data, `step` = 2 columns
    (vel_x, vel_y) per model call.  `train` / `test`: data.ResidentDataset of (x [n, N, 2], fx [n, N, T_in], yy [n, N, >= T])
    on the model's device (any device: a CPU module goes through the same loop).

    Per batch the teacher-forced iteration (T / step calls, summed loss, the loss of the whole trajectory, zero_grad,
    backward, [grad_sync], [clip], optimizer.step(), scheduler.step()); per epoch the prediction-feedback test pass
    (`scored_rollout` on the GPU).  Metrics, unrounded, as the script prints them: train_step = sum / ntrain / (T / step),
    train_full = sum / ntrain, test_step = sum / ntest / (T / step), test_full = sum / ntest.  One host synchronisation
    per epoch.  The whole model's state_dict is saved when ep % save_every == 0 and after the last epoch.
    `calls`: a list that receives every loss value (device tensors) in the script's call order.
    `graphed=True` (CUDA, optim.FusedAdamW, one rank, no dropout, clip inside the optimizer): full batches replay ONE
    hipGraph of the whole iteration with its optimizer step and the test pass one GraphedScoredRollout, bit for bit the
    eager results; the short last batch runs eagerly."""
    _velocity_setup("fit_velocity", model, optimizer, max_grad_norm, graphed)
    loss_fn = loss_fn or TestLoss(size_average=False)

    def forward(key, x, fx, yy, vals):
        return velocity_iteration(model, x, fx, yy, step, loss_fn, vals)
    run = _velocity_runner(model, optimizer, scheduler, batch_size, graphed, max_grad_norm, grad_sync, calls, forward, 2,
                           dict(set_to_none=False))
    return _fit_teacher_forced(model, train, test, lambda x, fx, yy: run(0, x, fx, yy), True, calls, graphed, epochs=epochs,
                               batch_size=batch_size, T=T, step=step, loss_fn=loss_fn, epoch_orders=epoch_orders,
                               generator=generator, save_path=save_path, save_every=save_every, on_epoch=on_epoch)


def _fit_sol(who, sol_model, optimizer, scheduler, train, test, curriculum, iteration, *, accumulate, fused, zero_grad_kw,
             epochs, batch_size, T, step, loss_fn, epoch_orders, generator, save_path, save_every, graphed, grad_sync, on_epoch,
             calls):
    """The epoch loop of the three SOL scripts (fit_unrolled, fit_velocity_unrolled, fit_unrolled_t): the curriculum stepped
    before an epoch's first batch, the per-look-ahead `iteration` (eager, or one graph per look-ahead value) with a step that
    never clips, the loss of a batch added to the epoch's (`accumulate`) or put in its place, the test pass on the INNER
    model with the step loss only (`fused`: on the scored rollout), the inner model saved."""
    _velocity_setup(who, sol_model, optimizer, None, graphed)
    loss_fn = loss_fn or TestLoss(size_average=False)
    ntest, ncalls = len(test), T / step
    inner = sol_model.transolver_model
    sol_model.n = curriculum.look_ahead

    def forward(la, x, fx, yy, vals):
        return (iteration(sol_model, x, fx, yy, la, step, loss_fn, vals),)
    run = _velocity_runner(sol_model, optimizer, scheduler, batch_size, graphed, None, grad_sync, calls, forward, 1,
                           zero_grad_kw)
    graphs = {}

    def batches(ep):
        sol_model.n = curriculum.update(ep)      # before the epoch's first batch; it then holds for the epoch
        return _epoch_batches(train, batch_size, ep, epoch_orders, generator)

    def train_batch(batch, acc):
        x, fx, yy = batch
        (loss,) = run(curriculum.look_ahead, x, fx, yy[..., :T])
        if accumulate:
            acc[0] += loss
        else:
            acc[0] = loss

    return _fit(sol_model, epochs=epochs, n_acc=4, batches=batches, train_batch=train_batch,
                test_pass=lambda acc: _rollout_test_pass(inner, test, batch_size, T, step, loss_fn, acc, False, fused, calls,
                                                         graphed, graphs),
                metrics=lambda a: dict(train_step=a[0], test_step=_ns_test_metrics(a, ntest, ncalls)["test_step"],
                                       look_ahead=curriculum.look_ahead),
                on_epoch=on_epoch, save_path=save_path, save_every=save_every, save_module=inner)


def fit_velocity_unrolled(sol_model, optimizer, scheduler, train, test, *, epochs, batch_size, T=20, step=2, look_ahead=1,
                          max_look_ahead=8, period=40, loss_fn=None, epoch_orders=None, generator=None, save_path=None,
                          save_every=100, graphed=False, grad_sync=None, on_epoch=None, calls=None):
    """The epoch loop of ns_velocity_unrolling.main() (ns_velocity_unrolling.py:202-313) on the SOL wrapper.  Per batch ONE
    window: `look_ahead` chained calls scored against yy[..., offset - step:offset], zero_grad, backward, [grad_sync],
    step, scheduler.step(); it never clips.  look_ahead += 1 when ep % period == 0 and ep >= period and look_ahead <=
    max_look_ahead (`StepCurriculum`; the defaults are the script's module constants).  The test pass runs the inner
    `transolver_model` with prediction feedback and keeps the step loss.

    Returns one dict per epoch: test_step = sum / ntest / (T / step), as printed; train_step = the loss of the epoch's
    LAST batch (the script assigns, it does not add, and never prints it), kept on the device and read with the epoch's one
    synchronisation (the script's per-batch `loss.item()` is gone); look_ahead.  Saves the inner model's state_dict.
    `calls`, `graphed`: as fit_velocity, with one graph per look-ahead value, built when the curriculum first reaches it."""
    return _fit_sol("fit_velocity_unrolled", sol_model, optimizer, scheduler, train, test,
                    StepCurriculum(period, look_ahead, max_look_ahead), unrolled_window_iteration, accumulate=False,
                    fused=True, zero_grad_kw=dict(set_to_none=False), epochs=epochs, batch_size=batch_size, T=T, step=step,
                    loss_fn=loss_fn, epoch_orders=epoch_orders, generator=generator, save_path=save_path,
                    save_every=save_every, graphed=graphed, grad_sync=grad_sync, on_epoch=on_epoch, calls=calls)


def fit_unrolled_t(sol_model, optimizer, scheduler, train, test, *, epochs, batch_size, T=10, step=2, look_ahead=1,
                   max_look_ahead=4, period=10, loss_fn=None, epoch_orders=None, generator=None, save_path=None,
                   save_every=100, graphed=False, grad_sync=None, on_epoch=None, calls=None):
    """The epoch loop of ns_unrolling2_with_t.main() (ns_unrolling2_with_t.py:200-313) on the SOL wrapper: per batch every
    window t in range(0, T - offset + step, step), `look_ahead` chained calls scored against yy[..., t + offset - step:
    t + offset], the window then advanced by `step` ground-truth columns; one backward over the summed loss.  look_ahead
    += 1 when ep % period == 0 and ep >= period and look_ahead <= max_look_ahead.

    Returns one dict per epoch: train_step = the RAW epoch sum (what the script prints), test_step = sum / ntest /
    (T / step), look_ahead.  Everything else as fit_velocity_unrolled."""
    return _fit_sol("fit_unrolled_t", sol_model, optimizer, scheduler, train, test,
                    StepCurriculum(period, look_ahead, max_look_ahead), unrolled_t_iteration, accumulate=True,
                    fused=True, zero_grad_kw=dict(set_to_none=False), epochs=epochs, batch_size=batch_size, T=T, step=step,
                    loss_fn=loss_fn, epoch_orders=epoch_orders, generator=generator, save_path=save_path,
                    save_every=save_every, graphed=graphed, grad_sync=grad_sync, on_epoch=on_epoch, calls=calls)
