"""The slice-learner trainers on the MI355X: `SequenSolver.code_windows`, the four steps (LearnSlice, SliceLearner,
VorticitySliceLearner, PreviousSliceLearner) eager and folded, `previous_slice_rollout` and `fit_slice_learner`.

Tiny models (6 x 5 mesh, M = 8, C = 16, T = 2, layers = 2, the encoder of test_gpu_sequensolver.py) at B = 2 with n = 3 output
frames are held to the float64 restatement of the EAGER loops (tests/previous_slice_restatement.py) with plain SGD on both
sides.  What is compared: every loss, and every trained tensor's UPDATE (after - before; the parameters themselves would
hide a wrong gradient behind the unchanged initial values).  Bounds, the rule of test_gpu_sequence_drivers.py:
max(4 x own, base), `own` the float32 CPU restatement's deviation from float64, base 1e-5 for losses and 1e-4 for
parameters.  The eager and the folded step run in the same test under the same bounds.  Every figure is printed before it
is asserted; the worst measured ones are in DESIGN 4.18."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_l2
import previous_slice_restatement as R
import slicepredictor_restatement as RS
import test_gpu_sequensolver as TP

pytestmark = pytest.mark.gpu
GEOM = dict(T=2, W=5, H=6, M=8, C=16)
B, NOUT, LAYERS, LR = 2, 3, 2, 0.1
KINDS = ["learnslice", "conv", "vorticity", "previous"]
BASE = {"loss": 1e-5, "param": 1e-4}
UNREAD = ("param.placeholder",)                    # SliceLearner reads its placeholder only without fx
WP_LAST = "weight_projection.linear_post"          # its bias shifts all M logits of a softmax alike: true gradient 0


def _solver(seed=71):
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    torch.manual_seed(seed)
    m = SequenSolver(None, B=B, layers=LAYERS, encoder_config=TP.TINY_ENCODER, **GEOM)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(".bias") or k.startswith("ln_"):
                p.add_(0.1 * torch.randn_like(p))
    for p in m.parameters():
        p.requires_grad = False
    return m.eval()


def _learner(kind, seed=72):
    """(module on the CPU with seeded weights, harness kind)."""
    from transformerbasednavierstokesolver_amd import LearnSlice as LS, SliceLearner as SL
    M, C, T, H, W = GEOM["M"], GEOM["C"], GEOM["T"], GEOM["H"], GEOM["W"]
    torch.manual_seed(seed)
    if kind == "learnslice":
        m = LS.LearnSlice(unified_pos=0, use_vorticity=1, C=C, M=M, T=T)
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.add_(0.1 * torch.randn_like(p))
            m.weight_projection.linear_post.weight.mul_(4.0)
        return m
    if kind == "conv":
        m, shapes = SL.SliceLearner(space_dim=2, n_hidden=32, fun_dim=T, H=H, W=W, slice_num=M), \
            RS.slice_learner_shapes(space_dim=2, n_hidden=32, fun_dim=T, slice_num=M)
    elif kind == "vorticity":
        m, shapes = SL.VorticitySliceLearner(0, True, C=C, M=M, T=T, H=H, W=W, n_hidden=32), RS.vorticity_shapes(0, True, C, M, T, 32)
    else:
        m, shapes = SL.PreviousSliceLearner(C=C, M=M), R.previous_slice_shapes(C, M)
    sd = RS.draw_state(shapes, seed, 0.5)
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m


def _data(seed=73, nout=NOUT):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, GEOM["H"] * GEOM["W"], 2, generator=g)
    seq = torch.randn(B, GEOM["H"] * GEOM["W"], GEOM["T"] + nout, generator=g)
    seq[1] = 3.0 * seq[1] + 0.5             # the two samples of a call differ in scale: per-call statistics matter
    return x, seq[..., :GEOM["T"]].contiguous(), seq[..., GEOM["T"]:].contiguous()


def _restated(kind, dtype):
    """(losses, {tensor: update}) of one batch of the restated eager loop in `dtype`."""
    solver, learner = _solver(), _learner(kind)
    x, fx, yy = (t.to(dtype) for t in _data())
    ssd = {k: v.detach().to(dtype) for k, v in solver.state_dict().items()}
    sd0 = {k: v.detach().to(dtype).clone() for k, v in learner.state_dict().items()}
    trainable = {k for k, _ in learner.named_parameters()}
    sd = {k: v.clone().requires_grad_(k in trainable) for k, v in sd0.items()}
    losses = R.train_step(kind, sd, R.Frozen(ssd, TP.TINY_ENCODER, LAYERS), x, fx, yy, GEOM, LR)
    return _pack(losses, {k: sd[k].detach() - sd0[k] for k in trainable})


def _pack(losses, delta):
    out = {"loss": torch.stack([torch.as_tensor(v).double().cpu() for v in losses])}
    if WP_LAST + ".bias" in delta:          # rounding only: judged with its layer's weight, as one tensor
        delta[WP_LAST + ".[weight|bias]"] = torch.cat((delta[WP_LAST + ".weight"].reshape(-1), delta.pop(WP_LAST + ".bias").reshape(-1)))
    out.update({"param." + k: v.double().cpu() for k, v in delta.items()})
    return out


def _step(kind, learner, solver, opt, x, fx, yy, **kw):
    from transformerbasednavierstokesolver_amd import harness
    if kind == "learnslice":
        return harness.learnslice_train_step(learner, opt, None, solver, x, fx, yy, 1, **kw)
    if kind == "previous":
        return [harness.previous_slice_train_step(learner, opt, None, solver, x, fx, yy, **kw)]
    return [harness.slice_predictor_train_step(learner, opt, None, solver, x, fx, yy, **kw)]


def _device(kind, fold, engine="f32"):
    solver, learner = _solver().cuda().set_engine(engine), _learner(kind).cuda().train()
    if hasattr(learner, "set_engine"):
        learner.set_engine(engine)
    x, fx, yy = (t.cuda() for t in _data())
    before = {k: p.detach().clone() for k, p in learner.named_parameters()}
    opt = torch.optim.SGD(learner.parameters(), lr=LR)
    losses = _step(kind, learner, solver, opt, x, fx, yy, fold_time=fold)
    return _pack(losses, {k: p.detach() - before[k] for k, p in learner.named_parameters()})


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = (_restated(kind, torch.float64), _restated(kind, torch.float32))
        return cache[kind]
    return get


def _judge(got, r64, r32, label):
    assert sorted(got) == sorted(r64), (label, sorted(got), sorted(r64))
    worst = {"loss": 0.0, "param": 0.0}
    for k, want in r64.items():
        fam = "loss" if k == "loss" else "param"
        if float(want.abs().max()) == 0:        # a tensor the loop never reads (SliceLearner's placeholder with fx given)
            assert k in UNREAD and float(got[k].abs().max()) == 0, (label, k, "moved on the device only")
            continue
        own, err = rel_l2(r32[k], want), rel_l2(got[k], want)
        bound = max(4 * own, BASE[fam])
        worst[fam] = max(worst[fam], err)
        print(f"{label} {k}: rel-L2 {err:.3g}, own float32 {own:.3g}, bound {bound:.3g}")
        assert err <= bound, (label, k, err, bound)
    print(f"{label}: worst loss error {worst['loss']:.3g}, worst update error {worst['param']:.3g}")


@pytest.mark.parametrize("kind", KINDS)
def test_steps_eager_and_folded_against_the_restated_loop(kind, restated):
    r64, r32 = restated(kind)
    assert r64["loss"].numel() == (NOUT if kind == "learnslice" else 1)
    for fold in (False, True):
        _judge(_device(kind, fold), r64, r32, f"{kind} step fold_time={fold}")


def test_code_windows_against_the_per_call_functions():
    """codes[k] = get_code on window k; frame f of the slice table = what encoder.encode leaves cached for that frame (the
    target of call f - T, and get_last_slice_weight of call f - T + 1); the cached slice weights afterwards are the eager
    loop's (the last window's last frame); `code` and `slice_weights` are not touched.  Both sides are the same float32
    kernels on different batch compositions: 1e-5 rel-L2, the figure of test_gpu_sequence_fold.py."""
    solver = _solver().cuda()
    x, fx, yy = (t.cuda() for t in _data())
    T, seq = GEOM["T"], torch.cat((fx, yy), -1)
    solver.code, marker = None, solver.slice_weights.clone()
    codes, slices = solver.code_windows(x, seq)
    assert tuple(codes.shape) == (NOUT, B, 1, GEOM["M"], GEOM["C"]) and tuple(slices.shape) == ((T + NOUT) * B, 1, 30, GEOM["M"])
    assert not codes.requires_grad and not slices.requires_grad
    assert solver.code is None and torch.equal(solver.slice_weights, marker)
    cached = solver.encoder.get_attention_slice().clone()
    with torch.no_grad():
        for k in range(NOUT):
            win = seq[..., k:k + T]
            solver.encoder.encode(x, seq[..., T + k:T + k + 1])
            target = solver.encoder.get_attention_slice().clone()
            code = solver.get_code(x, win, None)
            prev = solver.get_last_slice_weight(x, win).clone()
            errs = (rel_l2(codes[k], code), rel_l2(slices[(T + k) * B:(T + k + 1) * B], target),
                    rel_l2(slices[(T + k - 1) * B:(T + k) * B], prev))
            print(f"code_windows call {k}: code {errs[0]:.3g}, target {errs[1]:.3g}, previous slice {errs[2]:.3g}")
            assert max(errs) <= 1e-5, (k, errs)
        assert cached.shape == prev.shape and rel_l2(cached, solver.encoder.get_attention_slice()) <= 1e-5
    with pytest.raises(ValueError, match="n >= 1"):
        solver.code_windows(x, fx)


@pytest.mark.parametrize("kind", ["vorticity", "previous"])
def test_a_cut_fold_gives_what_one_folded_call_gives(monkeypatch, kind):
    """n = 3 calls cut into folds of 2 + 1, in the frozen model's blocks and in the predictor, against one fold."""
    from transformerbasednavierstokesolver_amd import SequenSolver as S, harness
    whole = _device(kind, True)
    seen = []
    monkeypatch.setattr(S, "fold_calls", lambda n, *a: seen.append(("blocks", n)) or 2)
    monkeypatch.setattr(harness, "_slice_fold_group", lambda model, n, *a: seen.append(("predictor", n)) or 2)
    cut = _device(kind, True)
    assert seen == [("blocks", NOUT), ("predictor", NOUT)]
    assert sorted(cut) == sorted(whole)
    for k in whole:
        err = rel_l2(cut[k], whole[k])
        print(f"{kind} cut fold {k}: rel-L2 {err:.3g}")
        assert err <= BASE["loss" if k == "loss" else "param"], (k, err)


def test_previous_slice_rollout_against_the_restated_loop():
    from transformerbasednavierstokesolver_amd import harness
    solver, learner = _solver(), _learner("previous")
    x, fx, _ = _data()

    def restated_rollout(dtype):
        ssd = {k: v.detach().to(dtype) for k, v in solver.state_dict().items()}
        sd = {k: v.detach().to(dtype) for k, v in learner.state_dict().items()}
        return R.previous_rollout(sd, R.Frozen(ssd, TP.TINY_ENCODER, LAYERS), x.to(dtype), fx.to(dtype), 3)

    r64, r32 = restated_rollout(torch.float64), restated_rollout(torch.float32)
    solver, learner = solver.cuda().set_engine("f32"), learner.cuda().set_engine("f32").eval()
    before = fx.clone()
    got = harness.previous_slice_rollout(learner, solver, x.cuda(), fx.cuda(), 3)
    assert tuple(got.shape) == (B, 30, 3) and torch.equal(fx, before)
    own, err = rel_l2(r32, r64), rel_l2(got, r64)
    print(f"previous_slice_rollout 3 steps: rel-L2 {err:.3g}, own float32 {own:.3g}")
    assert err <= max(4 * own, 1e-5)
    assert not torch.equal(got[..., 0], got[..., 1])                     # the prediction entered the window
    # the last step's raw prediction is what the sequence model decodes with
    left, last = solver.slice_weights.clone(), _window(fx.cuda(), got, 2)
    with torch.no_grad():
        again = learner(solver.get_last_slice_weight(x.cuda(), last), solver.get_code(x.cuda(), last, None))
    assert left.shape == again.shape and rel_l2(left, again) <= 1e-6


def _window(fx, preds, k):
    """The window of rollout step k: the last T columns of cat(fx, preds[..., :k])."""
    return torch.cat((fx, preds[..., :k]), -1)[..., -fx.shape[-1]:].contiguous()


@pytest.mark.parametrize("kind", ["learnslice", "vorticity", "previous"])
def test_fit_slice_learner_is_the_hand_written_loop(kind):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.data import ResidentDataset
    ntrain, ntest, epochs = 3, 2, 2
    g = torch.Generator().manual_seed(91)
    pos = torch.rand(1, 30, 2, generator=g).cuda()
    a = torch.randn(ntrain + ntest, 30, GEOM["T"], generator=g).cuda()
    u = torch.randn(ntrain + ntest, 30, 2, generator=g).cuda()
    orders = [[2, 0, 1], [1, 2, 0]]
    solver = _solver().cuda()
    base = _learner(kind).cuda()
    steps = ntrain * (2 if kind == "learnslice" else 1)

    def make():
        m = copy.deepcopy(base)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        return m, opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, epochs=epochs, steps_per_epoch=steps)

    m1, opt1, sched1 = make()
    hist = harness.fit_slice_learner(m1, opt1, sched1, solver, pos, ResidentDataset(a[:ntrain], u[:ntrain]),
                                     ResidentDataset(a[ntrain:], u[ntrain:]), epochs=epochs, epoch_orders=orders, kind=kind)
    assert harness.slice_learner_kind(m1) == kind
    m2, opt2, sched2 = make()
    for ep in range(epochs):
        m2.train()
        acc = torch.zeros(2, dtype=torch.float64, device="cuda")
        for i in orders[ep]:
            fx, yy = a[i:i + 1], u[i:i + 1]
            if kind == "learnslice":
                acc[0] += torch.stack(harness.learnslice_train_step(m2, opt2, sched2, solver, pos, fx, yy, 1)).sum() / 2
            elif kind == "vorticity":
                acc[0] += harness.slice_predictor_train_step(m2, opt2, sched2, solver, pos, fx, yy)
            else:
                acc[0] += harness.previous_slice_train_step(m2, opt2, sched2, solver, pos, fx, yy)
        m2.eval()
        for i in range(ntrain, ntrain + ntest):
            loss = harness.slice_learner_test_loss(kind, m2, solver, pos, a[i:i + 1], u[i:i + 1], 1)
            acc[1] += loss / 2 if kind == "learnslice" else loss
        s = acc.tolist()
        want = {"learnslice": dict(train=s[0] / ntrain, test=s[1] / ntrain),          # the script's own divisor: train batches
                "vorticity": dict(train=s[0], test=s[1] / ntest), "previous": dict(train=s[0], test=s[1])}[kind]
        assert hist[ep] == want, (ep, hist[ep], want)
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k
    # the previous loop's test pass never slides its window: the terms differ in the target only
    if kind == "previous":
        with torch.no_grad():
            fx, yy = a[ntrain:ntrain + 1], u[ntrain:ntrain + 1]
            out = m2(solver.get_last_slice_weight(pos, fx), solver.get_code(pos, fx, None))
            want = 0
            for t in range(2):
                solver.encoder.encode(pos, yy[..., t:t + 1])
                want = want + torch.nn.functional.mse_loss(out, solver.encoder.get_attention_slice())
        got = harness.slice_learner_test_loss(kind, m2, solver, pos, fx, yy)
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    # the folded loop runs the same epochs within the loss bound
    m3, opt3, sched3 = make()
    folded = harness.fit_slice_learner(m3, opt3, sched3, solver, pos, ResidentDataset(a[:ntrain], u[:ntrain]),
                                       ResidentDataset(a[ntrain:], u[ntrain:]), epochs=epochs, epoch_orders=orders, fold_time=True)
    for ep in range(epochs):
        for k, v in hist[ep].items():
            print(f"{kind} epoch {ep} {k}: eager {v:.9g}, folded {folded[ep][k]:.9g}")
            assert abs(folded[ep][k] - v) <= 2e-5 * abs(v), (ep, k)


def _parent_learnslice_step(model, optimizer, solver, x, fx, yy, use_vorticity):
    """harness.learnslice_train_step as it stood before `fold_time` existed."""
    from transformerbasednavierstokesolver_amd import functional as Fn, harness, ops
    losses = []
    with ops.weights_frozen():
        for t in range(yy.shape[-1]):
            y = yy[..., t:t + 1]
            with torch.no_grad():
                solver.encoder.encode(x, y)
                target = solver.encoder.get_attention_slice()
                code = solver.get_code(x, fx, y)
            loss = Fn.slice_mse(model.get_slice_weight(code, x, fx, use_vorticity=use_vorticity), target)
            optimizer.zero_grad()
            loss.backward()
            harness._apply_step(optimizer, None, (p for p in model.parameters() if p.requires_grad), None, None)
            losses.append(loss.detach())
            fx = torch.cat((fx[..., 1:], y), dim=-1)
    return losses


def _parent_predictor_step(model, optimizer, solver, x, fx, yy):
    """harness.slice_predictor_train_step as it stood before `fold_time` existed."""
    from transformerbasednavierstokesolver_amd import functional as Fn, harness, ops
    loss = 0
    with ops.weights_frozen():
        for t in range(yy.shape[-1]):
            y = yy[..., t:t + 1]
            with torch.no_grad():
                solver.encoder.encode(x, y)
                target = solver.encoder.get_attention_slice()
            pred, _ = harness._predict_slices(model, solver, x, fx)
            loss = loss + Fn.slice_mse(pred, target) / (pred.shape[0] * pred.shape[2])
            fx = torch.cat((fx[..., 1:], y), dim=-1)
        optimizer.zero_grad()
        loss.backward()
    harness._apply_step(optimizer, None, (p for p in model.parameters() if p.requires_grad), None, None)
    return [loss.detach()]


@pytest.mark.parametrize("kind", ["learnslice", "conv", "vorticity"])
def test_the_default_path_is_the_eager_loop_bit_for_bit(kind):
    """Called without the new keyword (and with fold_time=False) the existing steps give the bits of the loop they held
    before it; VorticitySliceLearner.forward is forward_folded with one group."""
    solver = _solver().cuda()
    x, fx, yy = (t.cuda() for t in _data())
    runs = []
    for how in ("parent", "default", "false"):
        learner = _learner(kind).cuda().train()
        opt = torch.optim.SGD(learner.parameters(), lr=LR)
        if how == "parent":
            losses = _parent_learnslice_step(learner, opt, solver, x, fx, yy, 1) if kind == "learnslice" else \
                _parent_predictor_step(learner, opt, solver, x, fx, yy)
        else:
            losses = _step(kind, learner, solver, opt, x, fx, yy, **({} if how == "default" else {"fold_time": False}))
        runs.append((torch.stack(list(losses)), [p.detach().clone() for p in learner.parameters()]))
    for losses, params in runs[1:]:
        assert torch.equal(losses, runs[0][0])
        assert all(torch.equal(p, q) for p, q in zip(params, runs[0][1]))
    if kind == "vorticity":
        learner = _learner(kind).cuda().eval()
        code = torch.randn(B, 1, GEOM["M"], GEOM["C"], device="cuda")
        with torch.no_grad():
            assert torch.equal(learner(x, fx, code), learner.forward_folded(x, fx, code, groups=1))


def test_previous_slice_learner_meets_the_fixture_on_the_gpu():
    """PreviousSliceLearner at the reference's shape against the reference's own float64 forward_previous_slice
    (tests/golden/G23_previous_slice.npz): max(4 x the fixture's own float32 deviation, 1e-6 relative), fused entry and
    three-op route."""
    import os
    from conftest import GOLDEN
    from transformerbasednavierstokesolver_amd.SliceLearner import PreviousSliceLearner
    g = np.load(os.path.join(GOLDEN, "G23_previous_slice.npz"))
    sd, prev, token, target = R.draw_g23()
    m = PreviousSliceLearner(C=R.G23_SHAPE["C"], M=R.G23_SHAPE["M"])
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m = m.cuda().set_engine("f32")
    stride, want = int(g["point_stride"]), torch.from_numpy(g["out.f64"])
    bound = max(4 * float(g["fp32_self_error.out"]), 1e-6)
    for fused in (True, False):
        m.fused_entry = fused
        for p in m.parameters():
            p.grad = None
        out = m(torch.from_numpy(prev).cuda(), torch.from_numpy(token).cuda())
        err = rel_l2(out.detach()[0, 0, ::stride], want)
        print(f"G23 forward fused={fused}: rel-L2 {err:.3g}, bound {bound:.3g}")
        assert err <= bound
        assert abs(float(out.detach().double().norm()) - float(g["out.norm"])) <= bound * float(g["out.norm"])
        loss = torch.nn.functional.mse_loss(out, torch.from_numpy(target).cuda())
        loss.backward()
        lb = max(4 * float(g["fp32_self_error.loss"]), 1e-6)
        assert abs(float(loss.detach()) - float(g["loss.f64"])) <= lb * abs(float(g["loss.f64"])), (float(loss.detach()), float(g["loss.f64"]))
        grads = {k: p.grad for k, p in m.named_parameters()}
        for k in [str(s) for s in g["whole_keys"]]:
            e, b = rel_l2(grads[k], torch.from_numpy(g["grad." + k])), max(4 * float(g["fp32_self_error.grad." + k]), 1e-6)
            print(f"G23 grad {k} fused={fused}: rel-L2 {e:.3g}, bound {b:.3g}")
            assert e <= b, (k, e, b)
        for k in [str(s) for s in g["row_keys"]]:
            rows = grads[k][::int(g["row_stride"])]
            e, b = rel_l2(rows, torch.from_numpy(g["grad." + k])), max(4 * float(g["fp32_self_error.grad." + k]), 1e-6)
            print(f"G23 grad rows {k} fused={fused}: rel-L2 {e:.3g}, bound {b:.3g}")
            assert e <= b, (k, e, b)
            n = float(g["grad." + k + ".norm"])
            assert abs(float(grads[k].double().norm()) - n) <= b * n, k
