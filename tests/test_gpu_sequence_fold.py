"""The time-folded teacher-forced iteration of the latent-sequence models on the MI355X: `forward_windows` of both
SequenSolver classes and `harness.sequensolver_train_step(fold_time=True)`.

Tiny models are held to the float64 restatement of the EAGER loop (one restated call per window; tests/
sequensolver_merged_restatement.py, tests/sequensolver_restatement.py) under the rule of test_gpu_sequensolver*.py: bound =
4 x own if own > base / 4 else base, `own` the float32 CPU restatement's rel-L2 to float64 and `base` the acceptance table of
test_gpu_sequensolver._acceptance.  The eager step runs in the same test under the same bounds, so a fold that is merely
close to eager cannot hide an eager error.  B = 2 with n = 3 windows puts the z-score group boundaries inside the folded
batch of six samples.  Then the reference's recorded training losses (G13, G10) with the folded step, the freeze, the epoch
loop against a hand-written loop, and the unchanged groups = 1 path of the slice predictor."""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import rel_l2
import sequensolver_merged_restatement as RM
import sequensolver_restatement as RP
import test_gpu_sequensolver as TP
import test_gpu_sequensolver_merged as TM
from test_gpu_sequensolver import LAST, _acceptance, _bound
from test_sequensolver_merged_host import TINY_ENCODER as MERGED_ENCODER

pytestmark = pytest.mark.gpu
ENGINES = [None, "f32"]


def _spread(m, last):
    with torch.no_grad():      # spread the predicted slice weights, and give every parameter a non-trivial value
        for k, p in m.named_parameters():
            if k.endswith(".bias") or k.startswith("ln_"):
                p.add_(0.1 * torch.randn_like(p))
        last.weight.mul_(4.0)


def _restated_loop(sd, dtype, x, seq, T, call, plain):
    """The eager loop, restated: one call per window of true frames, the rel-L2 terms summed, one backward."""
    sd = {k: v.to(dtype).clone().requires_grad_(not k.startswith("encoder.")) for k, v in sd.items()}
    loss, outs = 0, []
    for k in range(seq.shape[-1] - T):
        y = seq[..., k + T:k + T + 1].to(dtype)
        out = call(sd, x.to(dtype), seq[..., k:k + T].to(dtype), y)
        loss = loss + RM.rel_l2_loss(out, y)
        outs.append(out)
    loss.backward()
    res = {"out": torch.cat(outs, -1).detach(), "loss": loss.detach()}
    skip = LAST + ".bias" if plain else None      # true gradient 0: judged with its layer's weight, as one tensor
    res.update({"grad." + k: v.grad for k, v in sd.items() if v.grad is not None and k != skip})
    if plain and sd[LAST + ".weight"].grad is not None:
        res[f"grad.{LAST}.[weight|bias]"] = torch.cat((sd[LAST + ".weight"].grad.reshape(-1), sd[LAST + ".bias"].grad.reshape(-1)))
    return res


def _device_step(m, x, seq, T, use_gt, fold, plain):
    """One sequensolver_train_step at lr = 0 (the gradients stay in .grad), and the per-window outputs of the same route."""
    from transformerbasednavierstokesolver_amd import harness
    for p in m.parameters():
        p.grad = None
    fx, yy = seq[..., :T].contiguous(), seq[..., T:].contiguous()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.0)
    loss, full = harness.sequensolver_train_step(m, opt, None, x, fx, yy, use_gt=use_gt, fold_time=fold)
    skip = LAST + ".bias" if plain else None
    got = {"loss": loss}
    got.update({"grad." + k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None and k != skip})
    if plain and m.weight_projection.linear_post.weight.grad is not None:
        wp = m.weight_projection.linear_post
        got[f"grad.{LAST}.[weight|bias]"] = torch.cat((wp.weight.grad.reshape(-1), wp.bias.grad.reshape(-1)))
    with torch.no_grad():
        if fold:
            got["out"] = m.forward_windows(x, seq, use_gt=use_gt)
        else:
            got["out"] = torch.cat([m(x, seq[..., k:k + T], seq[..., k + T:k + T + 1], use_gt=use_gt)
                                    for k in range(seq.shape[-1] - T)], -1)
        last = m(x, seq[..., -T - 1:-1], seq[..., -1:], use_gt=use_gt)
        state = (m.code.clone(), m.slice_weights.clone(), m.encoder.get_attention_slice().clone())
    return got, full, last, state


def _judge(got, r64, r32, label):
    assert sorted(got) == sorted(r64), label
    for k, want in r64.items():
        base, own = _acceptance("." + k), rel_l2(r32[k], want)
        bound = 4 * own if own > base / 4 else base
        err = rel_l2(got[k], want)
        print(f"{label} {k}: rel-L2 {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (label, k, err, bound)


def _fold_and_eager(m, x, seq, T, use_gt, plain, r64, r32, label):
    x, seq = x.cuda(), seq.cuda()
    eager, full_e, _, _ = _device_step(m, x, seq, T, use_gt, False, plain)
    _judge(eager, r64, r32, label + " eager")
    fold, full_f, last, state = _device_step(m, x, seq, T, use_gt, True, plain)
    _judge(fold, r64, r32, label + " folded")
    assert tuple(fold["out"].shape) == (seq.shape[0], seq.shape[1], seq.shape[-1] - T)
    assert rel_l2(full_f, full_e) <= 2e-5
    # after forward_windows the model holds what the eager loop's last call leaves
    m.forward_windows(x, seq, use_gt=use_gt)
    for name, a, b in zip(("code", "slice_weights", "cached slice weights"),
                          (m.code, m.slice_weights, m.encoder.get_attention_slice()), state):
        assert a.shape == b.shape and rel_l2(a.detach(), b) <= 1e-5, (label, name)


@pytest.mark.parametrize("engine", ENGINES)
def test_merged_tiny_model_folded_and_eager_against_the_restated_loop(engine):
    """TINY_ENCODER, 8 x 8 mesh, M=8, C=16, sequential_head=8, T=3, layers=2, B=2, n=3."""
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    torch.manual_seed(17)
    T, n = 3, 3
    m = SequenSolver(None, T=T, W=8, H=8, M=8, C=16, B=2, sequential_head=8, layers=2, encoder_config=MERGED_ENCODER)
    _spread(m, m.in_project_slice.linear_post)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(18)
    x = torch.from_numpy(RM.unified_positions(8, 8)).repeat(2, 1, 1)
    seq = torch.randn(2, 64, T + n, generator=g)
    seq[1] = 3.0 * seq[1] + 0.5          # the two samples of a call differ in scale: per-call statistics matter
    call = lambda s, xx, fx, y: RM.forward(s, MERGED_ENCODER, 2, 8, xx, fx, y)[0]
    r64 = _restated_loop(sd, torch.float64, x, seq, T, call, plain=False)
    r32 = _restated_loop(sd, torch.float32, x, seq, T, call, plain=False)
    m = m.cuda().set_engine(engine).train()
    _fold_and_eager(m, x, seq, T, False, False, r64, r32, f"merged tiny engine={engine}")
    # a fold that z-scored over all six samples would not be this model: the whole-batch statistics give another output
    with torch.no_grad():
        xs, sq = x.cuda(), seq.cuda()
        good = m.forward_windows(xs, sq, use_gt=False)
        real = m.forward_slice
        m.forward_slice = lambda a, b, c, groups=1: real(a, b, c, groups=1)
        bad = m.forward_windows(xs, sq, use_gt=False)
        m.forward_slice = real
    assert rel_l2(bad, good) > 1e-4


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("use_gt", [True, False])
def test_plain_tiny_model_folded_and_eager_against_the_restated_loop(use_gt, engine):
    """The tiny configuration of test_gpu_sequensolver.py (6 x 5 mesh, C=16, M=8, T=2, B=3, layers=2), n = 3."""
    from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
    torch.manual_seed(27)
    T, n = 2, 3
    m = SequenSolver(None, T=T, W=5, H=6, M=8, C=16, B=3, layers=2, encoder_config=TP.TINY_ENCODER)
    _spread(m, m.weight_projection.linear_post)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(28)
    x, seq = torch.rand(3, 30, 2, generator=g), torch.randn(3, 30, T + n, generator=g)
    call = lambda s, xx, fx, y: RP.forward(s, TP.TINY_ENCODER, 2, xx, fx, y, use_gt=use_gt)[0]
    r64 = _restated_loop(sd, torch.float64, x, seq, T, call, plain=True)
    r32 = _restated_loop(sd, torch.float32, x, seq, T, call, plain=True)
    m = m.cuda().set_engine(engine).train()
    _fold_and_eager(m, x, seq, T, use_gt, True, r64, r32, f"plain tiny use_gt={use_gt} engine={engine}")


@pytest.mark.parametrize("kind", ["merged", "plain-gt", "plain-pred"])
def test_a_cut_fold_gives_what_one_folded_call_gives(monkeypatch, kind):
    """n = 3 windows cut into folded calls of 2 + 1 (what the 4 GiB rule does at large sizes) against one folded call: the
    same outputs, loss gradients and left-over state within the forward / gradient bounds of the acceptance table."""
    from transformerbasednavierstokesolver_amd import SequenSolver as S, SequenSolverMerged as SM
    torch.manual_seed(61)
    g = torch.Generator().manual_seed(62)
    if kind == "merged":
        m = SM.SequenSolver(None, T=3, W=8, H=8, M=8, C=16, B=2, sequential_head=8, layers=2, encoder_config=MERGED_ENCODER)
        _spread(m, m.in_project_slice.linear_post)
        x, seq, mod, use_gt = torch.from_numpy(RM.unified_positions(8, 8)).repeat(2, 1, 1), torch.randn(2, 64, 6, generator=g), SM, False
    else:
        m = S.SequenSolver(None, T=2, W=5, H=6, M=8, C=16, B=3, layers=2, encoder_config=TP.TINY_ENCODER)
        _spread(m, m.weight_projection.linear_post)
        x, seq, mod, use_gt = torch.rand(3, 30, 2, generator=g), torch.randn(3, 30, 5, generator=g), S, kind == "plain-gt"
    m, x, seq = m.cuda().train(), x.cuda(), seq.cuda()
    y = seq[..., m.T:]

    def run():
        for p in m.parameters():
            p.grad = None
        out = m.forward_windows(x, seq, use_gt=use_gt)
        ((out - y) ** 2).sum().backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        return out.detach(), grads, (m.code.detach().clone(), m.slice_weights.detach().clone(),
                                     m.encoder.get_attention_slice().clone())

    whole = run()
    sizes = []
    real = mod.fold_calls
    monkeypatch.setattr(mod, "fold_calls", lambda n, *a: sizes.append(n) or 2)
    cut = run()
    monkeypatch.setattr(mod, "fold_calls", real)
    assert sizes == [3]
    assert rel_l2(cut[0], whole[0]) <= 1e-5
    assert sorted(cut[1]) == sorted(whole[1])
    for k in whole[1]:
        if k != LAST + ".bias" and float(whole[1][k].abs().max()) > 0:      # that bias: true gradient 0, rounding only
            assert rel_l2(cut[1][k], whole[1][k]) <= _acceptance(".grad." + k), k
    for a, b in zip(cut[2], whole[2]):
        assert a.shape == b.shape and rel_l2(a, b) <= 1e-5


# ---------------------------------------------------------------------------------------------- against the reference
def _reference_losses(golden, mod, use_gt, engine):
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    hyper = json.loads(str(golden["train.hyper"]))
    m, (pos, fx, _, yy) = mod._golden_model(golden, "a", engine)
    opt = FusedAdamW(m.parameters(), lr=hyper["lr"], weight_decay=hyper["weight_decay"])
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=hyper["lr"], epochs=hyper["epochs"],
                                                steps_per_epoch=hyper["steps_per_epoch"])
    losses = []
    for _ in range(hyper["steps"]):
        m.train()
        loss, _ = harness.sequensolver_train_step(m, opt, sched, pos, fx, yy, use_gt=use_gt, grad_sync=opt.sync,
                                                  fold_time=True)
        losses.append(float(loss))
    want, rtol = golden["a.train.losses"], _bound(golden, "a.train.losses")
    print(f"folded training losses engine={engine} {losses} against {want.tolist()}, rtol {rtol:.3g}")
    np.testing.assert_allclose(losses, want, rtol=rtol)


@pytest.mark.parametrize("engine", ENGINES)
def test_folded_training_reproduces_the_merged_references_losses(engine):
    _reference_losses(np.load(TM.G13), TM, False, engine)


@pytest.mark.parametrize("engine", ENGINES)
def test_folded_training_reproduces_the_plain_references_losses(engine):
    _reference_losses(np.load(TP.G10), TP, True, engine)


# ---------------------------------------------------------------------------------------------- freeze
def _tiny_merged(B=1, seed=31):
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    torch.manual_seed(seed)
    m = SequenSolver(None, T=3, W=8, H=8, M=8, C=16, B=B, sequential_head=8, layers=2, encoder_config=MERGED_ENCODER)
    _spread(m, m.in_project_slice.linear_post)
    return m.cuda().train()


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("optimizer", ["AdamW", "FusedAdamW"])
def test_frozen_tensors_stop_moving(optimizer, fold):
    """The optimizer is built BEFORE freeze_attention() and has stepped every tensor once (momentum and decay are live);
    after the freeze an iteration leaves the frozen tensors bit for bit where they were, and moves the others."""
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    m = _tiny_merged()
    g = torch.Generator().manual_seed(32)
    x = torch.from_numpy(RM.unified_positions(8, 8)).cuda()
    fx, yy = torch.randn(1, 64, 3, generator=g).cuda(), torch.randn(1, 64, 2, generator=g).cuda()
    if optimizer == "FusedAdamW":
        opt = FusedAdamW(m.parameters(), lr=1e-2, weight_decay=1e-2)
        sync = opt.sync
    else:
        opt, sync = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=1e-2), None
    harness.sequensolver_train_step(m, opt, None, x, fx, yy, use_gt=False, grad_sync=sync, fold_time=fold)
    m.freeze_attention()
    names = [k for k, p in m.named_parameters() if not k.startswith("encoder.")]
    frozen = [k for k in names if not dict(m.named_parameters())[k].requires_grad]
    assert len(frozen) == 11 and len(names) > len(frozen)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    for _ in range(2):
        loss, _ = harness.sequensolver_train_step(m, opt, None, x, fx, yy, use_gt=False, grad_sync=sync, fold_time=fold)
    assert torch.isfinite(loss)
    after = dict(m.named_parameters())
    for k in frozen:
        assert torch.equal(after[k].detach(), before[k]), f"{optimizer}: frozen {k} moved"
    for k in names:
        if k not in frozen:
            assert not torch.equal(after[k].detach(), before[k]), f"{optimizer}: {k} did not move"


# ---------------------------------------------------------------------------------------------- the epoch loop
def test_fit_sequensolver_unfolded_is_the_hand_written_loop():
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.data import ResidentDataset
    from transformerbasednavierstokesolver_amd.optim import FusedAdamW
    ntrain, ntest, epochs, Tout = 3, 2, 2, 2
    g = torch.Generator().manual_seed(41)
    pos = torch.from_numpy(RM.unified_positions(8, 8)).cuda()
    a, u = torch.randn(ntrain + ntest, 64, 3, generator=g).cuda(), torch.randn(ntrain + ntest, 64, Tout, generator=g).cuda()
    orders = [[2, 0, 1], [1, 2, 0]]
    base = _tiny_merged(seed=42)

    def make():
        m = copy.deepcopy(base)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, epochs=epochs, steps_per_epoch=ntrain)
        return m, opt, sched

    m1, opt1, sched1 = make()
    hist = harness.fit_sequensolver(m1, opt1, sched1, pos, ResidentDataset(a[:ntrain], u[:ntrain]),
                                    ResidentDataset(a[ntrain:], u[ntrain:]), epochs=epochs, epoch_orders=orders,
                                    grad_sync=opt1.sync)
    m2, opt2, sched2 = make()
    loss_fn = harness.TestLoss(size_average=False)
    for ep in range(epochs):
        m2.train()
        acc = torch.zeros(5, dtype=torch.float64, device="cuda")
        for i in orders[ep]:
            loss, full = harness.sequensolver_train_step(m2, opt2, sched2, pos, a[i:i + 1], u[i:i + 1], use_gt=False,
                                                         grad_sync=opt2.sync)
            acc[0] += loss
            acc[1] += full
        m2.eval()
        for i in range(ntrain, ntrain + ntest):
            pred, loss, full = harness.sequensolver_rollout(m2, pos, a[i:i + 1], u[i:i + 1], use_gt=True)
            acc[2] += loss
            acc[3] += full
            acc[4] += loss_fn(pred[..., 0].reshape(1, -1), u[i:i + 1, :, 0].reshape(1, -1))
        s = acc.tolist()
        want = dict(train_step=s[0] / ntrain / 3, train_full=s[1] / ntrain, test_step=s[2] / ntest / 3,
                    test_full=s[3] / ntest, test_first=s[4] / ntest)
        assert hist[ep] == want, (ep, hist[ep], want)
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k
    # the folded loop runs the same epochs within the loss bound of the acceptance table
    m3, opt3, sched3 = make()
    folded = harness.fit_sequensolver(m3, opt3, sched3, pos, ResidentDataset(a[:ntrain], u[:ntrain]),
                                      ResidentDataset(a[ntrain:], u[ntrain:]), epochs=epochs, epoch_orders=orders,
                                      grad_sync=opt3.sync, fold_time=True)
    for ep in range(epochs):
        for k, v in hist[ep].items():
            print(f"epoch {ep} {k}: eager {v:.9g}, folded {folded[ep][k]:.9g}")
            assert abs(folded[ep][k] - v) <= 2e-5 * abs(v), (ep, k)


# ---------------------------------------------------------------------------------------------- the unchanged path
def test_slice_predictor_groups_1_is_the_path_as_it_was():
    """groups = 1 (the default) runs the code as it was, per-sample loop included: the same bits with and without the
    keyword, at B = 2 (the loop) and B = 1.  groups = B (every sample its own call) equals B separate calls within the
    forward bound, which the whole-batch statistics of groups = 1 do not."""
    from transformerbasednavierstokesolver_amd import SliceLearner as SL
    torch.manual_seed(51)
    v = SL.VorticitySliceLearner(C=16, M=8, T=3, H=8, W=8, n_hidden=32).cuda()
    g = torch.Generator().manual_seed(52)
    x = torch.from_numpy(RM.unified_positions(8, 8)).repeat(2, 1, 1).cuda()
    fx, code = torch.randn(2, 64, 3, generator=g).cuda(), torch.randn(2, 1, 8, 16, generator=g).cuda()
    fx[1], code[1] = 3.0 * fx[1] + 0.5, 3.0 * code[1] + 0.5
    args = (v.preprocess, v.in_project_x, v.in_project_slice, v.temperature, 8, 8, 8, 16, None)
    with torch.no_grad():
        as_it_was = SL.code_conditioned_slice_weights(x, fx, code, *args)
        assert torch.equal(v(x, fx, code), as_it_was)
        assert torch.equal(SL.code_conditioned_slice_weights(x, fx, code, *args, groups=1), as_it_was)
        one = SL.code_conditioned_slice_weights(x[:1], fx[:1], code[:1], *args)
        assert torch.equal(SL.code_conditioned_slice_weights(x[:1], fx[:1], code[:1], *args, groups=1), one)
        each = torch.cat([SL.code_conditioned_slice_weights(x[b:b + 1], fx[b:b + 1], code[b:b + 1], *args) for b in range(2)])
        per_call = SL.code_conditioned_slice_weights(x, fx, code, *args, groups=2)
    assert rel_l2(per_call, each) <= 1e-5 and rel_l2(as_it_was, each) > 1e-5
