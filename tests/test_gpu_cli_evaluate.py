"""harness.evaluate_autoencoder / evaluate_sequensolver / evaluate_slice_learner on the MI355X against the evaluation loops
that the command lines held before they moved into the harness, restated below as they stood in train_sequence.py
(:138-150 auto-encoder, :180-192 both sequence models, :206-225 the LearnSlice rollout, which built and loaded its
LearnSlice once per test batch) and train_slices.py (:126-143).  The forward kernels are deterministic and both sides make the
same launches on the same values: the dicts are EQUAL, not close.  Tiny models of test_gpu_slice_trainers.py (6 x 5 mesh,
M = 8, C = 16, T = 2, layers = 2), test_gpu_sequensolver_merged.py and the encoder of both; test sets of 2 samples at batch size
1 with 3 output frames: more than one batch (the divisors) and more than one frame (the window feedback)."""
import pytest
import torch

import test_gpu_slice_trainers as ST
from test_sequensolver_merged_host import TINY_ENCODER

pytestmark = pytest.mark.gpu
NOUT = 3


# ------------------------------------------------------------------------------------- the loops as the command lines had them
def _was_autoencoder(model, d, batch_size, ntest, dev):
    from transformerbasednavierstokesolver_amd import data, harness
    model.eval()
    loss_fn = harness.TestLoss(size_average=False)
    pos = data.grid_positions(d["h"]).to(dev)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    with torch.no_grad():
        for fx, in data.ResidentDataset(d["test"], device=dev).batches(batch_size):
            bsz = fx.shape[0]
            total += loss_fn(model(pos.expand(bsz, -1, -1).contiguous(), fx=fx).reshape(bsz, -1), fx.reshape(bsz, -1))
    return dict(test_l2=float(total) / ntest)


def _was_sequensolver(model, pos, test, ntest, merged, dev, learner_file=None, build_learner=None):
    from transformerbasednavierstokesolver_amd import harness
    model.eval()
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for fx, yy in test.batches(1):
        if merged:
            _, _, full = harness.sequensolver_rollout(model, pos, fx, yy, use_gt=False)
        else:
            full = _was_slice_learner_rollout(model, learner_file, build_learner, pos, fx, yy)
        total += full
    return dict(test_full=float(total) / ntest)


def _was_slice_learner_rollout(model, learner_file, build_learner, pos, fx, yy):
    from transformerbasednavierstokesolver_amd import harness, ops
    from transformerbasednavierstokesolver_amd.SequenSolver import load_frozen
    learner = load_frozen(learner_file, build_learner, strict=True, device=fx.device, freeze=False)      # once per batch
    bsz, preds = fx.shape[0], []
    with torch.no_grad(), ops.weights_frozen():
        for t in range(yy.shape[-1]):
            im = model.solve_with_slice_learner(learner, pos.expand(bsz, -1, -1).contiguous(), fx, yy[..., t:t + 1],
                                                unified_pos=1, use_vorticity=1)
            preds.append(im)
            fx = torch.cat((fx[..., 1:], im), dim=-1)
    pred = torch.cat(preds, -1)
    return harness.TestLoss(size_average=False)(pred.reshape(bsz, -1), yy.reshape(bsz, -1))


def _was_slice_learner(kind, model, solver, pos, test, use_vorticity, dev):
    from transformerbasednavierstokesolver_amd import harness
    model.eval()
    loss_fn = harness.TestLoss(size_average=False)
    total = torch.zeros(2, dtype=torch.float64, device=dev)
    for fx, yy in test.batches(1):
        bsz = fx.shape[0]
        x = pos.expand(bsz, -1, -1).contiguous()
        if kind == "learnslice":
            total[0] += harness.slice_learner_test_loss(kind, model, solver, x, fx, yy, use_vorticity) / yy.shape[-1]
            continue
        rollout = harness.slice_predictor_rollout if kind == "vorticity" else harness.previous_slice_rollout
        pred = rollout(model, solver, x, fx, yy.shape[-1])
        total[1] += loss_fn(pred.reshape(bsz, -1), yy.reshape(bsz, -1))
    a = total.tolist()
    return dict(test_slice=a[0] / len(test)) if kind == "learnslice" else dict(test_full=a[1] / len(test))


# ------------------------------------------------------------------------------------- the harness functions against them
def _same(got, want):
    print(f"harness {got}  command-line loop {want}")
    assert list(got) == list(want)
    for k, v in want.items():
        assert isinstance(got[k], float) and v > 0 and got[k] == v, k      # bit for bit


def _slice_test_set():
    from transformerbasednavierstokesolver_amd.data import ResidentDataset
    x, fx, yy = (t.cuda() for t in ST._data(nout=NOUT))
    return x[:1].contiguous(), ResidentDataset(fx, yy)


def test_evaluate_autoencoder_is_the_command_line_loop():
    """3 trajectories of 3 frames on the 8 x 8 mesh, the last 2 the test set: 6 frames at batch size 4, one full and one
    short batch; the divisor is the 2 trajectories."""
    from transformerbasednavierstokesolver_amd import data, harness
    from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh2D_Encoder import Model
    torch.manual_seed(11)
    model = Model(**TINY_ENCODER).cuda()
    u = torch.randn(3, 8, 8, NOUT, generator=torch.Generator().manual_seed(12)).numpy()
    d = data.split_ns_all_frames(u, 1, 2)
    assert tuple(d["test"].shape) == (6, 64, 1)
    want = _was_autoencoder(model, d, 4, 2, torch.device("cuda"))
    model.train()
    _same(harness.evaluate_autoencoder(model, d, 4, 2), want)
    assert not model.training


def test_evaluate_sequensolver_merged_is_the_command_line_loop():
    from transformerbasednavierstokesolver_amd import data, harness
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    torch.manual_seed(7)
    m = SequenSolver(None, T=3, W=8, H=8, M=8, C=16, B=2, sequential_head=8, layers=2, encoder_config=TINY_ENCODER)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(".bias") or k.startswith("ln_"):
                p.add_(0.1 * torch.randn_like(p))
        m.in_project_slice.linear_post.weight.mul_(4.0)
    m = m.cuda()
    g = torch.Generator().manual_seed(8)
    pos = data.unified_positions(8, 8).cuda()
    test = data.ResidentDataset(torch.randn(2, 64, 3, generator=g).cuda(), torch.randn(2, 64, NOUT, generator=g).cuda())
    want = _was_sequensolver(m, pos, test, 2, True, torch.device("cuda"))
    m.train()
    _same(harness.evaluate_sequensolver(m, pos, test, 2, 1), want)
    assert not m.training


def test_evaluate_sequensolver_plain_is_the_command_line_loop(tmp_path):
    """The plain model with a LearnSlice: the harness is handed ONE module, the command line's loop loaded the checkpoint
    into a new one for every test batch."""
    from transformerbasednavierstokesolver_amd import harness
    from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
    from transformerbasednavierstokesolver_amd.SequenSolver import load_frozen
    solver = ST._solver().cuda()
    path = str(tmp_path / "learner.pt")
    torch.save(ST._learner("learnslice").state_dict(), path)
    g = ST.GEOM
    build = lambda: LearnSlice(unified_pos=0, use_vorticity=1, C=g["C"], M=g["M"], T=g["T"])
    pos, test = _slice_test_set()
    want = _was_sequensolver(solver, pos, test, 2, False, torch.device("cuda"), path, build)
    learner = load_frozen(path, build, strict=True, device=torch.device("cuda"), freeze=False)
    _same(harness.evaluate_sequensolver(solver, pos, test, 2, 1, slice_learner=learner), want)


@pytest.mark.parametrize("kind", ["learnslice", "vorticity", "previous"])
def test_evaluate_slice_learner_is_the_command_line_loop(kind):
    from transformerbasednavierstokesolver_amd import harness
    solver, model = ST._solver().cuda(), ST._learner(kind).cuda()
    pos, test = _slice_test_set()
    want = _was_slice_learner(kind, model, solver, pos, test, 1, torch.device("cuda"))
    model.train()
    _same(harness.evaluate_slice_learner(kind, model, solver, pos, test, 1), want)
    assert not model.training
