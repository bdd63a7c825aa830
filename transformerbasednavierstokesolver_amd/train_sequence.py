"""Command line in place of the reference's auto_encoder.py, SequenSolver.py and SequenSolverMerged.py training scripts:

    python -m transformerbasednavierstokesolver_amd.train_sequence --driver autoencoder --n-hidden 32 --n-layers 8 \\
        --n-heads 1 --slice_num 16 --unified_pos 1 --data_path /data/fno --save_name encoder_ep20_head_1
    python -m transformerbasednavierstokesolver_amd.train_sequence --driver sequensolver_merged --eval 0 --sim_num 10 \\
        --transolver_path sequential_checkpoints/encoder_ep20_head_1.pt --data_path /data/fno

`--driver autoencoder` has auto_encoder.py's argparse table with its defaults.  `--driver sequensolver_merged` has
SequenSolverMerged.py's (`--eval` default 1, `--epochs` 10, `--save_name buff`, `--sim_num` 10).  SequenSolver.py has no
parser: its hard-coded epochs = 10, ntrain = 10 (here `--sim_num`, as in the merged script), ntest = 2 and
save_name = tokenizer_ep10_sim10_2 are the defaults of `--driver sequensolver`, and so is `--eval 1` (its `__main__` calls
train(eval=True)).  lr = 1e-3, weight_decay = 1e-5, batch size 1, Tin = Tout = 10, 64 x 64, M = 16, C = 32, layers = 8 and
sequential_head = 16 are the scripts' constants.

Added: `--driver`, `--data_path` (the scripts hard-code theirs: a `.mat` file or the directory that holds
NavierStokes_V1e-5_N1200_T20.mat, directly or in a folder of that name), `--transolver_path` (the frozen encoder's
checkpoint; the scripts hard-code sequential_checkpoints/encoder_ep20_head_1.pt), `--engine`, `--ntest` (the scripts' 20, 2
and 10), `--gpu` where the script has none, `--slice_learner_path` (plain `--eval 1`) and `--fold_time`.

`--fold_time` defaults to 1: the Tout teacher-forced calls of an iteration run as one `forward_windows` call.  Measured on
the MI355X at both reference shapes the folded median (9.3 / 9.8 ms) lies outside, below, the eager route's whole measured
range (54.5 .. 164.2 / 62.6 .. 77.3 ms): DESIGN 4.17.  `--fold_time 0` runs the scripts' ten calls.

The optimizer is `optim.FusedAdamW`, the schedule `OneCycleLR` over the whole run, the loops `harness.fit_autoencoder` /
`fit_sequensolver`.  Checkpoints go to ./sequential_checkpoints/<save_name>.pt as in the scripts.  `--eval 1` loads that file
and runs the scripts' evaluation loops without their prints and plots: the auto-encoder's reconstruction loss / ntest, the
merged model's prediction-feedback rollout with use_gt=False, the plain model's `solve_with_slice_learner` rollout with the
script's unified_pos = 1, use_vorticity = 1 and the LearnSlice checkpoint `--slice_learner_path`."""
from __future__ import annotations

import argparse
import math
import os
import sys

DRIVERS = ("autoencoder", "sequensolver", "sequensolver_merged")
NS_FILE = "NavierStokes_V1e-5_N1200_T20"
T_IN = T_OUT = 10
STEP = 1
LR, WEIGHT_DECAY, BATCH_SIZE = 1e-3, 1e-5, 1                      # the sequence scripts' constants
GEOMETRY = dict(H=64, W=64, M=16, C=32)
LAYERS, SEQUENTIAL_HEAD = 8, 16
ENCODER_CHECKPOINT = os.path.join("sequential_checkpoints", "encoder_ep20_head_1.pt")
_SEQUENCE = {
    "sequensolver": dict(eval=1, epochs=10, save_name="tokenizer_ep10_sim10_2", sim_num=10, ntest=2),
    "sequensolver_merged": dict(eval=1, epochs=10, save_name="buff", sim_num=10, ntest=10),
}
FOLD_TIME_DEFAULT = 1


def build_parser(driver):
    """The reference script's flag table, then the flags that are not in the reference."""
    p = argparse.ArgumentParser("Training Transformer")
    if driver == "autoencoder":
        p.add_argument("--lr", type=float, default=1e-3)
        p.add_argument("--epochs", type=int, default=30)
        p.add_argument("--weight_decay", type=float, default=1e-5)
        p.add_argument("--model", type=str, default="Transolver_2D")
        p.add_argument("--n-hidden", type=int, default=64, help="hidden dim")
        p.add_argument("--n-layers", type=int, default=3, help="layers")
        p.add_argument("--n-heads", type=int, default=4)
        p.add_argument("--batch-size", type=int, default=8)
        p.add_argument("--gpu", type=str, default="0", help="GPU index to use")
        p.add_argument("--max_grad_norm", type=float, default=None)
        p.add_argument("--downsample", type=int, default=1)
        p.add_argument("--mlp_ratio", type=int, default=1)
        p.add_argument("--dropout", type=float, default=0.0)
        p.add_argument("--unified_pos", type=int, default=0)
        p.add_argument("--ref", type=int, default=8)
        p.add_argument("--slice_num", type=int, default=32)
        p.add_argument("--eval", type=int, default=0)
        p.add_argument("--save_name", type=str, default="ns_2d_UniPDE")
        p.add_argument("--data_path", type=str, default="/data/fno")
        p.add_argument("--ntrain", type=int, default=100)          # the script's module globals
        p.add_argument("--ntest", type=int, default=20)
    else:
        d = _SEQUENCE[driver]
        p.add_argument("--eval", type=int, default=d["eval"])
        p.add_argument("--epochs", type=int, default=d["epochs"])
        p.add_argument("--save_name", type=str, default=d["save_name"])
        p.add_argument("--sim_num", type=int, default=d["sim_num"])
        p.add_argument("--data_path", type=str, default="./data/fno")
        p.add_argument("--transolver_path", type=str, default=ENCODER_CHECKPOINT)
        p.add_argument("--ntest", type=int, default=d["ntest"])
        p.add_argument("--gpu", type=str, default="0", help="GPU index to use")
        p.add_argument("--fold_time", type=int, default=FOLD_TIME_DEFAULT,
                       help="1: the Tout teacher-forced calls of an iteration as one folded call")
        if driver == "sequensolver":
            p.add_argument("--slice_learner_path", type=str, default=None, help="LearnSlice checkpoint of --eval 1")
    p.add_argument("--driver", choices=DRIVERS, default=driver)
    p.add_argument("--engine", type=str, default=None, help="GEMM engine: f32 | split | bf16")
    return p


def parse_args(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--driver", choices=DRIVERS, required=True)
    driver = pre.parse_known_args(argv)[0].driver
    return build_parser(driver).parse_args(argv)


def _checkpoint(args):
    return os.path.join("./sequential_checkpoints", args.save_name + ".pt")


def _ns_mat(args):
    import scipy.io as scio
    from .train import _find
    return scio.loadmat(_find(args.data_path, (NS_FILE + ".mat", os.path.join(NS_FILE, NS_FILE + ".mat"))))["u"]


def _optim(model, lr, weight_decay, epochs, steps_per_epoch, clip=None):
    import torch
    from .optim import FusedAdamW
    opt = FusedAdamW(model.parameters(), lr=lr, weight_decay=weight_decay, max_grad_norm=clip)
    return opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, epochs=epochs, steps_per_epoch=steps_per_epoch)


def run_autoencoder(args):
    import torch
    from . import data, harness
    from .model import Transolver_Structured_Mesh2D_Encoder
    from .train import _device
    dev = _device(args)
    if args.downsample != 1:        # the script trains on data['u'][:ntrain, :, :, :] whatever --downsample says, at H = W = h
        raise SystemExit("--downsample other than 1: auto_encoder.py builds an h x h model and feeds it the full 64 x 64 frames")
    d = data.split_ns_all_frames(_ns_mat(args), args.ntrain, args.ntest)
    d = dict(d, train=d["train"].float(), test=d["test"].float())
    h = d["h"]
    model = Transolver_Structured_Mesh2D_Encoder.Model(
        space_dim=2, n_layers=args.n_layers, n_hidden=args.n_hidden, dropout=args.dropout, n_head=args.n_heads,
        Time_Input=False, mlp_ratio=args.mlp_ratio, fun_dim=1, out_dim=1, slice_num=args.slice_num, ref=args.ref,
        unified_pos=args.unified_pos, H=h, W=h).to(dev)
    if args.engine is not None:
        model.set_engine(args.engine)
    print(args)
    print(f"Total Trainable Params: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
    if args.eval:
        model.load_state_dict(torch.load(_checkpoint(args), map_location=dev, weights_only=True), strict=False)
        model.eval()
        loss_fn = harness.TestLoss(size_average=False)
        pos = data.grid_positions(h).to(dev)
        total = torch.zeros((), dtype=torch.float64, device=dev)
        with torch.no_grad():
            for fx, in data.ResidentDataset(d["test"], device=dev).batches(args.batch_size):
                bsz = fx.shape[0]
                total += loss_fn(model(pos.expand(bsz, -1, -1).contiguous(), fx=fx).reshape(bsz, -1), fx.reshape(bsz, -1))
        m = dict(test_l2=float(total) / args.ntest)
        print(m["test_l2"])
        return m
    steps = math.ceil(d["train"].shape[0] / args.batch_size)
    opt, sched = _optim(model, args.lr, args.weight_decay, args.epochs, steps)
    return harness.fit_autoencoder(
        model, opt, sched, d, epochs=args.epochs, batch_size=args.batch_size, ntrain=args.ntrain, ntest=args.ntest, T=T_OUT,
        step=STEP, max_grad_norm=args.max_grad_norm, save_path=_checkpoint(args), grad_sync=opt.sync,
        on_epoch=lambda ep, m: print(f"Epoch {ep} , train_step_loss:{m['train_step']} , test_step_loss:{m['test_step']}",
                                     flush=True))


def run_sequensolver(args):
    import torch
    from . import data, harness
    from .train import _device
    merged = args.driver == "sequensolver_merged"
    dev = _device(args)
    split = data.split_ns_trajectories(_ns_mat(args), args.sim_num, args.ntest, T_IN, T_OUT)
    pos = data.unified_positions(GEOMETRY["H"], GEOMETRY["W"]).to(dev)            # both scripts set unified_pos = 1
    train = data.ResidentDataset(split["train_a"].float(), split["train_u"].float(), device=dev)
    test = data.ResidentDataset(split["test_a"].float(), split["test_u"].float(), device=dev)
    if merged:
        from .SequenSolverMerged import SequenSolver
        model = SequenSolver(args.transolver_path, T=T_IN, B=BATCH_SIZE, layers=LAYERS, sequential_head=SEQUENTIAL_HEAD, **GEOMETRY)
    else:
        from .SequenSolver import SequenSolver
        model = SequenSolver(args.transolver_path, T=T_IN, B=BATCH_SIZE, layers=LAYERS, **GEOMETRY)
    model = model.to(dev)
    if args.engine is not None:
        model.set_engine(args.engine)
    print(args)
    if args.eval:
        model.load_state_dict(torch.load(_checkpoint(args), map_location=dev, weights_only=True), strict=False)
        model.eval()
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for fx, yy in test.batches(BATCH_SIZE):
            if merged:
                _, _, full = harness.sequensolver_rollout(model, pos, fx, yy, use_gt=False)
            else:
                full = _slice_learner_rollout(model, args.slice_learner_path, pos, fx, yy)
            total += full
        m = dict(test_full=float(total) / args.ntest)
        print(m["test_full"])
        return m
    opt, sched = _optim(model, LR, WEIGHT_DECAY, args.epochs, math.ceil(args.sim_num / BATCH_SIZE))

    def line(ep, m):
        print("Epoch {} , train_step_loss:{:.5f} , train_full_loss:{:.5f} , test_step_loss:{:.5f} , test_full_loss:{:.5f}".format(
            ep, m["train_step"], m["train_full"], m["test_step"], m["test_full"]), flush=True)
        if merged:
            print(f"first frame loss {m['test_first']}", flush=True)

    return harness.fit_sequensolver(model, opt, sched, pos, train, test, epochs=args.epochs, batch_size=BATCH_SIZE,
                                    variant="merged" if merged else "plain", Tin=T_IN, fold_time=bool(args.fold_time),
                                    save_path=_checkpoint(args), grad_sync=opt.sync, on_epoch=line)


def _slice_learner_rollout(model, slice_learner_path, pos, fx, yy):
    """SequenSolver.py:553-568: Tout prediction-feedback calls of solve_with_slice_learner; the full rel-L2 of the batch."""
    import torch
    from . import harness, ops
    from .LearnSlice import LearnSlice
    from .SequenSolver import load_frozen
    if slice_learner_path is None:
        raise SystemExit("--driver sequensolver --eval 1 needs --slice_learner_path (a LearnSlice checkpoint)")
    learner = load_frozen(slice_learner_path, lambda: LearnSlice(       # built once, not once per frame as the script does
        unified_pos=1, use_vorticity=1, use_code_for_vorticity=False, C=model.C, M=model.M, T=model.T),
        strict=True, device=fx.device, freeze=False)
    bsz, preds = fx.shape[0], []
    with torch.no_grad(), ops.weights_frozen():
        for t in range(yy.shape[-1]):
            im = model.solve_with_slice_learner(learner, pos.expand(bsz, -1, -1).contiguous(), fx, yy[..., t:t + 1],
                                                unified_pos=1, use_vorticity=1)
            preds.append(im)
            fx = torch.cat((fx[..., 1:], im), dim=-1)
    pred = torch.cat(preds, -1)
    return harness.TestLoss(size_average=False)(pred.reshape(bsz, -1), yy.reshape(bsz, -1))


def main(argv=None):
    args = parse_args(argv)
    if args.driver == "autoencoder":
        return run_autoencoder(args)
    return run_sequensolver(args)


if __name__ == "__main__":
    main(sys.argv[1:])
