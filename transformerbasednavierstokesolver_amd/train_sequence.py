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

from . import cli

DRIVERS = ("autoencoder", "sequensolver", "sequensolver_merged")
T_IN = T_OUT = 10
STEP = 1
LR, WEIGHT_DECAY, BATCH_SIZE = 1e-3, 1e-5, 1                      # the sequence scripts' constants
GEOMETRY = dict(H=64, W=64, M=16, C=32)
LAYERS, SEQUENTIAL_HEAD = 8, 16
CHECKPOINTS = "./sequential_checkpoints"
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
        cli.add_core_flags(p, epochs=30, gpu="0", save_name="ns_2d_UniPDE", downsample=1)
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
    cli.add_driver_flags(p, DRIVERS, driver)
    return p


def parse_args(argv=None):
    return cli.parse(argv, DRIVERS, build_parser, required=True)[1]


def run_autoencoder(args):
    from . import data, harness
    from .model import Transolver_Structured_Mesh2D_Encoder
    dev = cli.device(args)
    if args.downsample != 1:        # the script trains on data['u'][:ntrain, :, :, :] whatever --downsample says, at H = W = h
        raise SystemExit("--downsample other than 1: auto_encoder.py builds an h x h model and feeds it the full 64 x 64 frames")
    d = data.split_ns_all_frames(cli.ns_mat(args), args.ntrain, args.ntest)
    d = dict(d, train=d["train"].float(), test=d["test"].float())
    model = Transolver_Structured_Mesh2D_Encoder.Model(**cli.model_kwargs(args, 1, H=d["h"], W=d["h"])).to(dev)
    cli.set_engine(args, model)
    cli.describe(args, model)
    save_path = cli.checkpoint(CHECKPOINTS, args)
    if args.eval:
        cli.load_state(model, save_path, dev, strict=False)
        m = harness.evaluate_autoencoder(model, d, args.batch_size, args.ntest)
        print(m["test_l2"])
        return m
    opt, sched = cli.optim(model, args.lr, args.weight_decay, args.epochs, math.ceil(d["train"].shape[0] / args.batch_size))
    return harness.fit_autoencoder(
        model, opt, sched, d, epochs=args.epochs, batch_size=args.batch_size, ntrain=args.ntrain, ntest=args.ntest, T=T_OUT,
        step=STEP, max_grad_norm=args.max_grad_norm, save_path=save_path, grad_sync=opt.sync,
        on_epoch=lambda ep, m: print(f"Epoch {ep} , train_step_loss:{m['train_step']} , test_step_loss:{m['test_step']}",
                                     flush=True))


def load_slice_learner(args, model, dev):
    """The LearnSlice module of the plain script's evaluation (SequenSolver.py:541-570: unified_pos = 1, use_vorticity = 1),
    loaded ONCE from --slice_learner_path; the script builds and loads it once per frame."""
    from .LearnSlice import LearnSlice
    from .SequenSolver import load_frozen
    if args.slice_learner_path is None:
        raise SystemExit("--driver sequensolver --eval 1 needs --slice_learner_path (a LearnSlice checkpoint)")
    return load_frozen(args.slice_learner_path, lambda: LearnSlice(
        unified_pos=1, use_vorticity=1, use_code_for_vorticity=False, C=model.C, M=model.M, T=model.T),
        strict=True, device=dev, freeze=False)


def run_sequensolver(args):
    from . import data, harness
    merged = args.driver == "sequensolver_merged"
    dev = cli.device(args)
    split = data.split_ns_trajectories(cli.ns_mat(args), args.sim_num, args.ntest, T_IN, T_OUT)
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
    cli.set_engine(args, model)
    cli.describe(args)
    save_path = cli.checkpoint(CHECKPOINTS, args)
    if args.eval:
        cli.load_state(model, save_path, dev, strict=False)
        m = harness.evaluate_sequensolver(model, pos, test, args.ntest, BATCH_SIZE,
                                          slice_learner=None if merged else load_slice_learner(args, model, dev))
        print(m["test_full"])
        return m
    opt, sched = cli.optim(model, LR, WEIGHT_DECAY, args.epochs, math.ceil(args.sim_num / BATCH_SIZE))

    def line(ep, m):
        print("Epoch {} , train_step_loss:{:.5f} , train_full_loss:{:.5f} , test_step_loss:{:.5f} , test_full_loss:{:.5f}".format(
            ep, m["train_step"], m["train_full"], m["test_step"], m["test_full"]), flush=True)
        if merged:
            print(f"first frame loss {m['test_first']}", flush=True)

    return harness.fit_sequensolver(model, opt, sched, pos, train, test, epochs=args.epochs, batch_size=BATCH_SIZE,
                                    variant="merged" if merged else "plain", Tin=T_IN, fold_time=bool(args.fold_time),
                                    save_path=save_path, grad_sync=opt.sync, on_epoch=line)


def main(argv=None):
    args = parse_args(argv)
    if args.driver == "autoencoder":
        return run_autoencoder(args)
    return run_sequensolver(args)


if __name__ == "__main__":
    main(sys.argv[1:])
