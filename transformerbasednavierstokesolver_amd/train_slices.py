"""Command line in place of the three slice trainers of the reference's LearnSlice.py (train, train_from_vorticity,
train_from_previous), which have no parser: their hard-coded values are the flag defaults.

    python -m transformerbasednavierstokesolver_amd.train_slices --driver previous --eval 0 \\
        --encoder_path sequential_checkpoints/encoder_ep20_head_1.pt \\
        --sequensolver_path sequential_checkpoints/tokenizer_ep10_sim10_2.pt --data_path /data/fno

    driver       script function        model                               epochs  ntrain  save_name
    learnslice   train                  LearnSlice.LearnSlice               1       10      buff
    vorticity    train_from_vorticity   SliceLearner.VorticitySliceLearner  5       10      buff (the script's own is commented out)
    previous     train_from_previous    SliceLearner.PreviousSliceLearner   50      50      slice_ep5_sim50_unified_vort

Common to the three: lr = 1e-3, weight decay 1e-5, ntest = 10, unified_pos = 1, use_vorticity = 1 (learnslice: the point
features hold the window), use_code_for_vorticity = 1 (vorticity), batch size 1, Tin = Tout = 10, the frozen
SequenSolver(T=10, H=64, W=64, M=16, C=32, B=1, layers=8) built on `--encoder_path` and loaded from `--sequensolver_path`
(strict=False, as the scripts load it).  `--eval` defaults to 1 (LearnSlice.py's `__main__` calls train(eval=True)): it
loads ./sequential_checkpoints/<save_name>.pt and runs the kind's prediction-feedback rollout over the test set
(`slice_learner_test_loss` for learnslice, which has no rollout of its own); `--eval 0` trains with `harness.fit_slice_learner`.
The schedule is OneCycleLR over the run: one step per frame for learnslice (steps_per_epoch = batches * Tout, :405-406), one
per batch otherwise.  The optimizer is `optim.FusedAdamW`.  Data and positions come from train_sequence.py's loaders.

`--fold_time`: everything the frozen sequence model contributes to an iteration from ONE `SequenSolver.code_windows` call,
and the conv / previous-slice predictors on the Tout folded samples.  It defaults to 1 for all three drivers by the rule of
DESIGN 4.17: measured on the MI355X at the reference shape the folded median lies outside, below, the eager route's whole
measured range for each (ms, median (min .. max) of 9: learnslice 45.87 (45.28 .. 47.78) -> 7.58 (7.53 .. 7.76), vorticity
48.90 (48.76 .. 50.61) -> 6.07 (6.02 .. 6.18), previous 65.78 (65.45 .. 69.51) -> 11.81 (11.67 .. 12.08)).
`--fold_time 0` runs the scripts' loops."""
from __future__ import annotations

import argparse
import math
import os
import sys

from . import cli
from .train_sequence import BATCH_SIZE, CHECKPOINTS, ENCODER_CHECKPOINT, GEOMETRY, LAYERS, LR, T_IN, T_OUT, WEIGHT_DECAY

DRIVERS = ("learnslice", "vorticity", "previous")
SEQUENSOLVER_CHECKPOINT = os.path.join("sequential_checkpoints", "tokenizer_ep10_sim10_2.pt")
_SCRIPT = {
    "learnslice": dict(epochs=1, ntrain=10, save_name="buff"),
    "vorticity": dict(epochs=5, ntrain=10, save_name="buff"),
    "previous": dict(epochs=50, ntrain=50, save_name="slice_ep5_sim50_unified_vort"),
}
NTEST = 10
# folded median against the eager range on the MI355X at B = 1, N = 4096, M = 16, C = 32, T = Tout = 10:
# outside, below, for all three
FOLD_TIME_DEFAULT = {"learnslice": 1, "vorticity": 1, "previous": 1}


def build_parser(driver):
    """The script function's constants as flags, then what the scripts have no counterpart for."""
    d = _SCRIPT[driver]
    p = argparse.ArgumentParser("Training slice learners")
    p.add_argument("--epochs", type=int, default=d["epochs"])
    p.add_argument("--ntrain", type=int, default=d["ntrain"])
    p.add_argument("--ntest", type=int, default=NTEST)
    p.add_argument("--lr", type=float, default=LR)
    p.add_argument("--weight_decay", type=float, default=WEIGHT_DECAY)
    p.add_argument("--save_name", type=str, default=d["save_name"])
    p.add_argument("--unified_pos", type=int, default=1)
    p.add_argument("--use_vorticity", type=int, default=1)
    p.add_argument("--use_code_for_vorticity", type=int, default=1)
    p.add_argument("--eval", type=int, default=1)
    p.add_argument("--encoder_path", type=str, default=ENCODER_CHECKPOINT)
    p.add_argument("--sequensolver_path", type=str, default=SEQUENSOLVER_CHECKPOINT)
    p.add_argument("--data_path", type=str, default="./data/fno")
    p.add_argument("--fold_time", type=int, default=FOLD_TIME_DEFAULT[driver],
                   help="1: codes, targets and previous slices of an iteration from one code_windows call")
    p.add_argument("--gpu", type=str, default="0", help="GPU index to use")
    cli.add_driver_flags(p, DRIVERS, driver)
    return p


def parse_args(argv=None):
    return cli.parse(argv, DRIVERS, build_parser, required=True)[1]


def build_learner(args):
    """The driver's model at the scripts' geometry (M = 16, C = 32, T = 10, 64 x 64)."""
    M, C = GEOMETRY["M"], GEOMETRY["C"]
    if args.driver == "learnslice":
        from .LearnSlice import LearnSlice
        return LearnSlice(unified_pos=args.unified_pos, use_vorticity=args.use_vorticity, C=C, M=M, T=T_IN)
    if args.driver == "vorticity":
        from .SliceLearner import VorticitySliceLearner
        return VorticitySliceLearner(args.unified_pos, bool(args.use_code_for_vorticity), C=C, M=M, T=T_IN,
                                     H=GEOMETRY["H"], W=GEOMETRY["W"])
    from .SliceLearner import PreviousSliceLearner
    return PreviousSliceLearner(C=C, M=M)


def build_sequen_solver(args, dev):
    """The frozen sequence model of the three scripts (:389-398)."""
    from .SequenSolver import SequenSolver, load_frozen
    return load_frozen(args.sequensolver_path, lambda: SequenSolver(args.encoder_path, T=T_IN, B=BATCH_SIZE, layers=LAYERS,
                                                                    **GEOMETRY), strict=False, device=dev)


def run(args):
    from . import data, harness
    dev = cli.device(args)
    split = data.split_ns_trajectories(cli.ns_mat(args), args.ntrain, args.ntest, T_IN, T_OUT)
    H, W = GEOMETRY["H"], GEOMETRY["W"]
    pos = (data.unified_positions(H, W) if args.unified_pos else data.grid_positions(H, W)).to(dev)
    train = data.ResidentDataset(split["train_a"].float(), split["train_u"].float(), device=dev)
    test = data.ResidentDataset(split["test_a"].float(), split["test_u"].float(), device=dev)
    solver = build_sequen_solver(args, dev)
    model = build_learner(args).to(dev)
    cli.set_engine(args, solver, *([model] if hasattr(model, "set_engine") else []))
    cli.describe(args)
    kind = args.driver
    save_path = cli.checkpoint(CHECKPOINTS, args)
    if args.eval:
        cli.load_state(model, save_path, dev, strict=False)
        m = harness.evaluate_slice_learner(kind, model, solver, pos, test, args.use_vorticity, BATCH_SIZE)
        print(m)
        return m
    steps = math.ceil(args.ntrain / BATCH_SIZE) * (T_OUT if kind == "learnslice" else 1)
    opt, sched = cli.optim(model, args.lr, args.weight_decay, args.epochs, steps)
    return harness.fit_slice_learner(
        model, opt, sched, solver, pos, train, test, epochs=args.epochs, batch_size=BATCH_SIZE, kind=kind,
        fold_time=bool(args.fold_time), use_vorticity=args.use_vorticity, save_path=save_path, grad_sync=opt.sync,
        on_epoch=lambda ep, m: print(f"loss epoch {ep}: {m['train']} , overall test loss {m['test']}", flush=True))


def main(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
