"""Command line in place of the reference's ns_velocity.py, ns_velocity_unrolling.py and ns_unrolling2_with_t.py, the
trainers on PhiFlow velocity data (one prediction is a (vel_x, vel_y) pair: out_dim = step = 2):

    python -m transformerbasednavierstokesolver_amd.train_velocity --driver velocity --n-hidden 64 --n-heads 4 \\
        --n-layers 8 --slice_num 32 --batch-size 4 --data_path /data/ns_50_20.npy --save_name ns_velocity

`--driver {velocity,velocity_unrolled,unrolled_t}` selects the script.  The flags and their defaults are the scripts' own
(the three parsers are the same table).  Added: `--driver`, `--engine` (GEMM engine: f32 | split | bf16 | bf16s), `--graphed`
(0 | 1: full batches replay the whole iteration, optimizer step included, from one hipGraph per look-ahead value, and the
test pass replays one graphed scored rollout; bit-identical to `--graphed 0`), and the scripts' module-scope constants as
flags with the constants as defaults: `--ntrain` / `--ntest` (40 / 10, 40 / 10, 16 / 4), `--T_in` / `--T` (10, 20, 10 for
both), `--step` (2), `--max_look_ahead` (8 and 4; the unrolled drivers only).  `--gpu` is the device index.

`--data_path` is honoured (the scripts ignore it for a hard-coded path): the `.npy` file [S, 64, 64, >= T_in + T] whose
columns interleave (vel_x, vel_y) per frame, or a folder that holds ns_50_20.npy (ns_20_20.npy for `unrolled_t`);
`--data_path synthetic` runs on `synth.velocity_fields` (seeded, divergence-free) so that the command line works without
the PhiFlow file.

`velocity` builds `model_dict.get_model(args)`, the other two the SOL wrapper whatever --model says, as the scripts do.  The
optimizer is `optim.FusedAdamW` (clip threshold --max_grad_norm inside it; only ns_velocity.py clips), the schedule
OneCycleLR over the whole run, the loop `harness.fit_velocity` / `fit_velocity_unrolled` / `fit_unrolled_t`.  The
state_dict (the inner model's for the SOL drivers) goes to ./checkpoints/<save_name>.pt every 100 epochs and at the end;
`--eval 1` loads it and prints the test pass alone (no plots)."""
from __future__ import annotations

import argparse
import math
import sys

from . import cli

DRIVERS = ("velocity", "velocity_unrolled", "unrolled_t")
# the scripts' module-scope constants (ns_velocity.py:42-46, ns_velocity_unrolling.py:42-48, ns_unrolling2_with_t.py:42-48)
_CONSTANTS = {
    "velocity": dict(ntrain=40, ntest=10, T_in=10, T=10, file="ns_50_20.npy"),
    "velocity_unrolled": dict(ntrain=40, ntest=10, T_in=20, T=20, max_look_ahead=8, period=40, file="ns_50_20.npy"),
    "unrolled_t": dict(ntrain=16, ntest=4, T_in=10, T=10, max_look_ahead=4, period=10, file="ns_20_20.npy"),
}
STEP = 2
CHECKPOINTS = "./checkpoints"
SYNTHETIC = "synthetic"


def build_parser(driver):
    """The reference's flag table (one for the three scripts) with --driver / --engine."""
    p = argparse.ArgumentParser("Training Transformer")
    cli.add_core_flags(p, epochs=5, gpu="0", downsample=1, save_name="ns_2d_UniPDE")
    cli.add_driver_flags(p, DRIVERS, driver, engines="f32 | split | bf16 | bf16s")             # not in the reference
    return p


def command_line_parser(driver):
    """`build_parser(driver)` plus the scripts' module constants as flags and the flags that steer how this project runs
    the same loop."""
    p = build_parser(driver)
    c = _CONSTANTS[driver]
    for name in ("ntrain", "ntest", "T_in", "T"):
        p.add_argument("--" + name, type=int, default=c[name])
    p.add_argument("--step", type=int, default=STEP)
    if "max_look_ahead" in c:
        p.add_argument("--max_look_ahead", type=int, default=c["max_look_ahead"])
    p.add_argument("--graphed", type=int, default=0, help="1: full batches replay the whole iteration from one hipGraph")
    return p


def parse_args(argv=None):
    return cli.parse(argv, DRIVERS, command_line_parser, default="velocity")[1]


def _datasets(args, dev):
    from . import data, synth
    n_in = args.T_in + args.T
    if args.data_path == SYNTHETIC:
        arr = synth.velocity_fields(args.ntrain + args.ntest, frames=-(-n_in // STEP), seed=0)
    else:
        import numpy as np
        arr = np.load(cli.find(args.data_path, (_CONSTANTS[args.driver]["file"],)))
    h, train, test = data.split_velocity(arr, args.ntrain, args.ntest, args.T_in, args.T, args.downsample)
    return h, data.ResidentDataset(*(t.float() for t in train.tensors), device=dev), \
        data.ResidentDataset(*(t.float() for t in test.tensors), device=dev)


def run(args):
    from . import harness, model_dict
    from .model.SOL_Transolver_Structured_Mesh_2D import SOL_Transolver_Structured_Mesh_2D
    from .utils.testloss import FusedTestLoss
    dev = cli.device(args)
    h, train, test = _datasets(args, dev)
    kw = dict(cli.model_kwargs(args, args.T_in, H=h, W=h), out_dim=args.step)
    if args.driver == "velocity":
        model = inner = model_dict.get_model(args).Model(**kw).to(dev)
    else:
        model = SOL_Transolver_Structured_Mesh_2D(**kw, step=args.step, look_ahead=1).to(dev)
        inner = model.transolver_model
    cli.set_engine(args, inner)
    cli.describe(args, model)
    loss_fn = FusedTestLoss(size_average=False)
    save_path = cli.checkpoint(CHECKPOINTS, args)
    full = args.driver == "velocity"
    if args.eval:
        cli.load_state(inner, save_path, dev, strict=True)
        m = harness.evaluate_velocity(inner, test, args.batch_size, args.T, args.step, loss_fn, full=full,
                                      graphed=bool(args.graphed))
        print(m["test_full"] if full else "test_step_loss:{:.5f}".format(m["test_step"]))
        return m
    clip = args.max_grad_norm if full else None                 # the SOL scripts never clip
    opt, sched = cli.optim(model, args.lr, args.weight_decay, args.epochs, math.ceil(args.ntrain / args.batch_size), clip)
    common = dict(epochs=args.epochs, batch_size=args.batch_size, T=args.T, step=args.step, loss_fn=loss_fn, save_path=save_path,
                  grad_sync=opt.sync, graphed=bool(args.graphed))
    if full:
        return harness.fit_velocity(
            model, opt, sched, train, test, **common,
            on_epoch=lambda ep, m: print(
                "Epoch {} , train_step_loss:{:.5f} , train_full_loss:{:.5f} , test_step_loss:{:.5f} , test_full_loss:{:.5f}".format(
                    ep, m["train_step"], m["train_full"], m["test_step"], m["test_full"]), flush=True))
    c = _CONSTANTS[args.driver]
    if args.driver == "velocity_unrolled":
        return harness.fit_velocity_unrolled(
            model, opt, sched, train, test, **common, max_look_ahead=args.max_look_ahead, period=c["period"],
            on_epoch=lambda ep, m: print("Epoch {} , test_step_loss:{:.5f} , look_ahead:{}".format(
                ep, m["test_step"], m["look_ahead"]), flush=True))
    return harness.fit_unrolled_t(
        model, opt, sched, train, test, **common, max_look_ahead=args.max_look_ahead, period=c["period"],
        on_epoch=lambda ep, m: print("Epoch {} , train_step_loss:{:.5f} , test_step_loss:{:.5f} , look_ahead:{}".format(
            ep, m["train_step"], m["test_step"], m["look_ahead"]), flush=True))


def main(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
