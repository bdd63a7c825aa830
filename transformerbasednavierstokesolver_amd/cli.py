"""What the command lines train.py, train_sequence.py and train_slices.py share: the two-stage parse, the flag core of the
eight reference parsers that have one, and the pieces every `run_*` is put together from (device, data file, checkpoint
path, optimizer and schedule, the lines printed before a run, loading a checkpoint).  The flags themselves are documented
in the three modules' docstrings."""
from __future__ import annotations

import argparse
import os

NS_FILE = "NavierStokes_V1e-5_N1200_T20"


def parse(argv, drivers, build, **driver_flag):
    """Read `--driver` (`driver_flag`: default=... or required=True), then parse `argv` with that driver's own table
    `build(driver)`.  Returns (parser, args)."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--driver", choices=drivers, **driver_flag)
    parser = build(pre.parse_known_args(argv)[0].driver)
    return parser, parser.parse_args(argv)


def add_core_flags(p, *, epochs, gpu, save_name, downsample, model="Transolver_2D", data_path="/data/fno", ntrain=None):
    """`--lr` .. `--data_path` of exp_ns.py, ns_vorticity_unrolling.py, exp_darcy.py, exp_airfoil.py, exp_pipe.py,
    exp_elas.py, exp_plas.py and auto_encoder.py, in their order, with the defaults they differ in.  `downsample` None:
    `--downsamplex` / `--downsampley` in its place.  `ntrain` None: no `--ntrain` between `--dropout` and `--unified_pos`."""
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--epochs", type=int, default=epochs)
    p.add_argument("--weight_decay", type=float, default=1e-5)
    p.add_argument("--model", type=str, default=model)
    p.add_argument("--n-hidden", type=int, default=64, help="hidden dim")
    p.add_argument("--n-layers", type=int, default=3, help="layers")
    p.add_argument("--n-heads", type=int, default=4)
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--gpu", type=str, default=gpu, help="GPU index to use")
    p.add_argument("--max_grad_norm", type=float, default=None)
    if downsample is None:
        p.add_argument("--downsamplex", type=int, default=1)
        p.add_argument("--downsampley", type=int, default=1)
    else:
        p.add_argument("--downsample", type=int, default=downsample)
    p.add_argument("--mlp_ratio", type=int, default=1)
    p.add_argument("--dropout", type=float, default=0.0)
    if ntrain is not None:
        p.add_argument("--ntrain", type=int, default=ntrain)
    p.add_argument("--unified_pos", type=int, default=0)
    p.add_argument("--ref", type=int, default=8)
    p.add_argument("--slice_num", type=int, default=32)
    p.add_argument("--eval", type=int, default=0)
    p.add_argument("--save_name", type=str, default=save_name)
    p.add_argument("--data_path", type=str, default=data_path)


def add_driver_flags(p, drivers, driver, engines="f32 | split | bf16"):
    """`--driver` and `--engine`: in no reference parser."""
    p.add_argument("--driver", choices=drivers, default=driver)
    p.add_argument("--engine", type=str, default=None, help="GEMM engine: " + engines)


def device(args):
    import torch
    idx = int(args.gpu)
    if not torch.cuda.is_available() or idx >= torch.cuda.device_count():
        raise SystemExit(f"--gpu {args.gpu}: no such GPU ({torch.cuda.device_count()} visible); this package has no CPU path")
    torch.cuda.set_device(idx)
    return torch.device("cuda", idx)


def find(data_path, names):
    if os.path.isfile(data_path):
        return data_path
    for n in names:
        if os.path.isfile(os.path.join(data_path, n)):
            return os.path.join(data_path, n)
    raise FileNotFoundError(f"none of {list(names)} under --data_path {data_path}")


def ns_mat_file(args):
    return find(args.data_path, (NS_FILE + ".mat", os.path.join(NS_FILE, NS_FILE + ".mat")))


def ns_mat(args):
    """The array `u` of the Navier-Stokes file under --data_path."""
    import scipy.io as scio
    return scio.loadmat(ns_mat_file(args))["u"]


def checkpoint(folder, args):
    return os.path.join(folder, args.save_name + ".pt")


def optim(model, lr, weight_decay, epochs, steps_per_epoch, clip=None):
    """(FusedAdamW with the clip threshold inside it, its schedule): OneCycleLR over epochs * steps_per_epoch steps; with
    `steps_per_epoch` None the schedule that is stepped once per epoch, CosineAnnealingLR(T_max=epochs)."""
    import torch
    from .optim import FusedAdamW
    opt = FusedAdamW(model.parameters(), lr=lr, weight_decay=weight_decay, max_grad_norm=clip)
    if steps_per_epoch is None:
        return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs)
    return opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, epochs=epochs, steps_per_epoch=steps_per_epoch)


def describe(args, model=None):
    print(args)
    if model is not None:
        print(f"Total Trainable Params: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")


def load_state(model, path, dev, strict):
    import torch
    model.load_state_dict(torch.load(path, map_location=dev, weights_only=True), strict=strict)


def model_kwargs(args, fun_dim, **mesh):
    """The keywords of the reference models that take the whole flag core; `mesh`: H / W of a structured one."""
    return dict(space_dim=2, n_layers=args.n_layers, n_hidden=args.n_hidden, dropout=args.dropout, n_head=args.n_heads,
                Time_Input=False, mlp_ratio=args.mlp_ratio, fun_dim=fun_dim, out_dim=1, slice_num=args.slice_num,
                ref=args.ref, unified_pos=args.unified_pos, **mesh)


def set_engine(args, *models):
    if args.engine is not None:
        for model in models:
            model.set_engine(args.engine)
