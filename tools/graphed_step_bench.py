"""Time one training iteration of the five one-call drivers, eager and replayed from a hipGraph, on ONE GPU.

    python tools/graphed_step_bench.py [--mode both|eager|graphed] [--cases darcy,airfoil,pipe,elas,plas]
                                       [--iters 10] [--repeats 7] [--warmup 5] [--out FILE.json]

The configurations are the reference's scripts/Transolver_{Darcy,Airfoil,Pipe,Elas,Plas}.sh (8 layers, C = 128, 8 heads,
64 slices, clip 0.1; pipe mlp_ratio 2; Darcy unified_pos with ref 8): Darcy 85 x 85 at batch 4, airfoil 221 x 51 at batch 4,
pipe 129 x 129 at batch 8, elasticity 972 points at batch 1, plasticity 101 x 31 at batch 8 with its 20 optimizer steps per
batch.  Seeded random data of those shapes (timing does not depend on the values), optim.FusedAdamW with the clip inside,
OneCycleLR stepped where the drivers step it, the fused losses train.py uses.

Protocol (as bench.py's legs): `--warmup` iterations of each mode, then `--repeats` timed windows of `--iters` iterations
per mode, the two modes ALTERNATING window by window in the same process on the same card, each window closed by a device
synchronisation; reported: the median window, and the spread (min .. max), in ms per iteration.  Eager = the step
functions of harness.py (darcy_train_step / static_train_step / plas_train_step + scheduler), graphed =
harness.GraphedCallStep as fit_* use it.  `--mode eager` needs nothing newer than those step functions.
Kernel launches per iteration are counted from one profiled eager iteration AFTER the timed windows (torch.profiler
device events); "not measured" where the profiler gives none.  Prints one JSON line; there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from transformerbasednavierstokesolver_amd import harness  # noqa: E402
from transformerbasednavierstokesolver_amd.model import Transolver_Irregular_Mesh, Transolver_Structured_Mesh_2D  # noqa: E402
from transformerbasednavierstokesolver_amd.optim import FusedAdamW  # noqa: E402
from transformerbasednavierstokesolver_amd.utils.normalizer import UnitTransformer  # noqa: E402
from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss  # noqa: E402

COMMON = dict(space_dim=2, n_layers=8, n_hidden=128, dropout=0.0, n_head=8, slice_num=64, ref=8)
CASES = {
    "darcy": dict(H=85, W=85, batch=4, model=dict(fun_dim=1, out_dim=1, mlp_ratio=1, unified_pos=1, Time_Input=False)),
    "airfoil": dict(H=221, W=51, batch=4, model=dict(fun_dim=0, out_dim=1, mlp_ratio=1, unified_pos=0, Time_Input=False)),
    "pipe": dict(H=129, W=129, batch=8, model=dict(fun_dim=0, out_dim=1, mlp_ratio=2, unified_pos=0, Time_Input=False)),
    "elas": dict(N=972, batch=1, model=dict(fun_dim=0, out_dim=1, mlp_ratio=1, unified_pos=0, Time_Input=False)),
    "plas": dict(H=101, W=31, batch=8, T=20, model=dict(fun_dim=1, out_dim=4, mlp_ratio=1, unified_pos=0, Time_Input=True)),
}
CLIP, LR, WD = 0.1, 1e-3, 1e-5


def build(case, dev, seed=0):
    """(model, optimizer, scheduler, eager(), make_graphed() -> graphed()) of one case; one call = one ITERATION (plas: T
    optimizer steps and one scheduler step)."""
    c = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    B = c["batch"]
    if case == "elas":
        model = Transolver_Irregular_Mesh.Model(**COMMON, **c["model"]).to(dev)
        N = c["N"]
    else:
        model = Transolver_Structured_Mesh_2D.Model(**COMMON, **c["model"], H=c["H"], W=c["W"]).to(dev)
        N = c["H"] * c["W"]
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=CLIP)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=1_000_000)
    loss_fn = FusedTestLoss(size_average=False)
    x = torch.rand(B, N, 2, generator=gen).to(dev)
    if case == "darcy":
        fx, y, s = rnd(B, N), rnd(B, N), c["H"]
        yn = UnitTransformer(torch.randn(16, N, generator=gen)).to(dev)
        dx = 1.0 / s

        def eager():
            harness.darcy_train_step(model, opt, sched, x, fx, y, yn, dx, s, fused=True)

        def make_graphed():
            step = harness.GraphedCallStep(model, opt, sched, (x, fx.clone(), y.clone()), harness._darcy_body(yn, dx, s))
            return lambda: step(None, fx, y)
    elif case == "plas":
        T = c["T"]
        fx, yy = rnd(B, N, 1), rnd(B, N, 4, T)
        tim = torch.rand(B, T, generator=gen).to(dev)

        def eager():
            harness.plas_train_step(model, opt, x, fx, tim, yy, loss_fn=loss_fn)
            sched.step()

        def make_graphed():
            step = harness.GraphedCallStep(model, opt, None, (x, fx.clone(), tim[:, :1].clone(), yy.clone()),
                                           harness._plas_body(loss_fn))

            def run():
                step.static[1].copy_(fx)
                for k in range(T):
                    step.static[3][..., 0].copy_(yy[..., k])
                    step(None, None, tim[:, k:k + 1], None)
                sched.step()
            return run
    else:
        y = rnd(B, N)
        yn = None if case == "airfoil" else UnitTransformer(torch.randn(16, N, generator=gen)).to(dev)

        def eager():
            harness.static_train_step(model, opt, sched, x, y, yn, loss_fn=loss_fn)

        def make_graphed():
            step = harness.GraphedCallStep(model, opt, sched, (x.clone(), y.clone()), harness._static_body(loss_fn, yn))
            return lambda: step(x, y)
    return model, opt, eager, make_graphed


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def summary(ms):
    s = sorted(ms)
    return dict(median_ms=round(s[len(s) // 2], 4), min_ms=round(s[0], 4), max_ms=round(s[-1], 4), windows=len(s))


def count_launches(fn):
    """Device kernel events of one eager iteration (None if the profiler reports none on this build)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(kernels) or None
    except Exception as exc:      # a measurement that could not be taken is reported as such, never guessed
        print(f"launch count not measured: {exc!r}", file=sys.stderr)
        return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("both", "eager", "graphed"), default="both")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("graphed_step_bench needs a GPU: a CPU run cannot give a time")
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), mode=args.mode, iters=args.iters, repeats=args.repeats, cases={})
    for case in args.cases.split(","):
        iters = max(1, args.iters // 4) if case == "plas" else args.iters        # a plas iteration is 20 steps
        model, opt, eager, make_graphed = build(case, dev)
        model.train()
        modes = {}
        if args.mode in ("both", "eager"):
            modes["eager"] = eager
        if args.mode in ("both", "graphed"):
            modes["graphed"] = make_graphed()
        for fn in modes.values():
            window(fn, args.warmup)
        ms = {k: [] for k in modes}
        for _ in range(args.repeats):
            for k, fn in modes.items():          # alternating: both modes see the same neighbours on the card
                ms[k].append(window(fn, iters))
        rec = {k: summary(v) for k, v in ms.items()}
        rec["iters_per_window"] = iters
        rec["steps_per_iteration"] = CASES[case].get("T", 1)
        if not args.no_launch_count and "eager" in modes:
            rec["kernel_launches_per_iteration"] = count_launches(eager)
        if "eager" in rec and "graphed" in rec:
            rec["speedup_median"] = round(rec["eager"]["median_ms"] / rec["graphed"]["median_ms"], 3)
        rec["optimizer_steps"] = opt.steps
        out["cases"][case] = rec
        print(case, json.dumps(rec), file=sys.stderr, flush=True)
        del model, opt, eager, make_graphed, modes
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
