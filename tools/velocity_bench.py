"""Time one training iteration and one test pass of the three velocity-field loops, on ONE GPU.

    python tools/velocity_bench.py [--cases velocity,velocity_unrolled,unrolled_t] [--look_ahead 2] [--iters 10]
                                   [--repeats 7] [--warmup 3] [--out FILE.json]

The sizes are the fork's own (ns_velocity.ipynb): 64 x 64 points, C = 64, 4 heads, M = 32 slices, 8 layers,
batch 4, step = 2; T_in = T = 10 for `velocity` and `unrolled_t`, 20 for `velocity_unrolled`, as the scripts have them.  Data:
`synth.velocity_fields` (seeded; timing does not depend on the values).  optim.FusedAdamW, OneCycleLR, FusedTestLoss.

Per case, in ONE process on the same card, alternating window by window (tools/graphed_step_bench.py's protocol:
`--warmup` calls of each mode, then `--repeats` timed windows of `--iters` calls per mode, each closed by a device
synchronisation; reported: the median window and its spread, in ms per call):
  * iteration: eager (the loops' own eager iteration) against graphed (the whole iteration with its optimizer step from one
    hipGraph), at `--look_ahead` chained calls for the two SOL loops;
  * test pass of one batch: the torch loop (model call, loss on the reshaped target copy, torch.cat window shift, the full
    loss on the concatenated prediction for `velocity`) against `harness.scored_rollout` (one fused tail launch per step)
    against `harness.GraphedScoredRollout` (the whole rollout from one hipGraph).
Before anything is timed the graphed results are compared with the eager ones bit for bit, and the scored rollout's sums with
the torch loop's (reported as `check`).  Prints one JSON line; there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from transformerbasednavierstokesolver_amd import harness, synth  # noqa: E402
from transformerbasednavierstokesolver_amd.model import Transolver_Structured_Mesh_2D  # noqa: E402
from transformerbasednavierstokesolver_amd.model.SOL_Transolver_Structured_Mesh_2D import SOL_Transolver_Structured_Mesh_2D  # noqa: E402
from transformerbasednavierstokesolver_amd.optim import FusedAdamW  # noqa: E402
from transformerbasednavierstokesolver_amd.utils.testloss import FusedTestLoss  # noqa: E402

MODEL = dict(space_dim=2, n_layers=8, n_hidden=64, dropout=0.0, n_head=4, Time_Input=False, mlp_ratio=1, out_dim=2,
             slice_num=32, ref=8, unified_pos=0, H=64, W=64)
CASES = {"velocity": dict(T=10), "velocity_unrolled": dict(T=20), "unrolled_t": dict(T=10)}
BATCH, STEP, LR, WD = 4, 2, 1e-3, 1e-5


def build(case, dev, look_ahead):
    T = CASES[case]["T"]
    arr = torch.from_numpy(synth.velocity_fields(BATCH, 64, 64, frames=T, seed=3)).reshape(BATCH, 64 * 64, 2 * T).to(dev)
    fx, yy = arr[..., :T].contiguous(), arr[..., T:].contiguous()
    x = torch.from_numpy(synth.meshgrid_pos(BATCH, 64, 64)).to(dev)
    if case == "velocity":
        module = inner = Transolver_Structured_Mesh_2D.Model(**MODEL, fun_dim=T).to(dev)
    else:
        module = SOL_Transolver_Structured_Mesh_2D(**MODEL, fun_dim=T, step=STEP, look_ahead=look_ahead).to(dev)
        inner = module.transolver_model
    opt = FusedAdamW(module.parameters(), lr=LR, weight_decay=WD)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=1_000_000)
    loss_fn = FusedTestLoss(size_average=False)
    if case == "velocity":
        forward = lambda key, a, b, c, vals: harness.velocity_iteration(module, a, b, c, STEP, loss_fn, vals)
        nparts = 2
    else:
        it = harness.unrolled_window_iteration if case == "velocity_unrolled" else harness.unrolled_t_iteration
        forward = lambda key, a, b, c, vals: (it(module, a, b, c, key, STEP, loss_fn, vals),)
        nparts = 1
    runs = {mode: harness._velocity_runner(module, opt, sched, BATCH, mode == "graphed", None, None, None, forward, nparts,
                                           dict(set_to_none=False))
            for mode in ("eager", "graphed")}
    key = 0 if case == "velocity" else look_ahead
    train = {mode: (lambda run=run: run(key, x, fx, yy)) for mode, run in runs.items()}
    graphs = {}

    def test_pass(fused, graphed):
        def run():
            acc = torch.zeros(4, dtype=torch.float64, device=dev)
            harness._rollout_test_pass(inner, _OneBatch(x, fx, yy), BATCH, T, STEP, loss_fn, acc, case == "velocity", fused,
                                       None, graphed, graphs)
            return acc
        return run

    return module, opt, train, dict(torch_loop=test_pass(False, False), scored=test_pass(True, False),
                                    graphed=test_pass(True, True))


class _OneBatch:
    def __init__(self, *tensors):
        self.tensors = tensors

    def batches(self, batch_size):
        yield self.tensors


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


def alternate(modes, warmup, repeats, iters):
    for fn in modes.values():
        window(fn, warmup)
    ms = {k: [] for k in modes}
    for _ in range(repeats):
        for k, fn in modes.items():          # alternating: every mode sees the same neighbours on the card
            ms[k].append(window(fn, iters))
    return {k: summary(v) for k, v in ms.items()}


def check(case, dev, look_ahead):
    """Results before times: two fresh builds, three iterations each, eager against graphed bit for bit; the test passes
    against each other."""
    finals = []
    for mode in ("eager", "graphed"):
        torch.manual_seed(0)
        module, opt, train, _ = build(case, dev, look_ahead)
        module.train()
        losses = [float(train[mode]()[0]) for _ in range(3)]
        finals.append((losses, opt.flat_p.clone()))
    module.eval()
    _, _, _, tests = build(case, dev, look_ahead)
    a, b, c = (tests[k]().tolist() for k in ("torch_loop", "scored", "graphed"))
    rel = max(abs(p - q) / abs(p) for p, q in zip(a[2:], b[2:]) if p)
    return dict(iteration_bit_identical=finals[0][0] == finals[1][0] and bool(torch.equal(finals[0][1], finals[1][1])),
                graphed_rollout_bit_identical=b == c, scored_vs_torch_loop_rel=rel)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--look_ahead", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("velocity_bench needs a GPU: a CPU run cannot give a time")
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, repeats=args.repeats, batch=BATCH, step=STEP,
               model=MODEL, look_ahead=args.look_ahead, cases={})
    for case in args.cases.split(","):
        rec = dict(T=CASES[case]["T"], check=check(case, dev, args.look_ahead))
        torch.manual_seed(0)
        module, opt, train, tests = build(case, dev, args.look_ahead)
        module.train()
        rec["iteration"] = alternate(train, args.warmup, args.repeats, args.iters)
        module.eval()
        rec["test_pass"] = alternate(tests, args.warmup, args.repeats, args.iters)
        rec["iteration_speedup_median"] = round(rec["iteration"]["eager"]["median_ms"] / rec["iteration"]["graphed"]["median_ms"], 3)
        tp = rec["test_pass"]
        rec["scored_speedup_median"] = round(tp["torch_loop"]["median_ms"] / tp["scored"]["median_ms"], 3)
        rec["graphed_rollout_speedup_median"] = round(tp["torch_loop"]["median_ms"] / tp["graphed"]["median_ms"], 3)
        out["cases"][case] = rec
        print(case, json.dumps(rec), file=sys.stderr, flush=True)
        del module, opt, train, tests
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
