"""A/B of the fused block tail (Model.set_fused_tail) on graph-captured rollouts, on ONE GPU.

    python tools/fused_tail_bench.py [--batches 1,32] [--repeats 7] [--steps 20] [--panel 16|32] [--out FILE.json]

The bench model (BASELINE configs[1]: 64 x 64 mesh, 8 layers, C = 256, 8 heads, M = 64, synthetic weights) at each batch
size: one harness.GraphedRollout per route (fused off = the default path, fused on), captured once, then `--repeats` timed
`--steps`-step rollouts per route, the two routes ALTERNATING rollout by rollout in the same process on the same card (as
bench.py's rollout leg times its rollouts: one `run(fx, steps)` closed by a device synchronisation).  Reported per batch
and route: median, min and max in steps/s; whether the fused median lies outside the default route's measured range;
library calls (`_lib.check`ed entry points) and device kernels (torch.profiler; "null" where it reports none) of one
eager model call; and the largest per-sample rel-L2 between the two routes' final frames.
--panel forces the tail's panel height for the whole process (PA2D_TAIL_PANEL, read when the library loads).
Prints one JSON line; there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_run(gr, fx, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = gr.run(fx, steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(secs, steps):
    s = sorted(steps / t for t in secs)
    return dict(median_steps_per_s=round(s[len(s) // 2], 2), min_steps_per_s=round(s[0], 2), max_steps_per_s=round(s[-1], 2),
                rollouts=len(s))


def count_calls(model, x, fx, flag):
    """(library calls, device kernels or None) of one eager no-grad model call on the given route."""
    import torch
    from transformerbasednavierstokesolver_amd import _lib, ops
    n = [0]
    real = _lib.check

    def counting(rc, what):
        n[0] += 1
        return real(rc, what)

    model.set_fused_tail(flag)
    kernels = None
    try:
        with torch.no_grad(), ops.weights_frozen():
            model(x, fx=fx)                      # packs and images made: the counted call is a steady-state step
            _lib.check = counting
            model(x, fx=fx)
            _lib.check = real
            try:
                from torch.profiler import ProfilerActivity, profile
                torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    model(x, fx=fx)
                    torch.cuda.synchronize()
                ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                      and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
                kernels = len(ev) or None
            except Exception as exc:      # a measurement that could not be taken is reported as such, never guessed
                print(f"kernel count not measured: {exc!r}", file=sys.stderr)
    finally:
        _lib.check = real
        model.set_fused_tail(False)
    return n[0], kernels


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--panel", choices=("16", "32"), default=None)
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.panel:
        os.environ["PA2D_TAIL_PANEL"] = args.panel      # before the library is loaded
    import torch
    from transformerbasednavierstokesolver_amd import harness, synth
    if not torch.cuda.is_available():
        raise SystemExit("fused_tail_bench needs a GPU: a CPU run cannot give a time")
    if args.repeats < 7:
        print("fewer than 7 repeats: the range is too thin to call a difference", file=sys.stderr)
    cfg = synth.NS_CONFIG
    model = harness.build_model(cfg, synth.synth_state_dict(cfg, seed=0), "cuda").eval()
    out = dict(device=torch.cuda.get_device_name(0), steps=args.steps, repeats=args.repeats,
               panel=args.panel or "auto", batches={})
    for bsz in (int(b) for b in args.batches.split(",")):
        pos, a, _ = synth.ns_batch(bsz, seed=5)
        x, fx = torch.from_numpy(pos).cuda(), torch.from_numpy(a).cuda()
        routes = {"off": harness.GraphedRollout(model, x, fx, fused_tail=False),
                  "on": harness.GraphedRollout(model, x, fx, fused_tail=True)}
        last = {}
        for k, gr in routes.items():
            gr.run(fx, 2)
        secs = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, gr in routes.items():          # alternating: both routes see the same neighbours on the card
                dt, frames = timed_run(gr, fx, args.steps)
                secs[k].append(dt)
                last[k] = frames
        rec = {k: summary(v, args.steps) for k, v in secs.items()}
        fin = lambda t: t[..., -1].reshape(bsz, -1).double()
        rel = (fin(last["on"]) - fin(last["off"])).norm(dim=1) / fin(last["off"]).norm(dim=1)
        rec["max_row_rel_l2_final_frame"] = float(rel.max())
        rec["fused_median_outside_default_range"] = not (rec["off"]["min_steps_per_s"] <= rec["on"]["median_steps_per_s"]
                                                         <= rec["off"]["max_steps_per_s"])
        rec["speedup_median"] = round(rec["on"]["median_steps_per_s"] / rec["off"]["median_steps_per_s"], 3)
        if not args.no_counts:
            for k, flag in (("off", False), ("on", True)):
                calls, kernels = count_calls(model, x, fx, flag)
                rec[k]["library_calls_per_step"], rec[k]["kernels_per_step"] = calls, kernels
        out["batches"][f"b{bsz}"] = rec
        print(f"b{bsz}", json.dumps(rec), file=sys.stderr, flush=True)
        del routes
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
