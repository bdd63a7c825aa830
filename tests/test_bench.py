"""bench.py's result line and `--dump-outputs`: the file set, dtypes and size cap on the host; the timed step count,
ms_per_step and the dump of a real run on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_dump_outputs_writes_float32_arrays_of_the_last_step(tmp_path):
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(1024, 1024), torch.nn.Linear(1024, 7))     # 1.06 M > DUMP_MAX_GRADS
    m.unused = torch.nn.Parameter(torch.ones(3))                    # no gradient: zeros in grads.npy
    m(torch.randn(4, 1024)).square().sum().backward()
    loss, full = torch.tensor(1.5), torch.tensor(2.5, dtype=torch.float64)
    shapes = bench.dump_outputs(str(tmp_path / "a"), m, loss, full)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"loss", "full_loss", "params", "grads"} and all(a.dtype == np.float32 for a in got.values())
    assert shapes == {k: list(a.shape) for k, a in got.items()}
    assert float(got["loss"]) == 1.5 and float(got["full_loss"]) == 2.5
    ps = list(m.parameters())
    want_p = torch.cat([p.detach().reshape(-1) for p in ps]).numpy()
    assert np.array_equal(got["params"], want_p)                    # below the cap: every parameter, in order
    assert got["params"].size == sum(p.numel() for p in ps) < bench.DUMP_MAX_PARAMS
    assert got["grads"].size == bench.DUMP_MAX_GRADS < want_p.size  # above the cap: a sample ...
    want_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ps]).numpy()
    assert np.isin(got["grads"], want_g).all()
    bench.dump_outputs(str(tmp_path / "b"), m, loss, full)
    assert np.array_equal(np.load(tmp_path / "b" / "grads.npy"), got["grads"])      # ... the same one every run
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6


def test_seeded_sample_is_fixed_sorted_and_bounded():
    import bench
    x = np.arange(1000, dtype=np.float32)
    assert bench.seeded_sample(x, 1000, seed=3) is x
    s = bench.seeded_sample(x, 100, seed=3)
    assert s.size == 100 and np.all(np.diff(s) > 0) and np.array_equal(s, bench.seeded_sample(x, 100, seed=3))


@pytest.mark.gpu
def test_bench_times_the_requested_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch-per-gpu", "2", "--no-cpu-baseline", "--no-rollout", "--no-folded-leg", "--no-exact-leg",
                        "--no-darcy-leg", "--no-bf16-leg", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) < 1e-2 * rec["value"]
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"loss", "full_loss", "params", "grads"} and all(a.dtype == np.float32 for a in got.values())
    assert all(np.isfinite(a).all() for a in got.values())
    assert got["params"].size == 11240769 and got["grads"].size == 2 ** 20      # NS_CONFIG: every parameter
    # the loss the result line reports is the dumped loss of the last step
    assert abs(float(got["loss"]) / 2 / 10 - rec["final_loss_per_sample_call"]) < 1e-5


# what only `--full` measures: the secondary legs and the CPU baseline, at --batch-per-gpu 2
FULL_ONLY_KEYS = {"time_folded", "fp32_exact_engine", "rollout_steps_per_s_b2", "rollout_steps_per_s_b1", "rollout_sample",
                  "darcy421", "bf16_storage", "cpu_baseline", "rel_l2_gpu_vs_cpu_oracle"}


def test_plain_run_makes_no_secondary_measurement():
    import bench
    from transformerbasednavierstokesolver_amd import ops
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False
    for engine in (ops.ENGINE_F32, ops.ENGINE_SPLIT, ops.ENGINE_BF16, ops.ENGINE_BF16S):
        assert bench.secondary_legs(plain, engine, 1) == set() and bench.secondary_legs(plain, engine, 2) == set()


def test_full_run_keeps_every_leg_its_options_leave():
    import bench
    from transformerbasednavierstokesolver_amd import ops
    every = {"folded", "exact", "rollout", "darcy", "bf16", "cpu"}
    full = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full is True
    assert bench.secondary_legs(full, ops.ENGINE_SPLIT, 1) == every
    assert bench.secondary_legs(full, ops.ENGINE_SPLIT, 2) == every - {"cpu"}             # CPU baseline: N = 1 only
    assert bench.secondary_legs(full, ops.ENGINE_F32, 1) == every - {"exact"}              # the headline is that engine
    assert bench.secondary_legs(full, ops.ENGINE_BF16S, 1) == every - {"bf16"}
    for opt, leg in (("--no-folded-leg", "folded"), ("--no-exact-leg", "exact"), ("--no-split-leg", "exact"),
                     ("--no-rollout", "rollout"), ("--no-darcy-leg", "darcy"), ("--no-bf16-leg", "bf16"),
                     ("--no-cpu-baseline", "cpu")):
        assert bench.secondary_legs(bench.parse_args(["--full", opt]), ops.ENGINE_SPLIT, 1) == every - {leg}, opt
    for loop in ("--graph", "--fold-time"):        # legs compared with the default loop need that loop
        assert bench.secondary_legs(bench.parse_args(["--full", loop]), ops.ENGINE_SPLIT, 1) == {"rollout", "darcy", "cpu"}


def _bench_line(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone_and_full_run_adds_the_legs():
    base = ["--gpus", "1", "--steps", "1", "--warmup", "1", "--batch-per-gpu", "2"]
    plain = _bench_line(base)
    assert plain["full"] is False and not FULL_ONLY_KEYS & set(plain), sorted(FULL_ONLY_KEYS & set(plain))
    assert plain["steps"] == 1 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    # the rooflines come from HIP events inside the timed steps themselves: a plain run keeps them
    assert plain["roofline"]["launches_timed"] > 0 and plain["roofline_hbm"]["kernels"]
    full = _bench_line(base + ["--full", "--cpu-batch", "1", "--cpu-iters", "1", "--rollout-repeats", "1"])
    assert full["full"] is True and FULL_ONLY_KEYS <= set(full), sorted(FULL_ONLY_KEYS - set(full))
    assert full["steps"] == 1 and full["warmup"] == 1
    assert full["rel_l2_gpu_vs_cpu_oracle"] < 1e-4
