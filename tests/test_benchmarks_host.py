"""The airfoil / pipe / elasticity / plasticity drivers without a GPU (fixtures G17-G20, tools/make_golden_benchmarks.py):

  * every loader (data.load_airfoil_npy / load_pipe_npy / load_elas_npy / load_plas_mat) on the seeded synthetic files
    written to tmp_path, against an explicit construction from the arrays;
  * train.py's four new parser tables against the parsers the reference scripts built (`parser.*` of the fixtures), and
    the unchanged tables of the three older drivers;
  * the four new C-ABI symbols: exported, and bound with the arity include/pa2d.h declares;
  * harness.fit_static / fit_plas with the fp64 oracle wrapped as an nn.Module (tests/benchmark_restatement.py) and a stock
    torch.optim.AdamW on the CPU: every recorded loss call and epoch metric of the reference's own main() within
    max(1e-6 relative, 4 x the fixture's own deviation), every final parameter tensor within max(1e-5, 4 x its own
    deviation) rel-L2 (the bounds of tests/test_drivers_host.py).  That pins the short last batch, the decoded training
    loss against the raw test target, the per-epoch cosine schedule of exp_elas, the per-batch schedule and the T
    optimizer steps of exp_plas, and the replay of its time permutations."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import benchmark_restatement as br
import driver_restatement as dr
from conftest import ROOT
from transformerbasednavierstokesolver_amd import data, harness, train
from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss

CALL_FLOOR, PARAM_FLOOR = 1e-6, 1e-5
NEW_SYMBOLS = ("pa2d_rel_l2_affine_fwd", "pa2d_rel_l2_affine_bwd", "pa2d_embed_bias_fwd", "pa2d_embed_bias_bwd")


# ------------------------------------------------------------------------------------------------------------ loaders
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _unit(x):
    return x.mean(dim=(0, 1), keepdim=True), x.std(dim=(0, 1), keepdim=True) + 1e-8


def test_load_airfoil_npy(tmp_path):
    f = br.file_arrays("airfoil")
    path = br.write_files("airfoil", str(tmp_path))
    d = data.load_airfoil_npy(path, 1000, 200, 20, 10)
    rows, cols = list(range(0, 221, 20)), list(range(0, 51, 10))
    assert (d["s1"], d["s2"]) == (12, 6) == (len(rows), len(cols))
    X, Y, q = (torch.from_numpy(a) for a in (f["NACA_Cylinder_X.npy"], f["NACA_Cylinder_Y.npy"], f["NACA_Cylinder_Q.npy"][:, 4]))
    pick = lambda t, lo, hi: t[lo:hi][:, rows][:, :, cols]
    assert _same(d["x_train"], torch.stack([pick(X, 0, 1000), pick(Y, 0, 1000)], -1).reshape(1000, 72, 2))
    assert _same(d["y_train"], pick(q, 0, 1000).reshape(1000, 72))
    assert _same(d["x_test"], torch.stack([pick(X, 1000, 1200), pick(Y, 1000, 1200)], -1).reshape(200, 72, 2))
    assert _same(d["y_test"], pick(q, 1000, 1200).reshape(200, 72))
    assert d["x_normalizer"] is None and d["y_normalizer"] is None
    full = data.load_airfoil_npy(path, 5, 3)                       # the defaults: the whole 221 x 51 mesh
    assert (full["s1"], full["s2"]) == (221, 51) and _same(full["y_test"], q[5:8].reshape(3, 221 * 51))


def test_load_pipe_npy(tmp_path):
    f = br.file_arrays("pipe")
    path = br.write_files("pipe", str(tmp_path))
    d = data.load_pipe_npy(path, 1000, 200, 16, 16)
    idx = list(range(0, 129, 16))
    assert (d["s1"], d["s2"]) == (9, 9) and f["Pipe_X.npy"].shape[0] == 1210       # 10 samples past the script's N = 1200
    X, Y, q = (torch.from_numpy(a) for a in (f["Pipe_X.npy"], f["Pipe_Y.npy"], f["Pipe_Q.npy"][:, 0]))
    pick = lambda t, lo, hi: t[lo:hi][:, idx][:, :, idx]
    x_train = torch.stack([pick(X, 0, 1000), pick(Y, 0, 1000)], -1).reshape(1000, 81, 2)
    x_test = torch.stack([pick(X, 1000, 1200), pick(Y, 1000, 1200)], -1).reshape(200, 81, 2)     # the last 200 of the first 1200
    y_train, y_test = pick(q, 0, 1000).reshape(1000, 81), pick(q, 1000, 1200).reshape(200, 81)
    (xm, xs), (ym, ys) = _unit(x_train), _unit(y_train)
    assert xm.shape == (1, 1, 2) and ym.numel() == 1
    assert _same(d["x_normalizer"].mean, xm) and _same(d["x_normalizer"].std, xs)
    assert _same(d["y_normalizer"].mean, ym) and _same(d["y_normalizer"].std, ys)
    assert _same(d["x_train"], (x_train - xm) / xs) and _same(d["x_test"], (x_test - xm) / xs)
    assert _same(d["y_train"], (y_train - ym) / ys)
    assert _same(d["y_test"], y_test)                              # RAW: never encoded


def test_load_elas_npy(tmp_path):
    f = br.file_arrays("elas")
    path = br.write_files("elas", str(tmp_path))
    assert os.path.isfile(os.path.join(path, "elasticity", "Meshes", "Random_UnitCell_XY_10.npy"))
    d = data.load_elas_npy(path, 40, 200)
    s = torch.from_numpy(f["Random_UnitCell_sigma_10.npy"]).permute(1, 0)           # [samples, points]
    xy = torch.from_numpy(f["Random_UnitCell_XY_10.npy"]).permute(2, 0, 1)          # [samples, points, 2]
    assert s.shape == (245, 50) and xy.shape == (245, 50, 2)
    ym, ys = _unit(s[:40])
    assert _same(d["x_train"], xy[:40]) and _same(d["x_test"], xy[45:])             # the LAST 200, coordinates raw
    assert _same(d["y_train"], (s[:40] - ym) / ys) and _same(d["y_test"], s[45:])   # the test target RAW
    assert d["x_normalizer"] is None and _same(d["y_normalizer"].mean, ym) and d["s1"] is None


def test_load_plas_mat(tmp_path):
    """On a 12-sample file (7 train, the last 4 test), and the fixture's data through the same code."""
    f = br.plas_small_mat(12)
    path = br.write_files("plas", str(tmp_path))
    d = data.load_plas_mat(path, 7, 4)
    inp, out = torch.from_numpy(f["input"]), torch.from_numpy(f["output"])
    assert (d["s1"], d["s2"], d["T"]) == (101, 31, 20) and out.shape == (12, 101, 31, 20, 4)
    x_train = inp[:7, :, None].expand(7, 101, 31).reshape(7, 3131, 1)              # the die profile along the 31 columns
    x_test = inp[-4:, :, None].expand(4, 101, 31).reshape(4, 3131, 1)
    xm, xs = _unit(x_train)
    assert _same(d["x_train"], (x_train - xm) / xs) and _same(d["x_test"], (x_test - xm) / xs)
    assert d["y_normalizer"] is None and _same(d["x_normalizer"].mean, xm)
    assert _same(d["y_train"], out[:7].permute(0, 1, 2, 4, 3).reshape(7, 3131, 4, 20))           # [..., 4, T], raw
    assert _same(d["y_test"], out[-4:].permute(0, 1, 2, 4, 3).reshape(4, 3131, 4, 20))
    assert _same(d["t"], torch.tensor(np.linspace(0, 1, 20), dtype=torch.float))
    # the script's meshgrid: point k has first coordinate (k % 101) / 100 and second (k // 101) / 30: the 101-axis runs
    # fastest, unlike x and y above (31-axis fastest)
    k = np.arange(3131)
    want = torch.tensor(np.stack([(k % 101) / 100.0, (k // 101) / 30.0], -1), dtype=torch.float)
    assert d["pos"].shape == (1, 3131, 2) and torch.allclose(d["pos"][0], want, rtol=0, atol=1e-7)
    lim = br.load_data("plas")                                   # samples 0..2 and 907, 908 of the 987
    assert _same(lim["y_train"], d["y_train"][:3]) and lim["y_test"].shape == (2, 3131, 4, 20)
    inp_all = torch.from_numpy(br.plas_parts()[0])
    xm, xs = _unit(inp_all[:900, :, None].expand(900, 101, 31).reshape(900, 3131, 1))
    assert _same(lim["x_test"], ((inp_all[907:909, :, None].expand(2, 101, 31).reshape(2, 3131, 1)) - xm) / xs)


def test_synthetic_data_is_what_the_fixtures_were_made_on():
    for case in br.CASES:
        fx = br.Fixture(case)
        sums = br.data_sums(case)
        assert set(sums) == set(fx.settings["data_sums"])
        for k, v in sums.items():
            np.testing.assert_allclose(v, fx.settings["data_sums"][k], rtol=1e-9)
        assert fx.perms == br.permutations(case) and fx.settings["config"] == br.model_config(case)
    assert br.Fixture("plas").time_perms == br.time_permutations()


# ------------------------------------------------------------------------------------------------------------ parsers
@pytest.mark.parametrize("driver", list(br.CASES))
def test_train_parser_has_the_reference_flags_and_defaults(driver):
    recorded = br.Fixture(driver).parser
    ours = {a.dest: a for a in train.build_parser(driver)._actions if a.dest != "help"}
    for flags, dest, default, typ in recorded:
        a = ours[dest]
        assert list(a.option_strings) == flags and a.default == default and getattr(a.type, "__name__", None) == typ, dest
    extra = set(ours) - {r[1] for r in recorded}
    assert extra == {"driver", "engine", "ntest"} | ({"ntrain"} if driver != "elas" else set())
    args = train.parse_args(["--driver", driver])
    assert args.driver == driver and (args.ntrain, args.ntest) == {"airfoil": (1000, 200), "pipe": (1000, 200),
                                                                     "elas": (1000, 200), "plas": (900, 80)}[driver]
    assert hasattr(args, "downsample") == (driver == "elas") and hasattr(args, "downsamplex") == (driver != "elas")


def test_the_older_parsers_keep_their_flags():
    assert train.DRIVERS == ("ns", "unrolled", "darcy", "airfoil", "pipe", "elas", "plas")
    flags = lambda d: sorted(a.dest for a in train.build_parser(d)._actions if a.dest != "help")
    assert flags("ns") == flags("unrolled") == flags("darcy")
    assert "downsamplex" not in flags("ns") and "downsample" in flags("ns")


# ------------------------------------------------------------------------------------------------------------ C ABI
def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "pa2d.h")).read()
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/pa2d.h"
    return len([p for p in m.group(1).split(",") if p.strip()])


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_bound_with_the_headers_arity(name):
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    res, args = _lib.SIGNATURES[name]
    fn = getattr(lib, name)
    assert res is ctypes.c_int and fn.restype is ctypes.c_int and list(fn.argtypes) == list(args)
    assert len(args) == _header_arity(name)
    text = open(os.path.join(ROOT, "include", "pa2d.h")).read()
    assert int(re.search(r"#define PA2D_REL_L2_AFFINE_SPLIT (\d+)", text).group(1)) == _lib.REL_L2_AFFINE_SPLIT
    assert int(re.search(r"#define PA2D_EMBED_BIAS_CHUNKS (\d+)", text).group(1)) == _lib.EMBED_BIAS_CHUNKS


def test_contract_violations_are_refused_before_any_launch():
    """Shape / alignment contracts that need no GPU: a width that is no multiple of 4, a mean without a std."""
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    assert lib.pa2d_embed_bias_fwd(0, 0, 0, 0, 1, 2, 6, 0) == 1002
    assert lib.pa2d_embed_bias_bwd(0, 0, 0, 0, 0, 1, 2, 6, 0) == 1002
    assert lib.pa2d_embed_bias_fwd(0, 0, 0, 0, 0, 5, 8, 0) == 0                   # B = 0: nothing to do
    assert lib.pa2d_rel_l2_affine_fwd(0, 0, 1, 4, 16, 0, 0, 0, 0, 0, 0, 2, 4, 0) == 1001
    assert lib.pa2d_rel_l2_affine_fwd(0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0) == 0     # B = 0
    assert lib.pa2d_rel_l2_affine_bwd(0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0) == 0        # L = 0


# ------------------------------------------------------------------------------------------------------------ loops
def _adamw(model, case):
    a = br.parse_argv(br.CASES[case]["argv"])
    opt = torch.optim.AdamW(model.parameters(), lr=a["lr"], weight_decay=a["weight_decay"])
    return a, opt, br.scheduler(opt, case)


def _check(case, fx, rec, history, model):
    dr.check_scalars(rec.values(), fx.calls, fx.calls_dev, CALL_FLOOR, case + " loss calls")
    dr.check_scalars(br.script_metrics(case, history), fx.metrics, fx.metrics_dev, CALL_FLOOR, case + " metrics")
    dr.check_params(model.state_dict(), fx, PARAM_FLOOR, label=case)


@pytest.mark.parametrize("case", ["airfoil", "pipe", "elas"])
def test_fit_static_reproduces_the_scripts_main(case, tmp_path):
    fx = br.Fixture(case)
    model = br.oracle_model(case)
    a, opt, sched = _adamw(model, case)
    d = br.load_data(case)
    rec = dr.RecordingLoss(TestLoss(size_average=False))
    path = str(tmp_path / "checkpoints" / (case + ".pt"))
    lrs = []
    hist = harness.fit_static(model, opt, sched, d, epochs=a["epochs"], batch_size=a["batch_size"],
                              max_grad_norm=a["max_grad_norm"], loss_fn=rec, epoch_orders=fx.perms, save_path=path,
                              scheduler_per_epoch=case == "elas", on_epoch=lambda ep, m: lrs.append(opt.param_groups[0]["lr"]))
    assert len(hist) == a["epochs"]
    _check(case, fx, rec, hist, model)
    steps = math.ceil(br.CASES[case]["ntrain"] / a["batch_size"])
    assert sched.last_epoch == (a["epochs"] if case == "elas" else a["epochs"] * steps)      # per epoch / per batch
    if case == "elas":       # the cosine over T_max = epochs, read after each epoch's single step
        assert lrs == pytest.approx([a["lr"] * (1 + math.cos(math.pi * (ep + 1) / a["epochs"])) / 2 for ep in range(a["epochs"])],
                                    abs=1e-12)
    fresh = br.oracle_model(case)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    dr.check_params(fresh.state_dict(), fx, PARAM_FLOOR, label=case + " checkpoint")
    ev = harness.evaluate_static(model, d, a["batch_size"], TestLoss(size_average=False))
    assert ev["rel_err"] == pytest.approx(hist[-1]["rel_err"], rel=1e-12)


def test_elas_schedule_stepped_per_batch_is_another_run():
    """scheduler_per_epoch=False on the elas case steps the cosine 3 x as often: the fixture's calls are missed (the flag
    does something, and the fixture tells the two placements apart)."""
    case = "elas"
    fx = br.Fixture(case)
    model = br.oracle_model(case)
    a, opt, sched = _adamw(model, case)
    rec = dr.RecordingLoss(TestLoss(size_average=False))
    harness.fit_static(model, opt, sched, br.load_data(case), epochs=a["epochs"], batch_size=a["batch_size"], loss_fn=rec,
                       epoch_orders=fx.perms, scheduler_per_epoch=False)
    assert sched.last_epoch == a["epochs"] * 3
    with pytest.raises(AssertionError):
        dr.check_scalars(rec.values(), fx.calls, fx.calls_dev, CALL_FLOOR, "elas stepped per batch")


def test_fit_plas_reproduces_exp_plas_main(tmp_path):
    case = "plas"
    fx = br.Fixture(case)
    model = br.oracle_model(case)
    a, opt, sched = _adamw(model, case)
    d = br.load_data(case)
    rec = dr.RecordingLoss(TestLoss(size_average=False))
    steps = []
    opt.register_step_post_hook(lambda *_: steps.append(sched.last_epoch))
    path = str(tmp_path / "plas.pt")
    hist = harness.fit_plas(model, opt, sched, d, epochs=a["epochs"], batch_size=a["batch_size"], loss_fn=rec,
                            epoch_orders=fx.perms, time_orders=fx.time_perms, save_path=path)
    _check(case, fx, rec, hist, model)
    T, nb = br.PLAS_T, math.ceil(br.PLAS_LIMIT["train"] / a["batch_size"])
    # T optimizer steps per batch, the scheduler once per batch: 20 steps at each value of the schedule's counter
    assert steps == [b for b in range(a["epochs"] * nb) for _ in range(T)] and sched.last_epoch == a["epochs"] * nb
    ev = harness.evaluate_plas(model, d, a["batch_size"], TestLoss(size_average=False))
    assert ev["test_full"] == pytest.approx(hist[-1]["test_full"], rel=1e-12)
    assert ev["test_step"] == pytest.approx(hist[-1]["test_step"], rel=1e-12)
    fresh = br.oracle_model(case)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)


def test_fit_plas_time_orders_matter_and_a_generator_replaces_them():
    """Another time permutation is another run; without `time_orders` the
    permutations come from the generator: equal seeds, equal histories; every timestep is visited once per sample."""
    case = "plas"
    fx = br.Fixture(case)
    d = br.load_data(case)
    a = br.parse_argv(br.CASES[case]["argv"])
    model = br.oracle_model(case)
    _, opt, sched = _adamw(model, case)
    rec = dr.RecordingLoss(TestLoss(size_average=False))
    identity = [[list(range(br.PLAS_T))] * br.PLAS_LIMIT["train"]] * a["epochs"]
    harness.fit_plas(model, opt, sched, d, epochs=1, batch_size=a["batch_size"], loss_fn=rec, epoch_orders=fx.perms,
                     time_orders=identity)
    with pytest.raises(AssertionError):          # the first batch's T training calls already miss the fixture's
        dr.check_scalars(rec.values()[:br.PLAS_T], fx.calls[:br.PLAS_T], fx.calls_dev[:br.PLAS_T], CALL_FLOOR, "identity")
    hists, seen = [], []
    for _ in range(2):
        model = br.oracle_model(case)
        _, opt, sched = _adamw(model, case)
        real = model.forward
        model.forward = lambda x, fx=None, T=None: (seen.append(T.detach().clone()) if model.training else None, real(x, fx, T))[1]
        hists.append(harness.fit_plas(model, opt, sched, d, epochs=1, batch_size=a["batch_size"],
                                      generator=torch.Generator().manual_seed(9)))
    assert hists[0] == hists[1]
    first_batch = torch.cat(seen[:br.PLAS_T], 1)                      # [2, T]: the times of the first batch's calls
    want = torch.tensor(np.linspace(0, 1, br.PLAS_T), dtype=torch.float)
    assert all(torch.equal(row.sort().values, want) for row in first_batch)
    assert not torch.equal(first_batch[0], first_batch[1])            # each sample has its own permutation
