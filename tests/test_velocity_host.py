"""The epoch loops harness.fit_velocity / fit_velocity_unrolled / fit_unrolled_t against the reference scripts' own main()
(fixtures G25-G27, tools/make_golden_velocity_drivers.py), without a GPU: the fp64 oracle behind the reference's parameter
names (driver_restatement.OracleModel / OracleSOL) goes through the loops on the CPU with torch.optim.AdamW + OneCycleLR and
the fixtures' batch orders.  The bounds are those of test_drivers_host.py: every recorded loss call and epoch metric within
max(1e-6 relative, 4 x the fixture's own deviation), every final parameter tensor within max(1e-5, 4 x its own deviation)
rel-L2.  That pins the loop logic: the windows and their targets, the look-ahead curricula (1 -> 2 at epoch 40; 1 -> 2 -> 3
at epochs 10 and 20), the short last batch, the normalisations, the save cadence and which module is saved.  Plus: the
loader against a numpy restatement, the synthetic velocity field, train_velocity.py's flags against the recorded parsers,
the new C symbols against the header, and train.DRIVERS unchanged."""
import ctypes
import os

import numpy as np
import pytest
import torch

import driver_restatement as dr
import velocity_restatement as vr
from conftest import ROOT
from transformerbasednavierstokesolver_amd import data, harness, synth, train, train_velocity
from transformerbasednavierstokesolver_amd.utils.testloss import TestLoss

CALL_FLOOR, PARAM_FLOOR = 1e-6, 1e-5
NEW_SYMBOLS = {      # name: number of arguments in include/pa2d.h
    "pa2d_rel_l2_window_fwd": 13,
    "pa2d_rel_l2_window_bwd": 12,
    "pa2d_rollout_tail": 16,
    "pa2d_rollout_score": 7,
}


def _adamw(model, case):
    a = vr.parse_argv(vr.CASES[case]["argv"])
    opt = torch.optim.AdamW(model.parameters(), lr=a["lr"], weight_decay=a["weight_decay"])
    return a, opt, vr.one_cycle(opt, case)


def _count_saves(monkeypatch):
    saves = []
    real = torch.save
    monkeypatch.setattr(torch, "save", lambda obj, path, *a, **k: (saves.append((path, sorted(obj))), real(obj, path, *a, **k))[1])
    return saves


def _check(fx, calls, history, module, label):
    dr.check_scalars(vr.calls_of(calls), fx.calls, fx.calls_dev, CALL_FLOOR, label + " loss calls")
    dr.check_scalars(dr.history_table(history, fx.metric_names), fx.metrics, fx.metrics_dev, CALL_FLOOR, label + " metrics")
    dr.check_params(module.state_dict(), fx, PARAM_FLOOR, label=label)


def test_fit_velocity_reproduces_ns_velocity_main(tmp_path, monkeypatch):
    case = "velocity"
    fx = vr.Fixture(case)
    model = dr.OracleModel(vr.model_config(case), vr.weights(case))
    a, opt, sched = _adamw(model, case)
    train_set, test_set = vr.datasets(case)
    calls, saves = [], _count_saves(monkeypatch)
    path = str(tmp_path / "checkpoints" / "velocity.pt")
    hist = harness.fit_velocity(model, opt, sched, train_set, test_set, epochs=a["epochs"], batch_size=a["batch_size"],
                                loss_fn=TestLoss(size_average=False), epoch_orders=fx.perms, save_path=path, calls=calls)
    # the reference's cadence: ep % 100 == 0 and the end; the whole model
    assert [p for p, _ in saves] == [path] * 2 and all(keys == sorted(model.state_dict()) for _, keys in saves)
    assert len(hist) == a["epochs"] == 3
    _check(fx, calls, hist, model, case)
    fresh = dr.OracleModel(vr.model_config(case), vr.weights(case))
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    dr.check_params(fresh.state_dict(), fx, PARAM_FLOOR, label=case + " checkpoint")


@pytest.mark.parametrize("case,fit", [("velocity_unrolled", "fit_velocity_unrolled"), ("unrolled_t", "fit_unrolled_t")])
def test_sol_loops_reproduce_the_reference_mains(case, fit, tmp_path, monkeypatch):
    fx = vr.Fixture(case)
    s = vr.script(case)
    sol = dr.OracleSOL(vr.model_config(case), vr.weights(case), step=vr.STEP)
    a, opt, sched = _adamw(sol, case)
    train_set, test_set = vr.datasets(case)
    calls, saves = [], _count_saves(monkeypatch)
    path = str(tmp_path / (case + ".pt"))
    hist = getattr(harness, fit)(sol, opt, sched, train_set, test_set, epochs=a["epochs"], batch_size=a["batch_size"],
                                 T=s["T"], loss_fn=TestLoss(size_average=False), epoch_orders=fx.perms, save_path=path,
                                 calls=calls)                        # max_look_ahead, period: the defaults = the script's
    assert [h["look_ahead"] for h in hist] == vr.LOOK_AHEAD_HISTORY[case] == fx.settings["look_ahead"]
    inner_keys = sorted(sol.transolver_model.state_dict())
    assert [p for p, _ in saves] == [path] * 2 and all(keys == inner_keys for _, keys in saves)      # the INNER model
    _check(fx, calls, hist, sol.transolver_model, case)
    if case == "velocity_unrolled":      # train_step: the loss of the epoch's last batch (the script assigns, never adds)
        nb, per_epoch = -(-len(train_set) // a["batch_size"]), fx.calls.size // a["epochs"]
        last = fx.calls.reshape(a["epochs"], per_epoch)[:, nb - 1]
        dr.check_scalars([h["train_step"] for h in hist], last, fx.calls_dev.reshape(a["epochs"], per_epoch)[:, nb - 1],
                         CALL_FLOOR, "last-batch loss")
    fresh = dr.OracleModel(vr.model_config(case), vr.weights(case))       # the inner model's keys, no wrapper prefix
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    dr.check_params(fresh.state_dict(), fx, PARAM_FLOOR, label=case + " checkpoint")


def test_step_curriculum_is_the_scripts_rule():
    for period, top, epochs in ((40, 8, 500), (10, 4, 80)):
        c, la, want = harness.StepCurriculum(period, 1, top), 1, []
        got = [c.update(ep) for ep in range(epochs)]
        for ep in range(epochs):
            if ep % period == 0 and ep >= period and la <= top:
                la += 1
            want.append(la)
        assert got == want and max(got) == min(top + 1, 1 + (epochs - 1) // period)       # it can pass max_look_ahead by one


def test_synthetic_data_is_what_the_fixtures_were_made_on():
    for case in vr.CASES:
        fx = vr.Fixture(case)
        np.testing.assert_allclose(vr.data_sums(case), fx.settings["data_sums"], rtol=1e-9)
        assert fx.perms == vr.permutations(case)
        assert fx.settings["config"] == vr.model_config(case)
        s = vr.script(case)
        shipped = fx.settings["constants"]                     # the module constants the reference shipped with
        assert (shipped["ntrain"], shipped["ntest"], shipped["T_in"], shipped["T"], shipped["step"]) == \
            (s["ntrain"], s["ntest"], s["T_in"], s["T"], vr.STEP)
        assert shipped.get("max_look_ahead") == s["max_look_ahead"]


@pytest.mark.parametrize("r", [1, 4, 9])
def test_load_velocity_npy_against_a_numpy_restatement(r, tmp_path):
    rng = np.random.default_rng(5)
    arr = rng.standard_normal((7, 64, 64, 24)).astype(np.float32)
    path = str(tmp_path / "ns.npy")
    np.save(path, arr)
    ntrain, ntest, T_in, T = 4, 2, 10, 12
    h, train_set, test_set = data.load_velocity_npy(path, ntrain, ntest, T_in, T, r)
    assert h == int(((64 - 1) / r) + 1)
    for ds, block in ((train_set, arr[:ntrain]), (test_set, arr[-ntest:])):      # the LAST ntest samples test
        pos, a, u = ds.tensors
        want_a = block[:, ::r, ::r, :T_in][:, :h, :h, :]
        want_u = block[:, ::r, ::r, T_in:T + T_in][:, :h, :h, :]
        assert np.array_equal(a.numpy(), want_a.reshape(want_a.shape[0], -1, T_in))
        assert np.array_equal(u.numpy(), want_u.reshape(want_u.shape[0], -1, T))
        x, y = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, h))
        want_pos = torch.tensor(np.c_[x.ravel(), y.ravel()], dtype=torch.float)
        assert pos.shape == (block.shape[0], h * h, 2) and all(torch.equal(p, want_pos) for p in pos)


def test_velocity_fields_are_seeded_interleaved_and_divergence_free():
    v = synth.velocity_fields(2, 16, 16, frames=3, seed=9)
    assert v.shape == (2, 16, 16, 6) and v.dtype == np.float32 and np.array_equal(v, synth.velocity_fields(2, 16, 16, 3, 9))
    assert not np.array_equal(v, synth.velocity_fields(2, 16, 16, 3, 10)) and abs(float(v.std()) - 1.0) < 1e-5
    vx, vy = v[..., 0::2].astype(np.float64), v[..., 1::2].astype(np.float64)      # frame t: columns (2 t, 2 t + 1)
    ky = np.fft.fftfreq(16, d=1.0 / 16)[None, :, None, None]
    kx = np.fft.fftfreq(16, d=1.0 / 16)[None, None, :, None]
    div = kx * np.fft.fft2(vx, axes=(1, 2)) + ky * np.fft.fft2(vy, axes=(1, 2))
    assert np.abs(div).max() <= 1e-5 * np.abs(kx * np.fft.fft2(vx, axes=(1, 2))).max()      # fp32 rounding of the field only
    # the vorticity of the field is the generator's vorticity up to the scale and the dropped modes: it is not trivial
    assert np.abs(vx).max() > 0.1 and np.abs(vy).max() > 0.1


@pytest.mark.parametrize("case", list(vr.CASES))
def test_train_velocity_parser_has_the_reference_flags_and_defaults(case):
    driver = vr.CASES[case]["driver"]
    recorded = vr.Fixture(case).parser
    ours = {a.dest: a for a in train_velocity.build_parser(driver)._actions if a.dest != "help"}
    for flags, dest, default, typ in recorded:
        a = ours[dest]
        assert list(a.option_strings) == flags and a.default == default and getattr(a.type, "__name__", None) == typ, dest
    assert set(ours) - {r[1] for r in recorded} == {"driver", "engine"}
    args = train_velocity.parse_args(["--driver", driver])
    s = vr.script(case)
    assert (args.driver, args.ntrain, args.ntest, args.T_in, args.T, args.step, args.graphed) == \
        (driver, s["ntrain"], s["ntest"], s["T_in"], s["T"], vr.STEP, 0)
    assert getattr(args, "max_look_ahead", None) == s["max_look_ahead"]
    assert train_velocity.parse_args(["--driver", driver, "--data_path", "/x/y.npy", "--eval", "1"]).data_path == "/x/y.npy"


def test_existing_command_lines_are_unchanged():
    assert train.DRIVERS == ("ns", "unrolled", "darcy", "airfoil", "pipe", "elas", "plas")
    assert train_velocity.DRIVERS == ("velocity", "velocity_unrolled", "unrolled_t")
    with pytest.raises(SystemExit):
        train.parse_args(["--driver", "velocity"])


def test_c_abi_symbols_bound_with_header_arity():
    from transformerbasednavierstokesolver_amd import _lib, ops
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pa2d.h")).read()
    flat = " ".join(header.split())
    for name, arity in NEW_SYMBOLS.items():
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
        decl = flat.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(decl.split(",")) == arity, name
    for macro, value in (("PA2D_WINDOW_SPLIT", ops.WINDOW_SPLIT), ("PA2D_WINDOW_MAX_K", ops.WINDOW_MAX_K),
                         ("PA2D_WINDOW_MAX_F", ops.WINDOW_MAX_F)):
        assert f"#define {macro} {value}" in flat
    for name in ("rel_l2_window_fwd", "rel_l2_window_bwd", "rollout_tail", "rollout_score", "rollout_record"):
        assert callable(getattr(ops, name))


def test_graphed_loops_refuse_what_they_would_not_apply():
    case = "velocity"
    model = dr.OracleModel(vr.model_config(case), vr.weights(case))
    a, opt, sched = _adamw(model, case)
    train_set, test_set = vr.datasets(case)
    with pytest.raises(ValueError, match="max_grad_norm"):
        harness.fit_velocity(model, opt, sched, train_set, test_set, epochs=1, batch_size=4, max_grad_norm=0.1, graphed=True)
    with pytest.raises(TypeError, match="FusedAdamW"):
        harness.fit_velocity(model, opt, sched, train_set, test_set, epochs=1, batch_size=4, graphed=True)
    model.add_module("drop", torch.nn.Dropout(0.1))
    with pytest.raises(NotImplementedError, match="dropout"):
        harness.fit_velocity(model, opt, sched, train_set, test_set, epochs=1, batch_size=4, graphed=True)


def test_graphed_or_eager_keeps_one_graph_per_key():
    """On stubs: a full batch with key k builds once per distinct k and replays after that; a short batch goes to `eager`
    even when a graph for its key exists; with graphed=False `build` is never called; no key is the one key None.  A key
    that is given reaches build, replay and eager as their last argument."""
    full, short = torch.zeros(4, 1), torch.zeros(3, 1)
    for graphed in (True, False):
        log, keys = [], []
        run = harness._graphed_or_eager(graphed, 4,
                                        lambda x, tag, *k: keys.append(k) or log.append(("build", tag)) or ("graph", tag),
                                        lambda graph, x, tag, *k: keys.append(k) or log.append(("replay", graph, tag)) or "replayed",
                                        lambda x, tag, *k: keys.append(k) or log.append(("eager", x.shape[0], tag)) or "eager")
        got = [run(full, "a", key=1), run(full, "b", key=1), run(full, "c", key=2), run(short, "d", key=1),
               run(full, "e", key=1), run(full, "f"), run(full, "g"), run(short, "h")]
        if not graphed:
            assert got == ["eager"] * 8 and [e[0] for e in log] == ["eager"] * 8
            assert keys == [(1,), (1,), (2,), (1,), (1,), (), (), ()]
            continue
        assert keys == [(1,), (1,), (1,), (2,), (2,), (1,), (1,), (), (), (), ()]
        assert got == ["replayed", "replayed", "replayed", "eager", "replayed", "replayed", "replayed", "eager"]
        assert log == [("build", "a"), ("replay", ("graph", "a"), "a"), ("replay", ("graph", "a"), "b"),
                       ("build", "c"), ("replay", ("graph", "c"), "c"), ("eager", 3, "d"), ("replay", ("graph", "a"), "e"),
                       ("build", "f"), ("replay", ("graph", "f"), "f"), ("replay", ("graph", "f"), "g"), ("eager", 3, "h")]


def test_velocity_runner_hands_the_key_to_the_eager_iteration():
    """The short batch of a graphed SOL loop runs eagerly at ITS look-ahead, with the loop's own zero_grad argument."""
    seen = []
    model = torch.nn.Linear(1, 1)

    class Opt:
        def zero_grad(self, **kw):
            seen.append(("zero_grad", kw))

        def step(self):
            seen.append("step")

    def forward(key, x, fx, yy, vals):
        seen.append(("forward", key, x.shape[0]))
        return (model(x).sum(),)

    run = harness._velocity_runner(model, Opt(), None, 4, True, None, None, None, forward, 1, dict(set_to_none=False))
    (loss,) = run(3, torch.ones(2, 1), None, None)
    assert seen == [("forward", 3, 2), ("zero_grad", dict(set_to_none=False)), "step"] and not loss.requires_grad


def test_scored_rollout_refuses_a_cpu_module():
    case = "velocity"
    model = dr.OracleModel(vr.model_config(case), vr.weights(case))
    x, fx, yy = next(vr.datasets(case)[1].batches(2))
    assert not harness.scored_rollout_supported(model, x, fx, yy, vr.STEP, TestLoss(size_average=False))
    with pytest.raises(ValueError):
        harness.scored_rollout(model, x, fx, yy, vr.STEP)
