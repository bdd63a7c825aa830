"""The merged SequenSolver without a GPU: the module's interface against the reference
(tests/golden/G13_sequensolver_merged.npz, written by tools/make_golden_sequensolver_merged.py), the refusals, the new C ABI
symbols with their host-side refusals, the pseudo-row grouping and the positional table against explicit constructions, and
the fixture's float64 results against the torch float64 restatement of tests/sequensolver_merged_restatement.py."""
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import sequensolver_merged_restatement as R

G13 = os.path.join(GOLDEN, "G13_sequensolver_merged.npz")
NEW_SYMBOLS = {      # name: number of arguments in include/pa2d.h
    "pa2d_seq_attn_causal_fwd": 11,
    "pa2d_seq_attn_causal_bwd": 15,
    "pa2d_head_seq_attn_fwd": 13,
    "pa2d_head_seq_attn_bwd_workspace": 3,
    "pa2d_head_seq_attn_bwd": 19,
}
TINY_ENCODER = dict(space_dim=2, n_layers=2, n_hidden=16, n_head=1, slice_num=8, fun_dim=1, out_dim=1, mlp_ratio=1,
                    unified_pos=1, ref=8, H=8, W=8)


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


def _model(g13, case, **over):
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    cfg, geom = json.loads(str(g13[case + ".config"])), json.loads(str(g13["geometry"]))
    kw = dict(T=cfg["T"], layers=cfg["layers"], B=cfg["B"], sequential_head=cfg["sequential_head"], **geom)
    kw.update(over)
    return SequenSolver(None, **kw)


def _tiny(**over):
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    kw = dict(T=3, W=8, H=8, M=8, C=16, B=1, sequential_head=8, layers=2, encoder_config=TINY_ENCODER)
    kw.update(over)
    return SequenSolver(None, **kw)


def test_constructor_signature_and_defaults_match_reference(g13):
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    ref = [tuple(p) for p in json.loads(str(g13["signature"]))]
    params = [(k, p) for k, p in inspect.signature(SequenSolver.__init__).parameters.items() if k != "self"]
    ours = [(k, None if p.default is inspect.Parameter.empty else p.default) for k, p in params]
    assert ours[:len(ref)] == ref and len(ref) == 12 and ref[7] == ("sequential_head", 1)
    assert [(k, p.kind, p.default) for k, p in params[len(ref):]] == [("encoder_config", inspect.Parameter.KEYWORD_ONLY, None)]
    for name in ("forward", "forward_slice", "get_code", "get_last_slice_weight", "add_positional_encoding", "attention",
                 "decode", "z_score_normalization", "freeze_attention", "set_engine"):
        assert callable(getattr(SequenSolver, name)), name


@pytest.mark.parametrize("case", ["a", "b"])
def test_state_dict_keys_shapes_strict_load_and_attributes(g13, case):
    m = _model(g13, case)
    ours = m.state_dict()
    assert list(ours) == [str(k) for k in g13[case + ".keys"]]
    assert [list(v.shape) for v in ours.values()] == json.loads(str(g13[case + ".shapes"]))
    assert "temperature" not in ours and "slice_weights" not in ours and "pe" not in ours
    assert not any(k.startswith(("weight_projection", "slice_projection", "temporal_slice_projection")) for k in ours)
    assert "temperature" not in dict(m.named_parameters())
    assert torch.equal(m.temperature, torch.full((1, 1, 1, 1), 0.5)) and "temperature" in dict(m.named_buffers())
    sd = {k: torch.from_numpy(v) for k, v in R.golden_state_dict(g13, case).items()}
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    cfg = json.loads(str(g13[case + ".config"]))
    heads = cfg["sequential_head"]
    assert (m.T, m.W, m.H, m.M, m.C, m.N, m.B, m.dim, m.Head, m.layers) == (10, 64, 64, 16, 32, 4096, cfg["B"], 512, 1,
                                                                           cfg["layers"])
    assert (m.sequential_head, m.seq_dim, m.fundemental, m.concatenated) == (heads, 512 // heads, 74, 768)
    assert tuple(m.to_q.weight.shape) == (512 // heads, 512 // heads)
    assert m.scale == 512 ** -0.5 and m.code is None and tuple(m.slice_weights.shape) == (cfg["B"], 1, 4096, 16)
    assert not m.encoder.training and not any(p.requires_grad for p in m.encoder.parameters())
    m.train()
    assert m.training and not m.encoder.training


def test_freeze_attention_freezes_the_reference_set(g13):
    m = _model(g13, "a")
    m.freeze_attention()
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad and not k.startswith("encoder.")]
    assert frozen == json.loads(str(g13["a.frozen.names"])) and len(frozen) == 11
    assert not any(mod.training for mod in (m.to_q, m.to_k, m.to_v, m.mlp, m.ln_1, m.ln_2))


def test_positional_table_against_the_formula(g13):
    m = _tiny(T=5)
    pe = m.pe
    assert tuple(pe.shape) == (5, 128) and pe.dtype == torch.float32 and "pe" in dict(m.named_buffers())
    assert torch.equal(pe, R.pe_table(5, 128))
    for t in range(5):
        for i in range(0, 128, 2):
            div = 10000.0 ** (i / 128)
            assert abs(float(pe[t, i]) - math.sin(t / div)) < 2e-6 and abs(float(pe[t, i + 1]) - math.cos(t / div)) < 2e-6
    tok = torch.randn(2, 1, 5, 128)
    assert torch.equal(m.add_positional_encoding(tok), tok + pe)
    tok64 = tok.double()            # a float64 run adds the same fp32 table
    assert torch.equal(m.add_positional_encoding(tok64), tok64 + pe.double())
    other = torch.zeros(1, 1, 3, 8)      # another shape: the table of that shape, as the reference builds it per call
    assert torch.equal(m.add_positional_encoding(other)[0, 0], R.pe_table(3, 8))


@pytest.mark.parametrize("B,T,heads,sd", [(1, 10, 16, 32), (2, 3, 4, 12), (1, 7, 1, 8), (3, 5, 8, 4)])
def test_pseudo_row_grouping_against_explicit_indices(B, T, heads, sd):
    """Group g holds the pseudo-rows g*T .. g*T+T-1; pseudo-row p is chunk p % heads of real token p // heads.  The
    restatement's reshape is checked against a gather written index by index, and its attention against a loop over the
    groups with an explicit causal softmax."""
    g = torch.Generator().manual_seed(B + 10 * T + heads)
    dim = heads * sd
    x = torch.randn(B, T, dim, generator=g, dtype=torch.float64)
    wq, wk, wv = (torch.randn(sd, sd, generator=g, dtype=torch.float64) for _ in range(3))
    idx = R.pseudo_row_groups(T, heads)
    groups = torch.empty(B, heads, T, sd, dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            for i in range(T):
                tok, chunk = int(idx[h, i, 0]), int(idx[h, i, 1])
                groups[b, h, i] = x[b, tok, chunk * sd:(chunk + 1) * sd]
    assert torch.equal(groups, x.reshape(B, heads, T, sd))
    scale = dim ** -0.5
    want = torch.zeros(B, T, dim, dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            q, k, v = groups[b, h] @ wq.t(), groups[b, h] @ wk.t(), groups[b, h] @ wv.t()
            for i in range(T):
                logits = (k[:i + 1] @ q[i]) * scale
                a = torch.exp(logits - logits.max())
                row = (a / a.sum()) @ v[:i + 1]
                tok, chunk = int(idx[h, i, 0]), int(idx[h, i, 1])
                want[b, tok, chunk * sd:(chunk + 1) * sd] = row
    got = R.head_attention(x, wq, wk, wv, heads, scale)
    assert float((got - want).abs().max()) < 1e-12
    res = torch.randn(B, T, dim, generator=g, dtype=torch.float64)
    assert torch.equal(R.head_attention(x, wq, wk, wv, heads, scale, res=res), got + res)


def test_forward_slice_is_the_slice_learners_implementation(monkeypatch):
    from transformerbasednavierstokesolver_amd import SequenSolverMerged as SM, SliceLearner as SL
    assert SM.code_conditioned_slice_weights is SL.code_conditioned_slice_weights
    seen = []

    def spy(x, fx, code, preprocess, in_project_x, in_project_slice, temperature, H, W, M, C, engine):
        seen.append((preprocess, in_project_x, in_project_slice, temperature, H, W, M, C))
        return "sentinel"

    monkeypatch.setattr(SL, "code_conditioned_slice_weights", spy)
    monkeypatch.setattr(SM, "code_conditioned_slice_weights", spy)
    m = _tiny()
    x, fx, code = torch.zeros(1, 64, 64), torch.zeros(1, 64, 3), torch.zeros(1, 1, 8, 16)
    assert m.forward_slice(x, fx, code) == "sentinel"
    assert seen[-1][:4] == (m.preprocess, m.in_project_x, m.in_project_slice, m.temperature) and seen[-1][4:] == (8, 8, 8, 16)
    v = SL.VorticitySliceLearner(C=16, M=8, T=3, H=8, W=8, n_hidden=32)
    assert v(x, fx, code) == "sentinel"
    assert seen[-1][:4] == (v.preprocess, v.in_project_x, v.in_project_slice, v.temperature)
    with pytest.raises(ValueError, match="64 positional features"):
        m.forward_slice(torch.zeros(1, 64, 2), fx, code)


def test_refusals():
    from transformerbasednavierstokesolver_amd import ops
    from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver
    m = _tiny()
    with pytest.raises(NotImplementedError):
        m.set_engine("bf16s")
    m.set_engine("f32")
    assert m.engine == ops.ENGINE_F32 and m.encoder.engine == ops.ENGINE_F32
    assert all(mod.engine == ops.ENGINE_F32 for mod in (m.mlp, m.preprocess, m.in_project_slice))
    x, fx, y = torch.zeros(1, 64, 64), torch.zeros(1, 64, 3), torch.zeros(1, 64, 1)
    m.engine = ops.ENGINE_BF16S              # set behind set_engine's back: refused when the model runs
    for call in (lambda: m(x, fx, y), lambda: m.get_code(x, fx, y), lambda: m.attention(torch.zeros(1, 1, 3, 128)),
                 lambda: m.forward_slice(x, fx, torch.zeros(1, 1, 8, 16))):
        with pytest.raises(NotImplementedError, match="bf16"):
            call()
    md = _tiny(dropout=0.1).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        md(x, fx, y)
    with pytest.raises(NotImplementedError, match="dropout"):
        md.attention(torch.zeros(1, 1, 3, 128))
    with pytest.raises(ValueError, match="sequential_head = 3 must divide dim = M\\*C = 128"):
        _tiny(sequential_head=3)
    with pytest.raises(NotImplementedError, match="seq_dim % 4 == 0"):
        _tiny(sequential_head=64)                                     # seq_dim = 2
    with pytest.raises(NotImplementedError, match="T <= 32; got T = 33"):
        _tiny(T=33)
    for over in (dict(M=16), dict(C=32), dict(H=5, W=6), dict(H=12)):
        with pytest.raises(ValueError):
            _tiny(**over)
    with pytest.raises(ValueError):
        SequenSolver(None, T=3, W=64, H=64, M=8, C=32, B=1)          # the reference's hard-coded encoder has 16 slices


def test_c_abi_symbols_bound_with_header_arity():
    from transformerbasednavierstokesolver_amd import _lib
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pa2d.h")).read()
    flat = " ".join(header.split())
    for name, arity in NEW_SYMBOLS.items():
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
        decl = flat.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(decl.split(",")) == arity, name
        assert "SequenSolverMerged.py" in header.split(name + "(", 1)[0].rsplit("/* ----", 1)[1], name     # cites the reference


def test_host_side_refusals_with_null_pointers():
    from transformerbasednavierstokesolver_amd import _lib
    lib = _lib.load()
    ARG, UNSUP, WS = 1001, 1002, 1003
    # pa2d_head_seq_attn_fwd(x, wq, wk, wv, res, out, attn, G, T, sd, scale, causal, stream)
    fwd = lib.pa2d_head_seq_attn_fwd
    # pa2d_head_seq_attn_bwd(x, wq, wk, wv, attn, dout, dx, dwq, dwk, dwv, ws, ws_bytes, G, T, sd, scale, causal, acc, stream)
    bwd = lib.pa2d_head_seq_attn_bwd
    wsf = lib.pa2d_head_seq_attn_bwd_workspace
    for T, sd in ((0, 32), (33, 32), (10, 2), (10, 66), (10, 68)):
        assert fwd(0, 0, 0, 0, 0, 0, 0, 1, T, sd, 1.0, 1, 0) == UNSUP, (T, sd)
        assert bwd(*([0] * 12), 1, T, sd, 1.0, 1, 0, 0) == UNSUP, (T, sd)
        assert wsf(1, T, sd) == 0
    assert fwd(0, 0, 0, 0, 0, 0, 0, -1, 10, 32, 1.0, 1, 0) == ARG
    assert fwd(0, 0, 0, 0, 0, 0, 0, 1, 10, 32, 1.0, 1, 0) == ARG            # supported shape, null pointers
    assert fwd(0, 0, 0, 0, 0, 0, 0, 0, 10, 32, 1.0, 1, 0) == 0              # G = 0: no-op
    assert bwd(*([0] * 12), 0, 10, 32, 1.0, 1, 0, 0) == 0
    assert bwd(*([0] * 12), 0, 10, 32, 1.0, 1, 1, 0) == 0
    assert bwd(*([16] * 10), 0, 0, 1, 10, 32, 1.0, 1, 0, 0) == WS
    # one record of the three [sd, sd] gradients per workgroup, at most 32 workgroups however many groups
    assert wsf(1, 10, 32) == 3 * 32 * 32 * 4 and wsf(16, 10, 32) == 16 * 3 * 32 * 32 * 4
    assert wsf(40, 7, 20) == 32 * 3 * 20 * 20 * 4 == wsf(4000, 7, 20) and wsf(0, 10, 32) == 0
    # the causal mode of pa2d_seq_attn: the limits and the workspace of the plain entry points
    cf, cb = lib.pa2d_seq_attn_causal_fwd, lib.pa2d_seq_attn_causal_bwd
    assert cf(0, 0, 0, 0, 0, 0, 1, 0, 128, 1.0, 0) == UNSUP and cf(0, 0, 0, 0, 0, 0, 1, 33, 128, 1.0, 0) == UNSUP
    assert cf(0, 0, 0, 0, 0, 0, 1, 10, 126, 1.0, 0) == UNSUP and cf(0, 0, 0, 0, 0, 0, 1, 10, 1028, 1.0, 0) == UNSUP
    assert cf(0, 0, 0, 0, 0, 0, 1, 10, 128, 1.0, 0) == ARG and cf(0, 0, 0, 0, 0, 0, 0, 10, 128, 1.0, 0) == 0
    assert cb(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 33, 128, 1.0, 0) == UNSUP
    assert cb(16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 1, 10, 128, 1.0, 0) == WS
    assert cb(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 128, 1.0, 0) == 0


def test_python_layers_expose_the_new_paths():
    from transformerbasednavierstokesolver_amd import functional as Fn, ops
    assert (ops.HEAD_SEQ_ATTN_MAX_T, ops.HEAD_SEQ_ATTN_MAX_SD, ops.SEQ_ATTN_MAX_T) == (32, 64, 32)
    assert inspect.signature(Fn.seq_attention).parameters["causal"].default is False
    p = inspect.signature(Fn.head_seq_attention).parameters
    assert list(p)[:6] == ["xn", "wq", "wk", "wv", "heads", "scale"]
    assert (p["res"].default, p["causal"].default, p["engine"].default, p["fused"].default) == (None, True, None, None)
    x, w = torch.zeros(1, 3, 64), torch.zeros(16, 16)
    for fused in (None, False):                                # no CPU path on either route
        with pytest.raises(RuntimeError, match="GPU"):
            Fn.head_seq_attention(x, w, w, w, 4, 1.0, fused=fused)
    with pytest.raises(ValueError, match="must divide"):
        Fn.head_seq_attention(x, w, w, w, 5, 1.0)
    for fn in (ops.head_seq_attn_fwd, ops.seq_attn_causal_fwd):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(*((x.reshape(4, 3, 16), w, w, w, 1.0) if fn is ops.head_seq_attn_fwd else (x, x, x, 1.0)))


# ---------------------------------------------------------------------------------------------- restatement vs golden
def _restated(g13, case, frozen=False):
    from transformerbasednavierstokesolver_amd.SequenSolver import REFERENCE_ENCODER
    cfg = json.loads(str(g13[case + ".config"]))
    names = json.loads(str(g13[case + ".frozen.names"])) if frozen else []
    sd = {k: torch.from_numpy(v).double() for k, v in R.golden_state_dict(g13, case).items()}
    for k, v in sd.items():
        v.requires_grad_(not k.startswith("encoder.") and k not in names)
    pos, fx, y, _ = (torch.from_numpy(a).double() for a in R.golden_inputs(g13, case))
    out, code, sw = R.forward(sd, REFERENCE_ENCODER, cfg["layers"], cfg["sequential_head"], pos, fx, y)
    loss = R.rel_l2_loss(out, y)
    loss.backward()
    with torch.no_grad():
        plain = R.forward(sd, REFERENCE_ENCODER, cfg["layers"], cfg["sequential_head"], pos, fx, positional=False)[1]
    return sd, out, code, sw, loss, plain


@pytest.mark.parametrize("case", ["a", "b"])
def test_float64_restatement_reproduces_the_fixture(g13, case):
    """The fixture holds the reference's float64 results rounded to float32 (6e-8 relative), so the float64 restatement
    must meet them to 1e-6; 1e-5 for the gradients of to_q / to_k, which are differences of nearly equal terms (the bounds
    of the G10 check in test_sequensolver_host.py)."""
    sd, out, code, sw, loss, plain = _restated(g13, case)
    pre = f"{case}.pred."
    for key, got in (("out", out), ("code", code), ("slice_weights", sw)):
        err = R.golden_rel(g13, pre + key, got)
        print(f"{case} {key}: rel-L2 {err:.3g}")
        assert err < 1e-6, key
    assert R.golden_rel(g13, f"{case}.get_code", plain) < 1e-6
    assert R.golden_rel(g13, f"{case}.get_code", code) > 1e-3          # get_code adds no positional encoding
    assert abs(float(sw.detach().sum()) - float(g13[pre + "slice_weights.sum"])) < 1e-6 * sw.shape[0] * sw.shape[2]
    assert 0.3 <= float(sw.max(-1).values.mean()) <= 0.9
    assert abs(float(loss.detach()) - float(g13[pre + "loss"])) < 1e-9 * float(loss.detach())
    none = [k for k, v in sd.items() if v.grad is None]
    assert none == json.loads(str(g13[pre + "no_grad"])) and all(k.startswith("encoder.") for k in none)
    for k, v in sd.items():
        if k in none:
            continue
        tol = 1e-5 if k in ("to_q.weight", "to_k.weight") else 1e-6
        err = R.golden_rel(g13, pre + "grad." + k, v.grad)
        print(f"{case} grad {k}: rel-L2 {err:.3g}")
        assert err < tol, k
    if case == "a":
        assert R.golden_rel(g13, "a.gt.out", out) < 1e-6               # use_gt=True gives the same output


def test_float64_restatement_reproduces_the_frozen_case(g13):
    sd, _, _, _, loss, _ = _restated(g13, "a", frozen=True)
    assert abs(float(loss.detach()) - float(g13["a.frozen.loss"])) < 1e-9 * float(loss.detach())
    none = [k for k, v in sd.items() if v.grad is None]
    assert none == json.loads(str(g13["a.frozen.no_grad"]))
    for k, v in sd.items():
        if k not in none:
            assert R.golden_rel(g13, "a.frozen.grad." + k, v.grad) < 1e-6, k


def test_fixture_carries_the_float32_yardstick(g13):
    keys = [k for k in g13.files if k.startswith("fp32_self_error.")]
    assert len(keys) > 100
    for k in ("a.pred.out", "b.pred.slice_weights", "a.train.losses", "a.rollout.pred", "b.get_code", "a.gt.out",
              "b.frozen.grad.ln_3.weight", "b.pred.grad.in_project_x.weight"):
        assert "fp32_self_error." + k in g13.files, k
    assert len(g13["a.train.losses"]) == 3
    scale = json.loads(str(g13["slice_scale"]))
    assert sorted(scale) == ["linear_post.weight", "linear_pre.0.weight", "linears.0.0.weight"]
    for case in ("a", "b"):
        assert 0.3 <= json.loads(str(g13[case + ".mean_largest_weight"])) <= 0.9


# ---------------------------------------------------------------------------------------------- registration order
# Taken from the constructor as it stood before the two classes got their common base: the state_dict's key order, the
# parameter order (the layout of an optimizer's flat bucket) and the order in which construction draws from the RNG.
OWN_KEYS = [
    "to_q.weight", "to_k.weight", "to_v.weight", "ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias",
    "mlp.linear_pre.0.weight", "mlp.linear_pre.0.bias", "mlp.linear_post.weight", "mlp.linear_post.bias",
    "preprocess.linear_pre.0.weight", "preprocess.linear_pre.0.bias", "preprocess.linear_post.weight",
    "preprocess.linear_post.bias", "in_project_x.weight", "in_project_x.bias",
    "in_project_slice.linear_pre.0.weight", "in_project_slice.linear_pre.0.bias",
    "in_project_slice.linear_post.weight", "in_project_slice.linear_post.bias",
    "in_project_slice.linears.0.0.weight", "in_project_slice.linears.0.0.bias", "ln_3.weight", "ln_3.bias",
    "mlp2.weight", "mlp2.bias",
]
SEEDED_SHA256 = "389a4a1652c30a56a70060f0e35bbadac39067fb96ba0ad46569faeac9343d5a"


def test_registration_order_is_the_constructors_of_before_the_common_base():
    from test_sequensolver_host import ENCODER_KEYS
    m = _tiny()
    assert list(m.state_dict()) == ENCODER_KEYS + OWN_KEYS
    assert [n for n, _ in m.named_parameters()] == ENCODER_KEYS + OWN_KEYS
    assert [n for n, _ in m.named_buffers()] == ["slice_weights", "pe", "temperature", "encoder.pos"]


def test_seeded_construction_draws_from_the_rng_in_the_same_order():
    from test_sequensolver_host import _state_sha256
    torch.manual_seed(0)
    assert _state_sha256(_tiny()) == SEEDED_SHA256


def test_shared_methods_live_on_the_common_base():
    from transformerbasednavierstokesolver_amd import SequenSolver as S, SequenSolverMerged as SM
    assert issubclass(SM.SequenSolver, S._LatentSequence) and issubclass(S.SequenSolver, S._LatentSequence)
    assert not hasattr(SM.SequenSolver, "code_windows") and not hasattr(SM.SequenSolver, "solve_with_slice_learner")
    assert hasattr(S.SequenSolver, "code_windows") and hasattr(S.SequenSolver, "solve_with_slice_learner")
    # get_code stays its own here: no positional table, and the docstring that says so
    assert "get_code" in vars(SM.SequenSolver) and "positional" in SM.SequenSolver.get_code.__doc__
