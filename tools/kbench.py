#!/usr/bin/env python
"""Per-stage micro-benchmark at the bench shapes (B=32, N=4096, C=256, 8 heads, M=64): times each
libpa2d stage alone with events on the launch stream and prints achieved TFLOP/s or GB/s.
The conv3d_* stages time the 3x3x3 conv of the structured 3-D mesh on a --B3 x --S3^3 mesh (default 1 x 32^3).
The ae_* stages run at auto_encoder.py's shape (--AB x 64 x 64, C=64, 4 heads, M=--AM, 3 layers): the four kernels of the
auto-encoder attention (slice weights forward / backward, de-slice with explicit weights forward / backward; GB/s and the
fraction of the 8 TB/s HBM peak) and one whole auto-encoder training iteration (autoencoder_train_step, FusedAdamW).
The seq_attn_* / code_sw_* stages time the two SequenSolver stages at the reference's shape (--SB samples, T=10 tokens of
dim=512; 64 x 64 points, M=16, C=32; code_sw_* is the two-coordinate entry, served by the point_sw kernels with P = 2),
seq_iter one sequensolver_train_step (T=10, layers=8, Tout=1, FusedAdamW) at B=1 and B=8.
The head_seq_attn_* stages time the merged SequenSolver's attention at the reference's shape (--SB samples, T=10, 16 heads of
seq_dim=32): the fused kernel (one launch forward, two backward) and, as *_unfused, the same through three linears and the
causal seq_attn (functional.head_seq_attention, forward, and forward plus backward through autograd); merged_iter one
sequensolver_train_step of SequenSolverMerged (T=10, layers=8, sequential_head=16, Tout=1, use_gt=False, FusedAdamW) at B=1
with the fused kernel and without, ten runs each (median and range).
The point_sw_* stages time the LearnSlice kernel at the same shape with P = 2 / 64 / 74 point features and B = 1 / 8,
learnslice_iter one frame of learnslice_train_step (frozen SequenSolver T=10, layers=8; FusedAdamW) for the three widths.
The conv3x3_* / zscore / wide_sw_* stages time the kernels of the conv slice predictors at 64 x 64, C = 256, B = 1 and 8: the
single 3x3 conv beside the PAIR call at the same shape (conv_pair_*), the whole-tensor z-score, the wide slice weights at
D = 256 (SliceLearner) and D = 384 (the code-conditioned MLP's last layer), M = 16; slice_predictor_iter one
slice_predictor_train_step (frozen SequenSolver T=10, layers=8, Tout=1; FusedAdamW) of VorticitySliceLearner and SliceLearner.
The darcy_loss stages time harness.darcy_loss (exp_darcy.py's loss) at s = 85, B = 4 (scripts/Transolver_Darcy.sh) and
s = 421, B = 2, forward alone and forward plus backward, through the fused kernels and through the torch path.
The block_tail stage times the fused block tail (split engine) at the same shape, beside the five kernels it
replaces (deslice, linear_bias_res, ln_fwd, linear_gelu, linear_bias_res, ln_fwd): useful GEMM TFLOP/s of the three linears.
Usage: python tools/kbench.py [--only conv_fwd,linear_fwd,...] [--iters 10] [--B 32]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerbasednavierstokesolver_amd import ops  # noqa: E402


def timeit(fn, iters):
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--engine", default=None, help="f32 | split | bf16 (default: PA2D_GEMM / split)")
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--MR", type=int, default=1, help="MLP ratio of the block_tail stage")
    ap.add_argument("--B3", type=int, default=1, help="batch of the conv3d_* stages (3x3x3 conv, S3^3 mesh, C channels)")
    ap.add_argument("--S3", type=int, default=32, help="edge of the cubic mesh of the conv3d_* stages")
    ap.add_argument("--AB", type=int, default=8, help="batch of the ae_* stages (auto_encoder.py's shape)")
    ap.add_argument("--AM", type=int, default=32, help="slices of the ae_* stages")
    ap.add_argument("--SB", type=int, default=8, help="batch of the seq_attn_* / code_sw_* stages (SequenSolver's shape)")
    args = ap.parse_args()
    E = ops.resolve_engine(args.engine)
    print(f"engine {E}  B={args.B} H={args.H} W={args.W} C={args.C} M={args.M}", flush=True)
    only = set(filter(None, args.only.split(",")))
    dev = "cuda:0"
    B, H, W, C, heads, M = args.B, args.H, args.W, args.C, args.heads, args.M
    N, D = H * W, C // heads
    R = B * N
    g = torch.Generator(device=dev).manual_seed(0)
    zeros = os.environ.get("KBENCH_ZEROS") == "1"      # all-zero operands: the same instruction stream at low switching power
    rn = (lambda *s: torch.zeros(*s, device=dev)) if zeros else (lambda *s: torch.randn(*s, device=dev, generator=g))
    xn = rn(B, N, C)
    wx, wf = rn(C, C, 3, 3) * 0.02, rn(C, C, 3, 3) * 0.02
    bx, bf = rn(C), rn(C)
    dout2 = rn(B, N, 2 * C)
    w, bias = rn(C, C) * 0.06, rn(C)
    x2d, dy2d, res = xn.view(R, C), rn(R, C), rn(R, C)
    ws, bs = rn(M, D) * 0.2, rn(M) * 0.1
    temp = torch.full((heads,), 0.5, device=dev)
    wq, wk, wv = rn(D, D) * 0.2, rn(D, D) * 0.2, rn(D, D) * 0.2
    xf = rn(B, N, 2 * C)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)

    conv_flops = 2.0 * R * 9 * C * 2 * C
    lin_flops = 2.0 * R * C * C
    tests = {}
    tests["conv_fwd"] = (lambda: ops.conv3x3x2_fwd(xn, wx, bx, wf, bf, H, W, engine=E), conv_flops, "TF")
    tests["conv_bwd"] = (lambda: ops.conv3x3x2_bwd(dout2, xn, wx, wf, H, W, engine=E), 2 * conv_flops, "TF")
    tests["conv_bwd_wonly"] = (lambda: ops.conv3x3x2_bwd(dout2, xn, wx, wf, H, W, need_dx=False, engine=E), conv_flops, "TF")
    # 3x3x3 conv of the structured 3-D mesh (pa2d_conv3x3x3x2_*): [B3*S3^3, 27C] x [27C, 2C]
    S3 = args.S3
    xn3, dout3 = rn(args.B3, S3 ** 3, C), rn(args.B3, S3 ** 3, 2 * C)
    wx3, wf3 = rn(C, C, 3, 3, 3) * 0.02, rn(C, C, 3, 3, 3) * 0.02
    conv3_flops = 2.0 * args.B3 * S3 ** 3 * 27 * C * 2 * C
    tests["conv3d_fwd"] = (lambda: ops.conv3x3x3x2_fwd(xn3, wx3, bx, wf3, bf, S3, S3, S3, engine=E), conv3_flops, "TF")
    tests["conv3d_bwd"] = (lambda: ops.conv3x3x3x2_bwd(dout3, xn3, wx3, wf3, S3, S3, S3, engine=E), 2 * conv3_flops, "TF")
    tests["conv3d_bwd_wonly"] = (lambda: ops.conv3x3x3x2_bwd(dout3, xn3, wx3, wf3, S3, S3, S3, need_dx=False, engine=E),
                                 conv3_flops, "TF")
    tests["linear_fwd"] = (lambda: ops.linear_fwd(x2d, w, bias, act="gelu", want_pre=True, engine=E), lin_flops, "TF")   # MLP1
    tests["linear_plain"] = (lambda: ops.linear_fwd(x2d, w, engine=E), lin_flops, "TF")
    tests["linear_bias_res"] = (lambda: ops.linear_fwd(x2d, w, bias, res=res, engine=E), lin_flops, "TF")
    tests["linear_gelu"] = (lambda: ops.linear_fwd(x2d, w, bias, act="gelu", engine=E), lin_flops, "TF")
    tests["linear_bwd_plain"] = (lambda: ops.linear_bwd_data(dy2d, w, engine=E), lin_flops, "TF")
    tests["linear_bwd_data"] = (lambda: ops.linear_bwd_data(dy2d, w, pre=x2d, act="gelu", engine=E), lin_flops, "TF")
    tests["linear_bwd_weight"] = (lambda: ops.linear_bwd_weight(dy2d, x2d, engine=E), lin_flops, "TF")
    y, mean, rstd = ops.layernorm_fwd(x2d, gamma, beta)
    tests["ln_fwd"] = (lambda: ops.layernorm_fwd(x2d, gamma, beta), 2.0 * R * C * 4, "GB")
    tests["ln_bwd"] = (lambda: ops.layernorm_bwd(dy2d, x2d, mean, rstd, gamma, res), 4.0 * R * C * 4, "GB")
    spart, npart = ops.slice_scatter(xf, 2 * C, 0, xf, 2 * C, C, ws, bs, temp, B, N, heads, D, M)
    s, nrm, o = ops.token_attn_fwd(spart, npart, wq, wk, wv)
    tests["slice_scatter"] = (lambda: ops.slice_scatter(xf, 2 * C, 0, xf, 2 * C, C, ws, bs, temp, B, N, heads, D, M),
                              2.0 * R * C * 4, "GB")
    tests["token_fwd"] = (lambda: ops.token_attn_fwd(spart, npart, wq, wk, wv), 0, "us")
    tests["deslice"] = (lambda: ops.deslice_fwd(xf, 2 * C, 0, o, ws, bs, temp, B, N, heads, D, M), 2.0 * R * C * 4, "GB")
    # the fused block tail (ops.block_tail_fwd, split engine) beside the five kernels it replaces (deslice, linear_bias_res,
    # ln_fwd, linear_gelu, linear_bias_res, ln_fwd): --MR is the MLP ratio; images made once, as inside a rollout
    if E == ops.ENGINE_SPLIT and ops.block_tail_supported(C, heads, D, M, args.MR * C, "gelu", E):
        hid = args.MR * C
        w1, b1, w2 = rn(hid, C) * 0.06, rn(hid), rn(C, hid) * 0.06
        tail = lambda: ops.block_tail_fwd(xf, 2 * C, 0, o, ws, bs, temp, res, w, bias, gamma, beta, w1, b1, w2, bias, gamma,
                                          beta, B, N, heads, D, M, "gelu", engine=E)
        with ops.weights_frozen() as tail_scope:      # holds the three weight images, made by the first (untimed) call
            pass

        def tail_timed():
            with ops.weights_frozen(tail_scope):
                return tail()
        tests["block_tail"] = (tail_timed, 2.0 * R * C * (C + 2 * hid), "TF")
    dy3 = dy2d.view(B, N, C)
    dopart, _ = ops.slice_scatter(xf, 2 * C, 0, dy3, C, 0, ws, bs, temp, B, N, heads, D, M, want_norm=False)
    ds, dn, *_ = ops.token_attn_bwd(s, nrm, wq, wk, wv, dopart)
    tests["token_bwd"] = (lambda: ops.token_attn_bwd(s, nrm, wq, wk, wv, dopart), 0, "us")
    tests["slice_bwd"] = (lambda: ops.slice_bwd_points(xf, dy3, ws, bs, temp, o, ds, dn, B, N, heads, D, M),
                          5.0 * R * C * 4, "GB")
    if E in (ops.ENGINE_SPLIT, ops.ENGINE_BF16) and ops.conv_planes_mask(B, H, W, C, E) == 7:
        nt = 3 if E == ops.ENGINE_SPLIT else 1
        # the forms the model runs on the bf16 engines: LayerNorm and the slice backward write the conv's plane image
        tests["ln_fwd_planes"] = (lambda: ops.layernorm_fwd_planes(x2d, gamma, beta, E), (1.0 + nt * 0.5) * R * C * 4, "GB")
        tests["slice_bwd_planes"] = (lambda: ops.slice_bwd_points_planes(xf, dy3, ws, bs, temp, o, ds, dn, nrm, B, N, heads, D, M, E),
                                     (3.0 + nt * 1.0) * R * C * 4, "GB")
    # auto-encoder attention at auto_encoder.py's shape: [AB, 4096, 64], 4 heads (D = 16), AM slices
    AB, AN, AC, AH, AM = args.AB, 64 * 64, 64, 4, args.AM
    AD = AC // AH
    axf = rn(AB, AN, 2 * AC)
    axm = axf[:, :, :AC]
    aws, abs_, atemp = rn(AM, AD) * 0.25, rn(AM) * 0.1, torch.full((AH,), 0.5, device=dev)
    asw = ops.slice_weights_fwd(axm, aws, abs_, atemp, AH)
    adsw, acode, ady = rn(AB, AH, AN, AM), rn(AB, AH, AM, AD), rn(AB, AN, AC)
    swb, actb = 4.0 * AB * AH * AN * AM, 4.0 * AB * AN * AC          # bytes of one [B,h,N,M] / one [B,N,C] tensor
    tests["ae_sw_fwd"] = (lambda: ops.slice_weights_fwd(axm, aws, abs_, atemp, AH), actb + swb, "HBM")
    tests["ae_sw_bwd"] = (lambda: ops.slice_weights_bwd(axm, aws, abs_, atemp, adsw), 2 * actb + swb, "HBM")
    tests["ae_dsw_fwd"] = (lambda: ops.deslice_weights_fwd(acode, asw), actb + swb, "HBM")
    tests["ae_dsw_bwd"] = (lambda: ops.deslice_weights_bwd(acode, asw, ady), actb + 2 * swb, "HBM")
    if only & {"ae_iter"}:
        from transformerbasednavierstokesolver_amd import harness
        from transformerbasednavierstokesolver_amd.model.Transolver_Structured_Mesh2D_Encoder import Model as AEModel
        from transformerbasednavierstokesolver_amd.optim import FusedAdamW
        torch.manual_seed(0)
        ae = AEModel(space_dim=2, n_layers=3, n_hidden=AC, n_head=AH, fun_dim=1, out_dim=1, slice_num=AM, H=64, W=64)
        ae = ae.to(dev).set_engine(E)
        aopt = FusedAdamW(ae.parameters(), lr=1e-3, weight_decay=1e-5, max_grad_norm=1.0)
        apos, afx = torch.rand(AB, AN, 2, device=dev), rn(AB, AN, 1)
        tests["ae_iter"] = (lambda: harness.autoencoder_train_step(ae, aopt, None, apos, afx, grad_sync=aopt.sync), 0, "us")
    # SequenSolver stages at the reference's shape: T=10 tokens of dim = 16 * 32; 4096 points, M=16, C=32
    SB, ST, SM, SC = args.SB, 10, 16, 32
    sdim = SM * SC
    sq, sk, sv, sdo = (rn(SB, ST, sdim) for _ in range(4))
    _, sattn = ops.seq_attn_fwd(sq, sk, sv, sdim ** -0.5)
    tests["seq_attn_fwd"] = (lambda: ops.seq_attn_fwd(sq, sk, sv, sdim ** -0.5, sq), 0, "us")
    tests["seq_attn_bwd"] = (lambda: ops.seq_attn_bwd(sq, sk, sv, sattn, sdo, sdim ** -0.5), 0, "us")
    scode, spos = rn(SB, SM, SC), torch.rand(SB, 4096, 2, device=dev)
    swp = (rn(64, SC + 2) * 0.2, rn(64) * 0.1, rn(64, 64) * 0.12, rn(64) * 0.1, rn(1, 64) * 0.25, rn(1))
    sdsw = rn(SB, 1, 4096, SM)
    csw_flops = 2.0 * SB * 4096 * SM * (64 * 64 + 64 * 3)            # the hidden layer, the two-coordinate point term and the last dot
    tests["code_sw_fwd"] = (lambda: ops.code_slice_weights_fwd(scode, spos, swp), csw_flops, "VALU")
    tests["code_sw_bwd"] = (lambda: ops.code_slice_weights_bwd(scode, spos, swp, sdsw), 3 * csw_flops, "VALU")
    # the merged model's head attention: SB samples x 16 heads of T=10 pseudo-rows of 32 floats
    HH, HS = 16, sdim // 16
    hx, hdo = rn(SB * HH, ST, HS), rn(SB * HH, ST, HS)
    hwq, hwk, hwv = rn(HS, HS) * 0.18, rn(HS, HS) * 0.18, rn(HS, HS) * 0.18
    _, hattn = ops.head_seq_attn_fwd(hx, hwq, hwk, hwv, sdim ** -0.5)
    tests["head_seq_attn_fwd"] = (lambda: ops.head_seq_attn_fwd(hx, hwq, hwk, hwv, sdim ** -0.5, hx), 0, "us")
    tests["head_seq_attn_bwd"] = (lambda: ops.head_seq_attn_bwd(hx, hwq, hwk, hwv, hattn, hdo, sdim ** -0.5), 0, "us")

    def unfused_fwd():
        q, k, v = (ops.linear_fwd(hx.view(-1, HS), w_, engine=E)[0].view(hx.shape) for w_ in (hwq, hwk, hwv))
        return q, k, v, ops.seq_attn_fwd(q, k, v, sdim ** -0.5, hx, causal=True)

    uq, uk, uv, (_, uattn) = unfused_fwd()

    def unfused_bwd():
        dq, dk, dv = ops.seq_attn_bwd(uq, uk, uv, uattn, hdo, sdim ** -0.5, causal=True)
        dx = None
        for d_, w_ in ((dq, hwq), (dk, hwk), (dv, hwv)):
            ops.linear_bwd_weight(d_.view(-1, HS), hx.view(-1, HS), want_bias=False, engine=E)
            t_ = ops.linear_bwd_data(d_.view(-1, HS), w_, engine=E)
            dx = t_ if dx is None else dx.add_(t_)
        return dx

    tests["head_seq_attn_fwd_unfused"] = (unfused_fwd, 0, "us")
    tests["head_seq_attn_bwd_unfused"] = (unfused_bwd, 0, "us")
    if only & {"merged_iter"}:
        import statistics
        from transformerbasednavierstokesolver_amd import harness
        from transformerbasednavierstokesolver_amd.SequenSolverMerged import SequenSolver as MergedSolver
        from transformerbasednavierstokesolver_amd.optim import FusedAdamW
        torch.manual_seed(0)
        mm = MergedSolver(None, T=ST, W=64, H=64, M=SM, C=SC, B=1, layers=8, sequential_head=HH).to(dev).set_engine(E)
        mopt = FusedAdamW(mm.parameters(), lr=1e-3, weight_decay=1e-5)
        mx, mfx, myy = torch.rand(1, 4096, 64, device=dev), rn(1, 4096, ST), rn(1, 4096, 1)
        step = lambda: harness.sequensolver_train_step(mm, mopt, None, mx, mfx, myy, use_gt=False, grad_sync=mopt.sync)
        runs = {True: [], False: []}
        for _ in range(10):                      # the two routes alternate, so that drift hits both alike
            for fused in (True, False):
                mm.fused = None if fused else False
                runs[fused].append(timeit(step, args.iters))
        for fused, ms in runs.items():
            print(f"merged_iter B=1 fused={fused}: median {statistics.median(ms):.3f} ms, range {min(ms):.3f} .. "
                  f"{max(ms):.3f} ms over {len(ms)} runs of {args.iters} iterations, in order: "
                  + " ".join(f"{t:.2f}" for t in ms), flush=True)
    if only & {"seq_iter"}:
        from transformerbasednavierstokesolver_amd import harness
        from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
        from transformerbasednavierstokesolver_amd.optim import FusedAdamW
        for sb in (1, 8):
            torch.manual_seed(0)
            sm = SequenSolver(None, T=ST, W=64, H=64, M=SM, C=SC, B=sb, layers=8).to(dev).set_engine(E)
            sopt = FusedAdamW(sm.parameters(), lr=1e-3, weight_decay=1e-5)
            sx, sfx, syy = torch.rand(sb, 4096, 2, device=dev), rn(sb, 4096, ST), rn(sb, 4096, 1)
            for gt in (True, False):
                tests[f"seq_iter B={sb} use_gt={gt}"] = (
                    lambda sm=sm, sopt=sopt, sx=sx, sfx=sfx, syy=syy, gt=gt: harness.sequensolver_train_step(
                        sm, sopt, None, sx, sfx, syy, use_gt=gt, grad_sync=sopt.sync), 0, "us")
    # LearnSlice at the reference's shape (64 x 64, M=16, C=32): the point-feature stage at P = 2 / 64 / 74 and B = 1 / 8,
    # and one frame of learnslice_train_step (target encode, get_code, forward, loss, backward, FusedAdamW step)
    for pp in (2, 64, 74):
        for sb in (1, 8):
            pcode, pfeat, pdsw = rn(sb, SM, SC), torch.rand(sb, 4096, pp, device=dev), rn(sb, 1, 4096, SM)
            pwp = (rn(64, SC + pp) * (2.0 / (SC + pp) ** 0.5), rn(64) * 0.1, rn(64, 64) * 0.12, rn(64) * 0.1,
                   rn(1, 64) * 0.25, rn(1))
            pfl = 2.0 * sb * 4096 * (SM * (64 * 64 + 64 * 2) + 64 * pp)      # rows: hidden layer, table add, last dot; points: W1p
            tests[f"point_sw_fwd P={pp} B={sb}"] = (
                lambda c=pcode, f=pfeat, w=pwp: ops.point_slice_weights_fwd(c, f, w), pfl, "VALU")
            tests[f"point_sw_bwd P={pp} B={sb}"] = (
                lambda c=pcode, f=pfeat, w=pwp, d=pdsw: ops.point_slice_weights_bwd(c, f, w, d), 3 * pfl, "VALU")
    if only & {"learnslice_iter"}:
        from transformerbasednavierstokesolver_amd import harness
        from transformerbasednavierstokesolver_amd.LearnSlice import LearnSlice
        from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
        from transformerbasednavierstokesolver_amd.optim import FusedAdamW
        for sb in (1, 8):
            torch.manual_seed(0)
            lseq = SequenSolver(None, T=ST, W=64, H=64, M=SM, C=SC, B=sb, layers=8).to(dev).set_engine(E).eval()
            for prm in lseq.parameters():
                prm.requires_grad = False
            lfx, lyy = rn(sb, 4096, ST), rn(sb, 4096, 1)
            for up, uv, pp in ((0, 0, 2), (1, 0, 64), (1, 1, 74)):
                lm = LearnSlice(up, uv).to(dev)
                lopt = FusedAdamW(lm.parameters(), lr=1e-3, weight_decay=1e-5)
                lx = torch.rand(sb, 4096, 64 if up else 2, device=dev)
                tests[f"learnslice_iter P={pp} B={sb}"] = (
                    lambda lm=lm, lopt=lopt, lseq=lseq, lx=lx, lfx=lfx, lyy=lyy, uv=uv: harness.learnslice_train_step(
                        lm, lopt, None, lseq, lx, lfx, lyy, uv, grad_sync=lopt.sync), 0, "us")
    # conv slice predictors at 64 x 64, C = 256 (SliceLearner.py; LearnSlice.forward_from_vorticity), B = 1 and 8; the pair
    # call at the same shape runs beside the single conv.  Operands are made only when one of these stages is asked for.
    PRED = {"conv3x3_fwd", "conv3x3_bwd", "conv_pair_fwd", "conv_pair_bwd", "zscore", "wide_sw_fwd", "wide_sw_bwd"}
    for sb in ((1, 8) if not only or any(n.split(" ")[0] in PRED for n in only) else ()):
        pr = sb * 4096
        pxn, pdo, pdo2 = rn(sb, 4096, 256), rn(sb, 4096, 256), rn(sb, 4096, 512)
        pw, pw2, pb = rn(256, 256, 3, 3) * 0.02, rn(256, 256, 3, 3) * 0.02, rn(256)
        cfl = 2.0 * pr * 9 * 256 * 256
        tests[f"conv3x3_fwd B={sb}"] = (lambda a=pxn, w=pw, b=pb: ops.conv3x3_fwd(a, w, b, 64, 64, engine=E), cfl, "TF")
        tests[f"conv3x3_bwd B={sb}"] = (lambda d=pdo, a=pxn, w=pw: ops.conv3x3_bwd(d, a, w, 64, 64, engine=E), 2 * cfl, "TF")
        tests[f"conv_pair_fwd B={sb}"] = (lambda a=pxn, w=pw, v=pw2, b=pb: ops.conv3x3x2_fwd(a, w, b, v, b, 64, 64, engine=E),
                                          2 * cfl, "TF")
        tests[f"conv_pair_bwd B={sb}"] = (lambda d=pdo2, a=pxn, w=pw, v=pw2: ops.conv3x3x2_bwd(d, a, w, v, 64, 64, engine=E),
                                          4 * cfl, "TF")
        zy, zst = ops.zscore_fwd(pxn)
        tests[f"zscore fwd B={sb}"] = (lambda a=pxn: ops.zscore_fwd(a), 3.0 * pr * 256 * 4, "HBM")       # x twice, y once
        tests[f"zscore bwd B={sb}"] = (lambda d=pdo, y=zy, st=zst: ops.zscore_bwd(d, y, st), 5.0 * pr * 256 * 4, "HBM")
        ptemp = torch.full((1,), 0.5, device=dev)
        for dd in (256, 384):
            wxx, wws, wbs, wds = rn(sb, 4096, dd), rn(16, dd) * (1.0 / dd ** 0.5), rn(16) * 0.1, rn(sb, 4096, 16)
            wbytes = 4.0 * pr * (dd + 16)
            tests[f"wide_sw_fwd D={dd} B={sb}"] = (lambda a=wxx, w=wws, b=wbs: ops.wide_slice_weights_fwd(a, w, b, ptemp),
                                                   wbytes, "HBM")
            tests[f"wide_sw_bwd D={dd} B={sb}"] = (lambda a=wxx, w=wws, b=wbs, d=wds: ops.wide_slice_weights_bwd(a, w, b, ptemp, d),
                                                   4.0 * pr * (3 * dd + 2 * 16), "HBM")     # x (kernel + GEMM), dx, dsw, dl
    if only & {"zscore_grouped"}:      # a folded iteration's z-score: 10 calls x 4096 rows x 256, one launch pair against ten
        gx, gd = rn(10 * 4096, 256), rn(10 * 4096, 256)
        gy, gst = ops.zscore_grouped_fwd(gx, 10)
        parts = [(gx[k * 4096:(k + 1) * 4096], gd[k * 4096:(k + 1) * 4096]) + ops.zscore_fwd(gx[k * 4096:(k + 1) * 4096])
                 for k in range(10)]
        gbytes = 10 * 4096 * 256 * 4.0
        tests["zscore_grouped fwd 10x4096x256"] = (lambda: ops.zscore_grouped_fwd(gx, 10), 3.0 * gbytes, "HBM")
        tests["zscore_grouped fwd 10 ungrouped calls"] = (lambda: [ops.zscore_fwd(p[0]) for p in parts], 3.0 * gbytes, "HBM")
        tests["zscore_grouped bwd 10x4096x256"] = (lambda: ops.zscore_grouped_bwd(gd, gy, gst), 5.0 * gbytes, "HBM")
        tests["zscore_grouped bwd 10 ungrouped calls"] = (lambda: [ops.zscore_bwd(p[1], p[2], p[3]) for p in parts],
                                                          5.0 * gbytes, "HBM")
    if only & {"slice_predictor_iter"}:
        from transformerbasednavierstokesolver_amd import harness
        from transformerbasednavierstokesolver_amd.SequenSolver import SequenSolver
        from transformerbasednavierstokesolver_amd.SliceLearner import SliceLearner, VorticitySliceLearner
        from transformerbasednavierstokesolver_amd.optim import FusedAdamW
        for sb in (1, 8):
            torch.manual_seed(0)
            pseq = SequenSolver(None, T=ST, W=64, H=64, M=SM, C=SC, B=sb, layers=8).to(dev).set_engine(E).eval()
            for prm in pseq.parameters():
                prm.requires_grad = False
            px, pfx, pyy = torch.rand(sb, 4096, 2, device=dev), rn(sb, 4096, ST), rn(sb, 4096, 1)
            for label, pm in (("vorticity", VorticitySliceLearner(0, True)),
                              ("slicelearner", SliceLearner(space_dim=2, fun_dim=ST, H=64, W=64, slice_num=SM))):
                pm = pm.to(dev).set_engine(E)
                popt = FusedAdamW(pm.parameters(), lr=1e-3, weight_decay=1e-5)
                tests[f"slice_predictor_iter {label} B={sb}"] = (
                    lambda pm=pm, popt=popt, pseq=pseq, px=px, pfx=pfx, pyy=pyy: harness.slice_predictor_train_step(
                        pm, popt, None, pseq, px, pfx, pyy, grad_sync=popt.sync), 0, "us")
    if not only or only & {"darcy_loss"}:
        from transformerbasednavierstokesolver_amd import harness, synth
        from transformerbasednavierstokesolver_amd.utils.normalizer import UnitTransformer
        for ds, db in ((85, 4), (421, 2)):
            _, _, dsol = synth.darcy_batch(db, ds, seed=3)
            dsol = torch.from_numpy(dsol).to(dev)
            dyn = UnitTransformer(dsol)
            dy_n = dyn.encode(dsol)
            dout_n = (dy_n + 0.1 * rn(db, ds * ds)).requires_grad_(True)
            dbytes = 2.0 * db * ds * ds * 4                       # forward: out_n and y_n once; backward: + d out_n

            def dl_fwd(fused, o=dout_n, y=dy_n, n=dyn, s=ds):
                with torch.no_grad():
                    return harness.darcy_loss(o, y, n, 1.0 / s, s, fused=fused)

            def dl_fwd_bwd(fused, o=dout_n, y=dy_n, n=dyn, s=ds):
                o.grad = None
                harness.darcy_loss(o, y, n, 1.0 / s, s, fused=fused)[0].backward()

            for label, fused in (("fused", True), ("torch", False)):
                tests[f"darcy_loss {label} fwd s={ds} B={db}"] = (lambda f=dl_fwd, u=fused: f(u), dbytes, "HBM")
                tests[f"darcy_loss {label} fwd+bwd s={ds} B={db}"] = (lambda f=dl_fwd_bwd, u=fused: f(u), 2.5 * dbytes, "HBM")
    for name, (fn, work, unit) in tests.items():
        if only and name not in only and name.split(" ")[0] not in only:
            continue
        ms = timeit(fn, args.iters)
        if unit == "TF":
            print(f"{name:20s} {ms:9.3f} ms  {work / ms / 1e9:8.1f} TFLOP/s  ({work / ms / 1e9 / 157.3:.3f} of fp32 MFMA peak)", flush=True)
        elif unit == "HBM":
            print(f"{name:20s} {ms * 1e3:9.1f} us  {work / ms / 1e6:8.0f} GB/s  ({work / ms / 1e9 / 8.0:.3f} of 8 TB/s HBM)",
                  flush=True)
        elif unit == "VALU":
            print(f"{name:20s} {ms * 1e3:9.1f} us  {work / ms / 1e9:8.1f} TFLOP/s useful fp32 (FMA = 2)", flush=True)
        elif unit == "GB":
            print(f"{name:20s} {ms:9.3f} ms  {work / ms / 1e6:8.0f} GB/s algorithmic", flush=True)
        else:
            print(f"{name:20s} {ms * 1e3:9.1f} us", flush=True)


if __name__ == "__main__":
    main()
