"""tools/isa_count.py --cover: how many MFMAs lie between an LDS fragment read and the s_waitcnt that retires it.

Host only.  The synthetic case pins the tool's rules (in-order retirement, a read burst, a wait inside a loop whose read
was issued in the previous iteration); the two hipcc cases audit the halo conv's 16x16x32 consumers: the loop that reads
its fragments ahead (conv_halo_kernel<3, float, 1, true>) and the reference loop (conv_halo_ref_kernel, PA2D_CONV_AHEAD=0).
"""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transformerbasednavierstokesolver_amd", "csrc")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_count", os.path.join(ROOT, "tools", "isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MFMA = "\tv_mfma_f32_16x16x32_bf16 v[20:23], v[0:3], v[4:7], v[20:23]"
SYNTHETIC = "\n".join([
    "_Z3fooPf:                                ; @_Z3fooPf",
    "\ts_load_dwordx2 s[0:1], s[4:5], 0x0",
    "\ts_waitcnt lgkmcnt(0)",                    # retires a scalar load only: not a fragment wait
    "\tds_read_b128 v[0:3], v40",                # burst of three reads: A, B, C
    "\tds_read_b128 v[4:7], v40 offset:64",
    "\tds_read_b128 v[8:11], v40 offset:128",
    MFMA,
    "\ts_waitcnt lgkmcnt(2)",                    # retires A: cover 1
    MFMA,
    MFMA,
    "\ts_waitcnt lgkmcnt(1)",                    # retires B: cover 3
    "\ts_waitcnt lgkmcnt(1)",                    # retires nothing
    "\ts_waitcnt lgkmcnt(0)",                    # retires C: cover 3
    ".LBB0_1:                                ; =>This Inner Loop Header: Depth=1",
    "\ts_waitcnt lgkmcnt(0)",                    # steady state: retires Y and Z of the previous iteration: cover 2
    MFMA,
    "\tds_read_b128 v[0:3], v41",                # X
    "\tds_write_b128 v42, v[12:15]",             # Y: a write queues behind X
    MFMA, MFMA, MFMA, MFMA,
    "\ts_waitcnt lgkmcnt(1)",                    # in order: retires X only, cover 4
    MFMA,
    "\ts_waitcnt vmcnt(0)",                      # no lgkmcnt field
    "\tds_read_b128 v[4:7], v41 offset:64",      # Z
    MFMA, MFMA,
    "\ts_cbranch_scc1 .LBB0_1",
    "; %bb.2:",
    "\ts_endpgm",
    ".Lfunc_end0:",
])


def test_cover_synthetic_listing():
    lines = SYNTHETIC.split("\n")
    assert len(lines) <= 35
    rep = _tool().cover_report(lines, "fooPf")
    assert [r["loop"] for r in rep] == ["kernel", ".LBB0_1"]
    kernel, loop = rep
    assert kernel["mfma"] == 11 and kernel["covers"] == [1, 3, 3, 4]      # one linear pass: the loop's first wait finds nothing
    assert loop["mfma"] == 8 and loop["covers"] == [2, 4]                 # second pass of the loop
    assert _tool().cover_report(lines, "no_such_kernel") is None


@pytest.fixture(scope="module")
def conv_halo_listing(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "pa2d_conv_halo.s"
    # the Makefile's code-generation flags
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "pa2d_conv_halo.hip"), "-o", str(out)], check=True, cwd=CSRC,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out.read_text().split("\n")


def _stage_loop(rep):
    loops = [r for r in rep if r["loop"] != "kernel" and r["mfma"] == 192]      # one weight stage = 192 MFMAs per wave
    assert loops, rep
    return loops[0]


def test_conv_halo_ahead_loop_has_no_wait_under_8_mfmas(conv_halo_listing):
    """Every steady-state wait of the new consumer loop that retires a fragment read has >= 8 MFMAs of cover.  No wait is
    exempted: the first A read after a halo swap is issued behind the second barrier with 12 MFMAs still to run (the
    issue allowed exempting it).  The walk includes the chunk-boundary barrier's own wait in every pass."""
    loop = _stage_loop(_tool().cover_report(conv_halo_listing, "conv_halo_kernelILi3EfLi1ELb1E"))
    print("ahead loop covers:", sorted(loop["covers"]))
    assert loop["covers"] and min(loop["covers"]) >= 8


def test_conv_halo_reference_loop_has_five_zero_cover_waits(conv_halo_listing):
    """The "before": the compiler's own order drains the pipe five times per stage."""
    loop = _stage_loop(_tool().cover_report(conv_halo_listing, "conv_halo_ref_kernel"))
    print("reference loop covers:", sorted(loop["covers"]))
    assert sum(c == 0 for c in loop["covers"]) == 5
    assert len(loop["covers"]) == 22
