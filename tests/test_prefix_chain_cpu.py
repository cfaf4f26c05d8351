"""CPU-only: the cross-wave part of the pressure scan with one LDS round trip per batch of records (RMT_PREFIX_MODE 4,
csrc/kernels/25_prefix.inc; profiles/prefix_chain.md).  The static conditions on the cross-compiled
bench code object - from the hipRTC bundled with PyTorch, hence measured in a process of its own
(tests/helpers/prefix_chain_isa.py) -, a one-wave unit that must compile to what it compiled to before, and the functions
themselves on the host (tests/helpers/prefix_chain_emu.cpp): the batched form against the scalar loop and the plain loop,
bit for bit, for 1, 4 and 8 waves and every wave index; once more under AddressSanitizer and UBSan."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "helpers")
PREFIX_INC = os.path.join(ROOT, "rmt_app_amd", "csrc", "kernels", "25_prefix.inc")
# rmt_n2_rk4_reg of the 64 x 1 caching unit (256 copies of the notebook's row, 20 nodes) BEFORE this change, from the
# same compiler: step-loop counts and the digest of the kernel's mnemonic sequence
ONE_WAVE_BEFORE = {"instructions": 3077, "valu": 2109, "valu_f64": 1446, "rcp_f64": 11, "salu": 805, "lds": 163,
                   "scratch": 0, "lane_moves": 0}
ONE_WAVE_DIGEST_BEFORE = "7040bfb296ef7fdc6ed3b83c"


@pytest.fixture(scope="module")
def figures():
    out = subprocess.run([sys.executable, os.path.join(HELPERS, "prefix_chain_isa.py")], capture_output=True, text=True,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    fig = json.loads(out.stdout.strip().split("\n")[-1])
    assert "torch" in fig["hiprtc"], fig["hiprtc"]            # the bundled hipRTC: the figures below are its
    return fig


def test_bench_code_object_static_conditions(figures):
    """The bench unit's default: at most two waits for LDS on any wave's way from the barrier to its entering pressure
    (all five RHS evaluations of the step loop), no more scratch, registers, LDS or VALU than before: 3280 + 16."""
    b = figures["bench"]
    st, res = b["step_loop"], b["resources"]
    print("bench unit:", b["kernel_digest"], st, res, b["barriers"])
    assert len(b["barriers"]) == 5
    for k, bar in enumerate(b["barriers"]):
        assert bar["max_fmas"] == 7, k                        # the walk saw the whole chain of wave 7
        assert bar["max_lds_waits"] <= 2, k
    assert st["scratch"] <= 2
    assert res["vgpr_count"] <= 256
    assert res["group_segment_fixed_size"] == 161072
    assert st["valu"] <= 3280 + 16


def test_the_walk_tells_the_scalar_loop_apart(figures):
    """The same unit with RMT_PREFIX_MODE=2: the walk meets the scalar loop (a wait per trip) behind every barrier."""
    m2 = figures["bench_mode2"]
    print("mode 2:", m2["kernel_digest"], m2["step_loop"], m2["barriers"])
    assert m2["kernel_digest"] != figures["bench"]["kernel_digest"]
    assert len(m2["barriers"]) == 5
    assert all(bar["max_lds_waits"] > 7 for bar in m2["barriers"])
    assert m2["resources"]["group_segment_fixed_size"] == 161072


def test_one_wave_unit_compiles_to_what_it_did(figures):
    o = figures["one_wave"]
    print("64 x 1:", o["kernel_digest"], o["step_loop"])
    assert {k: o["step_loop"][k] for k in ONE_WAVE_BEFORE} == ONE_WAVE_BEFORE
    assert o["kernel_digest"] == ONE_WAVE_DIGEST_BEFORE
    assert o["resources"]["group_segment_fixed_size"] == 14912 and o["resources"]["vgpr_count"] == 112


def test_only_the_bench_unit_gets_the_batched_form(figures):
    """n2.code_plan writes RMT_PREFIX_MODE 4 into the defines of the caching one-workgroup RK4 unit at 512 x 2 and of no
    other: not the RK45 unit of the same geometry (the adaptive_rk45 row of `bench.py --full`, whose rmt_n2_rk45_reg is
    instruction for instruction that of its RMT_PREFIX_MODE=2 twin), not a unit with the stiff stepper, not another
    geometry, model or precision; a caller's own value stands."""
    import numpy as np
    import inputs as INP
    from rmt_app_amd import n2, plan
    dme = plan.Mechanism(INP.dme_notebook_input())
    _, row = plan.member_constants(INP.dme_notebook_input(), dme, 1024)
    rows = np.tile(row, (4, 1))
    mode = lambda **kw: n2.code_plan(dme, kw.pop("N", 1024), rows=rows, **kw).defines.get("RMT_PREFIX_MODE")
    assert mode(block=512, npt=2) == "4" and mode(N=899, block=512, npt=2) == "4"
    assert mode(defines={"RMT_PREFIX_MODE": "2"}) == "2"
    b45, n45, d45 = n2.rk45_geometry(dme.V, 1024, E=256)
    assert (b45, n45) == (512, 2) and mode(block=b45, npt=n45, defines=d45) is None
    assert mode(block=512, npt=2, features=("ros4",)) is None
    assert mode(block=512, npt=2, defines={"RMT_KCACHE": "0"}) is None
    assert mode(N=4096, block=512, npt=2) is None                      # chained
    assert mode(N=200, block=256, npt=1) is None and mode(N=20, block=64, npt=1) is None
    assert mode(block=512, npt=2, fp32=True) is None
    m2 = plan.Mechanism(INP.m2_dme_input())
    _, r2 = plan.member_constants_m2(INP.m2_dme_input(), m2, 1024)
    assert n2.code_plan(m2, 1024, block=512, npt=2, rows=np.tile(r2, (4, 1))).defines.get("RMT_PREFIX_MODE") is None
    a, b = figures["rk45"], figures["rk45_mode2"]
    print("rk45 unit:", a["kernel_digest"], a["step_loop"])
    assert a["kernel_digest"] == b["kernel_digest"] and a["step_loop"] == b["step_loop"] and a["resources"] == b["resources"]


def _build(tmp, nw, extra=(), tag=""):
    exe = os.path.join(tmp, "prefix_chain_%d%s" % (nw, tag))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DRMT_NW=%d" % nw,
                    "-DRMT_PREFIX_SOURCE=\"%s\"" % PREFIX_INC, *extra, os.path.join(HELPERS, "prefix_chain_emu.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("nw", [1, 4, 8])
def test_batched_prefix_on_the_host_bit_for_bit(nw, tmp_path):
    out = subprocess.run([_build(str(tmp_path), nw)], capture_output=True, text=True)
    print(out.stdout.strip())
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ok", str(2000*nw*4)]


def test_batched_prefix_on_the_host_under_sanitizers(tmp_path):
    """the stand-alone program itself, built with -fsanitize=address,undefined and run directly (the totals are a heap
    block of exactly RMT_NW records: a batch reading past the last one would be reported)"""
    exe = _build(str(tmp_path), 8, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "_san")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ok", str(2000*8*4)]
