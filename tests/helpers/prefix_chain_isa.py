"""TEST HELPER (run as a program by tests/test_prefix_chain_cpu.py): cross-compiles the bench code object, its twin with
RMT_PREFIX_MODE=2, a one-wave unit and the RK45 unit of the bench geometry (with its RMT_PREFIX_MODE=2 twin) with the
hipRTC bundled with PyTorch - the one every GPU run loads; a process uses whichever hipRTC it loaded first, hence a process of its own that imports torch before the library - and prints one
JSON object: per unit the step-loop instruction mix and the resources of rmt_n2_rk4_reg (rmt_app_amd/isa.py), and per
`s_barrier` of the step loop what lies between it and the end of the cross-wave pressure chain (chain_paths)."""
import json
import os
import sys

import torch  # noqa: F401  (first: its hipRTC is the one the library then binds)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import inputs as INP  # noqa: E402
from rmt_app_amd import hipbind, isa, n2, plan  # noqa: E402
from rmt_app_amd.ensemble import DistributedEnsemble  # noqa: E402

KERNEL = "rmt_n2_rk4_reg"
UNBOUNDED = 10**6


def _in_chain(op):
    """Instructions the stretch between the barrier and the end of the chain is made of: LDS reads, waits, the fmas and
    the moves around them, scalar compares / branches / arithmetic.  Anything else (the lane-0 block's s_and_saveexec, the
    node function's arithmetic) ends the stretch."""
    if op.startswith("s_"):
        return not (op in ("s_barrier", "s_endpgm") or "saveexec" in op or op.startswith(("s_load", "s_buffer")))
    return op.startswith(("ds_read", "v_mov_b", "v_fmac_f64", "v_fma_f64"))


def chain_paths(ins, labels, start):
    """Every path from instruction index `start` to the end of the stretch: (s_waitcnt that wait for LDS, fp64 fmas) per
    path; a path that comes back to an instruction it has passed (a loop: one wait per trip) counts UNBOUNDED waits."""
    index = {a: i for i, (a, _, _) in enumerate(ins)}
    out = []

    def target(args):
        return index[labels[args.split()[-1].strip("<>")]]

    def go(i, seen, waits, fmas):
        while True:
            if i >= len(ins) or not _in_chain(ins[i][1]):
                out.append((waits, fmas))
                return
            if i in seen:
                out.append((UNBOUNDED, fmas))
                return
            seen = seen | {i}
            _, op, args = ins[i]
            if op == "s_waitcnt" and "lgkmcnt" in args:
                waits += 1
            if op.startswith(("v_fmac_f64", "v_fma_f64")):
                fmas += 1
            if op == "s_branch":
                i = target(args)
                continue
            if op.startswith("s_cbranch"):
                go(target(args), seen, waits, fmas)
            i += 1

    go(start, frozenset(), 0, 0)
    return out


def figures(blob, KERNEL=KERNEL):
    st = isa.kernel_stats(blob, KERNEL)
    ins, labels = isa.disassemble(blob, KERNEL)
    # the step loop as isa.kernel_stats finds it: the backward branch with the longest span
    best = None
    for a, op, args in ins:
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(args.split()[-1].strip("<>")) if args else None
            if t is not None and t < a and (best is None or a - t > best[1] - best[0]):
                best = (t, a)
    barriers = []
    for i, (a, op, _) in enumerate(ins):
        if op == "s_barrier" and best and best[0] <= a <= best[1]:
            paths = chain_paths(ins, labels, i + 1)
            barriers.append({"max_lds_waits": max(w for w, _ in paths), "max_fmas": max(f for _, f in paths),
                             "paths": len(paths)})
    return {"kernel_digest": st["kernel_digest"], "step_loop": st["step_loop"],
            "resources": isa.kernel_resources(blob, KERNEL), "barriers": barriers}


def bench_blob(defines):
    inputs = bench.sweep_member_inputs(0, bench.MEMBERS_PER_GPU, total=max(2048, bench.MEMBERS_PER_GPU))
    mech = plan.Mechanism(inputs[0])
    ens = DistributedEnsemble(mech, inputs, bench.N_NODES, compile_fn=lambda mdef: n2.compile_mechanism(
        mech, bench.N_NODES, defines={**defines, **mdef}, E=bench.MEMBERS_PER_GPU))
    return ens.code


def one_wave_blob():
    dme = plan.Mechanism(INP.dme_notebook_input())
    _, row = plan.member_constants(INP.dme_notebook_input(), dme, 20)
    block, npt, defs, src, key = n2.device_source(dme, np.tile(row, (256, 1)), 20, block=64, npt=1)
    assert (block, npt) == (64, 1) and defs.get("RMT_KCACHE") == "1"
    return hipbind.compile_cached(src, key, "gfx950", n2.compile_options(block, npt, (), "", defs))


def rk45_blob(defines):
    """the unit behind the adaptive_rk45 row of `bench.py --full`: the sweep's members at rk45_geometry (512 x 2 there)"""
    inputs = bench.sweep_member_inputs(0, bench.MEMBERS_PER_GPU, total=max(2048, bench.MEMBERS_PER_GPU))
    mech = plan.Mechanism(inputs[0])
    rows = np.array([plan.member_constants(mi, mech, bench.N_NODES)[1] for mi in inputs])
    block, npt, defs = n2.rk45_geometry(mech.V, bench.N_NODES, E=bench.MEMBERS_PER_GPU)
    assert (block, npt) == (512, 2)
    cp = n2.code_plan(mech, bench.N_NODES, block=block, npt=npt, defines={**defs, **defines}, rows=rows)
    assert cp.defines.get("RMT_KCACHE") == "1" and cp.defines.get("RMT_PREFIX_MODE") == defines.get("RMT_PREFIX_MODE")
    return n2.compile_plan(mech, False, cp)


if __name__ == "__main__":
    print(json.dumps({"hiprtc": os.path.realpath(hipbind.lib().rmt_n2_hiprtc_path().decode()),
                      "bench": figures(bench_blob({})),
                      "bench_mode2": figures(bench_blob({"RMT_PREFIX_MODE": "2"})),
                      "one_wave": figures(one_wave_blob()),
                      "rk45": figures(rk45_blob({}), "rmt_n2_rk45_reg"),
                      "rk45_mode2": figures(rk45_blob({"RMT_PREFIX_MODE": "2"}), "rmt_n2_rk45_reg")}))
