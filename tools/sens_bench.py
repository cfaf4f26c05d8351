#!/usr/bin/env python3
"""What the sensitivity sweep costs: rmt_n2_steady_sens against rmt_n2_steady_march on the same rows, and against the
2 NP extra marches a central difference per parameter would take - that figure is an extrapolation, 2 NP times the
measured time of one cold march, not a measured differencing run (profiles/sensitivity.md).

For E members (a T/P sweep around the DME notebook input) of N nodes and NP = 1, 4, 8 parameters (the coolant temperature,
the inlet temperature, the inlet pressure, then feed components): the kernel times (rmt_n2_last_kernel_ms; one warm-up
launch, then the median of `--repeat`) of the march and of the sweep on a handle of the sensitivity unit (n2.sens_plan),
and the registers, spills and scratch of the two kernels in that gfx950 code object.  Needs a GPU.  One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--nodes", type=int, nargs="+", default=[20])
    ap.add_argument("--parameters", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    import torch  # noqa: F401
    import inputs as INP
    from rmt_app_amd import isa, n2, plan, sensitivity
    from rmt_app_amd.ensemble import expand_members
    base = INP.dme_notebook_input(ivp="hip-ros4")
    comps = base["feed"]["components"]["shell"]
    every = ["medium-temperature", "inlet-temperature", "inlet-pressure"] + [{"inlet-concentration": c} for c in comps]
    for N in a.nodes:
        for E in a.members:
            nT = max(1, int(round(E**0.5)))
            members = [base] if E == 1 else expand_members(base, {"temperature": list(np.linspace(518.0, 528.0, nT)),
                                                                  "pressure": list(np.linspace(4.8e6, 5.2e6, E//nT))})
            mech = n2.mechanism_for(base, members, base["solver-config"])
            pairs = [plan.member_constants(m, mech, N) for m in members]
            rows = np.array([r for _, r in pairs])
            IV = plan.initial_states([nm for nm, _ in pairs], mech, N)
            for NP in a.parameters:
                spec = dict(base, **{"solver-config": dict(base["solver-config"], initial="steady",
                                                           sensitivity={"parameters": every[:NP]})})
                sens = sensitivity.parse(spec)
                kinds, idx = sens.descriptors(mech)
                cp = n2.sens_plan(mech, N, NP, None, rows)
                code = n2.compile_plan(mech, False, cp, n2.device_arch())
                out = {"members": len(rows), "nodes": N, "parameters": NP,
                       "resources": {k: isa.kernel_resources(code, k) for k in ("rmt_n2_steady_march", "rmt_n2_steady_sens")}}
                dev = n2.N2Device(mech, rows, N, block=cp.block, npt=cp.npt, defines=cp.defines, specialize=False,
                                  features=cp.features)
                try:
                    ms = []
                    for _ in range(a.repeat + 1):
                        y = dev.to_device(IV)
                        dev.steady_march(y)
                        ms.append(dev.last_kernel_ms())
                    st, flags = dev.march_result()
                    assert not np.any(flags), flags
                    out.update({"march_ms": float(np.median(ms[1:])), "march_ms_all": ms[1:],
                                "march_iterations": int(st["iterations"].max())})
                    ms = []
                    for _ in range(a.repeat + 1):
                        raw = dev.steady_sens(y, kinds, idx)
                        ms.append(dev.last_kernel_ms())
                    assert not np.any(dev.sens_status()) and bool(torch.isfinite(raw).all())
                    out.update({"sens_ms": float(np.median(ms[1:])), "sens_ms_all": ms[1:]})
                    out["sens_over_march"] = out["sens_ms"]/out["march_ms"]
                    out["differencing_ms"] = 2*NP*out["march_ms"]             # extrapolated: 2 NP x ONE measured march
                    out["differencing_over_sens"] = out["differencing_ms"]/out["sens_ms"]
                finally:
                    dev.close()
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
