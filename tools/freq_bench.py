#!/usr/bin/env python3
"""What the frequency sweep costs: rmt_n2_steady_freq against the rmt_n2_steady_march that precedes it, on the same rows
(profiles/frequency_response.md).

For E members (a T/P sweep around the DME notebook input) of N nodes, F log-spaced frequencies and NP = 1, 4 inputs (the
coolant temperature, then the inlet temperature, the inlet pressure and the CO feed): the kernel times
(rmt_n2_last_kernel_ms; one warm-up launch, then the median of `--repeat`) of the march and of the sweep - E F lanes - on a
handle of the frequency unit (n2.freq_plan), and the registers, spills and scratch of the kernels in that gfx950 code
object.  The sweep's time is the kernel's alone: the upload of the frequencies and the copy of the result are outside the
two events.  No forced transient is run here, so no cost of that alternative is given.  Needs a GPU.  One JSON line per
shape."""
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
    ap.add_argument("--frequencies", type=int, default=32)
    ap.add_argument("--inputs", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    import torch  # noqa: F401
    import inputs as INP
    from rmt_app_amd import frequency, isa, n2, plan
    from rmt_app_amd.ensemble import expand_members
    base = INP.dme_notebook_input(ivp="hip-ros4")
    every = ["medium-temperature", "inlet-temperature", "inlet-pressure", {"inlet-concentration": "CO"}]
    for N in a.nodes:
        for E in a.members:
            nT = max(1, int(round(E**0.5)))
            members = [base] if E == 1 else expand_members(base, {"temperature": list(np.linspace(518.0, 528.0, nT)),
                                                                  "pressure": list(np.linspace(4.8e6, 5.2e6, E//nT))})
            mech = n2.mechanism_for(base, members, base["solver-config"])
            pairs = [plan.member_constants(m, mech, N) for m in members]
            rows = np.array([r for _, r in pairs])
            named = [nm for nm, _ in pairs]
            IV = plan.initial_states(named, mech, N)
            for NP in a.inputs:
                spec = dict(base, **{"solver-config": dict(base["solver-config"], initial="steady", **{
                    frequency.KEY: {"inputs": every[:NP], "frequencies": {"range": [1e-2, 1e2], "points": a.frequencies}}})})
                fr = frequency.parse(spec)
                kinds, idx = fr.descriptors(mech)
                cp = n2.freq_plan(mech, N, NP, None, rows)
                code = n2.compile_plan(mech, False, cp, n2.device_arch())
                out = {"members": len(rows), "nodes": N, "frequencies": fr.F, "inputs": NP, "lanes": len(rows)*fr.F,
                       "resources": {k: isa.kernel_resources(code, k) for k in ("rmt_n2_steady_march", "rmt_n2_steady_freq")}}
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
                    Yh = y.cpu().numpy()
                    peaks = [frequency.peak_node(Yh[e], mech, named[e]) for e in range(len(rows))]
                    ms = []
                    for _ in range(a.repeat + 1):
                        got, _, failed = dev.steady_freq(y, kinds, idx, fr.omegas, peaks, False)
                        ms.append(dev.last_kernel_ms())
                    assert not np.any(dev.freq_status()) and np.all(failed == -1) and np.all(np.isfinite(got))
                    out.update({"freq_ms": float(np.median(ms[1:])), "freq_ms_all": ms[1:]})
                    out["freq_over_march"] = out["freq_ms"]/out["march_ms"]
                    out["freq_us_per_lane_node"] = 1e3*out["freq_ms"]/(out["lanes"]*N)
                finally:
                    dev.close()
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
