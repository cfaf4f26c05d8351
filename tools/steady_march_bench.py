#!/usr/bin/env python3
"""What the steady-state march costs against what it replaces (profiles/steady_march.md).

For E members (a T/P sweep around the DME notebook input) of N nodes: the kernel time of rmt_n2_steady_march
(rmt_n2_last_kernel_ms; one warm-up launch, then the median of `--repeat`), and next to it the alternative a user has
without the key - the stiff stepper from the cold start, in legs of 1 s of model time, until max|dy/dt| (rmt_n2_rhs) is
down to what the march left (host clock around launches that end in a synchronise; at most `--budget` seconds of wall
per shape, the figure reached is printed either way).  Needs a GPU.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 256, 2048])
    ap.add_argument("--nodes", type=int, nargs="+", default=[20, 1024])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--budget", type=float, default=40.0)
    ap.add_argument("--no-transient", action="store_true")
    a = ap.parse_args()
    import torch
    import inputs as INP
    from rmt_app_amd import n2, plan
    from rmt_app_amd.ensemble import expand_members
    from rmt_app_amd.settings import DEVICE_DEFAULTS
    base = INP.dme_notebook_input(ivp="hip-ros4")
    for N in a.nodes:
        for E in a.members:
            nT = max(1, int(round(E**0.5)))
            members = [base] if E == 1 else expand_members(base, {"temperature": list(np.linspace(518.0, 528.0, nT)),
                                                                  "pressure": list(np.linspace(4.8e6, 5.2e6, E//nT))})
            mech = n2.mechanism_for(base, members, base["solver-config"])
            pairs = [plan.member_constants(m, mech, N) for m in members]
            rows = np.array([r for _, r in pairs])
            IV = plan.initial_states([nm for nm, _ in pairs], mech, N)
            out = {"members": len(members), "nodes": N}
            dev = n2.N2Device(mech, rows, N, block=n2.ros4_block(mech.V, N), npt=1, features=("ros4",)).attach_march()
            try:
                y = dev.to_device(IV)
                ms = []
                for k in range(a.repeat + 1):
                    y.copy_(dev.to_device(IV))
                    dev.steady_march(y)
                    ms.append(dev.march.last_kernel_ms())
                st, flags = dev.march_result()
                assert not np.any(flags), flags
                target = float(dev.rhs(y).abs().max().cpu())
                out.update({"march_ms_first": ms[0], "march_ms": float(np.median(ms[1:])), "march_ms_all": ms[1:],
                            "march_residual": target, "march_iterations": int(st["iterations"].max()),
                            "march_nodes_damped": int(st["nodes-damped"].max())})
                if not a.no_transient:
                    y = dev.to_device(IV)
                    cfg = {}
                    rtol, atol, h0, mx = n2.stepper_args(cfg, "ros4", True)
                    torch.cuda.synchronize()
                    t, wall, r = 0.0, 0.0, float("inf")
                    while wall < a.budget and t < 60.0:
                        t0 = time.perf_counter()
                        dev.ros4(y, t, t + 1.0, rtol, atol, h0 if t == 0.0 else -abs(h0), mx)
                        torch.cuda.synchronize()
                        wall += time.perf_counter() - t0
                        t += 1.0
                        dev.raise_on_flags()
                        r = float(dev.rhs(y).abs().max().cpu())
                        if r <= max(target, 1e-300):
                            break
                    out.update({"transient_model_time": t, "transient_wall_s": wall, "transient_residual": r,
                                "transient_reached": bool(r <= target)})
            finally:
                dev.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
