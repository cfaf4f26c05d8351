#!/usr/bin/env python3
"""What the fused activity update costs: rmt_n2_campaign_step against rmt_n2_steady_march on the same rows
(profiles/campaign.md).

For E members (a T/P sweep around the DME notebook input) of N nodes, fresh bed a = 1: the kernel time
(rmt_n2_last_kernel_ms; one warm-up launch, then the median of `--repeat`) of
  * rmt_n2_steady_march of the profiled march unit (n2.march_plan - the unit of "initial": "steady" on a profiled bed),
  * rmt_n2_campaign_step with dt = 0 (the same bed every launch: the two kernels do the same marching work),
  * rmt_n2_campaign_step along a campaign of `--steps` steps of `--dt` seconds (the law and step of golden DA; the bed ages: per-step times
    and the largest per-node iteration count of every step).
Needs a GPU.  One JSON line per shape."""
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
    ap.add_argument("--nodes", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--dt", type=float, default=1.25e5)
    a = ap.parse_args()
    import torch
    import inputs as INP
    from rmt_app_amd import campaign, n2, plan
    from rmt_app_amd.ensemble import expand_members
    base = INP.dme_notebook_input(ivp="hip-ros4")
    for N in a.nodes:
        for E in a.members:
            nT = max(1, int(round(E**0.5)))
            members = [base] if E == 1 else expand_members(base, {"temperature": list(np.linspace(518.0, 528.0, nT)),
                                                                  "pressure": list(np.linspace(4.8e6, 5.2e6, E//nT))})
            mech = n2.mechanism_for(base, members, base["solver-config"])
            pairs = [plan.member_constants(m, mech, N) for m in members]
            rows = np.array([r for _, r in pairs])
            E = len(rows)
            IV = plan.initial_states([nm for nm, _ in pairs], mech, N)
            table = np.stack([np.ones((E, N)), np.zeros((E, N))], axis=1)
            out = {"members": E, "nodes": N}
            mp = n2.march_plan(mech, N, {"RMT_PROFILE": "1"}, rows)
            dev = n2.N2Device(mech, rows, N, block=mp.block, npt=mp.npt, defines=mp.defines, specialize=False,
                              features=mp.features, profile=table)
            try:
                y = dev.to_device(IV)
                ms = []
                for _ in range(a.repeat + 1):
                    dev.steady_march(y)
                    ms.append(dev.last_kernel_ms())
                st, flags = dev.march_result()
                assert not np.any(flags), flags
                out.update({"march_ms": float(np.median(ms[1:])), "march_ms_all": ms[1:],
                            "march_iterations": int(st["iterations"].max())})
            finally:
                dev.close()
            cp = n2.campaign_plan(mech, N, rows)
            dev = n2.N2Device(mech, rows, N, block=cp.block, npt=cp.npt, defines=cp.defines, specialize=False,
                              features=cp.features, profile=table)
            try:
                dev.set_campaign_law(np.tile([2e-7, 8e4, 623.0, 1.0, 0.0], (E, 1)))
                y = dev.to_device(IV)
                log = torch.zeros((E, mech.V + campaign.LOG_EXTRA), dtype=torch.float64, device=y.device)
                ms = []
                for _ in range(a.repeat + 1):
                    dev.campaign_step(y, 0.0, log)
                    ms.append(dev.last_kernel_ms())
                assert not np.any(dev.status())
                out.update({"step_dt0_ms": float(np.median(ms[1:])), "step_dt0_ms_all": ms[1:]})
                out["ratio_dt0"] = out["step_dt0_ms"]/out["march_ms"]
                ms, its, mean = [], [], []
                for _ in range(a.steps):
                    dev.campaign_step(y, a.dt, log)
                    ms.append(dev.last_kernel_ms())
                    lg = log.cpu().numpy()
                    its.append(int(lg[:, mech.V + campaign.ITERATIONS].max()))
                    mean.append(float(lg[:, mech.V + campaign.MEAN].mean()))
                flags = dev.status()          # (a member whose march failed in an aged bed is counted, not hidden)
                out.update({"campaign_flagged": int(np.count_nonzero(flags)), "campaign_ms": ms, "campaign_iterations": its, "campaign_mean_activity": mean})
            finally:
                dev.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
