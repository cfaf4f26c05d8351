#!/usr/bin/env python3
"""What the coolant policy costs: rmt_n2_campaign_policy_step against rmt_n2_campaign_step on the same rows
(profiles/campaign_policy.md).

For E members (a T/P sweep around the DME notebook input) of N nodes, fresh bed a = 1, dt = 0: the kernel time
(rmt_n2_last_kernel_ms; one warm-up launch, then the median of `--repeat`) of
  * rmt_n2_campaign_step of the campaign unit (one march per member),
  * rmt_n2_campaign_policy_step of the policy unit holding x_DME at `--target` within `--limits`, the carried level set
    back to the member's MeTe before every launch (every launch does the same root-find), with the marches per member,
  * the same with the carried level left where the launch before put it (the root is carried in: lo, hi, carried).
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
    ap.add_argument("--nodes", type=int, nargs="+", default=[20])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--target", type=float, default=0.0150)
    ap.add_argument("--limits", type=float, nargs=2, default=[503.0, 543.0])
    a = ap.parse_args()
    import torch
    import inputs as INP
    from rmt_app_amd import campaign, n2, plan
    from rmt_app_amd.ensemble import expand_members
    base = INP.dme_notebook_input(ivp="hip-ros4")
    comp = list(base["feed"]["components"]["shell"]).index("DME")
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
            law = np.tile([2e-7, 8e4, 623.0, 1.0, 0.0], (E, 1))
            out = {"members": E, "nodes": N}
            cp = n2.campaign_plan(mech, N, rows)
            dev = n2.N2Device(mech, rows, N, block=cp.block, npt=cp.npt, defines=cp.defines, specialize=False,
                              features=cp.features, profile=table)
            try:
                dev.set_campaign_law(law)
                y = dev.to_device(IV)
                log = torch.zeros((E, mech.V + campaign.LOG_EXTRA), dtype=torch.float64, device=y.device)
                ms = []
                for _ in range(a.repeat + 1):
                    dev.campaign_step(y, 0.0, log)
                    ms.append(dev.last_kernel_ms())
                assert not np.any(dev.status())
                out.update({"step_ms": float(np.median(ms[1:])), "step_ms_all": ms[1:]})
            finally:
                dev.close()
            pp = n2.campaign_policy_plan(mech, N, rows)
            dev = n2.N2Device(mech, rows, N, block=pp.block, npt=pp.npt, defines=pp.defines, specialize=False,
                              features=pp.features, profile=table)
            try:
                dev.set_campaign_law(law)
                prow = np.tile([a.target, a.limits[0], a.limits[1], 1e-10], (E, 1))
                levels = np.clip(np.array([float(m["external-heat"]["MeTe"]) for m in members]), *a.limits)
                y = dev.to_device(IV)
                log = torch.zeros((E, mech.V + campaign.LOG_EXTRA), dtype=torch.float64, device=y.device)
                plog = torch.zeros((E, campaign.POLICY_LOG), dtype=torch.float64, device=y.device)
                for tag, reset in (("policy", True), ("policy_carried", False)):
                    ms = []
                    for _ in range(a.repeat + 1):
                        if reset or not ms:
                            dev.set_campaign_policy(prow, comp, levels)
                        dev.campaign_policy_step(y, 0.0, log, plog)
                        ms.append(dev.last_kernel_ms())
                    flags = dev.status()
                    pl = plog.cpu().numpy()
                    ev = pl[:, campaign.EVALUATIONS]
                    out.update({tag + "_ms": float(np.median(ms[1:])), tag + "_ms_all": ms[1:],
                                tag + "_marches_mean": float(ev.mean()), tag + "_marches_max": int(ev.max()),
                                tag + "_saturated": int(np.count_nonzero(pl[:, campaign.SATURATED])),
                                tag + "_flagged": int(np.count_nonzero(flags)),
                                tag + "_ratio": float(np.median(ms[1:]))/out["step_ms"]})
            finally:
                dev.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
