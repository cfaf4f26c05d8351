#!/usr/bin/env python3
"""What time-varying inlet / coolant conditions (solver-config "schedule") cost on the device.  Prints ONE JSON line:

* node-steps/s of the forced against the unforced rmt_n2_rk4_reg at 256 reactors x 1024 nodes (the unforced one is what
  an unscheduled run gets: member literals and the rate-constant cache; the forced one is the plain stepper with run-time
  rows and the forcing evaluated at every stage);
* wall time and step counts of the 256 x 1024 x 0.5 s hip-ros4 job through rmtExe, without a schedule and with case A's
  step (at t = 0.2: MeTe +10 K, T_in +5 K, P_in -2 % of the base pressure) as a relative schedule;
* the same two figures with a scheduled feed composition ("inlet-concentration", RMT_FORCING 2): rmt_n2_rk4_reg with a
  ramp of T_in, MeTe AND the composition against the RMT_FORCING 1 rate of the same session, and the hip-ros4 job with a
  composition step at t = 0.2 (CO2 -30, CO +30 mol/m^3, relative) against the job with case A's step;
* VGPR / AGPR / SGPR / scratch of the builds with RMT_FORCING 0, 1 and 2 (rmt_app_amd.isa.kernel_resources).

usage: schedule_bench.py [--steps 2000] [--members 256] [--nodes 1024] [--skip-ros4]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first: every process on the GPU box compiles with the hipRTC PyTorch bundles)
import inputs as INP  # noqa: E402
from rmt_app_amd import hipbind, isa, n2, plan, rmtExe, schedule  # noqa: E402
from rmt_app_amd.ensemble import expand_members  # noqa: E402


def sweep(members):
    nT = int(round(members**0.5))
    nP = members//nT
    return {"temperature": np.linspace(503.0, 543.0, nT).tolist(), "pressure": np.linspace(4.0e6, 6.0e6, nP).tolist()}


def resources(mech, block, npt, defs, kernels, features=()):
    tpl = hipbind.kernel_template()
    out = {}
    for level, tag in (("0", "unforced"), ("1", "forced"), ("2", "forced+composition")):
        d = dict(defs, **({"RMT_FORCING": level} if level != "0" else {}))
        blob = hipbind.compile_cached(mech.source(tpl, False, block, npt, None, d), mech.digest(tpl, False, block, npt, None, d),
                                      "gfx950", n2.compile_options(block, npt, features, "", d))
        for k in kernels:
            r = isa.kernel_resources(blob, k)
            out["%s %dx%d %s" % (k, block, npt, tag)] = {
                "vgpr": r.get("vgpr_count"), "agpr": r.get("agpr_count"), "sgpr": r.get("sgpr_count"),
                "scratch": r.get("private_segment_fixed_size")}
    return out


def rk4_rate(dev, y0, dt, steps, repeats=3):
    rates = []
    for _ in range(repeats + 1):
        y = y0.clone()
        dev.rk4(y, dt, steps)
        dev.torch.cuda.synchronize()
        rates.append(dev.E*dev.N*steps/(dev.last_kernel_ms()*1e-3))
    dev.raise_on_flags()
    return rates[1:]                     # (the first launch warms up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--skip-ros4", action="store_true")
    a = ap.parse_args()
    N = a.nodes
    base = INP.dme_notebook_input(ivp="hip-ros4", period=0.5)
    base["solver-config"].update({"zNo": N, "tNo": 5, "quiet": True, "ensemble-output": "outlet"})
    ens = sweep(a.members)
    members = expand_members(base, ens)
    mech = plan.Mechanism(base)
    pairs = [plan.member_constants(mi, mech, N) for mi in members]
    named, rows = [nm for nm, _ in pairs], np.array([r for _, r in pairs])
    out = {"members": len(members), "nodes": N, "steps": a.steps}
    # --- rmt_n2_rk4_reg, forced against unforced
    dt = 2e-6
    dev = n2.N2Device(mech, rows, N, block=512, npt=2)
    y0 = dev.to_device(plan.initial_states(named, mech, N))
    un = rk4_rate(dev, y0, dt, a.steps)
    dev.close()
    step_a = {"time": [0.0, 0.2, 0.2, 0.5], "inlet-temperature": [0.0, 0.0, 5.0, 5.0],
              "inlet-pressure": [0.0, 0.0, -1.0e5, -1.0e5], "medium-temperature": [0.0, 0.0, 10.0, 10.0], "relative": True}
    ramp = dict(base, **{"solver-config": dict(base["solver-config"], schedule={
        "time": [0.0, 1.0], "inlet-temperature": [0.0, 10.0], "medium-temperature": [0.0, 8.0], "relative": True})})
    sch = schedule.parse(ramp, members)
    dev = n2.N2Device(mech, sch.forced_rows(rows, named, 0.0, dt*a.steps), N, block=512, npt=2, defines={"RMT_FORCING": "1"})
    dev.set_mode("reg")
    fo = rk4_rate(dev, y0, dt, a.steps)
    dev.close()
    # ... and with the feed composition ramped as well (RMT_FORCING 2; CO2 -30, CO +30 mol/m^3 over the same second)
    feed_off = [0.0, -30.0, 0.0, 30.0, 0.0, 0.0]
    ramp2 = copy.deepcopy(ramp)
    ramp2["solver-config"]["schedule"]["inlet-concentration"] = [[0.0]*6, feed_off]
    sch2 = schedule.parse(ramp2, members)
    dev = n2.N2Device(mech, sch2.forced_rows(rows, named, 0.0, dt*a.steps), N, block=512, npt=2,
                      defines={"RMT_FORCING": sch2.forcing_level})
    dev.set_mode("reg")
    fc = rk4_rate(dev, y0, dt, a.steps)
    dev.close()
    out["rk4_reg_node_steps_per_s"] = {"unforced": float(np.median(un)), "forced": float(np.median(fo)),
                                       "forced_composition": float(np.median(fc)),
                                       "unforced_repeats": un, "forced_repeats": fo, "forced_composition_repeats": fc,
                                       "forced_over_unforced": float(np.median(fo)/np.median(un)),
                                       "composition_over_forced": float(np.median(fc)/np.median(fo))}
    # --- the stiff job through rmtExe
    if not a.skip_ros4:
        job = {}
        step_feed = {"time": [0.0, 0.2, 0.2, 0.5], "relative": True,
                     "inlet-concentration": [[0.0]*6, [0.0]*6, feed_off, feed_off]}
        for tag, spec in (("unscheduled", None), ("case_A_step", step_a), ("case_FA_feed_step", step_feed)):
            mi = dict(base, **{"solver-config": dict(base["solver-config"], ensemble=ens)})
            if spec is not None:
                mi["solver-config"]["schedule"] = spec
            walls = []
            for _ in range(2):
                t0 = time.time()
                res = rmtExe(mi)["resModel"]
                walls.append(time.time() - t0)
            st = res["device-stats"]
            job[tag] = {"wall_s": min(walls), "accepted": int(np.sum(st["accepted"])), "rejected": int(np.sum(st["rejected"])),
                        "launches": st.get("launches", 5), "rhs_evals": int(st["rhs_evals"])}
        out["ros4_job_0p5s"] = job
    # --- registers
    res = {}
    res.update(resources(mech, 512, 2, {}, ("rmt_n2_rk4_reg", "rmt_n2_rk4_mem")))
    res.update(resources(mech, 64, 1, {}, ("rmt_n2_rk4_reg", "rmt_n2_rk4_mem")))
    res.update(resources(mech, 512, 2, {"RMT_RK45_LDS": "2"}, ("rmt_n2_rk45_reg", "rmt_n2_rk45_mem")))
    res.update(resources(mech, 64, 1, {"RMT_RK45_LDS": "2"}, ("rmt_n2_rk45_reg", "rmt_n2_rk45_mem")))
    res.update(resources(mech, 256, 1, {"RMT_WITH_ROS4": "1"}, ("rmt_n2_ros4_mem",), ("ros4",)))
    res.update(resources(mech, 64, 1, {"RMT_WITH_ROS4": "1"}, ("rmt_n2_ros4_mem",), ("ros4",)))
    out["resources"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
