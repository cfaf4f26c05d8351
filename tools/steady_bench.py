#!/usr/bin/env python3
"""Steady packed-bed models M7 (runM3) and M1 (runM1) on one MI355X: one profile of the reference's test_rmt_DME3
input, and a 64x32 inlet-T/P sweep of it - 2048 profiles, one reactor per lane, in ONE launch - with profiles/s and
the per-profile step counts (accepted + rejected RODAS4 steps).  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inputs_steady as INS               # noqa: E402
from rmt_app_amd import rmtExe            # noqa: E402

out = {}
for model in ("M7", "M1"):
    mi = INS.STEADY_INPUTS[(model, "dme")]()
    rmtExe(mi)                             # JIT / code-object load
    t0 = time.perf_counter()
    res = rmtExe(mi)["resModel"]
    o = {"single": {"wall_s": time.perf_counter() - t0, "points": int(res["dataYs"].shape[1]),
                    "steps": res["device-stats"], "outlet_T": float(res["dataYs"][-1, -1])}}
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_%s.npz" % model.lower()))
    o["single"]["max_rel_vs_tight_lsoda"] = float(np.max(np.abs(res["dataYs"] - g["tight_dataYs"])/np.abs(g["tight_dataYs"])))
    mi = INS.STEADY_INPUTS[(model, "dme")]()
    mi["solver-config"]["ensemble"] = {"temperature": list(np.linspace(503.0, 553.0, 64)),
                                       "pressure": list(np.linspace(3e6, 6e6, 32))}
    rmtExe(mi)                             # warm-up (host packing of 2048 members is part of the timed call below)
    t0 = time.perf_counter()
    ens = rmtExe(mi)["resModel"]["ensemble"]
    w = time.perf_counter() - t0
    st = np.array([d["device-stats"]["accepted"] + d["device-stats"]["rejected"] for d in ens])
    o["sweep_64x32"] = {"profiles": len(ens), "wall_s_incl_host_packing": w, "profiles_per_s": len(ens)/w,
                        "steps_min_median_max": [int(st.min()), int(np.median(st)), int(st.max())],
                        "outlet_T_range": [float(min(d["dataYs"][-1, -1] for d in ens)),
                                           float(max(d["dataYs"][-1, -1] for d in ens))]}
    out[model] = o
print(json.dumps(out))
