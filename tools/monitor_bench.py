#!/usr/bin/env python3
"""What the monitor (solver-config "monitor") costs on the device.  Prints ONE JSON line.

--kernel   the row-reduction kernel on raw tensors, fp64, no mechanism: for every shape E x V x N, `--reps` back-to-back
           launches between two HIP events -> us per launch and effective GB/s (E*V*N*8 bytes read).  The shapes are
           launched in the order of SHAPES (a kernel trace of this run can be split by that order).  The environment
           variable RMT_N2_MONITOR_WAVE_BYTES replaces the library's rule for one wave or one workgroup per row (0: always
           a workgroup, a huge value: always a wave), RMT_N2_MONITOR_BLOCK sets the threads of the workgroup form.
--job      wall time of rmtExe for the 256 x 1024-node DME sweep, hip-ros4, 0.5 s, tNo 5: unmonitored, monitored with
           samples = 20, and unmonitored with the same 100 sample times as output times (profile output) - the only way to
           get that information without the monitor.

usage: monitor_bench.py (--kernel | --job) [--reps 50] [--members 256] [--nodes 1024] [--samples 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: every process on the GPU box compiles with the hipRTC PyTorch bundles)
import inputs as INP  # noqa: E402
from rmt_app_amd import hipbind, rmtExe  # noqa: E402

SHAPES = [(256, 7, 1024), (2048, 7, 1024), (2048, 7, 20), (1, 7, 16384),
          (256, 7, 128), (256, 7, 256), (256, 7, 512), (256, 7, 2048), (2048, 7, 512), (2048, 13, 20),
          (512, 7, 2048), (1024, 7, 2048), (2048, 7, 2048), (256, 7, 4096), (1024, 7, 4096), (16, 7, 16384), (64, 7, 4096)]


def kernel(reps):
    mon = hipbind.Monitor(torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    stream = torch.cuda.current_stream().cuda_stream
    out = {"wave_bytes_env": os.environ.get("RMT_N2_MONITOR_WAVE_BYTES"), "reps": reps, "shapes": []}
    for E, V, N in SHAPES:
        y = torch.randn((E, V, N), dtype=torch.float64, device="cuda")
        d = torch.randn((E, V, N), dtype=torch.float64, device="cuda")
        o = torch.zeros((E, V, 5), dtype=torch.float64, device="cuda")
        rec = {"shape": [E, V, N], "MB": E*V*N*8/1e6}
        for tag, dp in (("y", 0), ("y+dydt", d.data_ptr())):
            for _ in range(3):                                   # warm-up
                mon.reduce(stream, y.data_ptr(), dp, E, V, N, False, o.data_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                mon.reduce(stream, y.data_ptr(), dp, E, V, N, False, o.data_ptr())
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1)*1e3/reps
            rec[tag] = {"us": us, "GBps": (2 if dp else 1)*E*V*N*8/us/1e3}
        rec["rows_per_block"] = mon.last_rows_per_block()
        out["shapes"].append(rec)
    mon.close()
    return out


def job(members, nodes, samples):
    nT = members//32                    # bench.py's sweep (rmtexe_ensemble_wall): its code object is in the cache
    ens = {"temperature": list(np.linspace(503.0, 543.0, 64)[:nT]), "pressure": list(np.linspace(3.0e6, 7.0e6, 32))}
    out = {"members": nT*32, "nodes": nodes, "samples": samples, "tNo": 5}
    for tag, tNo, mon in (("unmonitored", 5, None), ("monitored", 5, {"samples": samples}),
                          ("unmonitored_fine_outputs", 5*samples, None)):
        mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.5)
        mi["solver-config"].update({"zNo": nodes, "tNo": tNo, "quiet": True, "ensemble": ens})
        if mon is not None:
            mi["solver-config"]["monitor"] = mon
        walls = []
        for _ in range(3):
            t0 = time.time()
            res = rmtExe(mi)["resModel"]
            walls.append(time.time() - t0)
        st = res["device-stats"]
        out[tag] = {"wall_s": min(walls), "walls": walls, "accepted": int(np.sum(st["accepted"])),
                    "rejected": int(np.sum(st["rejected"]))}
        del res
    out["monitored_over_unmonitored"] = out["monitored"]["wall_s"]/out["unmonitored"]["wall_s"]
    out["fine_outputs_over_monitored"] = out["unmonitored_fine_outputs"]["wall_s"]/out["monitored"]["wall_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--job", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=20)
    a = ap.parse_args()
    if a.kernel == a.job:
        ap.error("give one of --kernel and --job")
    print(json.dumps(kernel(a.reps) if a.kernel else job(a.members, a.nodes, a.samples)))


if __name__ == "__main__":
    main()
