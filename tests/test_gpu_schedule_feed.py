"""solver-config "schedule" with "inlet-concentration" end to end on the device, through rmtExe, against golden G14
(tools/make_golden.py feed: SciPy at rtol 1e-10 / atol 1e-13 on the oracle's RHS with the forced feed composition - and
inlet temperature, case FB - as functions of t, restarted at every breakpoint; every disturbance leaves max(SpCoi0)
unchanged, so the oracle's scaling is the member's own).  Error measure, stepper configurations and bounds are those of
test_gpu_schedule.py: max |dMoFri| and |dT|/T over ALL nodes at every output time; 1e-8 for hip-rk4 at dt 2.5e-6, 1e-6 for
hip-rk45, hip-ros4 and "default".  A stepper that ignored the composition would miss by five orders of magnitude (the
step moves the CO2 and CO profiles by up to 0.12).

Measured on MI355X (profiles/schedule_feed.md has the table): see the figures each test prints."""
import copy
import json
import os

import numpy as np
import pytest

import inputs as INP
from rmt_app_amd import rmtExe
from rmt_app_amd.ensemble import expand_members
from test_gpu_schedule import STEPPERS, profile_error

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(G, "g14_feed.json")) as _f:
    CASES = json.load(_f)["cases"]
KEY = "inlet-concentration"


def case_input(name, ivp, with_schedule=True, **cfg):
    c = CASES[name]
    mi = INP.ALL_N2_INPUTS[c["input"]](ivp=ivp, period=c["period"])
    mi["solver-config"].update({"zNo": c["zNo"], "tNo": c["tNo"], "quiet": True})
    mi["solver-config"].update(STEPPERS[ivp][0])
    mi["solver-config"].update(cfg)
    if with_schedule:
        mi["solver-config"]["schedule"] = copy.deepcopy(c["schedule"])
    return mi


@pytest.mark.parametrize("ivp", list(STEPPERS))
@pytest.mark.parametrize("name", ["FA", "FA1", "FB"])
def test_step_and_ramp_against_g14(name, ivp):
    """FA: CO2 -> CO step of the feed at an output time; FA1: the same step between two output times; FB: ramp of the same
    change together with a ramp of T_in, one output inside the ramp - whole profiles at every output time."""
    g = np.load(os.path.join(G, "g14_feed_%s.npz" % name))
    res = rmtExe(case_input(name, ivp))["resModel"]
    dp = res["dataPack"]
    assert len(dp) == CASES[name]["tNo"]                      # breakpoints add no entries
    for k in range(len(dp)):
        assert abs(dp[k]["dataTime"] - g["times"][k]) < 1e-12
    ex, et = profile_error(dp, g["states"], 523.0)
    print("G14 %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  stats %s" % (
        name, ivp, ex, et, {k: v for k, v in res["device-stats"].items() if k in ("steps", "launches", "device-mode")}))
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)
    sch = res["schedule"]                                     # the forced composition of the base member at the output times
    assert sch[KEY].shape == (len(dp), 6)
    assert sch[KEY][-1].tolist() == CASES[name]["schedule"][KEY][-1]


@pytest.mark.parametrize("mode", [None, "mem"])
@pytest.mark.parametrize("ivp", ["hip-rk4", "hip-rk45", "hip-ros4"])
def test_several_node_blocks_against_g14(ivp, mode):
    """Case FC, 600 nodes: once on what the host selects for a forced reactor of that size (the on-chip forms at 512 x 2,
    where thread 0 rewrites the inlet slots per stage), once on the memory-resident forms with 128-node blocks, where the
    stage hand-overs carry the forced inlet composition from block to block."""
    g = np.load(os.path.join(G, "g14_feed_FC.npz"))
    cfg = {} if mode is None else {"device-mode": "mem", "block": 128, "nodes-per-thread": 1}
    res = rmtExe(case_input("FC", ivp, **cfg))["resModel"]
    st = res["device-stats"]
    ex, et = profile_error(res["dataPack"], g["states"], 523.0)
    print("G14 FC %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  mode %s geometry %s" % (
        ivp, mode or "host", ex, et, st["device-mode"], st["last-geometry"]))
    # which kernel ran: never a chained form (one workgroup per reactor), and the form the host / the switch chose
    assert st["last-geometry"][0] == 1
    want = "mem" if (mode == "mem" or ivp == "hip-ros4") else "reg"
    assert list(st["device-mode"].values()) == [want]
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)


@pytest.mark.parametrize("ivp", ["hip-rk45", "hip-ros4"])
def test_relative_composition_on_a_sweep(ivp):
    """Case FD: one relative schedule (CO2 -30, CO +30 mol/m^3 from t = 0.2 on) on an 8 x 4 T/P sweep whose members have
    different feeds - ONE run, the three golden members; the bound of test_relative_schedule_on_a_sweep's comparison."""
    c = CASES["FD"]
    g = np.load(os.path.join(G, "g14_feed_FD.npz"))
    base = case_input("FD", ivp)
    base["solver-config"]["ensemble"] = copy.deepcopy(c["ensemble"])
    res = rmtExe(base)["resModel"]
    ens = res["ensemble"]
    members = expand_members(base, base["solver-config"]["ensemble"])
    assert len(ens) == len(members) == 32
    bound = 2*STEPPERS[ivp][1]
    for m in c["members"]:
        Tf = members[m]["operating-conditions"]["temperature"]
        ex, et = profile_error(ens[m]["dataPack"], g["states_%d" % m], Tf)
        print("G14 FD %s member %d: max|dMoFri| = %.3e  max|dT|/T = %.3e" % (ivp, m, ex, et))
        assert ex <= bound and et <= bound, (m, ex, et)


@pytest.mark.parametrize("ivp", list(STEPPERS))
def test_constant_composition_reproduces_the_unscheduled_run(ivp):
    """A composition held at the member's own feed: within twice the stepper's bound of the run without a schedule; the
    stiff stepper takes the same steps (a hold skips the f_t pass, zero slopes add exact zeros)."""
    def run(with_schedule):
        mi = INP.dme_notebook_input(ivp=ivp, period=0.1)
        mi["solver-config"].update({"zNo": 20, "tNo": 2, "quiet": True})
        mi["solver-config"].update(STEPPERS[ivp][0])
        if with_schedule:
            feed = [float(v) for v in mi["feed"]["concentration"]]
            mi["solver-config"]["schedule"] = {"time": [0.0, 0.1], KEY: [feed, feed]}
        return rmtExe(mi)["resModel"]
    a, b = run(True), run(False)
    worst = 0.0
    for k in range(2):
        x, y = np.asarray(a["dataPack"][k]["dataYs"]), np.asarray(b["dataPack"][k]["dataYs"])
        worst = max(worst, float(np.max(np.abs(x[:6] - y[:6]))), float(np.max(np.abs(x[6] - y[6])/y[6])))
    print("constant composition %s: against the unscheduled run %.3e" % (ivp, worst))
    assert worst <= 2*STEPPERS[ivp][1], worst
    assert KEY in a["schedule"] and "schedule" not in b
    if ivp == "hip-ros4":
        sa, sb = a["device-stats"], b["device-stats"]
        assert np.array_equal(sa["accepted"], sb["accepted"]) and np.array_equal(sa["rejected"], sb["rejected"])


def test_monitored_run_with_a_composition_step():
    """Case FA with a monitor of two samples per output interval: the monitor's outlet rows at the output times are the
    dataPack's outlet values (the refined launch list keeps the composition's breakpoints)."""
    res = rmtExe(case_input("FA", "hip-rk45", monitor={"samples": 2}))["resModel"]
    mon, dp = res["monitor"], res["dataPack"]
    assert len(mon["time"]) == 5 and len(dp) == 2
    for pk in dp:
        k = int(np.argmin(np.abs(mon["time"] - pk["dataTime"])))
        assert mon["time"][k] == pk["dataTime"]
        a, b = np.asarray(mon["outlet"][k], float), np.asarray(pk["dataYs"], float)[:, -1]
        e = float(np.max(np.abs(a - b)/np.maximum(np.abs(b), 1e-300)))
        print("monitor at t = %.2f: outlet against the dataPack %.3e" % (pk["dataTime"], e))
        assert e <= 1e-14, (k, e)
    g = np.load(os.path.join(G, "g14_feed_FA.npz"))
    ex, et = profile_error(dp, g["states"], 523.0)
    print("G14 FA hip-rk45 monitored: max|dMoFri| = %.3e  max|dT|/T = %.3e" % (ex, et))
    assert ex <= STEPPERS["hip-rk45"][1] and et <= STEPPERS["hip-rk45"][1]
