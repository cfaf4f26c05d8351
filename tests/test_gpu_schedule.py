"""solver-config "schedule" end to end on the device, through rmtExe, against golden G13 (tools/make_golden.py schedule:
SciPy at rtol 1e-10 / atol 1e-13 on the oracle's RHS with the forced T0, P0 and Tm as functions of t, restarted at every
breakpoint).  Error measure: max |dMoFri| and |dT|/T over ALL nodes at every output time; the bounds are the ones the
end-to-end tests of test_gpu_parity.py assert for the same stepper against a tight LSODA run.

Measured on MI355X (profiles/schedule.md has the table): see the figures each test prints."""
import copy
import json
import os

import numpy as np
import pytest

import inputs as INP
from rmt_app_amd import plan, rmtExe
from rmt_app_amd.ensemble import expand_members
from rmt_app_amd.n2 import N2Device

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(G, "g13_schedule.json")) as _f:
    CASES = json.load(_f)["cases"]

# stepper -> (solver-config, bound)
STEPPERS = {
    "hip-rk4": ({"dt": 2.5e-6}, 1e-8),
    "hip-rk45": ({"rtol": 1e-8, "atol": 1e-11}, 1e-6),
    "hip-ros4": ({}, 1e-6),
    "default": ({}, 1e-6),
}


def case_input(name, ivp, with_schedule=True, **cfg):
    c = CASES[name]
    mi = INP.ALL_N2_INPUTS[c["input"]](ivp=ivp, period=c["period"])
    mi["solver-config"].update({"zNo": c["zNo"], "tNo": c["tNo"], "quiet": True})
    mi["solver-config"].update(STEPPERS[ivp][0])
    mi["solver-config"].update(cfg)
    if with_schedule:
        mi["solver-config"]["schedule"] = copy.deepcopy(c["schedule"])
    return mi


def profile_error(dp, states, Tf, S=6):
    """max |dMoFri|, max |dT|/T over all nodes and output times; states: golden [K][V*N] (scaled variables)."""
    ex = et = 0.0
    assert len(dp) == len(states)
    for k in range(len(dp)):
        Y = np.asarray(states[k]).reshape(S + 1, -1)
        mofr = Y[:S]/np.sum(Y[:S], axis=0)
        T = Y[S]*Tf + Tf
        a = np.asarray(dp[k]["dataYs"])
        ex = max(ex, float(np.max(np.abs(a[:S] - mofr))))
        et = max(et, float(np.max(np.abs(a[S] - T)/T)))
    return ex, et


@pytest.mark.parametrize("ivp", list(STEPPERS))
@pytest.mark.parametrize("name", ["A", "A1", "B"])
def test_step_and_ramp_against_g13(name, ivp):
    """A: step of MeTe, T_in and P_in at an output time; A1: the same step between two output times; B: ramp of T_in and
    MeTe with one output inside the ramp - whole profiles at every output time."""
    g = np.load(os.path.join(G, "g13_schedule_%s.npz" % name))
    res = rmtExe(case_input(name, ivp))["resModel"]
    dp = res["dataPack"]
    assert len(dp) == CASES[name]["tNo"]                      # breakpoints add no entries
    for k in range(len(dp)):
        assert abs(dp[k]["dataTime"] - g["times"][k]) < 1e-12
    ex, et = profile_error(dp, g["states"], 523.0)
    print("G13 %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  stats %s" % (
        name, ivp, ex, et, {k: v for k, v in res["device-stats"].items() if k in ("steps", "launches", "device-mode")}))
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)
    sch = res["schedule"]                                     # the forced values of the base member at the output times
    assert len(sch["time"]) == len(dp) and sch["inlet-temperature"][-1] == CASES[name]["schedule"]["inlet-temperature"][-1]


@pytest.mark.parametrize("mode", [None, "mem"])
@pytest.mark.parametrize("ivp", ["hip-rk4", "hip-rk45", "hip-ros4"])
def test_several_node_blocks_against_g13(ivp, mode):
    """Case C, 600 nodes: once on what the host selects for a forced reactor of that size, once on the memory-resident
    forms with 128-node blocks, where the hand-over between node blocks carries the forced inlet and wall temperature."""
    g = np.load(os.path.join(G, "g13_schedule_C.npz"))
    cfg = {} if mode is None else {"device-mode": "mem", "block": 128, "nodes-per-thread": 1}
    res = rmtExe(case_input("C", ivp, **cfg))["resModel"]
    st = res["device-stats"]
    ex, et = profile_error(res["dataPack"], g["states"], 523.0)
    print("G13 C %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  mode %s geometry %s" % (
        ivp, mode or "host", ex, et, st["device-mode"], st["last-geometry"]))
    # which kernel ran: never a chained form (one workgroup per reactor), and the form the host / the switch chose
    assert st["last-geometry"][0] == 1
    want = "mem" if (mode == "mem" or ivp == "hip-ros4") else "reg"
    assert list(st["device-mode"].values()) == [want]
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)


@pytest.mark.parametrize("ivp", ["hip-rk45", "hip-ros4"])
def test_relative_schedule_on_a_sweep(ivp):
    """Case D: one relative schedule on an 8 x 4 T/P sweep - the three golden members, and every member against its own
    single-member run (both are within the stepper's bound of the same exact solution: twice the bound)."""
    c = CASES["D"]
    g = np.load(os.path.join(G, "g13_schedule_D.npz"))
    base = case_input("D", ivp)
    base["solver-config"]["ensemble"] = copy.deepcopy(c["ensemble"])
    res = rmtExe(base)["resModel"]
    ens = res["ensemble"]
    members = expand_members(base, base["solver-config"]["ensemble"])
    assert len(ens) == len(members) == 32
    bound = STEPPERS[ivp][1]
    for m in c["members"]:
        Tf = members[m]["operating-conditions"]["temperature"]
        ex, et = profile_error(ens[m]["dataPack"], g["states_%d" % m], Tf)
        print("G13 D %s member %d: max|dMoFri| = %.3e  max|dT|/T = %.3e" % (ivp, m, ex, et))
        assert ex <= bound and et <= bound, (m, ex, et)
    worst = 0.0
    for e, mem in enumerate(members):
        single = dict(mem)
        single["solver-config"] = {k: v for k, v in base["solver-config"].items() if k != "ensemble"}
        one = rmtExe(single)["resModel"]["dataPack"]
        for k in range(len(one)):
            a, b = np.asarray(ens[e]["dataPack"][k]["dataYs"]), np.asarray(one[k]["dataYs"])
            d = max(float(np.max(np.abs(a[:6] - b[:6]))), float(np.max(np.abs(a[6] - b[6])/b[6])))
            worst = max(worst, d)
    print("G13 D %s: every member against its own single run: %.3e" % (ivp, worst))
    assert worst <= 2*bound, worst


@pytest.mark.parametrize("ivp", list(STEPPERS))
def test_constant_schedule_reproduces_the_unscheduled_run(ivp):
    """All values equal to the member's own: within twice the stepper's bound of the run without a schedule (the forced
    build may be the plain stepper where the unforced one caches rate constants); where both use the same kernel form
    (hip-ros4 at zNo 20) the step counts are equal - a zero slope adds exact zeros."""
    def run(with_schedule):
        mi = INP.dme_notebook_input(ivp=ivp, period=0.1)
        mi["solver-config"].update({"zNo": 20, "tNo": 2, "quiet": True})
        mi["solver-config"].update(STEPPERS[ivp][0])
        if with_schedule:
            mi["solver-config"]["schedule"] = {"time": [0.0, 0.1], "inlet-temperature": [523.0, 523.0],
                                               "inlet-pressure": [5.0e6, 5.0e6], "medium-temperature": [523.0, 523.0]}
        return rmtExe(mi)["resModel"]
    a, b = run(True), run(False)
    worst = 0.0
    for k in range(2):
        x, y = np.asarray(a["dataPack"][k]["dataYs"]), np.asarray(b["dataPack"][k]["dataYs"])
        worst = max(worst, float(np.max(np.abs(x[:6] - y[:6]))), float(np.max(np.abs(x[6] - y[6])/y[6])))
    print("constant schedule %s: against the unscheduled run %.3e" % (ivp, worst))
    assert worst <= 2*STEPPERS[ivp][1], worst
    assert "schedule" in a and "schedule" not in b
    if ivp == "hip-ros4":
        sa, sb = a["device-stats"], b["device-stats"]
        assert np.array_equal(sa["accepted"], sb["accepted"]) and np.array_equal(sa["rejected"], sb["rejected"])


def test_forced_domain_error_raises_like_an_unforced_one():
    """An inlet pressure stepped down to 100 Pa: the pressure march goes negative inside the bed and sqrt(KH2 PH2) has no
    real value - the reference's lambda raises ValueError('math domain error'), and so does the device, forced or not."""
    mi = INP.dme_notebook_input(ivp="hip-rk4", period=0.002)
    mi["solver-config"].update({"zNo": 20, "tNo": 2, "quiet": True, "dt": 2.5e-6,
                                "schedule": {"time": [0.0, 0.001, 0.001, 0.002], "inlet-pressure": [5e6, 5e6, 100.0, 100.0]}})
    with pytest.raises(ValueError, match="math domain error"):
        rmtExe(mi)
    # the unforced counterpart: the same member row with P0 = 100 Pa
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, 20)
    row = row.copy()
    row[plan.MEMBER_FIELDS["P0"]] = 100.0
    dev = N2Device(mech, row, 20)
    dev.rhs(dev.to_device(plan.initial_state(named, mech, 20)))
    with pytest.raises(ValueError, match="math domain error"):
        dev.raise_on_flags()
    dev.close()
