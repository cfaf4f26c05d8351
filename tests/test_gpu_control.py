"""solver-config "control" on the device: the controller's kernel alone through the C ABI against numpy, bit for bit, and
closed-loop runs through rmtExe against golden G15 (tools/make_golden.py control: SciPy at rtol 1e-10 / atol 1e-13 on the
oracle's RHS, restarted at every sample time and breakpoint, the control law restated in the generator).  Error measure
and per-stepper bounds are those of tests/test_gpu_schedule.py: max |dMoFri| and |dT|/T over ALL nodes at every output time.

Every test prints its figures before it asserts; profiles/control.md is where they are recorded (the device figures are
still missing there: the kernel and the host walk have so far run on the host emulation only, tests/test_control_emulated_cpu.py)."""
import copy
import json
import os

import numpy as np
import pytest

import inputs as INP
from rmt_app_amd import control, hipbind, plan, rmtExe, schedule
from rmt_app_amd.ensemble import expand_members
from rmt_app_amd.n2 import N2Device

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(G, "g15_control.json")) as _f:
    CASES = json.load(_f)["cases"]

# stepper -> (solver-config, bound): tests/test_gpu_schedule.py
STEPPERS = {
    "hip-rk4": ({"dt": 2.5e-6}, 1e-8),
    "hip-rk45": ({"rtol": 1e-8, "atol": 1e-11}, 1e-6),
    "hip-ros4": ({}, 1e-6),
    "default": ({}, 1e-6),
}
S = 6


def case_input(name, ivp, with_control=True, **cfg):
    c = CASES[name]
    mi = INP.ALL_N2_INPUTS[c["input"]](ivp=ivp, period=c["period"])
    mi["solver-config"].update({"zNo": c["zNo"], "tNo": c["tNo"], "quiet": True})
    mi["solver-config"].update(STEPPERS[ivp][0])
    mi["solver-config"].update(cfg)
    if c.get("schedule"):
        mi["solver-config"]["schedule"] = copy.deepcopy(c["schedule"])
    if with_control:
        mi["solver-config"]["control"] = copy.deepcopy(c["control"])
    if "ensemble" in c:
        mi["solver-config"]["ensemble"] = copy.deepcopy(c["ensemble"])
    return mi


def profile_error(dp, states, Tf):
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


def measured_error(ctl_spec, got, want):
    """the logged measurements against G15's, in the measure of the states: |dT|/T, or |d mole fraction|"""
    d = np.abs(np.asarray(got) - np.asarray(want))
    return float(np.max(d if isinstance(ctl_spec["measured"], dict) else d/np.asarray(want)))


def law_holds(entry, ctl, e):
    """the logged output IS control.emulate of the logged measurements, bit for bit"""
    u, sat, _ = control.emulate(entry["measured"], entry["setpoint"], ctl.Kp[e], ctl.Ki[e], ctl.u0[e], ctl.lo[e], ctl.hi[e])
    assert np.array_equal(entry["setpoint"], ctl.setpoints[:, e])
    assert np.array_equal(entry["output"], u), float(np.max(np.abs(entry["output"] - u)))
    assert np.array_equal(entry["saturated"], sat)


def parsed(mi, ivp):
    members = expand_members(mi, mi["solver-config"]["ensemble"]) if "ensemble" in mi["solver-config"] else None
    sched = schedule.parse(mi, members, ivp)
    return control.parse(mi, members, ivp, sched)[0]


def same_states(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x["dataYs"]), np.asarray(y["dataYs"])), \
            float(np.max(np.abs(np.asarray(x["dataYs"]) - np.asarray(y["dataYs"]))))


# ----------------------------------------------------------------------------- 1. the kernel alone
def _reference(y, rows, prm, r, state, field, tail_at):
    """numpy: one update of every member.  Returns (log [E][4], state [E][3], rows)."""
    E, V, N = y.shape
    log, state, rows = np.zeros((E, control.LOG)), state.copy(), rows.copy()
    F = plan.MEMBER_FIELDS
    for e in range(E):
        sel, tf = int(prm[e, control.P_SELECT]), rows[e, F["TF"]]
        if sel == 2:
            tot = 0.0
            for i in range(S):
                tot += y[e, i, N - 1]
            pv = y[e, int(prm[e, control.P_SPECIES]), N - 1]/tot
        else:
            row = y[e, V - 1]
            theta = row[N - 1] if sel == 0 else np.max(np.where(np.isnan(row), -np.inf, row))
            pv = theta*tf + tf
        u, sat, I = control.emulate([pv], [r[e]], prm[e, 0], prm[e, 1], prm[e, 2], prm[e, 3], prm[e, 4], I0=state[e, 0])
        log[e] = [pv, r[e], u[0], float(sat[0])]
        state[e] = [I[0], u[0], state[e, 2] + 1.0]
        rows[e, (F["THETA_IN"], F["P0"], F["TM"])[field]] = (u[0] - tf)/tf if field == 0 else u[0]
        rows[e, tail_at + 1 + field] = 0.0
    return log, state, rows


@pytest.mark.parametrize("E", [1, 3, 130])
def test_kernel_alone_through_the_c_abi(E):
    """All three measurements and all three row fields, N in {1, 2, 63, 64, 65, 600}, state rows at aligned and unaligned
    addresses, the peak at node 0, at node N-1 (the scalar head / tail of an unaligned row) and in between, a NaN that is
    not the maximum, members with and without integral action, saturating and not; E = 130 is more members than the grid
    has waves (grid-stride walk).  pv, r, u, I, the saturated flag and the rows equal numpy bit for bit; hold mode changes
    nothing but the row field."""
    import torch
    rng = np.random.default_rng(150 + E)
    mi = INP.dme_notebook_input()
    mech = plan.Mechanism(mi)
    V, F = mech.V, plan.MEMBER_FIELDS
    base = plan.member_constants(mi, mech, 20)[1]
    rows0 = np.zeros((E, mech.row_width + schedule.TAIL))
    rows0[:, :mech.row_width] = base
    rows0[:, F["TF"]] = 500.0 + 40.0*rng.random(E)                     # every member its own Tf
    rows0[:, mech.row_width:] = rng.standard_normal((E, schedule.TAIL))   # slopes that are NOT zero
    dev = N2Device(mech, rows0, 20, block=64, npt=1, defines={"RMT_FORCING": "1"}, specialize=False)
    kernel = hipbind.Control("gfx950" if not torch.cuda.is_available() else
                             torch.cuda.get_device_properties(dev.device).gcnArchName.split(":")[0])
    tail_at = mech.row_width
    n_sat = n_free = 0
    try:
        for N in (1, 2, 63, 64, 65, 600):
            for shift in (0, 1):                                   # the state buffer at a 16-byte boundary / 8 bytes behind one
                for sel, field in ((0, 1), (1, 0), (2, 2)):
                    y = 0.2*rng.random((E, V, N)) + 0.05
                    for e in range(E):
                        pos = (0, N - 1, N//2)[e % 3]
                        y[e, V - 1, pos] = 0.31 + 0.01*rng.random()   # the peak of the temperature row
                        if N >= 2 and e % 2 == 0:
                            y[e, V - 1, (pos + 1) % N] = np.nan       # a NaN that is not the maximum
                    prm = np.zeros((E, control.PARAMS))
                    # (gains that leave about half of the members inside their limits)
                    prm[:, control.P_KP] = rng.choice([-1.0, 1.0], E)*(1.0 + rng.random(E))*(0.1, 2.0e3, 20.0)[field]
                    prm[:, control.P_KI] = np.where(rng.random(E) < 0.3, 0.0, 0.2*prm[:, control.P_KP])
                    u0 = 5.0e6 if field == 1 else 520.0
                    prm[:, control.P_U0] = u0*(1.0 + 0.02*rng.random(E))
                    width = (2.0e5 if field == 1 else 8.0)*np.where(rng.random(E) < 0.5, 0.05, 1.0)     # half of them saturate
                    prm[:, control.P_LO], prm[:, control.P_HI] = prm[:, control.P_U0] - width, prm[:, control.P_U0] + width
                    prm[:, control.P_SELECT], prm[:, control.P_SPECIES] = sel, rng.integers(0, S, E)
                    K = 3
                    scale = 1.0 if sel == 2 else 600.0
                    sp = (0.15 if sel == 2 else 660.0) + 0.01*scale*rng.standard_normal((K, E))
                    buf = torch.zeros(E*V*N + 1, dtype=torch.float64, device=dev.device)
                    yd = buf[shift:shift + E*V*N]
                    yd.copy_(torch.from_numpy(y.reshape(-1)))
                    d_prm, d_sp = torch.from_numpy(prm).to(dev.device), torch.from_numpy(sp).to(dev.device)
                    d_state = torch.zeros((E, control.STATE), dtype=torch.float64, device=dev.device)
                    d_log = torch.zeros((K, E, control.LOG), dtype=torch.float64, device=dev.device)
                    dev.set_members(rows0)
                    state, rows = np.zeros((E, control.STATE)), rows0.copy()
                    for k in range(K):
                        kernel.update(dev.h, yd.data_ptr(), V, N, d_prm.data_ptr(), d_sp[k].data_ptr(), d_state.data_ptr(),
                                      d_log[k].data_ptr(), tail_at, field)
                        log, state, rows = _reference(y, rows, prm, sp[k], state, field, tail_at)
                        what = (E, N, shift, sel, field, k)
                        assert np.array_equal(d_log[k].cpu().numpy(), log, equal_nan=True), what
                        assert np.array_equal(d_state.cpu().numpy(), state, equal_nan=True), what
                        assert np.array_equal(dev.get_members(), rows, equal_nan=True), what
                        n_sat, n_free = n_sat + int(np.sum(log[:, 3] == 1.0)), n_free + int(np.sum(log[:, 3] == 0.0))
                    # hold: the refresh uploads whole rows, the kernel writes the held value again - and nothing else
                    dev.set_members(rows0)
                    before = (d_log.cpu().numpy(), d_state.cpu().numpy())
                    kernel.update(dev.h, 0, V, N, 0, 0, d_state.data_ptr(), 0, tail_at, field, hold=True)
                    assert np.array_equal(dev.get_members(), rows, equal_nan=True), (E, N, shift, sel, field, "hold")
                    assert np.array_equal(d_log.cpu().numpy(), before[0], equal_nan=True)
                    assert np.array_equal(d_state.cpu().numpy(), before[1], equal_nan=True)
                    # a member that has not been sampled yet keeps the row it has
                    d_state.zero_()
                    dev.set_members(rows0)
                    kernel.update(dev.h, 0, V, N, 0, 0, d_state.data_ptr(), 0, tail_at, field, hold=True)
                    assert np.array_equal(dev.get_members(), rows0)
    finally:
        kernel.close()
        dev.close()
    print("control kernel, E = %d: %d saturated and %d free member-samples" % (E, n_sat, n_free))
    assert n_sat > 0 and n_free > 0


# ----------------------------------------------------------------------------- 2. closed loops against G15
@pytest.mark.parametrize("ivp", list(STEPPERS))
@pytest.mark.parametrize("name", ["CA", "CB", "CD"])
def test_closed_loop_against_g15(name, ivp):
    """CA: PI on the outlet temperature through a coolant step and a setpoint step; CB: the same loop between narrow
    limits (anti-windup); CD: a 2 x 2 T/P ensemble on the outlet mole fraction of DME, golden members 0 and 3.  Whole
    profiles at every output time and the logged measurements within the stepper's bound of G15; the logged output is
    control.emulate of the logged measurements, bit for bit."""
    c = CASES[name]
    g = np.load(os.path.join(G, "g15_control_%s.npz" % name))
    mi = case_input(name, ivp)
    res = rmtExe(mi)["resModel"]
    ctl = parsed(mi, ivp)
    bound = STEPPERS[ivp][1]
    assert set(res["control"]) == {"time", "measured", "setpoint", "output", "saturated"}
    members = expand_members(mi, c["ensemble"]) if "ensemble" in c else [mi]
    worst = []
    for m in c.get("members", [None]):
        e, tag = (0, "") if m is None else (m, "_%d" % m)
        out = res if m is None else res["ensemble"][m]
        Tf = members[e]["operating-conditions"]["temperature"]
        ex, et = profile_error(out["dataPack"], g["states" + tag], Tf)
        log = g["log" + tag]
        assert np.array_equal(out["control"]["time"], log[:, 0])
        em = measured_error(c["control"], out["control"]["measured"], log[:, 1])
        du = float(np.max(np.abs(out["control"]["output"] - log[:, 3])))
        print("G15 %s%s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  measured %.3e  max|du| = %.3e Pa  saturated %d/%d  "
              "launches %s" % (name, tag, ivp, ex, et, em, du, int(np.sum(out["control"]["saturated"])), len(log),
                               res["device-stats"]["launches"]))
        worst.append((ex, et, em))
    for e in range(len(members)):
        law_holds(res["control"] if len(members) == 1 else res["ensemble"][e]["control"], ctl, e)
    if len(members) > 1:
        assert np.array_equal(res["control"]["output"], res["ensemble"][0]["control"]["output"])
    for ex, et, em in worst:
        assert ex <= bound and et <= bound and em <= bound, (ex, et, em)
    if name == "CB":
        assert np.sum(res["control"]["saturated"]) >= 3
    if name == "CA":
        assert not np.any(res["control"]["saturated"])


# ----------------------------------------------------------------------------- 3. several node blocks, forcing level 2
@pytest.mark.parametrize("mode", [None, "mem"])
@pytest.mark.parametrize("ivp", ["hip-rk4", "hip-rk45", "hip-ros4"])
def test_peak_temperature_on_both_kernel_forms_against_g15(ivp, mode):
    """Case CC, 600 nodes, peak temperature, a schedule that also moves the feed (RMT_FORCING 2): once on what the host
    selects for a forced reactor of that size, once on the memory-resident forms with 128-node blocks."""
    g = np.load(os.path.join(G, "g15_control_CC.npz"))
    cfg = {} if mode is None else {"device-mode": "mem", "block": 128, "nodes-per-thread": 1}
    mi = case_input("CC", ivp, **cfg)
    res = rmtExe(mi)["resModel"]
    st = res["device-stats"]
    ex, et = profile_error(res["dataPack"], g["states"], 523.0)
    em = measured_error(CASES["CC"]["control"], res["control"]["measured"], g["log"][:, 1])
    print("G15 CC %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  measured %.3e  mode %s geometry %s" % (
        ivp, mode or "host", ex, et, em, st["device-mode"], st["last-geometry"]))
    assert st["last-geometry"][0] == 1
    want = "mem" if (mode == "mem" or ivp == "hip-ros4") else "reg"
    assert list(st["device-mode"].values()) == [want]
    law_holds(res["control"], parsed(mi, ivp), 0)
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound and em <= bound, (ex, et, em)


# ----------------------------------------------------------------------------- 4. open-loop replay
@pytest.mark.parametrize("ivp", list(STEPPERS))
def test_open_loop_replay_is_bit_identical(ivp):
    """The logged u_k of a CA run as a schedule of the inlet pressure with a jump at every sample time, without
    "control": the same launch list and the same rows, so the states are equal bit for bit - which pins the order in the
    stream (refresh, controller, stepper), the hold mode and the row mapping.  Two monitor samples between control samples
    give both runs two launches that start at no sample time: there the controller's kernel runs in hold mode."""
    off = {"monitor": {"times": [0.155, 0.305]}}
    closed = rmtExe(case_input("CA", ivp, **off))["resModel"]
    assert closed["device-stats"]["launches"] == 4 + 27 + 2            # output times, the other samples, the monitor's
    t, u = closed["control"]["time"], closed["control"]["output"]
    mi = case_input("CA", ivp, with_control=False, **off)
    sch = mi["solver-config"]["schedule"]
    assert sch["time"] == [0.0, 0.2, 0.2, 0.4] and sch["medium-temperature"] == [523.0, 523.0, 533.0, 533.0]
    step = min((float(x) for x in t), key=lambda x: abs(x - 0.2))          # the coolant's step IS a sample time
    assert abs(step - 0.2) < 1e-12
    times, P, Tm, held = [0.0], [5.0e6], [523.0], 5.0e6                     # before "start": the member's own pressure
    for b, new in zip((float(x) for x in t), (float(x) for x in u)):
        times += [b, b]
        P += [held, new]                                                    # a jump at every sample time, held between
        Tm += [523.0 if b <= step else 533.0, 523.0 if b < step else 533.0]
        held = new
    mi["solver-config"]["schedule"] = {"time": times, "inlet-pressure": P, "medium-temperature": Tm}
    replay = rmtExe(mi)["resModel"]
    assert replay["device-stats"]["launches"] == closed["device-stats"]["launches"]
    assert "control" not in replay
    same_states(closed["dataPack"], replay["dataPack"])


# ----------------------------------------------------------------------------- 5. gain 0
@pytest.mark.parametrize("ivp", list(STEPPERS))
def test_gain_zero_reproduces_the_uncontrolled_run(ivp):
    """gain 0: u = u0, the member's own value, exactly - the run without "control" on the same launch list (a monitor
    with "times" at the sample times), bit for bit."""
    mi = case_input("CA", ivp)
    mi["solver-config"]["control"]["gain"] = 0.0
    a = rmtExe(mi)["resModel"]
    assert np.all(a["control"]["output"] == 5.0e6) and not np.any(a["control"]["saturated"])
    plain = case_input("CA", ivp, with_control=False)
    plain["solver-config"]["monitor"] = {"times": [float(x) for x in a["control"]["time"]]}
    b = rmtExe(plain)["resModel"]
    assert b["device-stats"]["launches"] == a["device-stats"]["launches"] and "control" not in b
    same_states(a["dataPack"], b["dataPack"])


# ----------------------------------------------------------------------------- 6. ensemble
@pytest.mark.parametrize("ivp", ["hip-rk45", "hip-ros4"])
def test_every_member_runs_its_own_loop(ivp):
    """Every member of the CD ensemble against its own single-member run (both are within the stepper's bound of the
    same exact solution: twice the bound)."""
    base = case_input("CD", ivp)
    res = rmtExe(base)["resModel"]
    members = expand_members(base, base["solver-config"]["ensemble"])
    assert len(res["ensemble"]) == len(members) == 4
    worst = worst_u = 0.0
    for e, mem in enumerate(members):
        single = dict(mem)
        single["solver-config"] = {k: v for k, v in base["solver-config"].items() if k != "ensemble"}
        one = rmtExe(single)["resModel"]
        for k in range(len(one["dataPack"])):
            a, b = np.asarray(res["ensemble"][e]["dataPack"][k]["dataYs"]), np.asarray(one["dataPack"][k]["dataYs"])
            worst = max(worst, float(np.max(np.abs(a[:S] - b[:S]))), float(np.max(np.abs(a[S] - b[S])/b[S])))
        worst_u = max(worst_u, float(np.max(np.abs(res["ensemble"][e]["control"]["output"] - one["control"]["output"]))))
        assert res["ensemble"][e]["control"]["output"][0] != members[e]["operating-conditions"]["pressure"]
    print("G15 CD %s: every member against its own single run: %.3e (max|du| = %.3e Pa)" % (ivp, worst, worst_u))
    assert worst <= 2*STEPPERS[ivp][1], worst
