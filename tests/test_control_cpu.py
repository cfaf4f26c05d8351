"""solver-config "control" without a GPU: validation (through rmtExe, before any device work), sample times and the
refined launch list, the control law in numpy against the logs of golden G15 (tools/make_golden.py control), the
parameter blocks against plan.forced_fields, the cross-compilation of the kernel's translation unit - and that a run without
the key is the run it was."""
import copy
import ctypes
import json
import os
import types

import numpy as np
import pytest

import inputs as INP
from rmt_app_amd import control, hipbind, isa, launches, monitor, plan, rmtExe, schedule
from rmt_app_amd import n2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(G, "g15_control.json")) as _f:
    CASES = json.load(_f)["cases"]

PI = {"measured": "outlet-temperature", "manipulated": "inlet-pressure", "setpoint": 620.0, "sample-time": 0.01,
      "start": 0.1, "gain": 5.0e4, "integral-time": 0.05, "limits": [4.0e6, 6.0e6]}


def _input(model="N2", ivp="hip-rk4", period=0.4, **ctl):
    mi = INP.dme_notebook_input(ivp=ivp, period=period) if model != "M2" else INP.m2_dme_input(ivp=ivp, period=period)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 4, "display-result": "False"})
    mi["solver-config"]["control"] = {**PI, **ctl}
    return mi


def _raises(mi, kind, word, capsys):
    with pytest.raises(kind, match="control") as e:          # through rmtExe, before any device work (there is no device
        rmtExe(mi)                                            # here: anything later raises RmtN2Error)
    assert word in str(e.value), str(e.value)
    capsys.readouterr()


# ----------------------------------------------------------------------------- validation
BAD = [
    ({"measured": "inlet-temperature"}, "measured"),
    ({"measured": {"outlet-mole-fraction": "N2"}}, "shell component"),
    ({"measured": {"mole-fraction": "DME"}}, "measured"),
    ({"manipulated": "feed"}, "manipulated"),
    ({"sample-time": 0.0}, "sample-time"),
    ({"sample-time": "0.01"}, "sample-time"),
    ({"start": -0.1}, "start"),
    ({"start": 0.4}, "start"),
    ({"gain": None}, "gain"),
    ({"gain": float("nan")}, "gain"),
    ({"integral-time": 0.0}, "integral-time"),
    ({"integral-time": -1.0}, "integral-time"),
    ({"limits": [6.0e6, 4.0e6]}, "limits"),
    ({"limits": [0.0, 4.0e6]}, "limits"),
    ({"limits": [4.0e6]}, "limits"),
    ({"limits": None}, "limits"),
    ({"setpoint": {"time": [0.1, 0.2], "value": [1.0, 2.0]}}, "setpoint"),
    ({"setpoint": {"time": [0.0, 0.2, 0.1], "value": [1.0, 2.0, 3.0]}}, "setpoint"),
    ({"setpoint": {"time": [0.0, 0.2], "value": [1.0]}}, "setpoint"),
    ({"setpoint": "high"}, "setpoint"),
    ({"derivative-time": 0.1}, "derivative-time"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    _raises(_input(**spec), ValueError, word, capsys)


@pytest.mark.parametrize("key", ["measured", "manipulated", "setpoint", "sample-time", "gain", "limits"])
def test_required_keys(key, capsys):
    mi = _input()
    del mi["solver-config"]["control"][key]
    _raises(mi, ValueError, key, capsys)


def test_the_errors_of_schedule_apply(capsys):
    for model in ("M2", "N1", "M7"):
        _raises(_input(model), ValueError, "only available for model 'N2'", capsys)
    for ivp in ("AM", "hip-ab3"):
        _raises(_input(ivp=ivp), ValueError, "ivp", capsys)
    mi = _input()
    mi["solver-config"]["dtype"] = "fp32"
    _raises(mi, ValueError, "fp32", capsys)
    mi = _input(manipulated="medium-temperature", limits=[400.0, 600.0])
    mi["external-heat"]["MeTe"] = 0
    _raises(mi, ValueError, "MeTe", capsys)
    for spec in ({"manipulated": "inlet-temperature", "limits": [400.0, 600.0],
                  "measured": {"outlet-mole-fraction": "DME"}},
                 {"manipulated": "medium-temperature", "limits": [400.0, 600.0],
                  "measured": {"outlet-mole-fraction": "DME"}},
                 {"measured": "peak-temperature"}):
        mi = _input(**spec)
        mi["operating-conditions"]["process-type"] = "iso-thermal"
        _raises(mi, ValueError, "iso-thermal", capsys)
    # a quantity has one master
    mi = _input()
    mi["solver-config"]["schedule"] = {"time": [0.0, 0.4], "inlet-pressure": [5.0e6, 4.9e6]}
    _raises(mi, ValueError, "'inlet-pressure'", capsys)
    mi = _input()                                                  # ... a member's own schedule as well
    mi["solver-config"]["schedule"] = {"time": [0.0, 0.4], "medium-temperature": [523.0, 533.0]}
    mi["solver-config"]["ensemble"] = [{}, {"solver-config": {"schedule": {"inlet-pressure": [5.0e6, 4.9e6]}}}]
    _raises(mi, ValueError, "'inlet-pressure'", capsys)


def test_multi_rank_runs_are_refused(monkeypatch, capsys):
    mi = _input()
    mi["solver-config"]["ensemble"] = {"temperature": [518.0, 528.0]}
    monkeypatch.setattr(n2, "active_ranks", lambda n: types.SimpleNamespace(counts=[1, 1], lo=0, hi=1, rank=0, world=2))
    _raises(mi, NotImplementedError, "multi-rank", capsys)


def test_members_override_the_law_not_the_times(capsys):
    mi = _input()
    mi["solver-config"]["ensemble"] = [{}, {"solver-config": {"control": {"sample-time": 0.02}}}]
    _raises(mi, ValueError, "sample-time", capsys)
    base = _input()
    members = [base, copy.deepcopy(base), copy.deepcopy(base)]
    members[1]["solver-config"]["control"] = {"gain": -2.0e4, "integral-time": None, "limits": [4.5e6, 5.5e6]}
    members[2]["solver-config"]["control"] = {"setpoint": {"time": [0.0, 0.2, 0.2], "value": [620.0, 620.0, 618.0]}}
    members[2]["operating-conditions"]["pressure"] = 4.8e6
    ctl, sched = control.parse(base, members, "hip-rk4")
    assert ctl.E == 3 and ctl.K == 30 and sched.E == 3 and sched.given == (False, False, False)
    assert list(ctl.Kp) == [5.0e4, -2.0e4, 5.0e4]
    assert list(ctl.Ki) == [5.0e4*0.01/0.05, 0.0, 5.0e4*0.01/0.05]
    assert list(ctl.u0) == [5.0e6, 5.0e6, 4.8e6] and list(ctl.lo) == [4.0e6, 4.5e6, 4.0e6]
    assert np.all(ctl.setpoints[:, :2] == 620.0)
    assert list(ctl.setpoints[[9, 10, 11], 2]) == [620.0, 618.0, 618.0]          # the jump at 0.2 holds from 0.2 on
    # the constant schedule of a run without "schedule": every member's own values
    assert np.array_equal(sched.values[:, :, 0], [[523.0, 5.0e6, 523.0], [523.0, 5.0e6, 523.0], [523.0, 4.8e6, 523.0]])
    span = np.linspace(0.0, 0.4, 5)
    assert sched.forcing_level == "1"
    assert [l[:3] for l in launches.merge(0.4, 4, sched.times)[0]] == [(float(span[i]), float(span[i + 1]), i + 1)
                                                                       for i in range(4)]


# ----------------------------------------------------------------------------- sample times, launch lists
def test_sample_times():
    t = control.sample_times(0.1, 0.01, 0.4)
    assert len(t) == 30 and t[0] == 0.1 and t[-1] == 0.1 + 29*0.01 and np.all(t < 0.4)
    assert list(control.sample_times(0.0, 0.1, 0.25)) == [0.0, 0.1, 0.2]
    assert len(control.sample_times(0.0, 0.1, 0.3)) == 3            # t_k < period: 0.30000000000000004 is the period
    assert len(control.sample_times(0.35, 1.0, 0.4)) == 1


def test_refine_merges_with_output_times_breakpoints_and_monitor_samples():
    mi = _input(start=0.05, **{"sample-time": 0.05})
    mi["solver-config"]["tNo"] = 2
    mi["solver-config"]["schedule"] = {"time": [0.0, 0.15, 0.15, 0.4], "medium-temperature": [523.0, 523.0, 533.0, 533.0]}
    mi["solver-config"]["monitor"] = {"times": [0.1, 0.12]}
    sched = schedule.parse(mi, None, "hip-rk4")
    ctl, forced_by = control.parse(mi, None, "hip-rk4", sched)
    assert forced_by is sched and ctl.K == 7
    mon = monitor.parse(mi, 2)
    L, _, times = launches.merge(0.4, 2, sched.times, mon.times, ctl.times)
    t = [l[0] for l in L] + [L[-1][1]]
    assert np.allclose(t, [0.0, 0.05, 0.1, 0.12, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4], rtol=0, atol=1e-15)
    assert all(a[1] == b[0] for a, b in zip(L[:-1], L[1:]))
    # (t0, t1, output ended at, monitor sample ended at, control sample taken at the start)
    assert [l.out for l in L] == [None, None, None, None, 1, None, None, None, 2]
    assert [l.sample for l in L] == [None, 1, 2, None, None, None, None, None, None]
    assert [l.control for l in L] == [None, 0, 1, None, 2, 3, 4, 5, 6]
    # a sample that coincides with a breakpoint (0.15), with an output time (0.2) and with a monitor sample (0.1) carries
    # that mark's value, bit for bit
    assert times[2] == 0.15 and times[3] == 0.2 and times[1] == 0.1 and L[5].t0 == 0.2
    # a controller that starts at 0 samples ahead of the first launch
    ctl0, _ = control.parse(_input(start=0.0, **{"sample-time": 0.1}), None, "hip-rk4")
    L0 = launches.merge(0.4, 4, controls=ctl0.times)[0]
    assert [l.control for l in L0] == [0, 1, 2, 3] and len(L0) == 4


def test_without_the_key_nothing_changes():
    mi = _input()
    del mi["solver-config"]["control"]
    assert control.parse(mi, None, "hip-rk4") == (None, None)
    mi["solver-config"]["schedule"] = {"time": [0.0, 0.13, 0.4], "medium-temperature": [523.0, 533.0, 533.0]}
    mi["solver-config"]["monitor"] = {"samples": 2}
    sched = schedule.parse(mi, None, "hip-rk4")
    assert control.parse(mi, None, "hip-rk4", sched) == (None, sched)
    mon = monitor.parse(mi, 4)
    span = np.linspace(0, 0.4, 5)
    # the list of the run without "control": output times 0.1 .. 0.4, the breakpoint 0.13, samples half way and at the ends
    want = [(0.0, 0.05, None, 1), (0.05, 0.1, 1, 2), (0.1, 0.13, None, None), (0.13, 0.15000000000000002, None, 3),
            (0.15000000000000002, 0.2, 2, 4), (0.2, 0.25, None, 5), (0.25, 0.30000000000000004, 3, 6),
            (0.30000000000000004, 0.35000000000000003, None, 7), (0.35000000000000003, 0.4, 4, 8)]
    L = launches.merge(0.4, 4, sched.times, mon.times, None)[0]
    assert [l[:4] for l in L] == want
    assert all(l.control is None for l in L)
    plain = [(float(span[i]), float(span[i + 1]), i + 1, None, None) for i in range(4)]
    assert launches.merge(0.4, 4)[0] == plain
    # the code object of an uncontrolled run: same plan, same cache key as before the controller existed
    mech = plan.Mechanism(mi)
    row = plan.member_constants(mi, mech, 20)[1]
    cp = n2.code_plan(mech, 20, rows=row)
    assert "RMT_FORCING" not in cp.defines
    assert n2.plan_unit(mech, False, cp)[1] == mech.digest(hipbind.kernel_template(), False, cp.block, cp.npt, cp.lds_state,
                                                           cp.defines)
    assert "rmt_n2_control" not in hipbind.kernel_template()        # the stepper template does not know the controller


# ----------------------------------------------------------------------------- the law
def _g15_logs():
    for name, c in CASES.items():
        g = np.load(os.path.join(G, "g15_control_%s.npz" % name))
        for m in c.get("members", [None]):
            yield name, m, c, g["log" if m is None else "log_%d" % m]


def _case_control(c, m, ivp="hip-rk4"):
    mi = INP.ALL_N2_INPUTS[c["input"]](ivp=ivp, period=c["period"])
    mi["solver-config"].update({"zNo": c["zNo"], "tNo": c["tNo"], "quiet": True, "control": copy.deepcopy(c["control"])})
    if c.get("schedule"):
        mi["solver-config"]["schedule"] = copy.deepcopy(c["schedule"])
    members = None
    if "ensemble" in c:
        from rmt_app_amd.ensemble import expand_members
        members = expand_members(mi, c["ensemble"])
    sched = schedule.parse(mi, members, ivp)
    return control.parse(mi, members, ivp, sched)[0]


def test_emulate_reproduces_the_g15_logs_bit_for_bit():
    seen = 0
    for name, m, c, log in _g15_logs():
        ctl = _case_control(c, m)
        e = 0 if m is None else m
        assert np.array_equal(ctl.times, log[:, 0]), name                    # the generator's sample times
        assert np.array_equal(ctl.setpoints[:, e], log[:, 2]), name          # ... and setpoints r(t_k)
        u, sat, _ = control.emulate(log[:, 1], log[:, 2], ctl.Kp[e], ctl.Ki[e], ctl.u0[e], ctl.lo[e], ctl.hi[e])
        assert np.array_equal(u, log[:, 3]), (name, m, np.max(np.abs(u - log[:, 3])))
        assert np.array_equal(sat, log[:, 4] != 0), (name, m)
        seen += 1
    assert seen == 5


def test_the_law_saturation_and_anti_windup():
    # P only: no integral state, whatever the error
    u, sat, I = control.emulate([619.0, 622.0], 620.0, 5.0e4, 0.0, 5.0e6, 4.0e6, 6.0e6)
    assert list(u) == [5.05e6, 4.9e6] and not sat.any() and list(I) == [0.0, 0.0]
    # PI: I' = I + Ki e, v = u0 + Kp e + I'
    u, sat, I = control.emulate([619.0, 619.0], 620.0, 5.0e4, 1.0e4, 5.0e6, 4.0e6, 6.0e6)
    assert list(I) == [1.0e4, 2.0e4] and list(u) == [5.06e6, 5.07e6]
    # saturated: u sits at the limit and the integral does NOT move; it moves again once v is inside
    u, sat, I = control.emulate([600.0, 600.0, 619.5], 620.0, 5.0e4, 1.0e4, 5.0e6, 4.0e6, 5.5e6)
    assert list(u) == [5.5e6, 5.5e6, 5.0e6 + 2.5e4 + 5.0e3] and list(sat) == [True, True, False]
    assert list(I) == [0.0, 0.0, 5.0e3]
    # gain 0: the member's own value, exactly
    u, sat, I = control.emulate([600.0, 640.0], 620.0, 0.0, 0.0, 4.8e6, 4.0e6, 6.0e6)
    assert list(u) == [4.8e6, 4.8e6] and not sat.any()
    # a NaN measurement: u is NaN (the steppers flag it), flagged as not free, the integral keeps its value
    u, sat, I = control.emulate([619.0, float("nan")], 620.0, 5.0e4, 1.0e4, 5.0e6, 4.0e6, 6.0e6)
    assert np.isnan(u[1]) and sat[1] and I[1] == I[0]


def test_setpoint_is_piecewise_linear_with_jumps():
    T, v = [0.0, 0.1, 0.1, 0.3], [1.0, 1.0, 2.0, 4.0]
    assert control.setpoint_at(T, v, 0.05) == 1.0 and control.setpoint_at(T, v, 0.1) == 2.0
    assert control.setpoint_at(T, v, 0.2) == 2.0 + 2.0*(0.2 - 0.1)/(0.3 - 0.1) and control.setpoint_at(T, v, 0.35) == 4.0
    assert control.setpoint_at(T, v, 0.1 - 1e-14, tol=1e-13) == 2.0 and control.setpoint_at(T, v, 0.1 - 1e-14) == 1.0


# ----------------------------------------------------------------------------- rows, parameter blocks
@pytest.mark.parametrize("key,u", [("inlet-temperature", 531.25), ("inlet-pressure", 4.87e6), ("medium-temperature", 517.5)])
def test_row_value_and_scaling_equal_forced_fields(key, u):
    mi = _input(manipulated=key, limits=[0.5*u, 2*u])
    mi["operating-conditions"]["temperature"] = 519.0               # Tf != the manipulated temperature
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, 20)
    ctl, sched = control.parse(mi, None, "hip-rk4")
    prm = ctl.params()
    assert prm.shape == (1, control.PARAMS) and prm[0, control.P_U0] == schedule._own(mi, key)
    assert list(prm[0, :2]) == [5.0e4, 5.0e4*0.01/0.05] and list(prm[0, 3:7]) == [0.5*u, 2*u, 0.0, 0.0]
    assert ctl.field == schedule.ORDER.index(key)
    # what plan.forced_fields writes for (T_in, P_in, MeTe) with u at the manipulated position
    values = sched.at(0.0)
    values[0, ctl.field] = u
    want = plan.forced_fields(np.array([row]), [named], values)[0]
    idx, slope = control.row_field(key)
    got = row.copy()
    got[idx] = control.field_value(key, u, row[plan.MEMBER_FIELDS["TF"]])
    assert np.array_equal(got, want) and got[idx] != row[idx]
    # the slope that goes with the field in the tail of a forced row
    forced = sched.forced_rows(np.array([row]), [named], 0.0, 0.1)[0]
    assert len(forced) == mech.row_width + schedule.TAIL and forced[mech.row_width] == 0.0
    s = np.zeros((1, 3))
    s[0, ctl.field] = 1.0
    assert np.nonzero(plan.forced_slopes([named], s)[0])[0][0] + 1 == slope


def test_mole_fraction_selector_and_species_index():
    ctl, _ = control.parse(_input(measured={"outlet-mole-fraction": "DME"}, setpoint=0.015), None, "hip-rk4")
    assert ctl.select == 2 and ctl.species == 5 and list(ctl.params()[0, 5:7]) == [2.0, 5.0]
    assert control.parse(_input(measured="peak-temperature"), None, "hip-rk4")[0].select == 1


# ----------------------------------------------------------------------------- compilation, exports
def test_control_kernel_cross_compiles_without_contraction():
    src = hipbind.control_source()
    assert src == open(os.path.join(ROOT, "rmt_app_amd", "csrc", "control_kernels.inc")).read()
    assert hipbind.CONTROL_OPTS == "-ffp-contract=off"
    blob = hipbind.control_code("gfx950")
    assert blob[:4] == b"\x7fELF"
    assert any(f.startswith("control-") and f.endswith("-gfx950.hsaco") for f in os.listdir(hipbind.CACHE_DIR))
    res = isa.kernel_resources(blob, "rmt_n2_control_update_f64")
    assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == 0
    mix = isa.kernel_stats(blob, "rmt_n2_control_update_f64")["whole"]
    assert mix["scratch"] == 0 and mix["vmem"] > 0
    L = ctypes.CDLL(hipbind.LIB_PATH)
    for name in ("rmt_n2_control_source", "rmt_n2_control_create", "rmt_n2_control_update", "rmt_n2_control_destroy"):
        assert hasattr(L, name), name
    assert hipbind.lib().rmt_n2_abi_version() == 2                   # additions only
    # the constants the kernel restates
    F = plan.MEMBER_FIELDS
    for name, val in (("RMT_CTL_M_TF", F["TF"]), ("RMT_CTL_M_P0", F["P0"]), ("RMT_CTL_M_THETA_IN", F["THETA_IN"]),
                      ("RMT_CTL_M_TM", F["TM"]), ("RMT_CTL_PARAMS", control.PARAMS), ("RMT_CTL_STATE", control.STATE),
                      ("RMT_CTL_LOG", control.LOG)):
        assert "#define %s %d" % (name, val) in src, name
