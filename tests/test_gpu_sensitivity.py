"""solver-config "sensitivity" on the device: the kernel rmt_n2_steady_sens through rmtExe and through
N2Device.steady_sens, against the goldens G21 (tools/make_golden.py sensitivity, tests/sens_ref.py), against the host
emulation of the same unit, and against central differences of runs that use nothing of the feature.

Bounds:
* against G21, per (parameter, row): 10 x the golden's fd_error + the case's sens_ref.FLOOR_REL of the row's largest magnitude (sens_ref.bound,
  the bound of tests/test_sensitivity_cpu.py);
* device against the host emulation of the same unit on the same state: 1e-8 of the row's largest magnitude - the bound the
  march's device test holds its states to (tests/test_gpu_initial.py STATE_BOUND); the device divides and exponentiates with
  its lean fp64 forms, the host with the library's;
* the independent check: central differences at d and d/2 of the monitor's sample-0 values of members whose coolant is
  offset by a constant relative "schedule"; Richardson value against the analytic one within 10 x |D(d/2) - D(d)| + FLOOR_REL
  of the value; the same for the whole state row [V][N] from the members' packed profiles, per variable with
  fd_error = max_z |D(d/2) - D(d)| and the floor of the row's largest magnitude.  d = 4e-4 MeTe: the difference of the two quotients is then truncation (deterministic), not the noise of
  the marched states (1e-10 relative, 3e-7 of the quotient).
Each test prints its figures."""
import os
import subprocess

import numpy as np
import pytest

import inputs as INP
from helpers.host_build import build_helper
import sens_ref as SR
from rmt_app_amd import n2, plan, rmtExe, sensitivity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "sens_emu.cpp")
FLOOR_REL = SR.FLOOR_REL["SA"]         # the floor of the plain dme_nb bed (tests/sens_ref.py)
EMU_BOUND = 1e-8         # tests/test_gpu_initial.py STATE_BOUND
F = plan.MEMBER_FIELDS


def run_input(zNo=20, period=0.05, tNo=2, params=("medium-temperature",), **cfg):
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=period)
    mi["solver-config"].update({"zNo": zNo, "tNo": tNo, "quiet": True, "initial": "steady"})
    if params is not None:
        mi["solver-config"]["sensitivity"] = {"parameters": list(params)}
    mi["solver-config"].update(cfg)
    return mi


def rows_of(entry):
    """[P][V+1][N] of a result entry: the golden's rows"""
    return np.concatenate([entry["state"], entry["pressure"][:, None, :]], axis=1)


def open_unit(mi, members=None, pick=None, rows=None):
    """A handle of the sensitivity unit on the members' rows: (device, sens, named, rows).  ``pick``: only these members'
    rows (their own handle); ``rows``: replace the rows."""
    zNo = mi["solver-config"]["zNo"]
    inputs = members or [mi]
    sens = sensitivity.parse(mi, members)
    base = n2.mechanism_for(mi, inputs, mi["solver-config"])
    sens.mech = mech = plan.Mechanism(mi, params=sens.unit_params(base.params))
    pairs = [plan.member_constants(m, mech, zNo) for m in inputs]
    named = [nm for nm, _ in pairs]
    allrows = np.array([r for _, r in pairs]) if rows is None else np.array(rows)
    if pick is not None:
        allrows, named = allrows[list(pick)], [named[e] for e in pick]
    sens.rows = allrows
    cp = n2.sens_plan(mech, zNo, sens.NP, None, allrows)
    dev = n2.N2Device(mech, allrows, zNo, block=cp.block, npt=cp.npt, specialize=False, features=cp.features,
                      defines=cp.defines)
    return dev, sens, named, allrows


def direct(mi, members=None, pick=None):
    """N2Device.steady_march + steady_sens on such a handle: (raw [E][NP][V+1][N], flags, state [E][V*N], sens, named, rows)"""
    dev, sens, named, rows = open_unit(mi, members, pick)
    try:
        y = dev.to_device(np.zeros((len(rows), sens.mech.V*dev.N)))
        dev.steady_march(y)
        st, flags = dev.march_result()
        assert not np.any(flags), flags
        kinds, idx = sens.descriptors(sens.mech)
        raw = dev.steady_sens(y, kinds, idx).cpu().numpy()
        return raw, dev.sens_status(), y.cpu().numpy(), sens, named, rows
    finally:
        dev.close()


# ----------------------------------------------------------------------------- 1. the golden cases through rmtExe
@pytest.mark.parametrize("name", ["SA", "SB", "SK"])
def test_rmtexe_against_the_golden_sensitivities(name):
    res = rmtExe(SR.case_input(name, ivp="hip-ros4"))["resModel"]
    entry, gold = res["sensitivity"], SR.golden(name)
    got = rows_of(entry)
    diff = np.max(np.abs(got - gold["D"]), axis=2)
    mag = np.max(np.abs(gold["D"]), axis=2)
    rel = np.where(mag > 0, diff/np.where(mag > 0, mag, 1.0), 0.0)
    print("G21 %s on the device: largest |sensitivity - golden| / max|row| = %.3e (golden fd_error / max|row| at most %.3e); "
          "normalized peak sensitivities %s at z = %.3f" % (name, rel.max(), SR.meta()["cases"][name]["fd_error_relative"],
                                                            entry["normalized-peak"], entry["peak-position"]))
    assert entry["parameters"] == SR.meta()["cases"][name]["labels"]
    assert np.allclose(entry["values"], gold["values"], rtol=1e-14, atol=0)
    assert np.all(diff <= SR.bound(gold, name)), np.argwhere(diff > SR.bound(gold, name))
    # the peak row is the temperature row at the node of the discrete maximum of the golden state
    S = len(entry["labelList"]) - 1
    n = int(np.argmax(gold["rows"][S]))
    assert entry["peak-position"] == np.linspace(0, 1, got.shape[2])[n]
    assert np.array_equal(entry["peak-temperature"], entry["state"][:, S, n])
    assert np.allclose(entry["normalized-peak"], gold["values"]/gold["rows"][S, n]*gold["D"][:, S, n], rtol=1e-4, atol=1e-12)
    assert "initial" in res and len(res["dataPack"]) == 2


# ----------------------------------------------------------------------------- 2. device against host emulation
def test_device_buffer_against_the_host_emulation_of_the_same_unit(tmp_path):
    mi = SR.case_input("SK", ivp="hip-ros4")
    raw, flags, y, sens, named, rows = direct(mi)
    assert not np.any(flags)
    mech, N = sens.mech, 20
    src, _ = n2.plan_unit(mech, False, n2.sens_plan(mech, N, sens.NP, None, rows))
    exe = build_helper(HELPER, src, str(tmp_path), "sk", "sens_emu")
    kinds, idx = sens.descriptors(mech)
    hexes = lambda v: " ".join(float(x).hex() for x in np.ravel(v))
    text = "M %s\nS %d %s %s\n" % (hexes(rows[0]), N, " ".join("%d %d" % (k, i) for k, i in zip(kinds, idx)), hexes(y[0]))
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.split("\n") if ln.startswith("out")][0].split()[1:]
    emu = np.array([float.fromhex(v) for v in line]).reshape(raw[0].shape)
    scale = np.max(np.abs(emu), axis=2, keepdims=True)
    err = np.max(np.abs(raw[0] - emu)/np.where(scale > 0, scale, 1.0))
    print("device against host emulation (SK, the same converged state): %.3e of the row's largest magnitude" % err)
    assert np.all(np.abs(raw[0] - emu) <= EMU_BOUND*scale)


# ----------------------------------------------------------------------------- 3. an ensemble over two workgroups
def test_sixty_five_members_of_a_coolant_sweep_each_its_own():
    """65 members: the second workgroup holds one live lane and 63 dead ones.  One launch through rmtExe and one on a
    handle of the unit; EVERY member equals the single-member run of its own rows bit for bit (one E = 1 handle of the same
    unit, its row replaced member by member), in the device buffer and in rmtExe's result entry."""
    params = ("medium-temperature", "inlet-temperature")
    mi = run_input(params=params)
    levels = np.linspace(503.0, 543.0, 65)
    spec = [{"external-heat": {"MeTe": float(v)}} for v in levels]
    mi["solver-config"]["ensemble"] = spec
    res = rmtExe(mi)["resModel"]
    assert len(res["ensemble"]) == 65
    s = np.array([m["sensitivity"]["normalized-peak"] for m in res["ensemble"]])
    k = int(np.argmax(np.abs(s[:, 0])))
    print("coolant sweep 503 .. 543 K: the normalised sensitivity of the peak temperature to the coolant temperature runs "
          "%.3f .. %.3f, largest %.3f at MeTe = %.2f K" % (s[:, 0].min(), s[:, 0].max(), s[k, 0], levels[k]))
    assert np.all(np.isfinite(s)) and np.all(s[:, 0] > 0)
    from rmt_app_amd.ensemble import expand_members
    base = run_input(params=params)
    members = expand_members(base, spec)
    raw, flags, y, sens, named, rows = direct(base, members)
    assert raw.shape == (65, 2, 8, 20) and not np.any(flags)
    dev1, sens1, _, _ = open_unit(base, members, pick=[0])
    try:
        kinds, idx = sens1.descriptors(sens1.mech)
        for e in range(65):
            dev1.set_members(rows[e:e + 1])
            y1 = dev1.to_device(np.zeros((1, sens1.mech.V*20)))
            dev1.steady_march(y1)
            st, f1 = dev1.march_result()
            one = dev1.steady_sens(y1, kinds, idx).cpu().numpy()
            assert not np.any(f1) and not np.any(dev1.sens_status()), e
            assert np.array_equal(one[0], raw[e]) and np.array_equal(y1.cpu().numpy()[0], y[e]), e
            entry = sensitivity.result_entry(sens1, one[0], y1.cpu().numpy()[0], rows[e], named[e], sens1.mech)
            got = res["ensemble"][e]["sensitivity"]
            for key in ("state", "pressure", "outlet-mole-fraction", "peak-temperature", "normalized-peak", "values"):
                assert np.array_equal(entry[key], got[key]), (e, key)
            assert entry["peak-position"] == got["peak-position"], e
    finally:
        dev1.close()
    assert np.max(np.abs(raw[0] - raw[64])) > 1e-3                  # (the members do differ)


# ----------------------------------------------------------------------------- 4. against differences of plain runs
def test_analytic_row_against_differences_of_runs_with_offset_coolant():
    """Only code from before the feature: members whose constant relative "schedule" offsets the coolant by +-d and +-d/2
    start from their steady states; the monitor's sample 0 gives their outlet and peak temperature."""
    period, d = 0.01, 4e-4*523.0
    base = run_input(period=period, tNo=1, params=None, monitor={"times": [period]},
                     schedule={"time": [0.0, period], "relative": True, "medium-temperature": [0.0, 0.0]})
    offs = [0.0, d, -d, 0.5*d, -0.5*d]
    base["solver-config"]["ensemble"] = [{"solver-config": {"schedule": {"medium-temperature": [o, o]}}} if o else {}
                                         for o in offs]
    res = rmtExe(base)["resModel"]
    assert "sensitivity" not in res
    val = np.array([np.concatenate([m["monitor"]["outlet"][0], [m["monitor"]["peak-temperature"][0]]])
                    for m in res["ensemble"]])                   # [5][S + 2]: outlet mole fractions, outlet T, peak T
    D1, D2 = (val[1] - val[2])/(2*d), (val[3] - val[4])/d
    rich, fd_error = (4*D2 - D1)/3, np.abs(D2 - D1)
    ana = rmtExe(run_input(period=period, tNo=1))["resModel"]["sensitivity"]
    S = len(ana["labelList"]) - 1
    got = np.concatenate([ana["outlet-mole-fraction"][0], [ana["state"][0, S, -1], ana["peak-temperature"][0]]])
    bound = 10*fd_error + FLOOR_REL*np.abs(rich)
    print("analytic d/dMeTe of (outlet mole fractions, outlet T, peak T) against Richardson differences of plain runs:\n"
          "  analytic %s\n  |analytic - differences| %s\n  fd_error %s" % (got, np.abs(got - rich), fd_error))
    assert res["ensemble"][0]["monitor"]["peak-position"][0] == ana["peak-position"]
    assert np.all(np.abs(got - rich) <= bound), np.abs(got - rich)/bound
    # ... and the whole "medium-temperature" row of the state [V][N] against the members' packed profiles (dataYCons2,
    # dataYTemp2 at t = 0.01 s: the bed has not moved from its steady state; the pressure is not in a dataPack entry)
    prof = np.array([np.concatenate([np.asarray(m["dataPack"][0]["dataYCons2"]), np.asarray(m["dataPack"][0]["dataYTemp2"])])
                     for m in res["ensemble"]])                  # [5][V][N]
    P1, P2 = (prof[1] - prof[2])/(2*d), (prof[3] - prof[4])/d
    prich, perr = (4*P2 - P1)/3, np.max(np.abs(P2 - P1), axis=1)
    pdiff = np.max(np.abs(ana["state"][0] - prich), axis=1)
    pbound = 10*perr + FLOOR_REL*np.max(np.abs(prich), axis=1)
    print("the whole row d(state)/dMeTe [V][N] against Richardson differences of the packed profiles, per variable:\n"
          "  largest |analytic - differences| %s\n  fd_error %s\n  largest magnitude %s"
          % (pdiff, perr, np.max(np.abs(prich), axis=1)))
    assert prof.shape[1:] == ana["state"][0].shape and np.all(pdiff <= pbound), pdiff/pbound


# ----------------------------------------------------------------------------- 5. nothing else of the run changes
@pytest.mark.parametrize("name", ["SA", "SK"])
def test_the_run_itself_is_the_run_without_the_key(name):
    """SA: the sensitivity unit in the place of the march unit; SK: a rate constant that the run keeps a literal - the march
    stays on the plain march unit, the sweep has a handle of its own."""
    with_key = rmtExe(SR.case_input(name, ivp="hip-ros4"))["resModel"]
    plain_in = SR.case_input(name, ivp="hip-ros4")
    del plain_in["solver-config"]["sensitivity"]
    plain = rmtExe(plain_in)["resModel"]
    assert "sensitivity" in with_key and "sensitivity" not in plain
    assert with_key["initial"] == plain["initial"]
    assert len(with_key["dataPack"]) == len(plain["dataPack"]) == 2
    for a, b in zip(with_key["dataPack"], plain["dataPack"]):
        for key in ("dataYs", "dataYCons1", "dataYCons2", "dataYTemp1", "dataYTemp2", "dataTime"):
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


# ----------------------------------------------------------------------------- 6. a singular node
def test_a_singular_node_raises_naming_member_and_node():
    """Member 1's rows have no convection and no reaction term in the species balances (F1 = FM = 0): the species rows of
    its node Jacobian vanish, the first pivot is zero.  Plain data - nothing faults."""
    mi = run_input(params=("medium-temperature", "inlet-pressure"))
    raw, flags, y, sens, named, rows = direct(mi, [mi, mi])
    assert not np.any(flags)
    bad = rows.copy()
    bad[1, F["F1"]] = bad[1, F["INV_MACOTE"]] = 0.0
    dev, sens2, named2, _ = open_unit(mi, [mi, mi], rows=bad)
    try:
        kinds, idx = sens2.descriptors(sens2.mech)
        yd = dev.to_device(y)                                     # (the good rows' steady state for both members)
        raw2 = dev.steady_sens(yd, kinds, idx).cpu().numpy()
        flags2 = dev.sens_status()
        assert list(flags2) == [0, 8]                              # RMT_N2_FLAG_NONFINITE on member 1 only
        assert np.array_equal(raw2[0], raw[0])
        assert sensitivity.failed_node(raw2[1]) == 0 and np.all(np.isnan(raw2[1][:, :, 0])) and not np.any(raw2[1][:, :, 1:])
        with pytest.raises(FloatingPointError, match=r"'sensitivity'.*node 0 of member 1.*0x8"):
            n2.start_sensitivity(dev, yd, sens2, named2)
    finally:
        dev.close()
