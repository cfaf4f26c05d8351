"""solver-config "axial-profile" on the device: catalyst activity and coolant offset per mesh node.

* the right-hand side and ten RK4 steps of a profiled N2Device against the oracle with the profile applied
  (tests/profile_ref.py), row-relative < 1e-12 (the bound of tests/test_gpu_parity.py), at the smallest shapes at which the
  table's indexing can go wrong: 20 nodes on one wave (44 lanes beyond the end), 101 nodes at two nodes per lane (odd
  length), 300 nodes in three node blocks (the last partial), and the unit a profiled run gets at 512 x 2;
* rmtExe against the goldens G18 (tools/make_golden.py profile: SciPy at rtol 1e-10 / atol 1e-13 on the profiled oracle
  RHS) with the settings and bounds of tests/test_gpu_schedule.py: 1e-8 (hip-rk4), 1e-6 (hip-rk45, hip-ros4, default) on
  max|dMoFri| and max|dT|/T over all nodes and output times;
* the key together with "initial": "steady", "schedule" and "monitor" (bounds of tests/test_gpu_initial.py);
* the stiff stepper's analytic Jacobian against its forward-difference form on the profiled bed;
* the library's guards."""
import copy
import os

import numpy as np
import pytest

import inputs as INP
import profile_ref as PR
from oracle import n2_oracle as O
from parity import rowwise_err
from rmt_app_amd import hipbind, n2, plan, rmtExe
from rmt_app_amd.n2 import N2Device

pytestmark = pytest.mark.gpu
GOLD = PR.GOLD
STEPPERS = {                                     # tests/test_gpu_schedule.py STEPPERS
    "hip-rk4": ({"dt": 2.5e-6}, 1e-8),
    "hip-rk45": ({"rtol": 1e-8, "atol": 1e-11}, 1e-6),
    "hip-ros4": ({}, 1e-6),
    "default": ({}, 1e-6),
}
STATE_BOUND = 1e-8                               # tests/test_gpu_initial.py
# attempted steps (accepted + rejected) of hip-ros4 on the plain twin of case A, analytic against forward-difference node
# Jacobian, |n_an - n_fd| / n_fd as measured at the parent commit: 160 attempts with either form (profiles/axial_profile.md)
PARENT_JAC_GAP = 0.0


def case_input(name, ivp, with_profile=True, **cfg):
    c = PR.CASES[name]
    kw = {"process_type": c["process-type"]} if "process-type" in c else {}
    mi = INP.ALL_N2_INPUTS[c["input"]](ivp=ivp, period=c.get("period", 0.05), **kw)
    mi["solver-config"].update({"zNo": c["zNo"], "tNo": c.get("tNo", 2), "quiet": True})
    mi["solver-config"].update(STEPPERS[ivp][0])
    mi["solver-config"].update(cfg)
    if with_profile and "axial-profile" in c:
        mi["solver-config"]["axial-profile"] = copy.deepcopy(c["axial-profile"])
    if "schedule" in c:
        mi["solver-config"]["schedule"] = copy.deepcopy(c["schedule"])
    return mi


def profile_error(dp, states, Tf, S=6, iso=False):
    """max |dMoFri|, max |dT|/T over all nodes and output times; states: golden [K][V*N] (scaled variables)."""
    ex = et = 0.0
    assert len(dp) == len(states)
    for k in range(len(dp)):
        Y = np.asarray(states[k]).reshape(S + (0 if iso else 1), -1)
        mofr = Y[:S]/np.sum(Y[:S], axis=0)
        a = np.asarray(dp[k]["dataYs"])
        ex = max(ex, float(np.max(np.abs(a[:S] - mofr))))
        if not iso:
            T = Y[S]*Tf + Tf
            et = max(et, float(np.max(np.abs(a[S] - T)/T)))
    return ex, et


def packed_state(pk):
    return np.concatenate((np.asarray(pk["dataYCons1"]), np.asarray(pk["dataYTemp1"]).reshape(1, -1)), axis=0).flatten()


# ----------------------------------------------------------------------------- right-hand side and RK4 on the device
SHAPES = [(20, 64, 1), (101, 64, 2), (300, 128, 1)]
_REF = {}


def reference(name, N, E=3):
    """(input, mechanism, row, named, oracle constants, tables [E][2][N], per-member profiled oracle RHS): computed once"""
    key = (name, N, E)
    if key not in _REF:
        mi = INP.ALL_N2_INPUTS[name]()
        mech = plan.Mechanism(mi)
        nm, row = plan.member_constants(mi, mech, N)
        pr = O.setup_n2(mi, N)
        tabs = PR.make_tables(N, E)
        if name == "dme_nb" and N == 20:
            a, d = PR.bed(PR.BED_A, N, pr["Tm"])                 # one of them is the bed of the golden cases
            tabs[E - 1, 0], tabs[E - 1, 1] = a, d
        fs = [PR.profiled_rhs(O, pr, tabs[e, 0], tabs[e, 1]) for e in range(E)]
        _REF[key] = (mi, mech, row, nm, pr, tabs, fs)
    return _REF[key]


def states(name, N, pr, mech, E):
    """E well-conditioned states: the reference-generated G2 states where there are some, else smooth variations of the
    oracle's initial state (positive concentrations, a few percent in theta)"""
    g = np.load(os.path.join(GOLD, "g2_rhs.npz"))
    if "%s_%d_y" % (name, N) in g.files:
        return np.array(g["%s_%d_y" % (name, N)][:E], dtype=float)
    z = np.arange(N)/float(N - 1)
    out = []
    for e in range(E):
        Y = np.array(pr["IV"], dtype=float).reshape(mech.V, N).copy()
        for i in range(mech.S):
            Y[i] *= 1.0 + 0.1*np.sin(3.0*z + i + e)
        if not mech.iso:
            Y[mech.S] = 0.02*np.sin(5.0*z + e)
        out.append(Y.flatten())
    return np.array(out)


@pytest.mark.parametrize("name,N,block,npt", [("dme_nb",) + s for s in SHAPES] + [("syn12", 20, 64, 1)])
def test_rhs_against_the_profiled_oracle(name, N, block, npt):
    E = 3
    mi, mech, row, nm, pr, tabs, fs = reference(name, N, E)
    assert np.any(tabs[0, 0] == 0)                               # a zero-activity zone
    dev = N2Device(mech, np.tile(row, (E, 1)), N, block=block, npt=npt, profile=tabs)
    try:
        assert dev.profiled and dev.defines["RMT_PROFILE"] == "1"
        Y = states(name, N, pr, mech, E)
        out = dev.rhs(dev.to_device(Y)).cpu().numpy()
        assert not dev.status().any()
        for e in range(E):
            err = rowwise_err(out[e], fs[e](0.0, Y[e]), mech.V)
            print("rhs %s N=%d %dx%d member %d: %.3e" % (name, N, block, npt, e, err))
            assert err < 1e-12, (e, err)
            other = rowwise_err(out[e], fs[(e + 1) % E](0.0, Y[e]), mech.V)
            assert other > 1e-6, (e, other)                      # (a wrong member stride would pass a shared table)
    finally:
        dev.close()


def _rk4_case(N, block, npt, mode, E=3, steps=10, h=1e-5):
    mi, mech, row, nm, pr, tabs, fs = reference("dme_nb", N, E)
    dev = N2Device(mech, np.tile(row, (E, 1)), N, block=block, npt=npt, profile=tabs)
    try:
        if mode is not None:
            dev.set_mode(mode)
        y = dev.to_device(np.tile(plan.initial_state(nm, mech, N), (E, 1)))
        dev.rk4(y, h, steps)
        got = y.cpu().numpy()
        assert not dev.status().any() and dev.fallbacks() == 0
        assert dev.last_geometry()[0] == 1
        for e in range(E):
            want = O.rk4(0.0, steps*h, steps, pr["IV"], fs[e], keep=False)
            err = rowwise_err(got[e], want, mech.V)
            print("rk4 N=%d %dx%d %s member %d unit %s: %.3e" % (
                N, block, npt, mode or "reg", e, {k: v for k, v in dev.defines.items() if k.startswith("RMT_KCACHE")}, err))
            assert err < 1e-12, (e, err)
        plain = O.rk4(0.0, steps*h, steps, pr["IV"], O.make_rhs_vec(pr), keep=False)
        assert rowwise_err(got[0], plain, mech.V) > 1e-9         # (the profile is felt within ten steps)
    finally:
        dev.close()


@pytest.mark.parametrize("N,block,npt,mode", [(20, 64, 1, None), (101, 64, 2, None), (300, 128, 1, "mem")])
def test_ten_rk4_steps_against_the_profiled_oracle(N, block, npt, mode):
    _rk4_case(N, block, npt, mode)


def test_ten_rk4_steps_on_the_unit_of_the_bench_geometry():
    """whatever unit code_plan selects for a profiled run at 512 x 2 with N = 1024, E = 2"""
    _rk4_case(1024, 512, 2, None, E=2)


# ----------------------------------------------------------------------------- end to end against G18
@pytest.mark.parametrize("ivp", list(STEPPERS))
@pytest.mark.parametrize("name", ["A", "B"])
def test_against_g18(name, ivp):
    c = PR.CASES[name]
    g = PR.golden(name)
    iso = "process-type" in c
    res = rmtExe(case_input(name, ivp))["resModel"]
    dp = res["dataPack"]
    assert len(dp) == c["tNo"]
    for k in range(len(dp)):
        assert abs(dp[k]["dataTime"] - g["times"][k]) < 1e-12
    ex, et = profile_error(dp, g["states"], 523.0, iso=iso)
    print("G18 %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  stats %s" % (
        name, ivp, ex, et, {k: v for k, v in res["device-stats"].items() if k in ("steps", "device-mode", "last-geometry")}))
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)
    # the result entry: the node values the device used
    entry = res["axial-profile"]
    N = c["zNo"]
    a, d = PR.bed(c["axial-profile"], N, 523.0)
    assert np.array_equal(entry["position"], np.arange(N)/float(N - 1))
    assert np.array_equal(entry["catalyst-activity"], a) and np.array_equal(entry["medium-temperature"], 523.0 + d)
    if name == "A" and ivp == "hip-rk45":                        # a run that ignores the key is four orders away
        plain = rmtExe(case_input(name, ivp, with_profile=False))["resModel"]
        px, pt = profile_error(plain["dataPack"], g["states"], 523.0)
        assert "axial-profile" not in plain and max(px, pt) > 1e3*bound
        tx, tt = profile_error(plain["dataPack"], PR.golden("A0")["states"], 523.0)     # (the plain twin is well chosen)
        print("G18 A0 (plain twin) %s: max|dMoFri| = %.3e  max|dT|/T = %.3e" % (ivp, tx, tt))
        assert tx <= bound and tt <= bound


@pytest.mark.parametrize("mode", [None, "mem"])
@pytest.mark.parametrize("ivp", ["hip-rk4", "hip-rk45", "hip-ros4"])
def test_several_node_blocks_against_g18_c(ivp, mode):
    g = PR.golden("C")
    cfg = {} if mode is None else {"device-mode": "mem", "block": 128, "nodes-per-thread": 1}
    res = rmtExe(case_input("C", ivp, **cfg))["resModel"]
    st = res["device-stats"]
    ex, et = profile_error(res["dataPack"], g["states"], 523.0)
    print("G18 C %s %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  mode %s geometry %s" % (
        ivp, mode or "host", ex, et, st["device-mode"], st["last-geometry"]))
    assert st["last-geometry"][0] == 1                            # never a chained form
    want = "mem" if (mode == "mem" or ivp == "hip-ros4") else "reg"
    assert list(st["device-mode"].values()) == [want]
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)


@pytest.mark.parametrize("ivp", ["hip-rk45", "hip-ros4"])
def test_the_identity_profile_is_the_run_without_the_key(ivp):
    mi = case_input("A", ivp, with_profile=False)
    plain = rmtExe(mi)["resModel"]
    assert "axial-profile" not in plain
    mi = case_input("A", ivp, with_profile=False)
    mi["solver-config"]["axial-profile"] = {"position": [0, 1], "catalyst-activity": [1, 1]}
    res = rmtExe(mi)["resModel"]
    assert np.all(res["axial-profile"]["catalyst-activity"] == 1.0) and np.all(res["axial-profile"]["medium-temperature"] == 523.0)
    ex, et = profile_error(res["dataPack"], [packed_state(pk) for pk in plain["dataPack"]], 523.0)
    print("identity profile %s: max|dMoFri| = %.3e  max|dT|/T = %.3e" % (ivp, ex, et))
    assert ex <= 2*STEPPERS[ivp][1] and et <= 2*STEPPERS[ivp][1]


def test_four_members_with_four_activity_patterns():
    ivp = "hip-rk45"
    bound = STEPPERS[ivp][1]
    pats = [None, [1.0, 1.0, 0.4, 0.4, 0.4, 0.4], [0.0, 0.0, 0.0, 0.0, 1.0, 1.0], [0.7]*6]
    members = [{} if p is None else {"solver-config": {"axial-profile": {"catalyst-activity": p}}} for p in pats]
    mi = case_input("A", ivp)
    mi["solver-config"]["ensemble"] = members
    res = rmtExe(mi)["resModel"]
    ens = res["ensemble"]
    assert len(ens) == 4
    ex, et = profile_error(ens[0]["dataPack"], PR.golden("A")["states"], 523.0)       # case A's member
    print("ensemble member 0 against G18 A: %.3e %.3e" % (ex, et))
    assert ex <= bound and et <= bound
    ends = []
    for e, p in enumerate(pats):
        one = case_input("A", ivp)
        if p is not None:
            one["solver-config"]["axial-profile"]["catalyst-activity"] = p
        single = rmtExe(one)["resModel"]
        sx, st = profile_error(ens[e]["dataPack"], [packed_state(pk) for pk in single["dataPack"]], 523.0)
        print("ensemble member %d against its own single run: %.3e %.3e" % (e, sx, st))
        assert sx <= 2*bound and st <= 2*bound
        assert np.array_equal(ens[e]["axial-profile"]["catalyst-activity"], single["axial-profile"]["catalyst-activity"])
        ends.append(np.asarray(ens[e]["dataPack"][-1]["dataYs"]))
    for i in range(4):
        for j in range(i + 1, 4):
            assert np.max(np.abs(ends[i][:6] - ends[j][:6])) > 1e3*bound, (i, j)


# ----------------------------------------------------------------------------- with the other keys
def _steady_input(ivp="hip-ros4", **cfg):
    mi = INP.dme_notebook_input(ivp=ivp, period=0.05)
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "initial": "steady",
                                "axial-profile": copy.deepcopy(PR.BED_A)})
    mi["solver-config"].update(cfg)
    return mi


def test_initial_steady_is_the_steady_state_of_the_profiled_bed():
    gold = PR.golden("S")["state"]
    res = rmtExe(_steady_input())["resModel"]
    ini = res["initial"]
    ex, et = profile_error(res["dataPack"], [gold, gold], 523.0)
    print("G18 S: initial %s (golden residual %.3e); max|dMoFri| = %.3e  max|dT|/T = %.3e"
          % (ini, PR.G18["steady"]["residual"], ex, et))
    assert ini["residual"] <= 10*PR.G18["steady"]["residual"]
    assert len(res["dataPack"]) == 2 and ex <= STATE_BOUND and et <= STATE_BOUND
    g17 = np.load(os.path.join(GOLD, "g17_steady_dme_nb.npz"))["state"]
    fx, ft = profile_error(res["dataPack"], [g17, g17], 523.0)
    assert max(fx, ft) > 1e3*STATE_BOUND                         # not the unprofiled steady state


def test_monitor_with_residual_finds_the_hot_spot_of_the_profiled_bed():
    gold = PR.golden("S")["state"].reshape(7, 20)
    res = rmtExe(_steady_input(monitor={"samples": 1, "residual": True}))["resModel"]
    mon = res["monitor"]
    print("monitor: peak-position %s peak-temperature %s residual %s" % (
        mon["peak-position"], mon["peak-temperature"], mon.get("residual")))
    assert np.all(np.asarray(mon["peak-position"]) == np.linspace(0, 1, 20)[int(np.argmax(gold[6]))])
    assert np.max(np.asarray(mon["residual"])[0]) <= 10*PR.G18["steady"]["residual"]      # (sample 0: the started state)


@pytest.mark.parametrize("ivp", list(STEPPERS))
def test_a_scheduled_coolant_moves_the_common_level_and_the_zones_keep_their_offsets(ivp):
    g = PR.golden("AS")
    res = rmtExe(case_input("AS", ivp))["resModel"]
    ex, et = profile_error(res["dataPack"], g["states"], 523.0)
    print("G18 AS %s: max|dMoFri| = %.3e  max|dT|/T = %.3e  stats %s" % (
        ivp, ex, et, {k: v for k, v in res["device-stats"].items() if k in ("steps", "launches", "device-mode")}))
    bound = STEPPERS[ivp][1]
    assert ex <= bound and et <= bound, (ex, et)
    assert res["schedule"]["medium-temperature"][-1] == 533.0 and res["axial-profile"]["medium-temperature"][0] == 533.0
    ax, at = profile_error(res["dataPack"][1:], PR.golden("A")["states"][1:], 523.0)  # (the step is felt)
    assert max(ax, at) > 10*bound


# ----------------------------------------------------------------------------- the stiff stepper's Jacobian on the device
def _ros4_attempts(profiled, fd):
    """case A (or its plain twin) by N2Device.ros4 over the two output intervals with rmtExe's default tolerances:
    (attempted steps, dataPack-like end states)"""
    c = PR.CASES["A"]
    mi = INP.dme_notebook_input()
    mech = plan.Mechanism(mi)
    N = c["zNo"]
    nm, row = plan.member_constants(mi, mech, N)
    kw = {}
    if profiled:
        a, d = PR.bed(c["axial-profile"], N, 523.0)
        kw["profile"] = np.stack([a, d])[None]
    dev = N2Device(mech, row, N, block=n2.ros4_block(mech.V, N), npt=1, features=("ros4",), specialize=False,
                   defines={"RMT_ROS_JAC_FD": "1"} if fd else {}, **kw)
    try:
        dev.set_mode("mem")
        y = dev.to_device(plan.initial_state(nm, mech, N))
        tried, out = 0, []
        for i, (t0, t1) in enumerate(((0.0, 0.2), (0.2, 0.4))):
            dev.ros4(y, t0, t1, *n2.stepper_args({}, "ros4", i == 0))
            st = dev.rk45_stats()
            assert not dev.status().any() and st["t_end"][0] == t1
            tried += int(st["accepted"][0] + st["rejected"][0])
            out.append(y.cpu().numpy()[0].copy())
        return tried, out
    finally:
        dev.close()


def _state_error(states, gold, Tf=523.0, S=6):
    ex = et = 0.0
    for y, g in zip(states, gold):
        Y, R = np.reshape(y, (S + 1, -1)), np.reshape(g, (S + 1, -1))
        ex = max(ex, float(np.max(np.abs(Y[:S]/np.sum(Y[:S], axis=0) - R[:S]/np.sum(R[:S], axis=0)))))
        et = max(et, float(np.max(np.abs((Y[S] - R[S])*Tf)/(R[S]*Tf + Tf))))
    return ex, et


def test_analytic_and_forward_difference_jacobian_on_the_profiled_bed():
    g = PR.golden("A")["states"]
    n_an, y_an = _ros4_attempts(True, False)
    n_fd, y_fd = _ros4_attempts(True, True)
    p_an, _ = _ros4_attempts(False, False)
    p_fd, _ = _ros4_attempts(False, True)
    gap, twin = abs(n_an - n_fd)/float(n_fd), abs(p_an - p_fd)/float(p_fd)
    print("hip-ros4 attempts on case A: analytic %d, forward differences %d (gap %.4f); plain twin %d / %d (gap %.4f, "
          "recorded at the parent commit: %.4f)" % (n_an, n_fd, gap, p_an, p_fd, twin, PARENT_JAC_GAP))
    for tag, ys in (("analytic", y_an), ("forward differences", y_fd)):
        ex, et = _state_error(ys, g)
        print("  %s: max|dMoFri| = %.3e  max|dT|/T = %.3e" % (tag, ex, et))
        assert ex <= STEPPERS["hip-ros4"][1] and et <= STEPPERS["hip-ros4"][1]
    assert gap <= PARENT_JAC_GAP + 0.05


# ----------------------------------------------------------------------------- the library's guards
def test_a_profiled_device_launches_nothing_before_its_table_is_there():
    mi, mech, row, nm, pr, tabs, fs = reference("dme_nb", 20, 3)
    dev = N2Device(mech, row, 20, block=64, npt=1, specialize=False, defines={"RMT_PROFILE": "1"}, features=("march",))
    try:
        y = dev.to_device(plan.initial_state(nm, mech, 20))
        before = y.clone()
        with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_set_profile"):
            dev.rhs(y)
        with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_set_profile"):
            dev.rk4(y, 1e-5, 2)
        with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_set_profile"):
            dev.rk45(y, 0.0, 1e-4, 1e-6, 1e-9, 1e-6, 100)
        with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_set_profile"):
            dev.steady_march(y)
        assert self_equal(y, before)                             # no kernel ran
        with pytest.raises(hipbind.RmtN2Error, match=r"\[E\]\[2\]\[N\]"):
            dev.set_profile(np.zeros((1, 2, 19)))
        dev.set_profile(tabs[:1])
        out = dev.rhs(y).cpu().numpy()[0]
        assert rowwise_err(out, fs[0](0.0, before.cpu().numpy()[0]), mech.V) < 1e-12
    finally:
        dev.close()


def self_equal(a, b):
    return bool((a == b).all().item())


def test_set_profile_on_an_unprofiled_device_raises():
    mi, mech, row, nm, pr, tabs, fs = reference("dme_nb", 20, 3)
    dev = N2Device(mech, row, 20, block=64, npt=1, specialize=False)
    try:
        assert not dev.profiled
        with pytest.raises(hipbind.RmtN2Error, match="RMT_PROFILE"):
            dev.set_profile(tabs[:1])
        dev.rhs(dev.to_device(plan.initial_state(nm, mech, 20)))  # ... and it goes on working
        assert not dev.status().any()
    finally:
        dev.close()
