"""solver-config "deactivation" "policy" on the device: the kernel rmt_n2_campaign_policy_step through rmtExe and through
N2Device, against the goldens G20 (tools/make_golden.py policy; tests/policy_ref.py: per step scipy.optimize.brentq on the
oracle's profiled right-hand side, the saturation rule and the law restated).

Bounds, all from the issue and none from what the device gives:
* states at every output within STATE_BOUND = 1e-8 (max |d mole fraction|, max |dT|/T over all nodes);
* the coolant level of a step that is not saturated within STATE_BOUND / |dr/dT|, the slope from the golden's own samples
  of that step; a saturated step sits on its limit exactly;
* the saturated flags equal; `held` within the policy's tolerance of the target wherever saturated == 0;
* activity: campaign_ref.activity_bound;
* identities (degenerate limits, members against single runs) bit for bit.
Each test prints its figures; profiles/campaign_policy.md records them."""
import copy

import numpy as np
import pytest

import campaign_ref as CR
import inputs as INP
import policy_ref as PO
from rmt_app_amd import campaign, hipbind, n2, plan, rmtExe

pytestmark = pytest.mark.gpu

STATE_BOUND = 1e-8
_RUNS = {}


def run_case(name):
    """rmtExe of a golden case, once"""
    if name not in _RUNS:
        _RUNS[name] = rmtExe(PO.case_input(name))["resModel"]
    return _RUNS[name]


def state_error(pk, ref, S, Tf):
    """(max |dMoFri|, max |dT|/T) of a dataPack entry against a golden state [V*N] (scaled variables)"""
    Y = np.asarray(ref).reshape(S + 1, -1)
    a = np.asarray(pk["dataYs"])
    T = Y[S]*Tf + Tf
    return float(np.max(np.abs(a[:S] - Y[:S]/np.sum(Y[:S], axis=0)))), float(np.max(np.abs(a[S] - T)/T))


def check_policy_entry(res, K):
    """the shape of resModel["deactivation"]["policy"], and that the per-step entries describe the accepted march"""
    d = res["deactivation"]
    p = d["policy"]
    for key in ("medium-temperature", "held", "evaluations", "saturated"):
        assert len(p[key]) == K + 1, key
    lo, hi = p["limits"]
    assert np.all((p["medium-temperature"] >= lo) & (p["medium-temperature"] <= hi)) and np.all(p["evaluations"] >= 1)
    assert set(np.unique(p["saturated"])) <= {-1, 0, 1}
    assert np.all(p["medium-temperature"][p["saturated"] == -1] == lo) and np.all(p["medium-temperature"][p["saturated"] == 1] == hi)
    inside = p["saturated"] == 0
    assert np.all(np.abs(p["held"][inside] - p["target"]) <= p["tolerance"])
    hit = np.nonzero(~inside)[0]
    assert p["end-of-run"] == (d["time-on-stream"][hit[0]] if len(hit) else None)
    c = d["labelList"].index(p["component"])
    assert np.allclose(d["outlet"][:, c], p["held"], rtol=1e-13, atol=0)          # the outlet row is the accepted march's
    return p


# ----------------------------------------------------------------------------- 1. the golden cases through rmtExe
@pytest.mark.parametrize("name", ["PA", "PS", "PB"])
def test_policy_against_the_golden(name):
    case, gold = PO.case_of(name), PO.golden(name)
    res = run_case(name)
    d = res["deactivation"]
    K = len(gold["times"]) - 1
    p = check_policy_entry(res, K)
    S, N = len(d["labelList"]) - 1, case["zNo"]
    Tf = INP.ALL_N2_INPUTS[case["input"]]()["operating-conditions"]["temperature"]
    assert np.allclose(d["time-on-stream"], gold["times"], rtol=1e-15, atol=0) and np.array_equal(d["output-steps"], gold["marks"])
    assert np.array_equal(p["saturated"], gold["saturated"])
    if name == "PS":
        first = int(np.nonzero(gold["saturated"])[0][0])
        assert 0 < first < K and p["end-of-run"] == gold["times"][first]
    else:
        assert p["end-of-run"] is None
    for k in range(K + 1):
        if gold["saturated"][k] == 0:
            lb = PO.level_bound(gold, k, STATE_BOUND)
            print("G20 %s step %d: level %.6f K, golden %.6f K, |d| = %.3e (bound %.3e), held - target %.2e, %d marches"
                  % (name, k, p["medium-temperature"][k], gold["level"][k], abs(p["medium-temperature"][k] - gold["level"][k]),
                     lb, p["held"][k] - p["target"], p["evaluations"][k]))
            assert abs(p["medium-temperature"][k] - gold["level"][k]) <= lb
        else:
            print("G20 %s step %d: saturated %d at %.6f K, held %.10f, golden %.10f, %d marches"
                  % (name, k, p["saturated"][k], p["medium-temperature"][k], p["held"][k], gold["held"][k], p["evaluations"][k]))
            assert p["medium-temperature"][k] == gold["level"][k] and abs(p["held"][k] - gold["held"][k]) <= STATE_BOUND
    ex = et = ea = 0.0
    for i, k in enumerate(gold["marks"]):
        x, t = state_error(res["dataPack"][i], gold["states"][i], S, Tf)
        ex, et = max(ex, x), max(et, t)
        ea = max(ea, float(np.max(np.abs(d["catalyst-activity"][i + 1] - gold["activity"][k])/gold["activity"][k])))
    bound = CR.activity_bound(case, gold, Tf, S + 1, N, STATE_BOUND)
    print("G20 %s: states max|dMoFri| = %.3e max|dT|/T = %.3e (bound %.1e); activity max rel. error %.3e (bound %.3e); "
          "marches per step %s (mean %.2f)" % (name, ex, et, STATE_BOUND, ea, bound, p["evaluations"].tolist(), p["evaluations"].mean()))
    assert ex <= STATE_BOUND and et <= STATE_BOUND
    assert ea <= bound
    assert res["device-stats"]["launches"] == K + 1
    assert ("axial-profile" in res) == ("axial-profile" in case)


# ----------------------------------------------------------------------------- 2. degenerate limits: the plain campaign
def test_degenerate_limits_equal_the_campaign_without_a_policy_bit_for_bit():
    mi = PO.case_input("PA")
    mete = float(mi["external-heat"]["MeTe"])
    mi["solver-config"]["deactivation"]["policy"]["limits"] = [mete, mete]
    plain = copy.deepcopy(mi)
    del plain["solver-config"]["deactivation"]["policy"]
    a, b = rmtExe(mi)["resModel"], rmtExe(plain)["resModel"]
    assert "policy" not in b["deactivation"]
    for key in ("catalyst-activity", "outlet", "iterations", "mean-activity", "min-activity", "peak-temperature", "residual"):
        assert np.array_equal(a["deactivation"][key], b["deactivation"][key]), key
    assert len(a["dataPack"]) == len(b["dataPack"])
    for pa, pb in zip(a["dataPack"], b["dataPack"]):
        assert pa.keys() == pb.keys()
        for key in pa:
            assert np.array_equal(np.asarray(pa[key]), np.asarray(pb[key])), key
    p = check_policy_entry(a, len(a["deactivation"]["time-on-stream"]) - 1)
    assert np.all(p["saturated"] != 0) and np.all(p["evaluations"] == 1) and np.all(p["medium-temperature"] == mete)
    assert p["end-of-run"] == 0.0


# ----------------------------------------------------------------------------- 3. an ensemble over two workgroups
def test_seventy_members_with_their_own_targets():
    """lanes in different phases of the state machine within one wave (some saturated at lo, some at hi, the others with
    root-finds of different lengths), and the dead lanes of the second block"""
    base = PO.case_input("PA")
    base["solver-config"]["deactivation"].update({"time-on-stream": [1e6], "steps": 2})
    targets = np.linspace(0.0138, 0.0177, 70)
    own = [{"solver-config": {"deactivation": {"policy": {"target": float(t)}}}} for t in targets]
    mi = copy.deepcopy(base)
    mi["solver-config"]["ensemble"] = own
    res = rmtExe(mi)["resModel"]
    assert len(res["ensemble"]) == 70 and res["device-stats"]["launches"] == 3
    sat = np.array([m["deactivation"]["policy"]["saturated"] for m in res["ensemble"]])
    evs = np.array([m["deactivation"]["policy"]["evaluations"] for m in res["ensemble"]])
    assert np.any(sat == 1) and np.any(sat == -1) and np.any(np.all(sat == 0, axis=1))
    assert len(np.unique(evs)) >= 3                                        # marches of different lengths in one wave
    for e in (0, 63, 64, 69):                                              # equal single runs of their own rows
        m = res["ensemble"][e]
        p = check_policy_entry(m, 2)
        assert p["target"] == targets[e]
        single = copy.deepcopy(base)
        single["solver-config"]["deactivation"]["policy"]["target"] = float(targets[e])
        one = rmtExe(single)["resModel"]
        for key in ("medium-temperature", "held", "evaluations", "saturated"):
            assert np.array_equal(one["deactivation"]["policy"][key], p[key]), (e, key)
        for key in ("catalyst-activity", "mean-activity", "outlet", "peak-temperature", "iterations", "residual"):
            assert np.array_equal(one["deactivation"][key], m["deactivation"][key]), (e, key)
        for a, b in zip(one["dataPack"], m["dataPack"]):
            assert np.array_equal(a["dataYs"], b["dataYs"]) and a["dataTime"] == b["dataTime"]
    print("70 members: saturated at lo %d, at hi %d, inside %d (step 0); marches per step %d .. %d"
          % (np.sum(sat[:, 0] == -1), np.sum(sat[:, 0] == 1), np.sum(sat[:, 0] == 0), evs.min(), evs.max()))


# ----------------------------------------------------------------------------- 4. identity with the existing features
def test_last_activity_and_level_fed_back_start_at_the_campaign_state():
    """the last logged activity of PA as an "axial-profile" and its last level as MeTe, with "initial": "steady": the
    started dynamic run sits at the campaign's last state"""
    res = run_case("PA")
    d = res["deactivation"]
    last = res["dataPack"][-1]
    mi = INP.ALL_N2_INPUTS["dme_nb"](ivp="hip-ros4", period=0.05)
    mi["external-heat"]["MeTe"] = float(d["policy"]["medium-temperature"][-1])
    mi["solver-config"].update({"zNo": 20, "tNo": 2, "quiet": True, "initial": "steady", "axial-profile": {
        "position": list(d["position"]), "catalyst-activity": list(d["catalyst-activity"][-1])}})
    dyn = rmtExe(mi)["resModel"]
    S = len(d["labelList"]) - 1
    ex = et = 0.0
    for pk in dyn["dataPack"]:
        a, b = np.asarray(pk["dataYs"]), np.asarray(last["dataYs"])
        ex, et = max(ex, float(np.max(np.abs(a[:S] - b[:S])))), max(et, float(np.max(np.abs(a[S] - b[S])/b[S])))
    print("PA fed back: started run against the campaign's last state max|dMoFri| = %.3e max|dT|/T = %.3e" % (ex, et))
    assert ex <= STATE_BOUND and et <= STATE_BOUND


# ----------------------------------------------------------------------------- 5. saturation and the two ways to give up
def test_a_target_out_of_reach_saturates_and_does_not_raise():
    for target in (0.5, 1e-4):
        mi = PO.case_input("PA")
        mi["solver-config"]["deactivation"].update({"time-on-stream": [1e6], "steps": 1})
        mi["solver-config"]["deactivation"]["policy"]["target"] = target
        res = rmtExe(mi)["resModel"]
        p = check_policy_entry(res, 1)
        assert np.all(p["saturated"] != 0) and p["end-of-run"] == 0.0 and np.all(p["evaluations"] <= 3)
        # the limit with the smaller |r|: the other limit's outlet is farther from the target
        other = copy.deepcopy(mi)
        lo, hi = p["limits"]
        far = hi if p["saturated"][0] < 0 else lo
        other["solver-config"]["deactivation"]["policy"]["limits"] = [far, far]
        q = rmtExe(other)["resModel"]["deactivation"]["policy"]
        assert abs(q["held"][0] - target) >= abs(p["held"][0] - target)


def test_the_evaluation_limit_raises_naming_member_step_and_time(capsys):
    mi = PO.case_input("PA")
    mi["solver-config"]["deactivation"]["policy"]["max-evaluations"] = 4
    with pytest.raises(RuntimeError, match="'deactivation' 'policy'.*'max-evaluations' = 4.*member 0 in step 0 .time on stream 0 s"):
        rmtExe(mi)
    capsys.readouterr()


# ----------------------------------------------------------------------------- 6. the C ABI refuses what is not ready
def test_the_new_entry_points_refuse_a_handle_that_is_not_ready():
    mi = INP.ALL_N2_INPUTS["dme_nb"]()
    mech = plan.Mechanism(mi)
    N = 20
    row = plan.member_constants(mi, mech, N)[1]
    table = np.stack([np.ones((1, N)), np.zeros((1, N))], axis=1)
    law = np.array([[2e-7, 8e4, 623.0, 1.0, 0.0]])
    rows, levels = np.array([[0.0150, 503.0, 543.0, 1e-10]]), np.array([523.0])
    import torch

    def buffers(dev):
        y = dev.to_device(np.zeros((1, mech.V*N)))
        return (y, torch.zeros((1, mech.V + campaign.LOG_EXTRA), dtype=torch.float64, device=y.device),
                torch.zeros((1, campaign.POLICY_LOG), dtype=torch.float64, device=y.device))
    # a handle without the unit: the plain campaign unit, with its table and law
    cp = n2.campaign_plan(mech, N, row)
    dev = n2.N2Device(mech, row, N, block=cp.block, npt=cp.npt, defines=cp.defines, specialize=False, features=cp.features,
                      profile=table)
    try:
        dev.set_campaign_law(law)
        y, log, plog = buffers(dev)
        for call, name in ((lambda: dev.set_campaign_policy(rows, 5, levels), "rmt_n2_set_campaign_policy"),
                           (lambda: dev.campaign_policy_step(y, 0.0, log, plog), "rmt_n2_campaign_policy_step"),
                           (dev.get_campaign_level, "rmt_n2_get_campaign_level")):
            with pytest.raises(hipbind.RmtN2Error, match=name + ".*no rmt_n2_campaign_policy_step"):
                call()
    finally:
        dev.close()
    pp = n2.campaign_policy_plan(mech, N, row)
    dev = n2.N2Device(mech, row, N, block=pp.block, npt=pp.npt, defines=pp.defines, specialize=False, features=pp.features)
    try:
        y, log, plog = buffers(dev)
        calls = ((lambda: dev.set_campaign_policy(rows, 5, levels), "rmt_n2_set_campaign_policy"),
                 (lambda: dev.campaign_policy_step(y, 0.0, log, plog), "rmt_n2_campaign_policy_step"),
                 (dev.get_campaign_level, "rmt_n2_get_campaign_level"))
        for call, name in calls:                                           # no table
            with pytest.raises(hipbind.RmtN2Error, match=name + ".*no profile table"):
                call()
        dev.set_profile(table)
        for call, name in calls:                                           # no law
            with pytest.raises(hipbind.RmtN2Error, match=name + ".*no deactivation law"):
                call()
        dev.set_campaign_law(law)
        for call, name in calls[1:]:                                       # no policy
            with pytest.raises(hipbind.RmtN2Error, match=name + ".*no policy has been set"):
                call()
        for bad_rows, comp, lev in ((np.array([[1.5, 503.0, 543.0, 1e-10]]), 5, levels),
                                    (np.array([[0.015, 543.0, 503.0, 1e-10]]), 5, levels),
                                    (np.array([[0.015, 503.0, 543.0, 0.0]]), 5, levels),
                                    (rows, 6, levels), (rows, -1, levels), (rows, 5, np.array([550.0]))):
            with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_set_campaign_policy.*bad arguments"):
                dev.set_campaign_policy(bad_rows, comp, lev)
        dev.set_campaign_policy(rows, 5, levels)
        assert np.array_equal(dev.get_campaign_level(), levels)
        with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_campaign_policy_step.*bad arguments"):
            dev.campaign_policy_step(y, -1.0, log, plog)
        with pytest.raises(hipbind.RmtN2Error, match="rmt_n2_campaign_policy_step.*bad arguments"):
            dev.campaign_policy_step(y, 0.0, log, plog, max_evaluations=3)
        dev.campaign_policy_step(y, 0.0, log, plog)                        # ready: dt = 0 leaves the table as it is
        assert np.array_equal(dev.get_profile(), table) and not np.any(dev.status())
        got = plog.cpu().numpy()[0]
        assert got[campaign.SATURATED] == 0 and abs(got[campaign.HELD] - 0.0150) <= 1e-10
        assert dev.get_campaign_level()[0] == got[campaign.LEVEL] and 503.0 < got[campaign.LEVEL] < 543.0
        assert np.all(np.isfinite(log.cpu().numpy()))
    finally:
        dev.close()
