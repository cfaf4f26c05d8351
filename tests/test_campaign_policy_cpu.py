"""solver-config "deactivation" "policy" without a GPU: validation, the root-find in numpy (campaign.policy_emulate), the
code-object plan (the policy unit is a unit of its own, the campaign unit and every other unit stay what they are),
cross-compilation, and the policy step compiled for the host (tests/helpers/campaign_policy_emu.cpp: the product's node
solver and update function, the state machine restated) against the goldens G20 (tools/make_golden.py policy: per step
scipy.optimize.brentq on the oracle's profiled right-hand side - tests/policy_ref.py).

Bounds (those of tests/test_gpu_campaign_policy.py):
* states at every output within STATE_BOUND = 1e-8 in the metric of tests/test_campaign_cpu.py;
* the coolant level within STATE_BOUND / |dr/dT|, the slope from the golden's own 9 samples of that step (an error of
  STATE_BOUND in the held mole fraction moves the root by that much) - where the step is not saturated; a saturated step
  sits at its limit exactly;
* the saturated flags equal;
* activity: campaign_ref.activity_bound.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the hipRTC that compiles is the one torch bundles)

import campaign_ref as CR
import inputs as INP
import policy_ref as PO
from helpers.host_build import build_helper
from rmt_app_amd import campaign, hipbind, initial, n2, plan, profile, rmtExe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_BOUND = 1e-8
TOL, MAX_IT = initial.DEFAULTS["tolerance"], initial.DEFAULTS["max-iterations"]
PARENT_TEMPLATE = "7bf57c6113ca3354278d2fa9cbeabd03f1e41442afd6d353284981d0fbb35604"      # tests/test_campaign_cpu.py
LAW = {"rate-constant": 2e-7, "activation-energy": 8.0e4, "reference-temperature": 623.0}
POLICY = {"hold": "outlet-mole-fraction", "component": "DME", "target": 0.0150, "manipulated": "medium-temperature",
          "limits": [503.0, 543.0]}


def profile_error(y, ref, mech, zNo, Tf):
    """(max |d mole fraction|, max |dT|/T) over all nodes of two states [V*zNo] (tests/test_campaign_cpu.py)"""
    Y, R = np.reshape(y, (mech.V, zNo)), np.reshape(ref, (mech.V, zNo))
    x, xr = Y[:mech.S]/np.sum(Y[:mech.S], axis=0), R[:mech.S]/np.sum(R[:mech.S], axis=0)
    T, Tr = Y[mech.S]*Tf + Tf, R[mech.S]*Tf + Tf
    return float(np.max(np.abs(x - xr))), float(np.max(np.abs(T - Tr)/Tr))


# ----------------------------------------------------------------------------- validation
def _input(policy="default", process_type=None, **cfg):
    kw = {"process_type": process_type} if process_type else {}
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.05, **kw)
    mi["model"] = "N2"
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False"})
    mi["solver-config"]["deactivation"] = {"time-on-stream": [5e5, 1e6], "steps": 2, **LAW,
                                           "policy": dict(POLICY) if policy == "default" else policy}
    mi["solver-config"].update(cfg)
    return mi


def _with(**kw):
    return {**POLICY, **kw}


def _without(key):
    return {k: v for k, v in POLICY.items() if k != key}


BAD = [
    ("on", "policy"),
    (_with(gain=1.0), "gain"),                                      # unknown key
    (_with(hold="conversion"), "hold"),
    (_without("hold"), "hold"),
    (_with(manipulated="inlet-temperature"), "manipulated"),
    (_without("manipulated"), "manipulated"),
    (_with(component="N2"), "component"),                           # not in the feed
    (_without("component"), "component"),
    (_without("target"), "target"),
    (_with(target=0.0), "target"),
    (_with(target=1.0), "target"),
    (_with(target="high"), "target"),
    (_without("limits"), "limits"),
    (_with(limits=[543.0, 503.0]), "limits"),
    (_with(limits=[0.0, 503.0]), "limits"),
    (_with(limits=[503.0]), "limits"),
    (_with(limits=[503.0, float("inf")]), "limits"),
    (_with(limits=523.0), "limits"),
    (_with(tolerance=0.0), "tolerance"),
    (_with(tolerance="tight"), "tolerance"),
    (_with(**{"max-evaluations": 3}), "max-evaluations"),
    (_with(**{"max-evaluations": 10.5}), "max-evaluations"),
    (_with(**{"max-evaluations": True}), "max-evaluations"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_policies_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec)
    with pytest.raises(ValueError, match="'deactivation' 'policy'") as e:
        campaign.parse(mi)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="'deactivation' 'policy'") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)
    assert word in str(e.value)
    capsys.readouterr()


def test_policy_needs_a_wall(capsys):
    with pytest.raises(ValueError, match="'deactivation' 'policy'.*iso-thermal"):
        rmtExe(_input(process_type="iso-thermal"))
    mi = _input()
    mi["external-heat"]["MeTe"] = 0
    with pytest.raises(ValueError, match="'deactivation' 'policy'.*MeTe = 0"):
        rmtExe(mi)
    capsys.readouterr()


def test_good_policies_defaults_members_and_what_stays_excluded(capsys):
    c = campaign.parse(_input())
    p = c.policy
    assert (p.component, p.index, p.tolerance, p.max_evaluations) == ("DME", 5, 1e-10, 40)
    assert np.array_equal(p.rows, [[0.0150, 503.0, 543.0, 1e-10]]) and np.array_equal(p.levels, [523.0])
    assert campaign.parse(_input(_with(limits=[530.0, 543.0]))).policy.levels[0] == 530.0     # MeTe clipped to the limits
    assert campaign.parse(_input(_with(limits=[503.0, 510.0]))).policy.levels[0] == 510.0
    assert campaign.parse(_input(_with(limits=[523.0, 523.0]))).policy.rows[0, 1] == 523.0    # lo == hi is allowed
    q = campaign.parse(_input(_with(tolerance=1e-8, **{"max-evaluations": 4}))).policy
    assert (q.tolerance, q.max_evaluations) == (1e-8, 4)
    mi = _input()
    del mi["solver-config"]["deactivation"]["policy"]
    assert campaign.parse(mi).policy is None
    # list-form members: their own target and limits, nothing else
    from rmt_app_amd.ensemble import expand_members
    base = _input()
    members = expand_members(base, [{}, {"solver-config": {"deactivation": {"policy": {"target": 0.0152}}}},
                                    {"solver-config": {"deactivation": {"policy": {"limits": [513.0, 533.0]},
                                                                        "rate-constant": 4e-7}}}])
    e = campaign.parse(base, members)
    assert np.array_equal(e.policy.rows, [[0.0150, 503.0, 543.0, 1e-10], [0.0152, 503.0, 543.0, 1e-10],
                                          [0.0150, 513.0, 533.0, 1e-10]])
    assert e.law[2, 0] == 4e-7 and e.law[0, 0] == 2e-7
    for own, word in (({"tolerance": 1e-8}, "tolerance"), ({"component": "CO"}, "component"), ({"gain": 1.0}, "gain"),
                      ({"max-evaluations": 10}, "max-evaluations"), ({"target": 2.0}, "target"),
                      ({"limits": [5.0, 1.0]}, "limits")):
        with pytest.raises(ValueError, match="'deactivation' 'policy' of member 1") as err:
            campaign.parse(base, expand_members(base, [{}, {"solver-config": {"deactivation": {"policy": own}}}]))
        assert word in str(err.value)
    plain = _input()
    del plain["solver-config"]["deactivation"]["policy"]
    with pytest.raises(ValueError, match="'deactivation' of member 1.*'policy'"):
        campaign.parse(plain, expand_members(plain, [{}, {"solver-config": {"deactivation": {"policy": dict(POLICY)}}}]))
    # the exclusions of "deactivation" stay
    with pytest.raises(ValueError, match="'deactivation'.*'control'"):
        rmtExe(_input(control={"anything": 1}))
    with pytest.raises(NotImplementedError, match="'deactivation'.*fp32"):
        rmtExe(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'deactivation'.*multi-rank"):
        campaign.parse(_input(), multi_rank=True)
    # the log budget covers the four doubles of the policy log: [K+1][E][V+6+4]
    c.check_budget(7, 5*17*8)
    with pytest.raises(ValueError, match="'deactivation'.*'steps'"):
        c.check_budget(7, 5*17*8 - 1)
    capsys.readouterr()


# ----------------------------------------------------------------------------- the root-find in numpy
def test_policy_emulate_on_analytic_functions():
    row = (0.5, 500.0, 540.0, 1e-12)
    # a decreasing and an increasing function: the sign of the slope comes from the bracket
    for fn, root in ((lambda T: -1e-3*(T - 531.25), 531.25), (lambda T: 2e-3*(T - 507.5) + 1e-5*(T - 507.5)**2, 507.5),
                     (lambda T: 1e-2*np.tanh(0.3*(T - 520.0)), 520.0)):
        out = campaign.policy_emulate(row, 520.5, 40, fn)
        assert out["saturated"] == 0 and abs(out["residual"]) <= 1e-12 and abs(out["level"] - root) < 1e-6
        assert out["levels"][:3] == [500.0, 540.0, 520.5] and out["evaluations"] == len(out["levels"]) < 40
        again = campaign.policy_emulate(row, 520.5, 40, [fn(T) for T in out["levels"]])      # a recorded sequence of r
        assert again["levels"] == out["levels"]
        edge = campaign.policy_emulate(row, 500.0, 40, fn)                  # the carried level on a limit: not marched again
        assert edge["levels"][:2] == [500.0, 540.0] and 500.0 < edge["levels"][2] < 540.0 and edge["saturated"] == 0
    # no sign change: the limit with the smaller |r|, a tie goes to lo; the accepted level is the last one marched
    up = campaign.policy_emulate(row, 520.0, 40, lambda T: 1e-3*(T - 490.0))
    assert (up["saturated"], up["levels"], up["evaluations"]) == (-1, [500.0, 540.0, 500.0], 3)
    down = campaign.policy_emulate(row, 520.0, 40, lambda T: -1e-3*(T - 490.0))
    assert (down["saturated"], down["levels"]) == (-1, [500.0, 540.0, 500.0])
    high = campaign.policy_emulate(row, 520.0, 40, lambda T: 1e-3*(T - 560.0))
    assert (high["saturated"], high["levels"], high["level"]) == (1, [500.0, 540.0], 540.0)
    tie = campaign.policy_emulate(row, 520.0, 40, lambda T: 1e-3)
    assert (tie["saturated"], tie["level"]) == (-1, 500.0)
    one = campaign.policy_emulate((0.5, 523.0, 523.0, 1e-12), 523.0, 40, lambda T: 0.25)
    assert (one["saturated"], one["levels"]) == (-1, [523.0])
    # a jump: the bracket collapses; a slow function and a small budget: the evaluation limit
    jump = campaign.policy_emulate(row, 520.0, 200, lambda T: 1e-3 if T < 517.3 else -1e-3)
    assert jump["saturated"] == campaign.BRACKET_COLLAPSED and abs(jump["level"] - 517.3) < 1e-8
    few = campaign.policy_emulate(row, 520.0, 4, lambda T: 1e-2*np.tanh(0.3*(T - 511.0)))
    assert few["saturated"] == campaign.EVALUATION_LIMIT and few["evaluations"] == 4


# ----------------------------------------------------------------------------- the plan
def _rows(name="dme_nb", zNo=20, **kw):
    mi = INP.ALL_N2_INPUTS[name](**kw)
    mech = plan.Mechanism(mi)
    return mi, mech, plan.member_constants(mi, mech, zNo)[1]


def test_the_policy_unit_is_a_unit_of_its_own():
    mi, mech, row = _rows()
    whole = hipbind.kernel_template()
    tpl = plan.without_campaign(whole)
    assert hashlib.sha256(tpl.encode()).hexdigest() == PARENT_TEMPLATE
    assert "policy" not in tpl.lower() and whole.startswith(tpl)
    plain = n2.campaign_plan(mech, 20, row)
    assert "RMT_CAMPAIGN_POLICY" not in plain.defines
    cp = n2.campaign_policy_plan(mech, 20, row)
    assert (cp.block, cp.npt, cp.features) == (plain.block, plain.npt, plain.features) == (64, 1, ("march",))
    assert cp.defines == {**plain.defines, "RMT_CAMPAIGN_POLICY": "1"}
    assert not any(k.startswith("RMT_MC_") for k in cp.defines)          # one object for every operating point and policy
    src, key = n2.plan_unit(mech, False, cp)
    psrc, pkey = n2.plan_unit(mech, False, plain)
    assert "#define RMT_CAMPAIGN_POLICY 1" in src and "void rmt_n2_campaign_policy_step(" in src and key != pkey
    assert "#define RMT_CAMPAIGN_POLICY" not in psrc
    assert src.count("rmt_steady_node(m, up, P, yz, tol, max_iter, flag)") == 3      # march, campaign step, policy step: ONE call each
    assert '#error "RMT_CAMPAIGN_POLICY: only together with RMT_CAMPAIGN' in src
    with pytest.raises(ValueError, match="RMT_CAMPAIGN_POLICY"):          # the define without the campaign unit
        n2.plan_unit(mech, False, n2.CodePlan(cp.block, cp.npt, cp.lds_state,
                                              {k: v for k, v in cp.defines.items() if k != "RMT_CAMPAIGN"}, cp.features))


@pytest.mark.parametrize("name", ["dme_nb", "syn12"])
def test_policy_unit_cross_compiles_for_gfx950(name):
    mi, mech, row = _rows(name)
    code = n2.compile_plan(mech, False, n2.campaign_policy_plan(mech, 20, row), "gfx950")
    assert code[:4] == b"\x7fELF" and b"rmt_n2_campaign_policy_step" in code and b"rmt_n2_campaign_step" in code
    plain = n2.compile_plan(mech, False, n2.campaign_plan(mech, 20, row), "gfx950")
    assert b"rmt_n2_campaign_policy_step" not in plain


def test_c_abi_exports_and_version():
    L = hipbind.lib()
    for name in ("rmt_n2_set_campaign_policy", "rmt_n2_campaign_policy_step", "rmt_n2_get_campaign_level"):
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "rmt_n2.h")) as f:
        header = f.read()
    for name in ("rmt_n2_set_campaign_policy(", "rmt_n2_campaign_policy_step(", "rmt_n2_get_campaign_level(",
                 "RMT_N2_FLAG_POLICY_BRACKET 64u", "RMT_N2_FLAG_POLICY_EVALS 128u"):
        assert name in header, name
    assert L.rmt_n2_abi_version() == hipbind.ABI_VERSION == 2                # additions only


# ----------------------------------------------------------------------------- the policy step on the host
HELPER = os.path.join(ROOT, "tests", "helpers", "campaign_policy_emu.cpp")
_BUILT = {}


@pytest.fixture(scope="module")
def bin_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("campaign_policy_emu"))


def _build(tmp, name, sanitize=False):
    case = PO.case_of(name)
    mi = PO.case_input(name)
    mech = plan.Mechanism(mi)
    zNo = case["zNo"]
    named, row = plan.member_constants(mi, mech, zNo)
    src, _ = n2.plan_unit(mech, False, n2.campaign_policy_plan(mech, zNo, row))
    tag = "%s%s" % (case["input"], "_san" if sanitize else "")
    if tag not in _BUILT:
        _BUILT[tag] = build_helper(HELPER, src, tmp, tag, "policy_%s" % tag, sanitize)
    return _BUILT[tag], mi, mech, named, row


def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _run(exe, mi, mech, row, zNo, max_evals=None, env=None):
    """the host emulation of the run rmtExe(mi) would make: (Campaign, per launch dict(fail, flags, itmax, level, held,
    evaluations, saturated, marches [n][2] = (T, r), act [N], state [V*N]))"""
    cam = campaign.parse(mi)
    pol = cam.policy
    prof = profile.parse(mi)
    table = prof.table()[0] if prof is not None else np.stack([np.ones(zNo), np.zeros(zNo)])
    text = "M %s\nT %d %s\nL %s\nP %s %d %d %s\nC %r %d %d %s\n" % (
        _hex(row), zNo, _hex(table), _hex(cam.law[0]), _hex(pol.rows[0]), pol.index, max_evals or pol.max_evaluations,
        _hex(pol.levels[0]), cam.tolerance, cam.max_iterations, cam.K + 1, _hex(cam.dts()))
    p = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out, lines = [], p.stdout.split("\n")
    fh = float.fromhex
    vec = lambda l: np.array([fh(v) for v in l.split()[1:]])
    for i, ln in enumerate(lines):
        if ln.startswith("step"):
            w, q = ln.split(), lines[i + 1].split()
            out.append({"fail": int(w[2]), "flags": int(w[3]), "itmax": int(w[5]), "level": fh(q[1]), "held": fh(q[2]),
                        "evaluations": int(q[3]), "saturated": int(q[4]), "marches": vec(lines[i + 2]).reshape(-1, 2),
                        "act": vec(lines[i + 3]), "state": vec(lines[i + 4])})
    return cam, out, p


@pytest.mark.parametrize("name", ["PA", "PS"])
def test_host_policy_against_the_golden(name, bin_dir):
    case, gold = PO.case_of(name), PO.golden(name)
    zNo = case["zNo"]
    exe, mi, mech, named, row = _build(bin_dir, name)
    cam, steps, _ = _run(exe, mi, mech, row, zNo)
    assert len(steps) == cam.K + 1 == len(gold["times"]) and all(s["fail"] == 0 and s["flags"] == 0 for s in steps)
    assert np.allclose(cam.times, gold["times"], rtol=1e-15, atol=0) and np.array_equal(cam.output_steps, gold["marks"])
    assert [s["saturated"] for s in steps] == list(gold["saturated"])
    if name == "PS":
        assert np.any(gold["saturated"][:-1] != 0)                     # the limit is reached before the last step
    target, (lo, hi), ptol = case["policy"]["target"], case["policy"]["limits"], cam.policy.tolerance
    bound = CR.activity_bound(case, gold, named["Tf"], mech.V, zNo, STATE_BOUND)
    carried = cam.policy.levels[0]
    for k, s in enumerate(steps):
        # campaign.policy_emulate fed the emulation's r values reproduces its sequence of levels bit for bit
        emu = campaign.policy_emulate(cam.policy.rows[0], carried, cam.policy.max_evaluations, s["marches"][:, 1])
        assert emu["levels"] == list(s["marches"][:, 0]) and emu["saturated"] == s["saturated"]
        assert emu["evaluations"] == s["evaluations"] == len(s["marches"]) and emu["level"] == s["level"]
        assert s["marches"][-1, 0] == s["level"] and s["held"] - target == s["marches"][-1, 1]      # the last march is the accepted one
        carried = s["level"]
        if s["saturated"] == 0:
            assert abs(s["held"] - target) <= ptol and lo < s["level"] < hi
            lb = PO.level_bound(gold, k, STATE_BOUND)
            print("G20 %s step %d (host emulation): level %.6f K, golden %.6f K, |d| = %.3e (bound %.3e), %d marches"
                  % (name, k, s["level"], gold["level"][k], abs(s["level"] - gold["level"][k]), lb, s["evaluations"]))
            assert abs(s["level"] - gold["level"][k]) <= lb
        else:
            assert s["level"] == (lo if s["saturated"] < 0 else hi) == gold["level"][k]
            assert abs(s["held"] - gold["held"][k]) <= STATE_BOUND
        worst_a = float(np.max(np.abs(s["act"] - gold["activity"][k])/gold["activity"][k]))
        assert worst_a <= bound, (k, worst_a, bound)
    for i, k in enumerate(cam.output_steps):
        ex, eT = profile_error(steps[k]["state"], gold["states"][i], mech, zNo, named["Tf"])
        print("G20 %s output %d (host emulation): max|dMoFri| = %.3e max|dT|/T = %.3e (bound %.1e)" % (name, i, ex, eT, STATE_BOUND))
        assert ex <= STATE_BOUND and eT <= STATE_BOUND


def test_host_policy_evaluation_limit(bin_dir):
    exe, mi, mech, named, row = _build(bin_dir, "PA")
    _, steps, _ = _run(exe, mi, mech, row, 20, max_evals=4)
    assert len(steps) == 1 and steps[0]["fail"] == campaign.FLAG_POLICY_EVALS
    assert steps[0]["saturated"] == campaign.EVALUATION_LIMIT and steps[0]["evaluations"] == 4


def test_host_policy_under_address_and_ub_sanitizers(bin_dir):
    """The same stand-alone program built with -fsanitize=address,undefined runs the first interval of PA clean."""
    exe, mi, mech, named, row = _build(bin_dir, "PA", sanitize=True)
    mi["solver-config"]["deactivation"]["time-on-stream"] = mi["solver-config"]["deactivation"]["time-on-stream"][:1]
    cam, steps, p = _run(exe, mi, mech, row, 20, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"})
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    assert len(steps) == cam.K + 1 and all(s["fail"] == 0 for s in steps)
