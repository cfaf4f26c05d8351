"""solver-config "deactivation" without a GPU: validation, the law in numpy (campaign.emulate), the code-object plan (the
campaign is a unit of its own, every other unit's source and cache key are untouched), cross-compilation, and the campaign
loop compiled for the host (tests/helpers/campaign_emu.cpp: the product's node solver and update function) against the
goldens G19 (tools/make_golden.py campaign: SciPy on the oracle's RHS, the law restated in numpy - tests/campaign_ref.py).

Bounds (those of tests/test_gpu_campaign.py):
* states at every output within STATE_BOUND = 1e-8 in the metric of tests/test_initial_cpu.py (max |d mole fraction|,
  max |dT|/T) - the bound of the march against G17;
* activity: relative error at most 2 x STATE_BOUND x Ed/(R T_min) x ln(a_0/a_min), from the golden: the first-order
  propagation of a temperature error through the law, doubled for the feedback;
* DI (iso-thermal): the closed form a_0 exp(-k_d t) to 1e-12 relative (a few ulp per exp, 20 steps);
* order on DA: the error of the last activity against the 32-step run of the same scheme halves from 1 to 2 and from 2 to
  4 steps per interval: ratio 2 +- 0.3 (the issue's CPU reference gives 2.05 and 2.13).
"""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the hipRTC that compiles is the one torch bundles)

import campaign_ref as CR
from helpers.host_build import build_helper
import inputs as INP
from oracle import n2_oracle as O
from rmt_app_amd import campaign, hipbind, initial, n2, plan, profile, rmtExe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = CR.meta()
STATE_BOUND = 1e-8
TOL, MAX_IT = initial.DEFAULTS["tolerance"], initial.DEFAULTS["max-iterations"]
LAW = {"rate-constant": 2e-6, "activation-energy": 8.0e4, "reference-temperature": 623.0, "order": 1.0,
       "residual-activity": 0.0}


case_input, activity_bound = CR.case_input, CR.activity_bound


def profile_error(y, ref, mech, zNo, Tf):
    """(max |d mole fraction|, max |dT|/T) over all nodes of two states [V*zNo] (tests/test_initial_cpu.py)"""
    Y, R = np.reshape(y, (mech.V, zNo)), np.reshape(ref, (mech.V, zNo))
    x, xr = Y[:mech.S]/np.sum(Y[:mech.S], axis=0), R[:mech.S]/np.sum(R[:mech.S], axis=0)
    ex = float(np.max(np.abs(x - xr)))
    if mech.iso:
        return ex, 0.0
    T, Tr = Y[mech.S]*Tf + Tf, R[mech.S]*Tf + Tf
    return ex, float(np.max(np.abs(T - Tr)/Tr))


# ----------------------------------------------------------------------------- validation
def _input(spec="default", model="N2", **cfg):
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.05) if model != "M2" else INP.m2_dme_input(ivp="hip-ros4", period=0.05)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False"})
    mi["solver-config"]["deactivation"] = {"time-on-stream": [5e5, 1e6], "steps": 2, **LAW} if spec == "default" else spec
    mi["solver-config"].update(cfg)
    return mi


def _with(**kw):
    return {"time-on-stream": [5e5, 1e6], "steps": 2, **LAW, **kw}


def _without(key):
    return {k: v for k, v in _with().items() if k != key}


BAD = [
    ("on", "deactivation"),
    ([1e5], "deactivation"),
    (_with(rate=1.0), "rate"),                                     # unknown key
    (_without("time-on-stream"), "time-on-stream"),
    (_without("rate-constant"), "rate-constant"),
    (_without("reference-temperature"), "reference-temperature"),  # Ed > 0 needs it
    (_with(**{"time-on-stream": []}), "time-on-stream"),
    (_with(**{"time-on-stream": [1e5, 1e5]}), "time-on-stream"),
    (_with(**{"time-on-stream": [2e5, 1e5]}), "time-on-stream"),
    (_with(**{"time-on-stream": [-1.0, 1e5]}), "time-on-stream"),
    (_with(**{"time-on-stream": [0.0, float("inf")]}), "time-on-stream"),
    (_with(**{"time-on-stream": "soon"}), "time-on-stream"),
    (_with(steps=0), "steps"),
    (_with(steps=2.5), "steps"),
    (_with(steps=True), "steps"),
    (_with(**{"rate-constant": 0.0}), "rate-constant"),
    (_with(**{"rate-constant": "fast"}), "rate-constant"),
    (_with(**{"activation-energy": -1.0}), "activation-energy"),
    (_with(**{"reference-temperature": 0.0}), "reference-temperature"),
    (_with(order=0.5), "order"),
    (_with(order=float("nan")), "order"),
    (_with(**{"residual-activity": 1.0}), "residual-activity"),
    (_with(**{"residual-activity": -0.1}), "residual-activity"),
    (_with(tolerance=0.0), "tolerance"),
    (_with(**{"max-iterations": 0}), "max-iterations"),
    (_with(**{"max-iterations": 2.5}), "max-iterations"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec)
    with pytest.raises(ValueError, match="deactivation") as e:
        campaign.parse(mi)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="deactivation") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)
    assert word in str(e.value)
    capsys.readouterr()


@pytest.mark.parametrize("other,value", [("schedule", {"time": [0.0, 0.05], "temperature": [523.0, 533.0]}),
                                         ("control", {"anything": 1}), ("monitor", {"samples": 2}), ("initial", "steady")])
def test_keys_of_a_transient_raise_together_with_it(other, value, capsys):
    mi = _input(**{other: value})
    with pytest.raises(ValueError, match="'deactivation'.*%r" % other):
        campaign.parse(mi)
    with pytest.raises(ValueError, match="'deactivation'.*%r" % other):
        rmtExe(mi)
    capsys.readouterr()


def test_good_specs_defaults_members_and_what_is_not_available(capsys, monkeypatch):
    mi = _input()
    del mi["solver-config"]["deactivation"]
    assert campaign.parse(mi) is None
    c = campaign.parse(_input())
    assert (c.steps, c.K, c.E, c.tolerance, c.max_iterations) == (2, 4, 1, TOL, MAX_IT)
    assert np.array_equal(c.times, [0.0, 2.5e5, 5e5, 7.5e5, 1e6]) and list(c.output_steps) == [2, 4]
    assert np.array_equal(c.dts(), [2.5e5, 2.5e5, 2.5e5, 2.5e5, 0.0])
    assert np.array_equal(c.law, [[2e-6, 8e4, 623.0, 1.0, 0.0]])
    z = campaign.parse(_input(_with(**{"time-on-stream": [0.0, 1e5]})))       # the first output is the fresh bed
    assert np.array_equal(z.times, [0.0, 5e4, 1e5]) and list(z.output_steps) == [0, 2]
    d = campaign.parse(_input({"time-on-stream": [1e5], "rate-constant": 1e-6}))
    assert np.array_equal(d.law, [[1e-6, 0.0, 298.15, 1.0, 0.0]]) and d.steps == 1 and d.K == 1
    # list-form members: their own law constants, nothing else
    from rmt_app_amd.ensemble import expand_members
    base = _input()
    members = expand_members(base, [{}, {"solver-config": {"deactivation": {"activation-energy": 1.0e5}}},
                                    {"solver-config": {"deactivation": {"rate-constant": 4e-6, "order": 2.0}}}])
    e = campaign.parse(base, members)
    assert np.array_equal(e.law, [[2e-6, 8e4, 623.0, 1.0, 0.0], [2e-6, 1e5, 623.0, 1.0, 0.0], [4e-6, 8e4, 623.0, 2.0, 0.0]])
    for own, word in (({"steps": 3}, "steps"), ({"time-on-stream": [1.0]}, "time-on-stream"), ({"order": 0.0}, "order"),
                      ({"rate": 1.0}, "rate"), ({"tolerance": 1e-8}, "tolerance")):
        with pytest.raises(ValueError, match="'deactivation' of member 1") as err:
            campaign.parse(base, expand_members(base, [{}, {"solver-config": {"deactivation": own}}]))
        assert word in str(err.value)
    # the dict form: one law for the sweep
    sweep = expand_members(base, {"temperature": [520.0, 530.0], "pressure": [4e6, 5e6]})
    assert campaign.parse(base, sweep).law.shape == (4, 5)
    for model in ("M2", "N1", "M7", "M1"):
        with pytest.raises(ValueError, match="'deactivation'.*only available for model 'N2'"):
            rmtExe(_input(model=model))
    with pytest.raises(NotImplementedError, match="'deactivation'.*fp32"):
        campaign.parse(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'deactivation'.*fp32"):
        rmtExe(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'deactivation'.*multi-rank"):
        campaign.parse(_input(), multi_rank=True)
    campaign.parse(_input()).check_budget(7, 5*13*8)                          # the log [K+1][E][V+6] doubles: it fits
    with pytest.raises(ValueError, match="'deactivation'.*'steps'"):
        campaign.parse(_input()).check_budget(7, 5*13*8 - 1)
    monkeypatch.setattr(n2, "PIPELINE_BYTES", 64)                             # ... and through rmtExe, before any device work
    with pytest.raises(ValueError, match="'deactivation'.*'steps'"):
        rmtExe(_input())
    monkeypatch.undo()
    with pytest.raises(ValueError, match="'deactivation'.*'ensemble-output'"):
        rmtExe(_input(**{"ensemble": [{}, {}], "ensemble-output": "outlet"}))
    capsys.readouterr()


def test_rmtexe_refuses_model_m2():
    with pytest.raises(ValueError, match="deactivation"):
        rmtExe(_input(model="M2"))


# ----------------------------------------------------------------------------- the law in numpy
@pytest.mark.parametrize("law", [(2e-6, 8e4, 623.0, 1.0, 0.0), (6e-7, 1.2e5, 623.0, 2.0, 0.2), (1e-6, 0.0, 300.0, 1.5, 0.1)])
def test_emulate_properties(law):
    rng = np.random.default_rng(19)
    a = rng.uniform(0.0, 1.0, 200)
    T = rng.uniform(500.0, 650.0, 200)
    assert np.array_equal(campaign.emulate(a, T, 0.0, law), a)                       # dt = 0: the identity, bit for bit
    one = campaign.emulate(a, T, 4e5, law)
    two = campaign.emulate(campaign.emulate(a, T, 2e5, law), T, 2e5, law)
    assert np.allclose(one, two, rtol=1e-13, atol=0)                                 # exact at constant T
    assert np.all(one <= a) and np.all(one >= np.minimum(a, law[4]))                 # monotone, bounded
    still = a <= law[4]
    assert np.array_equal(one[still], a[still])                                      # a <= a_inf does not move
    assert np.allclose(one, CR.law_update(a, T, 4e5, dict(zip(CR.LAW_KEYS, law))), rtol=1e-13, atol=0)
    near = campaign.emulate(a, T, 4e5, law[:3] + (1.0 + 1e-7,) + law[4:])            # the limit m -> 1 (the difference is O(m - 1))
    assert np.allclose(near, campaign.emulate(a, T, 4e5, law[:3] + (1.0,) + law[4:]), rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------- the plan
# cache keys of the parent commit (dme_nb, 20 nodes): the stiff stepper's unit, the default RK4 unit, the march units
PARENT_KEYS = {"ros4": "94d65147b0eb862e80d4e91a", "rk4": "79c32098d0189e767da77668", "march": "1c6a5dbc92d453021167b860",
               "march_profiled": "301b8120f476d341378c4eda"}
PARENT_TEMPLATE = "7bf57c6113ca3354278d2fa9cbeabd03f1e41442afd6d353284981d0fbb35604"


def _rows(name="dme_nb", zNo=20, **kw):
    mi = INP.ALL_N2_INPUTS[name](**kw)
    mech = plan.Mechanism(mi)
    return mi, mech, plan.member_constants(mi, mech, zNo)[1]


def test_the_campaign_is_a_unit_of_its_own_and_every_other_unit_is_untouched():
    import hashlib
    mi, mech, row = _rows()
    whole = hipbind.kernel_template()
    tpl = plan.without_campaign(whole)
    assert hashlib.sha256(tpl.encode()).hexdigest() == PARENT_TEMPLATE
    assert "campaign" not in tpl.lower() and "rmt_n2_campaign_step" in whole and whole.startswith(tpl)
    units = {"ros4": n2.code_plan(mech, 20, block=n2.ros4_block(mech.V, 20), npt=1, rows=row, features=("ros4",)),
             "rk4": n2.code_plan(mech, 20, rows=row), "march": n2.march_plan(mech, 20, None, row),
             "march_profiled": n2.march_plan(mech, 20, {"RMT_PROFILE": "1"}, row)}
    for name, cp in units.items():
        src, key = n2.plan_unit(mech, False, cp)
        assert key == PARENT_KEYS[name], name
        assert "campaign" not in src.lower() and "RMT_CAMPAIGN" not in cp.defines
    cp = n2.campaign_plan(mech, 20, row)
    assert (cp.block, cp.npt, cp.features) == (64, 1, ("march",))
    assert cp.defines["RMT_CAMPAIGN"] == "1" and cp.defines["RMT_PROFILE"] == "1" and cp.defines["RMT_WITH_MARCH"] == "1"
    assert not any(k.startswith("RMT_MC_") for k in cp.defines)          # one object for every operating point and law
    src, key = n2.plan_unit(mech, False, cp)
    assert "#define RMT_CAMPAIGN 1" in src and "void rmt_n2_campaign_step(" in src and key not in PARENT_KEYS.values()
    # the unit without its march or without the profile does not compile: the template says so
    assert '#error "RMT_CAMPAIGN: needs RMT_WITH_MARCH and RMT_PROFILE' in src


@pytest.mark.parametrize("name,kw", [("dme_nb", {}), ("dme_nb", {"process_type": "iso-thermal"}), ("syn12", {})])
def test_campaign_unit_cross_compiles_for_gfx950(name, kw):
    mi, mech, row = _rows(name, **kw)
    code = n2.compile_plan(mech, False, n2.campaign_plan(mech, 20, row), "gfx950")
    assert code[:4] == b"\x7fELF" and b"rmt_n2_campaign_step" in code and b"rmt_n2_steady_march" in code


# ----------------------------------------------------------------------------- the campaign loop on the host
HELPER = os.path.join(ROOT, "tests", "helpers", "campaign_emu.cpp")
_BUILT = {}


def _build(tmp, name, sanitize=False):
    case = CR.CASES[name]
    mi = case_input(name)
    mech = plan.Mechanism(mi)
    zNo = case["zNo"]
    named, row = plan.member_constants(mi, mech, zNo)
    src, _ = n2.plan_unit(mech, False, n2.campaign_plan(mech, zNo, row))
    tag = "%s%s%s" % (case["input"], "_iso" if mech.iso else "", "_san" if sanitize else "")
    if tag not in _BUILT:
        _BUILT[tag] = build_helper(HELPER, src, tmp, tag, "campaign_%s" % tag, sanitize)
    return _BUILT[tag], mi, mech, named, row


@pytest.fixture(scope="module")
def bin_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("campaign_emu"))


def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _campaign(exe, mi, mech, row, zNo, steps=None, tol=TOL, max_it=MAX_IT, env=None):
    """the host emulation of the run rmtExe(mi) would make: (Campaign, per launch dict(fail, flags, worst, itmax, peak,
    peak-node, mean, min, iters [N], act [N], state [V*N]))"""
    if steps is not None:
        mi["solver-config"]["deactivation"]["steps"] = steps
    cam = campaign.parse(mi)
    prof = profile.parse(mi)
    table = prof.table()[0] if prof is not None else np.stack([np.ones(zNo), np.zeros(zNo)])
    text = "M %s\nT %d %s\nL %s\nC %r %d %d %s\n" % (_hex(row), zNo, _hex(table), _hex(cam.law[0]), tol, max_it, cam.K + 1,
                                                    _hex(cam.dts()))
    p = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out, lines = [], p.stdout.split("\n")
    for i, ln in enumerate(lines):
        if ln.startswith("step"):
            w = ln.split()
            fh = float.fromhex
            vec = lambda l: np.array([fh(v) for v in l.split()[1:]])
            out.append({"fail": int(w[2]), "flags": int(w[3]), "worst": fh(w[4]), "itmax": int(w[5]), "peak": fh(w[6]),
                        "peak-node": int(w[7]), "mean": fh(w[8]), "min": fh(w[9]),
                        "iters": np.array([int(v) for v in lines[i + 1].split()[1:]]), "act": vec(lines[i + 2]),
                        "state": vec(lines[i + 3])})
    return cam, out, p


@pytest.mark.parametrize("name", ["DA", "DB", "DC"])
def test_host_campaign_against_the_golden(name, bin_dir):
    case, gold = CR.CASES[name], CR.golden(name)
    zNo = case["zNo"]
    exe, mi, mech, named, row = _build(bin_dir, name)
    cam, steps, _ = _campaign(exe, mi, mech, row, zNo)
    assert len(steps) == cam.K + 1 == len(gold["times"]) and all(s["fail"] == 0 and s["flags"] == 0 for s in steps)
    assert np.allclose(cam.times, gold["times"], rtol=1e-15, atol=0) and np.array_equal(cam.output_steps, gold["marks"])
    bound = activity_bound(case, gold, named["Tf"], mech.V, zNo, STATE_BOUND)
    worst_a, worst_x, worst_T = 0.0, 0.0, 0.0
    for k, s in enumerate(steps):
        assert np.all(s["act"] <= (steps[k - 1]["act"] if k else np.inf))           # non-increasing in time
        assert np.all(s["act"] >= min(case["law"]["residual-activity"], steps[0]["act"].min()))
        assert s["mean"] == pytest.approx(s["act"].mean(), rel=1e-14) and s["min"] == s["act"].min()
        worst_a = max(worst_a, float(np.max(np.abs(s["act"] - gold["activity"][k])/gold["activity"][k])))
    for i, k in enumerate(cam.output_steps):
        ex, eT = profile_error(steps[k]["state"], gold["states"][i], mech, zNo, named["Tf"])
        worst_x, worst_T = max(worst_x, ex), max(worst_T, eT)
        T = np.reshape(steps[k]["state"], (mech.V, zNo))[-1]
        assert steps[k]["peak-node"] == int(np.argmax(T)) and steps[k]["peak"] == T.max()
    print("G19 %s (host emulation): states max|dMoFri| = %.3e max|dT|/T = %.3e (bound %.1e); activity max rel. error %.3e "
          "(bound %.3e); %d pseudo-time steps per node at most, peak node %d -> %d, activity ends at %.4f .. %.4f"
          % (name, worst_x, worst_T, STATE_BOUND, worst_a, bound, max(s["itmax"] for s in steps), steps[0]["peak-node"],
             steps[-1]["peak-node"], steps[-1]["act"].min(), steps[-1]["act"].max()))
    assert worst_x <= STATE_BOUND and worst_T <= STATE_BOUND
    assert worst_a <= bound


def test_host_campaign_isothermal_closed_form(bin_dir):
    """DI: at the member's inlet temperature every node follows a_0 exp(-k_d t); 1 step per interval equals 5."""
    case, gold = CR.CASES["DI"], CR.golden("DI")
    zNo = case["zNo"]
    exe, mi, mech, named, row = _build(bin_dir, "DI")
    assert mech.iso
    law = case["law"]
    kd = law["rate-constant"]*np.exp(-(law["activation-energy"]/CR.R_GAS)*(1.0/named["Tf"] - 1.0/law["reference-temperature"]))
    ends = {}
    for n in (5, 1):
        cam, steps, _ = _campaign(exe, mi, mech, row, zNo, steps=n)
        assert all(s["fail"] == 0 for s in steps)
        worst = max(float(np.max(np.abs(s["act"]/(steps[0]["act"]*np.exp(-kd*t)) - 1.0))) for s, t in zip(steps, cam.times))
        print("DI (host emulation), %d steps per interval: activity against the closed form %.3e relative" % (n, worst))
        assert worst <= 1e-12
        ends[n] = steps[-1]
    assert np.max(np.abs(ends[1]["act"]/ends[5]["act"] - 1.0)) <= 1e-12
    assert np.max(np.abs(ends[5]["act"]/gold["activity"][-1] - 1.0)) <= 1e-12
    ex, _ = profile_error(ends[5]["state"], gold["states"][-1], mech, zNo, named["Tf"])
    print("DI (host emulation): last state against the golden max|dMoFri| = %.3e" % ex)
    assert ex <= STATE_BOUND


def test_host_campaign_order_of_the_scheme(bin_dir):
    """DA: the error of the last activity against the 32-step run of the same scheme halves with the step."""
    exe, mi, mech, named, row = _build(bin_dir, "DA")
    last = {}
    for n in (1, 2, 4, 32):
        _, steps, _ = _campaign(exe, mi, mech, row, 20, steps=n)
        last[n] = steps[-1]["act"]
    err = {n: float(np.max(np.abs(last[n] - last[32]))) for n in (1, 2, 4)}
    r12, r24 = err[1]/err[2], err[2]/err[4]
    print("DA order (host emulation): errors %.3e %.3e %.3e, ratios %.3f %.3f" % (err[1], err[2], err[4], r12, r24))
    assert abs(r12 - 2.0) <= 0.3 and abs(r24 - 2.0) <= 0.3


def test_host_campaign_failure_stops_and_keeps_the_activity_downstream(bin_dir):
    exe, mi, mech, named, row = _build(bin_dir, "DA")
    _, steps, _ = _campaign(exe, mi, mech, row, 20, max_it=2)
    assert len(steps) == 1 and steps[0]["fail"] & 16 and steps[0]["iters"][0] == 2 and np.all(steps[0]["iters"][1:] == 0)


def test_update_function_on_the_host(bin_dir):
    """rmt_campaign_update itself: dt = 0 is the identity bit for bit, a <= a_inf does not move, and it is campaign.emulate"""
    exe, *_ = _build(bin_dir, "DA")
    rng = np.random.default_rng(72)
    for law in ((2e-6, 8e4, 623.0, 1.0, 0.0), (6e-7, 1.2e5, 623.0, 2.0, 0.2), (1e-6, 5e4, 600.0, 1.5, 0.1)):
        a, T = rng.uniform(0.0, 1.0, 40), rng.uniform(500.0, 650.0, 40)
        text = "L %s\n" % _hex(law) + "".join("U %s %s %s\n" % (float(x).hex(), float(t).hex(), float(dt).hex())
                                              for dt in (0.0, 3e5) for x, t in zip(a, T))
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0
        got = np.array([float.fromhex(ln.split()[1]) for ln in p.stdout.split("\n") if ln.startswith("upd")]).reshape(2, 40)
        assert np.array_equal(got[0], a)
        assert np.allclose(got[1], campaign.emulate(a, T, 3e5, law), rtol=1e-13, atol=0)
        assert np.array_equal(got[1][a <= law[4]], a[a <= law[4]])


def test_host_campaign_under_address_and_ub_sanitizers(bin_dir):
    """The same stand-alone program built with -fsanitize=address,undefined runs the first interval of DB clean."""
    exe, mi, mech, named, row = _build(bin_dir, "DB", sanitize=True)
    mi["solver-config"]["deactivation"]["time-on-stream"] = [5e5]
    cam, steps, p = _campaign(exe, mi, mech, row, 20, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"})
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    assert len(steps) == cam.K + 1 and all(s["fail"] == 0 for s in steps)
