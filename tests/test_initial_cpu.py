"""solver-config "initial" without a GPU: validation, the code-object plan (the march is a unit of its own, the stepper's
unit is untouched), cross-compilation of the march unit, and the node solver rmt_steady_node compiled for the host
(tests/helpers/steady_march_emu.cpp) against the golden steady states G17 (tools/make_golden.py steady: SciPy on the
oracle's RHS).

Bounds: the states against G17 within 1e-8 (max |d mole fraction|, max |dT|/T - the bound the device steppers meet against
tight goldens, tests/test_gpu_schedule.py); the oracle's max|f| at the marched state at most 10 x the residual the golden's
json records - both sit at the rounding floor conv eps |y|, one decade covers the different operation order."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the hipRTC that compiles is the one torch bundles)

import inputs as INP
from helpers.host_build import build_helper
from oracle import n2_oracle as O
from rmt_app_amd import hipbind, initial, n2, plan, rmtExe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLD, "g17_steady.json")) as _f:
    G17 = json.load(_f)
CASES = sorted(G17["cases"])
STATE_BOUND = 1e-8
TOL, MAX_IT = initial.DEFAULTS["tolerance"], initial.DEFAULTS["max-iterations"]


def _input(model="N2", spec="steady", **cfg):
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.05) if model != "M2" else INP.m2_dme_input(ivp="hip-ros4", period=0.05)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False", "initial": spec})
    mi["solver-config"].update(cfg)
    return mi


# ----------------------------------------------------------------------------- validation
BAD = [
    ("cold", "kind"),
    ({"kind": "warm"}, "kind"),
    ({"tolerance": 1e-8}, "kind"),                               # no kind
    ({"kind": "steady", "tol": 1e-8}, "tol"),                    # unknown key
    ({"kind": "steady", "tolerance": 0.0}, "tolerance"),
    ({"kind": "steady", "tolerance": -1e-10}, "tolerance"),
    ({"kind": "steady", "tolerance": "1e-10"}, "tolerance"),
    ({"kind": "steady", "tolerance": float("nan")}, "tolerance"),
    ({"kind": "steady", "max-iterations": 0}, "max-iterations"),
    ({"kind": "steady", "max-iterations": -3}, "max-iterations"),
    ({"kind": "steady", "max-iterations": 2.5}, "max-iterations"),
    ({"kind": "steady", "max-iterations": True}, "max-iterations"),
    (["steady"], "initial"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec=spec)
    with pytest.raises(ValueError, match="initial") as e:
        initial.parse(mi)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="initial") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)
    assert word in str(e.value)
    capsys.readouterr()


def test_good_specs_defaults_and_what_is_not_available(capsys):
    assert initial.parse(_input(spec=None)) is None
    a = initial.parse(_input())
    assert (a.kind, a.tolerance, a.max_iterations) == ("steady", 1e-10, 400) == ("steady", TOL, MAX_IT)
    b = initial.parse(_input(spec={"kind": "steady", "tolerance": 1e-8, "max-iterations": 50}))
    assert (b.kind, b.tolerance, b.max_iterations) == ("steady", 1e-8, 50)
    assert b.result_entry(1e-12, 17, 2) == {"kind": "steady", "residual": 1e-12, "iterations": 17, "nodes-damped": 2}
    for model in ("M2", "N1", "M7", "M1"):                        # any model but N2: from rmtExe, like "schedule"
        bad = _input(model)
        with pytest.raises(ValueError, match="'initial'.*only available for model 'N2'"):
            rmtExe(bad)
    with pytest.raises(NotImplementedError, match="'initial'.*fp32"):
        initial.parse(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'initial'.*fp32"):
        rmtExe(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'initial'.*multi-rank"):
        initial.parse(_input(), multi_rank=True)
    # a mechanism that needs the stiff stepper's four-lane layout is allowed: the march does not use that layout
    wide = plan.Mechanism(INP.syn12_input())
    assert n2.ros4_quad(wide)
    assert "RMT_ROS_QUAD" not in n2.march_plan(wide, 20).defines
    capsys.readouterr()


# ----------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def template():
    return hipbind.kernel_template()


def _rows(name, zNo=20):
    mi = INP.ALL_N2_INPUTS[name]()
    mech = plan.Mechanism(mi)
    return mi, mech, plan.member_constants(mi, mech, zNo)[1]


def test_the_march_is_a_unit_of_its_own_and_the_stepper_unit_is_untouched(template):
    mi, mech, row = _rows("dme_nb")
    kw = dict(block=n2.ros4_block(mech.V, 20), npt=1, rows=row)
    without = n2.code_plans(mech, 20, features=("ros4",), **kw)
    with_key = n2.code_plans(mech, 20, features=("ros4", "march"), **kw)
    assert len(without) == 1 and len(with_key) == 2
    assert without[0] == n2.code_plan(mech, 20, features=("ros4",), **kw) == with_key[0]
    src0, key0 = n2.plan_unit(mech, False, without[0])
    src1, key1 = n2.plan_unit(mech, False, with_key[0])
    assert (src0, key0) == (src1, key1)                           # the stepper's source and cache key: identical
    assert "#define RMT_WITH_MARCH 1" not in src0 and "RMT_WITH_MARCH" not in without[0].defines
    march = with_key[1]
    assert (march.block, march.npt, march.features) == (64, 1, ("march",)) and march == n2.march_plan(mech, 20, None, row)
    msrc, mkey = n2.plan_unit(mech, False, march)
    assert "#define RMT_WITH_MARCH 1" in msrc and "rmt_n2_steady_march" in msrc and mkey != key0
    assert "rmt_kinetics_jac" in msrc and "#define RMT_WITH_ROS4 1" not in msrc
    assert not any(k.startswith("RMT_MC_") for k in march.defines)       # one object for every operating point
    # the template holds the kernel behind its switch only: a unit without the define has no such kernel to compile
    body = template[template.index("#if RMT_WITH_MARCH\n// ====="):]
    assert "rmt_n2_steady_march" in body and template.count("void rmt_n2_steady_march(") == 1
    # a forced run: the march unit reads the stepper's rows (tail included), nothing else of the run's defines travels
    forced = n2.march_plan(mech, 20, {"RMT_FORCING": "2", "RMT_CHECK_ALL_STAGES": "1", "RMT_RK45_LDS": "2"})
    assert forced.defines["RMT_FORCING"] == "2" and "RMT_CHECK_ALL_STAGES" not in forced.defines \
        and "RMT_RK45_LDS" not in forced.defines


@pytest.mark.parametrize("name", ["dme_nb", "ch4", "syn12"])
def test_march_unit_cross_compiles_for_gfx950(name):
    """hipRTC, no GPU: DME (V = 7), ch4 (isothermal) and the 12-species mechanism."""
    mi, mech, row = _rows(name)
    code = n2.compile_plan(mech, False, n2.march_plan(mech, 20, None, row), "gfx950")
    assert code[:4] == b"\x7fELF" and b"rmt_n2_steady_march" in code


# ----------------------------------------------------------------------------- the node solver on the host
HELPER = os.path.join(ROOT, "tests", "helpers", "steady_march_emu.cpp")


def _build(tmp, name, zNo=20, sanitize=False):
    mi, mech, row = _rows(name, zNo)
    src, _ = n2.plan_unit(mech, False, n2.march_plan(mech, zNo, None, row))
    exe = build_helper(HELPER, src, tmp, name, "march_%s%s" % (name, "_san" if sanitize else ""), sanitize)
    return exe, mi, mech, row


def _hex(v):
    return " ".join(float(x).hex() for x in v)


def _run(exe, text):
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.split("\n")


def _march(exe, row, zNo, tol=TOL, max_it=MAX_IT):
    out = _run(exe, "M %s\nR %d %r %d\n" % (_hex(row), zNo, tol, max_it))
    nodes = [ln.split() for ln in out if ln.startswith("node")]
    state = np.array([float.fromhex(v) for v in [ln for ln in out if ln.startswith("state")][0].split()[1:]])
    end = [ln for ln in out if ln.startswith("end")][0].split()
    return nodes, state, {"fail": int(end[1]), "flags": int(end[2]), "worst": float.fromhex(end[3]),
                          "iterations": int(end[4]), "nodes-damped": int(end[5])}


def profile_error(y, ref, mech, zNo, Tf):
    """(max |d mole fraction|, max |dT|/T) over all nodes of two states [V*zNo]"""
    Y, R = np.reshape(y, (mech.V, zNo)), np.reshape(ref, (mech.V, zNo))
    x, xr = Y[:mech.S]/np.sum(Y[:mech.S], axis=0), R[:mech.S]/np.sum(R[:mech.S], axis=0)
    ex = float(np.max(np.abs(x - xr)))
    if mech.iso:
        return ex, 0.0
    T, Tr = Y[mech.S]*Tf + Tf, R[mech.S]*Tf + Tf
    return ex, float(np.max(np.abs(T - Tr)/Tr))


@pytest.mark.parametrize("name", CASES)
def test_host_march_against_the_golden_steady_state(name, tmp_path):
    case = G17["cases"][name]
    zNo = case["zNo"]
    exe, mi, mech, row = _build(str(tmp_path), name, zNo)
    nodes, y, end = _march(exe, row, zNo)
    assert end["fail"] == 0 and end["flags"] == 0 and len(nodes) == zNo
    assert end["iterations"] <= MAX_IT          # (the worst scaled node residual is printed: it may sit at its noise, above TOL)
    gold = np.load(os.path.join(GOLD, "g17_steady_%s.npz" % name))
    pr = O.setup_n2(mi, zNo)
    ex, eT = profile_error(y, gold["state"], mech, zNo, pr["Tf"])
    r = float(np.max(np.abs(O.make_rhs_vec(pr)(0.0, y))))
    print("G17 %s: max|dMoFri| = %.3e max|dT|/T = %.3e; oracle max|f| = %.3e, golden %.3e; %d steps at most, %d nodes damped, "
          "worst scaled node residual %.3e" % (name, ex, eT, r, case["residual"], end["iterations"], end["nodes-damped"],
                                               end["worst"]))
    assert ex <= STATE_BOUND and eT <= STATE_BOUND
    assert r <= 10*case["residual"]


def test_node_zero_with_products_at_the_clamp(tmp_path):
    """The case plain Newton loses: node 0 of dme_nb fed with the products at the clamp 1e-30 (a feed without them), where
    the node Jacobian's columns of those species vanish.  The pseudo-transient iteration converges, and no iterate is non-finite."""
    exe, mi, mech, row = _build(str(tmp_path), "dme_nb")
    up = np.array(list(row[plan.MEMBER_FIXED:plan.MEMBER_FIXED + mech.S]) + [row[3]])
    products = [mech.compList.index(s) for s in ("H2O", "CH3OH", "DME")]
    up[products] = 1e-30
    out = _run(exe, "M %s\nZ %s %r %d %s\n" % (_hex(row), float(row[2]).hex(), TOL, MAX_IT, _hex(up)))
    node = [ln.split() for ln in out if ln.startswith("node")][0]
    y = np.array([float.fromhex(v) for v in [ln for ln in out if ln.startswith("state")][0].split()[1:]])
    fail, iters, nonfinite, res = int(node[2]), int(node[3]), int(node[5]), float.fromhex(node[6])
    print("node 0 of dme_nb: %d steps, %d rejected, scaled residual %.3e" % (iters, int(node[4]), res))
    assert fail == 0 and nonfinite == 0 and iters <= MAX_IT
    assert np.all(np.isfinite(y)) and np.all(y[:mech.S] > 1e-30)  # the products left the clamp
    # ... and it is the node's steady state by the oracle's node function: the same bound as for the whole bed
    pr = O.setup_n2(mi, 20)
    S = mech.S
    sh = (S, 1, 1)
    fo, _, _ = O.make_local_rhs(pr)(y[:S].reshape(sh), y[S].reshape(1, 1), up[:S].reshape(sh), up[S].reshape(1, 1),
                                    np.full((1, 1), row[2]))
    r = float(np.max(np.abs(fo)))
    print("oracle node function at the converged state: max|f| = %.3e" % r)
    assert r <= 10*G17["cases"]["dme_nb"]["residual"]
    # one step cannot converge: the failure is reported, not papered over
    out = _run(exe, "M %s\nZ %s %r %d %s\n" % (_hex(row), float(row[2]).hex(), TOL, 1, _hex(up)))
    assert int([ln.split() for ln in out if ln.startswith("node")][0][2]) & 16            # RMT_FLAG_STEP


def test_host_march_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined marches the DME case clean."""
    exe, mi, mech, row = _build(str(tmp_path), "dme_nb", sanitize=True)
    p = subprocess.run([exe], input="M %s\nR 20 %r %d\n" % (_hex(row), TOL, MAX_IT), capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"})
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    end = [ln for ln in p.stdout.split("\n") if ln.startswith("end")][0].split()
    assert int(end[1]) == 0
