"""solver-config "axial-profile" without a GPU: validation, the node values, the code-object plan (a unit without the
define is untouched), cross-compilation of the profiled units, and the profiled node function compiled for the host
(tests/helpers/profile_emu.cpp) against the oracle's right-hand side with the profile applied (tests/profile_ref.py), its
analytic node Jacobian against forward differences, and the march against the golden steady state G18-S.

Bounds: the right-hand side within 1e-11 row-relative of the profiled oracle RHS (the bound tests/test_schedule_cpu.py uses
for the same comparison); the Jacobian within 2e-5 of the node's largest entry away from the clamp (mask and bound of
test_host_cpu.py::test_analytic_node_jacobian_vs_forward_differences); the identity against the unprofiled source within
1e-13; the marched state against G18-S within the bounds tests/test_initial_cpu.py uses for G17 (1e-8 on mole fractions
and dT/T, the oracle's max|f| at most 10 x the residual the golden records)."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the hipRTC that compiles is the one torch bundles)

import inputs as INP
from helpers.host_build import build_helper
import profile_ref as PR
from oracle import n2_oracle as O
from oracle.hostemu import HostEmu
from parity import rowwise_err
from rmt_app_amd import hipbind, initial, n2, plan, profile, rmtExe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HELPER = os.path.join(ROOT, "tests", "helpers", "profile_emu.cpp")
EXAMPLE = {"position": [0.0, 0.3, 0.3, 1.0], "catalyst-activity": [0.4, 0.4, 1.0, 1.0],
           "medium-temperature": [533.0, 533.0, 513.0, 513.0]}
STATE_BOUND = 1e-8


def _input(spec=EXAMPLE, model="N2", ivp="hip-rk45", name="dme_nb", **cfg):
    mi = INP.m2_dme_input(ivp="hip-ros4", period=0.05) if model == "M2" else INP.ALL_N2_INPUTS[name](ivp=ivp, period=0.05)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False"})
    if spec is not None:
        mi["solver-config"]["axial-profile"] = copy.deepcopy(spec)
    mi["solver-config"].update(cfg)
    return mi


# ----------------------------------------------------------------------------- validation
def _with(**kw):
    s = copy.deepcopy(EXAMPLE)
    for k, v in kw.items():
        if v is None:
            s.pop(k.replace("_", "-"), None)
        else:
            s[k.replace("_", "-")] = v
    return s


BAD = [
    (_with(position=[0.1, 0.3, 0.3, 1.0]), "position"),                     # does not start at 0
    (_with(position=[0.0, 0.3, 0.3, 0.9]), "position"),                     # does not end at 1
    (_with(position=[0.0, 0.5, 0.3, 1.0]), "position"),                     # decreases
    (_with(position=None), "position"),                                     # missing
    (_with(position=[0.0, float("nan"), 0.3, 1.0]), "position"),
    (_with(position="everywhere"), "position"),
    (_with(catalyst_activity=[0.4, 1.0, 1.0]), "catalyst-activity"),        # length
    (_with(medium_temperature=[533.0, 513.0]), "medium-temperature"),       # length
    (_with(catalyst_activity=[0.4, -0.1, 1.0, 1.0]), "catalyst-activity"),  # negative
    (_with(catalyst_activity=[0.4, float("inf"), 1.0, 1.0]), "catalyst-activity"),
    (_with(medium_temperature=[533.0, float("nan"), 513.0, 513.0]), "medium-temperature"),
    (_with(medium_temperature=[533.0, 0.0, 513.0, 513.0]), "medium-temperature"),     # not positive
    (_with(medium_temperature=[533.0, -5.0, 513.0, 513.0]), "medium-temperature"),
    (_with(catalyst_activity=[[0.4, 0.4], [1.0, 1.0]]), "catalyst-activity"),         # nested
    (_with(catalyst_activity=["a", "b", "c", "d"]), "catalyst-activity"),
    (_with(activity=[1.0, 1.0, 1.0, 1.0]), "activity"),                     # unknown key
    ([0.0, 1.0], "axial-profile"),                                          # not a dict
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec)
    with pytest.raises(ValueError, match="axial-profile") as e:
        profile.parse(mi, None, "hip-rk45")
    assert word in str(e.value)
    with pytest.raises(ValueError, match="axial-profile") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)
    assert word in str(e.value)
    capsys.readouterr()


def _ensemble(members):
    mi = _input()
    mi["solver-config"]["ensemble"] = members
    return mi


def test_a_member_position_that_differs_raises(capsys):
    own = {"solver-config": {"axial-profile": {"position": [0.0, 0.4, 0.4, 1.0]}}}
    mi = _ensemble([{}, own])
    with pytest.raises(ValueError, match="axial-profile.*member 1.*'position'"):
        rmtExe(mi)
    from rmt_app_amd.ensemble import expand_members
    with pytest.raises(ValueError, match="axial-profile.*member 1.*'position'"):
        profile.parse(mi, expand_members(mi, mi["solver-config"]["ensemble"]), "hip-rk45")
    bad = _ensemble([{}, {"solver-config": {"axial-profile": {"catalyst-activity": [1.0, 1.0, -1.0, 1.0]}}}])
    with pytest.raises(ValueError, match="axial-profile.*member 1.*catalyst-activity"):
        rmtExe(bad)
    capsys.readouterr()


def test_every_refusal_of_the_issue(capsys):
    assert profile.parse(_input(None)) is None
    for model in ("M2", "N1", "M7", "M1"):                          # a model other than N2
        with pytest.raises(ValueError, match="'axial-profile'.*only available for model 'N2'"):
            rmtExe(_input(model=model))
    for ivp in ("AM", "hip-ab3"):                                   # the multistep methods
        with pytest.raises(ValueError, match="'axial-profile'.*'ivp'"):
            rmtExe(_input(ivp=ivp))
        with pytest.raises(ValueError, match="'axial-profile'.*'ivp'"):
            profile.parse(_input(ivp=ivp), None, n2.resolve_ivp(ivp))
    with pytest.raises(ValueError, match="'axial-profile'.*'device-mode'"):
        rmtExe(_input(**{"device-mode": "chain"}))
    with pytest.raises(ValueError, match="'device-mode'.*'axial-profile'"):     # ... and any other unknown form
        n2.forced_mode("explicit", 20, 64, 1, "fast", "axial-profile", "profile")
    # the coolant needs a wall: the adiabatic switch and iso-thermal runs (the rule of schedule.parse)
    adiabatic = _input()
    adiabatic["external-heat"]["MeTe"] = 0
    with pytest.raises(ValueError, match="'axial-profile'.*'medium-temperature'.*MeTe"):
        rmtExe(adiabatic)
    iso = INP.dme_notebook_input(ivp="hip-rk45", process_type="iso-thermal", period=0.05)
    iso["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "axial-profile": copy.deepcopy(EXAMPLE)})
    with pytest.raises(ValueError, match="'axial-profile'.*'medium-temperature'.*iso-thermal"):
        rmtExe(iso)
    iso["solver-config"]["axial-profile"].pop("medium-temperature")             # activity alone is allowed there
    p = profile.parse(iso, None, "hip-rk45")
    assert p.given == (True, False) and not np.any(p.delta)
    adiabatic["solver-config"]["axial-profile"].pop("medium-temperature")       # ... and in an adiabatic bed
    assert profile.parse(adiabatic, None, "hip-rk45").given == (True, False)
    # NotImplementedError: fp32, a multi-rank run, the stiff stepper's four-lane layout
    with pytest.raises(NotImplementedError, match="'axial-profile'.*fp32"):
        rmtExe(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'axial-profile'.*multi-rank"):
        profile.parse(_input(), None, "hip-rk45", multi_rank=True)
    wide = _input(_with(medium_temperature=None), name="syn12", ivp="hip-ros4")
    assert n2.ros4_quad(plan.Mechanism(wide))
    for ivp in ("hip-ros4", "default", "hip-auto"):
        wide["solver-config"]["ivp"] = ivp
        with pytest.raises(NotImplementedError, match="'axial-profile'.*stiff stepper"):
            rmtExe(wide)
    assert profile.parse(wide, None, "hip-rk45") is not None                    # the explicit steppers serve it
    capsys.readouterr()


# ----------------------------------------------------------------------------- node values
def test_node_values_linear_pieces_jumps_and_the_last_node():
    # linear pieces: a ramp 0 -> 1 over [0, 0.5], then 1
    v = profile.node_values([0.0, 0.5, 1.0], [0.0, 1.0, 1.0], 11)
    assert np.allclose(v, np.minimum(1.0, 2*np.arange(11)/10.0), rtol=0, atol=1e-15)
    # a jump that falls between two nodes (0.33 on 11 nodes: between node 3 and node 4)
    v = profile.node_values([0.0, 0.33, 0.33, 1.0], [0.4, 0.4, 1.0, 1.0], 11)
    assert list(v) == [0.4]*4 + [1.0]*7
    # a jump that falls ON a node: 3/10 == 0.3 exactly - the node takes the value behind the jump
    assert 3/10.0 == 0.3
    v = profile.node_values([0.0, 0.3, 0.3, 1.0], [0.4, 0.4, 1.0, 1.0], 11)
    assert list(v) == [0.4]*3 + [1.0]*8
    # node N-1 takes the last value, also with a jump at z = 1; node 0 with a jump at z = 0 the value behind it
    v = profile.node_values([0.0, 0.0, 1.0, 1.0], [5.0, 1.0, 2.0, 7.0], 5)
    assert v[0] == 1.0 and v[-1] == 7.0 and np.allclose(v[1:-1], [1.25, 1.5, 1.75])
    assert np.array_equal(profile.node_positions(20), np.arange(20)/19.0)
    # the restated rule of the goldens' generator agrees
    for pos, val, N in (([0.0, 0.3, 0.3, 1.0], [0.4, 0.4, 1.0, 1.0], 20), ([0.0, 0.4, 0.4, 1.0], [533.0, 525.0, 525.0, 513.0], 600)):
        assert np.array_equal(profile.node_values(pos, val, N), PR.nodes(pos, val, N))


def test_identity_defaults_member_overrides_and_delta_against_each_members_own_mete():
    p = profile.parse(_input({"position": [0.0, 1.0]}), None, "hip-rk45")
    assert p.given == (False, False) and np.all(p.activity == 1.0) and not np.any(p.delta)
    assert p.table().shape == (1, 2, 20)
    p = profile.parse(_input(_with(medium_temperature=None)), None, "hip-rk45")          # coolant not given: MeTe
    assert not np.any(p.delta) and p.activity[0, 0] == 0.4 and p.activity[0, -1] == 1.0
    from rmt_app_amd.ensemble import expand_members
    members = [{}, {"external-heat": {"MeTe": 530.0}},
               {"solver-config": {"axial-profile": {"catalyst-activity": [0.0, 0.0, 0.7, 0.7]}}},
               {"external-heat": {"MeTe": 500.0},
                "solver-config": {"axial-profile": {"medium-temperature": [520.0, 520.0, 510.0, 510.0],
                                                    "position": [0.0, 0.3, 0.3, 1.0]}}}]
    mi = _ensemble(members)
    p = profile.parse(mi, expand_members(mi, members), "hip-rk45")
    assert p.E == 4 and p.table().shape == (4, 2, 20) and p.table().flags["C_CONTIGUOUS"]
    a_base, tm_base = PR.nodes(EXAMPLE["position"], EXAMPLE["catalyst-activity"], 20), \
        PR.nodes(EXAMPLE["position"], EXAMPLE["medium-temperature"], 20)
    assert np.array_equal(p.activity[0], a_base) and np.array_equal(p.activity[1], a_base)
    assert np.array_equal(p.delta[0], tm_base - 523.0) and np.array_equal(p.delta[1], tm_base - 530.0)
    assert np.array_equal(p.activity[2], PR.nodes(EXAMPLE["position"], [0.0, 0.0, 0.7, 0.7], 20))
    assert np.array_equal(p.delta[3], PR.nodes(EXAMPLE["position"], [520.0, 520.0, 510.0, 510.0], 20) - 500.0)
    assert np.array_equal(p.table()[3, 1], p.delta[3]) and np.array_equal(p.table()[2, 0], p.activity[2])
    for e in range(4):
        r = profile.result_entry(p, e)
        assert np.array_equal(r["position"], np.arange(20)/19.0) and np.array_equal(r["catalyst-activity"], p.activity[e])
        assert np.array_equal(r["medium-temperature"], p.mete[e] + p.delta[e])
    assert profile.result_entry(p, 3)["medium-temperature"][0] == 520.0


# ----------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def template():
    return hipbind.kernel_template()


def _rows(name, zNo=20):
    mi = INP.ALL_N2_INPUTS[name]()
    mech = plan.Mechanism(mi)
    return mi, mech, plan.member_constants(mi, mech, zNo)[1]


def test_a_unit_without_the_define_is_untouched_and_the_march_carries_it(template):
    mi, mech, row = _rows("dme_nb")
    kw = dict(block=64, npt=1, rows=row, specialize=False)
    plain = n2.code_plans(mech, 20, features=("march",), **kw)
    assert all("RMT_PROFILE" not in cp.defines for cp in plain)
    assert plain[0] == n2.code_plan(mech, 20, **kw) and plain[1] == n2.march_plan(mech, 20, None, row)
    src0, key0 = n2.plan_unit(mech, False, plain[0])
    assert (src0, key0) == (mech.source(template, False, 64, 1, plain[0].lds_state, plain[0].defines),
                            mech.digest(template, False, 64, 1, plain[0].lds_state, plain[0].defines))
    assert "#define RMT_PROFILE" not in src0.split("// generated by")[1].split("typedef")[0]
    prof = n2.code_plans(mech, 20, features=("march",), defines={"RMT_PROFILE": "1"}, **kw)
    assert all(cp.defines["RMT_PROFILE"] == "1" for cp in prof)             # the stepper's unit AND the march unit
    assert (prof[0].block, prof[0].npt, prof[0].lds_state) == (plain[0].block, plain[0].npt, plain[0].lds_state)
    src1, key1 = n2.plan_unit(mech, False, prof[0])
    assert key1 != key0 and src1.count("#define RMT_PROFILE 1\n") == 1
    assert src1.replace("#define RMT_PROFILE 1\n", "", 1) == src0           # the define is the only difference
    msrc, _ = n2.plan_unit(mech, False, prof[1])
    assert "#define RMT_PROFILE 1\n" in msrc and "#define RMT_WITH_MARCH 1\n" in msrc
    assert msrc.replace("#define RMT_PROFILE 1\n", "", 1) == n2.plan_unit(mech, False, plain[1])[0]
    # a forced, profiled run hands both row layout and profile to the march; nothing else travels
    both = n2.march_plan(mech, 20, {"RMT_FORCING": "1", "RMT_PROFILE": "1", "RMT_RK45_LDS": "2"})
    assert both.defines["RMT_FORCING"] == "1" and both.defines["RMT_PROFILE"] == "1" and "RMT_RK45_LDS" not in both.defines
    # a profiled reactor beyond one workgroup never gets a chained unit's cache
    long = n2.code_plan(mech, 600, block=128, npt=1, defines={"RMT_PROFILE": "1"})
    assert "RMT_KCACHE_CHAIN" not in long.defines
    # the template holds everything behind the switch, and the switch defaults to off
    assert "#ifndef RMT_PROFILE\n#define RMT_PROFILE 0\n#endif" in template
    assert template.count("rmt_profile_tab") >= 2 and "#if RMT_PROFILE\n" in template


def test_the_unprofiled_code_object_has_no_profile_symbol():
    mi, mech, row = _rows("dme_nb")
    kw = dict(block=64, npt=1, rows=row, specialize=False)
    code0 = n2.compile_plan(mech, False, n2.code_plan(mech, 20, **kw), "gfx950")
    code1 = n2.compile_plan(mech, False, n2.code_plan(mech, 20, defines={"RMT_PROFILE": "1"}, **kw), "gfx950")
    assert code0[:4] == b"\x7fELF" and b"rmt_profile" not in code0
    assert b"rmt_profile_tab" in code1
    for chained in (b"rmt_n2_rk4_chain", b"rmt_n2_rk45_chain", b"rmt_n2_multistep_mem"):
        assert chained in code0 or chained == b"rmt_n2_rk45_chain"
        assert chained not in code1                                          # a profiled unit has no chained form


@pytest.mark.parametrize("name", ["dme_nb", "ch4", "syn12"])
def test_profiled_units_cross_compile_for_gfx950(name):
    """hipRTC, no GPU: DME (V = 7), ch4 (isothermal) and the 12-species mechanism (explicit steppers and march only)."""
    mi, mech, row = _rows(name)
    d = {"RMT_PROFILE": "1"}
    code = n2.compile_plan(mech, False, n2.code_plan(mech, 20, block=64, npt=1, rows=row, specialize=False, defines=d))
    assert code[:4] == b"\x7fELF" and b"rmt_n2_rk4_reg" in code and b"rmt_profile_tab" in code
    b45, n45, d45 = n2.rk45_geometry(mech.V, 20, chain=False)
    code = n2.compile_plan(mech, False, n2.code_plan(mech, 20, block=b45, npt=n45, rows=row, specialize=False,
                                                     defines={**d45, **d}))
    assert b"rmt_n2_rk45_reg" in code and b"rmt_n2_rk45_mem" in code
    code = n2.compile_plan(mech, False, n2.march_plan(mech, 20, d, row))
    assert b"rmt_n2_steady_march" in code and b"rmt_profile_tab" in code
    if not n2.ros4_quad(mech):
        code = n2.compile_plan(mech, False, n2.code_plan(mech, 20, block=n2.ros4_block(mech.V, 20), npt=1, rows=row,
                                                         specialize=False, defines=d, features=("ros4",)))
        assert b"rmt_n2_ros4_mem" in code and b"rmt_n2_ros4_chain" not in code


# ----------------------------------------------------------------------------- the node function on the host
def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _build(tmp, name, zNo, feature):
    mi, mech, row = _rows(name, zNo)
    d = {"RMT_PROFILE": "1"}
    cp = n2.march_plan(mech, zNo, d, row) if feature == "march" else \
        n2.code_plan(mech, zNo, block=64, npt=1, rows=row, specialize=False, defines=d, features=(feature,))
    src, _ = n2.plan_unit(mech, False, cp)
    tag = "%s_%s" % (name, feature)
    return build_helper(HELPER, src, tmp, tag, "profile_" + tag), mi, mech, row, src


def _run(exe, text):
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.split("\n")


def _vec(lines, word):
    return np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith(word + " ")][0].split()[1:]])


@pytest.fixture(scope="module")
def ros_unit(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("profile_ros")), "dme_nb", 20, "ros4")


def test_host_rhs_against_the_profiled_oracle(ros_unit):
    exe, mi, mech, row, _ = ros_unit
    Ys = np.load(os.path.join(GOLD, "g2_rhs.npz"))["dme_nb_20_y"]
    tab = PR.make_tables(20)[0]                       # a zero-activity zone, a jump, both signs of the coolant offset
    assert np.any(tab[0] == 0) and np.any(tab[1] > 0) and np.any(tab[1] < 0) and len(set(tab[0])) >= 3
    pr = O.setup_n2(mi, 20)
    f = PR.profiled_rhs(O, pr, tab[0], tab[1])
    f_plain = O.make_rhs_vec(pr)
    worst = 0.0
    for Y in Ys:
        out = _run(exe, "M %s\nT 20 %s %s\nF %s\n" % (_hex(row), _hex(tab[0]), _hex(tab[1]), _hex(Y)))
        got = _vec(out, "rhs")
        assert [ln for ln in out if ln.startswith("flags")][0].split()[1] == "0"
        err = rowwise_err(got, f(0.0, Y), mech.V)
        worst = max(worst, err)
        assert err < 1e-11
        assert rowwise_err(got, f_plain(0.0, Y), mech.V) > 1e-3          # (the table is not a bystander)
    print("profiled node function against the profiled oracle RHS: worst row-relative error %.3e" % worst)


def test_host_jacobian_against_forward_differences_under_the_table(ros_unit):
    exe, mi, mech, row, _ = ros_unit
    V, zNo = mech.V, 20
    Ys = np.load(os.path.join(GOLD, "g2_rhs.npz"))["dme_nb_20_y"]
    tab = PR.make_tables(20)[1]
    tab[0, :4] = 0.0                                   # inert packing in front as well
    checked, worst = 0, 0.0
    for Y in Ys:
        out = _run(exe, "M %s\nT 20 %s %s\nJ %s\n" % (_hex(row), _hex(tab[0]), _hex(tab[1]), _hex(Y)))
        jan, jfd = _vec(out, "jan").reshape(zNo, V, V), _vec(out, "jfd").reshape(zNo, V, V)
        ok = np.all(Y.reshape(V, zNo)[:mech.S] > 1e-30, axis=0)
        ok[1:] &= ok[:-1]                       # the upstream node's clamp enters through `up`
        scale = np.max(np.abs(jfd), axis=(1, 2), keepdims=True)
        err = np.max((np.abs(jan - jfd)/scale)[ok])
        worst = max(worst, float(err))
        assert err < 2e-5
        checked += int(ok.sum())
    assert checked >= zNo
    print("analytic against forward-difference node Jacobian under the table: worst %.3e over %d nodes" % (worst, checked))


def test_an_unaware_caller_of_a_profiled_source_gets_the_unprofiled_function(ros_unit, template):
    _, mi, mech, row, src = ros_unit
    Ys = np.load(os.path.join(GOLD, "g2_rhs.npz"))["dme_nb_20_y"]
    assert "#define RMT_PROFILE 1\n" in src
    emu1 = HostEmu(src, tag="profile_identity", openmp=False)             # the unchanged driver: never sets the fields
    emu0 = HostEmu(src.replace("#define RMT_PROFILE 1\n", "", 1), tag="profile_plain", openmp=False)
    rows = np.tile(row, (len(Ys), 1))
    f1, fl1 = emu1.rhs(Ys, rows, 20)
    f0, fl0 = emu0.rhs(Ys, rows, 20)
    assert not fl1.any() and not fl0.any()
    for k in range(len(Ys)):
        assert rowwise_err(f1[k], f0[k], mech.V) < 1e-13
    jan1, _ = emu1.node_jac(Ys[0], row, 20)
    jan0, _ = emu0.node_jac(Ys[0], row, 20)
    assert np.max(np.abs(jan1 - jan0)) <= 1e-13*np.max(np.abs(jan0))


# ----------------------------------------------------------------------------- the march on the host
def test_host_march_with_the_table_against_g18_s(tmp_path):
    case = PR.CASES["S"]
    zNo = case["zNo"]
    exe, mi, mech, row, _ = _build(str(tmp_path), "dme_nb", zNo, "march")
    pr = O.setup_n2(mi, zNo)
    a, d = PR.bed(case["axial-profile"], zNo, pr["Tm"])
    TOL, MAX_IT = initial.DEFAULTS["tolerance"], initial.DEFAULTS["max-iterations"]
    out = _run(exe, "M %s\nT %d %s %s\nR %r %d\n" % (_hex(row), zNo, _hex(a), _hex(d), TOL, MAX_IT))
    y = _vec(out, "state")
    end = [ln for ln in out if ln.startswith("end")][0].split()
    assert int(end[1]) == 0 and int(end[2]) == 0 and int(end[4]) <= MAX_IT
    assert len([ln for ln in out if ln.startswith("node")]) == zNo
    gold = PR.golden("S")
    Y, R = y.reshape(mech.V, zNo), gold["state"].reshape(mech.V, zNo)
    x, xr = Y[:mech.S]/np.sum(Y[:mech.S], axis=0), R[:mech.S]/np.sum(R[:mech.S], axis=0)
    ex = float(np.max(np.abs(x - xr)))
    eT = float(np.max(np.abs((Y[mech.S] - R[mech.S])*pr["Tf"])/(R[mech.S]*pr["Tf"] + pr["Tf"])))
    r = float(np.max(np.abs(PR.profiled_rhs(O, pr, a, d)(0.0, y))))
    print("G18 S: max|dMoFri| = %.3e max|dT|/T = %.3e; profiled oracle max|f| = %.3e, golden %.3e"
          % (ex, eT, r, PR.G18["steady"]["residual"]))
    assert ex <= STATE_BOUND and eT <= STATE_BOUND
    assert r <= 10*PR.G18["steady"]["residual"]
    # ... and it is not the unprofiled steady state (G17): four orders above the bound
    g17 = np.load(os.path.join(GOLD, "g17_steady_dme_nb.npz"))["state"].reshape(mech.V, zNo)
    assert np.max(np.abs(Y[mech.S] - g17[mech.S])) > 1e3*STATE_BOUND
