"""solver-config "sensitivity" without a GPU: validation, the code-object plan (the sweep is a unit of its own, every other
unit is untouched), cross-compilation of the unit, and its per-node code compiled for the host
(tests/helpers/sens_emu.cpp) against central differences of the node function itself and against the goldens G21
(tools/make_golden.py sensitivity, tests/sens_ref.py: Richardson-extrapolated differences of steady states of the oracle).

Bounds:
* analytic columns against central differences of the node function (relative step 1e-5): 1e-6 of the column's largest
  magnitude.  Truncation is O(h^2) = 1e-10; rounding is eps/h = 1e-11 of the TERMS of f, which exceed a column by up to
  three decades where fast equilibrium reactions cancel - 1e-8, two decades below the bound.
* the sweep against G21, per (parameter, row): 10 x the golden's fd_error plus the case's floor, sens_ref.FLOOR_REL of the
  row's largest magnitude (sens_ref.bound).  The floor is 10 x the case's own largest difference measured on the first run
  (profiles/sensitivity.md), and never above 1e-6 - it covers that the host march's state and the golden's differ by 1e-9
  and the sweep linearises about its own.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the hipRTC that compiles is the one torch bundles)

import inputs as INP
import profile_ref as PR
import sens_ref as SR
from helpers.host_build import build_helper
from rmt_app_amd import hipbind, isa, n2, plan, rmtExe, sensitivity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "sens_emu.cpp")
COLUMN_BOUND = 1e-6
TOL, MAX_IT = 1e-10, 400
F = plan.MEMBER_FIELDS


def _input(model="N2", spec=None, **cfg):
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.05)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False", "initial": "steady",
                                "sensitivity": {"parameters": ["medium-temperature"]} if spec is None else spec})
    mi["solver-config"].update(cfg)
    return mi


# ----------------------------------------------------------------------------- validation
BAD = [
    ("medium-temperature", "sensitivity"),                                  # not a dict
    ({"params": ["medium-temperature"]}, "params"),                         # unknown key
    ({"parameters": []}, "parameters"),
    ({"parameters": "medium-temperature"}, "parameters"),
    ({"parameters": ["coolant"]}, "coolant"),
    ({"parameters": [{"inlet-concentration": "N2O"}]}, "N2O"),
    ({"parameters": [{"outlet-concentration": "CO"}]}, "outlet-concentration"),
    ({"parameters": [{"rate-constant": "nope"}]}, "nope"),
    ({"parameters": [{"inlet-concentration": "CO", "rate-constant": "CaBeDe"}]}, "ONE key"),
    ({"parameters": ["inlet-pressure", "inlet-pressure"]}, "duplicate"),
    ({"parameters": [{"inlet-concentration": "CO"}, {"inlet-concentration": "CO"}]}, "duplicate"),
    ({"parameters": ["medium-temperature", "inlet-temperature", "inlet-pressure"]
      + [{"inlet-concentration": c} for c in ("H2", "CO2", "H2O", "CO", "CH3OH", "DME")]}, "at most 8"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec=spec)
    with pytest.raises(ValueError, match="sensitivity") as e:
        sensitivity.parse(mi)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="sensitivity") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)
    assert word in str(e.value)
    capsys.readouterr()


def test_good_specs_and_what_is_not_available(capsys):
    mi = _input()
    del mi["solver-config"]["sensitivity"]
    assert sensitivity.parse(mi) is None
    s = sensitivity.parse(_input(spec={"parameters": SR.BOUNDARY4 + [{"rate-constant": "CaBeDe"}]}))
    assert s.NP == 5 and s.labels == ["medium-temperature", "inlet-temperature", "inlet-pressure", "inlet-concentration:CO",
                                      "rate-constant:CaBeDe"]
    assert s.rate_constants == ["CaBeDe"] and s.unit_params(()) == ("CaBeDe",) and s.unit_params(("CaBeDe",)) == ("CaBeDe",)
    mech = plan.Mechanism(_input(), params=s.unit_params(()))
    kinds, idx = s.descriptors(mech)
    assert list(kinds) == [0, 1, 2, 3, 4] and list(idx) == [0, 0, 0, mech.compList.index("CO"), 0]
    eight = ["medium-temperature", "inlet-temperature"] + [{"inlet-concentration": c} for c in mech.compList]
    assert len(eight) == 8 and sensitivity.parse(_input(spec={"parameters": eight})).NP == 8
    for model in ("M2", "N1", "M7", "M1"):
        with pytest.raises(NotImplementedError, match="'sensitivity'.*only available for model 'N2'"):
            rmtExe(_input(model))
    with pytest.raises(NotImplementedError, match="'sensitivity'.*fp32"):
        rmtExe(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'sensitivity'.*multi-rank"):
        sensitivity.parse(_input(), multi_rank=True)
    no_initial = _input()
    del no_initial["solver-config"]["initial"]
    with pytest.raises(NotImplementedError, match="'sensitivity'.*\"initial\": \"steady\""):
        rmtExe(no_initial)
    dea = _input(deactivation={"time-on-stream": [1e5], "steps": 2, "rate-constant": 2e-7, "activation-energy": 8e4,
                               "reference-temperature": 623.0})
    with pytest.raises(NotImplementedError, match="'sensitivity'.*'deactivation'"):
        rmtExe(dea)
    with pytest.raises(NotImplementedError, match="'sensitivity'.*not a scalar constant"):
        name = [k for k, v in _input()["reaction-rates"]["VARS"].items() if callable(v)][0]
        rmtExe(_input(spec={"parameters": [{"rate-constant": name}]}))
    capsys.readouterr()


# ----------------------------------------------------------------------------- the plan
def _rows(name="dme_nb", zNo=20, params=()):
    mi = INP.ALL_N2_INPUTS[name]()
    mech = plan.Mechanism(mi, params=params)
    return mi, mech, plan.member_constants(mi, mech, zNo)[1]


def test_the_sweep_is_a_unit_of_its_own_and_every_other_unit_is_untouched():
    from test_campaign_cpu import PARENT_KEYS, PARENT_TEMPLATE
    mi, mech, row = _rows()
    whole = hipbind.kernel_template()
    tpl = plan.without_campaign(whole)
    assert hashlib.sha256(tpl.encode()).hexdigest() == PARENT_TEMPLATE          # the template of every ordinary unit
    assert "sens" not in tpl.lower() and "rmt_n2_steady_sens" in whole and whole.startswith(tpl)
    units = {"ros4": n2.code_plan(mech, 20, block=n2.ros4_block(mech.V, 20), npt=1, rows=row, features=("ros4",)),
             "rk4": n2.code_plan(mech, 20, rows=row), "march": n2.march_plan(mech, 20, None, row),
             "march_profiled": n2.march_plan(mech, 20, {"RMT_PROFILE": "1"}, row)}
    for name, cp in units.items():
        src, key = n2.plan_unit(mech, False, cp)
        assert key == PARENT_KEYS[name], name                                  # ... and their cache keys
        assert "rmt_n2_steady_sens" not in src and "RMT_SENS" not in src
    camp, ckey = n2.plan_unit(mech, False, n2.campaign_plan(mech, 20, row))
    assert "rmt_n2_steady_sens" not in camp and "RMT_SENS" not in camp and "void rmt_n2_campaign_step(" in camp
    cp = n2.sens_plan(mech, 20, 4, None, row)
    march = n2.march_plan(mech, 20, None, row)
    assert (cp.block, cp.npt, cp.features) == (64, 1, ("march",))
    assert cp.defines == {**march.defines, "RMT_SENS": "1", "RMT_SENS_NP": "4"}
    assert not any(k.startswith("RMT_MC_") for k in cp.defines)
    src, key = n2.plan_unit(mech, False, cp)
    assert "#define RMT_SENS 1" in src and "void rmt_n2_steady_sens(" in src and "void rmt_n2_steady_march(" in src
    assert "rmt_kinetics_jacs" in src and "campaign" not in src.lower()
    assert key not in PARENT_KEYS.values() and key != ckey
    assert '#error "RMT_SENS: needs RMT_WITH_MARCH' in src
    # forced and profiled rows travel as they do for the march
    fp = n2.sens_plan(mech, 20, 2, {"RMT_FORCING": "2", "RMT_PROFILE": "1", "RMT_RK45_LDS": "2"})
    assert fp.defines["RMT_FORCING"] == "2" and fp.defines["RMT_PROFILE"] == "1" and "RMT_RK45_LDS" not in fp.defines
    with pytest.raises(ValueError, match="RMT_SENS_NP"):
        mech.source(whole, False, 64, 1, None, {"RMT_WITH_MARCH": "1", "RMT_SENS_NP": "2"})


def test_campaign_unit_key_is_what_it_is_without_this_file(tmp_path):
    """the campaign unit's source is generated from the template without the sweep's text: it equals the source generated
    from a template that never had it"""
    mi, mech, row = _rows()
    whole = hipbind.kernel_template()
    cp = n2.campaign_plan(mech, 20, row)
    assert mech.source(whole, False, cp.block, cp.npt, cp.lds_state, cp.defines) == \
        mech.source(plan._cut(whole, plan.SENS_MARKS), False, cp.block, cp.npt, cp.lds_state, cp.defines)
    assert plan._cut(whole, plan.SENS_MARKS).endswith(plan.CAMPAIGN_MARKS[1])


@pytest.mark.parametrize("name,NP", [("dme_nb", 4), ("dme_nb", 8), ("ch4", 1), ("syn12", 2)])
def test_sens_unit_cross_compiles_for_gfx950(name, NP):
    """hipRTC, no GPU: DME (V = 7), ch4 (isothermal) and the 12-species mechanism; the registers are reported."""
    mi, mech, row = _rows(name)
    code = n2.compile_plan(mech, False, n2.sens_plan(mech, 20, NP, None, row), "gfx950")
    assert code[:4] == b"\x7fELF" and b"rmt_n2_steady_sens" in code and b"rmt_n2_steady_march" in code
    res = isa.kernel_resources(code, "rmt_n2_steady_sens")
    print("%s NP = %d: rmt_n2_steady_sens %s" % (name, NP, res))
    if name != "syn12":
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0


# ----------------------------------------------------------------------------- the per-node code on the host
_BUILT = {}


def _build(tmp, name, NP, params=(), profiled=False, zNo=20, sanitize=False):
    key = (name, NP, tuple(params), profiled, sanitize)
    if key not in _BUILT:
        mi, mech, row = _rows(name, zNo, params)
        src, _ = n2.plan_unit(mech, False, n2.sens_plan(mech, zNo, NP, {"RMT_PROFILE": "1"} if profiled else None, row))
        tag = "%s_%d_%d%s%s" % (name, NP, len(params), "_p" if profiled else "", "_san" if sanitize else "")
        _BUILT[key] = build_helper(HELPER, src, tmp, tag, "sens_%s" % tag, sanitize)
    mi, mech, row = _rows(name, zNo, params)
    return _BUILT[key], mi, mech, row


@pytest.fixture(scope="module")
def bdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sens"))


def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _run(exe, text, env=None):
    p = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = {}
    for ln in p.stdout.split("\n"):
        w = ln.split()
        if w:
            out.setdefault(w[0], []).append(np.array([float.fromhex(v) if "x" in v or "n" in v else float(v) for v in w[1:]]))
    return out, p


def _table(table):
    return "" if table is None else "A %d %s\n" % (table.shape[1], _hex(table))


def _march(exe, row, N, table=None):
    return _run(exe, "M %s\n%sR %d %r %d\n" % (_hex(row), _table(table), N, TOL, MAX_IT))[0]["state"][0]


def _sweep(exe, row, N, kinds, idx, y, table=None):
    out, _ = _run(exe, "M %s\n%sS %d %s %s\n" % (_hex(row), _table(table), N,
                                                 " ".join("%d %d" % (k, i) for k, i in zip(kinds, idx)), _hex(y)))
    return out["out"][0].reshape(len(kinds), -1, N), int(out["end"][0][0])


def _node(exe, row, P, y, up=None, act=1.0, dtm=0.0):
    """the F record (f [V], az) or, without ``up``, the J record of the helper"""
    if up is not None:
        f = _run(exe, "M %s\nF %s %s %s %s %s\n" % (_hex(row), float(P).hex(), float(act).hex(), float(dtm).hex(), _hex(y),
                                                    _hex(up)))[0]["f"][0]
        assert abs(f[-1] - (1.0 + f[-2])) <= 2.3e-16          # az as rmt_node_pre returns it IS 1 + the re-formed az - 1
        return f[:-2], f[-2]
    return _run(exe, "M %s\nJ %s %s %s %s\n" % (_hex(row), float(P).hex(), float(act).hex(), float(dtm).hex(), _hex(y)))[0]


def _central(fun, x0, h):
    return (fun(x0 + h) - fun(x0 - h))/(2*h)


@pytest.mark.parametrize("name,profiled", [("dme_nb", False), ("dme_nb", True), ("syn12", False)])
def test_analytic_columns_against_differences_of_the_node_function(name, profiled, bdir):
    """Every analytic column of the sweep (df/dy, df/dup, df/dP, df/dTM, df/du_k, d az/dy) at a converged node of the bed
    against central differences of the node function, evaluated in the same helper."""
    params = ("CaBeDe",) if name == "dme_nb" else ()
    exe, mi, mech, row = _build(bdir, name, 2, params, profiled)
    N, V, S = 20, mech.V, mech.S
    table = np.stack(PR.bed(PR.BED_A, N, row[F["TM"]])) if profiled else None
    Y = _march(exe, row, N, table).reshape(V, N)
    worst = {}
    for z in (0, 7, N - 1):
        act, dtm = (table[0, z], table[1, z]) if profiled else (1.0, 0.0)
        y = Y[:, z]
        up = np.concatenate([np.maximum(row[F["CIN"]:F["CIN"] + S], 1e-30), [row[F["THETA_IN"]]]]) if z == 0 \
            else np.concatenate([np.maximum(Y[:S, z - 1], 1e-30), [Y[S, z - 1]]])
        P = row[F["P0"]]*(1.0 - 1e-3*z)                                   # (any pressure near the node's own serves)
        J = _node(exe, row, P, y, act=act, dtm=dtm)
        a = J["a"][0].reshape(V, V)
        assert np.array_equal(J["a"][0], J["ajac"][0])          # rmt_sens_eval restates rmt_node_jac: bit for bit

        def f_of(row_=row, P_=P, y_=y, up_=up):
            return _node(exe, row_, P_, y_, up_, act, dtm)

        def check(what, got, want):
            scale = max(np.max(np.abs(want)), 1e-300)
            worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(got - want))/scale))

        for j in range(V):
            h = 1e-5*max(abs(y[j]), 1e-3)
            e = np.zeros(V)
            e[j] = h
            fp, azp = f_of(y_=y + e)
            fm, azm = f_of(y_=y - e)
            check("df/dy", -a[:, j], (fp - fm)/(2*h))
            check("daz/dy", J["daz"][0][j], np.array([(azp - azm)/(2*h)]))
            hu = 1e-5*max(abs(up[j]), 1e-3)
            e[j] = hu
            want = (f_of(up_=up + e)[0] - f_of(up_=up - e)[0])/(2*hu)
            U = np.zeros(V)
            U[j] = row[F["F1"]]*row[F["INV_DZ"]] if j < S else row[F["FT"]]*row[F["INV_DZ"]]
            check("df/dup", U, want)
        hP = 1e-5*P
        check("df/dP", J["fP"][0], (f_of(P_=P + hP)[0] - f_of(P_=P - hP)[0])/(2*hP))

        def with_field(i, v):
            r = row.copy()
            r[i] = v
            return r
        i, h = F["TM"], 1e-5*row[F["TM"]]
        want = (f_of(row_=with_field(i, row[i] + h))[0] - f_of(row_=with_field(i, row[i] - h))[0])/(2*h)
        ftm = np.zeros(V)
        ftm[S] = J["ftm"][0][0]
        check("df/dTM", ftm, want)
        for k in range(len(params)):
            i = plan.MEMBER_FIXED + S + k
            h = 1e-5*row[i]
            want = (f_of(row_=with_field(i, row[i] + h))[0] - f_of(row_=with_field(i, row[i] - h))[0])/(2*h)
            check("df/du", J["fU"][0].reshape(-1, V)[k], want)
    print("%s%s: analytic columns against central differences, relative to the column's largest magnitude: %s"
          % (name, " (bed A)" if profiled else "", ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    assert len(worst) == (6 if params else 5) and max(worst.values()) <= COLUMN_BOUND, worst


def _case(name, bdir, sanitize=False):
    """(exe, mech, named, row, table, sens, kinds, idx) of a golden case"""
    case = SR.CASES[name]
    mi = SR.case_input(name)
    sens = sensitivity.parse(mi)
    params = sens.unit_params(())
    profiled = bool(SR.profile_spec(case))
    exe, _, mech, _ = _build(bdir, case["input"], sens.NP, params, profiled, case["zNo"], sanitize)
    named, row = plan.member_constants(mi, mech, case["zNo"])
    table = np.stack(PR.bed(SR.profile_spec(case), case["zNo"], row[F["TM"]])) if profiled else None
    kinds, idx = sens.descriptors(mech)
    return exe, mech, named, row, table, sens, kinds, idx


_MEASURED = {}


@pytest.mark.parametrize("name", list(SR.CASES))
def test_host_sweep_against_the_golden_sensitivities(name, bdir):
    """The whole sweep on the host march's state against G21: per (parameter, row) within 10 fd_error + the floor."""
    exe, mech, named, row, table, sens, kinds, idx = _case(name, bdir)
    N = SR.CASES[name]["zNo"]
    y = _march(exe, row, N, table)
    raw, failed = _sweep(exe, row, N, kinds, idx, y, table)
    assert failed == -1 and np.all(np.isfinite(raw))
    gold = SR.golden(name)
    p, unit = sensitivity.parameter_values(sens, row, named, mech)
    assert np.allclose(p, gold["values"], rtol=1e-14, atol=0)
    state, pressure = sensitivity.to_physical(raw, unit, named, mech)
    got = np.concatenate([state, pressure[:, None, :]], axis=1)            # [P][V+1][N], the golden's rows
    diff = np.max(np.abs(got - gold["D"]), axis=2)
    mag = np.max(np.abs(gold["D"]), axis=2)
    over = diff - 10*gold["fd_error"]
    rel = np.where(mag > 0, diff/np.where(mag > 0, mag, 1.0), 0.0)
    _MEASURED[name] = float(rel.max())
    print("G21 %s: largest |sweep - golden| / max|row| = %.3e (the golden's fd_error / max|row| at most %.3e); largest "
          "excess over 10 fd_error, relative to the row: %.3e"
          % (name, rel.max(), SR.meta()["cases"][name]["fd_error_relative"],
             float(np.max(np.where(mag > 0, over/np.where(mag > 0, mag, 1.0), 0.0)))))
    assert np.all(diff <= SR.bound(gold, name)), (name, np.argwhere(diff > SR.bound(gold, name)))
    # the result entry: the peak row is the temperature row at the node of the discrete maximum
    entry = sensitivity.result_entry(sens, raw, y, row, named, mech)
    T = y.reshape(mech.V, N)[mech.S]*named["Tf"] + named["Tf"]
    n = int(np.argmax(T))
    assert np.array_equal(entry["peak-temperature"], state[:, mech.S, n]) and entry["peak-position"] == np.linspace(0, 1, N)[n]
    assert np.array_equal(entry["normalized-peak"], p/T[n]*state[:, mech.S, n])
    assert entry["state"].shape == (sens.NP, mech.V, N) and entry["pressure"].shape == (sens.NP, N)
    assert entry["outlet-mole-fraction"].shape == (sens.NP, mech.S)
    assert np.max(np.abs(entry["outlet-mole-fraction"].sum(axis=1))) < 1e-12*np.max(np.abs(entry["outlet-mole-fraction"]))
    assert entry["parameters"] == sens.labels and entry["labelList"] == mech.compList + ["Temperature"]


def test_numpy_emulation_agrees_with_the_helper(bdir):
    """sensitivity.emulate on the helper's per-node blocks reproduces the helper's sweep (case SK: a rate constant and
    the coolant temperature)."""
    exe, mech, named, row, table, sens, kinds, idx = _case("SK", bdir)
    N, V, S = 20, mech.V, mech.S
    Y = _march(exe, row, N).reshape(V, N)
    raw, _ = _sweep(exe, row, N, kinds, idx, Y)
    blocks, P = [], row[F["P0"]]
    U = np.array([row[F["F1"]]*row[F["INV_DZ"]]]*S + [row[F["FT"]]*row[F["INV_DZ"]]])
    for z in range(N):
        J = _node(exe, row, P, Y[:, z])
        ftm = np.zeros(V)
        ftm[S] = J["ftm"][0][0]
        blocks.append({"a": J["a"][0].reshape(V, V), "fP": J["fP"][0], "fp": [J["fU"][0].reshape(-1, V)[0], ftm], "U": U,
                       "D": np.concatenate([(Y[:S, z] > 1e-30).astype(float), [1.0]]), "daz": J["daz"][0],
                       "az": J["az"][0][0], "P": P})
        P = J["az"][0][0]*P + row[F["BETA"]]
    emu = sensitivity.emulate(blocks, (np.zeros((2, V)), np.zeros(2)))
    scale = np.max(np.abs(raw), axis=2, keepdims=True)
    print("numpy emulation against the helper: %.2e of the row's largest magnitude" % float(np.max(np.abs(emu - raw)/scale)))
    assert np.all(np.abs(emu - raw) <= 1e-10*scale)          # (LAPACK's inverse against Gauss-Jordan: condition x eps)


def test_one_node_clamped_feed_and_wall_off(bdir):
    exe, mi, mech, row = _build(bdir, "dme_nb", 4)
    V, S = mech.V, mech.S
    co, h2o = mech.compList.index("CO"), mech.compList.index("H2O")
    kinds, idx = [0, 1, 2, 3], [0, 0, 0, co]
    # N = 1: one node, its own sensitivities; the pressure row is the seed (dP_0/dP0 = 1)
    y1 = _march(exe, row, 1)
    raw1, failed = _sweep(exe, row, 1, kinds, idx, y1)
    y20 = _march(exe, row, 20).reshape(V, 20)
    raw20, _ = _sweep(exe, row, 20, kinds, idx, y20)
    assert failed == -1 and raw1.shape == (4, V + 1, 1) and np.array_equal(raw1[:, V, 0], [0.0, 0.0, 1.0, 0.0])
    assert np.array_equal(y1, y20[:, 0]) and np.array_equal(raw1[:, :, 0], raw20[:, :, 0])
    # a feed component at the clamp: an all-zero row (the inlet value the model uses is the clamp)
    clamped = row.copy()                                  # (a feed without the products, as tests/test_initial_cpu.py has it)
    for sym in ("H2O", "CH3OH", "DME"):
        clamped[F["CIN"] + mech.compList.index(sym)] = 0.0
    yc = _march(exe, clamped, 20)
    rawc, failed = _sweep(exe, clamped, 20, [0, 1, 2, 3], [0, 0, 0, h2o], yc)
    assert failed == -1 and not np.any(rawc[3]) and np.any(rawc[0]) and np.any(rawc[1]) and np.any(rawc[2])
    # wall off: a zero "medium-temperature" row
    off = row.copy()
    off[F["TM"]] = 0.0
    yo = _march(exe, off, 20)
    rawo, failed = _sweep(exe, off, 20, kinds, idx, yo)
    assert failed == -1 and not np.any(rawo[0]) and np.any(rawo[1]) and np.any(rawo[3])
    # a singular node is reported, with NaN rows at that node and nothing behind it
    dead = row.copy()
    dead[F["F1"]] = dead[F["INV_MACOTE"]] = 0.0
    rawd, failed = _sweep(exe, dead, 20, kinds, idx, y20)
    assert failed == 0 and np.all(np.isnan(rawd[:, :, 0])) and not np.any(rawd[:, :, 1:])
    assert sensitivity.failed_node(rawd) == 0 and sensitivity.failed_node(raw20) == -1


def test_host_sweep_under_address_and_ub_sanitizers(bdir):
    """The same stand-alone program built with -fsanitize=address,undefined marches and sweeps case SA clean."""
    exe, mech, named, row, table, sens, kinds, idx = _case("SA", bdir, sanitize=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"}
    out, p = _run(exe, "M %s\nR 20 %r %d\n" % (_hex(row), TOL, MAX_IT), env)
    y = out["state"][0]
    text = "M %s\nS 20 %s %s\n" % (_hex(row), " ".join("%d %d" % (k, i) for k, i in zip(kinds, idx)), _hex(y))
    out, p = _run(exe, text, env)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    assert int(out["end"][0][0]) == -1
