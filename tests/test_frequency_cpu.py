"""solver-config "frequency-response" without a GPU: validation, `crossover`, the numpy restatement of the sweep, the
code-object plan (the sweep is a unit of its own, every other unit is untouched), cross-compilation of the unit, the C
entry point, and the per-node code compiled for the host (tests/helpers/freq_emu.cpp) against the goldens G23
(tools/make_golden.py frequency, tests/freq_ref.py: the dense linearisation of the oracle, solved by LAPACK per frequency).

Bounds:
* frequency.emulate at w = 0 against sensitivity.emulate: 1e-13 of the row's largest magnitude (the same elimination on the
  same numbers, once through a solve and once through an inverse, on blocks of condition < 10);
* frequency.emulate against the dense complex solve of the assembled block-bidiagonal system, random well-conditioned
  blocks: 1e-11 of the row's largest magnitude;
* the host emulation of the unit against G23, per (input, row): 10 x the golden's fd_error plus the case's floor,
  freq_ref.FLOOR_REL of the row's largest magnitude (freq_ref.bound) - the rule of sens_ref.FLOOR_REL: 10 x the case's own
  largest difference as first measured, never above 1e-6 (profiles/frequency_response.md has the measured values);
* crossover on 1/(1+s)^3, 200 log-spaced points: w_u = sqrt(3) and K_u = 8 to 1e-3 relative.
Each test prints its figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the hipRTC that compiles is the one torch bundles)

import freq_ref as FQ
import inputs as INP
import profile_ref as PR
import sens_ref as SR
from helpers.host_build import build_helper
from rmt_app_amd import frequency, hipbind, isa, n2, plan, rmtExe, sensitivity
from rmt_app_amd.codeplan import freq_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "freq_emu.cpp")
TOL, MAX_IT = 1e-10, 400
F = plan.MEMBER_FIELDS
# cache keys of the sensitivity units of the commit before this feature (dme_nb and ch4 at 1, 2, 4 parameters, profiled 4)
PARENT_SENS_KEYS = {("dme_nb", 1, False): "fdbfd068abfbae14e8f2e9d8", ("dme_nb", 2, False): "b7fde9b60f753526559ea935",
                    ("dme_nb", 4, False): "a6e69e8e958a1f3771b7bb36", ("dme_nb", 4, True): "5b638805ceb194355de754b7",
                    ("ch4", 1, False): "3f63a88c94db2c2718e8bd48", ("ch4", 2, False): "e64bcd741389164bc78d2473",
                    ("ch4", 4, False): "6c292f20e0bbf8739c93ce4a", ("ch4", 4, True): "06f40a1a0f308d0e7c628334"}


def _input(model="N2", spec=None, **cfg):
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.05)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False", "initial": "steady",
                                "frequency-response": {"inputs": ["medium-temperature"], "frequencies": [0.0, 1.0]}
                                if spec is None else spec})
    mi["solver-config"].update(cfg)
    return mi


# ----------------------------------------------------------------------------- validation
W = [0.0, 1.0]
BAD = [
    ("medium-temperature", "frequency-response"),                                   # not a dict
    ({"input": ["medium-temperature"], "frequencies": W}, "input"),                 # unknown key
    ({"inputs": [], "frequencies": W}, "inputs"),
    ({"inputs": "medium-temperature", "frequencies": W}, "inputs"),
    ({"inputs": ["coolant"], "frequencies": W}, "coolant"),
    ({"inputs": [{"inlet-concentration": "N2O"}], "frequencies": W}, "N2O"),
    ({"inputs": [{"rate-constant": "CaBeDe"}], "frequencies": W}, "rate-constant"),
    ({"inputs": ["inlet-pressure", "inlet-pressure"], "frequencies": W}, "duplicate"),
    ({"inputs": ["medium-temperature", "inlet-temperature", "inlet-pressure", {"inlet-concentration": "CO"},
                 {"inlet-concentration": "H2"}], "frequencies": W}, "at most 4"),
    ({"inputs": ["medium-temperature"]}, "'frequencies' is missing"),
    ({"inputs": ["medium-temperature"], "frequencies": []}, "frequencies"),
    ({"inputs": ["medium-temperature"], "frequencies": [1.0, -1.0]}, ">= 0"),
    ({"inputs": ["medium-temperature"], "frequencies": [1.0, float("nan")]}, "finite"),
    ({"inputs": ["medium-temperature"], "frequencies": [1.0, "fast"]}, "numbers"),
    ({"inputs": ["medium-temperature"], "frequencies": list(np.linspace(0, 1, 4097))}, "at most 4096"),
    ({"inputs": ["medium-temperature"], "frequencies": {"range": [0.0, 1.0], "points": 8}}, "w_lo"),
    ({"inputs": ["medium-temperature"], "frequencies": {"range": [2.0, 1.0], "points": 8}}, "w_lo"),
    ({"inputs": ["medium-temperature"], "frequencies": {"range": [1.0, 2.0], "points": 1}}, "points"),
    ({"inputs": ["medium-temperature"], "frequencies": {"range": [1.0, 2.0], "points": 5000}}, "at most 4096"),
    ({"inputs": ["medium-temperature"], "frequencies": {"range": [1.0, 2.0]}}, "'range' and 'points'"),
    ({"inputs": ["medium-temperature"], "frequencies": W, "profile": "yes"}, "profile"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec=spec)
    with pytest.raises(ValueError, match="frequency-response") as e:
        frequency.parse(mi)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="frequency-response") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)
    assert word in str(e.value)
    capsys.readouterr()


def test_good_specs_and_what_is_not_available(capsys):
    mi = _input()
    del mi["solver-config"]["frequency-response"]
    assert frequency.parse(mi) is None
    fr = frequency.parse(_input(spec={"inputs": SR.BOUNDARY4, "frequencies": [0, 0.5, 2], "profile": True}))
    assert fr.NP == 4 and fr.F == 3 and fr.profile and list(fr.omegas) == [0.0, 0.5, 2.0]
    assert fr.labels == ["medium-temperature", "inlet-temperature", "inlet-pressure", "inlet-concentration:CO"]
    mech = plan.Mechanism(_input())
    kinds, idx = fr.descriptors(mech)
    assert list(kinds) == [0, 1, 2, 3] and list(idx) == [0, 0, 0, mech.compList.index("CO")]
    fr = frequency.parse(_input(spec={"inputs": ["inlet-pressure"], "frequencies": {"range": [1e-2, 1e2], "points": 32}}))
    assert fr.F == 32 and not fr.profile and fr.omegas[0] == 1e-2 and fr.omegas[-1] == 1e2
    assert np.allclose(np.diff(np.log(fr.omegas)), np.log(1e4)/31, rtol=1e-12)
    assert frequency.parse(_input(spec={"inputs": ["inlet-pressure"], "frequencies": list(np.linspace(0, 1, 4096))})).F == 4096
    for model in ("M2", "N1", "M7", "M1"):
        with pytest.raises(NotImplementedError, match="'frequency-response'.*only available for model 'N2'"):
            rmtExe(_input(model))
    with pytest.raises(NotImplementedError, match="'frequency-response'.*fp32"):
        rmtExe(_input(dtype="fp32"))
    with pytest.raises(NotImplementedError, match="'frequency-response'.*multi-rank"):
        frequency.parse(_input(), multi_rank=True)
    no_initial = _input()
    del no_initial["solver-config"]["initial"]
    with pytest.raises(ValueError, match="'frequency-response'.*\"initial\": \"steady\""):
        rmtExe(no_initial)
    dea = _input(deactivation={"time-on-stream": [1e5], "steps": 2, "rate-constant": 2e-7, "activation-energy": 8e4,
                               "reference-temperature": 623.0})
    with pytest.raises(NotImplementedError, match="'frequency-response'.*'deactivation'"):
        rmtExe(dea)
    with pytest.raises(NotImplementedError, match="'frequency-response'.*'fit'"):
        frequency.parse(_input(fit={"parameters": ["A1"]}))
    import fit_ref
    fitted = fit_ref.case_input("FA")                  # (through rmtExe "fit" itself refuses the "initial" this key needs)
    fitted["solver-config"].update({"initial": "steady", "frequency-response": {"inputs": ["medium-temperature"], "frequencies": W}})
    with pytest.raises(NotImplementedError):
        rmtExe(fitted)
    wide = INP.syn12_input(ivp="hip-ros4")
    wide["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False", "initial": "steady",
                                  "frequency-response": {"inputs": ["medium-temperature"], "frequencies": W}})
    with pytest.raises(NotImplementedError, match="'frequency-response'.*at most 8 variables"):
        frequency.parse(wide, V=plan.Mechanism(wide).V)
    capsys.readouterr()


# ----------------------------------------------------------------------------- crossover
def test_crossover_of_a_third_order_lag():
    w = np.exp(np.linspace(np.log(1e-2), np.log(1e2), 200))
    G = 1.0/(1.0 + 1j*w)**3
    wu, Ku = frequency.crossover(w, G)
    print("crossover of 1/(1+s)^3 on 200 points: w_u = %.6f (sqrt 3 = %.6f), K_u = %.5f" % (wu, np.sqrt(3.0), Ku))
    assert abs(wu - np.sqrt(3.0)) <= 1e-3*np.sqrt(3.0) and abs(Ku - 8.0) <= 1e-3*8.0
    # a grid that starts at 0, a negative gain (the phase is relative to G(0)), and responses that never get there
    w0 = np.concatenate([[0.0], w])
    wu0, Ku0 = frequency.crossover(w0, -2.5/(1.0 + 1j*w0)**3)
    assert abs(wu0 - np.sqrt(3.0)) <= 1e-3*np.sqrt(3.0) and abs(Ku0 - 8.0/2.5) <= 1e-3*8.0/2.5
    assert frequency.crossover(w, 1.0/(1.0 + 1j*w)) is None and frequency.crossover(w, 1.0/(1.0 + 1j*w)**2) is None
    assert frequency.crossover(w, np.zeros(200)) is None
    with pytest.raises(ValueError):
        frequency.crossover(w[::-1], G)


# ----------------------------------------------------------------------------- the numpy restatement
def _random_blocks(rng, N, V, NP):
    blocks = []
    for z in range(N):
        a = np.eye(V)*(2.0 + rng.random()) + 0.3*rng.standard_normal((V, V))/np.sqrt(V)
        blocks.append({"a": a, "fP": 0.1*rng.standard_normal(V), "fp": 0.5*rng.standard_normal((NP, V)),
                       "U": 1.0 + rng.random(V), "D": (rng.random(V) > 0.2).astype(float), "daz": 0.1*rng.standard_normal(V),
                       "az": 1.0 - 0.01*rng.random(), "P": 1.0 + rng.random()})
    return blocks, (rng.standard_normal((NP, V)), rng.standard_normal(NP))


def _dense(blocks, seeds, w):
    """the assembled block lower-bidiagonal system in the unknowns (s_0, pi_0, s_1, pi_1, ..) solved by LAPACK: [NP][V+1][N]"""
    sd, pi = seeds
    NP, V = sd.shape
    N, n = len(blocks), V + 1
    A = np.zeros((N*n, N*n), dtype=np.complex128)
    rhs = np.zeros((N*n, NP), dtype=np.complex128)
    for z, b in enumerate(blocks):
        r = z*n
        A[r:r + V, r:r + V] = np.asarray(b["a"]) + 1j*w*np.eye(V)
        A[r:r + V, r + V] = -np.asarray(b["fP"])
        rhs[r:r + V] = np.asarray(b["fp"]).T
        A[r + V, r + V] = 1.0
        if z == 0:
            rhs[r:r + V] += (np.asarray(b["U"])[None, :]*sd).T
            rhs[r + V] = pi
        else:
            q = blocks[z - 1]
            A[r:r + V, r - n:r - n + V] = -np.diag(np.asarray(b["U"])*np.asarray(q["D"]))
            A[r + V, r - n + V] = -q["az"]
            A[r + V, r - n:r - n + V] = -q["P"]*np.asarray(q["daz"])
    x = np.linalg.solve(A, rhs)
    return np.transpose(x.reshape(N, n, NP), (2, 1, 0))


def test_emulate_at_zero_frequency_and_against_the_dense_solve():
    rng = np.random.default_rng(2310)
    blocks, seeds = _random_blocks(rng, 12, 5, 3)
    omegas = [0.0, 0.3, 4.0, 50.0]
    emu = frequency.emulate(blocks, seeds, omegas)
    assert emu.shape == (4, 3, 6, 12) and emu.dtype == np.complex128
    real = sensitivity.emulate(blocks, seeds)
    scale = np.max(np.abs(real), axis=2, keepdims=True)
    e0 = float(np.max(np.abs(emu[0] - real)/scale))
    assert not np.any(emu[0].imag) and e0 <= 1e-13
    worst = 0.0
    for f, w in enumerate(omegas):
        want = _dense(blocks, seeds, w)
        worst = max(worst, float(np.max(np.abs(emu[f] - want)/np.max(np.abs(want), axis=2, keepdims=True))))
    print("frequency.emulate: w = 0 against sensitivity.emulate %.2e, against the dense solve %.2e of the row" % (e0, worst))
    assert worst <= 1e-11
    assert np.max(np.abs(emu[3] - emu[0])) > 1e-2              # (the shift does something)


# ----------------------------------------------------------------------------- the plan
def _rows(name="dme_nb", zNo=20, iso=False):
    mi = INP.ALL_N2_INPUTS[name]()
    if iso:
        mi["operating-conditions"]["process-type"] = "iso-thermal"
    mech = plan.Mechanism(mi)
    return mi, mech, plan.member_constants(mi, mech, zNo)[1]


def test_the_sweep_is_a_unit_of_its_own_and_every_other_unit_is_untouched():
    from test_campaign_cpu import PARENT_KEYS, PARENT_TEMPLATE
    import hashlib
    whole = hipbind.kernel_template()
    assert hashlib.sha256(plan.without_campaign(whole).encode()).hexdigest() == PARENT_TEMPLATE
    nofreq = plan._cut(whole, plan.FREQ_MARKS)
    assert "rmt_n2_steady_freq" in whole and "freq" not in nofreq.lower() and nofreq.endswith(plan.SENS_MARKS[1])
    for name in ("dme_nb", "ch4"):
        mi, mech, row = _rows(name)
        units = {"ros4": n2.code_plan(mech, 20, block=n2.ros4_block(mech.V, 20), npt=1, rows=row, features=("ros4",)),
                 "rk4": n2.code_plan(mech, 20, rows=row), "march": n2.march_plan(mech, 20, None, row),
                 "march_profiled": n2.march_plan(mech, 20, {"RMT_PROFILE": "1"}, row),
                 "campaign": n2.campaign_plan(mech, 20, row)}
        for NP, prof in ((1, False), (2, False), (4, False), (4, True)):
            units[(name, NP, prof)] = n2.sens_plan(mech, 20, NP, {"RMT_PROFILE": "1"} if prof else None, row)
        for what, cp in units.items():
            src, key = n2.plan_unit(mech, False, cp)
            # the unit is what a template that never had the file gives
            assert src == mech.source(nofreq, False, cp.block, cp.npt, cp.lds_state, cp.defines), what
            assert "rmt_n2_steady_freq" not in src and "RMT_FREQ" not in src, what
            if name == "dme_nb" and what in PARENT_KEYS:
                assert key == PARENT_KEYS[what], what
            if what in PARENT_SENS_KEYS:
                assert key == PARENT_SENS_KEYS[what], what
    mi, mech, row = _rows()
    cp = freq_plan(mech, 20, 4, None, row)
    sens = n2.sens_plan(mech, 20, 4, None, row)
    assert (cp.block, cp.npt, cp.features) == (64, 1, ("march",))
    assert cp.defines == {**sens.defines, "RMT_FREQ": "1", "RMT_FREQ_NP": "4"} and n2.freq_plan is freq_plan
    src, key = n2.plan_unit(mech, False, cp)
    assert "#define RMT_FREQ 1" in src and "#define RMT_FREQ_NP 4" in src and "void rmt_n2_steady_freq(" in src
    assert "void rmt_n2_steady_sens(" in src and "void rmt_n2_steady_march(" in src and "campaign" not in src.lower()
    assert key not in PARENT_KEYS.values() and key not in PARENT_SENS_KEYS.values()
    assert src.count("rmt_sens_eval(") == 3          # defined once, called by the two sweeps: restated nowhere
    fp = freq_plan(mech, 20, 2, {"RMT_FORCING": "2", "RMT_PROFILE": "1", "RMT_RK45_LDS": "2"})
    assert fp.defines["RMT_FORCING"] == "2" and fp.defines["RMT_PROFILE"] == "1" and "RMT_RK45_LDS" not in fp.defines
    for bad in ({"RMT_WITH_MARCH": "1", "RMT_FREQ": "1", "RMT_FREQ_NP": "2"},
                {"RMT_WITH_MARCH": "1", "RMT_SENS": "1", "RMT_SENS_NP": "2", "RMT_FREQ_NP": "2"}):
        with pytest.raises(ValueError, match="RMT_FREQ"):
            mech.source(whole, False, 64, 1, None, bad)


@pytest.mark.parametrize("name,NP,iso", [("dme_nb", 1, False), ("dme_nb", 4, False), ("ch4", 1, True), ("ch4", 4, False)])
def test_freq_unit_cross_compiles_for_gfx950(name, NP, iso):
    """hipRTC, no GPU; the registers of the kernel are reported (profiles/frequency_response.md has them)."""
    mi, mech, row = _rows(name, iso=iso)
    assert mech.iso == iso
    code = n2.compile_plan(mech, False, freq_plan(mech, 20, NP, None, row), "gfx950")
    assert code[:4] == b"\x7fELF" and b"rmt_n2_steady_freq" in code and b"rmt_n2_steady_sens" in code
    res = isa.kernel_resources(code, "rmt_n2_steady_freq")
    print("%s%s NP = %d: rmt_n2_steady_freq %s" % (name, " (iso-thermal)" if iso else "", NP, res))
    assert res["vgpr_count"] <= 512


def test_c_entry_point():
    L = hipbind.lib()
    assert L.rmt_n2_abi_version() == hipbind.ABI_VERSION == 2
    assert hasattr(ctypes.CDLL(hipbind.LIB_PATH), "rmt_n2_steady_freq")
    hdr = open(os.path.join(ROOT, "include", "rmt_n2.h")).read()
    assert "int rmt_n2_steady_freq(rmt_n2_handle* h" in hdr
    one, w = (ctypes.c_int*1)(0), (ctypes.c_double*1)(1.0)
    out = (ctypes.c_double*64)()
    assert L.rmt_n2_steady_freq(None, None, 1, one, one, 1, w, one, 0, out) != 0
    assert b"rmt_n2_steady_freq: null argument" in L.rmt_n2_last_error()


# ----------------------------------------------------------------------------- the per-node code on the host
_BUILT = {}


@pytest.fixture(scope="module")
def bdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("freq"))


def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _run(exe, text):
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = {}
    for ln in p.stdout.split("\n"):
        w = ln.split()
        if w:
            out.setdefault(w[0], []).append(np.array([float.fromhex(v) if "x" in v or "n" in v else float(v) for v in w[1:]]))
    return out


def _table(table):
    return "" if table is None else "A %d %s\n" % (table.shape[1], _hex(table))


def march(exe, row, N, table=None):
    return _run(exe, "M %s\n%sR %d %r %d\n" % (_hex(row), _table(table), N, TOL, MAX_IT))["state"][0]


def sweep(exe, row, N, omegas, kinds, idx, y, table=None):
    """the helper's W record: ([F][NP][V+1][N] complex, failed [F])"""
    out = _run(exe, "M %s\n%sW %d %d %s %s %s\n" % (_hex(row), _table(table), N, len(omegas), _hex(omegas),
                                                   " ".join("%d %d" % (k, i) for k, i in zip(kinds, idx)), _hex(y)))
    raw = out["out"][0].reshape(len(omegas), len(kinds), -1, N, 2)
    return raw[..., 0] + 1j*raw[..., 1], out["end"][0].astype(int)


def case_unit(name, bdir):
    """(exe, mech, named, row, table, fr, kinds, idx) of a golden case"""
    case = FQ.CASES[name]
    mi = FQ.case_input(name)
    fr = frequency.parse(mi)
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, case["zNo"])
    profiled = bool(SR.profile_spec(case))
    if name not in _BUILT:
        src, _ = n2.plan_unit(mech, False, freq_plan(mech, case["zNo"], fr.NP, {"RMT_PROFILE": "1"} if profiled else None, row))
        _BUILT[name] = build_helper(HELPER, src, bdir, name, "freq_%s" % name)
    table = np.stack(PR.bed(SR.profile_spec(case), case["zNo"], row[F["TM"]])) if profiled else None
    kinds, idx = fr.descriptors(mech)
    return _BUILT[name], mech, named, row, table, fr, kinds, idx


@pytest.mark.parametrize("name", list(FQ.CASES))
def test_host_sweep_against_the_golden_responses(name, bdir):
    """The whole sweep on the host march's state against G23: per (input, row) within 10 fd_error + the floor."""
    exe, mech, named, row, table, fr, kinds, idx = case_unit(name, bdir)
    N = FQ.CASES[name]["zNo"]
    gold = FQ.golden(name)
    assert np.array_equal(fr.omegas, gold["frequencies"]) and fr.omegas[0] == 0.0 and fr.F == 9
    y = march(exe, row, N, table)
    raw, failed = sweep(exe, row, N, fr.omegas, kinds, idx, y, table)
    assert np.all(failed == -1) and np.all(np.isfinite(raw))
    p, unit = sensitivity.parameter_values(fr, row, named, mech)
    assert np.allclose(p, gold["values"], rtol=1e-14, atol=0)
    got = frequency.scale_rows(np.transpose(raw, (1, 0, 3, 2)), unit, named, mech)       # [P][F][N][V+1]
    got = np.transpose(got, (0, 1, 3, 2))                                                # [P][F][V+1][N]
    diff = np.max(np.abs(got - gold["G"]), axis=(1, 3))
    mag = np.max(np.abs(gold["G"]), axis=(1, 3))
    rel = np.where(mag > 0, diff/np.where(mag > 0, mag, 1.0), 0.0)
    print("G23 %s: largest |host sweep - golden| / max|row| = %.3e (the golden's fd_error / max|row| at most %.3e)"
          % (name, rel.max(), FQ.meta()["cases"][name]["fd_error_relative"]))
    assert np.all(diff <= FQ.bound(gold, name)), (name, np.argwhere(diff > FQ.bound(gold, name)))
    # w = 0 is real, and the golden's G(0) of FA is G21's D of SA within the two fd_errors
    assert not np.any(raw[0].imag)
    if name == "FA":
        sa = SR.golden("SA")
        assert np.all(np.max(np.abs(gold["G"][:, 0] - sa["D"]), axis=2) <= gold["fd_error"] + sa["fd_error"])
    # the result entry from the rows the kernel returns without and with "profile"
    peak = frequency.peak_node(y, mech, named)
    rows = np.stack([raw[..., N - 1], raw[..., peak if peak >= 0 else 0]], axis=2)       # [F][NP][2][V+1]
    entry = frequency.result_entry(fr, rows, raw, y, row, named, mech)
    assert np.array_equal(FQ.rows_of_entry(entry), got)
    assert entry["inputs"] == fr.labels and np.array_equal(entry["frequencies"], fr.omegas)
    assert entry["outlet-state"].shape == (fr.NP, fr.F, mech.V) and entry["outlet-pressure"].shape == (fr.NP, fr.F)
    assert np.array_equal(entry["outlet-state"], np.transpose(got[:, :, :mech.V, -1], (0, 1, 2)))
    assert np.array_equal(entry["outlet-pressure"], got[:, :, mech.V, -1])
    dx = entry["outlet-mole-fraction"]
    assert dx.shape == (fr.NP, fr.F, mech.S) and np.max(np.abs(dx.sum(axis=2))) <= 1e-12*max(np.max(np.abs(dx)), 1e-300)
    if mech.iso:
        assert entry["outlet-temperature"] is None and entry["peak-temperature"] is None and entry["peak-position"] is None
        assert entry["labelList"] == mech.compList
    else:
        assert np.array_equal(entry["outlet-temperature"], got[:, :, mech.S, -1])
        assert np.array_equal(entry["peak-temperature"], got[:, :, mech.S, peak])
        assert entry["peak-position"] == np.linspace(0, 1, N)[peak] and entry["labelList"] == mech.compList + ["Temperature"]
    short = frequency.result_entry(fr, rows, None, y, row, named, mech)
    assert "state" not in short and "pressure" not in short
    assert np.array_equal(short["outlet-state"], entry["outlet-state"])
    # G(0) of the entry is what sensitivity.result_entry makes of the real sweep's rows
    sens = sensitivity.result_entry(fr, raw[0].real, y, row, named, mech)
    assert np.allclose(entry["state"][:, 0].real, sens["state"], rtol=1e-15, atol=0)
    assert np.allclose(dx[:, 0].real, sens["outlet-mole-fraction"], rtol=1e-12, atol=1e-300)


def test_numpy_emulation_agrees_with_the_helper(bdir):
    """frequency.emulate on the helper's per-node blocks (the J record: what rmt_sens_eval forms) reproduces the helper's
    sweep of case FA: LAPACK's solve against the kernel's elimination without pivoting."""
    exe, mech, named, row, table, fr, kinds, idx = case_unit("FA", bdir)
    N, V, S = 20, mech.V, mech.S
    Y = march(exe, row, N).reshape(V, N)
    raw, _ = sweep(exe, row, N, fr.omegas, kinds, idx, Y)
    blocks, P = [], row[F["P0"]]
    U = np.array([row[F["F1"]]*row[F["INV_DZ"]]]*S + [row[F["FT"]]*row[F["INV_DZ"]]])
    for z in range(N):
        J = _run(exe, "M %s\nJ %s %s %s %s\n" % (_hex(row), float(P).hex(), float(1.0).hex(), float(0.0).hex(), _hex(Y[:, z])))
        ftm = np.zeros(V)
        ftm[S] = J["ftm"][0][0]
        blocks.append({"a": J["a"][0].reshape(V, V), "fP": J["fP"][0], "fp": [ftm, np.zeros(V), np.zeros(V), np.zeros(V)],
                       "U": U, "D": np.concatenate([(Y[:S, z] > 1e-30).astype(float), [1.0]]), "daz": J["daz"][0],
                       "az": J["az"][0][0], "P": P})
        P = J["az"][0][0]*P + row[F["BETA"]]
    sd = np.zeros((4, V))
    sd[1, S] = 1.0                                              # inlet temperature
    sd[3, idx[3]] = 1.0                                         # CO feed
    emu = frequency.emulate(blocks, (sd, np.array([0.0, 0.0, 1.0, 0.0])), fr.omegas)
    scale = np.max(np.abs(raw), axis=3, keepdims=True)
    err = float(np.max(np.abs(emu - raw)/scale))
    print("numpy emulation against the helper (FA, 9 frequencies): %.2e of the row's largest magnitude" % err)
    assert err <= 1e-10          # (condition x eps, the bound of the real sweep's twin test)


def test_host_sweep_under_address_and_ub_sanitizers(bdir):
    """The same stand-alone program built with -fsanitize=address,undefined marches and sweeps case FB (the profiled bed)
    clean."""
    exe, mech, named, row, table, fr, kinds, idx = case_unit("FB", bdir)
    src, _ = n2.plan_unit(mech, False, freq_plan(mech, 20, fr.NP, {"RMT_PROFILE": "1"}, row))
    san = build_helper(HELPER, src, bdir, "FB_san", "freq_FB_san", sanitize=True)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"}
    text = "M %s\n%sR 20 %r %d\n" % (_hex(row), _table(table), TOL, MAX_IT)
    p = subprocess.run([san], input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    y = march(exe, row, 20, table)
    text = "M %s\n%sW 20 %d %s %s %s\n" % (_hex(row), _table(table), fr.F, _hex(fr.omegas),
                                          " ".join("%d %d" % (k, i) for k, i in zip(kinds, idx)), _hex(y))
    p = subprocess.run([san], input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    ends = [ln for ln in p.stdout.split("\n") if ln.startswith("end")][0].split()[1:]
    assert all(float.fromhex(v) == -1.0 for v in ends)


def test_failure_stops_the_lane_at_the_node(bdir):
    """A NaN in the temperature at node 3 of the state: every frequency stops there with NaN at that node and nothing behind it."""
    exe, mech, named, row, table, fr, kinds, idx = case_unit("FA", bdir)
    y = march(exe, row, 20).reshape(mech.V, 20)
    good, _ = sweep(exe, row, 20, fr.omegas[:3], kinds, idx, y)
    y[mech.S, 3] = np.nan                 # (the temperature: the model's clamp takes a NaN in a species for a 0)
    raw, failed = sweep(exe, row, 20, fr.omegas[:3], kinds, idx, y)
    assert list(failed) == [3, 3, 3] and np.all(np.isnan(raw[..., 3])) and not np.any(raw[..., 4:])
    assert np.array_equal(raw[..., :3], good[..., :3])
