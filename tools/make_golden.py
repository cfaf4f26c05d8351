#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING THE REFERENCE (PyREMOT).

Runs only in the build container, where /root/reference exists:

    PYTHONPATH=/root/reference MPLBACKEND=Agg python3 tools/make_golden.py <what> [...]

<what> in: setup rhs rk4 tight=<case> default=<case> multistep n1 helpers plot m2 m2run setting m7 m1 schedule feed control steady profile campaign policy sensitivity fit frequency  (see
SURVEY.md section 8(c), G1..G7; m7 / m1: the steady models, G12; schedule[=probes|A|A1|B|C|D]: time-varying inlet and
coolant conditions, G13; feed[=probes|FA|FA1|FB|FC|FD]: time-varying feed composition, G14; control[=json|CA|CB|CC|CD]:
closed-loop runs with the sampled PI controller, G15; steady[=dme_script|dme_nb|syn12]: discrete steady states of model N2,
G17; profile[=A|B|C|AS|A0|C0|S]: axial profiles of catalyst activity and coolant temperature, G18; campaign[=DA|DB|DC|DI]:
time-on-stream runs with catalyst deactivation, G19; policy[=PA|PS|PB]: the coolant policy of such a run, G20;
sensitivity[=SA|SB|SK|SW]: parametric sensitivities of the steady state, G21; fit[=FA|FB|FN]: kinetic parameter
estimation from steady-state data, G22; fit_ext[=FC|FP|FL|FL:<feed>]: the same with log-scaled and bounded parameters and data
along the bed, G24; frequency[=FA|FB|FI]: frequency response of the steady state, G23 - like G13..G15 these
run SciPy on oracle/n2_oracle.py, so the repository root must be on PYTHONPATH as well).
The reference never travels to the GPU box; only the small .npz/.json files written here do.
Inputs come from tests/inputs.py (this repo's restatement of the reference's test inputs).
"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

import inputs as INP  # noqa: E402

import PyREMOT  # noqa: E402  (the reference)
from PyREMOT import rmtExe  # noqa: E402
import PyREMOT.docs.pbHomoReactor as PBH  # noqa: E402
from PyREMOT.docs.pbHomoReactor import PackedBedHomoReactorClass as PB  # noqa: E402
from PyREMOT.solvers.solSetting import solverSetting  # noqa: E402
from PyREMOT.solvers import odeSolver as ODES  # noqa: E402
import scipy.integrate  # noqa: E402

REAL_SOLVE_IVP = scipy.integrate.solve_ivp


class _Captured(Exception):
    pass


@contextlib.contextmanager
def quiet():
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        yield


@contextlib.contextmanager
def mesh(zNo=None, tNo=None, model="N2"):
    old = dict(solverSetting[model])
    if zNo is not None:
        solverSetting[model]["zNo"] = zNo
    if tNo is not None:
        solverSetting[model]["tNo"] = tNo
    try:
        yield
    finally:
        solverSetting[model].clear()
        solverSetting[model].update(old)


def capture(mi, zNo):
    """Run rmtExe up to the first solve_ivp call; return (IV, paramsSet)."""
    box = {}

    def fake(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
        box["IV"] = np.array(y0, dtype=float)
        box["params"] = args[0]
        raise _Captured()

    PBH.solve_ivp = fake
    try:
        with mesh(zNo), quiet():
            try:
                rmtExe(mi)
            except _Captured:
                pass
    finally:
        PBH.solve_ivp = REAL_SOLVE_IVP
    return box["IV"], box["params"]


def rhs(params, y):
    return np.array(PB.modelEquationN2(0.0, np.array(y, dtype=float), params), dtype=float)


def run_with_tol(mi, zNo, method, rtol=None, atol=None):
    nfev = [0]

    def wrapped(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
        if rtol is not None:
            kw["rtol"] = rtol
        if atol is not None:
            kw["atol"] = atol
        sol = REAL_SOLVE_IVP(fun, t_span, y0, method=method, t_eval=t_eval, args=args, **kw)
        nfev[0] += sol.nfev
        return sol

    mi = dict(mi)
    mi["solver-config"] = dict(mi["solver-config"], ivp=method)
    PBH.solve_ivp = wrapped
    t0 = time.time()
    try:
        with mesh(zNo), quiet():
            res = rmtExe(mi)
    finally:
        PBH.solve_ivp = REAL_SOLVE_IVP
    return res, nfev[0], time.time() - t0


def pack_datapack(res):
    dp = res["resModel"]["dataPack"]
    out = {}
    for k, d in enumerate(dp):
        for key in ("dataYs", "dataYCons1", "dataYCons2", "dataYTemp1", "dataYTemp2", "dataXs"):
            out["%s_%d" % (key, k)] = np.array(d[key], dtype=float)
        out["dataTime_%d" % k] = np.array(float(d["dataTime"]))
    out["n"] = np.array(len(dp))
    return out


def tolist(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [tolist(x) for x in v]
    if isinstance(v, dict):
        return {k: tolist(x) for k, x in v.items() if not callable(x)}
    return v


def synthetic_states(IV, V, N, seed):
    """Deterministic test states of the (V,N) layout: smooth profile, noisy, and one with
    negative / tiny concentrations (exercises the EPS clamp, pbHomoReactor.py:3899,4093)."""
    rng = np.random.default_rng(seed)
    Y0 = IV.reshape(V, N)
    z = np.linspace(0, 1, N)
    states = []
    s1 = Y0.copy()
    for i in range(V):
        if i < V - 1 or V == Y0.shape[0]:
            s1[i] = Y0[i]*(1.0 + 0.15*np.sin(2.0*np.pi*(z + 0.1*i))) + 0.003*(i + 1)*z
    s1[V - 1] = 0.02*z + 0.01*np.sin(3*np.pi*z)
    states.append(s1)
    s2 = np.abs(Y0*(1 + 0.05*rng.standard_normal(Y0.shape))) + 1e-4*rng.random(Y0.shape)
    s2[V - 1] = 0.03*rng.random(N) - 0.005
    states.append(s2)
    s3 = s1.copy()
    idx = rng.integers(0, N, size=max(2, N//10))
    S = V - 1
    s3[min(2, S - 1), idx] = -1e-3*rng.random(len(idx))
    if S > 4:
        s3[4, idx[::2]] = 0.0
    s3[0, idx[1::2]] = -5e-2
    states.append(s3)
    return [s.flatten() for s in states]


# --------------------------------------------------------------------------- G1
def g_setup():
    out = {}
    for name, fn in INP.ALL_N2_INPUTS.items():
        mi = fn()
        IV, params = capture(mi, 20)
        rls, rsc, FunParam, DAP, ptype = params
        out[name] = {
            "input": {
                "concentration": tolist(np.array(mi["feed"]["concentration"], dtype=float)),
                "volumetric-flowrate": float(mi["feed"]["volumetric-flowrate"]),
            },
            "const": tolist(FunParam["const"]),
            "constBC1": tolist(FunParam["constBC1"]),
            "ExHe": tolist(FunParam["ExHe"]),
            "DimensionlessAnalysisParams": tolist(DAP),
            "reactionListSorted": tolist(rls),
            "reactionStochCoeff": tolist(rsc),
            "processType": ptype,
            "IV": IV.tolist(),
        }
    # iso-thermal variant of the notebook case
    mi = INP.dme_notebook_input(process_type="iso-thermal")
    IV, params = capture(mi, 20)
    out["dme_nb_iso"] = {"const": tolist(params[2]["const"]), "IV": IV.tolist(),
                         "DimensionlessAnalysisParams": tolist(params[3])}
    with open(os.path.join(GOLD, "g1_setup.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("G1 written")


# --------------------------------------------------------------------------- G2
def g_rhs():
    out = {}
    cases = [("dme_nb", 20), ("dme_nb", 100), ("dme_nb", 1024), ("dme_script", 20),
             ("dme_script", 100), ("ch4", 20), ("ch4", 100), ("syn12", 20), ("syn12", 100)]
    for name, zNo in cases:
        mi = INP.ALL_N2_INPUTS[name]()
        IV, params = capture(mi, zNo)
        V = params[2]["const"]["varNo"]
        states = [IV] + synthetic_states(IV, V, zNo, seed=zNo + len(name))
        if zNo == 1024:
            states = states[:3]
        Y = np.array(states)
        t0 = time.time()
        F = np.array([rhs(params, y) for y in Y])
        print("G2 %s zNo=%d: %d RHS calls in %.1fs" % (name, zNo, len(Y), time.time() - t0))
        out["%s_%d_y" % (name, zNo)] = Y
        out["%s_%d_f" % (name, zNo)] = F
    # iso-thermal variant
    mi = INP.dme_notebook_input(process_type="iso-thermal")
    IV, params = capture(mi, 20)
    Y = np.array([IV] + [s.reshape(7, 20)[:6].flatten() for s in synthetic_states(
        np.concatenate([IV, np.zeros(20)]), 7, 20, seed=5)])
    out["dme_nb_iso_20_y"] = Y
    out["dme_nb_iso_20_f"] = np.array([rhs(params, y) for y in Y])
    # mid-transient states from the tight run (if present)
    p = os.path.join(GOLD, "g4_tight_dme_script_lsoda.npz")
    if os.path.exists(p):
        g4 = np.load(p)
        mi = INP.dme_script_input()
        IV, params = capture(mi, 20)
        Y = np.array([np.concatenate([g4["dataYCons1_%d" % k].flatten(),
                                      g4["dataYTemp1_%d" % k].flatten()]) for k in range(5)])
        out["dme_script_20_transient_y"] = Y
        out["dme_script_20_transient_f"] = np.array([rhs(params, y) for y in Y])
    np.savez_compressed(os.path.join(GOLD, "g2_rhs.npz"), **out)
    print("G2 written")


# --------------------------------------------------------------------------- G3
def g_rk4():
    out = {}
    for name, zNo, h, n, stride in [("dme_nb", 20, 1e-5, 200, 1), ("dme_script", 20, 1e-5, 200, 1),
                                    ("dme_nb", 100, 1e-5, 100, 10), ("ch4", 20, 1e-3, 200, 1),
                                    ("syn12", 20, 1e-5, 100, 1)]:
        mi = INP.ALL_N2_INPUTS[name]()
        IV, params = capture(mi, zNo)
        t0 = time.time()
        traj = ODES.RK4(0.0, n*h, n, IV, PB.modelEquationN2, params)
        print("G3 %s zNo=%d n=%d: %.1fs" % (name, zNo, n, time.time() - t0))
        key = "%s_%d" % (name, zNo)
        out[key + "_traj"] = traj[:, ::stride]
        out[key + "_h"] = np.array(h)
        out[key + "_n"] = np.array(n)
        out[key + "_stride"] = np.array(stride)
    np.savez_compressed(os.path.join(GOLD, "g3_rk4.npz"), **out)
    print("G3 written")


# --------------------------------------------------------------------------- G4/G5
def g_multistep():
    """Reference PreCorr3 / AdBash3 (PyREMOT/solvers/odeSolver.py:43-102) trajectories."""
    out = {}
    for name, zNo, h, n in [("dme_nb", 20, 2e-6, 120), ("ch4", 20, 1e-3, 120)]:
        mi = INP.ALL_N2_INPUTS[name]()
        IV, params = capture(mi, zNo)
        for meth in ("PreCorr3", "AdBash3"):
            traj = getattr(ODES, meth)(0.0, n*h, n, IV, PB.modelEquationN2, params)
            out["%s_%d_%s" % (name, zNo, meth)] = traj[:, [3, n//2, n]]
        out["%s_%d_h" % (name, zNo)] = np.array(h)
        out["%s_%d_n" % (name, zNo)] = np.array(n)
    np.savez_compressed(os.path.join(GOLD, "g3b_multistep.npz"), **out)
    print("G3b written")


def g_tight(which):
    name, method = which.split(":")
    tol = {"lsoda": ("LSODA", 1e-10, 1e-12), "bdf": ("BDF", 1e-9, 1e-12)}[method]
    mi = INP.ALL_N2_INPUTS[name]()
    res, nfev, wall = run_with_tol(mi, 20, tol[0], tol[1], tol[2])
    out = pack_datapack(res)
    out["nfev"] = np.array(nfev)
    out["wall"] = np.array(wall)
    np.savez_compressed(os.path.join(GOLD, "g4_tight_%s_%s.npz" % (name, method)), **out)
    print("G4 %s %s: nfev=%d wall=%.1fs" % (name, method, nfev, wall))


def g_default(name):
    mi = INP.ALL_N2_INPUTS[name]()
    res, nfev, wall = run_with_tol(mi, 20, "LSODA")
    out = pack_datapack(res)
    out["nfev"] = np.array(nfev)
    out["wall"] = np.array(wall)
    out["computation_time"] = np.array(res["resModel"]["computation-time"])
    np.savez_compressed(os.path.join(GOLD, "g5_default_%s.npz" % name), **out)
    print("G5 %s: nfev=%d wall=%.1fs" % (name, nfev, wall))


# --------------------------------------------------------------------------- G6
def g_n1():
    mi = INP.n1_notebook_input()
    t0 = time.time()
    with quiet():
        res = rmtExe(mi)
    d = res["resModel"][0]
    out = {k: np.array(d[k], dtype=float) for k in
           ("dataYs", "dataYCons1", "dataYCons2", "dataYTemp1", "dataYTemp2", "dataXs")}
    out["wall"] = np.array(time.time() - t0)
    # a few direct RHS probes of modelEquationN1
    box = {}

    def fake(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
        box["IV"] = np.array(y0, float)
        box["params"] = args[0]
        raise _Captured()
    PBH.solve_ivp = fake
    try:
        with quiet():
            try:
                rmtExe(mi)
            except _Captured:
                pass
    finally:
        PBH.solve_ivp = REAL_SOLVE_IVP
    IV = box["IV"]
    ys = [IV, d["dataYCons1"][:, 50].tolist() + [d["dataYs"][6, 50]/5e6, d["dataYTemp1"][50]],
          d["dataYCons1"][:, 100].tolist() + [d["dataYs"][6, 100]/5e6, d["dataYTemp1"][100]]]
    ys = np.array([np.array(y, float) for y in ys])
    with quiet():
        fs = np.array([PB.modelEquationN1(0.37, y, box["params"]) for y in ys])
    out["rhs_y"] = ys
    out["rhs_f"] = fs
    np.savez_compressed(os.path.join(GOLD, "g6_n1.npz"), **out)
    print("G6 written")


# --------------------------------------------------------------------------- G7
def g_helpers():
    from PyREMOT.docs.rmtThermo import (calHeatCapacityAtConstantPressure,
                                        calMeanHeatCapacityAtConstantPressure,
                                        calMixtureHeatCapacityAtConstantPressure,
                                        calStandardEnthalpyOfReaction,
                                        calEnthalpyChangeOfReaction)
    from PyREMOT.docs.gasTransPor import calGasViscosity, calMixturePropertyM1
    from PyREMOT.docs.rmtUtility import rmtUtilityClass as U
    from PyREMOT.data import componentSymbolList, componentDataStore
    comps = list(componentSymbolList)
    out = {"components": comps, "MW": [c["MW"] for c in componentDataStore["payload"]],
           "dHf25": [c["dHf25"]["val"] for c in componentDataStore["payload"]], "probes": []}
    mf = np.arange(1, len(comps) + 1, dtype=float)
    mf = mf/mf.sum()
    MW = np.array(out["MW"])
    for T in (298.15, 400.0, 523.0, 700.0, 973.0):
        cp = calHeatCapacityAtConstantPressure(comps, T)
        cpm = calMeanHeatCapacityAtConstantPressure(comps, T)
        vis = calGasViscosity(comps, T)
        out["probes"].append({
            "T": T, "Cp": cp.tolist(), "CpMean": cpm.tolist(),
            "CpMix": float(calMixtureHeatCapacityAtConstantPressure(mf, cpm)),
            "GaVii": vis.tolist(),
            "GaMiVi": float(calMixturePropertyM1(len(comps), vis, mf, MW)),
        })
    out["molefrac"] = mf.tolist()
    rx = dict(INP.SYN12_REACTIONS)
    rls = U.buildReactionCoefficient(rx)
    out["reactions"] = rx
    out["reactionListSorted"] = tolist(rls)
    out["reactionStochCoeff"] = tolist(U.buildReactionCoeffVector(rls))
    out["StHeRe25"] = [float(calStandardEnthalpyOfReaction(r)) for r in rx.values()]
    out["EnChList_600"] = [float(v) for v in calEnthalpyChangeOfReaction(rls, 600.0)]
    with open(os.path.join(GOLD, "g7_helpers.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("G7 written")


# --------------------------------------------------------------------------- G9 (model M2)
def m2_capture(mi, zNo):
    """rmtExe(model M2) up to the first solve_ivp call (pbReactor.py:719): IV and the args tuple."""
    import PyREMOT.docs.pbReactor as PBR
    box = {}

    def fake(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
        box["IV"] = np.array(y0, dtype=float)
        box["args"] = args
        box["fun"] = fun
        raise _Captured()

    PBR.solve_ivp = fake
    try:
        with mesh(zNo, model="S2"), quiet():
            try:
                rmtExe(mi)
            except _Captured:
                pass
    finally:
        PBR.solve_ivp = REAL_SOLVE_IVP
    return box["IV"], box["args"], box["fun"]


def m2_states(IV, V, N, seed):
    """dimensional test states: rows C_i [kmol/m^3], last row T [K]"""
    rng = np.random.default_rng(seed)
    Y0 = IV.reshape(V, N)
    z = np.linspace(0, 1, N)
    s1 = Y0.copy()
    for i in range(V - 1):
        s1[i] = Y0[i]*(1.0 + 0.15*np.sin(2.0*np.pi*(z + 0.1*i))) + 0.003*(i + 1)*z*Y0[0]
    s1[V - 1] = Y0[V - 1] + 12.0*z + 4.0*np.sin(3*np.pi*z)
    s2 = np.abs(Y0*(1 + 0.05*rng.standard_normal(Y0.shape))) + 1e-4*rng.random(Y0.shape)*Y0[0]
    s2[V - 1] = Y0[V - 1] + 15.0*rng.random(N) - 3.0
    s3 = s1.copy()
    idx = rng.integers(0, N, size=max(2, N//10))
    s3[2, idx] = -1e-3*rng.random(len(idx))
    s3[4, idx[::2]] = 0.0
    s3[0, idx[1::2]] = -5e-2
    return [s.flatten() for s in (s1, s2, s3)]


def g_m2():
    out, setup = {}, {}
    mi = INP.m2_dme_input()
    for zNo in (20, 100, 1024):
        IV, args, fun = m2_capture(mi, zNo)
        rls, rsc, FunParam = args
        V = FunParam["const"]["varNo"]
        if zNo == 20:
            setup = {"const": tolist(FunParam["const"]), "constBC1": tolist(FunParam["constBC1"]),
                     "ExHe": tolist(FunParam["ExHe"]), "ReSpec": tolist(FunParam["ReSpec"]),
                     "IV": IV.tolist()}
        states = [IV] + m2_states(IV, V, zNo, seed=zNo + 2)
        if zNo == 1024:
            states = states[:2]
        Y = np.array(states)
        t0 = time.time()
        with quiet():
            F = np.array([np.array(fun(0.0, y, *args), dtype=float) for y in Y])
        print("G9 M2 zNo=%d: %d RHS calls in %.1fs" % (zNo, len(Y), time.time() - t0))
        out["rhs_%d_y" % zNo] = Y
        out["rhs_%d_f" % zNo] = F
    # the reference's own RK4 on the M2 RHS (odeSolver.py:17-40), zNo=20, 100 steps of 1e-6 s
    IV, args, fun = m2_capture(mi, 20)
    with quiet():
        traj = ODES.RK4(0.0, 100*1e-6, 100, IV, lambda t, y, p: fun(t, y, *p), args)
    out["rk4_20_traj"] = np.array(traj, dtype=float)[:, ::10]
    out["rk4_20_h"] = np.array(1e-6)
    np.savez_compressed(os.path.join(GOLD, "g9_m2.npz"), **out)
    with open(os.path.join(GOLD, "g9_m2_setup.json"), "w") as f:
        json.dump(setup, f, indent=1)
    print("G9 written")


def g_m2_run(zNo=20, tNo=2, rtol=1e-10, atol=1e-13, method="LSODA"):
    """rmtExe(model M2) end to end with tolerances injected at the solve_ivp call site; the
    reference returns plot lists only (pbReactor.py:835-840), so the end state of every output
    interval is recorded at the call site."""
    import PyREMOT.docs.pbReactor as PBR
    mi = INP.m2_dme_input(ivp=method)
    ends, nfev = [], [0]

    def wrapped(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
        sol = REAL_SOLVE_IVP(fun, t_span, y0, method=method, t_eval=t_eval, args=args,
                             rtol=rtol, atol=atol)
        ends.append((float(t_span[1]), np.array(sol.y[:, -1], dtype=float)))
        nfev[0] += sol.nfev
        return sol

    PBR.solve_ivp = wrapped
    t0 = time.time()
    try:
        with mesh(zNo, tNo, model="S2"), quiet():
            res = rmtExe(mi)
    finally:
        PBR.solve_ivp = REAL_SOLVE_IVP
    np.savez_compressed(os.path.join(GOLD, "g9_m2_tight_%s.npz" % method.lower()),
                        zNo=zNo, tNo=tNo, rtol=rtol, atol=atol, nfev=nfev[0], wall_s=time.time() - t0,
                        times=np.array([t for t, _ in ends]), states=np.array([y for _, y in ends]),
                        last_leg=np.array([d["leg"] for d in res["resModel"]["dataList"]]),
                        last_y=np.array([d["y"] for d in res["resModel"]["dataList"]], dtype=float))
    print("G9 M2 tight run: nfev=%d wall=%.0fs" % (nfev[0], time.time() - t0))


# --------------------------------------------------------------------------- G10 (plot/export layer)
def synthetic_respack():
    """small resPack of the runN2 schema (pbHomoReactor.py:3664-3696); deterministic numbers"""
    S, N, tNo = 3, 6, 5
    xs = np.linspace(0, 1, N)
    packs = []
    for k in range(tNo):
        ys = np.array([[0.1*(i + 1) + 0.01*k + 0.001*j for j in range(N)] for i in range(S)] +
                      [[500.0 + k + 0.5*j for j in range(N)]])
        packs.append({"modelId": "N2", "processType": "non-iso-thermal", "successStatus": True,
                      "dataShape": (S + 1, N), "labelList": ["A", "B", "C", "Temperature"],
                      "indexList": [S, S + 1, S], "dataTime": 0.1*(k + 1), "dataXs": xs, "dataYs": ys})
    return {"computation-time": 1.234, "dataPack": packs}, tNo


def g_plot():
    import tempfile
    import PyREMOT.solvers.solResultAnalysis as SRA
    from PyREMOT.core.utilities import selectRandomForList, selectFromListByIndex
    from PyREMOT.library.saveResult import saveResultClass as sRes
    out = {"picks": {}}
    for seed in (0, 1, 7, 1234):
        np.random.seed(seed)
        out["picks"][str(seed)] = [int(v) for v in selectRandomForList(list(range(5)), 2)]
    np.random.seed(3)
    out["picks10"] = [int(v) for v in selectRandomForList(list(range(10)), 2)]
    out["select"] = [selectFromListByIndex([], [1, 2, 3]), selectFromListByIndex([2, 0], [1, 2, 3])]
    figs = []
    real = SRA.pltc.plots2D
    SRA.pltc.plots2D = staticmethod(lambda data, xLabel, yLabel, title="": figs.append(
        {"title": title, "xlabel": xLabel, "ylabel": yLabel,
         "lines": [{"leg": d["leg"], "x": tolist(d["x"]), "y": tolist(d["y"])} for d in
                   (data if isinstance(data, list) else [data])]}))
    try:
        resPack, tNo = synthetic_respack()
        np.random.seed(11)
        SRA.plotResultsDynamic(resPack, tNo)
        out["dynamic"] = list(figs)
        figs.clear()
        d = dict(resPack["dataPack"][0])
        d.update({"modelId": "N1", "computation-time": 0.5, "labelList": ["A", "B", "C", "Pressure", "Temperature"],
                  "indexList": [3, 3, 4], "dataYs": np.vstack([d["dataYs"][:3], np.linspace(50, 49, 6), d["dataYs"][3:]])})
        SRA.plotResultsSteadyState([d])
        out["steady"] = list(figs)
    finally:
        SRA.pltc.plots2D = real
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            sRes.saveListToText([1.5, "abc", [1, 2], np.float64(2.25)])
            sRes.saveListToCSV([[1, 2.5, "x"], [3, 4.0, "y,z"]], ["a", "b", "c"])
            out["txt"] = open("saveFile.txt", newline="").read()
            out["csv"] = open("saveFile.csv", newline="").read()
        finally:
            os.chdir(cwd)
    with open(os.path.join(GOLD, "g10_plot_export.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("G10 written")


def g_model_setting():
    """G11: what the reference does when MODEL_SETTING['GaMaCoTe0'] is not "MAX" (the per-species scaling branch of
    pbHomoReactor.py:3461-3463 / :3901-3904 / :3159-3160 and solResultAnalysis.py:285-288).  Recorded, not assumed:
    rmtExe is run end to end for N2 and N1 (zNo = 20) with the setting mutated, and for M2 (which never reads it);
    the outcome - exception type and message, or success - is the fixture the device build is held to."""
    import PyREMOT.docs.modelSetting as MS
    out = {"setting": "FIX", "reference": "PyREMOT %s" % getattr(PyREMOT, "__version__", "1.0.17")}
    cases = {"N2": (INP.dme_notebook_input(period=0.01), "N2"), "N1": (INP.n1_notebook_input(), "N1"),
             "M2": (INP.m2_dme_input(period=0.01), "S2")}
    old = MS.MODEL_SETTING["GaMaCoTe0"]
    MS.MODEL_SETTING["GaMaCoTe0"] = "FIX"            # the one dict object every module imported
    try:
        for name, (mi, key) in cases.items():
            try:
                with mesh(20, 2, key) if key != "N1" else mesh(20, None, key), quiet():
                    rmtExe(mi)
                out[name] = {"raises": None}
            except Exception as e:                   # noqa: BLE001 - the outcome IS the fixture
                out[name] = {"raises": type(e).__name__, "message": str(e)}
        # N1 runs under "FIX" (per-species scale SpCoi0[i], GaMaCoTe0[i] = (vf/zf) SpCoi0[i], while the initial
        # values stay SpCoi0[i]/max(SpCoi0), pbHomoReactor.py:2819-2834, 3159-3162): record its profile and RHS probes
        mi = INP.n1_notebook_input()
        with quiet():
            d = rmtExe(mi)["resModel"][0]
        prof = {k: np.array(d[k], dtype=float) for k in
                ("dataYs", "dataYCons1", "dataYCons2", "dataYTemp1", "dataYTemp2", "dataXs")}
        box = {}

        def fake(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
            box["IV"] = np.array(y0, float)
            box["params"] = args[0]
            raise _Captured()
        PBH.solve_ivp = fake
        try:
            with quiet():
                try:
                    rmtExe(mi)
                except _Captured:
                    pass
        finally:
            PBH.solve_ivp = REAL_SOLVE_IVP
        ys = [box["IV"], d["dataYCons1"][:, 50].tolist() + [d["dataYs"][6, 50]/5e6, d["dataYTemp1"][50]],
              d["dataYCons1"][:, 100].tolist() + [d["dataYs"][6, 100]/5e6, d["dataYTemp1"][100]]]
        ys = np.array([np.array(y, float) for y in ys])
        with quiet():
            prof["rhs_f"] = np.array([PB.modelEquationN1(0.37, y, box["params"]) for y in ys])
        prof["rhs_y"] = ys
        np.savez_compressed(os.path.join(GOLD, "g11_n1_fix.npz"), **prof)
    finally:
        MS.MODEL_SETTING["GaMaCoTe0"] = old
    with open(os.path.join(GOLD, "g11_model_setting.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(out)


# --------------------------------------------------------------------------- G12 (steady models M7 / M1)
def steady_solve(mi, method=None, rtol=None, atol=None):
    """rmtExe of a steady packed-bed model (runM3 for "M7", runM1 for "M1", pbReactor.py:141-352, 1170-1369) with the
    solve_ivp call recorded: IV, the args tuple, the model function and sol.t / sol.y."""
    import PyREMOT.docs.pbReactor as PBR
    box = {"nfev": 0}

    def wrapped(fun, t_span, y0, method=None, t_eval=None, args=None, **kw):
        box.update(IV=np.array(y0, dtype=float), args=args, fun=fun)
        if rtol is not None:
            kw["rtol"] = rtol
        if atol is not None:
            kw["atol"] = atol
        sol = REAL_SOLVE_IVP(fun, t_span, y0, method=method, t_eval=t_eval, args=args, **kw)
        box.update(t=np.array(sol.t, dtype=float), y=np.array(sol.y, dtype=float))
        box["nfev"] += sol.nfev
        return sol

    if method is not None:
        mi = dict(mi)
        mi["solver-config"] = dict(mi["solver-config"], ivp=method)
    PBR.solve_ivp = wrapped
    t0 = time.time()
    try:
        with quiet():
            res = rmtExe(mi)
    finally:
        PBR.solve_ivp = REAL_SOLVE_IVP
    box["wall"] = time.time() - t0
    return res, box


def steady_states(IV, Y, model):
    """Model-function probes: the feed, three states of the run, one hot perturbed state, one with a species near
    1e-12 of the total.  Returns (states, near_equilibrium flags)."""
    S = len(IV) - (2 if model == "M7" else 3)
    n = Y.shape[1]
    ys = [IV.copy(), Y[:, 2].copy(), Y[:, n//2].copy(), Y[:, -1].copy()]
    hot = Y[:, n//3].copy()
    hot[:S] *= 1.0 + 0.05*np.sin(np.arange(S) + 1.0)
    hot[S + (0 if model == "M7" else 1)] += 40.0          # T + 40 K
    hot[-1] *= 0.97                                       # P - 3 %
    ys.append(hot)
    tiny = Y[:, 1].copy()
    tiny[S - 1] = 1e-12*np.sum(tiny[:S])                  # last species (DME) at 1e-12 of the total
    ys.append(tiny)
    # the three run states sit close to the equilibria of methanol synthesis and dehydration (R1, R3): the rates of
    # H2O, CH3OH, DME and the heat of reaction are differences of nearly equal terms (golden tolerance 1e-7, not 1e-11)
    equil = np.array([False, True, True, True, False, False])
    return np.array(ys), equil


def g_steady(model):
    import inputs_steady as INS
    mi = INS.STEADY_INPUTS[(model, "dme")]()
    res, box = steady_solve(mi)
    rls, rsc, FunParam = box["args"]
    setup = {"IV": box["IV"].tolist(), "const": tolist(FunParam["const"]), "ReSpec": tolist(FunParam["ReSpec"]),
             "ExHe": tolist(FunParam["ExHe"]), "constBC1": tolist(FunParam.get("constBC1", {})),
             "t_eval": box["t"].tolist()}
    states, equil = steady_states(box["IV"], box["y"], model)
    with quiet():
        F = np.array([np.array(box["fun"](0.3, y, *box["args"]), dtype=float) for y in states])
    rm = res["resModel"]
    out = {"rhs_y": states, "rhs_f": F, "rhs_equil": equil,
           "default_dataYs": np.array(rm["dataYs"], dtype=float),
           "default_x": np.array([xy[0] for xy in rm["XYList"]], dtype=float),
           "default_XY_y": np.array([xy[1] for xy in rm["XYList"]], dtype=float),
           "default_dataList_y": np.array([d["y"] for d in rm["dataList"]], dtype=float),
           "default_legends": np.array([d["leg"] for d in rm["dataList"]]),
           "default_sol_y": box["y"], "default_nfev": np.array(box["nfev"]), "default_wall": np.array(box["wall"])}
    # the accuracy reference: LSODA at rtol 1e-11, atol 1e-13 of each variable's own scale
    S = len(mi["feed"]["components"]["shell"])
    IV = box["IV"]
    scale = np.abs(IV).copy()
    scale[:S] = np.sum(np.abs(IV[:S]))
    res_t, box_t = steady_solve(mi, "LSODA", 1e-11, 1e-13*scale)
    rt = res_t["resModel"]
    out.update(tight_dataYs=np.array(rt["dataYs"], dtype=float),
               tight_XY_y=np.array([xy[1] for xy in rt["XYList"]], dtype=float),
               tight_sol_y=box_t["y"], tight_nfev=np.array(box_t["nfev"]), tight_wall=np.array(box_t["wall"]))
    name = "g12_%s" % model.lower()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    with open(os.path.join(GOLD, name + "_setup.json"), "w") as f:
        json.dump(setup, f, indent=1)
    print("G12 %s: default nfev=%d (%.2fs), tight nfev=%d (%.2fs)" % (
        model, box["nfev"], box["wall"], box_t["nfev"], box_t["wall"]))


# --------------------------------------------------------------------------- G13
# Time-varying inlet / coolant conditions (solver-config "schedule", rmt_app_amd/schedule.py).  The cases are written to
# g13_schedule.json and read from there by the tests; nothing of the product is imported here: the piecewise-linear
# functions are restated below.
def _sched_abs(times, T=None, P=None, Tm=None):
    return {"time": times, "inlet-temperature": T, "inlet-pressure": P, "medium-temperature": Tm}


G13_STEP = lambda ts: {"time": [0.0, ts, ts, 0.4], "inlet-temperature": [523.0, 523.0, 528.0, 528.0],     # noqa: E731
                       "inlet-pressure": [5.0e6, 5.0e6, 4.9e6, 4.9e6], "medium-temperature": [523.0, 523.0, 533.0, 533.0]}
G13_CASES = {
    "A": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "schedule": G13_STEP(0.2)},
    "A1": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 4, "schedule": G13_STEP(0.23)},
    "B": {"input": "dme_nb", "zNo": 20, "period": 0.3, "tNo": 6,
          "schedule": {"time": [0.0, 0.1, 0.2, 0.3], "inlet-temperature": [523.0, 523.0, 533.0, 533.0],
                       "medium-temperature": [523.0, 523.0, 531.0, 531.0]}},
    "C": {"input": "dme_nb", "zNo": 600, "period": 0.06, "tNo": 3, "method": "DOP853",
          "schedule": {"time": [0.0, 0.02, 0.04, 0.06], "inlet-temperature": [523.0, 523.0, 533.0, 533.0],
                       "medium-temperature": [523.0, 523.0, 531.0, 531.0]}},
    "D": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "members": [0, 15, 31],
          "ensemble": {"temperature": [513.0, 516.0, 519.0, 522.0, 525.0, 528.0, 531.0, 534.0],
                       "pressure": [4.0e6, 4.5e6, 5.0e6, 5.5e6]},
          "schedule": {"time": [0.0, 0.2, 0.2, 0.4], "inlet-temperature": [0.0, 0.0, 5.0, 5.0],
                       "inlet-pressure": [0.0, 0.0, -1.0e5, -1.0e5], "medium-temperature": [0.0, 0.0, 10.0, 10.0],
                       "relative": True}},
}
G13_KEYS = (("inlet-temperature", "T0"), ("inlet-pressure", "P0"), ("medium-temperature", "Tm"))


def _pw_piece(times, vals, a, b):
    """(value at a, slope) of the linear piece of the schedule that holds over (a, b) - no breakpoint inside."""
    T = np.asarray(times, dtype=float)
    k = int(np.searchsorted(T, 0.5*(a + b), side="right")) - 1
    if k >= len(T) - 1:
        return float(vals[-1]), 0.0
    s = (vals[k + 1] - vals[k])/(T[k + 1] - T[k])
    return float(vals[k] + s*(a - T[k])), float(s)


def _pw_right(times, vals, t):
    """value at t; at a jump the one that holds from t on."""
    T = np.asarray(times, dtype=float)
    k = int(np.searchsorted(T, t, side="right")) - 1
    if k >= len(T) - 1:
        return float(vals[-1])
    return float(vals[k] + (vals[k + 1] - vals[k])*(t - T[k])/(T[k + 1] - T[k]))


def _g13_member_input(case, member=None):
    mi = INP.ALL_N2_INPUTS[case["input"]](period=case["period"])
    if member is None:
        return mi
    Ts, Ps = case["ensemble"]["temperature"], case["ensemble"]["pressure"]
    T, P = Ts[member//len(Ps)], Ps[member % len(Ps)]
    c0 = np.asarray(mi["feed"]["concentration"], dtype=float)
    mi["operating-conditions"].update({"temperature": float(T), "pressure": float(P)})
    mi["feed"]["concentration"] = (c0/c0.sum())*float(P)/(8.314472*float(T))       # the sweep rule of the ensemble API
    return mi


def g13_trajectory(case, member=None, rtol=1e-10, atol=1e-13):
    """Whole states at the output times: SciPy on the oracle's vectorised RHS with T0, P0 and Tm as functions of t,
    restarted at every breakpoint."""
    from oracle import n2_oracle as O
    mi = _g13_member_input(case, member)
    pr = dict(O.setup_n2(mi, zNo=case["zNo"]))
    f = O.make_rhs_vec(pr)
    sch = case["schedule"]
    own = {"T0": pr["T0"], "P0": pr["P0"], "Tm": pr["Tm"]}
    vals = {}
    for key, name in G13_KEYS:
        if sch.get(key) is not None:
            v = np.asarray(sch[key], dtype=float)
            vals[name] = own[name] + v if sch.get("relative") else v
    out_t = np.linspace(0.0, case["period"], case["tNo"] + 1)
    marks = sorted(set(out_t.tolist()) | {b for b in sch["time"] if 0 < b < case["period"]
                                          and np.min(np.abs(out_t - b)) > 1e-12*case["period"]})
    y = np.array(pr["IV"], dtype=float)
    states, nfev = [], 0
    method = case.get("method", "LSODA")
    for a, b in zip(marks[:-1], marks[1:]):
        piece = {name: _pw_piece(sch["time"], v, a, b) for name, v in vals.items()}

        def ft(t, yy, piece=piece, a=a):
            for name, (v0, s) in piece.items():
                pr[name] = v0 + s*(t - a)
            return f(t, yy)
        t0 = time.time()
        sol = REAL_SOLVE_IVP(ft, (a, b), y, method=method, rtol=rtol, atol=atol)
        if not sol.success:
            raise RuntimeError(sol.message)
        y = sol.y[:, -1]
        nfev += sol.nfev
        print("G13 %s%s: (%.4f, %.4f) nfev=%d %.0f s" % (case.get("name", ""), "" if member is None else " member %d" % member,
                                                          a, b, sol.nfev, time.time() - t0), flush=True)
        if np.min(np.abs(out_t - b)) <= 1e-12*case["period"]:
            states.append(y.copy())
    return out_t[1:], np.array(states), nfev


def g13_probes():
    """The reference's own modelEquationN2 with only constBC1['T0'], constBC1['P0'] and ExHe['MeTe'] replaced by the
    forced values: five times of schedule B and two of schedule A (the pressure step), six states each."""
    import copy
    mi = INP.dme_notebook_input()
    IV, params = capture(mi, 20)
    V = params[2]["const"]["varNo"]
    Y = np.array([IV] + synthetic_states(IV, V, 20, seed=13) + synthetic_states(IV, V, 20, seed=131)[:2])
    assert len(Y) == 6
    probes = [("B", t) for t in (0.0, 0.1, 0.15, 0.2, 0.3)] + [("A", t) for t in (0.1, 0.2)]
    forced, F = [], []
    for name, t in probes:
        sch = G13_CASES[name]["schedule"]
        v = {"T0": 523.0, "P0": 5.0e6, "Tm": 523.0}
        for key, nm in G13_KEYS:
            if sch.get(key) is not None:
                v[nm] = _pw_right(sch["time"], sch[key], t)
        p2 = list(params)
        p2[2] = copy.deepcopy(params[2])
        p2[2]["constBC1"]["T0"] = v["T0"]
        p2[2]["constBC1"]["P0"] = v["P0"]
        p2[2]["ExHe"]["MeTe"] = v["Tm"]
        forced.append([v["T0"], v["P0"], v["Tm"]])
        F.append([rhs(tuple(p2), y) for y in Y])
    np.savez_compressed(os.path.join(GOLD, "g13_schedule_probes.npz"), y=Y, f=np.array(F), forced=np.array(forced),
                        times=np.array([t for _, t in probes]), case=np.array([n for n, _ in probes]))
    print("G13 probes written")


def g_schedule(which=None):
    with open(os.path.join(GOLD, "g13_schedule.json"), "w") as f:
        json.dump({"cases": G13_CASES, "rtol": 1e-10, "atol": 1e-13,
                   "reference": "SciPy LSODA (case C: DOP853) on oracle.n2_oracle.make_rhs_vec, restarted at breakpoints"},
                  f, indent=1)
    todo = [which] if which else ["probes", "A", "A1", "B", "C", "D"]
    for name in todo:
        if name == "probes":
            g13_probes()
            continue
        case = dict(G13_CASES[name], name=name)
        out = {}
        t0 = time.time()
        if "members" in case:
            for m in case["members"]:
                times, states, nfev = g13_trajectory(case, m)
                out["states_%d" % m] = states
        else:
            times, states, nfev = g13_trajectory(case)
            out["states"] = states
        np.savez_compressed(os.path.join(GOLD, "g13_schedule_%s.npz" % name), times=times, nfev=nfev,
                            wall_s=time.time() - t0, **out)
        print("G13 %s written (%.0f s)" % (name, time.time() - t0))


# --------------------------------------------------------------------------- G14
# Time-varying feed composition (solver-config "schedule", key "inlet-concentration").  Every disturbance keeps H2, the
# largest feed concentration, fixed: the reference takes its scaling from max(constBC1['SpCoi0']) (pbHomoReactor.py:3901,
# 4090), so only then is "replace constBC1['SpCoi0']" the same model as a boundary value that moves under a fixed
# scaling.  The cases are written to g14_feed.json; nothing of the product is imported, the piecewise-linear functions
# are restated (vector-valued) below.
G14_FEED = [574.8978, 287.4489, 0.0115, 287.4489, 0.0115, 0.0115]       # dme_nb: H2, CO2, H2O, CO, CH3OH, DME
G14_NEW = [574.8978, 250.0, 0.0115, 324.8978, 0.0115, 0.0115]           # CO2 -37.4489, CO +37.4489
G14_STEP = lambda ts: {"time": [0.0, ts, ts, 0.4], "inlet-concentration": [G14_FEED, G14_FEED, G14_NEW, G14_NEW]}  # noqa: E731
G14_CASES = {
    "FA": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "schedule": G14_STEP(0.2)},
    "FA1": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 4, "schedule": G14_STEP(0.23)},
    "FB": {"input": "dme_nb", "zNo": 20, "period": 0.3, "tNo": 6,
           "schedule": {"time": [0.0, 0.1, 0.2, 0.3], "inlet-concentration": [G14_FEED, G14_FEED, G14_NEW, G14_NEW],
                        "inlet-temperature": [523.0, 523.0, 533.0, 533.0]}},
    "FC": {"input": "dme_nb", "zNo": 600, "period": 0.06, "tNo": 3, "method": "DOP853",
           "schedule": {"time": [0.0, 0.02, 0.04, 0.06], "inlet-concentration": [G14_FEED, G14_FEED, G14_NEW, G14_NEW]}},
    "FD": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "members": [0, 15, 31],
           "ensemble": {"temperature": [513.0, 516.0, 519.0, 522.0, 525.0, 528.0, 531.0, 534.0],
                        "pressure": [4.0e6, 4.5e6, 5.0e6, 5.5e6]},
           "schedule": {"time": [0.0, 0.2, 0.2, 0.4], "relative": True,
                        "inlet-concentration": [[0.0]*6, [0.0]*6, [0.0, -30.0, 0.0, 30.0, 0.0, 0.0],
                                                [0.0, -30.0, 0.0, 30.0, 0.0, 0.0]]}},
}


def _pwv_piece(times, vals, a, b):
    """(values at a, slopes) of the linear piece that holds over (a, b); vals [K] or [K][S]."""
    T = np.asarray(times, dtype=float)
    vals = np.asarray(vals, dtype=float)
    k = int(np.searchsorted(T, 0.5*(a + b), side="right")) - 1
    if k >= len(T) - 1:
        return vals[-1].copy(), np.zeros_like(vals[-1])
    s = (vals[k + 1] - vals[k])/(T[k + 1] - T[k])
    return vals[k] + s*(a - T[k]), s


def _pwv_right(times, vals, t):
    """values at t; at a jump the ones that hold from t on; vals [K] or [K][S]."""
    T = np.asarray(times, dtype=float)
    vals = np.asarray(vals, dtype=float)
    k = int(np.searchsorted(T, t, side="right")) - 1
    if k >= len(T) - 1:
        return vals[-1].copy()
    return vals[k] + (vals[k + 1] - vals[k])*(t - T[k])/(T[k + 1] - T[k])


def g14_trajectory(case, member=None, rtol=1e-10, atol=1e-13):
    """Whole states at the output times: SciPy on the oracle's vectorised RHS with SpCoi0 (and T0, P0, Tm where the case
    schedules them) as functions of t, restarted at every breakpoint.  The oracle's scaling is max(SpCoi0), which no case
    moves (asserted)."""
    from oracle import n2_oracle as O
    mi = _g13_member_input(case, member)
    pr = dict(O.setup_n2(mi, zNo=case["zNo"]))
    f = O.make_rhs_vec(pr)
    sch = case["schedule"]
    own = {"T0": pr["T0"], "P0": pr["P0"], "Tm": pr["Tm"], "SpCoi0": np.array(pr["SpCoi0"], dtype=float)}
    cmax = float(np.max(own["SpCoi0"]))
    vals = {}
    for key, name in G13_KEYS + (("inlet-concentration", "SpCoi0"),):
        if sch.get(key) is not None:
            v = np.asarray(sch[key], dtype=float)
            vals[name] = own[name] + v if sch.get("relative") else v
    assert np.all(np.max(vals["SpCoi0"], axis=1) == cmax), "the disturbance must leave max(SpCoi0) unchanged"
    out_t = np.linspace(0.0, case["period"], case["tNo"] + 1)
    marks = sorted(set(out_t.tolist()) | {b for b in sch["time"] if 0 < b < case["period"]
                                          and np.min(np.abs(out_t - b)) > 1e-12*case["period"]})
    y = np.array(pr["IV"], dtype=float)
    states, nfev = [], 0
    method = case.get("method", "LSODA")
    for a, b in zip(marks[:-1], marks[1:]):
        piece = {name: _pwv_piece(sch["time"], v, a, b) for name, v in vals.items()}

        def ft(t, yy, piece=piece, a=a):
            for name, (v0, s) in piece.items():
                pr[name] = v0 + s*(t - a)
            return f(t, yy)
        t0 = time.time()
        sol = REAL_SOLVE_IVP(ft, (a, b), y, method=method, rtol=rtol, atol=atol)
        if not sol.success:
            raise RuntimeError(sol.message)
        y = sol.y[:, -1]
        nfev += sol.nfev
        print("G14 %s%s: (%.4f, %.4f) nfev=%d %.0f s" % (case.get("name", ""), "" if member is None else " member %d" % member,
                                                          a, b, sol.nfev, time.time() - t0), flush=True)
        if np.min(np.abs(out_t - b)) <= 1e-12*case["period"]:
            states.append(y.copy())
    return out_t[1:], np.array(states), nfev


def g14_probes():
    """The reference's own modelEquationN2 with only constBC1['SpCoi0'] replaced by the forced composition (one probe
    also with constBC1['T0']): before, inside (two times) and after the ramp of schedule FB, and before and behind the
    step of schedule FA; the six G13 probe states each."""
    import copy
    mi = INP.dme_notebook_input()
    IV, params = capture(mi, 20)
    V = params[2]["const"]["varNo"]
    Y = np.array([IV] + synthetic_states(IV, V, 20, seed=13) + synthetic_states(IV, V, 20, seed=131)[:2])
    assert len(Y) == 6
    probes = [("FB", t) for t in (0.05, 0.125, 0.15, 0.25)] + [("FA", t) for t in (0.1, 0.2)]
    conc, forced, F = [], [], []
    for name, t in probes:
        sch = G14_CASES[name]["schedule"]
        v = {"T0": 523.0, "P0": 5.0e6, "Tm": 523.0}
        for key, nm in G13_KEYS:
            if sch.get(key) is not None:
                v[nm] = float(_pwv_right(sch["time"], sch[key], t))
        c = _pwv_right(sch["time"], sch["inlet-concentration"], t)
        p2 = list(params)
        p2[2] = copy.deepcopy(params[2])
        p2[2]["constBC1"]["SpCoi0"] = np.array(c, dtype=float)
        p2[2]["constBC1"]["T0"] = v["T0"]
        p2[2]["constBC1"]["P0"] = v["P0"]
        p2[2]["ExHe"]["MeTe"] = v["Tm"]
        conc.append(c)
        forced.append([v["T0"], v["P0"], v["Tm"]])
        F.append([rhs(tuple(p2), y) for y in Y])
    np.savez_compressed(os.path.join(GOLD, "g14_feed_probes.npz"), y=Y, f=np.array(F), conc=np.array(conc),
                        forced=np.array(forced), times=np.array([t for _, t in probes]),
                        case=np.array([n for n, _ in probes]))
    print("G14 probes written")


def g_feed(which=None):
    with open(os.path.join(GOLD, "g14_feed.json"), "w") as f:
        json.dump({"cases": G14_CASES, "rtol": 1e-10, "atol": 1e-13,
                   "reference": "SciPy LSODA (case FC: DOP853) on oracle.n2_oracle.make_rhs_vec with SpCoi0(t), restarted "
                                "at breakpoints; max(SpCoi0) stays fixed"}, f, indent=1)
    todo = [which] if which else ["probes", "FA", "FA1", "FB", "FC", "FD"]
    for name in todo:
        if name == "probes":
            g14_probes()
            continue
        case = dict(G14_CASES[name], name=name)
        out = {}
        t0 = time.time()
        if "members" in case:
            for m in case["members"]:
                times, states, nfev = g14_trajectory(case, m)
                out["states_%d" % m] = states
        else:
            times, states, nfev = g14_trajectory(case)
            out["states"] = states
        np.savez_compressed(os.path.join(GOLD, "g14_feed_%s.npz" % name), times=times, nfev=nfev,
                            wall_s=time.time() - t0, **out)
        print("G14 %s written (%.0f s)" % (name, time.time() - t0))


# --------------------------------------------------------------------------- G15
# Closed-loop runs (solver-config "control", rmt_app_amd/control.py): a sampled PI controller moves the inlet pressure.
# SciPy on the oracle's RHS with pr["T0"], pr["P0"], pr["Tm"] (and pr["SpCoi0"]) set per call, restarted at every sample
# time and breakpoint; the control law, the sample times and the setpoint are restated here - nothing of the product is
# imported.  The cases are written to g15_control.json; each .npz holds the states at the output times and the log
# (t_k, pv_k, r_k, u_k, saturated).
G15_SP_STEP = {"time": [0.0, 0.25, 0.25, 0.4], "value": [621.0, 621.0, 620.0, 620.0]}
G15_PI = {"measured": "outlet-temperature", "manipulated": "inlet-pressure", "setpoint": G15_SP_STEP, "sample-time": 0.01,
          "start": 0.1, "gain": 5.0e4, "integral-time": 0.05, "limits": [4.0e6, 6.0e6]}
G15_CASES = {
    "CA": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 4,
           "schedule": {"time": [0.0, 0.2, 0.2, 0.4], "medium-temperature": [523.0, 523.0, 533.0, 533.0]},
           "control": dict(G15_PI)},
    "CB": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 4,
           "schedule": {"time": [0.0, 0.2, 0.2, 0.4], "medium-temperature": [523.0, 523.0, 533.0, 533.0]},
           # (setpoint 622.2 -> 621.2 instead of CA's 621 -> 620: with CA's the output sat at the lower limit for the whole run
           # and the rerun at rtol 1e-12 missed the 1e-9 condition; with 622.5 -> 621.5 only two samples saturated,
           # profiles/control.md)
           "control": dict(G15_PI, limits=[4.95e6, 5.05e6],
                           setpoint={"time": [0.0, 0.25, 0.25, 0.4], "value": [622.2, 622.2, 621.2, 621.2]})},
    # (in the first 0.06 s the bed heats up from the feed temperature and the hottest node is the outlet: the setpoint ramp
    # runs a few K ahead of the open-loop peak, 524.5 K at t = 0.01 .. 564.5 K at t = 0.05)
    "CC": {"input": "dme_nb", "zNo": 600, "period": 0.06, "tNo": 3, "method": "DOP853",
           "schedule": {"time": [0.0, 0.02, 0.04, 0.06], "medium-temperature": [523.0, 523.0, 531.0, 531.0],
                        "inlet-concentration": [G14_FEED, G14_FEED, G14_NEW, G14_NEW]},
           "control": {"measured": "peak-temperature", "manipulated": "inlet-pressure",
                       "setpoint": {"time": [0.0, 0.06], "value": [520.0, 580.0]}, "sample-time": 0.01, "start": 0.01,
                       "gain": 5.0e4, "integral-time": 0.05, "limits": [4.0e6, 6.0e6]}},
    # (the gain is filled in by g15_cd_gain: half the inverse of the generator's own open-loop step response)
    "CD": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "members": [0, 3],
           "ensemble": {"temperature": [518.0, 528.0], "pressure": [4.8e6, 5.2e6]},
           "control": {"measured": {"outlet-mole-fraction": "DME"}, "manipulated": "inlet-pressure", "setpoint": 0.0150,
                       "sample-time": 0.02, "start": 0.1, "gain": None, "integral-time": 0.05, "limits": [4.0e6, 6.0e6]}},
}
G15_SHELL = ["H2", "CO2", "H2O", "CO", "CH3OH", "DME"]       # dme_nb's shell components
G15_LOOSEST_BOUND = 1e-6                                     # the loosest bound of tests/test_gpu_control.py


def _g15_setpoint(sp, t, tol):
    if not isinstance(sp, dict):
        return float(sp)
    T, v = np.asarray(sp["time"], dtype=float), np.asarray(sp["value"], dtype=float)
    j = int(np.argmin(np.abs(T - t)))
    if abs(T[j] - t) <= tol:
        t = float(T[j])
    k = int(np.searchsorted(T, t, side="right")) - 1
    if k >= len(T) - 1:
        return float(v[-1])
    return float(v[k] + (v[k + 1] - v[k])*(t - T[k])/(T[k + 1] - T[k]))


def _g15_measure(ctl, y, S, N, Tf):
    Y = np.asarray(y, dtype=float).reshape(S + 1, N)
    m = ctl["measured"]
    if m == "outlet-temperature":
        return float(Y[S, N - 1]*Tf + Tf)
    if m == "peak-temperature":
        return float(np.max(Y[S])*Tf + Tf)
    s = G15_SHELL.index(m["outlet-mole-fraction"])
    tot = 0.0
    for i in range(S):
        tot += float(Y[i, N - 1])
    return float(Y[s, N - 1])/tot


def g15_trajectory(case, member=None, rtol=1e-10, atol=1e-13, gain=None, step=None, t_stop=None, quiet_run=False):
    """Closed loop: whole states at the output times and the log [K][5] = (t_k, pv_k, r_k, u_k, saturated).
    ``gain``: replaces the case's (0.0: the open loop on the same restarts); ``step`` = (t_s, dP): no controller, the inlet
    pressure steps by dP at sample time t_s (the open-loop step response); ``t_stop``: stop there."""
    from oracle import n2_oracle as O
    mi = _g13_member_input(case, member)
    pr = dict(O.setup_n2(mi, zNo=case["zNo"]))
    f = O.make_rhs_vec(pr)
    S, N, Tf = pr["compNo"], case["zNo"], float(pr["Tf"])
    sch = case.get("schedule") or {"time": [0.0]}
    ctl = case["control"]
    assert ctl["manipulated"] == "inlet-pressure"
    own = {"T0": pr["T0"], "P0": pr["P0"], "Tm": pr["Tm"], "SpCoi0": np.array(pr["SpCoi0"], dtype=float)}
    vals = {}
    for key, name in G13_KEYS + (("inlet-concentration", "SpCoi0"),):
        if sch.get(key) is not None:
            vals[name] = np.asarray(sch[key], dtype=float)
    assert "P0" not in vals
    if "SpCoi0" in vals:
        assert np.all(np.max(vals["SpCoi0"], axis=1) == float(np.max(own["SpCoi0"])))
    period = float(case["period"])
    tol = 1e-12*period
    out_t = np.linspace(0.0, period, case["tNo"] + 1)
    marks = sorted(set(out_t.tolist()) | {b for b in sch["time"] if 0 < b < period and np.min(np.abs(out_t - b)) > tol})
    Ts, start = float(ctl["sample-time"]), float(ctl.get("start", 0.0))
    samples, k = [], 0
    while start + k*Ts < period - tol:
        t = start + k*Ts
        j = int(np.argmin(np.abs(np.array(marks) - t)))
        samples.append(marks[j] if abs(marks[j] - t) <= tol else t)      # a sample at a mark IS that mark
        k += 1
    marks = sorted(set(marks) | set(samples))
    Kp = float((ctl["gain"] or 0.0) if gain is None else gain)      # (None: case CD before g15_cd_gain, step runs only)
    Ti = ctl.get("integral-time")
    Ki = 0.0 if Ti is None else Kp*Ts/float(Ti)
    lo, hi = (float(x) for x in ctl["limits"])
    u0 = float(own["P0"])
    I, u = 0.0, u0
    y = np.array(pr["IV"], dtype=float)
    states, log = [], []
    method = case.get("method", "LSODA")
    for a, b in zip(marks[:-1], marks[1:]):
        if t_stop is not None and a >= t_stop - tol:
            break
        if a in samples:
            pv = _g15_measure(ctl, y, S, N, Tf)
            r = _g15_setpoint(ctl["setpoint"], a, tol)
            if step is None:
                # the law: one rounded fp64 operation each, in this order
                e = r - pv
                Ip = I + Ki*e if Ki != 0.0 else I
                v = (u0 + Kp*e) + Ip
                u = lo if v < lo else v
                u = hi if u > hi else u
                if v == u:
                    I = Ip
                log.append([a, pv, r, u, float(v != u)])
            else:
                if abs(a - step[0]) <= tol:
                    u = u0 + step[1]
                log.append([a, pv, r, u, 0.0])
        piece = {name: _pwv_piece(sch["time"], v, a, b) for name, v in vals.items()}
        pr["P0"] = u

        def ft(t, yy, piece=piece, a=a):
            for name, (v0, s) in piece.items():
                pr[name] = v0 + s*(t - a)
            return f(t, yy)
        t0 = time.time()
        sol = REAL_SOLVE_IVP(ft, (a, b), y, method=method, rtol=rtol, atol=atol)
        if not sol.success:
            raise RuntimeError(sol.message)
        y = sol.y[:, -1]
        if not quiet_run:
            print("G15 %s%s: (%.4f, %.4f) u=%.6e nfev=%d %.0f s" % (
                case.get("name", ""), "" if member is None else " member %d" % member, a, b, u, sol.nfev,
                time.time() - t0), flush=True)
        if np.min(np.abs(out_t - b)) <= tol:
            states.append(y.copy())
    return out_t[1:len(states) + 1], np.array(states), np.array(log)


def _g15_state_difference(A, B, S, Tf):
    """max over nodes and output times of |d mole fraction| and |dT|/T between two sets of states [K][V*N]"""
    d = 0.0
    for a, b in zip(A, B):
        a, b = a.reshape(S + 1, -1), b.reshape(S + 1, -1)
        xa, xb = a[:S]/np.sum(a[:S], axis=0), b[:S]/np.sum(b[:S], axis=0)
        Ta, Tb = a[S]*Tf + Tf, b[S]*Tf + Tf
        d = max(d, float(np.max(np.abs(xa - xb))), float(np.max(np.abs(Ta - Tb)/Tb)))
    return d


def g15_cd_gain():
    """Case CD's gain from the open-loop step of member 0: the inlet pressure steps by +1e5 Pa at the first sample time,
    the outlet mole fraction of DME one sample later against the run without the step; Kp = 0.5/(dx/dP), two digits."""
    case = dict(G15_CASES["CD"], name="CD-step")
    ctl = case["control"]
    t1 = ctl["start"] + ctl["sample-time"]
    _, _, with_step = g15_trajectory(case, 0, step=(ctl["start"], 1.0e5), t_stop=t1 + ctl["sample-time"], quiet_run=True)
    _, _, without = g15_trajectory(case, 0, step=(ctl["start"], 0.0), t_stop=t1 + ctl["sample-time"], quiet_run=True)
    dx = with_step[1, 1] - without[1, 1]
    g = dx/1.0e5
    Kp = float("%.1e" % (0.5/g))
    print("G15 CD open-loop step: x_DME %.9e -> %.9e one sample after +1e5 Pa: dx/dP = %.4e 1/Pa, gain = %.1e Pa"
          % (without[1, 1], with_step[1, 1], g, Kp))
    return Kp


def g15_case(name):
    case = dict(G15_CASES[name], name=name)
    case["control"] = dict(case["control"])
    if case["control"]["gain"] is None:
        case["control"]["gain"] = g15_cd_gain()
    return case


def g_control(which=None):
    """``control`` writes the case file and every case; ``control=json`` the case file alone, ``control=<case>`` one case."""
    if which in (None, "json"):
        cases = {n: {k: v for k, v in g15_case(n).items() if k != "name"} for n in G15_CASES}
        with open(os.path.join(GOLD, "g15_control.json"), "w") as f:
            json.dump({"cases": cases, "rtol": 1e-10, "atol": 1e-13,
                       "reference": "SciPy LSODA (case CC: DOP853) on oracle.n2_oracle.make_rhs_vec, restarted at every "
                                    "sample time and breakpoint; the control law restated in tools/make_golden.py"},
                      f, indent=1)
        if which == "json":
            return
    for name in ([which] if which else list(G15_CASES)):
        case = g15_case(name)
        ctl = case["control"]
        lo, hi = ctl["limits"]
        S = 6
        out = {}
        t0 = time.time()
        for m in case.get("members", [None]):
            tag = "" if m is None else "_%d" % m
            times, states, log = g15_trajectory(case, m)
            Tf = float(_g13_member_input(case, m)["operating-conditions"]["temperature"])
            u, sat = log[:, 3], log[:, 4] != 0
            print("G15 %s%s: u in [%.6e, %.6e], moves by %.4e Pa, %d of %d samples saturated, pv %.6f .. %.6f" % (
                name, tag, u.min(), u.max(), u.max() - u.min(), int(sat.sum()), len(u), log[:, 1].min(), log[:, 1].max()))
            if name == "CA":
                assert not sat.any() and u.min() > lo and u.max() < hi, "CA: u touches a limit"
                assert u.max() - u.min() >= 1.0e4, "CA: u moves by less than 1e4 Pa"
            if name == "CB":
                assert int(sat.sum()) >= 3, "CB: fewer than three saturated samples"
            _, open_states, _ = g15_trajectory(case, m, gain=0.0, quiet_run=True)
            d_open = _g15_state_difference(states, open_states, S, Tf)
            print("G15 %s%s: closed loop against gain = 0: %.4e (needs >= %.1e)" % (name, tag, d_open, 100*G15_LOOSEST_BOUND))
            assert d_open >= 100*G15_LOOSEST_BOUND, "the closed loop does not differ enough from the open loop"
            _, tight, tlog = g15_trajectory(case, m, rtol=1e-12, atol=1e-15, quiet_run=True)
            # relative in the solver's own error weight: |dy| / (|y| + atol/rtol) - a component far below atol/rtol = 1e-3
            # is held to the absolute tolerance only, its own relative change says nothing about convergence
            d_tol = float(np.max(np.abs(tight - states)/(np.abs(states) + 1e-13/1e-10)))
            d_abs = _g15_state_difference(states, tight, S, Tf)
            print("G15 %s%s: rerun at rtol 1e-12: relative %.4e, in the tests' measure %.4e, u %.4e relative" % (
                name, tag, d_tol, d_abs, float(np.max(np.abs(tlog[:, 3] - u)/u))))
            assert d_tol < 1e-9, "the golden states are not converged to 1e-9 relative"
            out["states" + tag], out["log" + tag] = states, log
        np.savez_compressed(os.path.join(GOLD, "g15_control_%s.npz" % name), times=times, wall_s=time.time() - t0, **out)
        print("G15 %s written (%.0f s)" % (name, time.time() - t0))


# ------------------------------------------------------------------ G17: discrete steady states of model N2
# (solver-config "initial": "steady", rmt_app_amd/initial.py).  SciPy on the oracle's vectorised RHS: the transient from
# the reference's cold start until max|f| stops falling, then a polish of f(y) = 0 on the full system.  Nothing of the
# product is imported.  The isothermal ch4 case relaxes far more slowly (2.5e-2 after 10 s) and is not a golden.
G17_CASES = {"dme_script": {"input": "dme_script", "zNo": 20}, "dme_nb": {"input": "dme_nb", "zNo": 20},
             "syn12": {"input": "syn12", "zNo": 20}}
G17_GATE = 1e-9          # a case whose final max|f| under the oracle RHS exceeds this is not written
G17_CHUNK = 10.0         # simulated seconds per LSODA leg
G17_T_MAX = 400.0


def g17_state(case, rtol=1e-10, atol=1e-13):
    """(state [V*N], max|f| reached, simulated time used, residual after LSODA alone)"""
    import scipy.optimize
    from oracle import n2_oracle as O
    pr = O.setup_n2(INP.ALL_N2_INPUTS[case["input"]](), zNo=case["zNo"])
    f = O.make_rhs_vec(pr)
    y, t, prev = np.array(pr["IV"], dtype=float), 0.0, np.inf
    while t < G17_T_MAX:
        t0 = time.time()
        sol = REAL_SOLVE_IVP(f, (t, t + G17_CHUNK), y, method="LSODA", rtol=rtol, atol=atol)
        if not sol.success:
            raise RuntimeError(sol.message)
        y, t = sol.y[:, -1], t + G17_CHUNK
        r = float(np.max(np.abs(f(t, y))))
        print("G17 %s: t = %.0f s max|f| = %.3e nfev=%d %.0f s" % (case["input"], t, r, sol.nfev, time.time() - t0), flush=True)
        if not r < 0.5*prev:            # stopped falling
            break
        prev = r
    r_ode = float(np.max(np.abs(f(t, y))))
    best, r_best = y, r_ode
    sol = scipy.optimize.root(lambda v: f(0.0, v), y)        # (the default method, MINPACK's hybrd, with its default tolerance)
    r = float(np.max(np.abs(f(0.0, sol.x))))
    print("G17 %s: root max|f| = %.3e" % (case["input"], r), flush=True)
    if np.all(np.isfinite(sol.x)) and r < r_best:          # (a polish that does not lower max|f| leaves the transient's state)
        best, r_best = np.array(sol.x, dtype=float), r
    return best, r_best, t, r_ode


def g_steady_state(which=None):
    path = os.path.join(GOLD, "g17_steady.json")
    meta = {"cases": {}, "gate": G17_GATE, "rtol": 1e-10, "atol": 1e-13,
            "reference": "SciPy LSODA on oracle.n2_oracle.make_rhs_vec from the oracle's IV until max|f| stops falling, "
                         "then scipy.optimize.root on the full system"}
    if which and os.path.exists(path):
        with open(path) as fh:
            meta["cases"] = json.load(fh)["cases"]
    for name in ([which] if which else list(G17_CASES)):
        case = G17_CASES[name]
        y, r, t, r_ode = g17_state(case)
        if not r <= G17_GATE:
            raise SystemExit("G17 %s: max|f| = %.3e under the oracle RHS exceeds the gate %.1e - not written" % (name, r, G17_GATE))
        np.savez_compressed(os.path.join(GOLD, "g17_steady_%s.npz" % name), state=y, residual=r)
        meta["cases"][name] = dict(case, residual=r, time=t, residual_lsoda=r_ode)
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G17 %s written: max|f| = %.3e after %.0f s (LSODA alone %.3e)" % (name, r, t, r_ode), flush=True)


# ------------------------------------------------------------------ G18: axial profiles of model N2
# (solver-config "axial-profile", rmt_app_amd/profile.py): catalyst activity a(z) on every reaction rate, coolant
# temperature Tm(z) in the wall term.  The oracle does not change: the activity wraps every entry of pr["RATES"] in a
# closure (vectorised_kinetics rebinds the user lambda through the closure cell and broadcasts the node array), and the
# coolant uses that the right-hand side is affine in Tm - pr["Tm"] must stay a scalar (make_local_rhs tests pr["Tm"] == 0)
# - so f(Tm(z)) = f0 + (f1 - f0) delta(z) on the temperature row, f0 / f1 evaluated at MeTe and MeTe + 1.  Against
# rhs_loop node by node with scalar a_z and Tm(z_n) the two agree to 2.1e-15 relative (DME, 20 nodes).  Nothing of the
# product is imported: the node rule (z_n = n/(N-1), right-continuous at a repeated position) is restated below.
G18_BED_A = {"position": [0.0, 0.3, 0.3, 0.5, 0.5, 1.0], "catalyst-activity": [0.4, 0.4, 1.0, 1.0, 1.0, 1.0],
             "medium-temperature": [533.0, 533.0, 533.0, 533.0, 513.0, 513.0]}
G18_CASES = {
    "A": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "axial-profile": G18_BED_A},
    "B": {"input": "dme_nb", "process-type": "iso-thermal", "zNo": 20, "period": 0.4, "tNo": 2,
          "axial-profile": {"position": [0.0, 0.5, 1.0], "catalyst-activity": [0.0, 1.0, 1.0]}},
    "C": {"input": "dme_nb", "zNo": 600, "period": 0.06, "tNo": 3, "method": "DOP853",
          "axial-profile": {"position": [0.0, 0.4, 0.4, 1.0], "catalyst-activity": [0.5, 0.5, 1.0, 1.0],
                            "medium-temperature": [533.0, 525.0, 525.0, 513.0]}},
    "AS": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2, "axial-profile": G18_BED_A,
           "schedule": {"time": [0.0, 0.2, 0.2, 0.4], "medium-temperature": [523.0, 523.0, 533.0, 533.0]}},
    "A0": {"input": "dme_nb", "zNo": 20, "period": 0.4, "tNo": 2},                         # the plain twin of A
    "C0": {"input": "dme_nb", "zNo": 600, "period": 0.06, "tNo": 3, "method": "DOP853"},   # the plain twin of C
    "S": {"input": "dme_nb", "zNo": 20, "axial-profile": G18_BED_A, "steady": True},
}


def g18_nodes(position, values, N):
    """the piecewise-linear function at z_n = n/(N-1): right-continuous at a jump, the last value at z = 1"""
    p, v = np.asarray(position, dtype=float), np.asarray(values, dtype=float)
    out = np.zeros(N)
    for n in range(N):
        z = n/float(N - 1)
        k = int(np.searchsorted(p, z, side="right")) - 1
        out[n] = v[-1] if k >= len(p) - 1 else v[k] + (v[k + 1] - v[k])*(z - p[k])/(p[k + 1] - p[k])
    return out


def g18_profiled_pr(pr, a):
    """pr with every rate multiplied by the node array a [N]"""
    def wrap(f, a):
        return lambda x: a*f(x)
    out = dict(pr)
    out["RATES"] = {k: wrap(f, a) for k, f in pr["RATES"].items()}
    return out


def g18_profiled_rhs(O, pr, a, delta):
    """(f(t, y), the two parameter dicts whose "Tm" a schedule moves together) of the profiled bed"""
    p0 = g18_profiled_pr(pr, np.asarray(a, dtype=float))
    p1 = dict(p0)
    f0, f1 = O.make_rhs_vec(p0), O.make_rhs_vec(p1)
    S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
    delta = np.asarray(delta, dtype=float)
    if pr["iso"] or pr["Tm"] == 0 or not np.any(delta != 0):
        return f0, (p0,)

    def f(t, y):
        p1["Tm"] = p0["Tm"] + 1.0
        r0 = np.array(f0(t, y), dtype=float)
        r1 = np.asarray(f1(t, y), dtype=float)
        R0, R1 = r0.reshape((-1, V, N)), r1.reshape((-1, V, N))
        R0[:, S, :] += (R1[:, S, :] - R0[:, S, :])*delta
        return r0
    return f, (p0,)


def _g18_input(case):
    kw = {"period": case["period"]} if "period" in case else {}
    if "process-type" in case:
        kw["process_type"] = case["process-type"]
    return INP.ALL_N2_INPUTS[case["input"]](**kw)


def _g18_bed(case, pr):
    N = case["zNo"]
    spec = case.get("axial-profile") or {}
    a = g18_nodes(spec["position"], spec["catalyst-activity"], N) if "catalyst-activity" in spec else np.ones(N)
    d = g18_nodes(spec["position"], spec["medium-temperature"], N) - pr["Tm"] if "medium-temperature" in spec else np.zeros(N)
    return a, d


def g18_trajectory(case, rtol=1e-10, atol=1e-13):
    """Whole states at the output times (the G13 recipe on the profiled RHS; a "schedule" moves the common coolant level)"""
    from oracle import n2_oracle as O
    pr = dict(O.setup_n2(_g18_input(case), zNo=case["zNo"]))
    a, d = _g18_bed(case, pr)
    f, moved = g18_profiled_rhs(O, pr, a, d)
    sch = case.get("schedule")
    out_t = np.linspace(0.0, case["period"], case["tNo"] + 1)
    marks = sorted(set(out_t.tolist()) | ({b for b in sch["time"] if 0 < b < case["period"]
                                           and np.min(np.abs(out_t - b)) > 1e-12*case["period"]} if sch else set()))
    y = np.array(pr["IV"], dtype=float)
    states, nfev = [], 0
    for lo, hi in zip(marks[:-1], marks[1:]):
        piece = _pw_piece(sch["time"], np.asarray(sch["medium-temperature"], dtype=float), lo, hi) if sch else None

        def ft(t, yy, piece=piece, lo=lo):
            if piece is not None:
                for p in moved:
                    p["Tm"] = piece[0] + piece[1]*(t - lo)
            return f(t, yy)
        t0 = time.time()
        sol = REAL_SOLVE_IVP(ft, (lo, hi), y, method=case.get("method", "LSODA"), rtol=rtol, atol=atol)
        if not sol.success:
            raise RuntimeError(sol.message)
        y = sol.y[:, -1]
        nfev += sol.nfev
        print("G18 %s: (%.4f, %.4f) nfev=%d %.0f s" % (case.get("name", ""), lo, hi, sol.nfev, time.time() - t0), flush=True)
        if np.min(np.abs(out_t - hi)) <= 1e-12*case["period"]:
            states.append(y.copy())
    return out_t[1:], np.array(states), nfev


def g18_steady(case, rtol=1e-10, atol=1e-13):
    """the recipe of g17_state on the profiled RHS"""
    import scipy.optimize
    from oracle import n2_oracle as O
    pr = dict(O.setup_n2(_g18_input(case), zNo=case["zNo"]))
    a, d = _g18_bed(case, pr)
    f, _ = g18_profiled_rhs(O, pr, a, d)
    y, t, prev = np.array(pr["IV"], dtype=float), 0.0, np.inf
    while t < G17_T_MAX:
        t0 = time.time()
        sol = REAL_SOLVE_IVP(f, (t, t + G17_CHUNK), y, method="LSODA", rtol=rtol, atol=atol)
        if not sol.success:
            raise RuntimeError(sol.message)
        y, t = sol.y[:, -1], t + G17_CHUNK
        r = float(np.max(np.abs(f(t, y))))
        print("G18 S: t = %.0f s max|f| = %.3e nfev=%d %.0f s" % (t, r, sol.nfev, time.time() - t0), flush=True)
        if not r < 0.5*prev:
            break
        prev = r
    r_ode = float(np.max(np.abs(f(t, y))))
    best, r_best = y, r_ode
    sol = scipy.optimize.root(lambda v: f(0.0, v), y)
    r = float(np.max(np.abs(f(0.0, sol.x))))
    print("G18 S: root max|f| = %.3e" % r, flush=True)
    if np.all(np.isfinite(sol.x)) and r < r_best:
        best, r_best = np.array(sol.x, dtype=float), r
    return best, r_best, t, r_ode


def g_profile(which=None):
    path = os.path.join(GOLD, "g18_profile.json")
    meta = {"cases": G18_CASES, "rtol": 1e-10, "atol": 1e-13, "gate": G17_GATE, "steady": {},
            "reference": "SciPy LSODA (cases C, C0: DOP853) on oracle.n2_oracle.make_rhs_vec with the rates wrapped by the "
                         "node activities and the coolant offsets through the affine dependence on Tm; case S: the recipe "
                         "of G17"}
    if os.path.exists(path):
        with open(path) as fh:
            meta["steady"] = json.load(fh).get("steady", {})
    for name in ([which] if which else list(G18_CASES)):
        case = dict(G18_CASES[name], name=name)
        t0 = time.time()
        if case.get("steady"):
            y, r, t, r_ode = g18_steady(case)
            if not r <= G17_GATE:
                raise SystemExit("G18 S: max|f| = %.3e exceeds the gate %.1e - not written" % (r, G17_GATE))
            np.savez_compressed(os.path.join(GOLD, "g18_profile_%s.npz" % name), state=y, residual=r)
            meta["steady"] = {"residual": r, "time": t, "residual_lsoda": r_ode}
        else:
            times, states, nfev = g18_trajectory(case)
            np.savez_compressed(os.path.join(GOLD, "g18_profile_%s.npz" % name), times=times, nfev=nfev,
                                wall_s=time.time() - t0, states=states)
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G18 %s written (%.0f s)" % (name, time.time() - t0), flush=True)


# ------------------------------------------------------------------ G19: time-on-stream runs with catalyst deactivation
# (solver-config "deactivation", rmt_app_amd/campaign.py).  The oracle does not change and nothing of the product is
# imported: tests/campaign_ref.py restates the law in numpy and finds every steady state with scipy.optimize.root on the
# profiled right-hand side of G18, started from the previous step's state (above the gate of G17: LSODA legs first).
def g_campaign(which=None):
    import campaign_ref as CR
    from oracle import n2_oracle as O
    path = os.path.join(GOLD, "g19_campaign.json")
    meta = {"cases": {}, "gate": CR.GATE,
            "reference": "per step scipy.optimize.root on profile_ref.profiled_rhs from the previous step's state (above the "
                         "gate: the recipe of G17 - LSODA legs from the cold start until max|f| stops falling, then root), the activity moved by the frozen-temperature "
                         "exact solution of the law in numpy (tests/campaign_ref.py)"}
    if os.path.exists(path):
        with open(path) as fh:
            meta["cases"] = json.load(fh)["cases"]
    for name in ([which] if which else list(CR.CASES)):
        case = CR.CASES[name]
        t0 = time.time()
        out = CR.run_case(O, INP, case, log=lambda msg: print("G19 %s: %s" % (name, msg), flush=True))
        np.savez_compressed(os.path.join(GOLD, "g19_campaign_%s.npz" % name), times=out["times"], marks=out["marks"],
                            activity=out["activity"], states=out["states"], residual=out["residual"], delta=out["delta"])
        if os.path.exists(path):
            with open(path) as fh:
                meta["cases"] = json.load(fh)["cases"]
        meta["cases"][name] = dict(case, residual=float(out["residual"].max()), lsoda_steps=int(np.sum(out["legs"] > 0)),
                                   activity_end=[float(out["activity"][-1].min()), float(out["activity"][-1].max())])
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G19 %s written (%.0f s): max|f| <= %.3e, activity ends at %.4f .. %.4f" % (
            name, time.time() - t0, out["residual"].max(), out["activity"][-1].min(), out["activity"][-1].max()), flush=True)


# ------------------------------------------------------------------ G20: the coolant policy of a time-on-stream run
# (solver-config "deactivation" "policy").  tests/policy_ref.py: per step scipy.optimize.brentq on r(T) = x_c,outlet(T) -
# target, every value a steady state of the profiled right-hand side of G18 with the uniform coolant offset T - MeTe, the
# saturation rule restated, the law of G19.  A case is refused (SystemExit) when a steady state ends above the gate of G17,
# when r at 9 equidistant levels changes sign more than once in a step, or when two adjacent samples differ by more than
# 20 x the median difference.
def g_policy(which=None):
    import policy_ref as PO
    from oracle import n2_oracle as O
    path = os.path.join(GOLD, "g20_policy.json")
    meta = {"cases": {}, "gate": PO.CR.GATE, "xtol": PO.XTOL, "samples": PO.SAMPLES, "jump": PO.JUMP,
            "reference": "per step scipy.optimize.brentq (xtol 1e-10 K) on r(T) = x_c,outlet(T) - target within the limits, "
                         "every value a steady state of profile_ref.profiled_rhs with the uniform coolant offset T - MeTe "
                         "(campaign_ref.steady_state from the nearest known state), no sign change between the limits: the "
                         "limit with the smaller |r| (a tie: lo); the activity moved by campaign_ref.law_update "
                         "(tests/policy_ref.py)"}
    for name in ([which] if which else list(PO.CASES)):
        case = PO.CASES[name]
        t0 = time.time()
        out = PO.run_case(O, INP, case, log=lambda msg: print("G20 %s: %s" % (name, msg), flush=True))
        np.savez_compressed(os.path.join(GOLD, "g20_policy_%s.npz" % name), times=out["times"], marks=out["marks"],
                            activity=out["activity"], states=out["states"], level=out["level"], held=out["held"],
                            saturated=out["saturated"], sample_levels=out["sample_levels"], samples=out["samples"],
                            residual=out["residual"], delta=out["delta"])
        if os.path.exists(path):           # (read again: the cases may be made by several processes)
            with open(path) as fh:
                meta["cases"] = json.load(fh)["cases"]
        meta["cases"][name] = dict(case, residual=float(out["residual"].max()), level=[float(v) for v in out["level"]],
                                   saturated=[int(v) for v in out["saturated"]])
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G20 %s written (%.0f s): levels %s, saturated %s" % (name, time.time() - t0, out["level"], out["saturated"]),
              flush=True)


# ------------------------------------------------------------------ G21: parametric sensitivities of the N2 steady state
# (solver-config "sensitivity", rmt_app_amd/sensitivity.py).  tests/sens_ref.py: Richardson-extrapolated central differences
# of steady states of the oracle's right-hand side with ONE value moved, each found by the recipe and under the gate of
# G17 / G18; nothing of the product is imported.  The step starts at 1e-4 |p| (a concentration: 1e-4 of the largest feed
# concentration); a case whose fd_error = max|D(d/2) - D(d)| exceeds 1e-5 of a row's largest magnitude is refused
# (SystemExit) - move the step of that parameter within [1e-5, 1e-3] |p| (G21_DELTAS), not the cap.
G21_DELTAS = {}          # case -> {parameter label: relative step}; empty: every parameter at sens_ref.DELTA0


def g_sensitivity(which=None):
    import sens_ref as SR
    from oracle import n2_oracle as O
    path = os.path.join(GOLD, "g21_sensitivity.json")
    meta = {"cases": {}, "gate": SR.CR.GATE, "fd_cap": SR.FD_CAP,
            "reference": "central differences at d and d/2 of steady states of oracle.n2_oracle.make_rhs_vec (bed A: "
                         "profile_ref.profiled_rhs) with one value moved, each from campaign_ref.steady_state and a Newton "
                         "polish, D = (4 D(d/2) - D(d))/3, fd_error = max|D(d/2) - D(d)| per (parameter, row) "
                         "(tests/sens_ref.py)"}
    for name in ([which] if which else list(SR.CASES)):
        for rel in G21_DELTAS.get(name, {}).values():
            assert 1e-5 <= rel <= 1e-3
        t0 = time.time()
        out = SR.run_case(O, INP, name, G21_DELTAS.get(name), log=lambda msg: print("G21 %s" % msg, flush=True))
        bad = SR.refused(out)
        if bad:
            raise SystemExit("G21 %s: fd_error exceeds %.0e of the row's largest magnitude in (parameter, row) %s - not written"
                             % (name, SR.FD_CAP, bad))
        np.savez_compressed(os.path.join(GOLD, "g21_sensitivity_%s.npz" % name), state=out["state"], rows=out["rows"],
                            values=out["values"], delta=out["delta"], D=out["D"], fd_error=out["fd_error"])
        if os.path.exists(path):
            with open(path) as fh:
                meta["cases"] = json.load(fh)["cases"]
        mag = np.max(np.abs(out["D"]), axis=2)
        rel = np.where(mag > 0, out["fd_error"]/np.where(mag > 0, mag, 1.0), 0.0)
        meta["cases"][name] = dict(SR.CASES[name], labels=[SR.label(p) for p in SR.CASES[name]["parameters"]],
                                   values=[float(v) for v in out["values"]], delta=[float(v) for v in out["delta"]],
                                   residual=float(out["residual"]), fd_error_relative=float(rel.max()))
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G21 %s written (%.0f s): steps %s, worst fd_error / max|row| %.2e, worst max|f| %.2e"
              % (name, time.time() - t0, out["delta"], rel.max(), out["residual"]), flush=True)


# ------------------------------------------------------------------ G22: kinetic parameter estimation from steady-state data
# (solver-config "fit", rmt_app_amd/fit.py).  tests/fit_ref.py: data from steady states of the oracle at p_true (the recipe
# and the gate of G17), the fit by scipy.optimize.least_squares with central differences of those steady states as the
# Jacobian; nothing of the product is imported.  A case is refused (SystemExit) when a steady state at the start or at
# p_true ends above the gate, when the noise-free fit misses p_true by more than 1e-7 relative, or when the
# Marquardt-scaled cond(H) at the optimum exceeds 1e8 - then widen the spread of the conditions, not the cap.
def g_fit(which=None):
    import fit_ref as FR
    from oracle import n2_oracle as O
    path = os.path.join(GOLD, "g22_fit.json")
    meta = {"cases": {}, "gate": FR.CR.GATE, "cond_cap": FR.COND_CAP, "true_cap": FR.TRUE_CAP, "zNo": FR.ZNO,
            "sigma": FR.SIGMA, "noise_seed": FR.NOISE_SEED, "p_true": FR.P_TRUE, "conditions": FR.conditions(),
            "labels": [FR.labels(e) for e in range(len(FR.conditions()))],
            "reference": "steady states of oracle.n2_oracle.make_rhs_vec from campaign_ref.steady_state (cold start) and "
                         "sens_ref.polish; scipy.optimize.least_squares (trf, x_scale 'jac', tolerances 1e-14) with "
                         "central differences (1e-4 |p|) of those steady states as the Jacobian (tests/fit_ref.py)"}
    if which in (None, "states"):
        # the experiments' steady states at p_true (the same for every case): where the CPU test of the reference starts
        ref = FR.Reference(O, FR.NAMES, log=lambda msg: print("G22 %s" % msg, flush=True))
        ref.predict(np.array([FR.P_TRUE[nm] for nm in FR.NAMES]), keep=True, gate=True)
        np.savez_compressed(os.path.join(GOLD, "g22_fit_states.npz"), states=np.array(ref.last))
        print("G22 states written: worst max|f| %.2e" % ref.worst, flush=True)
        if which == "states":
            return
    for name in ([which] if which else list(FR.CASES)):
        t0 = time.time()
        out = FR.run_case(O, name, log=lambda msg: print("G22 %s" % msg, flush=True))
        cov = out["covariance"]
        np.savez_compressed(os.path.join(GOLD, "g22_fit_%s.npz" % name), measured=out["measured"],
                            predicted_true=out["predicted_true"], p_ref=out["p_ref"],
                            p_ref_noise_free=out["p_ref_noise_free"], cost=out["cost"], hessian=out["hessian"],
                            covariance=cov if cov is not None else np.zeros((0, 0)))
        if os.path.exists(path):
            with open(path) as fh:
                meta["cases"] = json.load(fh)["cases"]
        meta["cases"][name] = dict(FR.CASES[name], p_ref=[float(v) for v in out["p_ref"]], cost=float(out["cost"]),
                                   cond=float(out["cond"]), residual=float(out["residual_gate"]))
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G22 %s written (%.0f s): p_ref %s, cost %.6e, scaled cond(H) %.3e, worst max|f| %.2e"
              % (name, time.time() - t0, out["p_ref"], out["cost"], out["cond"], out["residual_gate"]), flush=True)


# ------------------------------------------------------------------ G23: frequency response of the N2 operating point
# (solver-config "frequency-response", rmt_app_amd/frequency.py).  tests/freq_ref.py: the dense Jacobian, input columns and
# output map of the oracle's right-hand side around its steady state by Richardson-extrapolated central differences,
# G(iw) = R_y (iwI - J)^-1 B + R_p by LAPACK; nothing of the product is imported.  A case is refused (SystemExit) when
# fd_error exceeds sens_ref.FD_CAP of a row's largest magnitude, when the steady state misses the gate, when a species is
# within 10 differencing steps of the clamp, or (FA) when G(0) differs from G21's D of case SA by more than the two fd_errors.
def g_frequency(which=None):
    import freq_ref as FQ
    import sens_ref as SR
    from oracle import n2_oracle as O
    path = os.path.join(GOLD, "g23_frequency.json")
    meta = {"cases": {}, "gate": SR.CR.GATE, "fd_cap": SR.FD_CAP, "delta": FQ.DELTA0,
            "reference": "dense J, B and the output map of oracle.n2_oracle.make_rhs_vec (bed A: profile_ref.profiled_rhs) "
                         "around its steady state by central differences at d and d/2 with Richardson; G(iw) = R_y (iwI - "
                         "J)^-1 B + R_p by LAPACK; fd_error = max|G(d/2) - G(d)| per (input, row) (tests/freq_ref.py)"}
    for name in ([which] if which else list(FQ.CASES)):
        t0 = time.time()
        out = FQ.run_case(O, INP, name, log=lambda msg: print("G23 %s" % msg, flush=True))
        bad = FQ.refused(out)
        if bad:
            raise SystemExit("G23 %s: fd_error exceeds %.0e of the row's largest magnitude in (input, row) %s - not written"
                             % (name, SR.FD_CAP, bad))
        if name == "FA":          # the same bed and inputs as G21's SA: G(0) is its D
            sa = SR.golden("SA")
            diff = np.max(np.abs(out["G"][:, 0] - sa["D"]), axis=2)
            if not np.all(diff <= out["fd_error"] + sa["fd_error"]):
                raise SystemExit("G23 FA: G(0) differs from G21 SA by more than the two fd_errors: %s"
                                 % (diff/(out["fd_error"] + sa["fd_error"])))
            print("G23 FA: G(0) against G21 SA, largest part of the two fd_errors: %.3f"
                  % float(np.max(diff/(out["fd_error"] + sa["fd_error"]))), flush=True)
        np.savez_compressed(os.path.join(GOLD, "g23_frequency_%s.npz" % name), state=out["state"], rows=out["rows"],
                            values=out["values"], frequencies=out["frequencies"], G=out["G"], fd_error=out["fd_error"])
        if os.path.exists(path):
            with open(path) as fh:
                meta["cases"] = json.load(fh)["cases"]
        mag = np.max(np.abs(out["G"]), axis=(1, 3))
        rel = np.where(mag > 0, out["fd_error"]/np.where(mag > 0, mag, 1.0), 0.0)
        meta["cases"][name] = dict(FQ.CASES[name], labels=[SR.label(p) for p in FQ.CASES[name]["inputs"]],
                                   values=[float(v) for v in out["values"]],
                                   frequencies=[float(v) for v in out["frequencies"]], residual=float(out["residual"]),
                                   fd_error_relative=float(rel.max()), slowest_rate=float(out["slowest"]),
                                   convective_rate=float(out["convective"]), largest_real_part=float(out["max_real"]))
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)
        print("G23 %s written (%.0f s): worst fd_error / max|row| %.2e, max|f| %.2e"
              % (name, time.time() - t0, rel.max(), out["residual"]), flush=True)


# ------------------------------------------------------------------ G24: log-scaled and bounded parameters, data along the bed
# (solver-config "fit" with "scale", "bounds", "temperature-profile", "mole-fraction-profile").  tests/fit_ext_ref.py: FC
# and FP by scipy.optimize.least_squares with bounds= on the oracle's steady states, polished on the face the fit ends on;
# FL by the product's numpy law (fit.emulate_update_ex) on the oracle, at the lowest of fit_ext_ref.FL_FEEDS times the
# notebook's feed rate at which it reaches p_true within fit_ref.TRUE_CAP in at most 30 iterations - a candidate that does
# not is refused (SystemExit is caught per candidate, recorded under "tried", and the next one is run); fit_ext=FL:<feed>
# runs one candidate alone.  The refusals of G22 (the gate on the steady states, COND_CAP) hold.
def g_fit_ext(which=None):
    import fit_ext_ref as FX
    import fit_ref as FR
    from oracle import n2_oracle as O
    path = os.path.join(GOLD, "g24_fit_ext.json")

    def say(msg):
        print("G24 %s" % msg, flush=True)

    def record(name, entry):
        meta = {"cases": {}}
        if os.path.exists(path):
            with open(path) as fh:
                meta = json.load(fh)
        meta.update({"gate": FR.CR.GATE, "cond_cap": FR.COND_CAP, "true_cap": FR.TRUE_CAP, "zNo": FX.ZNO, "sigma": FX.SIGMA,
                     "noise_seed": FX.NOISE_SEED, "on_bound": FX.ON_BOUND, "positions": list(FX.T_POSITIONS),
                     "port": list(FX.PORT), "fl_feeds": list(FX.FL_FEEDS),
                     "reference": "tests/fit_ext_ref.py: scipy.optimize.least_squares (trf, bounds=) on steady states of "
                                  "oracle.n2_oracle, polished on the active face; FL: fit.emulate_update_ex on the oracle"})
        case = meta["cases"].setdefault(name, {})
        entry = dict(entry, tried=dict(case.get("tried", {}), **entry["tried"])) if "tried" in entry else entry
        case.update(entry)
        with open(path, "w") as fh:
            json.dump(meta, fh, indent=1)

    feed_only = None
    if which and which.startswith("FL:"):
        which, feed_only = "FL", float(which.split(":", 1)[1])
    for name in ([which] if which else ["FC", "FP", "FL"]):
        t0 = time.time()
        if name == "FL":
            tried = {}
            for feed in ([feed_only] if feed_only else FX.FL_FEEDS):
                try:
                    out = FX.run_fl(O, feed, say)
                except SystemExit as err:
                    tried["%g" % feed] = str(err)
                    say(str(err))
                    record("FL", {"tried": tried})
                    continue
                tried["%g" % feed] = "converged in %d iterations" % out["iterations"]
                np.savez_compressed(os.path.join(GOLD, "g24_fit_ext_FL.npz"), **{k: np.asarray(v) for k, v in out.items()})
                record("FL", dict(FX.CASES["FL"], tried=tried, feed=float(feed), p_ref=[float(v) for v in out["p_ref"]],
                                  iterations=int(out["iterations"]), residual=float(out["residual_gate"]),
                                  linear_law_on_the_device="does not reach p_true from this start at 40 times the "
                                                           "notebook's feed rate (profiles/fit.md)"))
                say("FL written at %gx feed (%.0f s)" % (feed, time.time() - t0))
                break
            else:
                raise SystemExit("G24 FL: no candidate of %s converged: %s" % (list(FX.FL_FEEDS), tried))
            continue
        out = FX.run_case(O, name, say)
        np.savez_compressed(os.path.join(GOLD, "g24_fit_ext_%s.npz" % name), **{k: np.asarray(v) for k, v in out.items()})
        record(name, dict(FX.CASES[name], p_ref=[float(v) for v in out["p_ref"]], active=[int(v) for v in out["active"]],
                          cost=float(out["cost"]), cond=float(out["cond"]), residual=float(out["residual_gate"]),
                          nfev=int(out["nfev"])))
        say("%s written (%.0f s): p_ref %s, active %s, cost %.6e, scaled cond(H) %.3e, worst max|f| %.2e"
            % (name, time.time() - t0, out["p_ref"], out["active"], out["cost"], out["cond"], out["residual_gate"]))


def main(argv):
    os.makedirs(GOLD, exist_ok=True)
    for what in argv:
        if what == "setup":
            g_setup()
        elif what == "rhs":
            g_rhs()
        elif what == "rk4":
            g_rk4()
        elif what.startswith("tight="):
            g_tight(what.split("=", 1)[1])
        elif what.startswith("default="):
            g_default(what.split("=", 1)[1])
        elif what == "multistep":
            g_multistep()
        elif what == "n1":
            g_n1()
        elif what == "helpers":
            g_helpers()
        elif what == "plot":
            g_plot()
        elif what == "setting":
            g_model_setting()
        elif what == "m2":
            g_m2()
        elif what in ("m7", "m1"):
            g_steady(what.upper())
        elif what == "schedule" or what.startswith("schedule="):
            g_schedule(what.split("=", 1)[1] if "=" in what else None)
        elif what == "feed" or what.startswith("feed="):
            g_feed(what.split("=", 1)[1] if "=" in what else None)
        elif what == "control" or what.startswith("control="):
            g_control(what.split("=", 1)[1] if "=" in what else None)
        elif what == "steady" or what.startswith("steady="):
            g_steady_state(what.split("=", 1)[1] if "=" in what else None)
        elif what == "profile" or what.startswith("profile="):
            g_profile(what.split("=", 1)[1] if "=" in what else None)
        elif what == "campaign" or what.startswith("campaign="):
            g_campaign(what.split("=", 1)[1] if "=" in what else None)
        elif what == "policy" or what.startswith("policy="):
            g_policy(what.split("=", 1)[1] if "=" in what else None)
        elif what == "sensitivity" or what.startswith("sensitivity="):
            g_sensitivity(what.split("=", 1)[1] if "=" in what else None)
        elif what == "fit_ext" or what.startswith("fit_ext="):
            g_fit_ext(what.split("=", 1)[1] if "=" in what else None)
        elif what == "fit" or what.startswith("fit="):
            g_fit(what.split("=", 1)[1] if "=" in what else None)
        elif what == "frequency" or what.startswith("frequency="):
            g_frequency(what.split("=", 1)[1] if "=" in what else None)
        elif what.startswith("m2run"):
            kw = dict(a.split("=") for a in what.split(":")[1:])
            g_m2_run(int(kw.get("zNo", 20)), int(kw.get("tNo", 2)), float(kw.get("rtol", 1e-10)),
                     float(kw.get("atol", 1e-13)), kw.get("method", "LSODA"))
        else:
            raise SystemExit("unknown target " + what)


if __name__ == "__main__":
    main(sys.argv[1:])
