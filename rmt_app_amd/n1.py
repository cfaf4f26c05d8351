"""Steady-state model N1 on the device: the replacement for PackedBedHomoReactorClass.runN1
(PyREMOT/docs/pbHomoReactor.py:2694-3015).  The reference integrates the S+2 unknowns
[c_i, P*, theta] along the dimensionless length with solve_ivp(LSODA) and samples
t_eval = linspace(0, 1, zNo+1) (:2931); here one launch integrates every member of an ensemble
(one reactor per lane) with the RODAS4 scheme of the N2 stiff stepper."""
from timeit import default_timer as timer

import numpy as np

from . import plan
from . import n2 as _n2
from .settings import MODEL_SETTING, ROUND_FUN_ACCURACY, solverSetting


def pack_profile(U, named, mech, modelId, elapsed):
    """dataPack entry of runN1 (pbHomoReactor.py:2947-3008; sortResult4, solResultAnalysis.py:191-249).
    U: (nout, S+2) dimensionless states."""
    S = mech.S
    Y = np.asarray(U, dtype=np.float64).T                     # (S+2, nout) like sol.y
    nout = Y.shape[1]
    conc_dl = Y[0:S, :]
    temp_dl = Y[S + 1, :] if not mech.iso else np.repeat(0, nout).reshape(nout)
    # sortResult4 (solResultAnalysis.py:226-231): species i times Cif[i] when MODEL_SETTING['GaMaCoTe0'] != "MAX"
    scale = named.get("SpCoi0_Set", named["Cmax"])
    conc = conc_dl*(np.reshape(scale, (-1, 1)) if np.ndim(scale) else scale)
    Preal = (Y[S]*named["Pf"]).reshape((1, nout))
    mofr = conc/np.sum(conc, axis=0)
    labelList = list(mech.compList) + ["Pressure"]
    parts = [mofr, Preal]
    Treal = None
    if not mech.iso:
        labelList.append("Temperature")
        Treal = (Y[S + 1]*named["Tf"] + named["Tf"]).reshape((1, nout))
        parts.append(Treal)
    dataXs = np.linspace(0, 1, nout)
    return {
        "modelId": modelId, "processType": mech.processType, "successStatus": True,
        "computation-time": elapsed, "dataShape": np.array(dataXs).shape, "labelList": labelList,
        "indexList": [S, S, S + 1], "dataTime": [], "dataXs": dataXs,
        "dataYCons1": conc_dl, "dataYCons2": conc, "dataYTemp1": temp_dl,
        "dataYTemp2": Treal if Treal is not None else np.zeros((1, nout)),
        "dataYs": np.concatenate(parts, axis=0),
    }


def run_n1(modelInput, members_inputs=None):
    """runN1 on the device; returns the reference's list with one dataPack dict (or, for an
    ensemble, a list with one dict per member)."""
    start = timer()
    cfg = modelInput['solver-config']
    displayResult = cfg['display-result'] == "True"
    zNo = int(cfg.get('zNo', solverSetting['N1']['zNo']))
    nout = zNo + 1
    # the handle is an N2 handle (same generated module); its N2 member rows are not used here.
    # MODEL_SETTING['GaMaCoTe0'] != "MAX": model N1 runs with per-species scaling in the reference (:2819, 3159)
    got = _n2.steady_profiles(
        modelInput, members_inputs, plan.member_constants_n1, nout,
        {"RMT_N1_SCALE_FIX": "1"} if MODEL_SETTING['GaMaCoTe0'] != "MAX" else None,
        handle_rows=lambda inputs, mech: np.array([plan.member_constants(mi, mech, 64)[1] for mi in inputs]))
    if got is None:
        return None
    mech, named, U, stats = got
    elapsed = np.round(timer() - start, ROUND_FUN_ACCURACY)
    packs = [pack_profile(U[e], named[e], mech, modelInput['model'], elapsed) for e in range(len(named))]
    for p, acc, rej in zip(packs, stats["accepted"], stats["rejected"]):
        p["device-stats"] = {"accepted": int(acc), "rejected": int(rej)}
    if displayResult:
        from .plotting import plotResultsSteadyState
        plotResultsSteadyState([packs[0]])                       # pbHomoReactor.py:3011-3013
    return packs if members_inputs else [packs[0]]
