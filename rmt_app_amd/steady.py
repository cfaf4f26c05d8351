"""Steady-state packed-bed models M7 and M1 on the device: the replacements for PackedBedReactorClass.runM3 (model
"M7", rmtCore.M7Init) and PackedBedReactorClass.runM1 (model "M1", rmtCore.M1Init), PyREMOT/docs/pbReactor.py:1170-1575
and :141-547.  The reference integrates [C_i, T, P] (M7) or [F_i, F*, T, P] (M1) along the bed with solve_ivp (LSODA
unless `ivp` names another SciPy method) on t_eval = linspace(0, ReLe, n); here one launch of rmt_n1_ros4 integrates
every member of an ensemble (one reactor per lane) with the RODAS4 scheme of model N1, in scaled variables along
z* = z/ReLe (layouts in csrc/kernels/23_node_steady.inc).  Every `ivp` value selects this stepper."""
from timeit import default_timer as timer

import numpy as np

from . import plan
from . import n2 as _n2
from .settings import ROUND_FUN_ACCURACY, solverSetting

SS_MODEL_DEFINE = {"M7": "7", "M1": "1"}
# the methods the reference hands to solve_ivp ("default" = LSODA, pbReactor.py:270, :1294) and the device names
STEADY_IVPS = ("default", "LSODA", "BDF", "Radau", "RK45", "RK23", "DOP853", "hip-ros4", "hip-auto")


def output_points(model, cfg):
    """runM3 samples solverSetting['M9']['zNo'] points (pbReactor.py:1283), runM1 solverSetting['S3']['timesNo']
    (:259); solver-config.zNo overrides either."""
    if 'zNo' in cfg:
        return int(cfg['zNo'])
    return int(solverSetting['M9']['zNo'] if model == "M7" else solverSetting['S3']['timesNo'])


def result_dict(Y, named, mech, model):
    """The dict runM3 / runM1 return (pbReactor.py:1300-1369, :276-352) from the solve_ivp variables Y (V1, n)."""
    S = mech.S
    n = Y.shape[1]
    dataX = np.linspace(0, named["ReLe"], n)                     # sol.t at t_eval
    dataYs1 = Y[0:S, :]
    dataYs1_MoFri = dataYs1/np.sum(dataYs1, axis=0)
    labelList = list(mech.compList)
    if model == "M7":
        labelList += ["Temperature", "Pressure"]                # :1202-1204
        _dataYs = np.concatenate((dataYs1_MoFri, [Y[S, :]]), axis=0)                        # :1321-1322
        dataYs = _dataYs
    else:
        labelList += ["Flux", "Temperature", "Pressure"]         # :166-169
        _dataYs = np.concatenate((dataYs1_MoFri, [Y[S, :]], [Y[S + 1, :]], [Y[S + 2, :]]), axis=0)   # :299-300
        dataYs = np.concatenate((dataYs1_MoFri, [Y[S + 1, :]]), axis=0)                     # :302-303
    # plots2DSetXYList / plots2DSetDataList (PyREMOT/library/plot.py:85-115): one entry per row of _dataYs
    XYList = [[dataX, item] for item in _dataYs]
    dataList = [{"x": XYList[i][0], "y": XYList[i][1], "leg": labelList[i]} for i in range(len(XYList))]
    return {"dataYs": dataYs, "XYList": XYList, "dataList": dataList}


def run_steady(model, modelInput, members_inputs=None):
    """runM3 (model "M7") or runM1 (model "M1") on the device.  Returns the reference's result dict for the base
    input (members_inputs[0] for an ensemble) plus "computation-time" and "device-stats"; an ensemble also gets
    "ensemble", one such dict per member.  The reference plots the profiles unconditionally (a blocking window,
    :1344, :325); this does not."""
    start = timer()
    cfg = modelInput['solver-config']
    if cfg.get('ivp', 'default') not in STEADY_IVPS:
        raise ValueError("`ivp` must be one of %s (got %r)" % (STEADY_IVPS, cfg.get('ivp')))
    if cfg.get('dtype', 'fp64') not in ('fp64', 'float64'):
        raise ValueError("model %s is built in fp64 only" % model)
    nout = output_points(model, cfg)
    if nout < 2:
        raise ValueError("zNo must be at least 2")
    pack = plan.member_constants_m7 if model == "M7" else plan.member_constants_m1
    got = _n2.steady_profiles(modelInput, members_inputs, pack, nout, {"RMT_SS_MODEL": SS_MODEL_DEFINE[model]},
                              extra=2 if model == "M7" else 3)
    if got is None:
        return None
    mech, named, U, stats = got
    elapsed = np.round(timer() - start, ROUND_FUN_ACCURACY)
    results = []
    for e in range(len(named)):
        Y = plan.unscale_steady(U[e], named[e], model, mech.S).T          # (V1, nout) like sol.y
        r = result_dict(Y, named[e], mech, model)
        r["computation-time"] = elapsed
        r["device-stats"] = {"accepted": int(stats["accepted"][e]), "rejected": int(stats["rejected"][e])}
        results.append(r)
    res = dict(results[0])
    if members_inputs:
        res["ensemble"] = results
    return res


def run_m7(modelInput, members_inputs=None):
    """Model M7 (rmtCore.M7Init -> PackedBedReactorClass.runM3)."""
    return run_steady("M7", modelInput, members_inputs)


def run_m1(modelInput, members_inputs=None):
    """Model M1 (rmtCore.M1Init -> PackedBedReactorClass.runM1)."""
    return run_steady("M1", modelInput, members_inputs)
