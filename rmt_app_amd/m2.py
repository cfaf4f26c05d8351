"""Model "M2" on the device: the reference's DIMENSIONAL dynamic packed-bed model
(PackedBedReactorClass.runM2 / modelEquationM2, PyREMOT/docs/pbReactor.py:552-842, 845-1165;
dispatched by rmtCore.M2Init, PyREMOT/docs/rmtCore.py:239-249).  SURVEY.md section 8(f) rank 3.

Same kernel generator, same steppers and C ABI as N2 (``RMT_MODEL 2`` selects the M2 node
functions in csrc/kernels/21_node_m2.inc): concentrations in kmol/m^3, EOS gas velocity - hence a
nonlinear Ergun march, solved on the device by Newton sweeps over the affine scan - and the
catalyst's thermal mass in the energy balance.

The reference returns only plot lists from runM2 (pbReactor.py:835-840: the temperature series
of every output time); ``run_m2`` returns exactly those two keys plus ``dataPack`` (the per-interval
records the reference builds internally, :745-753), ``computation-time`` and ``device-stats``.
"""
import numpy as np

from . import plan
from .n2 import run_dynamic


def pack_interval(Yflat, mech, zNo, t_end):
    """One entry of runM2's dataPack (pbReactor.py:729-753)."""
    Y = np.reshape(Yflat, (mech.V, zNo))
    C = Y[:mech.S].copy()
    T = np.array([Y[mech.S]])
    return {"successStatus": True, "dataTime": t_end, "dataYCons": C, "dataYTemp": T,
            "dataYs": np.concatenate((C/np.sum(C, axis=0), T), axis=0)}


def result_lists(packs, ReLe, zNo, opTSpan):
    """The dict runM2 returns (pbReactor.py:806-840): after its loop over the variables the names
    XYList/dataList hold the LAST variable's (temperature's) series, one per output time, built by
    plots2DSetXYList / plots2DSetDataList (PyREMOT/library/plot.py:85-115)."""
    dataXs = np.linspace(0, ReLe, zNo)
    series = np.array([p["dataYs"][-1] for p in packs])
    XYList = [[dataXs, row] for row in series]
    dataList = [{"x": XYList[t][0], "y": XYList[t][1], "leg": "Temperature at t=" + str(opTSpan[t + 1])}
                for t in range(len(packs))]
    return {"XYList": XYList, "dataList": dataList}


def run_m2(modelInput, members_inputs=None):
    if modelInput['solver-config'].get('dtype', 'fp64') not in ('fp64', 'float64'):
        raise ValueError("model M2 is built in fp64 only")
    return run_dynamic(modelInput, members_inputs, "M2", plan.member_constants_m2, plan.initial_state_m2,
                       lambda Yg, named, mech, zNo, t1: [pack_interval(Y, mech, zNo, t1) for Y in Yg],
                       lambda dataPack, mi, zNo, opTSpan: dict(result_lists(dataPack, mi['reactor']['ReLe'], zNo, opTSpan),
                                                               dataPack=dataPack))
