"""Steady packed-bed models M7 (runM3) and M1 (runM1) on the GPU through rmtExe: the profiles against the reference's
runs recorded in golden G12 (tools/make_golden.py m7 m1), a 64 x 32 T/P sweep in one launch, the `ivp` values, and a
rate-expression domain error raised through the status word."""
import math
import os

import numpy as np
import pytest

import inputs_steady as INS
from rmt_app_amd import rmtExe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NPTS = {"M7": 30, "M1": 25}


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)/np.maximum(np.abs(b), 1e-300))


def run(model, **cfg):
    mi = INS.STEADY_INPUTS[(model, "dme")]()
    mi["solver-config"].update(cfg)
    return rmtExe(mi)["resModel"]


@pytest.mark.parametrize("model", ("M7", "M1"))
def test_profile_against_reference_runs(model):
    g = np.load(os.path.join(G, "g12_%s.npz" % model.lower()))
    res = run(model)
    n = NPTS[model]
    assert res["dataYs"].shape == (7, n)
    # the accuracy reference: LSODA at rtol 1e-11
    assert relerr(res["dataYs"], g["tight_dataYs"]) <= 1e-6, relerr(res["dataYs"], g["tight_dataYs"])
    # the reference's own default run is accurate to a few 1e-3
    assert relerr(res["dataYs"], g["default_dataYs"]) <= 5e-3
    assert relerr([xy[1] for xy in res["XYList"]], g["tight_XY_y"]) <= 1e-6
    assert len(res["XYList"]) == len(g["default_x"])
    for xy in res["XYList"]:
        assert np.array_equal(xy[0], np.linspace(0, 1, n))
    assert [d["leg"] for d in res["dataList"]] == [str(s) for s in g["default_legends"]]
    assert res["device-stats"]["accepted"] > 0
    assert "computation-time" in res


def test_tp_sweep_one_launch_matches_single_runs():
    Ts = np.linspace(503.0, 553.0, 64)
    Ps = np.linspace(3e6, 6e6, 32)
    mi = INS.m7_dme_input()
    mi["solver-config"]["ensemble"] = {"temperature": Ts.tolist(), "pressure": Ps.tolist()}
    res = rmtExe(mi)["resModel"]
    ens = res["ensemble"]
    assert len(ens) == 2048
    assert all(d["dataYs"].shape == (7, 30) for d in ens)
    for e in (0, 1000, 2047):
        T, P = Ts[e // 32], Ps[e % 32]
        one = INS.m7_dme_input()
        one["operating-conditions"].update(temperature=float(T), pressure=float(P))
        c0 = np.asarray(one["feed"]["concentration"], float)
        one["feed"]["concentration"] = c0/c0.sum()*float(P)/(8.314472*float(T))
        single = rmtExe(one)["resModel"]
        assert relerr(ens[e]["dataYs"], single["dataYs"]) <= 1e-9, e
    outlet_T = np.array([d["dataYs"][-1, -1] for d in ens]).reshape(64, 32)
    assert np.all(np.diff(outlet_T, axis=0) > 0)          # outlet T rises with feed T at every pressure


@pytest.mark.parametrize("model", ("M7", "M1"))
def test_ivp_values_select_the_same_stepper(model):
    base = run(model, ivp="default")["dataYs"]
    for ivp in ("LSODA", "BDF", "hip-ros4"):
        assert np.array_equal(run(model, ivp=ivp)["dataYs"], base), ivp


def test_rate_domain_error_raises_through_status_word():
    mi = INS.m7_dme_input()
    V = mi["reaction-rates"]["VARS"]
    V["lnT"] = lambda x: math.log(x['T'] - 530.0)          # negative argument below 530 K
    R = mi["reaction-rates"]["RATES"]
    r3 = R["r3"]
    R["r3"] = lambda x: r3(x) + 1e-30*x['lnT']
    mi["solver-config"]["ensemble"] = {"temperature": [540.0, 523.0]}
    with pytest.raises(ValueError, match="math domain error"):
        rmtExe(mi)
