"""Model inputs of the steady-state packed-bed models M7 and M1 (data, like tests/inputs.py).

* ``m7_dme_input`` - PyREMOT/tests/test_rmt_DME3.py:25-257 (model "M7"): the DME mechanism with the
  feed built through float32 mole fractions (PyREMOT/data/initData.py:11-40), concentrations in
  mol/m^3 (``ct0*1000``), the molar flowrate from the volumetric flowrate at STP
  (rmtUtility.py:98-119) and reactor constants of PyREMOT/data/inputDataReactor.py:9-39.
* ``m1_dme_input`` - the same input under model id "M1": runM1 reads its ``mole-fraction`` and
  ``molar-flowrate`` keys (pbReactor.py:190-193).

Nothing here imports the reference.
"""
import math

import numpy as np

from inputs import DME_COMPONENTS, DME_REACTIONS_SPACED, _feed_concentration_rounded, dme_kinetics

PSTP, TSTP = 101325, 273.15          # PyREMOT/core/constants.py:18-20


def _dme3_feed(P, T):
    """setFeedMoleFraction(1, 0.5) (initData.py:11-40, float32) and the derived feed quantities of test_rmt_DME3.py."""
    y0_H2O = y0_CH3OH = y0_DME = 0.00001
    tmf0 = 1 - (y0_H2O + y0_CH3OH + y0_DME)
    COx = tmf0/(1 + 1)
    y0_H2 = 1*COx
    y0_CO2 = 0.5*COx
    y0_CO = COx - y0_CO2
    MoFri0 = np.array([y0_H2, y0_CO2, y0_H2O, y0_CO, y0_CH3OH, y0_DME], dtype=np.float32)
    ct0 = _feed_concentration_rounded(MoFri0, P, T)           # [kmol/m^3]
    return MoFri0, ct0


def m7_dme_input(ivp="default", model="M7"):
    P = 5*1e6
    T = 523
    MoFri0, ct0 = _dme3_feed(P, T)
    rea_D, rea_L, bed_por = 0.0381, 1, 0.39
    cat_d, cat_rho, cat_Cp, cat_por = 0.002, 1982, 960, 0.45
    bulk_rho = cat_rho*(1 - bed_por)
    SuGaVe = 0.2
    InGaVe = SuGaVe/bed_por
    rea_CSA = bed_por*(math.pi*(rea_D**2)/4)                   # rmtUtility.py:122-130
    VoFlRa = InGaVe*rea_CSA
    VoFlRaSTP = VoFlRa*(P/PSTP)*(TSTP/T)                       # rmtUtility.py:98-108
    MoFlRa0 = VoFlRaSTP/0.02241                                # rmtUtility.py:111-119
    rr = dme_kinetics(bulk_rho)
    varis = {"CaDe": cat_rho, "CaBeDe": bulk_rho, "CaPo": cat_por}
    varis.update({k: v for k, v in rr["VARS"].items() if k != "CaBeDe"})
    return {
        "model": model,
        "operating-conditions": {"pressure": P, "temperature": T, "period": 50},
        "feed": {
            "mole-fraction": MoFri0,
            "molar-flowrate": MoFlRa0,
            "molar-flux": 0,
            "volumetric-flowrate": VoFlRa,
            "concentration": ct0*1000,
            "mixture-viscosity": 1e-5,
            "components": {"shell": list(DME_COMPONENTS), "tube": [], "medium": []},
        },
        "reactions": dict(DME_REACTIONS_SPACED),
        "reaction-rates": {"VARS": varis, "RATES": rr["RATES"]},
        "external-heat": {"OvHeTrCo": 50, "EfHeTrAr": 4/rea_D, "MeTe": 523},
        "reactor": {
            "ReInDi": rea_D, "ReLe": rea_L, "PaDi": cat_d, "BeVoFr": bed_por,
            "CaBeDe": bulk_rho, "CaDe": cat_rho, "CaSpHeCa": cat_Cp/1000,
        },
        "solver-config": {"ivp": ivp},
    }


def m1_dme_input(ivp="default"):
    return m7_dme_input(ivp, model="M1")


STEADY_INPUTS = {("M7", "dme"): m7_dme_input, ("M1", "dme"): m1_dme_input}
