"""Global solver / model switches, mirroring the reference's module-level dicts.

``solverSetting``  <- PyREMOT/solvers/solSetting.py:30-106 (only the entries the N2 path reads:
                      N2.zNo/tNo/timesNo at pbHomoReactor.py:3435,3557,3561 and
                      T1.ode-solver.PreCorr3.n at :3572; S3.timesNo and M9.zNo: the output points of
                      the steady models M1 and M7, pbReactor.py:259, :1283).  Like the reference's dict it is a plain
                      mutable object read at run time, so ``solverSetting['N2']['zNo'] = 1024``
                      before ``rmtExe`` changes the mesh exactly as it does there.
``MODEL_SETTING``  <- PyREMOT/docs/modelSetting.py:10-18;  ``PROCESS_SETTING`` <- :21-23.

The device build additionally reads optional per-run overrides from
``modelInput['solver-config']`` (keys zNo, tNo, dt, rtol, atol, dtype, max-steps); absent keys
mean "reference behaviour".
"""
solverSetting = {
    "N1": {"zNo": 100},
    "N2": {"zNo": 20, "rNo": 5, "tNo": 5, "timesNo": 5},
    "S2": {"tNo": 10, "zNo": 100, "rNo": 7, "timesNo": 5},        # model M2 (solSetting.py:44-49)
    "S3": {"timesNo": 25},                                        # model M1's output points (solSetting.py:50-52)
    "M9": {"zNo": 30, "rNo": 1},                                  # model M7's output points (solSetting.py:53-62)
    "T1": {"ode-solver": {"PreCorr3": {"n": 100}}},
}

# (only "GaMaCoTe0" is read on the homogeneous paths built here: N2 raises under any value but "MAX" exactly like the
# reference's own RHS does, N1 switches to per-species scaling, M2 ignores it - golden G11; the other keys belong to
# the heterogeneous models)
MODEL_SETTING = {"g": "FIX", "MaTrCo": "FIX", "HeTrCo": "FIX", "GaDii": "FIX", "GaThCoi": "FIX", "GaVii": "FIX",
                 "GaMaCoTe0": "MAX"}
PROCESS_SETTING = {"ISO-THER": "iso-thermal", "NON-ISO-THER": "non-iso-thermal"}

# defaults of the device integrators (not in the reference: it delegates to scipy's defaults)
DEVICE_DEFAULTS = {
    "rk45-rtol": 1e-6,
    "rk45-atol": 1e-9,
    "rk45-h0": 1e-6,
    "rk45-max-steps": 50_000_000,
    "rk4-dt": 2e-6,
    # RODAS4 (tools/ros4_tol_scan.py, profiles/round1_ros_scheme.md): the outlet error against the tight
    # SciPy run falls smoothly with the tolerance - 4.5e-7 at rtol 1e-5, 1.1e-7 at 1e-6, 4e-8 at 1e-7 -
    # so 1e-6 keeps the 1e-6 requirement with a factor 9 in hand (the Kaps-Rentrop pair needed 1e-7)
    "ros4-rtol": 1e-6,
    "ros4-atol": 1e-9,
    "ros4-h0": 1e-5,
    # ivp "hip-auto" (what "default" / "LSODA" resolve to): explicit phase of the automatic stiff / non-stiff choice
    "auto-rk45-rtol": 1e-8,
    "auto-rk45-atol": 1e-11,
    "auto-probe-steps": 40,          # RK45 steps spent on finding out how stiff the interval is
    "auto-max-explicit-steps": 2000,  # estimated RK45 steps per output interval above which the stiff stepper takes over
    "n1-rtol": 1e-8,     # the steady profile is one lane's worth of work: afford tight defaults
    "n1-atol": 1e-11,
}

ROUND_FUN_ACCURACY = 3   # PyREMOT/core/config.py:8-24 ("computation-time" rounding)
