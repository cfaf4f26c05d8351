"""What the sensitivity tests share (tests/test_sensitivity_cpu.py, tests/test_gpu_sensitivity.py) and what
tools/make_golden.py (target ``sensitivity``) runs: the reference of solver-config "sensitivity" on the unchanged oracle,
and the goldens G21.

Nothing of the product is imported.  The reference differences steady states: for a parameter p every steady state
f(y; p +- d) = 0 comes from campaign_ref.steady_state (scipy.optimize.root from the base state; above the gate of G17 the
recipe of G17 - LSODA legs from the cold start, then root) on the oracle's right-hand side with the ONE value moved and
everything else of the setup - the scaling Cmax, Tf and the constants formed from the feed - unchanged:

    medium-temperature    pr["Tm"]            inlet-temperature   pr["T0"]          inlet-pressure   pr["P0"]
    inlet-concentration   pr["SpCoi0"][i]     (a component that is not the feed's largest: max(SpCoi0) is the scaling)
    rate-constant         pr["VARS"][name]

Central differences at d and d/2, D = (4 D(d/2) - D(d))/3 (Richardson), and per (parameter, row) fd_error =
max_z |D(d/2) - D(d)|.  Rows: the V state rows in the units of the packed profiles (concentration, K) and the pressure row
[Pa].  A case whose fd_error exceeds 1e-5 of a row's largest magnitude is refused.
"""
import json
import os

import numpy as np

import campaign_ref as CR
import profile_ref as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FD_CAP = 1e-5            # fd_error / max|row| above which a case is refused
DELTA0 = 1e-4            # the first d: 1e-4 |p| (a concentration: 1e-4 of the largest feed concentration)
# Beside 10 fd_error a row may differ from G21 by this part of its largest magnitude: 10 x the case's own largest
# |sweep - golden| / max|row| as first measured (4.882e-8, 5.085e-8, 8.814e-6, 3.403e-9: profiles/sensitivity.md), and
# never above 1e-6
FLOOR_REL = {"SA": 4.9e-7, "SB": 5.1e-7, "SK": 1e-6, "SW": 3.4e-8}
BOUNDARY4 = ["medium-temperature", "inlet-temperature", "inlet-pressure", {"inlet-concentration": "CO"}]
CASES = {
    "SA": {"input": "dme_nb", "zNo": 20, "parameters": BOUNDARY4},
    "SB": {"input": "dme_nb", "zNo": 20, "parameters": BOUNDARY4, "axial-profile": "G18-A"},
    "SK": {"input": "dme_nb", "zNo": 20, "parameters": [{"rate-constant": "CaBeDe"}, "medium-temperature"]},
    "SW": {"input": "syn12", "zNo": 20, "parameters": ["medium-temperature", "inlet-pressure"]},      # host emulation only
}


def meta():
    with open(os.path.join(GOLD, "g21_sensitivity.json")) as f:
        return json.load(f)


def golden(name):
    return np.load(os.path.join(GOLD, "g21_sensitivity_%s.npz" % name))


def profile_spec(case):
    return dict(PR.BED_A) if case.get("axial-profile") == "G18-A" else case.get("axial-profile")


def case_input(name, **cfg):
    """the modelInput of a golden case, with the keys "initial" and "sensitivity" set"""
    import inputs as INP
    case = CASES[name]
    mi = INP.ALL_N2_INPUTS[case["input"]]()
    mi["solver-config"].update({"quiet": True, "zNo": case["zNo"], "tNo": 2, "display-result": "False",
                                "initial": "steady", "sensitivity": {"parameters": list(case["parameters"])}})
    if profile_spec(case):
        mi["solver-config"]["axial-profile"] = profile_spec(case)
    mi["solver-config"].update(cfg)
    return mi


def label(p):
    if isinstance(p, str):
        return p
    (k, nm), = p.items()
    return "%s:%s" % (k, nm)


def base_value(pr, p):
    """the parameter's value at the operating point, and the magnitude its step is taken from"""
    if isinstance(p, str):
        v = float(pr[{"medium-temperature": "Tm", "inlet-temperature": "T0", "inlet-pressure": "P0"}[p]])
        return v, abs(v)
    (k, nm), = p.items()
    if k == "inlet-concentration":
        return float(pr["SpCoi0"][pr["compList"].index(nm)]), float(np.max(pr["SpCoi0"]))
    v = float(pr["VARS"][nm])
    return v, abs(v)


def moved(pr, p, d):
    """a copy of the oracle's parameter dict with the one value moved by d"""
    out = dict(pr)
    if isinstance(p, str):
        key = {"medium-temperature": "Tm", "inlet-temperature": "T0", "inlet-pressure": "P0"}[p]
        out[key] = pr[key] + d
        return out
    (k, nm), = p.items()
    if k == "inlet-concentration":
        i = pr["compList"].index(nm)
        c = np.array(pr["SpCoi0"], dtype=float)
        c[i] += d
        assert np.max(c) == np.max(pr["SpCoi0"]) and i != int(np.argmax(pr["SpCoi0"])), \
            "the moved component must leave max(SpCoi0), the scaling, unchanged"
        out["SpCoi0"] = c
    else:
        out["VARS"] = dict(pr["VARS"], **{nm: float(pr["VARS"][nm]) + d})
    return out


def rhs_of(O, pr, case):
    spec = profile_spec(case)
    if not spec:
        return O.make_rhs_vec(pr)
    a, delta = PR.bed(spec, case["zNo"], case["MeTe0"])
    return PR.profiled_rhs(O, pr, a, delta)


def rows_of(O, pr, y):
    """[V+1][N]: the state in the units of the packed profiles (concentration, K) and the node pressures"""
    S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
    Y = np.reshape(np.asarray(y, dtype=float), (V, N))
    out = np.zeros((V + 1, N))
    out[:S] = Y[:S]*np.max(pr["SpCoi0"])
    if not pr["iso"]:
        out[S] = Y[S]*pr["Tf"] + pr["Tf"]
    out[V] = O.neighbourhood(pr, Y.reshape(1, V, N))[4][0]
    return out


def polish(f, y):
    """Newton steps on f(0, y) = 0 with a central-difference Jacobian (the steady states that are differenced have to be
    converged well below the step of the differencing); the best iterate by max|f| comes back"""
    y = np.array(y, dtype=float)
    best, r_best = y.copy(), float(np.max(np.abs(f(0.0, y))))
    for _ in range(3):
        h = 1e-7*np.maximum(np.abs(y), 1e-6)
        Yp = y[None, :] + np.diag(h)
        Ym = y[None, :] - np.diag(h)
        J = ((np.asarray(f(0.0, Yp)) - np.asarray(f(0.0, Ym)))/(2*h)[:, None]).T
        try:
            y = y - np.linalg.solve(J, np.asarray(f(0.0, y)))
        except np.linalg.LinAlgError:
            break
        r = float(np.max(np.abs(f(0.0, y))))
        if np.all(np.isfinite(y)) and r < r_best:
            best, r_best = y.copy(), r
        else:
            break
    return best, r_best


def steady(O, pr, case, start, log=None):
    f = rhs_of(O, pr, case)
    y, r, legs = CR.steady_state(f, start, pr["IV"], log)
    y, r = polish(f, y)
    if not r <= CR.GATE:
        raise SystemExit("a steady state ends at max|f| = %.3e, above the gate %.1e: the case is refused" % (r, CR.GATE))
    return y, r


def start_state(case):
    """the golden steady state the differencing starts from: G18 S for bed A, G17 else"""
    if case.get("axial-profile") == "G18-A":
        return np.array(PR.golden("S")["state"], dtype=float)
    return np.array(np.load(os.path.join(GOLD, "g17_steady_%s.npz" % case["input"]))["state"], dtype=float)


def run_case(O, INP, name, deltas=None, log=None):
    """The reference of a case: dict(state [V*N], rows [V+1][N], values [P], delta [P], D [P][V+1][N] (Richardson),
    fd_error [P][V+1], residual).  ``deltas``: relative steps per parameter label (default DELTA0)."""
    case = dict(CASES[name])
    pr = dict(O.setup_n2(INP.ALL_N2_INPUTS[case["input"]](), zNo=case["zNo"]))
    case["MeTe0"] = pr["Tm"]
    y0, r0 = steady(O, pr, case, start_state(case), log)
    base = rows_of(O, pr, y0)
    params = case["parameters"]
    P = len(params)
    D = np.zeros((P,) + base.shape)
    err = np.zeros((P, base.shape[0]))
    vals, steps, worst = np.zeros(P), np.zeros(P), r0
    for n, p in enumerate(params):
        vals[n], mag = base_value(pr, p)
        d = float((deltas or {}).get(label(p), DELTA0))*mag
        steps[n] = d
        diff = []
        for h in (d, 0.5*d):
            side = []
            for sgn in (+1.0, -1.0):
                prm = moved(pr, p, sgn*h)
                y, r = steady(O, prm, case, y0, log)
                worst = max(worst, r)
                side.append(rows_of(O, prm, y))
            diff.append((side[0] - side[1])/(2*h))
        D[n] = (4*diff[1] - diff[0])/3
        err[n] = np.max(np.abs(diff[1] - diff[0]), axis=1)
        if log:
            rel = err[n]/np.maximum(np.max(np.abs(D[n]), axis=1), 1e-300)
            log("%s %s: p = %.6g d = %.3g, fd_error / max|row| at most %.2e" % (name, label(p), vals[n], d,
                                                                                 float(np.max(rel[np.max(np.abs(D[n]), axis=1) > 0]))))
    return {"state": y0, "rows": base, "values": vals, "delta": steps, "D": D, "fd_error": err, "residual": worst}


def refused(res):
    """the (parameter, row) pairs whose fd_error exceeds FD_CAP of the row's largest magnitude"""
    mag = np.max(np.abs(res["D"]), axis=2)
    return [(int(p), int(v)) for p, v in zip(*np.nonzero(res["fd_error"] > FD_CAP*mag))]


def bound(gold, name):
    """[P][V+1]: 10 fd_error + FLOOR_REL[name] max|row| - what a sensitivity may differ from G21 by, per row"""
    assert FLOOR_REL[name] <= 1e-6
    return 10*gold["fd_error"] + FLOOR_REL[name]*np.max(np.abs(gold["D"]), axis=2)
