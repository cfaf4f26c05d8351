"""What the frequency-response tests share (tests/test_frequency_cpu.py, tests/test_gpu_frequency.py) and what
tools/make_golden.py (target ``frequency``) runs: the reference of solver-config "frequency-response" on the unchanged
oracle, and the goldens G23.

Nothing of the product is imported.  A case starts from the oracle's steady state (the recipe and the gate of
sens_ref.steady, on oracle.n2_oracle.make_rhs_vec, profile_ref.profiled_rhs for a profiled bed).  Around it the DENSE
Jacobian J = df/dy [V N x V N], the input columns B = df/dp (sens_ref.moved: the ONE value moved), and the output map of
the rows (sens_ref.rows_of: the state in the units of the packed profiles and the node pressures, which are algebraic in
y and p) R_y, R_p are taken by central differences at the relative step d and at d/2 and Richardson-extrapolated,
X = (4 X(d/2) - X(d))/3.  Then, per frequency, by LAPACK

    G(iw) = R_y (iw I - J)^-1 B + R_p                      [P][F][V+1][N] complex, per unit of the input

and fd_error per (input, row) = max over frequencies and nodes of |G from the d/2 differences - G from the d differences|.
A case is refused when fd_error exceeds sens_ref.FD_CAP of the row's largest magnitude, when the steady state misses the
gate, or when a species of the steady state is within 10 differencing steps of the clamp 1e-30 (the kink of the clamp
would make a central difference meaningless).  The frequency grid is 0 and 8 log-spaced values from one decade below the
slowest |Re lambda| of J to one decade above the convective rate (the species' upwind coupling F1/dz), rounded to three
digits; the chosen values are in the golden's json and in profiles/frequency_response.md.
"""
import json
import os

import numpy as np

import profile_ref as PR
import sens_ref as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DELTA0 = 1e-4            # the relative step d of the differencing
THETA_FLOOR = 1e-2       # the scaled temperature (T - Tf)/Tf passes through 0: its step is d max(|theta|, this)
CLAMP = 1e-30
POINTS = 8
# Beside 10 fd_error a row may differ from G23 by this part of its largest magnitude: 10 x the case's own largest
# |host emulation - golden| / max|row| as first measured (MEASURED; profiles/frequency_response.md), and never above 1e-6.
# Ten times the measured value is above the cap in all three cases, so the cap it is.
MEASURED = {"FA": 3.241e-7, "FB": 1.224e-7, "FI": 8.224e-6}
FLOOR_REL = {name: min(10*v, 1e-6) for name, v in MEASURED.items()}
CASES = {
    "FA": {"input": "dme_nb", "zNo": 20, "inputs": SR.BOUNDARY4},
    "FB": {"input": "dme_nb", "zNo": 20, "inputs": ["medium-temperature", "inlet-temperature"], "axial-profile": "G18-A"},
    "FI": {"input": "ch4", "zNo": 20, "inputs": [{"inlet-concentration": "C2H4"}], "process-type": "iso-thermal"},
}


def meta():
    with open(os.path.join(GOLD, "g23_frequency.json")) as f:
        return json.load(f)


def golden(name):
    return np.load(os.path.join(GOLD, "g23_frequency_%s.npz" % name))


def base_input(name):
    import inputs as INP
    case = CASES[name]
    mi = INP.ALL_N2_INPUTS[case["input"]]()
    if case.get("process-type"):
        mi["operating-conditions"]["process-type"] = case["process-type"]
    return mi


def case_input(name, frequencies=None, **cfg):
    """the modelInput of a golden case, with the keys "initial" and "frequency-response" set (the golden's grid)"""
    case = CASES[name]
    mi = base_input(name)
    w = list(meta()["cases"][name]["frequencies"]) if frequencies is None else list(frequencies)
    mi["solver-config"].update({"quiet": True, "zNo": case["zNo"], "tNo": 2, "display-result": "False", "initial": "steady",
                                "frequency-response": {"inputs": list(case["inputs"]), "frequencies": w, "profile": True}})
    if SR.profile_spec(case):
        mi["solver-config"]["axial-profile"] = SR.profile_spec(case)
    mi["solver-config"].update(cfg)
    return mi


def start_state(case, pr):
    if case["input"] == "ch4":
        return np.array(pr["IV"], dtype=float)           # (no golden steady state of this bed: from the cold start)
    return SR.start_state(case)


def steps_of(pr, y, d):
    """the differencing step per state entry [V*N]"""
    S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
    Y = np.reshape(np.asarray(y, dtype=float), (V, N))
    h = d*np.abs(Y)
    if not pr["iso"]:
        h[S] = d*np.maximum(np.abs(Y[S]), THETA_FLOOR)
    return h.reshape(-1)


def near_clamp(pr, y, d):
    """the species entries of the state within 10 differencing steps of the clamp"""
    S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
    Y = np.reshape(np.asarray(y, dtype=float), (V, N))[:S]
    h = steps_of(pr, y, d).reshape(V, N)[:S]
    return np.argwhere(Y - 10*h <= CLAMP)


def linearise(O, pr, case, y, inputs, d):
    """(J [VN][VN], B [VN][P], Ry [(V+1)N][VN], Rp [(V+1)N][P]) by central differences at the relative step d"""
    f = SR.rhs_of(O, pr, case)
    n = len(y)
    h = steps_of(pr, y, d)
    Yp, Ym = y[None, :] + np.diag(h), y[None, :] - np.diag(h)
    J = ((np.asarray(f(0.0, Yp)) - np.asarray(f(0.0, Ym)))/(2*h)[:, None]).T
    rows = lambda prm, v: SR.rows_of(O, prm, v).reshape(-1)
    Ry = np.array([(rows(pr, Yp[j]) - rows(pr, Ym[j]))/(2*h[j]) for j in range(n)]).T
    B, Rp = np.zeros((n, len(inputs))), np.zeros((Ry.shape[0], len(inputs)))
    for k, p in enumerate(inputs):
        _, mag = SR.base_value(pr, p)
        dp = d*mag
        pp, pm = SR.moved(pr, p, dp), SR.moved(pr, p, -dp)
        B[:, k] = (SR.rhs_of(O, pp, case)(0.0, y) - SR.rhs_of(O, pm, case)(0.0, y))/(2*dp)
        Rp[:, k] = (rows(pp, y) - rows(pm, y))/(2*dp)
    return J, B, Ry, Rp


def response(lin, omegas, shape):
    """G [P][F][V+1][N] of (J, B, Ry, Rp)"""
    J, B, Ry, Rp = lin
    n = J.shape[0]
    G = np.zeros((B.shape[1], len(omegas)) + shape, dtype=np.complex128)
    for f, w in enumerate(omegas):
        s = np.linalg.solve(1j*w*np.eye(n) - J, B.astype(np.complex128))
        G[:, f] = (Ry @ s + Rp).T.reshape((B.shape[1],) + shape)
    return G


def round3(v):
    return float("%.3g" % v)


def grid(J, pr):
    """(frequencies [1 + POINTS], slowest |Re lambda|, convective rate): 0 and POINTS log-spaced values from a decade below
    the slowest mode to a decade above the species' upwind coupling d f_(0,1) / d y_(0,0) = F1/dz"""
    N = pr["zNo"]
    lam = np.linalg.eigvals(J)
    slow = float(np.min(np.abs(lam.real)))
    conv = float(J[1, 0]) if N > 1 else float(-J[0, 0])
    lo, hi = round3(0.1*slow), round3(10*conv)
    w = [round3(v) for v in np.exp(np.linspace(np.log(lo), np.log(hi), POINTS))]
    return np.array([0.0] + w), slow, conv, lam


def run_case(O, INP, name, log=None, omegas=None):
    """The reference of a case: dict(state, rows, values, frequencies, G [P][F][V+1][N] (from the Richardson matrices),
    fd_error [P][V+1], residual, slowest, convective, max_real)."""
    case = dict(CASES[name])
    pr = dict(O.setup_n2(base_input(name), zNo=case["zNo"]))
    case["MeTe0"] = pr["Tm"]
    y0, r0 = SR.steady(O, pr, case, start_state(case, pr), log)
    bad = near_clamp(pr, y0, DELTA0)
    if len(bad):
        raise SystemExit("%s: species entries %s of the steady state are within 10 differencing steps of the clamp: the "
                         "case is refused" % (name, bad[:4].tolist()))
    base = SR.rows_of(O, pr, y0)
    inputs = case["inputs"]
    lin1 = linearise(O, pr, case, y0, inputs, DELTA0)
    lin2 = linearise(O, pr, case, y0, inputs, 0.5*DELTA0)
    rich = tuple((4*b - a)/3 for a, b in zip(lin1, lin2))
    w, slow, conv, lam = grid(rich[0], pr)
    if omegas is not None:
        w = np.asarray(omegas, dtype=float)
    G1, G2, G = (response(l, w, base.shape) for l in (lin1, lin2, rich))
    err = np.max(np.abs(G2 - G1), axis=(1, 3))
    if log:
        mag = np.max(np.abs(G), axis=(1, 3))
        log("%s: max|f| = %.2e; slowest |Re lambda| = %.4g, convective rate = %.4g, largest Re lambda = %.4g; frequencies %s; "
            "fd_error / max|row| at most %.2e" % (name, r0, slow, conv, float(np.max(lam.real)), w.tolist(),
                                                  float(np.max(err[mag > 0]/mag[mag > 0]))))
    return {"state": y0, "rows": base, "values": np.array([SR.base_value(pr, p)[0] for p in inputs]), "frequencies": w,
            "G": G, "fd_error": err, "residual": r0, "slowest": slow, "convective": conv, "max_real": float(np.max(lam.real)),
            "J": rich[0], "B": rich[1]}


def refused(res):
    """the (input, row) pairs whose fd_error exceeds sens_ref.FD_CAP of the row's largest magnitude"""
    mag = np.max(np.abs(res["G"]), axis=(1, 3))
    return [(int(p), int(v)) for p, v in zip(*np.nonzero(res["fd_error"] > SR.FD_CAP*mag))]


def bound(gold, name):
    """[P][V+1]: 10 fd_error + FLOOR_REL[name] max|row| - what a response may differ from G23 by, per (input, row)"""
    assert FLOOR_REL[name] <= 1e-6
    return 10*gold["fd_error"] + FLOOR_REL[name]*np.max(np.abs(gold["G"]), axis=(1, 3))


def rows_of_entry(entry):
    """[P][F][V+1][N] of a result entry with "profile": True: the golden's rows"""
    return np.concatenate([entry["state"], entry["pressure"][:, :, None, :]], axis=2)
