"""What the fit tests share (tests/test_fit_cpu.py, tests/test_gpu_fit.py) and what tools/make_golden.py (target ``fit``)
runs: the input and the experiments of solver-config "fit", its reference on the unchanged oracle, and the goldens G22.

Nothing of the product is imported.  The reference's predictions are read off steady states of the oracle's right-hand side
f(y; p) = 0 with the fitted VARS scalars moved: campaign_ref.steady_state from the cold start (the recipe of G17: root, else
LSODA legs and root - the branch the march takes) and sens_ref.polish; a neighbouring parameter point starts from the
experiment's last state.  The data are those predictions at P_TRUE (case FN: plus recorded Gaussian noise).  The fit is
scipy.optimize.least_squares (method "trf", x_scale "jac", tolerances 1e-14) with central differences of those steady states
as the Jacobian (step FD_STEP |p|).

Input: the DME notebook input with the pre-exponential factors of the three rate constants lifted into scalar VARS entries
A1, A2, A3.  Eight experiments at zNo = 20 and fifty times the notebook's feed rate: coolant 508 / 523 / 538 K crossed with 4 / 5 MPa, and two feed ratios.
A measured vector is ordered: the outlet mole fractions in the order of the experiment's dict, the outlet temperature, the
peak temperature.
"""
import copy
import json
import math
import os

import numpy as np

import campaign_ref as CR
import sens_ref as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R_GAS = 8.314472
ZNO = 20
NAMES = ("A1", "A2", "A3")
P_TRUE = {"A1": 35.45, "A2": 7.3976, "A3": 8.2894e4}
SIGMA = {"outlet-mole-fraction": 1e-4, "outlet-temperature": 0.1, "peak-temperature": 0.1}
FD_STEP = 1e-4
COND_CAP = 1e8           # Marquardt-scaled cond(H) at the optimum above which a case is refused
TRUE_CAP = 1e-7          # |p_ref - p_true| / |p_true| of a noise-free case above which it is refused
NOISE_SEED = 22
CASES = {
    "FA": {"parameters": ["A1", "A3"], "start": [1.3, 0.7], "noise": False},
    "FB": {"parameters": ["A1", "A2", "A3"], "start": [1.3, 1.4, 0.7], "noise": False},
    "FN": {"parameters": ["A1", "A3"], "start": [1.3, 0.7], "noise": True},
}
# Beside 10 |p_ref - p_true| a fitted value may differ from the target by this part of it: 10 x the largest
# |value - target| / |target| first measured on the device (2.50e-12 for FA, 9.76e-12 for FB, 2.08e-10 for FN:
# profiles/fit.md), never above 1e-6
FLOOR_REL = {"FA": 2.5e-11, "FB": 9.8e-11, "FN": 2.1e-9}
# entries of the covariance of FN relative to sqrt(C_ii C_jj): 10 x the first measured value (5.182e-8), never above 1e-3
COV_BOUND = 5.2e-7
X4 = ("CH3OH", "DME", "CO", "H2O")


def fit_kinetics(CaBeDe):
    """tests/inputs.py dme_kinetics with K1, K2, K3 = A_k exp(...) and A_k scalar VARS entries"""
    import inputs as INP
    rr = INP.dme_kinetics(CaBeDe)
    VARS = {}
    for k, v in rr["VARS"].items():
        if k == "K1":
            VARS.update({nm: P_TRUE[nm] for nm in NAMES})
            VARS["K1"] = lambda x: x['A1']*math.exp(-1.7069e4/x['RT'])
        elif k == "K2":
            VARS["K2"] = lambda x: x['A2']*math.exp(-2.0436e4/x['RT'])
        elif k == "K3":
            VARS["K3"] = lambda x: x['A3']*math.exp(-5.2940e4/x['RT'])
        else:
            VARS[k] = v
    return {"VARS": VARS, "RATES": rr["RATES"]}


def base_input(**cfg):
    import inputs as INP
    mi = INP.dme_notebook_input(ivp="hip-ros4", period=0.05)
    mi["reaction-rates"] = fit_kinetics(mi["reactor"]["CaBeDe"])
    mi["solver-config"].update({"quiet": True, "zNo": ZNO, "tNo": 2, "display-result": "False"})
    mi["solver-config"].update(cfg)
    return mi


WIDE = ("A1", "A2", "A3", "B1", "B2", "B3", "B4", "B5")


def wide_input():
    """base_input with five more scalar VARS entries no rate reads: a mechanism with eight per-reactor inputs, for the
    kernels' own test at P = 8"""
    mi = base_input()
    mi["reaction-rates"]["VARS"].update({nm: 1.0 + 0.125*k for k, nm in enumerate(WIDE[3:])})
    return mi


def feed(P, T, y):
    y = np.asarray(y, dtype=float)
    return [float(v) for v in y/y.sum()*P/(R_GAS*T)]


Y_BASE = (0.5, 0.25, 1e-5, 0.25, 1e-5, 1e-5)            # H2, CO2, H2O, CO, CH3OH, DME
# Fifty times the notebook's feed rate in every experiment.  At the notebook's own the bed is at equilibrium behind its first
# node and the outlet does not depend on A3 (a 100 % change moves the weighted residuals by 0.015; at forty times by 6.4).
# Between 15 and 40 times the law of solver-config "fit" (no bounds, no log-parameters) walks A3 through zero from the
# starts of FA or FB and does not come back; at 50 times both converge in 7 iterations; from 60 times on the steady-state
# march does not converge for these beds (measured on the device: profiles/fit.md)
FLOW = 50*0.000228


def conditions():
    """the eight experiments' overrides of the base input (members of the list form of "ensemble")"""
    out = []
    for Tm in (508.0, 523.0, 538.0):
        for P in (4.0e6, 5.0e6):
            out.append({"external-heat": {"MeTe": Tm}, "operating-conditions": {"pressure": P},
                        "feed": {"volumetric-flowrate": FLOW, "concentration": feed(P, 523.0, Y_BASE)}})
    for y in ((0.60, 0.15, 1e-5, 0.25, 1e-5, 1e-5), (0.40, 0.25, 1e-5, 0.35, 1e-5, 1e-5)):
        out.append({"external-heat": {"MeTe": 523.0}, "feed": {"volumetric-flowrate": FLOW, "concentration": feed(5.0e6, 523.0, y)}})
    return out


def quantities(e):
    """what experiment e measures: (components, outlet temperature?, peak temperature?)"""
    if e == 4:
        return ("DME",), True, False                     # two values only: the padding of the table
    return X4, True, e in (1, 6)


def labels(e):
    comps, tout, tpeak = quantities(e)
    return ["outlet-mole-fraction:%s" % c for c in comps] + (["outlet-temperature"] if tout else []) \
        + (["peak-temperature"] if tpeak else [])


def sigmas(e):
    comps, tout, tpeak = quantities(e)
    return np.array([SIGMA["outlet-mole-fraction"]]*len(comps) + ([SIGMA["outlet-temperature"]] if tout else [])
                    + ([SIGMA["peak-temperature"]] if tpeak else []))


def deep_merge(base, override):
    out = copy.copy(base)
    for k, v in override.items():
        out[k] = deep_merge(base[k], v) if isinstance(v, dict) and isinstance(base.get(k), dict) else v
    return out


def measured_entry(e, values):
    """the "measured" dict of experiment e from its vector"""
    comps, tout, tpeak = quantities(e)
    values = [float(v) for v in values]
    out = {"outlet-mole-fraction": dict(zip(comps, values[:len(comps)]))}
    rest = values[len(comps):]
    if tout:
        out["outlet-temperature"] = rest.pop(0)
    if tpeak:
        out["peak-temperature"] = rest.pop(0)
    return out


def case_input(name, measured=None, repeat=1, **fit_cfg):
    """the modelInput of a golden case: ``measured`` [E] vectors (default: the golden's); ``repeat``: every experiment
    that many times in a row"""
    case = CASES[name]
    if measured is None:
        g = golden(name)
        measured = [g["measured"][e][:len(labels(e))] for e in range(len(conditions()))]
    mi = base_input()
    for nm, s in zip(case["parameters"], case["start"]):
        mi["reaction-rates"]["VARS"][nm] = s*P_TRUE[nm]
    exps = []
    for e, cond in enumerate(conditions()):
        for _ in range(repeat):
            exps.append({"conditions": cond, "measured": measured_entry(e, measured[e]), "sigma": dict(SIGMA)})
    mi["solver-config"]["fit"] = dict({"parameters": [{"rate-constant": nm} for nm in case["parameters"]],
                                       "experiments": exps}, **fit_cfg)
    return mi


def meta():
    with open(os.path.join(GOLD, "g22_fit.json")) as f:
        return json.load(f)


def golden(name):
    return np.load(os.path.join(GOLD, "g22_fit_%s.npz" % name))


def p_true(name):
    return np.array([P_TRUE[nm] for nm in CASES[name]["parameters"]])


def value_bound(name, gold):
    """[P]: 10 |p_ref - p_true| + FLOOR_REL |target| - what a fitted value may differ from its target by"""
    assert FLOOR_REL[name] <= 1e-6
    target = np.asarray(gold["p_ref"]) if CASES[name]["noise"] else p_true(name)
    return 10*np.abs(np.asarray(gold["p_ref_noise_free"]) - p_true(name)) + FLOOR_REL[name]*np.abs(target)


# ----------------------------------------------------------------------------- the reference
class Reference:
    """The oracle's steady states of the eight experiments as a function of the fitted constants."""

    def __init__(self, O, names, log=None):
        self.O, self.names, self.log = O, list(names), log
        base = base_input()
        self.prs = [dict(O.setup_n2(deep_merge(base, c), zNo=ZNO)) for c in conditions()]
        self.last = [None]*len(self.prs)           # (None: the cold start)
        self.cold = None
        self.worst = 0.0
        self.solves = 0

    def state(self, e, p):
        pr = dict(self.prs[e])
        pr["VARS"] = dict(pr["VARS"], **{nm: float(v) for nm, v in zip(self.names, p)})
        f = self.O.make_rhs_vec(pr)
        start = pr["IV"] if self.last[e] is None else self.last[e]
        y, r, legs = CR.steady_state(f, start, pr["IV"], self.log)
        y, r = SR.polish(f, y)
        self.worst = max(self.worst, r)
        self.solves += 1
        return y, r

    def predict_one(self, e, y):
        pr = self.prs[e]
        S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
        Y = np.reshape(y, (V, N))
        c = np.maximum(Y[:S, -1], 1e-30)*np.max(pr["SpCoi0"])
        x = c/c.sum()
        T = Y[S]*pr["Tf"] + pr["Tf"]
        comps, tout, tpeak = quantities(e)
        out = [x[pr["compList"].index(s)] for s in comps]
        if tout:
            out.append(T[-1])
        if tpeak:
            out.append(np.max(T))
        return np.array(out)

    def predict(self, p, keep=True, gate=False):
        """[E] prediction vectors at p; ``keep``: the states become the next start; ``gate``: refuse above the gate"""
        out = []
        for e in range(len(self.prs)):
            y, r = self.state(e, p)
            if gate and not r <= CR.GATE:
                raise SystemExit("G22: the steady state of experiment %d at %s ends at max|f| = %.3e, above the gate %.1e"
                                 % (e, list(p), r, CR.GATE))
            if keep:
                self.last[e] = y
            out.append(self.predict_one(e, y))
        return out

    def residual(self, p, measured, keep=True):
        try:
            pred = self.predict(p, keep)
        except RuntimeError:            # no steady state there (LSODA gave up): a residual no trial is accepted with
            return np.full(sum(len(m[:len(labels(e))]) for e, m in enumerate(measured)), 1e3)
        return np.concatenate([(pr - np.asarray(m)[:len(pr)])/sigmas(e) for e, (pr, m) in enumerate(zip(pred, measured))])

    def jacobian(self, p, measured):
        p = np.asarray(p, dtype=float)
        J = []
        for j in range(len(p)):
            d = FD_STEP*abs(p[j])
            hi, lo = p.copy(), p.copy()
            hi[j] += d
            lo[j] -= d
            J.append((self.residual(hi, measured, False) - self.residual(lo, measured, False))/(2*d))
        return np.array(J).T


def reference_fit(ref, name, measured, start=None):
    """dict(p_ref, cost, hessian, covariance, cond, nfev): scipy's fit of a case on ``measured``"""
    import scipy.optimize
    case = CASES[name]
    x0 = np.array(case["start"])*p_true(name) if start is None else np.asarray(start, dtype=float)
    ref.last = list(ref.cold)                       # every experiment's branch: its state from the cold start at p_true
    sol = scipy.optimize.least_squares(lambda p: ref.residual(p, measured), x0, jac=lambda p: ref.jacobian(p, measured),
                                       method="trf", x_scale="jac", ftol=1e-14, xtol=1e-14, gtol=1e-14, max_nfev=60)
    J = ref.jacobian(sol.x, measured)
    r = ref.residual(sol.x, measured)
    H = J.T @ J
    cost = 0.5*float(r @ r)
    d = np.sqrt(np.diag(H))
    cond = float(np.linalg.cond(H/np.outer(d, d)))
    M, P = len(r), len(sol.x)
    cov = 2*cost/(M - P)*np.linalg.inv(H) if M > P else None
    return {"p_ref": sol.x, "cost": cost, "hessian": H, "covariance": cov, "cond": cond, "nfev": int(sol.nfev),
            "residual": r}


def pad(vectors, width=None):
    width = width or max(len(v) for v in vectors)
    out = np.full((len(vectors), width), np.nan)
    for e, v in enumerate(vectors):
        out[e, :len(v)] = v
    return out


def run_case(O, name, log=None):
    """The golden of a case (refusals as SystemExit): dict(measured [E][MQ] NaN-padded, predicted_true, p_ref,
    p_ref_noise_free, cost, hessian, covariance, cond, residual_gate)."""
    case = CASES[name]
    ref = Reference(O, case["parameters"], log)
    pt = p_true(name)
    states = os.path.join(GOLD, "g22_fit_states.npz")
    if os.path.exists(states):                      # (made from the cold start by the target fit=states)
        ref.last = list(np.load(states)["states"])
    truth = ref.predict(pt, keep=True, gate=True)
    ref.cold = list(ref.last)
    ref.predict(np.array(case["start"])*pt, keep=False, gate=True)
    clean = reference_fit(ref, name, truth)
    if log:
        log("%s noise-free: p_ref %s, cost %.3e, cond %.3e, %d evaluations, %d steady states"
            % (name, clean["p_ref"], clean["cost"], clean["cond"], clean["nfev"], ref.solves))
    rel = np.abs(clean["p_ref"] - pt)/np.abs(pt)
    if np.any(rel > TRUE_CAP):
        raise SystemExit("G22 %s: |p_ref - p_true| / |p_true| = %s exceeds %.0e - not written" % (name, rel, TRUE_CAP))
    out, measured = clean, truth
    if case["noise"]:
        rng = np.random.default_rng(NOISE_SEED)
        measured = [t + rng.standard_normal(len(t))*sigmas(e) for e, t in enumerate(truth)]
        out = reference_fit(ref, name, measured)
        if log:
            log("%s with noise: p_ref %s, cost %.6e, cond %.3e" % (name, out["p_ref"], out["cost"], out["cond"]))
    if out["cond"] > COND_CAP:
        raise SystemExit("G22 %s: Marquardt-scaled cond(H) = %.3e exceeds %.0e - widen the spread of the conditions"
                         % (name, out["cond"], COND_CAP))
    return {"measured": pad(measured), "predicted_true": pad(truth), "p_ref": out["p_ref"],
            "p_ref_noise_free": clean["p_ref"], "cost": out["cost"], "hessian": out["hessian"],
            "covariance": out["covariance"], "cond": out["cond"], "residual_gate": ref.worst}
