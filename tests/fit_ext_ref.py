"""What the tests of the extended fit share (tests/test_fit_ext_cpu.py, tests/test_gpu_fit_ext.py) and what
tools/make_golden.py (target ``fit_ext``) runs: log-scaled and bounded parameters, measurements along the bed, their
reference on the unchanged oracle, and the goldens G24.  Builds on tests/fit_ref.py, which stays as it is.

The new quantities are read off the oracle's steady states: the node temperatures in K and the node mole fractions of the
clamped node state, interpolated linearly between the two mesh nodes around z/L = pos (nodes at n/(N-1)).  The reference fit
is scipy.optimize.least_squares (method "trf", x_scale "jac", tolerances 1e-14) with ``bounds=``; a parameter that ends
within ON_BOUND of a bound against which the gradient pushes is then held at the bound and the others are refitted without
bounds, so that p_ref is the optimum on the face and not trf's interior approach to it.

Cases
* FC  FA (A1, A3 at fifty times the notebook's feed rate, noise-free data) with A3 bounded above by 0.9 p_true: the
      reference ends on the bound.
* FP  FN's noisy data plus, per experiment, a temperature profile at five positions (0, exactly a node, two between
      nodes, 1) and the DME mole fraction at one interior port, with recorded noise of their own.
* FL  FB's three constants, all log-scaled with bounds [start/10, 10 start], on noise-free data at the LOWEST of
      FL_FEEDS times the notebook's feed rate for which ``law_fit`` (the product's numpy law, fit.emulate_update_ex, on the
      oracle) converges to p_true within fit_ref.TRUE_CAP in at most 30 iterations; every candidate tried is recorded.
"""
import json
import os

import numpy as np

import fit_ref as FR

GOLD = FR.GOLD
ZNO = FR.ZNO
SIGMA = dict(FR.SIGMA, **{"temperature-profile": 0.1, "mole-fraction-profile": 1e-4})
NOISE_SEED = 24
ON_BOUND = 1e-6
NOTEBOOK_FLOW = 0.000228
FL_FEEDS = (25, 30, 40)              # tried from the lowest
T_POSITIONS = (0.0, 5.0/19.0, 0.3, 0.62, 1.0)     # (5/19: node 5 of the 20)
PORT = ("DME", 0.5)
CASES = {
    "FC": {"base": "FA", "parameters": ["A1", "A3"], "start": [1.3, 0.7], "bounds": [[None, None], [None, 0.9]]},
    "FP": {"base": "FN", "parameters": ["A1", "A3"], "start": [1.3, 0.7]},
    "FL": {"base": "FB", "parameters": ["A1", "A2", "A3"], "start": [1.3, 1.4, 0.7], "scale": "log",
           "bounds": [[0.13, 13.0], [0.14, 14.0], [0.07, 7.0]]},
}

def interpolate(q, pos):
    """(1-f) q[n0] + f q[n0+1] with n0 = min(floor(pos (N-1)), N-2), f = pos (N-1) - n0"""
    N = len(q)
    n0 = min(int(np.floor(pos*(N - 1))), N - 2)
    f = pos*(N - 1) - n0
    return (1.0 - f)*q[n0] + f*q[n0 + 1]


def extras(name, e):
    """what experiment e of a case measures along the bed: [(kind, component or None, position)]"""
    if name != "FP":
        return []
    return [("temperature-profile", None, z) for z in T_POSITIONS] + [("mole-fraction-profile",) + PORT]


def ext_labels(name, e):
    return FR.labels(e) + [k + ":" + ("%s:" % c if c else "") + "%g" % z for k, c, z in extras(name, e)]


def ext_sigmas(name, e):
    return np.concatenate([FR.sigmas(e), [SIGMA[k] for k, _, _ in extras(name, e)]])


def conditions(feed=None):
    """fit_ref.conditions(), at ``feed`` times the notebook's feed rate when given"""
    out = FR.conditions()
    if feed is not None:
        out = [FR.deep_merge(c, {"feed": {"volumetric-flowrate": feed*NOTEBOOK_FLOW}}) for c in out]
    return out


class Reference(FR.Reference):
    """fit_ref.Reference with the conditions of a feed rate and the quantities along the bed of a case"""

    def __init__(self, O, names, case="FC", feed=None, log=None):
        self.O, self.names, self.log, self.case = O, list(names), log, case
        base = FR.base_input()
        self.prs = [dict(O.setup_n2(FR.deep_merge(base, c), zNo=ZNO)) for c in conditions(feed)]
        self.last = [None]*len(self.prs)
        self.cold = None
        self.worst = 0.0
        self.solves = 0

    def predict_one(self, e, y):
        out = list(FR.Reference.predict_one(self, e, y))
        pr = self.prs[e]
        S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
        Y = np.reshape(y, (V, N))
        c = np.maximum(Y[:S], 1e-30)*np.max(pr["SpCoi0"])
        x = c/c.sum(axis=0)
        T = Y[S]*pr["Tf"] + pr["Tf"]
        for kind, comp, z in extras(self.case, e):
            out.append(interpolate(T if comp is None else x[pr["compList"].index(comp)], z))
        return np.array(out)

    def residual(self, p, measured, keep=True):
        try:
            pred = self.predict(p, keep)
        except RuntimeError:            # no steady state there: a residual no trial is accepted with
            return np.full(sum(len(ext_labels(self.case, e)) for e in range(len(self.prs))), 1e3)
        return np.concatenate([(pr - np.asarray(m)[:len(pr)])/ext_sigmas(self.case, e)
                               for e, (pr, m) in enumerate(zip(pred, measured))])


def box(name):
    """(lo [P], hi [P]) of a case in the units of p, -inf / +inf where open"""
    case = CASES[name]
    pt = FR.p_true(case["base"])
    start = np.array(case["start"])*pt
    rel = case.get("bounds") or [[None, None]]*len(pt)          # (in parts of p_true; FL: [start/10, 10 start])
    lo = np.array([-np.inf if a is None else a*r for (a, _), r in zip(rel, pt)])
    hi = np.array([np.inf if b is None else b*r for (_, b), r in zip(rel, pt)])
    return lo, hi


def summary(ref, x, measured, free):
    """cost, J^T J, covariance over the free parameters (NaN rows and columns elsewhere), Marquardt-scaled cond(H_free)"""
    J, r = ref.jacobian(x, measured), ref.residual(x, measured)
    H = J.T @ J
    cost = 0.5*float(r @ r)
    idx = np.nonzero(free)[0]
    Hf = H[np.ix_(idx, idx)]
    d = np.sqrt(np.diag(Hf))
    cond = float(np.linalg.cond(Hf/np.outer(d, d)))
    cov = np.full(H.shape, np.nan)
    M, P = len(r), len(idx)
    if M > P:
        cov[np.ix_(idx, idx)] = 2*cost/(M - P)*np.linalg.inv(Hf)
    return {"cost": cost, "hessian": H, "covariance": cov, "cond": cond, "residual": r, "gradient": J.T @ r}


def reference_fit(ref, name, measured, log=None):
    """scipy's bounded fit of a case on ``measured``, polished on the face it ends on: dict(p_ref, active, cost, hessian,
    covariance, cond, nfev)"""
    import scipy.optimize
    case = CASES[name]
    pt = FR.p_true(case["base"])
    x0 = np.array(case["start"])*pt
    lo, hi = box(name)
    ref.last = list(ref.cold)
    kw = dict(method="trf", x_scale="jac", ftol=1e-14, xtol=1e-14, gtol=1e-14)
    sol = scipy.optimize.least_squares(lambda p: ref.residual(p, measured), x0, jac=lambda p: ref.jacobian(p, measured),
                                       bounds=(lo, hi), max_nfev=40, **kw)
    x, nfev = sol.x.copy(), int(sol.nfev)
    g = ref.jacobian(x, measured).T @ ref.residual(x, measured)
    active = np.zeros(len(x), dtype=int)
    for j in range(len(x)):
        if np.isfinite(hi[j]) and hi[j] - x[j] <= ON_BOUND*abs(hi[j]) and g[j] < 0:
            active[j], x[j] = 1, hi[j]
        elif np.isfinite(lo[j]) and x[j] - lo[j] <= ON_BOUND*abs(lo[j]) and g[j] > 0:
            active[j], x[j] = -1, lo[j]
    if log:
        log("%s: trf ends at %s after %d evaluations (status %d), active %s" % (name, sol.x, nfev, sol.status, active))
    free = active == 0
    if np.any(~free) and np.any(free):
        idx = np.nonzero(free)[0]

        def lift(z):
            p = x.copy()
            p[idx] = z
            return p
        pol = scipy.optimize.least_squares(lambda z: ref.residual(lift(z), measured), x[idx],
                                           jac=lambda z: ref.jacobian(lift(z), measured)[:, idx], max_nfev=30, **kw)
        x, nfev = lift(pol.x), nfev + int(pol.nfev)
    out = summary(ref, x, measured, free)
    out.update(p_ref=x, active=active, nfev=nfev)
    for j in np.nonzero(~free)[0]:
        if not out["gradient"][j]*active[j] < 0:
            raise SystemExit("G24 %s: the gradient at the polished point does not push parameter %d against its bound" % (name, j))
    return out


def law_fit(ref, names, measured, start, lo, hi, log_scale, max_iterations=30, tolerance=1e-8, damping=1e-3, log=None):
    """The product's numpy law (rmt_app_amd.fit.emulate_update_ex; the plain emulate_update when nothing is log-scaled or
    bounded) around the oracle's residuals and central-difference Jacobian: dict(values, converged, iterations, history)."""
    from rmt_app_amd import fit
    P = len(names)
    flags = [1 if log_scale else 0]*P
    plain = not log_scale and not np.any(np.isfinite(lo)) and not np.any(np.isfinite(hi))
    bx = fit.box(lo, hi, flags)
    state, at, hist = np.zeros(fit.STATE), np.asarray(start, dtype=float), []
    for k in range(max_iterations):
        s = np.zeros(fit.CONTRIB)
        r = ref.residual(at, measured)
        s[0] = 0.5*float(r @ r)
        failed = bool(np.all(r == 1e3))
        s[fit.CONTRIB - 1] = 1.0 if failed else 0.0
        if not failed and (k == 0 or s[0] < state[1]):           # (g and H are read only when the trial is accepted)
            J = ref.jacobian(at, measured)
            if log_scale:
                J = J*at[None, :]
            s[1:1 + P] = J.T @ r
            H = J.T @ J
            for a in range(P):
                for b in range(a, P):
                    s[1 + 8 + fit.tri(a, b)] = H[a, b]
        row = fit.emulate_update(s, state, P, start, tolerance, damping) if plain \
            else fit.emulate_update_ex(s, state, P, start, tolerance, damping, flags, bx)
        hist.append(row)
        if log:
            log("law pass %d: trial cost %.6e, current %.6e, lambda %.2e, accepted %d, trial %s"
                % (k, row[0], row[1], row[2], row[4], row[fit.LOG_PTRIAL:fit.LOG_PTRIAL + P]))
        if row[5] != 0.0 or row[7] != 0.0:
            break
        at = row[fit.LOG_PTRIAL:fit.LOG_PTRIAL + P].copy()
    last = hist[-1]
    return {"values": last[fit.LOG_PCUR:fit.LOG_PCUR + P].copy(), "converged": bool(last[5]), "status": int(last[7]),
            "iterations": len(hist), "history": np.array(hist)}


def run_case(O, name, log=None):
    """The golden of FC or FP (refusals as SystemExit)."""
    case = CASES[name]
    base = case["base"]
    ref = Reference(O, case["parameters"], name, None, log)
    pt = FR.p_true(base)
    ref.last = list(np.load(os.path.join(GOLD, "g22_fit_states.npz"))["states"])
    truth = ref.predict(pt, keep=True, gate=True)
    ref.cold = list(ref.last)
    ref.predict(np.array(case["start"])*pt, keep=False, gate=True)
    g22 = FR.golden(base)
    measured = []
    rng = np.random.default_rng(NOISE_SEED)
    for e, t in enumerate(truth):
        n = len(FR.labels(e))
        old = np.asarray(g22["measured"][e][:n])
        new = t[n:] + rng.standard_normal(len(t) - n)*ext_sigmas(name, e)[n:]
        measured.append(np.concatenate([old, new]))
    out = reference_fit(ref, name, measured, log)
    if out["cond"] > FR.COND_CAP:
        raise SystemExit("G24 %s: Marquardt-scaled cond(H) = %.3e exceeds %.0e" % (name, out["cond"], FR.COND_CAP))
    if not ref.worst <= FR.CR.GATE:
        raise SystemExit("G24 %s: a steady state ends at max|f| = %.3e, above the gate" % (name, ref.worst))
    lo, hi = box(name)
    return {"measured": FR.pad(measured), "predicted_true": FR.pad(truth), "p_ref": out["p_ref"], "active": out["active"],
            "p_ref_noise_free": np.asarray(g22["p_ref_noise_free"]), "cost": out["cost"], "hessian": out["hessian"],
            "covariance": out["covariance"], "cond": out["cond"], "residual_gate": ref.worst, "lo": lo, "hi": hi,
            "nfev": out["nfev"]}


def run_fl(O, feed, log=None):
    """One candidate of FL at ``feed`` times the notebook's feed rate: the golden's entries, or SystemExit when the
    log-scaled bounded law does not reach p_true within fit_ref.TRUE_CAP in at most 30 iterations."""
    case = CASES["FL"]
    names = case["parameters"]
    pt = FR.p_true("FB")
    start = np.array(case["start"])*pt
    lo, hi = box("FL")
    ref = Reference(O, names, "FL", feed, log)
    truth = ref.predict(pt, keep=True, gate=True)
    ref.cold = list(ref.last)
    fitted = law_fit(ref, names, truth, start, lo, hi, True, log=log)
    rel = np.abs(fitted["values"] - pt)/pt
    if not (fitted["converged"] and np.all(rel <= FR.TRUE_CAP)):
        raise SystemExit("G24 FL at %gx feed: the log-scaled bounded law ends at %s (p / p_true) after %d iterations, "
                         "converged %s, status %d - not written" % (feed, fitted["values"]/pt, fitted["iterations"],
                                                                    fitted["converged"], fitted["status"]))
    return {"measured": FR.pad(truth), "predicted_true": FR.pad(truth), "p_ref": fitted["values"],
            "p_ref_noise_free": fitted["values"], "iterations": fitted["iterations"], "feed": float(feed),
            "lo": lo, "hi": hi, "residual_gate": ref.worst, "history": fitted["history"]}


def meta():
    with open(os.path.join(GOLD, "g24_fit_ext.json")) as f:
        return json.load(f)


def golden(name):
    return np.load(os.path.join(GOLD, "g24_fit_ext_%s.npz" % name))


def have(name):
    return os.path.exists(os.path.join(GOLD, "g24_fit_ext_%s.npz" % name))


def measured_entry(name, e, values):
    """the "measured" dict of experiment e of a case from its vector"""
    n = len(FR.labels(e))
    out = FR.measured_entry(e, values[:n])
    prof, ports = {"position": [], "value": []}, {}
    for (kind, comp, z), v in zip(extras(name, e), values[n:]):
        d = prof if comp is None else ports.setdefault(comp, {"position": [], "value": []})
        d["position"].append(float(z))
        d["value"].append(float(v))
    if prof["position"]:
        out["temperature-profile"] = prof
    if ports:
        out["mole-fraction-profile"] = ports
    return out


def case_input(name, plain=False, **fit_cfg):
    """the modelInput of a G24 case; ``plain``: without "scale" and "bounds" """
    case = CASES[name]
    g = golden(name)
    mi = FR.base_input()
    pt = FR.p_true(case["base"])
    for nm, s, t in zip(case["parameters"], case["start"], pt):
        mi["reaction-rates"]["VARS"][nm] = s*t
    feed = float(g["feed"]) if "feed" in g.files else None
    exps = []
    for e, cond in enumerate(conditions(feed)):
        m = g["measured"][e][:len(ext_labels(name, e))]
        exps.append({"conditions": cond, "measured": measured_entry(name, e, m), "sigma": dict(SIGMA)})
    params = []
    for j, nm in enumerate(case["parameters"]):
        entry = {"rate-constant": nm}
        if not plain:
            if case.get("scale"):
                entry["scale"] = case["scale"]
            lo, hi = float(g["lo"][j]), float(g["hi"][j])
            if np.isfinite(lo) or np.isfinite(hi):
                entry["bounds"] = [lo if np.isfinite(lo) else None, hi if np.isfinite(hi) else None]
        params.append(entry)
    mi["solver-config"]["fit"] = dict({"parameters": params, "experiments": exps}, **fit_cfg)
    return mi
