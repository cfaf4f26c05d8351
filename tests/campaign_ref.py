"""What the campaign tests share (tests/test_campaign_cpu.py, tests/test_gpu_campaign.py) and what tools/make_golden.py
(target ``campaign``) runs: the reference of solver-config "deactivation" on the unchanged oracle, and the goldens G19.

Nothing of the product is imported.  The law is restated in numpy in its textbook form,

    b = max(a - a_inf, 0);   m == 1: b <- b exp(-k_d dt);   else: b <- b (1 + (m-1) k_d dt b^(m-1))^(-1/(m-1)),
    k_d(T) = k_ref exp(-(Ed/R)(1/T - 1/Tref)),   T = Tf (1 + theta_n)   (the inlet temperature in an iso-thermal run),

and every steady state f(y; a) = 0 comes from scipy.optimize.root on profile_ref.profiled_rhs, started from the previous
step's state.  When max|f| stays above the gate of G17 the recipe of G17 comes first: LSODA legs from the cold start until
max|f| stops falling, then root.  A case in which any step ends above the gate is refused.
"""
import json
import os

import numpy as np

import profile_ref as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R_GAS = 8.314472
GATE = 1e-9              # G17_GATE of tools/make_golden.py
CHUNK, T_MAX = 10.0, 400.0
OUT4 = [5e5, 1e6, 1.5e6, 2e6]
CASES = {
    # plain bed
    "DA": {"input": "dme_nb", "zNo": 20, "steps": 4, "time-on-stream": OUT4,
           "law": {"rate-constant": 2e-7, "activation-energy": 8.0e4, "reference-temperature": 623.0, "order": 1.0,
                   "residual-activity": 0.0}},
    # bed A of G18 (graded activity, two coolant zones), started from its golden steady state S
    "DB": {"input": "dme_nb", "zNo": 20, "steps": 4, "time-on-stream": OUT4, "axial-profile": "G18-A", "start": "G18-S",
           "law": {"rate-constant": 6e-7, "activation-energy": 1.2e5, "reference-temperature": 623.0, "order": 2.0,
                   "residual-activity": 0.2}},
    # the hot spot travels to the outlet and the bed dies
    "DC": {"input": "dme_nb", "zNo": 20, "steps": 4, "time-on-stream": [5e5, 1e6, 1.5e6, 2e6, 2.5e6, 3e6],
           "law": {"rate-constant": 2e-6, "activation-energy": 8.0e4, "reference-temperature": 623.0, "order": 1.0,
                   "residual-activity": 0.0}},
    # iso-thermal bed with an activity ramp: the law has a closed form
    "DI": {"input": "dme_nb", "process-type": "iso-thermal", "zNo": 20, "steps": 5,
           "time-on-stream": [2.5e5, 5e5, 7.5e5, 1e6],
           "axial-profile": {"position": [0.0, 1.0], "catalyst-activity": [0.5, 1.0]},
           "law": {"rate-constant": 1e-6, "activation-energy": 8.0e4, "reference-temperature": 623.0, "order": 1.0,
                   "residual-activity": 0.0}},
}
LAW_KEYS = ("rate-constant", "activation-energy", "reference-temperature", "order", "residual-activity")


def meta():
    with open(os.path.join(GOLD, "g19_campaign.json")) as f:
        return json.load(f)


def golden(name):
    return np.load(os.path.join(GOLD, "g19_campaign_%s.npz" % name))


def profile_spec(case):
    """the "axial-profile" of a case as the input takes it (None: the plain bed)"""
    spec = case.get("axial-profile")
    return dict(PR.BED_A) if spec == "G18-A" else spec


def case_input(name, steps=None, model="N2", **cfg):
    """the modelInput of a golden case"""
    import inputs as INP
    case = CASES[name]
    kw = {"process_type": case["process-type"]} if "process-type" in case else {}
    mi = INP.ALL_N2_INPUTS[case["input"]](**kw)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": case["zNo"], "display-result": "False"})
    mi["solver-config"]["deactivation"] = {"time-on-stream": list(case["time-on-stream"]), "steps": steps or case["steps"],
                                           **case["law"]}
    if profile_spec(case):
        mi["solver-config"]["axial-profile"] = profile_spec(case)
    mi["solver-config"].update(cfg)
    return mi


def activity_bound(case, gold, Tf, V, N, state_bound):
    """2 x state_bound x Ed/(R T_min) x ln(a_0/a_min), from the golden: the first-order propagation of a temperature error
    through the law, doubled for the feedback"""
    T = gold["states"].reshape(-1, V, N)[:, -1]*Tf + Tf
    a = gold["activity"]
    return 2*state_bound*case["law"]["activation-energy"]/(R_GAS*float(T.min()))*np.log(float(a[0].max())/float(a.min()))


def step_times(outputs, steps):
    """every step time, 0 first, and the index of every output time (restated)"""
    times, marks, t = [0.0], [], 0.0
    for out in outputs:
        if out > t:
            times += [t + (out - t)*j/steps for j in range(1, steps)] + [float(out)]
            t = float(out)
        marks.append(len(times) - 1)
    return np.array(times), np.array(marks)


def law_update(a, T, dt, law):
    """the frozen-temperature exact solution over dt, textbook form"""
    k, ed, tref, m, ainf = (float(law[key]) for key in LAW_KEYS)
    a = np.asarray(a, dtype=float)
    kd = k*np.exp(-(ed/R_GAS)*(1.0/np.asarray(T, dtype=float) - 1.0/tref))
    b = np.maximum(a - ainf, 0.0)
    if m == 1.0:
        bn = b*np.exp(-kd*dt)
    else:
        bn = b*(1.0 + (m - 1.0)*kd*dt*b**(m - 1.0))**(-1.0/(m - 1.0))
    return np.where(a > ainf, ainf + bn, a)


def temperatures(y, pr):
    """T_n [K] of a state [V*N]"""
    S, N = pr["compNo"], pr["zNo"]
    if pr["iso"]:
        return np.full(N, float(pr["Tf"]))
    return pr["Tf"]*(1.0 + np.reshape(y, (pr["varNo"], N))[S])


def steady_state(f, start, cold, log=None):
    """(state, max|f|, LSODA legs used) of f(0, y) = 0: root from ``start``; when that ends above the gate the recipe of G17
    as tools/make_golden.py g17_state has it - LSODA legs from the cold start ``cold`` (the oracle's IV) until max|f| stops
    falling, then root.  Where a node has two steady states the fallback therefore lands on the one the cold start reaches,
    root alone on the one next to ``start``."""
    import scipy.integrate
    import scipy.optimize
    res = lambda v: float(np.max(np.abs(f(0.0, v))))
    sol = scipy.optimize.root(lambda v: f(0.0, v), start)
    y = np.array(sol.x, dtype=float)
    if np.all(np.isfinite(y)) and res(y) <= GATE:
        return y, res(y), 0
    y, t, prev, legs = np.array(cold, dtype=float), 0.0, np.inf, 0
    while t < T_MAX:
        s = scipy.integrate.solve_ivp(f, (t, t + CHUNK), y, method="LSODA", rtol=1e-10, atol=1e-13)
        if not s.success:
            raise RuntimeError(s.message)
        y, t, legs = s.y[:, -1], t + CHUNK, legs + 1
        r = res(y)
        if log:
            log("  LSODA leg to t = %.0f s: max|f| = %.3e" % (t, r))
        if not r < 0.5*prev:
            break
        prev = r
    best, r_best = y, res(y)
    sol = scipy.optimize.root(lambda v: f(0.0, v), y)
    if np.all(np.isfinite(sol.x)) and res(sol.x) < r_best:
        best, r_best = np.array(sol.x, dtype=float), res(sol.x)
    return best, r_best, legs


def run_case(O, INP, case, steps=None, log=None):
    """The reference campaign of a case: dict(times [K+1], marks, activity [K+1][N], states [n_out][V*N], residual [K+1],
    legs [K+1], delta [N]).  ``steps`` overrides the case's steps per interval (the order test's fine reference)."""
    kw = {"process_type": case["process-type"]} if "process-type" in case else {}
    pr = dict(O.setup_n2(INP.ALL_N2_INPUTS[case["input"]](**kw), zNo=case["zNo"]))
    N = case["zNo"]
    spec = profile_spec(case)
    a, delta = PR.bed(spec, N, pr["Tm"]) if spec else (np.ones(N), np.zeros(N))
    times, marks = step_times(case["time-on-stream"], steps or case["steps"])
    start = case.get("start")
    if start == "G18-S":
        y = np.array(PR.golden("S")["state"], dtype=float)
    elif not pr["iso"]:
        y = np.array(np.load(os.path.join(GOLD, "g17_steady_%s.npz" % case["input"]))["state"], dtype=float)
    else:
        y = np.array(pr["IV"], dtype=float)
    acts, states, resid, legs = [], [], [], []
    for k, t in enumerate(times):
        y, r, n = steady_state(PR.profiled_rhs(O, pr, a, delta), y, pr["IV"], log)
        if log:
            log("step %d t = %.4g s: max|f| = %.3e (%d LSODA legs), activity %.4f .. %.4f, peak T %.2f K at node %d"
                % (k, t, r, n, a.min(), a.max(), temperatures(y, pr).max(), int(np.argmax(temperatures(y, pr)))))
        if not r <= GATE:
            raise SystemExit("step %d ends at max|f| = %.3e, above the gate %.1e: the case is refused" % (k, r, GATE))
        acts.append(a.copy())
        resid.append(r)
        legs.append(n)
        if k in marks:
            states.append(y.copy())
        if k + 1 < len(times):
            a = law_update(a, temperatures(y, pr), times[k + 1] - t, case["law"])
    return {"times": times, "marks": marks, "activity": np.array(acts), "states": np.array(states),
            "residual": np.array(resid), "legs": np.array(legs), "delta": delta}
