"""What the policy tests share (tests/test_campaign_policy_cpu.py, tests/test_gpu_campaign_policy.py) and what
tools/make_golden.py (target ``policy``) runs: the reference of solver-config "deactivation" "policy" on the unchanged
oracle, and the goldens G20.

Nothing of the product is imported.  Per step the coolant level T that holds the outlet mole fraction of one component at
its target is found with scipy.optimize.brentq on

    r(T) = x_c,outlet(T) - target,

every value of r a steady state of profile_ref.profiled_rhs with the uniform coolant offset delta = T - MeTe added to the
zones' own (campaign_ref.steady_state: scipy.optimize.root from the nearest state known so far, brought close with a tight
root first; above the gate of G17 the LSODA legs of G17), xtol = 1e-10 K.  The saturation rule is restated: when r(lo) and r(hi) have no opposite signs
the limit with the smaller |r| is taken (a tie: lo).  The activities then move with campaign_ref.law_update at the node
temperatures of the accepted state.

A case is REFUSED when a steady state ends above the gate, when r sampled at 9 equidistant levels across the limits
changes sign more than once in a step (several roots), or when two adjacent samples differ by more than 20 times the
median difference (a branch jump inside the limits).
"""
import json
import os

import numpy as np
import scipy.optimize

import campaign_ref as CR
import profile_ref as PR

GOLD = CR.GOLD
XTOL = 1e-10             # K
SAMPLES = 9
JUMP = 20.0
LAW_DA = CR.CASES["DA"]["law"]
CASES = {
    # interior root throughout
    "PA": {"input": "dme_nb", "zNo": 20, "steps": 2, "time-on-stream": [1e6, 2e6], "law": LAW_DA,
           "policy": {"hold": "outlet-mole-fraction", "component": "DME", "target": 0.0150,
                      "manipulated": "medium-temperature", "limits": [503.0, 543.0]}},
    # PA with a tighter lower limit: the level of PA falls through 531.85 K between steps 2 and 3, so the coolant reaches
    # its limit before the last step and "end-of-run" is set
    "PS": {"input": "dme_nb", "zNo": 20, "steps": 2, "time-on-stream": [1e6, 2e6], "law": LAW_DA,
           "policy": {"hold": "outlet-mole-fraction", "component": "DME", "target": 0.0150,
                      "manipulated": "medium-temperature", "limits": [531.85, 543.0]}},
    # bed A of G18 (graded activity, two coolant zones): the policy moves the common level, the zones keep their offsets
    "PB": {"input": "dme_nb", "zNo": 20, "steps": 2, "time-on-stream": [1e6, 2e6], "axial-profile": "G18-A",
           "start": "G18-S", "law": LAW_DA,
           "policy": {"hold": "outlet-mole-fraction", "component": "DME", "target": 0.0150,
                      "manipulated": "medium-temperature", "limits": [503.0, 543.0]}},
}


def meta():
    with open(os.path.join(GOLD, "g20_policy.json")) as f:
        return json.load(f)


def golden(name):
    return np.load(os.path.join(GOLD, "g20_policy_%s.npz" % name))


def case_of(name):
    """the case as the golden was made from it (the json records the settled constants)"""
    return meta()["cases"][name]


def case_input(name, **cfg):
    """the modelInput of a golden case"""
    import inputs as INP
    case = case_of(name)
    mi = INP.ALL_N2_INPUTS[case["input"]]()
    mi["model"] = "N2"
    mi["solver-config"].update({"quiet": True, "zNo": case["zNo"], "display-result": "False"})
    mi["solver-config"]["deactivation"] = {"time-on-stream": list(case["time-on-stream"]), "steps": case["steps"],
                                           **case["law"], "policy": dict(case["policy"])}
    if CR.profile_spec(case):
        mi["solver-config"]["axial-profile"] = CR.profile_spec(case)
    mi["solver-config"].update(cfg)
    return mi


def outlet_fraction(y, pr, index):
    S, N = pr["compNo"], pr["zNo"]
    c = np.reshape(y, (pr["varNo"], N))[:S, -1]
    return float(c[index]/np.sum(c))


def slope(gold, k):
    """|dr/dT| of step k from the golden's own samples: the sample interval that holds the accepted level"""
    T, r = gold["sample_levels"], gold["samples"][k]
    i = int(np.clip(np.searchsorted(T, gold["level"][k], side="right") - 1, 0, len(T) - 2))
    return abs(float(r[i + 1] - r[i])/float(T[i + 1] - T[i]))


def level_bound(gold, k, state_bound):
    """state_bound / |dr/dT|: an error of state_bound in the held mole fraction moves the root by this much"""
    return state_bound/slope(gold, k)


class Bed:
    """r(T) of one step: the bed with activities ``a`` and zone offsets ``delta``, every steady state started from the
    nearest one known so far"""

    def __init__(self, O, pr, a, delta, target, index, known, log=None):
        self.O, self.pr, self.a, self.delta, self.target, self.index, self.log = O, pr, a, delta, target, index, log
        self.known = list(known)          # [(T, y)]
        self.solved = {}                  # T -> (y, r, max|f|, legs)
        self.worst, self.legs = 0.0, 0

    def __call__(self, T):
        T = float(T)
        if T not in self.solved:
            start = min(self.known, key=lambda ty: abs(ty[0] - T))[1]
            f = PR.profiled_rhs(self.O, self.pr, self.a, self.delta + (T - self.pr["Tm"]))
            # (root with its default tolerance ends a few K away from its start at max|f| = 2e-9 .. 6e-9, above the gate,
            # and steady_state would go through the LSODA legs for every value of r: the start is brought close first)
            near = scipy.optimize.root(lambda v: f(0.0, v), start, tol=1e-14).x
            if np.all(np.isfinite(near)):
                start = near
            y, res, legs = CR.steady_state(f, start, self.pr["IV"], self.log)
            if not res <= CR.GATE:
                raise SystemExit("the steady state at %.6f K ends at max|f| = %.3e, above the gate %.1e: the case is refused"
                                 % (T, res, CR.GATE))
            self.worst, self.legs = max(self.worst, res), self.legs + (1 if legs else 0)
            self.known.append((T, y))
            self.solved[T] = (y, outlet_fraction(y, self.pr, self.index) - self.target)
        return self.solved[T][1]

    def state(self, T):
        return self.solved[float(T)][0]


def check_samples(levels, r, where):
    """the two refusal rules on the 9 samples of a step"""
    signs = np.sign(r)
    changes = int(np.sum(signs[1:]*signs[:-1] < 0))
    if changes > 1:
        raise SystemExit("%s: r changes sign %d times across the limits (several roots): the case is refused; r = %s"
                         % (where, changes, np.array2string(r, precision=3)))
    d = np.abs(np.diff(r))
    if np.any(d > JUMP*np.median(d)):
        raise SystemExit("%s: adjacent samples differ by %.3e, more than %g x the median %.3e (a branch jump inside the "
                         "limits): the case is refused; r = %s" % (where, d.max(), JUMP, np.median(d),
                                                                 np.array2string(r, precision=3)))


def run_case(O, INP, case, log=None):
    """The reference run of a case: dict(times [K+1], marks, activity [K+1][N], states [n_out][V*N], level [K+1], held
    [K+1], saturated [K+1], sample_levels [9], samples [K+1][9], residual [K+1], delta [N])."""
    import scipy.optimize
    pr = dict(O.setup_n2(INP.ALL_N2_INPUTS[case["input"]](), zNo=case["zNo"]))
    N = case["zNo"]
    spec = CR.profile_spec(case)
    a, delta = PR.bed(spec, N, pr["Tm"]) if spec else (np.ones(N), np.zeros(N))
    times, marks = CR.step_times(case["time-on-stream"], case["steps"])
    pol = case["policy"]
    lo, hi = (float(v) for v in pol["limits"])
    target = float(pol["target"])
    index = list(INP.ALL_N2_INPUTS[case["input"]]()["feed"]["components"]["shell"]).index(pol["component"])
    if case.get("start") == "G18-S":
        y = np.array(PR.golden("S")["state"], dtype=float)
    else:
        y = np.array(np.load(os.path.join(GOLD, "g17_steady_%s.npz" % case["input"]))["state"], dtype=float)
    known = [(float(pr["Tm"]), y)]
    grid = np.linspace(lo, hi, SAMPLES)
    acts, states, level, held, sat, samples, resid = [], [], [], [], [], [], []
    for k, t in enumerate(times):
        bed = Bed(O, pr, a, delta, target, index, known, log)
        for T in sorted(grid, key=lambda v: abs(v - known[0][0])):       # outwards from the state that is known
            bed(T)
        r = np.array([bed(T) for T in grid])
        check_samples(grid, r, "step %d" % k)
        rlo, rhi = bed(lo), bed(hi)
        if lo == hi or not rlo*rhi < 0.0:
            Tk = hi if (lo != hi and abs(rhi) < abs(rlo)) else lo
            s = 1 if Tk == hi and lo != hi else -1
        else:
            Tk = float(scipy.optimize.brentq(bed, lo, hi, xtol=XTOL, rtol=4*np.finfo(float).eps))
            bed(Tk)
            s = 0
        yk = bed.state(Tk)
        if log:
            Tn = CR.temperatures(yk, pr)
            log("step %d t = %.4g s: level %.6f K, held %.10f (target %g), saturated %d, %d steady states (max|f| <= %.3e, "
                "%d with LSODA legs), activity %.4f .. %.4f, peak T %.2f K at node %d; r = %s"
                % (k, t, Tk, bed(Tk) + target, target, s, len(bed.solved), bed.worst, bed.legs, a.min(), a.max(), Tn.max(),
                   int(np.argmax(Tn)), np.array2string(r, precision=3)))
        acts.append(a.copy())
        level.append(Tk)
        held.append(bed(Tk) + target)
        sat.append(s)
        samples.append(r)
        resid.append(bed.worst)
        if k in marks:
            states.append(yk.copy())
        if k + 1 < len(times):
            a = CR.law_update(a, CR.temperatures(yk, pr), times[k + 1] - t, case["law"])
        known = [(Tk, yk)]
    return {"times": times, "marks": marks, "activity": np.array(acts), "states": np.array(states),
            "level": np.array(level), "held": np.array(held), "saturated": np.array(sat, dtype=np.int64),
            "sample_levels": grid, "samples": np.array(samples), "residual": np.array(resid), "delta": delta}
