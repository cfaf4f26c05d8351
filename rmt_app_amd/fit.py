"""Kinetic parameter estimation from steady-state data (solver-config "fit").

    "fit": {"parameters": [{"rate-constant": "A1"}, {"rate-constant": "A3"}],      # 1..8 scalar reaction-rates.VARS entries
            "experiments": [{"conditions": {"external-heat": {"MeTe": 513.0}},     # merged over the base input, as a member
                             "measured": {"outlet-mole-fraction": {"DME": 0.0150, "CH3OH": 0.021},    # of a list "ensemble"
                                          "outlet-temperature": 521.4, "peak-temperature": 529.8},
                             "sigma": {"outlet-mole-fraction": 1e-4, "outlet-temperature": 0.5, "peak-temperature": 0.5}},
                            ...],
            "max-iterations": 30, "tolerance": 1e-8, "damping": 1e-3, "batch": 8}

* Absent: nothing of any run changes.  Model N2, fp64, one rank.  Like "deactivation" the run integrates nothing in time:
  it is a sequence of steady states of all experiments at once ("period", "tNo" and "ivp" are unused).
* Weighted non-linear least squares, cost = 1/2 sum r^2 with r = (predicted - measured)/sigma (sigma defaults to 1), by
  Levenberg-Marquardt with Marquardt's scaling D = diag(J^T J) and Nielsen's damping update.  The Jacobian is the analytic
  sensitivity sweep (sensitivity.py) with respect to the fitted constants, traced as per-reactor inputs.
* Per iteration three calls are queued back to back on ONE handle of the sensitivity unit - rmt_n2_steady_march,
  rmt_n2_steady_sens, rmt_n2_fit_step (csrc/fit_kernels.inc: the reduction over the experiments and the LM step, which
  writes the trial values into the device rows) - and nothing leaves the device inside a "batch" of iterations: the host
  reads the log once per batch, stops queuing at `converged` and queues one finishing pass, so that state, sensitivities,
  predictions and J^T J on the device are those of the accepted parameters.
* The starting values are the base input's VARS values; a fitted constant is ONE value for all experiments (an experiment
  whose "conditions" give it a value of its own raises).  Experiments may differ in what the members of an ensemble may.
* Result: the shape of a list-form ensemble run whose members are the experiments, one dataPack entry each (the steady
  state at the fitted values) and a "fit" entry {"labels", "measured", "predicted", "residual" (weighted)};
  resModel["fit"] = {"parameters", "initial", "values", "cost", "iterations", "converged", "history", "hessian" (J^T J at
  the optimum), "covariance" (s^2 H^-1, s^2 = 2 cost/(M - P); None when M <= P), "standard-error", "correlation",
  "experiments": M's count per experiment}.
* No convergence within "max-iterations" raises RuntimeError naming the iteration count, the last cost and the last
  parameters; so does a failed march at the accepted parameters.  There is no silent partial result.
* A parameter entry may carry "scale": "linear" (default) | "log" and "bounds": [lo, hi] in the units of p, either end None:
  {"rate-constant": "A3", "scale": "log", "bounds": [1e3, 1e7]}.  With "log" the law works in theta = ln p (the start must
  be > 0, a lower bound too).  Required: lo < hi and the start inside; everything else raises ValueError naming the parameter.
  The step is an active-set projected one (``emulate_update_ex``): no trial leaves the box.
* "measured" (and "sigma", a scalar each) may carry data along the bed, positions z/L in [0, 1] with the mesh nodes at
  n/(N-1): "temperature-profile": {"position": [0.1, 0.25], "value": [528.1, 531.0]} and "mole-fraction-profile":
  {"DME": {"position": [0.5], "value": [0.008]}} - node temperatures in K, node mole fractions of the clamped node state,
  interpolated linearly between the two nodes around the position.  Labels "temperature-profile:0.25",
  "mole-fraction-profile:DME:0.5".  At most 64 measured values per experiment in all.
* A spec with any of these keys runs rmt_n2_fit_step_ex (the sibling kernels of the same translation unit); one without runs
  rmt_n2_fit_step exactly as before.  resModel["fit"] also holds "scale", "bounds" [P][2] (+-inf where open) and
  "active-bounds" [P] (-1 / 0 / +1 at the accepted values); "hessian" and the statistics stay in the units of p
  (H_p = diag(1/p) H_theta diag(1/p) for a log parameter) and are formed over the free parameters: rows and columns of a
  parameter on a bound are NaN, M - P counts the free ones.
* Not built: boundary or activity parameters; dynamic data; robust losses; skipping the sensitivity launch after a
  rejected trial; multi-rank runs.

Host side only: parsing and validation, the measurement and position tables, the result entries, and numpy restatements of
the kernels (``emulate_residuals``, ``emulate_update`` and their extended siblings ``emulate_residuals_ex``,
``emulate_update_ex``) for the tests.
"""
import numpy as np

from .lowering import is_scalar_constant

KEY = "fit"
MODELS = ("N2",)
MAX_PARAMETERS = 8
MAX_EXPERIMENTS = 4096
MAX_QUANTITIES = 64
KEYS = ("parameters", "experiments", "max-iterations", "tolerance", "damping", "batch")
EXPERIMENT_KEYS = ("conditions", "measured", "sigma")
QUANTITIES = ("outlet-mole-fraction", "outlet-temperature", "peak-temperature")
PROFILES = ("temperature-profile", "mole-fraction-profile")         # measured along the bed: code S+2, S+3+species
PARAMETER_KEYS = ("rate-constant", "scale", "bounds")
SCALES = ("linear", "log")
DEFAULTS = {"max-iterations": 30, "tolerance": 1e-8, "damping": 1e-3, "batch": 8}
EXCLUSIVE = ("ensemble", "schedule", "control", "monitor", "initial", "sensitivity", "deactivation", "axial-profile")
RATE_CONSTANT = "rate-constant"
EPS = 1e-30                      # the clamp of the concentrations
FLOOR = 1e-300
# the device buffers (csrc/fit_kernels.inc)
CONTRIB, STATE, LOG, TRI = 46, 80, 68, 36
ST_PCUR, ST_PTRIAL, ST_G, ST_H, ST_DELTA = 8, 16, 24, 32, 68
FIRST_FAILED, NOT_POSITIVE = 1, 2
LOG_PTRIAL, LOG_PCUR, LOG_G, LOG_H = 8, 16, 24, 32
# the extended kernels: the log slice is two words wider and state words 76, 77 hold the same two - the parameters of the
# current point on their lower / upper bound, one bit each; the position table [E][MQ][2] = {n0, f}
LOG_EX, LOG_LOWER, LOG_UPPER, ST_LOWER, ST_UPPER = 70, 68, 69, 76, 77
MEMBER_USER = 16                 # + S: the first user column of a member row (RMT_FIT_M_USER)


def check_model(modelInput):
    """NotImplementedError when the input asks for a fit on a model that has none (rmtExe, before any device work)."""
    if (modelInput.get('solver-config') or {}).get(KEY) is not None and modelInput.get('model') not in MODELS:
        raise NotImplementedError("solver-config 'fit' is only available for model 'N2' (got model %r)"
                                  % (modelInput.get('model'),))


def tri(a, b):
    """index of (a, b), a <= b, in the upper triangle of an 8 x 8 matrix stored row by row"""
    return a*MAX_PARAMETERS - a*(a - 1)//2 + (b - a)


def full(tri36, P):
    """the symmetric [P][P] matrix of an upper triangle [36]"""
    H = np.zeros((P, P))
    for a in range(P):
        for b in range(a, P):
            H[a, b] = H[b, a] = tri36[tri(a, b)]
    return H


class Fit:
    """A parsed "fit" spec: ``names`` (the fitted VARS entries), ``labels``, ``experiments`` = per experiment the list of
    (label, code, value, sigma) with code = species index | S (outlet temperature) | S+1 (peak temperature), ``conditions``
    (the members' overrides), and the four numbers of the iteration."""

    def __init__(self, names, experiments, conditions, S, max_iterations, tolerance, damping, batch, scales=None,
                 bounds=None, positions=None):
        """``scales`` [P] of SCALES, ``bounds`` [P] of (lo, hi) in the units of p with -inf / +inf where open,
        ``positions`` per experiment the z/L of each entry (None for an outlet or peak quantity)"""
        self.names = list(names)
        self.scales = list(scales) if scales is not None else ["linear"]*len(self.names)
        bounds = bounds if bounds is not None else [(-np.inf, np.inf)]*len(self.names)
        self.lo, self.hi = (np.array([b[k] for b in bounds], dtype=np.float64) for k in (0, 1))
        self.positions = positions if positions is not None else [[None]*len(x) for x in experiments]
        self.flags = [1 if s == "log" else 0 for s in self.scales]
        # the extended kernels run only for a spec that uses one of the new keys
        self.extended = bool(any(self.flags) or np.any(np.isfinite(self.lo)) or np.any(np.isfinite(self.hi))
                             or any(z is not None for zs in self.positions for z in zs))
        self.labels = ["%s:%s" % (RATE_CONSTANT, nm) for nm in self.names]
        self.NP = len(self.names)
        self.experiments, self.conditions, self.S = experiments, conditions, int(S)
        self.E = len(experiments)
        self.MQ = max(len(x) for x in experiments)
        self.M = sum(len(x) for x in experiments)
        self.max_iterations, self.tolerance, self.damping, self.batch = max_iterations, tolerance, damping, batch

    def sensitivity(self):
        """the sensitivity.Sensitivity of the fitted constants (descriptors, unit_params, widen)"""
        from .sensitivity import KIND_USER, Sensitivity
        return Sensitivity([(KIND_USER, nm) for nm in self.names])

    def members(self, modelInput):
        """the experiments' modelInputs (the members of the list form of "ensemble")"""
        from .ensemble import expand_members
        return expand_members(modelInput, self.conditions)

    def table(self):
        """meas [E][MQ][3] = {code, value, weight = 1/sigma}, padded with weight 0"""
        out = np.zeros((self.E, self.MQ, 3))
        for e, qs in enumerate(self.experiments):
            for q, (_, code, value, sigma) in enumerate(qs):
                out[e, q] = code, value, 1.0/sigma
        return out

    def position_table(self, N):
        """pos [E][MQ][2] = {n0, f} of the entries measured along the bed (mesh nodes at n/(N-1)), zero elsewhere"""
        out = np.zeros((self.E, self.MQ, 2))
        for e, zs in enumerate(self.positions):
            for q, z in enumerate(zs):
                if z is not None:
                    out[e, q] = position(z, N)
        return out

    def box(self):
        """[4][8]: the bounds in p and in theta (``box``)"""
        return box(self.lo, self.hi, self.flags)

    def active_bounds(self, row):
        """[P] ints -1 / 0 / +1 from the two words of an extended log slice (all 0 from a plain one)"""
        lower, upper = (int(row[k]) if len(row) > k else 0 for k in (LOG_LOWER, LOG_UPPER))
        return np.array([(upper >> j & 1) - (lower >> j & 1) for j in range(self.NP)], dtype=np.int64)

    def bounds_text(self, row):
        """' (on its bound: A3 at the upper 7.4e4)' for the error texts, '' when no bound is active"""
        on = ["%s at the %s %.12g" % (nm, "upper" if a > 0 else "lower", self.hi[j] if a > 0 else self.lo[j])
              for j, (nm, a) in enumerate(zip(self.names, self.active_bounds(row))) if a]
        return " (on bounds: %s)" % ", ".join(on) if on else ""

    def columns(self, mech):
        """the user column of each fitted constant in the rows of ``mech``"""
        return [mech.params.index(nm) for nm in self.names]

    def member_entry(self, e, pred):
        """experiment e's own "fit" entry from its row of the prediction buffer"""
        qs = self.experiments[e]
        measured = np.array([v for _, _, v, _ in qs])
        weight = np.array([1.0/s for _, _, _, s in qs])
        predicted = np.asarray(pred, dtype=np.float64)[:len(qs)].copy()
        return {"labels": [lb for lb, _, _, _ in qs], "measured": measured, "predicted": predicted,
                "residual": (predicted - measured)*weight}

    def history(self, logs, initial):
        """resModel["fit"]["history"] from the log slices [n][LOG]: per iteration the parameters it evaluated, their cost,
        the current cost, lambda, accepted, the failed experiments - and the trial it queued"""
        out, at = [], np.asarray(initial, dtype=np.float64)
        for row in logs:
            out.append({"parameters": at.copy(), "trial-cost": float(row[0]), "cost": float(row[1]), "lambda": float(row[2]),
                        "accepted": bool(row[4]), "converged": bool(row[5]), "failed-experiments": int(row[6]),
                        "trial-parameters": row[LOG_PTRIAL:LOG_PTRIAL + self.NP].copy()})
            at = row[LOG_PTRIAL:LOG_PTRIAL + self.NP]
        return out

    def result_entry(self, logs, initial, last):
        """resModel["fit"]: ``logs`` [n][LOG] the iterations' slices, ``last`` [LOG] the finishing pass's (H at the
        optimum)"""
        P = self.NP
        values = last[LOG_PCUR:LOG_PCUR + P].copy()
        cost = float(last[1])
        H = full(last[LOG_H:LOG_H + TRI], P)
        entry = {"parameters": list(self.labels), "initial": np.asarray(initial, dtype=np.float64).copy(), "values": values,
                 "cost": cost, "iterations": len(logs), "converged": bool(last[5]), "history": self.history(logs, initial),
                 "hessian": H, "experiments": [len(x) for x in self.experiments]}
        active = self.active_bounds(last)
        entry.update({"scale": list(self.scales), "bounds": np.stack([self.lo, self.hi], axis=1), "active-bounds": active})
        if any(self.flags) or np.any(active):
            # the sums are in theta = ln p for a log parameter: H_p = diag(1/p) H_theta diag(1/p)
            s = np.array([1.0/v if f else 1.0 for v, f in zip(values, self.flags)])
            entry["hessian"] = H = H*np.outer(s, s)
            entry.update(statistics_free(H, cost, self.M, active == 0))
        else:
            entry.update(statistics(H, cost, self.M))
        return entry


def statistics(H, cost, M):
    """{"covariance": s^2 H^-1 with s^2 = 2 cost/(M - P), "standard-error", "correlation"}; all None when M <= P"""
    H = np.asarray(H, dtype=np.float64)
    P = H.shape[0]
    if M <= P:
        return {"covariance": None, "standard-error": None, "correlation": None}
    cov = 2.0*cost/(M - P)*np.linalg.inv(H)
    se = np.sqrt(np.diag(cov))
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = cov/np.outer(se, se)
    return {"covariance": cov, "standard-error": se, "correlation": corr}


def statistics_free(H, cost, M, free):
    """``statistics`` over the free parameters only: rows and columns of a parameter on a bound are NaN, M - P counts the
    free ones; all None when M <= their number (or none is free)"""
    H, idx = np.asarray(H, dtype=np.float64), np.nonzero(free)[0]
    st = statistics(H[np.ix_(idx, idx)], cost, M) if len(idx) else statistics(H, cost, 0)
    if st["covariance"] is None:
        return st
    P = H.shape[0]
    cov, corr, se = np.full((P, P), np.nan), np.full((P, P), np.nan), np.full(P, np.nan)
    cov[np.ix_(idx, idx)], corr[np.ix_(idx, idx)], se[idx] = st["covariance"], st["correlation"], st["standard-error"]
    return {"covariance": cov, "standard-error": se, "correlation": corr}


def position(z, N):
    """(n0, f) of z/L = z on a mesh of N nodes at n/(N-1): n0 = min(floor(z (N-1)), N-2), f = z (N-1) - n0"""
    n0 = min(int(np.floor(z*(N - 1))), N - 2)
    return float(n0), z*(N - 1) - n0


def box(lo, hi, flags):
    """[4][8] = {lo, hi in p; lo, hi in theta (ln of a log parameter's)}, -inf / +inf where open or unused - what the
    extended update kernel takes by value.  The logarithms are taken here, on the host, once."""
    out = np.empty((4, MAX_PARAMETERS))
    out[0::2], out[1::2] = -np.inf, np.inf
    P = len(flags)
    out[0, :P], out[1, :P] = lo, hi
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(P):
            out[2, j] = np.log(out[0, j]) if flags[j] and out[0, j] > 0 else out[0, j] if not flags[j] else -np.inf
            out[3, j] = np.log(out[1, j]) if flags[j] else out[1, j]
    return out


def _number(v, what, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError("solver-config 'fit': %s must be a finite number (got %r)" % (what, v))
    if positive and not v > 0:
        raise ValueError("solver-config 'fit': %s must be > 0 (got %r)" % (what, v))
    return float(v)


def _bounds(nm, scale, given, start):
    """(lo, hi) of a parameter entry in the units of p (-inf / +inf where open), or ValueError naming the parameter"""
    where = "solver-config 'fit': parameter %r" % nm
    if scale not in SCALES:
        raise ValueError("%s: 'scale' must be 'linear' or 'log' (got %r)" % (where, scale))
    if scale == "log" and not start > 0:
        raise ValueError("%s: 'scale': 'log' needs a starting value > 0 (VARS[%r] = %r)" % (where, nm, start))
    if given is None:
        return -np.inf, np.inf
    if not isinstance(given, (list, tuple)) or len(given) != 2:
        raise ValueError("%s: 'bounds' must be [lo, hi], either may be None (got %r)" % (where, given))
    lo, hi = (d if v is None else _number(v, "parameter %r: 'bounds'" % nm) for v, d in zip(given, (-np.inf, np.inf)))
    if not lo < hi:
        raise ValueError("%s: 'bounds' must be lo < hi (got %r)" % (where, list(given)))
    if not lo <= start <= hi:
        raise ValueError("%s: the starting value %r lies outside its 'bounds' %r" % (where, start, list(given)))
    if scale == "log" and given[0] is not None and not lo > 0:
        raise ValueError("%s: the lower bound of a 'log' parameter must be > 0 (got %r)" % (where, given[0]))
    return lo, hi


def _profile(d, what):
    """(positions, values) of a {"position": [...], "value": [...]} entry"""
    if not (isinstance(d, dict) and set(d) == {"position", "value"} and isinstance(d["position"], (list, tuple))
            and isinstance(d["value"], (list, tuple)) and len(d["position"]) == len(d["value"]) >= 1):
        raise ValueError("solver-config 'fit': %s must be a dict {'position': [z/L, ...], 'value': [...]} of equal, "
                         "non-zero lengths" % what)
    zs = [_number(z, "%s: a position" % what) for z in d["position"]]
    for z in zs:
        if not 0.0 <= z <= 1.0:
            raise ValueError("solver-config 'fit': %s: a position is z/L in [0, 1] (got %r)" % (what, z))
    return zs, [_number(v, "%s: a value" % what) for v in d["value"]]


def parse(modelInput, multi_rank=False):
    """The Fit of a run (None when the input has no "fit"), or ValueError / NotImplementedError naming the offending
    key - all before any device work."""
    cfg = modelInput['solver-config']
    spec = cfg.get(KEY)
    if spec is None:
        return None
    check_model(modelInput)
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'fit' must be a dict with the keys 'parameters' and 'experiments'")
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'fit': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    for k in EXCLUSIVE:
        if cfg.get(k) is not None:
            raise NotImplementedError("solver-config 'fit' is not available with %r: the run is a sequence of steady states "
                                      "of the experiments, nothing else" % (k,))
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise NotImplementedError("solver-config 'fit' is not available with 'dtype': 'fp32': march, sweep and the "
                                  "Levenberg-Marquardt step are fp64 kernels")
    if multi_rank:
        raise NotImplementedError("solver-config 'fit' is not available in a multi-rank run")
    plist = spec.get('parameters')
    if not isinstance(plist, (list, tuple)) or len(plist) < 1:
        raise ValueError("solver-config 'fit': 'parameters' must be a non-empty list of {'%s': VARS name}" % RATE_CONSTANT)
    if len(plist) > MAX_PARAMETERS:
        raise ValueError("solver-config 'fit': 'parameters' holds %d entries, at most %d are supported"
                         % (len(plist), MAX_PARAMETERS))
    VARS = modelInput['reaction-rates']['VARS']
    names, scales, bounds = [], [], []
    for p in plist:
        if not (isinstance(p, dict) and RATE_CONSTANT in p and all(k in PARAMETER_KEYS for k in p)):
            raise ValueError("solver-config 'fit': a parameter is a dict {'%s': VARS name} (got %r)" % (RATE_CONSTANT, p))
        nm = p[RATE_CONSTANT]
        if not isinstance(nm, str) or nm not in VARS:
            raise ValueError("solver-config 'fit': '%s': %r is not an entry of reaction-rates.VARS" % (RATE_CONSTANT, nm))
        if not is_scalar_constant(VARS[nm]):
            raise NotImplementedError("solver-config 'fit': '%s': VARS[%r] is not a scalar constant" % (RATE_CONSTANT, nm))
        if nm in names:
            raise ValueError("solver-config 'fit': duplicate parameter %r in 'parameters'" % (p,))
        names.append(nm)
        scales.append(p.get("scale", SCALES[0]))
        bounds.append(_bounds(nm, scales[-1], p.get("bounds"), float(VARS[nm])))
    exps = spec.get('experiments')
    if not isinstance(exps, (list, tuple)) or len(exps) < 1:
        raise ValueError("solver-config 'fit': 'experiments' must be a non-empty list")
    if len(exps) > MAX_EXPERIMENTS:
        raise ValueError("solver-config 'fit': 'experiments' holds %d entries, at most %d are supported"
                         % (len(exps), MAX_EXPERIMENTS))
    comps = list(modelInput['feed']['components']['shell'])
    S = len(comps)
    iso = modelInput['operating-conditions'].get('process-type') == "iso-thermal"
    experiments, conditions, positions = [], [], []
    for e, x in enumerate(exps):
        where = "experiment %d" % e
        if not isinstance(x, dict):
            raise ValueError("solver-config 'fit': %s must be a dict with the key 'measured'" % where)
        for k in x:
            if k not in EXPERIMENT_KEYS:
                raise ValueError("solver-config 'fit': %s: unknown key %r (known: %s)" % (where, k, ", ".join(EXPERIMENT_KEYS)))
        cond = x.get('conditions') or {}
        if not isinstance(cond, dict):
            raise ValueError("solver-config 'fit': %s: 'conditions' must be a dict merged over the base input" % where)
        own = (cond.get('reaction-rates') or {}).get('VARS') or {}
        for nm in names:
            if nm in own and (not is_scalar_constant(own[nm]) or float(own[nm]) != float(VARS[nm])):
                raise ValueError("solver-config 'fit': %s gives the fitted constant %r a value of its own in 'conditions': "
                                 "a fitted constant is one value for all experiments" % (where, nm))
        ptype = (cond.get('operating-conditions') or {}).get('process-type')
        if ptype is not None and (ptype == "iso-thermal") != iso:
            raise ValueError("solver-config 'fit': %s differs from the base input in operating-conditions.process-type" % where)
        measured, sigma = x.get('measured'), x.get('sigma') or {}
        if not isinstance(measured, dict) or not isinstance(sigma, dict):
            raise ValueError("solver-config 'fit': %s: 'measured' and 'sigma' must be dicts" % where)
        for d, what in ((measured, 'measured'), (sigma, 'sigma')):
            for k in d:
                if k not in QUANTITIES + PROFILES:
                    raise ValueError("solver-config 'fit': %s: unknown key %r in %r (known: %s)"
                                     % (where, k, what, ", ".join(QUANTITIES + PROFILES)))
        qs, zs = [], []
        xs = measured.get(QUANTITIES[0]) or {}
        if not isinstance(xs, dict):
            raise ValueError("solver-config 'fit': %s: '%s' must be a dict {component: value}" % (where, QUANTITIES[0]))
        sig = {k: _number(sigma.get(k, 1.0), "%s: 'sigma' of '%s'" % (where, k)) for k in QUANTITIES + PROFILES}
        for k, s in sig.items():
            if not s > 0:
                raise ValueError("solver-config 'fit': %s: 'sigma' of '%s' must be > 0 (got %r)" % (where, k, s))
        for comp, v in xs.items():
            if comp not in comps:
                raise ValueError("solver-config 'fit': %s: '%s': %r is not a shell component (%s)"
                                 % (where, QUANTITIES[0], comp, ", ".join(comps)))
            qs.append(("%s:%s" % (QUANTITIES[0], comp), comps.index(comp),
                       _number(v, "%s: '%s' of %r" % (where, QUANTITIES[0], comp)), sig[QUANTITIES[0]]))
        for n, k in enumerate(QUANTITIES[1:]):
            if measured.get(k) is not None:
                if iso:
                    raise ValueError("solver-config 'fit': %s measures '%s' in an iso-thermal run: there is no "
                                     "temperature row" % (where, k))
                qs.append((k, S + n, _number(measured[k], "%s: '%s'" % (where, k)), sig[k]))
        zs = [None]*len(qs)
        k = PROFILES[0]
        if measured.get(k) is not None:
            if iso:
                raise ValueError("solver-config 'fit': %s measures '%s' in an iso-thermal run: there is no "
                                 "temperature row" % (where, k))
            for z, v in zip(*_profile(measured[k], "%s: '%s'" % (where, k))):
                qs.append(("%s:%g" % (k, z), S + 2, v, sig[k]))
                zs.append(z)
        k = PROFILES[1]
        ports = measured.get(k) or {}
        if not isinstance(ports, dict):
            raise ValueError("solver-config 'fit': %s: '%s' must be a dict {component: {'position', 'value'}}" % (where, k))
        for comp, d in ports.items():
            if comp not in comps:
                raise ValueError("solver-config 'fit': %s: '%s': %r is not a shell component (%s)"
                                 % (where, k, comp, ", ".join(comps)))
            for z, v in zip(*_profile(d, "%s: '%s' of %r" % (where, k, comp))):
                qs.append(("%s:%s:%g" % (k, comp, z), S + 3 + comps.index(comp), v, sig[k]))
                zs.append(z)
        seen = set()
        for lb, _, _, _ in qs:                  # (a label shows six digits of a position: two entries must not share one)
            if lb in seen:
                raise ValueError("solver-config 'fit': %s measures %r twice (positions are told apart to six digits)"
                                 % (where, lb))
            seen.add(lb)
        if not qs:
            raise ValueError("solver-config 'fit': %s has no measured value at all" % where)
        if len(qs) > MAX_QUANTITIES:
            raise ValueError("solver-config 'fit': %s holds %d measured values, at most %d are supported"
                             % (where, len(qs), MAX_QUANTITIES))
        experiments.append(qs)
        positions.append(zs)
        conditions.append(cond)
    its = spec.get('max-iterations', DEFAULTS['max-iterations'])
    batch = spec.get('batch', DEFAULTS['batch'])
    for v, k in ((its, 'max-iterations'), (batch, 'batch')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("solver-config 'fit': '%s' must be an integer >= 1 (got %r)" % (k, v))
    tol = _number(spec.get('tolerance', DEFAULTS['tolerance']), "'tolerance'", positive=True)
    damping = _number(spec.get('damping', DEFAULTS['damping']), "'damping'", positive=True)
    return Fit(names, experiments, conditions, S, int(its), tol, damping, int(batch), scales, bounds, positions)


# ----------------------------------------------------------------------------- the kernels in numpy
def _seq(values):
    """the sum in index order (np.sum adds pairwise)"""
    acc = np.float64(0.0)
    for v in values:
        acc = acc + np.float64(v)
    return acc


def emulate_residuals(y, sens, stats, rows, meas, S):
    """rmt_n2_fit_residuals_f64 in numpy: y [E][V][N], sens [E][P][V+1][N], stats [E][4], rows [E][width],
    meas [E][MQ][3] -> (pred [E][MQ], contrib [E][46]).  Every product and sum in the kernel's order."""
    y, sens, meas = (np.asarray(a, dtype=np.float64) for a in (y, sens, meas))
    E, V, N = y.shape
    P, MQ = sens.shape[1], meas.shape[1]
    pred, contrib = np.zeros((E, MQ)), np.zeros((E, CONTRIB))
    with np.errstate(all="ignore"):
        for e in range(E):
            cmax, tf = np.float64(rows[e][0]), np.float64(rows[e][1])
            peak = 0
            if V > S:
                T = y[e, S]
                peak = int(np.argmax(np.where(np.isnan(T), -np.inf, T)))
            r, J = np.zeros(MQ), np.zeros((MQ, MAX_PARAMETERS))
            bad = False
            for q in range(MQ):
                code, value, w = int(meas[e, q, 0]), meas[e, q, 1], meas[e, q, 2]
                if w == 0.0:
                    continue
                if 0 <= code < S:
                    yo = y[e, :S, N - 1]
                    c = np.where(yo > EPS, yo, EPS)*cmax
                    ctot, cs = _seq(c), c[code]
                    pv = cs/ctot
                    for p in range(P):
                        d = np.where(yo > EPS, sens[e, p, :S, N - 1]*cmax, 0.0)
                        dsum = _seq(d)
                        J[q, p] = (d[code]/ctot - (cs*dsum)/(ctot*ctot))*w
                elif V > S and code in (S, S + 1):
                    n = N - 1 if code == S else peak
                    pv = y[e, S, n]*tf + tf
                    for p in range(P):
                        J[q, p] = (sens[e, p, S, n]*tf)*w
                else:
                    pv = np.nan
                r[q] = (pv - value)*w
                pred[e, q] = pv
                bad = bad or not (np.isfinite(pv) and np.isfinite(r[q]) and np.all(np.isfinite(J[q])))
            contrib[e, 0] = 0.5*_seq(r*r)
            for a in range(MAX_PARAMETERS):
                contrib[e, 1 + a] = _seq(J[:, a]*r)
                for b in range(a, MAX_PARAMETERS):
                    contrib[e, 1 + MAX_PARAMETERS + tri(a, b)] = _seq(J[:, a]*J[:, b])
            bad = bad or not np.all(np.isfinite(contrib[e, :CONTRIB - 1]))
            contrib[e, CONTRIB - 1] = 1.0 if (bad or stats[e][1] >= 0.0) else 0.0
    return pred, contrib


def column_sums(contrib):
    """the 46 column sums over the experiments in index order, as rmt_n2_fit_update_f64 takes them"""
    contrib = np.asarray(contrib, dtype=np.float64)
    acc = np.zeros(contrib.shape[1])
    with np.errstate(all="ignore"):
        for row in contrib:
            acc = acc + row
    return acc


def _cholesky(a, P):
    for j in range(P):
        d = a[j, j]
        for k in range(j):
            d = d - a[j, k]*a[j, k]
        if not d > 0.0:
            return False
        l = np.sqrt(d)
        a[j, j] = l
        for i in range(j + 1, P):
            s = a[i, j]
            for k in range(j):
                s = s - a[i, k]*a[j, k]
            a[i, j] = s/l
    return True


def emulate_update(sums, state, P, p0, tolerance, damping):
    """The LM law of rmt_n2_fit_update_f64 in numpy: ``sums`` [46] (column_sums), ``state`` [80] (changed in place, zero
    before the first pass), ``p0`` [P] the fitted columns of member 0's row (read by the first pass only).  Returns the log
    slice [68]; its p_trial is what the kernel writes into the rows."""
    sums = np.asarray(sums, dtype=np.float64)
    M8 = MAX_PARAMETERS
    Ct, nfail = sums[0], sums[CONTRIB - 1]
    started = state[0] != 0.0
    Ccur, lam, nu, conv, status, red = state[1], state[2], state[3], state[4], int(state[6]), state[7]
    pc, pt = np.zeros(M8), np.zeros(M8)
    if started:
        pc[:] = state[ST_PCUR:ST_PCUR + M8]
        pt[:] = state[ST_PTRIAL:ST_PTRIAL + M8]
    else:
        pc[:P] = np.asarray(p0, dtype=np.float64)[:P]
        pt[:] = pc
    accepted = 0.0
    with np.errstate(all="ignore"):
        if conv == 0.0 and status == 0:
            ok = bool(np.isfinite(Ct)) and nfail == 0.0
            if not started:
                take = True
                if not ok:
                    status |= FIRST_FAILED
                lam, nu = np.float64(damping), np.float64(2.0)
            else:
                take = ok and Ct < Ccur
                if take:
                    rho = (Ccur - Ct)/red
                    t = 2.0*rho - 1.0
                    f = 1.0 - t*t*t
                    if not f > 1.0/3.0:
                        f = 1.0/3.0
                    lam, nu = lam*f, np.float64(2.0)
                else:
                    lam, nu = lam*nu, 2.0*nu
            if take:
                accepted = 1.0
                Ccur = Ct
                pc[:] = pt
                state[ST_G:ST_G + M8] = sums[1:1 + M8]
                state[ST_H:ST_H + TRI] = sums[1 + M8:1 + M8 + TRI]
            g, h = state[ST_G:ST_G + M8].copy(), state[ST_H:ST_H + TRI].copy()
            if Ccur == 0.0:
                conv = 1.0
            if conv == 0.0 and not status & FIRST_FAILED:
                d = np.array([h[tri(j, j)] if h[tri(j, j)] > FLOOR else FLOOR for j in range(P)])
                solved = False
                for tries in range(9):
                    if tries:
                        lam = 10.0*lam
                    a = np.zeros((M8, M8))
                    for i in range(P):
                        for j in range(i + 1):
                            a[i, j] = h[tri(j, i)] + lam*d[i] if i == j else h[tri(j, i)]
                    solved = _cholesky(a, P)
                    if solved:
                        break
                if not solved:
                    status |= NOT_POSITIVE
                else:
                    x = np.zeros(M8)
                    for i in range(P):
                        s = -g[i]
                        for k in range(i):
                            s = s - a[i, k]*x[k]
                        x[i] = s/a[i, i]
                    for i in range(P - 1, -1, -1):
                        s = x[i]
                        for k in range(i + 1, P):
                            s = s - a[k, i]*x[k]
                        x[i] = s/a[i, i]
                    q, step = np.float64(0.0), np.float64(0.0)
                    for j in range(P):
                        q = q + x[j]*((lam*d[j])*x[j] - g[j])
                        m = abs(pc[j])
                        rel = abs(x[j])/(m if m > FLOOR else FLOOR)
                        if not rel <= step:
                            step = rel
                    red = 0.5*q
                    if step <= tolerance:
                        conv = 1.0
                    pt[:P] = pc[:P] + x[:P]
                    state[ST_DELTA:ST_DELTA + P] = x[:P]
            if conv != 0.0 or status != 0:
                pt[:] = pc
            state[0], state[1], state[2], state[3], state[4] = 1.0, Ccur, lam, nu, conv
            state[5] += 1.0
            state[6], state[7] = float(status), red
            state[ST_PCUR:ST_PCUR + M8] = pc
            state[ST_PTRIAL:ST_PTRIAL + M8] = pt
    log = np.zeros(LOG)
    log[:8] = Ct, Ccur, lam, nu, accepted, conv, nfail, float(status)
    log[LOG_PTRIAL:LOG_PTRIAL + M8] = pt
    log[LOG_PCUR:LOG_PCUR + M8] = pc
    log[LOG_G:LOG_G + M8] = sums[1:1 + M8]
    log[LOG_H:LOG_H + TRI] = sums[1 + M8:1 + M8 + TRI]
    return log


# ----------------------------------------------------------------------------- the extended kernels in numpy
def _node_fraction(ye, se, S, n, code, cmax, P):
    """mole fraction of species ``code`` of the clamped state of node n and its derivatives [8], in the kernel's order"""
    yo = ye[:S, n]
    c = np.where(yo > EPS, yo, EPS)*cmax
    ctot, cs = _seq(c), c[code]
    dx = np.zeros(MAX_PARAMETERS)
    for p in range(P):
        d = np.where(yo > EPS, se[p, :S, n]*cmax, 0.0)
        dx[p] = d[code]/ctot - (cs*_seq(d))/(ctot*ctot)
    return cs/ctot, dx


def emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, columns, flags):
    """rmt_n2_fit_residuals_ex_f64 in numpy: ``emulate_residuals`` with the two codes measured along the bed - S+2 the
    temperature, S+3+i the mole fraction of species i, at pos [E][MQ][2] = {n0, f}: (1-f) q(n0) + f q(n0+1), the Jacobian
    row likewise - and column j of J multiplied by the member's own value of a log-scaled constant (``flags`` [P],
    ``columns`` [P] its user columns)."""
    y, sens, meas, pos = (np.asarray(a, dtype=np.float64) for a in (y, sens, meas, pos))
    E, V, N = y.shape
    P, MQ = sens.shape[1], meas.shape[1]
    pred, contrib = np.zeros((E, MQ)), np.zeros((E, CONTRIB))
    with np.errstate(all="ignore"):
        for e in range(E):
            cmax, tf = np.float64(rows[e][0]), np.float64(rows[e][1])
            peak = 0
            if V > S:
                T = y[e, S]
                peak = int(np.argmax(np.where(np.isnan(T), -np.inf, T)))
            r, J = np.zeros(MQ), np.zeros((MQ, MAX_PARAMETERS))
            bad = False
            for q in range(MQ):
                code, value, w = int(meas[e, q, 0]), meas[e, q, 1], meas[e, q, 2]
                if w == 0.0:
                    continue
                n0, f = int(pos[e, q, 0]), pos[e, q, 1]
                inside = 0 <= n0 <= N - 2
                if 0 <= code < S:
                    pv, dx = _node_fraction(y[e], sens[e], S, N - 1, code, cmax, P)
                    J[q] = dx*w
                elif V > S and code in (S, S + 1):
                    n = N - 1 if code == S else peak
                    pv = y[e, S, n]*tf + tf
                    for p in range(P):
                        J[q, p] = (sens[e, p, S, n]*tf)*w
                elif V > S and code == S + 2 and inside:
                    pv = (1.0 - f)*(y[e, S, n0]*tf + tf) + f*(y[e, S, n0 + 1]*tf + tf)
                    for p in range(P):
                        J[q, p] = ((1.0 - f)*(sens[e, p, S, n0]*tf) + f*(sens[e, p, S, n0 + 1]*tf))*w
                elif S + 3 <= code < 2*S + 3 and inside:
                    x0, d0 = _node_fraction(y[e], sens[e], S, n0, code - S - 3, cmax, P)
                    x1, d1 = _node_fraction(y[e], sens[e], S, n0 + 1, code - S - 3, cmax, P)
                    pv = (1.0 - f)*x0 + f*x1
                    J[q] = ((1.0 - f)*d0 + f*d1)*w
                else:
                    pv = np.nan
                for p in range(P):
                    if flags[p]:
                        J[q, p] = J[q, p]*np.float64(rows[e][MEMBER_USER + S + columns[p]])
                r[q] = (pv - value)*w
                pred[e, q] = pv
                bad = bad or not (np.isfinite(pv) and np.isfinite(r[q]) and np.all(np.isfinite(J[q])))
            contrib[e, 0] = 0.5*_seq(r*r)
            for a in range(MAX_PARAMETERS):
                contrib[e, 1 + a] = _seq(J[:, a]*r)
                for b in range(a, MAX_PARAMETERS):
                    contrib[e, 1 + MAX_PARAMETERS + tri(a, b)] = _seq(J[:, a]*J[:, b])
            bad = bad or not np.all(np.isfinite(contrib[e, :CONTRIB - 1]))
            contrib[e, CONTRIB - 1] = 1.0 if (bad or stats[e][1] >= 0.0) else 0.0
    return pred, contrib


def emulate_update_ex(sums, state, P, p0, tolerance, damping, flags, bx):
    """The law of rmt_n2_fit_update_ex_f64 in numpy: ``emulate_update`` in theta (= ln p of a log-scaled parameter,
    ``flags`` [P]) inside the box ``bx`` (``box``).  In order: the active set A = {j: on its lower bound with g_j > 0, or on
    its upper with g_j < 0} (tested on p), whose rows and columns of H + lambda D become the unit vector and whose g_j = 0;
    the step, clamped into the box; the predicted reduction - today's formula when nothing was clamped, else the model's own
    -(g^T d + 1/2 d^T H d), which must be > 0 or lambda grows like after a failed pivot; convergence on max |d_j|/s_j with
    s_j = 1 for a log parameter (all parameters in A: converged); the trial p_cur + d_j, p_cur exp(d_j) for a log
    parameter, the bound itself where the step was clamped, kept inside the box in p.  Returns the log slice [70]: the 68
    of the plain law and the parameters of the current point on their lower / upper bound, one bit each (state words 76, 77).
    Without flags and bounds: bit for bit the plain law."""
    sums = np.asarray(sums, dtype=np.float64)
    M8 = MAX_PARAMETERS
    Ct, nfail = sums[0], sums[CONTRIB - 1]
    started = state[0] != 0.0
    Ccur, lam, nu, conv, status, red = state[1], state[2], state[3], state[4], int(state[6]), state[7]
    pc, pt = np.zeros(M8), np.zeros(M8)
    if started:
        pc[:] = state[ST_PCUR:ST_PCUR + M8]
        pt[:] = state[ST_PTRIAL:ST_PTRIAL + M8]
    else:
        pc[:P] = np.asarray(p0, dtype=np.float64)[:P]
        pt[:] = pc
    accepted = 0.0
    with np.errstate(all="ignore"):
        if conv == 0.0 and status == 0:
            ok = bool(np.isfinite(Ct)) and nfail == 0.0
            if not started:
                take = True
                if not ok:
                    status |= FIRST_FAILED
                lam, nu = np.float64(damping), np.float64(2.0)
            else:
                take = ok and Ct < Ccur
                if take:
                    rho = (Ccur - Ct)/red
                    t = 2.0*rho - 1.0
                    f = 1.0 - t*t*t
                    if not f > 1.0/3.0:
                        f = 1.0/3.0
                    lam, nu = lam*f, np.float64(2.0)
                else:
                    lam, nu = lam*nu, 2.0*nu
            if take:
                accepted = 1.0
                Ccur = Ct
                pc[:] = pt
                state[ST_G:ST_G + M8] = sums[1:1 + M8]
                state[ST_H:ST_H + TRI] = sums[1 + M8:1 + M8 + TRI]
            g, h = state[ST_G:ST_G + M8].copy(), state[ST_H:ST_H + TRI].copy()
            lower = upper = 0
            for j in range(P):
                if pc[j] <= bx[0, j] and g[j] > 0.0:
                    lower |= 1 << j
                if pc[j] >= bx[1, j] and g[j] < 0.0:
                    upper |= 1 << j
            act = lower | upper
            for j in range(P):
                if act >> j & 1:
                    g[j] = 0.0
            state[ST_LOWER], state[ST_UPPER] = float(lower), float(upper)
            if Ccur == 0.0 or act == (1 << P) - 1:
                conv = 1.0
            if conv == 0.0 and not status & FIRST_FAILED:
                d = np.array([h[tri(j, j)] if h[tri(j, j)] > FLOOR else FLOOR for j in range(P)])
                th = np.array([np.log(pc[j]) if flags[j] else pc[j] for j in range(P)])
                solved = False
                for tries in range(9):
                    if tries:
                        lam = 10.0*lam
                    a = np.zeros((M8, M8))
                    for i in range(P):
                        for j in range(i + 1):
                            if act >> i & 1 or act >> j & 1:
                                a[i, j] = 1.0 if i == j else 0.0
                            else:
                                a[i, j] = h[tri(j, i)] + lam*d[i] if i == j else h[tri(j, i)]
                    if not _cholesky(a, P):
                        continue
                    x = np.zeros(M8)
                    for i in range(P):
                        s = -g[i]
                        for k in range(i):
                            s = s - a[i, k]*x[k]
                        x[i] = s/a[i, i]
                    for i in range(P - 1, -1, -1):
                        s = x[i]
                        for k in range(i + 1, P):
                            s = s - a[k, i]*x[k]
                        x[i] = s/a[i, i]
                    side = np.zeros(P, dtype=int)
                    for j in range(P):
                        t = th[j] + x[j]
                        if t < bx[2, j]:                    # (already on the bound: no step, whatever ln rounds to)
                            side[j], x[j] = -1, 0.0 if pc[j] <= bx[0, j] else bx[2, j] - th[j]
                        elif t > bx[3, j]:
                            side[j], x[j] = 1, 0.0 if pc[j] >= bx[1, j] else bx[3, j] - th[j]
                    if not np.any(side):
                        q = np.float64(0.0)
                        for j in range(P):
                            q = q + x[j]*((lam*d[j])*x[j] - g[j])
                        red = 0.5*q
                    else:
                        gd, hd = np.float64(0.0), np.float64(0.0)
                        for i in range(P):
                            gd = gd + g[i]*x[i]
                            row = np.float64(0.0)
                            for j in range(P):
                                row = row + h[tri(min(i, j), max(i, j))]*x[j]
                            hd = hd + x[i]*row
                        red = -(gd + 0.5*hd)
                        if not red > 0.0:
                            continue
                    solved = True
                    break
                if not solved:
                    status |= NOT_POSITIVE
                else:
                    step = np.float64(0.0)
                    for j in range(P):
                        m = abs(pc[j])
                        rel = abs(x[j]) if flags[j] else abs(x[j])/(m if m > FLOOR else FLOOR)
                        if not rel <= step:
                            step = rel
                    if step <= tolerance:
                        conv = 1.0
                    for j in range(P):
                        if side[j]:
                            v = bx[0, j] if side[j] < 0 else bx[1, j]
                        else:
                            v = pc[j]*np.exp(x[j]) if flags[j] else pc[j] + x[j]
                        v = bx[0, j] if v < bx[0, j] else v
                        pt[j] = bx[1, j] if v > bx[1, j] else v
                    state[ST_DELTA:ST_DELTA + P] = x[:P]
            if conv != 0.0 or status != 0:
                pt[:] = pc
            state[0], state[1], state[2], state[3], state[4] = 1.0, Ccur, lam, nu, conv
            state[5] += 1.0
            state[6], state[7] = float(status), red
            state[ST_PCUR:ST_PCUR + M8] = pc
            state[ST_PTRIAL:ST_PTRIAL + M8] = pt
    log = np.zeros(LOG_EX)
    log[:8] = Ct, Ccur, lam, nu, accepted, conv, nfail, float(status)
    log[LOG_PTRIAL:LOG_PTRIAL + M8] = pt
    log[LOG_PCUR:LOG_PCUR + M8] = pc
    log[LOG_G:LOG_G + M8] = sums[1:1 + M8]
    log[LOG_H:LOG_H + TRI] = sums[1 + M8:1 + M8 + TRI]
    log[LOG_LOWER], log[LOG_UPPER] = state[ST_LOWER], state[ST_UPPER]
    return log
