"""Time-on-stream runs of model N2 (solver-config "deactivation"): catalyst deactivation of a quasi-steady bed.

    "deactivation": {
        "time-on-stream": [5e5, 1e6, 1.5e6, 2e6],    # s, strictly increasing, first >= 0: the output times
        "steps": 4,                                   # equal activity steps per output interval, integer >= 1 (default 1)
        "rate-constant": 2e-6,                        # k_ref, 1/s, > 0
        "activation-energy": 8.0e4,                   # Ed, J/mol, >= 0 (default 0)
        "reference-temperature": 623.0,               # K, > 0:  k_d(T) = k_ref exp(-(Ed/R)(1/T - 1/Tref)); needed when Ed > 0
        "order": 1.0,                                 # m >= 1 (default 1)
        "residual-activity": 0.0,                     # a_inf in [0, 1) (default 0):  da/dt = -k_d(T) (a - a_inf)^m
        "tolerance": 1e-10, "max-iterations": 400}    # the march's own (defaults of initial.DEFAULTS)

* Deactivation runs over hours to months, the bed's transient over seconds: the bed is quasi-steady.  A campaign is a
  sequence of steady states f(y; a(t)) = 0 with the law between them; T is the node's temperature Tf (1 + theta_n) in
  kelvin, in an iso-thermal run the member's inlet temperature.  a <= a_inf does not move.
* With the key rmtExe integrates nothing in time: 'period', 'tNo' and 'ivp' are not used and no stepper is compiled.
  "schedule", "control", "monitor" and "initial" raise together with it (a quasi-steady bed has no transient);
  "axial-profile" combines: it is the fresh bed a(z, 0) and the coolant zones (without it a = 1, delta = 0).
* One step t_k -> t_k + dt is ONE launch of rmt_n2_campaign_step (csrc/kernels/72_campaign.inc): the march of
  "initial": "steady" with a^k, every node started from its converged upstream state, and behind every node's solve the
  exact solution of the law at that node's frozen temperature (`emulate` below restates it).  The update is positive,
  monotone, exact for an iso-thermal bed, first order in dt through the coupling with T, and the identity for dt = 0: the
  state at the last time is one more launch with dt = 0, a run of K steps K + 1 launches.
* Ensembles: the dict form shares one law; a member of the list form may carry its own five law constants under its own
  solver-config["deactivation"] (everything else there must be the base input's).  The law goes to the device as [E][5].
* Result: one dataPack entry per output time (its dataTime is the time on stream), and resModel["deactivation"] (every
  resModel["ensemble"][e] its own): "time-on-stream" [K+1] (all step times, 0 included), "output-steps", "position" [N],
  "catalyst-activity" [n_out+1][N] (t = 0, then every output time - a row can be fed back verbatim as the
  'catalyst-activity' of an "axial-profile" at 'position'), per step "mean-activity", "min-activity", "outlet" (as
  monitor.result_entry: mole fractions and T in K, with "labelList"), "peak-temperature", "peak-position", "iterations"
  (the largest per-node count of that march), "residual" (its worst scaled node residual), and "law".
* Constant-yield operation - the optional key "policy" inside "deactivation":
      "policy": {"hold": "outlet-mole-fraction", "component": "DME", "target": 0.0150,      # target in (0, 1)
                 "manipulated": "medium-temperature", "limits": [503.0, 543.0],             # K, 0 < lo <= hi
                 "tolerance": 1e-10, "max-evaluations": 40}                                 # absolute, on x_c; marches per step >= 4
  moves the common coolant level T (the member's MeTe; the zones of an "axial-profile" keep their offsets) in every step
  so that r(T) = x_c,outlet(T) - target = 0, inside ONE launch of rmt_n2_campaign_policy_step (the policy unit,
  codeplan.campaign_policy_plan; a run without the key loads the unit it always did and returns the same bits).  Every value of
  r is a whole march.  The scheme, which `policy_emulate` below restates: march at lo and at hi; without a sign change
  the limit with the smaller |r| is accepted (a tie: lo) and the step is "saturated"; else one march at the carried level
  (step 0: MeTe clipped to the limits, then the previous step's accepted level) shrinks the bracket and Illinois regula
  falsi runs until |r| <= "tolerance".  A bracket below 1e-9 K with |r| above the tolerance (the outlet jumps there: a node
  changed its branch of steady states) and "max-evaluations" marches without convergence raise, naming the member, the
  step and its time on stream.  The sign of dr/dT is taken from the bracket: the outlet of the DME bed is not monotone in
  the coolant level over its life.  Where the bracket holds several roots the policy takes the one Illinois reaches from
  the limits.  The accepted level is always the last one marched, so the state, the dataPack entries and the per-step
  entries above are those of the accepted march; the activities move after it, at its temperatures.  It raises for an
  iso-thermal run and for MeTe = 0 (the adiabatic switch).  A member of the list form may carry its own 'target' and
  'limits'.  Result: resModel["deactivation"]["policy"] with, per step, "medium-temperature" [K], "held", "evaluations",
  "saturated" (-1 at lo, 0 inside, +1 at hi), and "end-of-run": the time on stream of the first saturated step, or None.
* Not built: other laws (concentration-dependent poisoning, coking), other held quantities (conversion, peak
  temperature) and other manipulated ones (inlet temperature, pressure), tracking the previous root with a narrow
  bracket, adaptive activity steps, a warm start from the previous step's state, models other than N2, fp32, multi-rank
  runs.

Host side only (numpy): parsing and validation, the step times, the law in numpy and the result entry.
"""
import numpy as np

from . import initial

KEY = "deactivation"
LAW_KEYS = ("rate-constant", "activation-energy", "reference-temperature", "order", "residual-activity")
KEYS = ("time-on-stream", "steps") + LAW_KEYS + ("tolerance", "max-iterations", "policy")
POLICY = "policy"
POLICY_KEYS = ("hold", "component", "target", "manipulated", "limits", "tolerance", "max-evaluations")
POLICY_MEMBER_KEYS = ("target", "limits")            # what a member of the list form may carry of its own
POLICY_DEFAULTS = {"tolerance": 1e-10, "max-evaluations": 40}
POLICY_HOLD, POLICY_MANIPULATED = "outlet-mole-fraction", "medium-temperature"
POLICY_DEFINE = "RMT_CAMPAIGN_POLICY"
POLICY_ROW = 4           # csrc/kernels/72_campaign.inc RMT_POLICY_ROW: {target, lo, hi, tolerance}
POLICY_LOG = 4           # ... RMT_POLICY_LOG: {level, held, marches, saturated}
LEVEL, HELD, EVALUATIONS, SATURATED = range(POLICY_LOG)
MIN_BRACKET = 1e-9       # ... RMT_POLICY_MIN_BRACKET, K
FLAG_POLICY_BRACKET, FLAG_POLICY_EVALS = 64, 128     # include/rmt_n2.h RMT_N2_FLAG_POLICY_*
BRACKET_COLLAPSED, EVALUATION_LIMIT = 2, 3           # `saturated` of a step that failed (device log and policy_emulate)
EXCLUDES = ("schedule", "control", "monitor", "initial")
MODELS = ("N2",)
DEFINE = "RMT_CAMPAIGN"
LAW_DEFAULTS = {"activation-energy": 0.0, "order": 1.0, "residual-activity": 0.0}
R_CONST = 8.314472       # plan.R_CONST, the constant of the device template
LOG_EXTRA = 6            # csrc/kernels/72_campaign.inc RMT_CAMPAIGN_LOG = V + 6
PEAK, PEAK_NODE, MEAN, MIN, RESIDUAL, ITERATIONS = range(LOG_EXTRA)


def check_model(modelInput):
    """ValueError when the input asks for a campaign on a model that has none (rmtExe, before any device work)."""
    if (modelInput.get('solver-config') or {}).get(KEY) is not None and modelInput.get('model') not in MODELS:
        raise ValueError("solver-config 'deactivation' (time-on-stream runs of a quasi-steady bed) is only available for "
                         "model 'N2' (got model %r)" % (modelInput.get('model'),))


def _number(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)


def _law(spec, who=""):
    """the five law constants of a (complete) spec, checked"""
    def bad(key, what, v):
        raise ValueError("solver-config 'deactivation'%s: %r must be %s (got %r)" % (who, key, what, v))
    if 'rate-constant' not in spec:
        raise ValueError("solver-config 'deactivation'%s needs 'rate-constant' (k_ref, 1/s)" % who)
    k = spec['rate-constant']
    if not _number(k) or not k > 0:
        bad('rate-constant', "a positive number", k)
    ed = spec.get('activation-energy', LAW_DEFAULTS['activation-energy'])
    if not _number(ed) or ed < 0:
        bad('activation-energy', "a number >= 0", ed)
    if 'reference-temperature' not in spec and ed > 0:
        raise ValueError("solver-config 'deactivation'%s: 'activation-energy' > 0 needs 'reference-temperature' (K)" % who)
    tref = spec.get('reference-temperature', 298.15)
    if not _number(tref) or not tref > 0:
        bad('reference-temperature', "a positive number (K)", tref)
    m = spec.get('order', LAW_DEFAULTS['order'])
    if not _number(m) or m < 1:
        bad('order', "a number >= 1", m)
    ainf = spec.get('residual-activity', LAW_DEFAULTS['residual-activity'])
    if not _number(ainf) or not 0 <= ainf < 1:
        bad('residual-activity', "a number in [0, 1)", ainf)
    return [float(k), float(ed), float(tref), float(m), float(ainf)]


class Campaign:
    """A parsed "deactivation" spec of E members: ``outputs`` [n_out] (the output times), ``steps`` (per interval),
    ``times`` [K+1] (every step time, 0 first), ``output_steps`` [n_out] (indices into times), ``law`` [E][5] =
    {k_ref, Ed, Tref, m, a_inf}, ``tolerance``, ``max_iterations``."""

    def __init__(self, outputs, steps, law, tolerance, max_iterations, policy=None):
        self.policy = policy             # a Policy, or None: the coolant stays where the member rows have it
        self.outputs = np.asarray(outputs, dtype=np.float64)
        self.steps = int(steps)
        self.law = np.ascontiguousarray(law, dtype=np.float64).reshape(-1, len(LAW_KEYS))
        self.E = self.law.shape[0]
        self.tolerance, self.max_iterations = float(tolerance), int(max_iterations)
        times, marks, t = [0.0], [], 0.0
        for out in self.outputs:
            if out > t:
                # (equal steps; the interval's last time is the output time itself, not a sum of roundings)
                times += [t + (out - t)*j/self.steps for j in range(1, self.steps)] + [float(out)]
                t = float(out)
            marks.append(len(times) - 1)
        self.times = np.array(times, dtype=np.float64)
        self.output_steps = np.array(marks, dtype=np.int64)
        self.K = len(self.times) - 1

    def dts(self):
        """dt of launch k = 0..K: the step that follows the march at times[k]; 0 behind the last one"""
        return np.append(np.diff(self.times), 0.0)

    def check_budget(self, V, cap):
        """The device log [K+1][E][V+6] doubles (with a policy: and its [K+1][E][4]) must not exceed ``cap`` bytes
        (n2.PIPELINE_BYTES)."""
        need = (self.K + 1)*self.E*(int(V) + LOG_EXTRA + (POLICY_LOG if self.policy is not None else 0))*8
        if need > cap:
            raise ValueError("solver-config 'deactivation': %d output times x 'steps' = %d make %d launches of %d members "
                             "= %d bytes of log, more than the %d allowed - lower 'steps'"
                             % (len(self.outputs), self.steps, self.K + 1, self.E, need, cap))


def parse(modelInput, members_inputs=None, multi_rank=False):
    """The Campaign of a run (None when the base input has no "deactivation"), or ValueError / NotImplementedError naming
    'deactivation' and the offending key.  ``members_inputs``: the ensemble members (default: the base input alone)."""
    cfg = modelInput['solver-config']
    spec = cfg.get(KEY)
    if spec is None:
        return None
    check_model(modelInput)
    for other in EXCLUDES:
        if cfg.get(other) is not None:
            raise ValueError("solver-config 'deactivation' cannot be combined with %r: the bed of a time-on-stream run is "
                             "quasi-steady, it has no transient" % (other,))
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'deactivation' must be a dict with the keys %s" % (KEYS,))
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'deactivation': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    if 'time-on-stream' not in spec:
        raise ValueError("solver-config 'deactivation' needs 'time-on-stream': the output times in s")
    try:
        out = np.array(spec['time-on-stream'], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("solver-config 'deactivation': 'time-on-stream' must be a list of numbers")
    if out.ndim != 1 or len(out) < 1 or not np.all(np.isfinite(out)):
        raise ValueError("solver-config 'deactivation': 'time-on-stream' must be a non-empty list of finite numbers")
    if out[0] < 0 or np.any(np.diff(out) <= 0):
        raise ValueError("solver-config 'deactivation': 'time-on-stream' must be strictly increasing and start at or after "
                         "0 (got %r)" % (out.tolist(),))
    steps = spec.get('steps', 1)
    if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError("solver-config 'deactivation': 'steps' must be an integer >= 1 (got %r)" % (steps,))
    tol = spec.get('tolerance', initial.DEFAULTS['tolerance'])
    if not _number(tol) or not tol > 0:
        raise ValueError("solver-config 'deactivation': 'tolerance' must be a positive number (got %r)" % (tol,))
    it = spec.get('max-iterations', initial.DEFAULTS['max-iterations'])
    if isinstance(it, (bool, np.bool_)) or not isinstance(it, (int, np.integer)) or it < 1:
        raise ValueError("solver-config 'deactivation': 'max-iterations' must be an integer >= 1 (got %r)" % (it,))
    base = _law(spec)
    inputs = list(members_inputs) if members_inputs else [modelInput]
    law = []
    for e, mi in enumerate(inputs):
        own = (mi.get('solver-config') or {}).get(KEY) if mi is not modelInput else None
        if own is None or own is spec:
            law.append(base)
            continue
        who = " of member %d" % e
        if not isinstance(own, dict):
            raise ValueError("solver-config 'deactivation'%s must be a dict" % who)
        for k in own:
            if k not in KEYS:
                raise ValueError("solver-config 'deactivation'%s: unknown key %r" % (who, k))
            if k not in LAW_KEYS and k != POLICY:           # (a member's "policy": _policy below)
                same =np.array_equal(np.asarray(own[k], dtype=object), np.asarray(spec[k], dtype=object)) \
                    if k in spec else False
                if not same:
                    raise ValueError("solver-config 'deactivation'%s: %r differs from the base input's - a member may "
                                     "carry its own law constants only (%s)" % (who, k, ", ".join(LAW_KEYS)))
        law.append(_law({**{k: spec[k] for k in LAW_KEYS if k in spec}, **{k: own[k] for k in LAW_KEYS if k in own}}, who))
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise NotImplementedError("solver-config 'deactivation' is not available with 'dtype': 'fp32': the campaign step "
                                  "is an fp64 kernel")
    if multi_rank:
        raise NotImplementedError("solver-config 'deactivation' is not available in a multi-rank run")
    return Campaign(out, steps, law, tol, it, _policy(modelInput, spec, inputs))


class Policy:
    """A parsed "policy" of E members: ``component`` (name) and ``index`` (into the feed's component list), ``rows`` [E][4] =
    {target, lo, hi, tolerance} as the device takes them, ``levels`` [E] (the level step 0 carries in: the member's MeTe
    clipped to its limits), ``tolerance``, ``max_evaluations``."""

    def __init__(self, component, index, rows, levels, max_evaluations):
        self.component, self.index = component, int(index)
        self.rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, POLICY_ROW)
        self.levels = np.ascontiguousarray(levels, dtype=np.float64)
        self.tolerance = float(self.rows[0, 3])
        self.max_evaluations = int(max_evaluations)


def _policy_target_limits(pol, who):
    def bad(key, what, v):
        raise ValueError("solver-config 'deactivation' 'policy'%s: %r must be %s (got %r)" % (who, key, what, v))
    for key in POLICY_MEMBER_KEYS:
        if key not in pol:
            raise ValueError("solver-config 'deactivation' 'policy'%s needs %r" % (who, key))
    target = pol['target']
    if not _number(target) or not 0 < target < 1:
        bad('target', "a mole fraction in (0, 1)", target)
    lim = pol['limits']
    if not isinstance(lim, (list, tuple, np.ndarray)) or len(lim) != 2 or not all(_number(v) for v in lim) \
            or not 0 < lim[0] <= lim[1]:
        bad('limits', "[lo, hi] in kelvin with 0 < lo <= hi", lim)
    return float(target), float(lim[0]), float(lim[1])


def _policy(modelInput, spec, inputs):
    """The Policy of a run (None without the key), or ValueError naming 'deactivation' 'policy' and the offending entry."""
    pol = spec.get(POLICY)
    for e, mi in enumerate(inputs):                  # (a member cannot bring a policy the base input has not)
        own = (mi.get('solver-config') or {}).get(KEY) if mi is not modelInput else None
        if pol is None and isinstance(own, dict) and own is not spec and own.get(POLICY) is not None:
            raise ValueError("solver-config 'deactivation' of member %d: 'policy' differs from the base input's, which has "
                             "none - a member may carry its own %s of the base input's policy" % (e, POLICY_MEMBER_KEYS))
    if pol is None:
        return None
    if not isinstance(pol, dict):
        raise ValueError("solver-config 'deactivation' 'policy' must be a dict with the keys %s" % (POLICY_KEYS,))
    for k in pol:
        if k not in POLICY_KEYS:
            raise ValueError("solver-config 'deactivation' 'policy': unknown key %r (known: %s)" % (k, ", ".join(POLICY_KEYS)))
    for key, only in (("hold", POLICY_HOLD), ("manipulated", POLICY_MANIPULATED)):
        if pol.get(key) != only:
            raise ValueError("solver-config 'deactivation' 'policy': %r must be %r (got %r) - other %s quantities are not "
                             "built" % (key, only, pol.get(key), "held" if key == "hold" else "manipulated"))
    comps = list(modelInput['feed']['components']['shell'])
    comp = pol.get('component')
    if comp not in comps:
        raise ValueError("solver-config 'deactivation' 'policy': unknown 'component' %r (the feed has %s)"
                         % (comp, ", ".join(comps)))
    ptol = pol.get('tolerance', POLICY_DEFAULTS['tolerance'])
    if not _number(ptol) or not ptol > 0:
        raise ValueError("solver-config 'deactivation' 'policy': 'tolerance' must be a positive number (got %r)" % (ptol,))
    mev = pol.get('max-evaluations', POLICY_DEFAULTS['max-evaluations'])
    if isinstance(mev, (bool, np.bool_)) or not isinstance(mev, (int, np.integer)) or mev < 4:
        raise ValueError("solver-config 'deactivation' 'policy': 'max-evaluations' must be an integer >= 4 (got %r)" % (mev,))
    if modelInput['operating-conditions'].get('process-type') == "iso-thermal":
        raise ValueError("solver-config 'deactivation' 'policy': 'manipulated' %r needs an energy balance - process-type "
                         "'iso-thermal' has none" % (POLICY_MANIPULATED,))
    base = _policy_target_limits(pol, "")
    rows, levels = [], []
    for e, mi in enumerate(inputs):
        own = (mi.get('solver-config') or {}).get(KEY) if mi is not modelInput else None
        own = own.get(POLICY) if isinstance(own, dict) and own is not spec else None
        tl = base
        if own is not None and own is not pol:
            who = " of member %d" % e
            if not isinstance(own, dict):
                raise ValueError("solver-config 'deactivation' 'policy'%s must be a dict" % who)
            for k in own:
                if k not in POLICY_KEYS:
                    raise ValueError("solver-config 'deactivation' 'policy'%s: unknown key %r" % (who, k))
                if k not in POLICY_MEMBER_KEYS and (k not in pol or own[k] != pol[k]):
                    raise ValueError("solver-config 'deactivation' 'policy'%s: %r differs from the base input's - a member "
                                     "may carry its own %s only" % (who, k, " and ".join(POLICY_MEMBER_KEYS)))
            tl = _policy_target_limits({**{k: pol[k] for k in POLICY_MEMBER_KEYS}, **own}, who)
        mete = float(mi['external-heat']['MeTe'])
        if mete == 0:
            raise ValueError("solver-config 'deactivation' 'policy': 'manipulated' %r needs a member with external-heat MeTe "
                             "> 0 (MeTe = 0 is the adiabatic switch); member %d has MeTe = 0" % (POLICY_MANIPULATED, e))
        rows.append(tl + (float(ptol),))
        levels.append(min(max(mete, tl[1]), tl[2]))
    return Policy(comp, comps.index(comp), rows, levels, mev)


def policy_emulate(row, carried, max_evaluations, r):
    """One step of the policy's root-find in numpy, as rmt_n2_campaign_policy_step writes it.  ``row`` = (target, lo, hi,
    tolerance), ``carried`` the level the step carries in, ``r``: a callable T -> x_c,outlet(T) - target (one march per
    call), or a sequence of such values that is consumed in order.  Returns dict(levels: every level marched, in order;
    level: the last one; residual: r there; evaluations; saturated: -1 | 0 | +1, or BRACKET_COLLAPSED / EVALUATION_LIMIT
    for a step the device flags)."""
    _, lo, hi, ptol = (float(v) for v in row)
    carried = float(carried)
    if not callable(r):
        values = iter(r)
        r = lambda T: next(values)
    levels = []

    def march(T):
        levels.append(T)
        return float(r(T))

    def done(sat, res):
        return {"levels": levels, "level": levels[-1], "residual": res, "evaluations": len(levels), "saturated": sat}
    a, b = lo, hi
    ra = march(lo)
    if lo == hi:
        return done(-1, ra)
    rb = march(hi)
    if not ra*rb < 0.0:
        if abs(rb) < abs(ra):
            return done(1, rb)
        return done(-1, march(lo))                 # (the accepted level is the last one marched)
    side = 0
    if lo < carried < hi:
        T, illinois = carried, False
    else:
        T = a - ra*(b - a)/(rb - ra)
        T, illinois = (T if a < T < b else 0.5*(a + b)), True
    while True:
        res = march(T)
        if abs(res) <= ptol:
            return done(0, res)
        if res*rb > 0.0:
            b, rb = T, res
            if illinois and side == 1:
                ra *= 0.5
            side = 1
        else:
            a, ra = T, res
            if illinois and side == -1:
                rb *= 0.5
            side = -1
        if not illinois:
            side, illinois = 0, True
        if b - a < MIN_BRACKET:
            return done(BRACKET_COLLAPSED, res)
        if len(levels) >= int(max_evaluations):
            return done(EVALUATION_LIMIT, res)
        T = a - ra*(b - a)/(rb - ra)
        if not a < T < b:
            T = 0.5*(a + b)


def policy_entry(cam, e, plog):
    """resModel["deactivation"]["policy"] of member e from its policy log rows [K+1][4]."""
    plog = np.asarray(plog, dtype=np.float64).reshape(cam.K + 1, POLICY_LOG)
    sat = plog[:, SATURATED].astype(np.int64)
    hit = np.nonzero(sat != 0)[0]
    pol = cam.policy
    return {"hold": POLICY_HOLD, "component": pol.component, "manipulated": POLICY_MANIPULATED,
            "target": float(pol.rows[e, 0]), "limits": [float(pol.rows[e, 1]), float(pol.rows[e, 2])],
            "tolerance": pol.tolerance, "max-evaluations": pol.max_evaluations,
            "medium-temperature": plog[:, LEVEL].copy(), "held": plog[:, HELD].copy(),
            "evaluations": plog[:, EVALUATIONS].astype(np.int64), "saturated": sat,
            "end-of-run": float(cam.times[hit[0]]) if len(hit) else None}


def emulate(a, T, dt, law):
    """a(t + dt) at the frozen temperature T [K] - the law in numpy, as rmt_campaign_update writes it.  ``a`` and ``T``
    broadcast; ``law`` = (k_ref, Ed, Tref, m, a_inf)."""
    k, ed, tref, m, ainf = (float(v) for v in law)
    a = np.asarray(a, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    b = a - ainf
    moves = b > 0.0
    bs = np.where(moves, b, 1.0)
    x = k*np.exp(-(ed/R_CONST)*(1.0/T - 1.0/tref))*float(dt)
    q = m - 1.0
    if q == 0.0:
        new = a + bs*np.expm1(-x)
    else:
        new = a - bs*(1.0 - np.power(1.0 + q*x*np.power(bs, q), -1.0/q))
    return np.where(moves, new, a)


def result_entry(cam, e, log, activity, mech, zNo, named):
    """resModel["deactivation"] of member e from its log rows [K+1][V+6] and its activities at t = 0 and the output times
    [n_out+1][N].  Units as in the dataPack entries and in monitor.result_entry."""
    log = np.asarray(log, dtype=np.float64).reshape(cam.K + 1, mech.V + LOG_EXTRA)
    V, tf = mech.V, named["Tf"]
    last, extra = log[:, :V], log[:, V:]
    conc = (last if mech.iso else last[:, :-1])*named["Cmax"]
    T = np.zeros((cam.K + 1, 1))*tf + tf if mech.iso else last[:, -1:]*tf + tf
    xs = np.linspace(0, 1, zNo)
    return {
        "time-on-stream": cam.times.copy(), "output-steps": cam.output_steps.copy(), "position": xs,
        "catalyst-activity": np.array(activity, dtype=np.float64),
        "mean-activity": extra[:, MEAN].copy(), "min-activity": extra[:, MIN].copy(),
        "labelList": list(mech.compList) + ["Temperature"],
        "outlet": np.concatenate((conc/np.sum(conc, axis=1, keepdims=True), T), axis=1),
        "peak-temperature": extra[:, PEAK]*tf + tf, "peak-position": xs[extra[:, PEAK_NODE].astype(np.int64)],
        "iterations": extra[:, ITERATIONS].astype(np.int64), "residual": extra[:, RESIDUAL].copy(),
        "law": dict(zip(LAW_KEYS, (float(v) for v in cam.law[e]))),
    }
