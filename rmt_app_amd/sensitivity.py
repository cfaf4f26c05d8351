"""Parametric sensitivities of the steady state a dynamic N2 run starts from (solver-config "sensitivity").

    "initial": "steady",
    "sensitivity": {"parameters": ["medium-temperature", "inlet-temperature", "inlet-pressure",
                                   {"inlet-concentration": "CO"}, {"rate-constant": "<scalar reaction-rates.VARS entry>"}]}

* Absent: nothing of the run changes - no code object, no launch, no result entry.
* The derivatives are those of the discrete steady state f(y*) = 0 the march found ("initial": "steady", initial.py), with
  respect to the values the march read at t = 0.  The four boundary parameters mean exactly what "schedule" moves: the
  member-row values THETA_IN, P0, TM, CIN_i with the scaling and everything else of the member unchanged (so
  "inlet-concentration" does not move Cmax or the feed's mixture properties); "inlet-concentration" is in the unit of
  feed["concentration"].  "rate-constant" is the VARS scalar as it enters the rate lambdas; the sensitivity unit traces it
  as a per-reactor input u<k>, the way the parameter columns of an ensemble are, also when the members do not differ in it.
  (With boundary parameters only the sensitivity unit takes the place of the march unit - its march kernel is the march
  unit's text.  With a "rate-constant" that the run itself keeps a literal the march stays on the plain march unit and a
  handle of its own holds the sensitivity unit: either way the run is the run without the key, bit for bit.)
* All derivatives are analytic (csrc/kernels/73_sensitivity.inc, rmt_n2_steady_sens): the steady state is block lower-
  bidiagonal, so its tangent system is a downstream march as well - per node one inverse of a = -df/dy (the analytic node
  Jacobian) applied to every parameter's right-hand side, and the linearised Ergun recurrence for dP/dp.  No differencing.
* A feed component at the clamp (a feed concentration <= 1e-30 of the largest) has zero sensitivity: the inlet value the
  model uses there is the clamp, whatever the feed says.  A wall that is off (MeTe == 0) gives a zero "medium-temperature" row.
* resModel["sensitivity"] (every resModel["ensemble"][e] its own) = {"parameters": labels, "values": p, "labelList",
  "state": [P][V][N] d(concentration)/dp and dT/dp [K per unit of p], "pressure": [P][N] [Pa per unit of p],
  "outlet-mole-fraction": [P][S], "peak-temperature": [P] (the row of T at the node of the discrete maximum),
  "peak-position", "normalized-peak": [P] = (p / T_max) dT_max/dp - the Morbidelli-Varma normalised sensitivity}.
  An iso-thermal run has no temperature row; its three peak entries are None.
* A singular node raises FloatingPointError naming the member and the node.
* At most 8 parameters.  Not built: node-parallel assembly for one long reactor, second-order sensitivities,
  sensitivities of the dynamic trajectory, activity or zone-offset parameters, more than 8 parameters.

Host side only: parsing and validation, the conversion from the kernel's scaled rows to physical units, the result entry,
and a numpy restatement of the sweep (``emulate``) for the tests.
"""
import numpy as np

from .lowering import is_scalar_constant

KEY = "sensitivity"
DEFINE = "RMT_SENS"
DEFINE_NP = "RMT_SENS_NP"
MAX_PARAMETERS = 8
KEYS = ("parameters",)
BOUNDARY = ("medium-temperature", "inlet-temperature", "inlet-pressure")       # kinds 0, 1, 2 of the kernel
COMPOSITION, RATE_CONSTANT = "inlet-concentration", "rate-constant"             # kinds 3, 4
KIND_TM, KIND_TIN, KIND_PIN, KIND_CIN, KIND_USER = range(5)
MODELS = ("N2",)


def check_model(modelInput):
    """NotImplementedError when the input asks for sensitivities on a model that has none (rmtExe, before any device
    work)."""
    if (modelInput.get('solver-config') or {}).get(KEY) is not None and modelInput.get('model') not in MODELS:
        raise NotImplementedError("solver-config 'sensitivity' is only available for model 'N2' (got model %r)"
                                  % (modelInput.get('model'),))


class Sensitivity:
    """A parsed "sensitivity" spec: ``parameters`` = [(kind, name or None)], ``labels``."""

    def __init__(self, parameters):
        self.parameters = list(parameters)
        self.labels = [BOUNDARY[k] if k < KIND_CIN else "%s:%s" % ((COMPOSITION, RATE_CONSTANT)[k - KIND_CIN], nm)
                       for k, nm in self.parameters]
        self.NP = len(self.parameters)

    @property
    def rate_constants(self):
        return [nm for k, nm in self.parameters if k == KIND_USER]

    def unit_params(self, params):
        """The per-reactor inputs of the sensitivity unit's mechanism: the run's own (``params``) and behind them the
        rate constants asked for that are not among them."""
        params = list(params)
        return tuple(params + [nm for nm in self.rate_constants if nm not in params])

    def descriptors(self, mech):
        """(kinds, indices) as rmt_n2_steady_sens takes them, for a mechanism whose params hold the rate constants."""
        kinds, idx = [], []
        for k, nm in self.parameters:
            kinds.append(k)
            idx.append(mech.compList.index(nm) if k == KIND_CIN else mech.params.index(nm) if k == KIND_USER else 0)
        return np.array(kinds, dtype=np.int32), np.array(idx, dtype=np.int32)

    def widen(self, rows, mech, mech_s, inputs):
        """The member rows of the sensitivity unit [E][width of mech_s (+ the forced tail)]: the run's rows with the
        members' own values of the added rate constants behind their user columns."""
        extra = mech_s.params[len(mech.params):]
        if not extra:
            return rows
        rows = np.asarray(rows, dtype=np.float64)
        at = mech.row_width
        cols = np.array([[float(mi['reaction-rates']['VARS'][nm]) for nm in extra] for mi in inputs], dtype=np.float64)
        return np.ascontiguousarray(np.concatenate([rows[:, :at], cols, rows[:, at:]], axis=1))


def parse(modelInput, members_inputs=None, multi_rank=False):
    """The Sensitivity of a run (None when the input has no "sensitivity"), or ValueError / NotImplementedError naming
    the offending key."""
    cfg = modelInput['solver-config']
    spec = cfg.get(KEY)
    if spec is None:
        return None
    check_model(modelInput)
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'sensitivity' must be a dict with the key 'parameters'")
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'sensitivity': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    plist = spec.get('parameters')
    if not isinstance(plist, (list, tuple)) or len(plist) < 1:
        raise ValueError("solver-config 'sensitivity': 'parameters' must be a non-empty list")
    if len(plist) > MAX_PARAMETERS:
        raise ValueError("solver-config 'sensitivity': 'parameters' holds %d entries, at most %d are supported"
                         % (len(plist), MAX_PARAMETERS))
    comps = list(modelInput['feed']['components']['shell'])
    inputs = list(members_inputs) if members_inputs else [modelInput]
    out = []
    for p in plist:
        if isinstance(p, str):
            if p not in BOUNDARY:
                raise ValueError("solver-config 'sensitivity': unknown parameter %r in 'parameters' (known: %s, "
                                 "{'%s': component}, {'%s': VARS name})"
                                 % (p, ", ".join(BOUNDARY), COMPOSITION, RATE_CONSTANT))
            item = (BOUNDARY.index(p), None)
        elif isinstance(p, dict) and len(p) == 1:
            (k, nm), = p.items()
            if k == COMPOSITION:
                if nm not in comps:
                    raise ValueError("solver-config 'sensitivity': '%s': %r is not a shell component (%s)"
                                     % (COMPOSITION, nm, ", ".join(comps)))
                item = (KIND_CIN, nm)
            elif k == RATE_CONSTANT:
                for mi in inputs:
                    VARS = mi['reaction-rates']['VARS']
                    if not isinstance(nm, str) or nm not in VARS:
                        raise ValueError("solver-config 'sensitivity': '%s': %r is not an entry of reaction-rates.VARS"
                                         % (RATE_CONSTANT, nm))
                    if not is_scalar_constant(VARS[nm]):
                        raise NotImplementedError("solver-config 'sensitivity': '%s': VARS[%r] is not a scalar constant"
                                                  % (RATE_CONSTANT, nm))
                item = (KIND_USER, nm)
            else:
                raise ValueError("solver-config 'sensitivity': unknown parameter key %r in 'parameters' (known: '%s', '%s')"
                                 % (k, COMPOSITION, RATE_CONSTANT))
        else:
            raise ValueError("solver-config 'sensitivity': a parameter is a name (%s) or a dict with ONE key ('%s' or "
                             "'%s'), got %r" % (", ".join(BOUNDARY), COMPOSITION, RATE_CONSTANT, p))
        if item in out:
            raise ValueError("solver-config 'sensitivity': duplicate parameter %r in 'parameters'" % (p,))
        out.append(item)
    if cfg.get('deactivation') is not None:
        raise NotImplementedError("solver-config 'sensitivity' is not available with 'deactivation': a time-on-stream run "
                                  "has no single operating point")
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise NotImplementedError("solver-config 'sensitivity' is not available with 'dtype': 'fp32': the sweep is an "
                                  "fp64 kernel")
    if multi_rank:
        raise NotImplementedError("solver-config 'sensitivity' is not available in a multi-rank run")
    ini = cfg.get('initial')
    if not (ini == "steady" or (isinstance(ini, dict) and ini.get('kind') == "steady")):
        raise NotImplementedError("solver-config 'sensitivity' needs \"initial\": \"steady\": the sensitivities are those "
                                  "of the steady state the run starts from")
    return Sensitivity(out)


def parameter_values(sens, row, named, mech_s):
    """(p [NP], dp/d(row value) [NP]): the parameters' physical values at the operating point, and what one unit of
    the member-row value the kernel differentiates by is in the parameter's own unit."""
    from .plan import MEMBER_FIELDS as F
    tf, cmax = named["Tf"], named["Cmax"]
    kinds, idx = sens.descriptors(mech_s)
    p, unit = np.zeros(sens.NP), np.ones(sens.NP)
    for n, (k, i) in enumerate(zip(kinds, idx)):
        if k == KIND_TM:
            p[n] = row[F["TM"]]
        elif k == KIND_TIN:
            p[n], unit[n] = row[F["THETA_IN"]]*tf + tf, tf                 # T_in = Tf (1 + THETA_IN)
        elif k == KIND_PIN:
            p[n] = row[F["P0"]]
        elif k == KIND_CIN:
            p[n], unit[n] = row[F["CIN"] + i]*cmax, cmax                   # C_in,i = Cmax CIN_i
        else:
            p[n] = row[F["CIN"] + mech_s.S + i]
    return p, unit


def to_physical(raw, unit, named, mech):
    """The kernel's rows [NP][V+1][N] (scaled state per unit of the row value) -> (state [NP][V][N] in the units of the
    packed profiles per unit of p, pressure [NP][N])."""
    raw = np.asarray(raw, dtype=np.float64)
    S = mech.S
    state = raw[:, :mech.V, :].copy()
    state[:, :S] *= named["Cmax"]
    if not mech.iso:
        state[:, S] *= named["Tf"]
    state /= unit[:, None, None]
    return state, raw[:, mech.V, :]/unit[:, None]


def result_entry(sens, raw, y, row, named, mech_s):
    """One member's resModel["sensitivity"]: ``raw`` [NP][V+1][N] from the device, ``y`` the converged scaled state
    [V*N], ``row`` the member row of the sensitivity unit."""
    S, V = mech_s.S, mech_s.V
    N = np.asarray(raw).shape[-1]
    Y = np.reshape(np.asarray(y, dtype=np.float64), (V, N))
    p, unit = parameter_values(sens, row, named, mech_s)
    state, pressure = to_physical(raw, unit, named, mech_s)
    conc = np.maximum(Y[:S, -1], 1e-30)*named["Cmax"]              # (the model's own mole fractions: of the clamped state)
    dconc = np.where(Y[:S, -1] > 1e-30, state[:, :S, -1], 0.0)
    ctot = conc.sum()
    dx = dconc/ctot - conc[None, :]*dconc.sum(axis=1, keepdims=True)/ctot**2
    entry = {"parameters": list(sens.labels), "values": p, "labelList": list(mech_s.compList) + ([] if mech_s.iso else ["Temperature"]),
             "state": state, "pressure": pressure, "outlet-mole-fraction": dx,
             "peak-temperature": None, "peak-position": None, "normalized-peak": None}
    if not mech_s.iso:
        T = Y[S]*named["Tf"] + named["Tf"]
        n = int(np.argmax(T))
        entry["peak-temperature"] = state[:, S, n].copy()
        entry["peak-position"] = float(np.linspace(0, 1, N)[n]) if N > 1 else 1.0
        entry["normalized-peak"] = p/T[n]*state[:, S, n]
    return entry


def failed_node(raw):
    """The node at which a flagged member's sweep stopped: the first one whose rows are not finite (-1: none)."""
    bad = np.nonzero(~np.all(np.isfinite(np.asarray(raw)), axis=(0, 1)))[0]
    return int(bad[0]) if len(bad) else -1


def emulate(blocks, seeds):
    """The sweep in numpy, for the tests.  ``blocks``: per node a dict {"a": [V][V] = -df/dy, "fP": [V], "fp": [NP][V] (the
    parameter columns df/dp), "U": [V], "D": [V] (clamp derivative of THIS node's state), "daz": [V], "az", "P"};
    ``seeds``: (sd [NP][V] = D s of the inlet, pi [NP]).  Returns [NP][V+1][N] as the kernel writes it."""
    sd, pi = (np.array(v, dtype=np.float64) for v in seeds)
    NP, V = sd.shape
    out = np.zeros((NP, V + 1, len(blocks)))
    for z, b in enumerate(blocks):
        ainv = np.linalg.inv(np.asarray(b["a"], dtype=np.float64))
        for p in range(NP):
            rhs = np.asarray(b["U"])*sd[p] + np.asarray(b["fP"])*pi[p] + np.asarray(b["fp"])[p]
            s = ainv @ rhs
            out[p, :V, z], out[p, V, z] = s, pi[p]
            sd[p] = np.asarray(b["D"])*s
            pi[p] = b["az"]*pi[p] + b["P"]*float(np.dot(b["daz"], s))
    return out
