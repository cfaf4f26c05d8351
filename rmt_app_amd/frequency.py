"""Frequency response of the steady state a dynamic N2 run starts from (solver-config "frequency-response").

    "initial": "steady",
    "frequency-response": {"inputs": ["medium-temperature", "inlet-temperature", "inlet-pressure",
                                      {"inlet-concentration": "CO"}],
                           "frequencies": [1e-2, ..., 1e2],      # or {"range": [w_lo, w_hi], "points": 32}
                           "profile": False}

* Absent: nothing of the run changes - no code object, no launch, no result entry.  Present: the run itself is the run
  without the key, bit for bit (the sweep has a code object and a handle of its own).
* For a small harmonic disturbance p(t) = p0 + Re(dp e^{iwt}) of an input the linearised dynamic model - dy/dt = f with the
  pressure algebraic - settles on y* + Re(G(iw) dp e^{iwt}).  G is what this key returns: complex, in physical units per
  unit of the input, G(0) the derivative "sensitivity" gives.  The inputs are the four boundary values "schedule" moves,
  with the meaning, the units and the clamp rule of "sensitivity" (sensitivity.py); "rate-constant" is not an input.
* Frequencies are in radians per unit of model time - the unit of operating-conditions "period", which is the time unit of
  the right-hand side, so they reach the kernel as they are.  A list (0 allowed), or {"range": [lo, hi], "points": n}:
  n log-spaced values with both ends.  At most 4 inputs and 4096 frequencies.
* The steady state is block lower-bidiagonal, so the response is one more downstream march, in complex arithmetic
  (csrc/kernels/74_frequency.inc, rmt_n2_steady_freq): (a_z + i w I) s_z = U D s_(z-1) + (df/dP) pi_z + df/dp with the
  blocks of the sensitivity sweep, one (member, frequency) pair per lane.
* resModel["frequency-response"] (every resModel["ensemble"][e] its own) = {"inputs": labels, "values", "frequencies" [F],
  "labelList", "outlet-state" [P][F][V], "outlet-pressure" [P][F], "outlet-mole-fraction" [P][F][S], "outlet-temperature"
  [P][F], "peak-temperature" [P][F] (the T row at the node of the steady discrete maximum), "peak-position", and with
  "profile": True "state" [P][F][V][N] and "pressure" [P][F][N]}; complex128.  An iso-thermal run has None for the
  temperature entries.
* With "schedule" / "control" the operating point is that of their values at t = 0.
* A singular or non-finite node raises FloatingPointError naming member, frequency and node.
* Not built: inputs other than the four boundary kinds, sample-and-hold margins of "control", closed-loop transfer
  functions, models other than N2, the four-lane layout of mechanisms wider than 8 variables.

Host side only: parsing and validation, the conversion to physical units (sensitivity.to_physical's factors), the result
entry, a numpy restatement of the sweep (``emulate``) for the tests, and ``crossover`` (ultimate gain and frequency of a
scalar response on the grid).
"""
import numpy as np

from . import sensitivity

KEY = "frequency-response"
DEFINE = "RMT_FREQ"
DEFINE_NP = "RMT_FREQ_NP"
MAX_INPUTS = 4
MAX_FREQUENCIES = 4096
MAX_VARIABLES = 8            # wider mechanisms run one node on four lanes on the device: no sweep for them
KEYS = ("inputs", "frequencies", "profile")
MODELS = ("N2",)


def check_model(modelInput):
    """NotImplementedError when the input asks for a frequency response on a model that has none (rmtExe, before any
    device work)."""
    if (modelInput.get('solver-config') or {}).get(KEY) is not None and modelInput.get('model') not in MODELS:
        raise NotImplementedError("solver-config 'frequency-response' is only available for model 'N2' (got model %r)"
                                  % (modelInput.get('model'),))


class FrequencyResponse(sensitivity.Sensitivity):
    """A parsed "frequency-response" spec: the inputs as a Sensitivity holds its parameters, ``omegas`` [F], ``profile``."""

    def __init__(self, inputs, omegas, profile):
        super().__init__(inputs)
        self.omegas = np.asarray(omegas, dtype=np.float64)
        self.profile = bool(profile)
        self.F = len(self.omegas)


def frequencies(spec):
    """The grid [F] of a "frequencies" entry, or ValueError."""
    what = "solver-config 'frequency-response': 'frequencies'"
    if isinstance(spec, dict):
        if set(spec) != {"range", "points"}:
            raise ValueError("%s as a dict has the keys 'range' and 'points' (got %s)" % (what, ", ".join(map(repr, spec))))
        rng, n = spec["range"], spec["points"]
        if not isinstance(rng, (list, tuple)) or len(rng) != 2:
            raise ValueError("%s: 'range' must be [w_lo, w_hi]" % what)
        lo, hi = float(rng[0]), float(rng[1])
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
            raise ValueError("%s: 'range' needs 0 < w_lo < w_hi, both finite (got %r)" % (what, rng))
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 2:
            raise ValueError("%s: 'points' must be an integer >= 2 (got %r)" % (what, n))
        w = np.exp(np.linspace(np.log(lo), np.log(hi), int(n)))
        w[0], w[-1] = lo, hi
    elif isinstance(spec, (list, tuple, np.ndarray)) and len(spec) >= 1:
        try:
            w = np.array([float(v) for v in spec], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s must be a list of numbers" % what)
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError("%s: every frequency must be finite and >= 0" % what)
    else:
        raise ValueError("%s must be a non-empty list of numbers or {'range': [w_lo, w_hi], 'points': n}" % what)
    if len(w) > MAX_FREQUENCIES:
        raise ValueError("%s holds %d values, at most %d are supported" % (what, len(w), MAX_FREQUENCIES))
    return w


def parse(modelInput, members_inputs=None, multi_rank=False, V=None):
    """The FrequencyResponse of a run (None when the input has no "frequency-response"), or ValueError /
    NotImplementedError naming the offending key.  ``V``: the mechanism's variables per node, where the caller knows them."""
    cfg = modelInput['solver-config']
    spec = cfg.get(KEY)
    if spec is None:
        return None
    check_model(modelInput)
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'frequency-response' must be a dict with the keys 'inputs' and 'frequencies'")
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'frequency-response': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    plist = spec.get('inputs')
    if not isinstance(plist, (list, tuple)) or len(plist) < 1:
        raise ValueError("solver-config 'frequency-response': 'inputs' must be a non-empty list")
    if len(plist) > MAX_INPUTS:
        raise ValueError("solver-config 'frequency-response': 'inputs' holds %d entries, at most %d are supported"
                         % (len(plist), MAX_INPUTS))
    comps = list(modelInput['feed']['components']['shell'])
    known = "%s, {'%s': component}" % (", ".join(sensitivity.BOUNDARY), sensitivity.COMPOSITION)
    out = []
    for p in plist:
        if isinstance(p, str) and p in sensitivity.BOUNDARY:
            item = (sensitivity.BOUNDARY.index(p), None)
        elif isinstance(p, dict) and len(p) == 1 and sensitivity.COMPOSITION in p:
            nm = p[sensitivity.COMPOSITION]
            if nm not in comps:
                raise ValueError("solver-config 'frequency-response': '%s': %r is not a shell component (%s)"
                                 % (sensitivity.COMPOSITION, nm, ", ".join(comps)))
            item = (sensitivity.KIND_CIN, nm)
        elif isinstance(p, dict) and len(p) == 1 and sensitivity.RATE_CONSTANT in p:
            raise ValueError("solver-config 'frequency-response': '%s' is not an input (a rate constant is not a boundary "
                             "value; known: %s)" % (sensitivity.RATE_CONSTANT, known))
        else:
            raise ValueError("solver-config 'frequency-response': unknown input %r in 'inputs' (known: %s)" % (p, known))
        if item in out:
            raise ValueError("solver-config 'frequency-response': duplicate input %r in 'inputs'" % (p,))
        out.append(item)
    if 'frequencies' not in spec:
        raise ValueError("solver-config 'frequency-response': 'frequencies' is missing")
    omegas = frequencies(spec['frequencies'])
    profile = spec.get('profile', False)
    if not isinstance(profile, (bool, np.bool_)):
        raise ValueError("solver-config 'frequency-response': 'profile' must be True or False (got %r)" % (profile,))
    for other in ('deactivation', 'fit'):
        if cfg.get(other) is not None:
            raise NotImplementedError("solver-config 'frequency-response' is not available with '%s': such a run has no "
                                      "single operating point" % other)
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise NotImplementedError("solver-config 'frequency-response' is not available with 'dtype': 'fp32': the sweep is "
                                  "an fp64 kernel")
    if multi_rank:
        raise NotImplementedError("solver-config 'frequency-response' is not available in a multi-rank run")
    if V is not None:
        check_width(V)
    ini = cfg.get('initial')
    if not (ini == "steady" or (isinstance(ini, dict) and ini.get('kind') == "steady")):
        raise ValueError("solver-config 'frequency-response' needs \"initial\": \"steady\": the response is that of the "
                         "steady state the run starts from")
    return FrequencyResponse(out, omegas, profile)


def check_width(V):
    """NotImplementedError for the mechanisms the device runs in its four-lane layout (more than 8 variables per node)."""
    if V > MAX_VARIABLES:
        raise NotImplementedError("solver-config 'frequency-response' needs a mechanism of at most %d variables per node "
                                  "(this one has %d): the sweep has no four-lane form" % (MAX_VARIABLES, V))


def peak_node(y, mech, named):
    """The node of the steady discrete temperature maximum of one member's scaled state [V*N]; -1 for an iso-thermal run."""
    if mech.iso:
        return -1
    Y = np.reshape(np.asarray(y, dtype=np.float64), (mech.V, -1))
    return int(np.argmax(Y[mech.S]*named["Tf"] + named["Tf"]))


def scale_rows(rows, unit, named, mech):
    """The kernel's complex rows [NP][..][V+1] (last axis: scaled state, then the pressure; per unit of the row value) in
    the units of the packed profiles per unit of the input: sensitivity.to_physical's factors on the last axis."""
    rows = np.array(rows, dtype=np.complex128)
    S = mech.S
    rows[..., :S] *= named["Cmax"]
    if not mech.iso:
        rows[..., S] *= named["Tf"]
    return rows/np.asarray(unit).reshape((-1,) + (1,)*(rows.ndim - 1))


def result_entry(fr, rows, table, y, row, named, mech):
    """One member's resModel["frequency-response"]: ``rows`` [F][NP][2][V+1] and ``table`` [F][NP][V+1][N] (or None) from
    the device, ``y`` the converged scaled state [V*N], ``row`` the member row."""
    S, V = mech.S, mech.V
    Y = np.reshape(np.asarray(y, dtype=np.float64), (V, -1))
    N = Y.shape[1]
    p, unit = sensitivity.parameter_values(fr, row, named, mech)
    phys = scale_rows(np.transpose(rows, (1, 0, 2, 3)), unit, named, mech)            # [NP][F][2][V+1]
    outlet, peak = phys[:, :, 0], phys[:, :, 1]
    conc = np.maximum(Y[:S, -1], 1e-30)*named["Cmax"]             # (the linear map of sensitivity.result_entry)
    dconc = np.where(Y[:S, -1] > 1e-30, outlet[..., :S], 0.0)
    ctot = conc.sum()
    dx = dconc/ctot - conc*dconc.sum(axis=-1, keepdims=True)/ctot**2
    entry = {"inputs": list(fr.labels), "values": p, "frequencies": fr.omegas.copy(),
             "labelList": list(mech.compList) + ([] if mech.iso else ["Temperature"]),
             "outlet-state": outlet[..., :V].copy(), "outlet-pressure": outlet[..., V].copy(), "outlet-mole-fraction": dx,
             "outlet-temperature": None, "peak-temperature": None, "peak-position": None}
    if not mech.iso:
        n = peak_node(y, mech, named)
        entry["outlet-temperature"] = outlet[..., S].copy()
        entry["peak-temperature"] = peak[..., S].copy()
        entry["peak-position"] = float(np.linspace(0, 1, N)[n]) if N > 1 else 1.0
    if table is not None:
        full = scale_rows(np.transpose(table, (1, 0, 3, 2)), unit, named, mech)      # [NP][F][N][V+1]
        entry["state"] = np.ascontiguousarray(np.transpose(full[..., :V], (0, 1, 3, 2)))
        entry["pressure"] = np.ascontiguousarray(full[..., V])
    return entry


def emulate(blocks, seeds, omegas):
    """The sweep in numpy, for the tests: the complex twin of sensitivity.emulate, with the same ``blocks`` and ``seeds``.
    Returns [F][NP][V+1][N] complex as the kernel writes a lane's table."""
    sd0, pi0 = (np.array(v, dtype=np.float64) for v in seeds)
    NP, V = sd0.shape
    out = np.zeros((len(omegas), NP, V + 1, len(blocks)), dtype=np.complex128)
    for f, w in enumerate(omegas):
        sd, pi = sd0.astype(np.complex128), pi0.astype(np.complex128)
        for z, b in enumerate(blocks):
            a = np.asarray(b["a"], dtype=np.float64) + 1j*float(w)*np.eye(V)
            rhs = np.asarray(b["U"])[None, :]*sd + np.asarray(b["fP"])[None, :]*pi[:, None] + np.asarray(b["fp"])
            s = np.linalg.solve(a, rhs.T).T
            out[f, :, :V, z], out[f, :, V, z] = s, pi
            sd = np.asarray(b["D"])[None, :]*s
            pi = b["az"]*pi + b["P"]*(s @ np.asarray(b["daz"]))
    return out


def crossover(frequencies, G):
    """(w_u, K_u) of a scalar response G [F] on the grid ``frequencies`` [F] (ascending, from 0 or from well below the
    first corner, where G has the sign of the static gain G(0)): the first frequency at which the unwrapped phase relative
    to G(0) - that is, to 0 or 180 degrees by the sign of Re G[0] - crosses -180 degrees
    (interpolated linearly in log w, or in w from a grid point at 0) and 1/|G| there (|G| interpolated in log-log) - the
    ultimate frequency and gain of a proportional loop around G.  None when the phase never gets there."""
    w = np.asarray(frequencies, dtype=np.float64)
    G = np.asarray(G, dtype=np.complex128)
    if w.ndim != 1 or G.shape != w.shape or len(w) < 2 or np.any(np.diff(w) <= 0) or not np.all(np.isfinite(G)):
        raise ValueError("crossover: frequencies [F] ascending and G [F] finite, F >= 2")
    if G[0] == 0:
        return None
    phase = np.unwrap(np.angle(G if G[0].real >= 0 else -G))      # G(0) is real: its sign is all the reference there is
    below = np.nonzero(phase <= -np.pi)[0]
    if len(below) == 0:
        return None
    k = int(below[0])
    if k == 0:
        return None
    t = (-np.pi - phase[k - 1])/(phase[k] - phase[k - 1])
    mag = np.abs(G)
    if w[k - 1] > 0:
        wu = float(np.exp(np.log(w[k - 1]) + t*(np.log(w[k]) - np.log(w[k - 1]))))
    else:
        wu = float(w[k - 1] + t*(w[k] - w[k - 1]))
    if mag[k - 1] > 0 and mag[k] > 0:
        gu = float(np.exp(np.log(mag[k - 1]) + t*(np.log(mag[k]) - np.log(mag[k - 1]))))
    else:
        gu = float(mag[k - 1] + t*(mag[k] - mag[k - 1]))
    return wu, (1.0/gu if gu > 0 else float("inf"))
