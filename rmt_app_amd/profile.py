"""Axial profiles of the dynamic model N2 (solver-config "axial-profile"): catalyst activity and coolant zones.

    "axial-profile": {
        "position":           [0.0, 0.3, 0.3, 1.0],      # z/L, first 0, last 1, non-decreasing
        "catalyst-activity":  [0.4, 0.4, 1.0, 1.0],      # (optional) multiplies every reaction rate, >= 0
        "medium-temperature": [533, 533, 513, 513],      # (optional) K, coolant temperature along the bed, > 0
    }

* Each given quantity is piecewise linear in z/L between the breakpoints; a repeated position is a jump.
* The mesh nodes sit at z_n = n/(N-1), n = 0..N-1.  A node exactly on a jump takes the value behind it (right-continuous,
  the rule schedule.Schedule.at has in time); node N-1 takes the last value.
* A quantity that is not given stays the member's own: activity 1, external-heat MeTe.
* Per member and node the device holds a_n and delta_n = Tm(z_n) - MeTe of the member (csrc/kernels/12_profile.inc): the
  node function uses r_q <- a_n r_q for every reaction q - species sources and heat of reaction alike - and the wall term
  UA (tm + delta_n - T), tm being the member's medium temperature as it is at that stage.  With "schedule" or "control"
  moving 'medium-temperature' the coolant is therefore Tm(t) + delta(z): the zones keep their offsets, the common level
  moves.
* a = 0 is allowed: inert packing.
* 'medium-temperature' needs a wall: a member with MeTe = 0 (the adiabatic switch) or process-type "iso-thermal" raises,
  as in schedule.parse.  Activity alone is allowed in iso-thermal runs.
* Ensembles: "position" comes from the base input; a member of the list form may carry its own 'catalyst-activity' /
  'medium-temperature' under its own solver-config["axial-profile"]; a member "position" that differs raises.
* The upwind stencil, the Ergun recurrence and the scaling are untouched: the steady state stays block lower-bidiagonal
  and "initial": "steady" is the steady state of the profiled bed.
* Not built: models other than N2, fp32, multi-rank runs, the multistep methods, the chained kernels and the stiff
  stepper's four-lane layout (mechanisms wider than 8 variables per node; the explicit steppers and the march serve them).

Host side only (numpy): parsing and validation, the node values (the table [E][2][N] the device reads) and the result
entry.
"""
import numpy as np

ACTIVITY, COOLANT = "catalyst-activity", "medium-temperature"
KEYS = ("position", ACTIVITY, COOLANT)
MODELS = ("N2",)
DEFINE = "RMT_PROFILE"
WIDE = 8                 # codeplan.ros4_quad: beyond this many variables per node the stiff stepper runs its four-lane layout


def check_model(modelInput):
    """ValueError when the input asks for an axial profile on a model that has none (rmtExe, before any device work)."""
    if (modelInput.get('solver-config') or {}).get('axial-profile') is not None and modelInput.get('model') not in MODELS:
        raise ValueError("solver-config 'axial-profile' (catalyst activity / coolant zones along the bed) is only "
                         "available for model 'N2' (got model %r)" % (modelInput.get('model'),))


def node_positions(N):
    """z_n = n/(N-1), n = 0..N-1: the mesh of the N2 discretisation (dz = 1/(zNo-1))"""
    N = int(N)
    return np.arange(N, dtype=np.float64)/float(N - 1)


def node_values(position, values, N):
    """The piecewise-linear function (position [K], values [K]) at the N mesh nodes: right-continuous at a repeated
    position, the last value at and behind the last breakpoint."""
    p = np.asarray(position, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    z = node_positions(N)
    k = np.searchsorted(p, z, side="right") - 1
    last = k >= len(p) - 1
    k0 = np.clip(k, 0, max(len(p) - 2, 0))
    k1 = np.minimum(k0 + 1, len(p) - 1)
    span = p[k1] - p[k0]
    out = v[k0] + np.where(span > 0, (v[k1] - v[k0])*(z - p[k0])/np.where(span > 0, span, 1.0), 0.0)
    return np.where(last, v[-1], out)


class Profile:
    """A parsed "axial-profile" of E members on N nodes: ``position`` [K] (the breakpoints), ``z`` [N], ``activity``
    [E][N], ``delta`` [E][N] = Tm(z_n) - MeTe of the member, ``mete`` [E], ``given`` (activity?, coolant?)."""

    def __init__(self, position, activity, delta, mete, given):
        self.position = np.asarray(position, dtype=np.float64)
        self.activity = np.ascontiguousarray(activity, dtype=np.float64)
        self.delta = np.ascontiguousarray(delta, dtype=np.float64)
        self.mete = np.asarray(mete, dtype=np.float64)
        self.given = tuple(bool(g) for g in given)
        self.E, self.N = self.activity.shape
        self.z = node_positions(self.N)
        # what the run records: solver-config "device-mode" and the kernel forms the host fixed (n2.parse_keys, n2.fix_mode)
        self.want_mode, self.modes = None, {}

    def table(self):
        """[E][2][N] doubles: what rmt_n2_set_profile uploads (per member the activities, then the coolant offsets)"""
        return np.ascontiguousarray(np.stack([self.activity, self.delta], axis=1))


def _check_values(key, vals, n, who=""):
    try:
        arr = np.array(vals, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("solver-config 'axial-profile'%s: %r must be a list of numbers" % (who, key))
    if arr.ndim != 1 or len(arr) != n:
        raise ValueError("solver-config 'axial-profile'%s: %r has %s entries, 'position' has %d"
                         % (who, key, arr.shape[0] if arr.ndim == 1 else "nested", n))
    if not np.all(np.isfinite(arr)):
        raise ValueError("solver-config 'axial-profile'%s: %r holds a value that is not finite" % (who, key))
    return arr


def _n_vars(modelInput):
    from .plan import build_component_list
    iso = modelInput['operating-conditions'].get('process-type') == "iso-thermal"
    return len(build_component_list(modelInput['feed']['components'])) + (0 if iso else 1)


def parse(modelInput, members_inputs=None, ivp=None, multi_rank=False):
    """The Profile of a run (None when the base input has no "axial-profile"), or ValueError / NotImplementedError naming
    'axial-profile' and the offending key.  ``ivp``: the resolved device stepper; ``members_inputs``: the ensemble members
    (default: the base input alone)."""
    cfg = modelInput['solver-config']
    spec = cfg.get('axial-profile')
    if spec is None:
        return None
    check_model(modelInput)
    if ivp in ("AM", "hip-ab3"):
        raise ValueError("solver-config 'axial-profile' cannot be combined with 'ivp': %r - the multistep kernel does not "
                         "carry the profile (use hip-rk4, hip-rk45, hip-ros4 or 'default')" % (cfg.get('ivp'),))
    if cfg.get('device-mode') == "chain":
        raise ValueError("solver-config 'axial-profile' cannot be combined with 'device-mode': 'chain' - the chained "
                         "kernels do not carry the profile ('reg' or 'mem')")
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'axial-profile' must be a dict with the keys %s" % (KEYS,))
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'axial-profile': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    if 'position' not in spec:
        raise ValueError("solver-config 'axial-profile' needs 'position': the breakpoints in z/L")
    try:
        pos = np.array(spec['position'], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("solver-config 'axial-profile': 'position' must be a list of numbers")
    if pos.ndim != 1 or len(pos) < 2 or not np.all(np.isfinite(pos)):
        raise ValueError("solver-config 'axial-profile': 'position' must be a list of at least two finite numbers")
    if pos[0] != 0.0 or pos[-1] != 1.0:
        raise ValueError("solver-config 'axial-profile': 'position' must start at 0 and end at 1 (got %r .. %r)"
                         % (float(pos[0]), float(pos[-1])))
    if np.any(np.diff(pos) < 0):
        raise ValueError("solver-config 'axial-profile': 'position' must not decrease")
    from .settings import solverSetting
    N = int(cfg.get('zNo', solverSetting['N2']['zNo']))
    inputs = list(members_inputs) if members_inputs else [modelInput]
    iso = modelInput['operating-conditions'].get('process-type') == "iso-thermal"
    K = len(pos)
    act = np.ones((len(inputs), N))
    delta = np.zeros((len(inputs), N))
    mete = np.zeros(len(inputs))
    given = [False, False]
    for e, mi in enumerate(inputs):
        who = "" if mi is modelInput else " of member %d" % e
        own = (mi.get('solver-config') or {}).get('axial-profile') if mi is not modelInput else None
        if own is not None:
            if not isinstance(own, dict):
                raise ValueError("solver-config 'axial-profile' of member %d must be a dict" % e)
            for k in own:
                if k not in KEYS:
                    raise ValueError("solver-config 'axial-profile' of member %d: unknown key %r" % (e, k))
            if 'position' in own:
                try:
                    opos = np.array(own['position'], dtype=np.float64)
                except (TypeError, ValueError):
                    opos = None
                if opos is None or opos.shape != pos.shape or np.any(opos != pos):
                    raise ValueError("solver-config 'axial-profile' of member %d: 'position' differs from the base "
                                     "input's - the breakpoints come from the base input" % e)
        mete[e] = float(mi['external-heat']['MeTe'])
        src = own if (own is not None and ACTIVITY in own) else spec
        if ACTIVITY in src:
            given[0] = True
            arr = _check_values(ACTIVITY, src[ACTIVITY], K, who)
            if np.any(arr < 0):
                raise ValueError("solver-config 'axial-profile'%s: %r must not be negative (got %g)"
                                 % (who, ACTIVITY, float(np.min(arr))))
            act[e] = node_values(pos, arr, N)
        src = own if (own is not None and COOLANT in own) else spec
        if COOLANT in src:
            given[1] = True
            if iso:
                raise ValueError("solver-config 'axial-profile': %r needs an energy balance - process-type 'iso-thermal' "
                                 "has none (%r alone is allowed)" % (COOLANT, ACTIVITY))
            arr = _check_values(COOLANT, src[COOLANT], K, who)
            if mete[e] == 0:
                raise ValueError("solver-config 'axial-profile': %r needs a member with external-heat MeTe > 0 (MeTe = 0 "
                                 "is the adiabatic switch); member %d has MeTe = 0" % (COOLANT, e))
            if np.any(arr <= 0):
                raise ValueError("solver-config 'axial-profile'%s: %r must be positive (got %g K)"
                                 % (who, COOLANT, float(np.min(arr))))
            delta[e] = node_values(pos, arr, N) - mete[e]
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise NotImplementedError("solver-config 'axial-profile' is not available with 'dtype': 'fp32': the profiled "
                                  "kernels are fp64")
    if multi_rank:
        raise NotImplementedError("solver-config 'axial-profile' is not available in a multi-rank run")
    if ivp in ("hip-ros4", "hip-auto") and _n_vars(modelInput) > WIDE:
        raise NotImplementedError("solver-config 'axial-profile' with the stiff stepper ('ivp': %r) needs a mechanism of "
                                  "at most %d variables per node (this one has %d): its four-lane form does not carry the "
                                  "profile - use ivp 'hip-rk45' or 'hip-rk4'" % (cfg.get('ivp'), WIDE, _n_vars(modelInput)))
    return Profile(pos, act, delta, mete, given)


def result_entry(prof, e=0):
    """resModel["axial-profile"] of member e: the node values the device used; the coolant row holds the t = 0 values
    MeTe + delta_n."""
    return {"position": prof.z.copy(), ACTIVITY: prof.activity[e].copy(), COOLANT: prof.mete[e] + prof.delta[e]}
