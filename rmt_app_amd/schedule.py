"""Time-varying inlet and coolant conditions of the dynamic model N2 (solver-config "schedule").

    "schedule": {
        "time":               [0.0, 0.10, 0.20, 0.20, 0.5],    # s, non-decreasing, first entry 0
        "inlet-temperature":  [523, 523,  533,  528,  528],    # K    (optional)
        "inlet-pressure":     [5e6, 5e6,  5e6,  4.9e6, 4.9e6], # Pa   (optional)
        "medium-temperature": [523, 523,  523,  533,  533],    # K    (optional)
        "inlet-concentration": [[574.9, 287.4, 0.01, 287.4, 0.01, 0.01], ...],   # (optional) one row per breakpoint, one
                               # entry per shell component, in the order and unit of feed["concentration"]
        "relative": False,     # True: the values are offsets added to each member's own T, P, MeTe, feed concentration
    }

* Each given quantity is piecewise linear in time between the breakpoints.
* A repeated time is a jump: the left value holds up to that time, the right value from it on.
* After the last breakpoint the last value holds.
* A quantity that is not given stays the member's constant.
* Only the boundary values change: the inlet temperature is the upwind value of node 0
  (pbHomoReactor.py:4108), the inlet pressure the start of the pressure march (:3848), the medium
  temperature enters the wall term (:4036-4045).  All scaling constants, the initial state and everything
  derived from the feed stay those of the member's own input at t = 0 - what the reference's RHS computes
  when only constBC1['T0'], constBC1['P0'] and ExHe['MeTe'] are replaced.
* The feed composition ("inlet-concentration") follows the same rule: only node 0's upstream concentration becomes
  C_in,i(t)/Cmax (:4090).  Cmax = max(feed concentration) - the scaling of the state and of the result - GaMaCoTe0, GaDe0,
  Cp0, the Ergun coefficients and the initial state stay those of the member's own feed at t = 0.  That equals the
  reference's modelEquationN2 with only constBC1['SpCoi0'] replaced exactly when the disturbance leaves max(SpCoi0)
  unchanged: the reference takes its scaling from the same entry (:3901), so a disturbance that changes the maximum has
  no reference counterpart (here the scaling simply stays the member's own).  Each species is piecewise linear; entries
  are finite and >= 0 with at least one > 0 per breakpoint; iso-thermal runs may schedule it (no energy balance needed).
* The integration is split at every distinct breakpoint inside (0, period) in addition to the output times,
  so inside one launch every forced quantity is ONE linear function of t; the kernels evaluate it at every
  stage time from the launch's start values and slopes (csrc/kernels/11_forcing.inc).
* Ensembles: the breakpoint times come from the base input; a member may carry its own values under its
  own solver-config.schedule; with "relative": True one schedule applies to every member of a T/P sweep.

Host side only (numpy): parsing and validation, per launch and member the values at
the launch start and the slopes, and ``rows_at(t)`` - ordinary member rows with the forced fields at time t.
"""
import numpy as np

from . import plan
from .launches import MERGE_TOL     # noqa: F401  (a breakpoint this close, relative to the period, to an output time IS it)

# schedule key -> (where the member's own constant lives in the model input, unit)
QUANTITIES = {
    "inlet-temperature": (("operating-conditions", "temperature"), "K"),
    "inlet-pressure": (("operating-conditions", "pressure"), "Pa"),
    "medium-temperature": (("external-heat", "MeTe"), "K"),
}
ORDER = ("inlet-temperature", "inlet-pressure", "medium-temperature")     # columns of every [E][3] array below
COMPOSITION = "inlet-concentration"       # [K][S] per member, beside the three scalars: Schedule.conc
KEYS = ("time", "relative") + ORDER + (COMPOSITION,)
TAIL = 4          # doubles a forced member row carries behind the ordinary ones: t_ref and the three slopes
#                   (a schedule that moves the composition: S more, the slopes of CIN - Schedule.tail)


def _own(mi, key):
    a, b = QUANTITIES[key][0]
    return float(mi[a][b])


class Schedule:
    """Parsed schedule of E members: ``times`` [K], ``values`` [E][3][K] (absolute; a quantity that is not
    scheduled repeats the member's constant), ``given`` [3] which quantities are scheduled; ``conc`` [E][S][K] the
    inlet concentrations in the unit of feed["concentration"] (a member without the key repeats its own feed), None when
    no member schedules the composition."""

    def __init__(self, times, values, given, relative=False, conc=None):
        self.times = np.asarray(times, dtype=np.float64)
        self.values = np.asarray(values, dtype=np.float64)
        self.given = tuple(bool(g) for g in given)
        self.relative = bool(relative)
        self.E = self.values.shape[0]
        self.conc = None if conc is None else np.asarray(conc, dtype=np.float64)

    def members(self, lo, hi):
        """The schedule of members lo..hi-1 (one rank's block of an ensemble)."""
        return Schedule(self.times, self.values[lo:hi], self.given, self.relative,
                        None if self.conc is None else self.conc[lo:hi])

    @property
    def tail(self):
        """doubles a forced member row of this schedule carries behind the ordinary ones: TAIL, or TAIL + S"""
        return TAIL if self.conc is None else TAIL + self.conc.shape[1]

    @property
    def forcing_level(self):
        """the RMT_FORCING value of the code object that evaluates this schedule (csrc/kernels/11_forcing.inc)"""
        return "1" if self.conc is None else "2"

    # -- the piecewise-linear functions
    def _segment(self, t, side):
        T = self.times
        k = int(np.searchsorted(T, t, side="right" if side == "right" else "left")) - 1
        return k

    def at(self, t, side="right"):
        """[E][3] values (T_in [K], P_in [Pa], MeTe [K]) at time t; at a jump ``side`` picks the value that holds
        from t on ("right", the default) or the one that held up to t ("left")."""
        return self._at(self.values, t, side)

    def conc_at(self, t, side="right"):
        """[E][S] inlet concentrations at time t (``side`` as in ``at``); None when the composition is not scheduled."""
        return None if self.conc is None else self._at(self.conc, t, side)

    def _at(self, v, t, side):
        T = self.times
        k = self._segment(float(t), side)
        if k < 0:
            return v[:, :, 0].copy()
        if k >= len(T) - 1:
            return v[:, :, -1].copy()
        w = (float(t) - T[k])/(T[k + 1] - T[k])
        return v[:, :, k] + (v[:, :, k + 1] - v[:, :, k])*w

    def launch(self, t0, t1):
        """(values [E][3] at t0, slopes [E][3] per second) of the ONE linear piece that holds over the launch (t0, t1)
        - the launch must not straddle a breakpoint (launches.merge sees to that)."""
        return self._launch(self.values, t0, t1)

    def conc_launch(self, t0, t1):
        """(concentrations [E][S] at t0, slopes [E][S] per second) of the launch (t0, t1); None when not scheduled."""
        return None if self.conc is None else self._launch(self.conc, t0, t1)

    def _launch(self, v, t0, t1):
        T = self.times
        k = self._segment(0.5*(float(t0) + float(t1)), "right")
        if k >= len(T) - 1:
            return v[:, :, -1].copy(), np.zeros(v.shape[:2])
        slope = (v[:, :, k + 1] - v[:, :, k])/(T[k + 1] - T[k])
        return v[:, :, k] + slope*(float(t0) - T[k]), slope

    # -- member rows
    def rows_at(self, rows, named, t, side="right"):
        """The ordinary member rows with THETA_IN, P0 and TM at time t (what an unforced kernel - or the host build of
        the generated source - needs to evaluate the forced right-hand side at that time)."""
        rows = np.array(rows, dtype=np.float64).reshape(self.E, -1)
        plan.forced_fields(rows, named, self.at(t, side))
        if self.conc is not None:
            plan.forced_composition(rows, named, self.conc_at(t, side))
        return rows

    def forced_rows(self, rows, named, t0, t1):
        """Member rows of a forced code object for the launch (t0, t1): the ordinary fields hold the values at t_ref = t0,
        the tail of TAIL doubles t_ref and the slopes of THETA_IN, P0 and TM - and, when the composition is scheduled,
        CIN at t_ref and S more doubles, the slopes of CIN."""
        rows = np.array(rows, dtype=np.float64).reshape(self.E, -1)
        w = rows.shape[1]
        out = np.zeros((self.E, w + self.tail))
        out[:, :w] = rows
        v0, slope = self.launch(t0, t1)
        plan.forced_fields(out, named, v0)
        out[:, w] = float(t0)
        out[:, w + 1:w + TAIL] = plan.forced_slopes(named, slope)
        if self.conc is not None:
            c0, cslope = self.conc_launch(t0, t1)
            plan.forced_composition(out, named, c0)
            out[:, w + TAIL:] = plan.forced_composition_slopes(named, cslope)
        return out


def _check_values(key, vals, n):
    try:
        arr = np.array(vals, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("solver-config 'schedule': %r must be a list of numbers" % key)
    if arr.ndim != 1 or len(arr) != n:
        raise ValueError("solver-config 'schedule': %r has %s entries, 'time' has %d"
                         % (key, arr.shape[0] if arr.ndim == 1 else "nested", n))
    if not np.all(np.isfinite(arr)):
        raise ValueError("solver-config 'schedule': %r holds a value that is not finite" % key)
    return arr


def _check_composition(vals, n, S, e):
    try:
        arr = np.array(vals, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("solver-config 'schedule': %r must be a list of rows of numbers (member %d)" % (COMPOSITION, e))
    if arr.ndim != 2 or arr.shape[0] != n:
        raise ValueError("solver-config 'schedule': %r has %s rows, 'time' has %d (member %d; one row per breakpoint)"
                         % (COMPOSITION, arr.shape[0] if arr.ndim >= 1 else "no", n, e))
    if arr.shape[1] != S:
        raise ValueError("solver-config 'schedule': %r rows have %d entries, the feed has %d shell components (member %d)"
                         % (COMPOSITION, arr.shape[1], S, e))
    if not np.all(np.isfinite(arr)):
        raise ValueError("solver-config 'schedule': %r holds a value that is not finite (member %d)" % (COMPOSITION, e))
    return arr


def parse(modelInput, members_inputs=None, ivp=None):
    """The Schedule of a run (None when the base input has no "schedule"), or ValueError naming the offending key.
    ``ivp``: the resolved device stepper; ``members_inputs``: the ensemble members (default: the base input alone)."""
    cfg = modelInput['solver-config']
    spec = cfg.get('schedule')
    if spec is None:
        return None
    if modelInput.get('model', 'N2') != "N2":
        raise ValueError("solver-config 'schedule' is only available for model 'N2' (got model %r)"
                         % (modelInput.get('model'),))
    if ivp in ("AM", "hip-ab3"):
        raise ValueError("solver-config 'schedule' cannot be combined with 'ivp': %r - the multistep history does not "
                         "survive a breakpoint (use hip-rk4, hip-rk45, hip-ros4 or 'default')" % (cfg.get('ivp'),))
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise ValueError("solver-config 'schedule' cannot be combined with 'dtype': 'fp32' (fp64 only)")
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'schedule' must be a dict with the keys %s" % (KEYS,))
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'schedule': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    if 'time' not in spec:
        raise ValueError("solver-config 'schedule' needs 'time': the breakpoint times [s]")
    times = np.array(spec['time'], dtype=np.float64)
    if times.ndim != 1 or len(times) < 1 or not np.all(np.isfinite(times)):
        raise ValueError("solver-config 'schedule': 'time' must be a non-empty list of finite numbers")
    if times[0] != 0.0:
        raise ValueError("solver-config 'schedule': 'time' must start at 0 (got %r)" % (float(times[0]),))
    if np.any(np.diff(times) < 0):
        raise ValueError("solver-config 'schedule': 'time' must not decrease")
    inputs = list(members_inputs) if members_inputs else [modelInput]
    iso = modelInput['operating-conditions'].get('process-type') == "iso-thermal"
    K = len(times)
    values = np.zeros((len(inputs), 3, K))
    given = [False, False, False]
    conc = [None]*len(inputs)
    for e, mi in enumerate(inputs):
        own = (mi.get('solver-config') or {}).get('schedule') if mi is not modelInput else None
        if own is not None:
            if not isinstance(own, dict):
                raise ValueError("solver-config 'schedule' of member %d must be a dict" % e)
            for k in own:
                if k not in KEYS:
                    raise ValueError("solver-config 'schedule' of member %d: unknown key %r" % (e, k))
            if 'time' in own and (len(own['time']) != K or np.any(np.array(own['time'], dtype=np.float64) != times)):
                raise ValueError("solver-config 'schedule' of member %d: 'time' differs from the base input's - the "
                                 "breakpoint times come from the base input" % e)
        relative = bool((own or {}).get('relative', spec.get('relative', False)))
        for q, key in enumerate(ORDER):
            src = own if (own is not None and key in own) else spec
            base = _own(mi, key)
            if key not in src:
                values[e, q, :] = base
                continue
            given[q] = True
            if iso and key != "inlet-pressure":
                raise ValueError("solver-config 'schedule': %r needs an energy balance - process-type 'iso-thermal' "
                                 "has none ('inlet-pressure' is allowed)" % key)
            arr = _check_values(key, src[key], K)
            if key == "medium-temperature" and base == 0:
                raise ValueError("solver-config 'schedule': 'medium-temperature' needs a member with external-heat MeTe "
                                 "> 0 (MeTe = 0 is the adiabatic switch); member %d has MeTe = 0" % e)
            v = base + arr if relative else arr
            if np.any(v <= 0):
                raise ValueError("solver-config 'schedule': %r must stay positive (member %d reaches %g %s)"
                                 % (key, e, float(np.min(v)), QUANTITIES[key][1]))
            values[e, q, :] = v
        src = own if (own is not None and COMPOSITION in own) else spec
        if COMPOSITION in src:
            feed = np.array(mi['feed']['concentration'], dtype=np.float64).reshape(-1)
            arr = _check_composition(src[COMPOSITION], K, len(feed), e)
            c = feed + arr if relative else arr
            if np.any(c < 0):
                raise ValueError("solver-config 'schedule': %r must not be negative (member %d reaches %g)"
                                 % (COMPOSITION, e, float(np.min(c))))
            if not np.all(np.max(c, axis=1) > 0):
                raise ValueError("solver-config 'schedule': %r needs at least one positive entry per breakpoint "
                                 "(member %d, breakpoint %d)" % (COMPOSITION, e, int(np.argmin(np.max(c, axis=1)))))
            conc[e] = c.T
    # a quantity that only SOME members schedule: the others keep their constant (filled above)
    if any(c is not None for c in conc):
        conc = np.array([np.repeat(np.array(mi['feed']['concentration'], dtype=np.float64).reshape(-1, 1), K, axis=1)
                         if c is None else c for c, mi in zip(conc, inputs)])
    else:
        conc = None
    return Schedule(times, values, given, bool(spec.get('relative', False)), conc)


def result_entry(sched, out_times):
    """resModel["schedule"]: the forced values of the base member (member 0) at the output times."""
    vals = np.array([sched.at(t)[0] for t in out_times])
    out = {"time": np.array(out_times, dtype=np.float64), "inlet-temperature": vals[:, 0],
           "inlet-pressure": vals[:, 1], "medium-temperature": vals[:, 2]}
    if sched.conc is not None:          # [tNo][S], only when the key was given
        out[COMPOSITION] = np.array([sched.conc_at(t)[0] for t in out_times])
    return out
