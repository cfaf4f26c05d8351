"""Closed-loop runs of the dynamic model N2: one sampled PI controller per member, evaluated on the device
(solver-config "control").

    "control": {
        "measured":      "outlet-temperature" | "peak-temperature" | {"outlet-mole-fraction": "<shell component>"},
        "manipulated":   "inlet-pressure" | "inlet-temperature" | "medium-temperature",     # a schedule.ORDER key
        "setpoint":      620.0  |  {"time": [...], "value": [...]},    # piecewise linear, the rules of schedule "time"
        "sample-time":   0.01,           # Ts > 0 [s]
        "start":         0.1,            # first sample time [s], default 0.0
        "gain":          5.0e4,          # Kp, manipulated unit per measured unit, may be negative
        "integral-time": 0.05,           # Ti > 0 [s]; absent / None = P only
        "limits":        [4.0e6, 6.0e6]  # lo < hi, both > 0, required
    }

* Sample times are t_k = start + k Ts < period.  At t_k the measured value pv_k is taken from the state at t_k, before the
  launch that starts there.
* The control law (fp64, positional form, conditional-integration anti-windup):

      e = r(t_k) - pv_k;   I' = I + (Kp*Ts/Ti)*e   (I' = I when P only)
      v = u0 + Kp*e + I';  u_k = min(max(v, lo), hi);   I = I' only if v == u_k

  u0 is the member's own constant (schedule._own), I starts at 0, u_k holds (zero order) until t_{k+1}; before "start" the
  manipulated quantity is the member's own.
* Measured quantities: temperatures in K, theta*Tf + Tf with Tf from the member row; "peak-temperature" is the largest
  value of the temperature row over all nodes (plain >, a NaN never wins, as in the monitor); a mole fraction is
  C_s[N-1] / sum_i C_i[N-1] of the raw state.
* "control" combines with "schedule" - the schedule moves the disturbances, the controller its own quantity; a schedule
  that also gives the manipulated key is refused.  A run without "schedule" uses a constant schedule of the member's own
  values: a controlled run always loads a forced code object (csrc/kernels/11_forcing.inc).
* The integration is split at the sample times as "monitor" splits it at its samples (launches.merge); a sample time within
  schedule.MERGE_TOL * period of an output time, a breakpoint or a monitor sample IS that time.
* Ensembles: every member runs its own loop with its own u0, I and Tf; a member may override "gain", "integral-time",
  "setpoint" and "limits" in its own solver-config.control; the times come from the base input.
* Nothing leaves the device between the launches: a kernel of its own (csrc/control_kernels.inc) measures, evaluates the
  law and writes the manipulated field of the member's device row; the log [K][E][{pv, r, u, saturated}] comes back once,
  at the end of the run, as resModel["control"] = {"time", "measured", "setpoint", "output", "saturated"}.

Host side only (numpy): parsing and validation, the sample times, the parameter blocks of the
kernel and ``emulate`` - the law in numpy.
"""
import numpy as np

from . import schedule
from .schedule import MERGE_TOL, ORDER

KEYS = ("measured", "manipulated", "setpoint", "sample-time", "start", "gain", "integral-time", "limits")
MEMBER_KEYS = ("gain", "integral-time", "setpoint", "limits")        # what a member may override
MEASURED = ("outlet-temperature", "peak-temperature", "outlet-mole-fraction")       # the kernel's selector 0, 1, 2
MOLE_FRACTION = "outlet-mole-fraction"
# the parameter block of one member (csrc/control_kernels.inc RMT_CTL_*): eight doubles
PARAMS = 8
P_KP, P_KI, P_U0, P_LO, P_HI, P_SELECT, P_SPECIES, P_RESERVED = range(PARAMS)
STATE = 3              # doubles of controller state per member: I, u, number of samples taken
LOG = 4                # doubles per (sample, member): pv, r, u, saturated (0.0 / 1.0)


def check_model(modelInput):
    """ValueError when the input asks for a controller on a model that has none (rmtExe, before any device work)."""
    if (modelInput.get('solver-config') or {}).get('control') is not None and modelInput.get('model') != "N2":
        raise ValueError("solver-config 'control' (sampled PI controller on the device) is only available for model 'N2' "
                         "(got model %r)" % (modelInput.get('model'),))


def sample_times(start, Ts, period):
    """[K] sample times t_k = start + k*Ts < period"""
    out, k = [], 0
    tol = MERGE_TOL*float(period)
    while float(start) + k*float(Ts) < float(period) - tol:
        out.append(float(start) + k*float(Ts))
        k += 1
    return np.array(out, dtype=np.float64)


def setpoint_at(times, values, t, tol=0.0):
    """The piecewise-linear setpoint at time t: at a jump the value that holds from t on, behind the last breakpoint the
    last value.  A t within ``tol`` of a breakpoint is that breakpoint."""
    T = np.asarray(times, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    t = float(t)
    j = int(np.argmin(np.abs(T - t)))
    if abs(T[j] - t) <= tol:
        t = float(T[j])
    k = int(np.searchsorted(T, t, side="right")) - 1
    if k < 0:
        return float(v[0])
    if k >= len(T) - 1:
        return float(v[-1])
    return float(v[k] + (v[k + 1] - v[k])*(t - T[k])/(T[k + 1] - T[k]))


def emulate(pv, r, Kp, Ki, u0, lo, hi, I0=0.0):
    """The control law in numpy, sample by sample, for ONE member: measured values ``pv`` [K] and setpoints ``r`` [K]
    (or one number) -> (u [K], saturated [K] bool, I [K] the integral state behind each sample).  ``Ki`` = Kp*Ts/Ti, 0.0
    for a P-only controller.  Every operation is one correctly rounded fp64 operation in the order the kernel takes them
    (csrc/control_kernels.inc, compiled without floating-point contraction): the results are equal bit for bit."""
    pv = np.asarray(pv, dtype=np.float64).reshape(-1)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), pv.shape)
    Kp, Ki, u0, lo, hi = (np.float64(x) for x in (Kp, Ki, u0, lo, hi))
    I = np.float64(I0)
    u, sat, Is = np.zeros(len(pv)), np.zeros(len(pv), dtype=bool), np.zeros(len(pv))
    with np.errstate(all="ignore"):
        for k in range(len(pv)):
            e = r[k] - pv[k]
            Ip = I + Ki*e if Ki != 0.0 else I
            v = (u0 + Kp*e) + Ip
            uk = lo if v < lo else v
            uk = hi if uk > hi else uk
            if v == uk:
                I = Ip
            u[k], sat[k], Is[k] = uk, not (v == uk), I
    return u, sat, Is


def field_value(key, u, Tf):
    """The value of the member-row field that carries the manipulated quantity ``key`` at u, in the row's own scaling - the
    mapping of plan.forced_fields, which the kernel restates: THETA_IN = (T_in - Tf)/Tf, P0 = P_in, TM = MeTe."""
    u, Tf = np.float64(u), np.float64(Tf)
    return (u - Tf)/Tf if key == "inlet-temperature" else u


def row_field(key):
    """(index of the row field, index of its slope in the row's tail) of a manipulated key"""
    from .plan import MEMBER_FIELDS as F
    q = ORDER.index(key)
    return (F["THETA_IN"], F["P0"], F["TM"])[q], 1 + q


class Control:
    """A parsed control spec of E members: ``times`` [K]; per member ``Kp``, ``Ki`` (= Kp*Ts/Ti, 0 when P only), ``u0``,
    ``lo``, ``hi`` [E]; ``setpoints`` [K][E] = r(t_k); ``select`` (index into MEASURED), ``species`` (index of the shell
    component of a mole fraction, else 0), ``manipulated`` (a schedule.ORDER key)."""

    def __init__(self, times, Kp, Ki, u0, lo, hi, setpoints, select, species, manipulated, Ts, start):
        self.times = np.asarray(times, dtype=np.float64)
        self.K = len(self.times)
        self.Kp, self.Ki, self.u0, self.lo, self.hi = (np.asarray(a, dtype=np.float64) for a in (Kp, Ki, u0, lo, hi))
        self.E = len(self.Kp)
        self.setpoints = np.asarray(setpoints, dtype=np.float64).reshape(self.K, self.E)
        self.select, self.species, self.manipulated = int(select), int(species), manipulated
        self.field = ORDER.index(manipulated)
        self.Ts, self.start = float(Ts), float(start)

    def check_budget(self, cap):
        """The device log [K][E][4] doubles and the setpoints [K][E] must not exceed ``cap`` bytes (n2.PIPELINE_BYTES)."""
        need = self.K*self.E*(LOG + 1)*8
        if need > cap:
            raise ValueError("solver-config 'control': %d samples of %d members = %d bytes of log, more than the %d "
                             "allowed - raise 'sample-time'" % (self.K, self.E, need, cap))

    def params(self):
        """[E][PARAMS] parameter blocks of the kernel"""
        out = np.zeros((self.E, PARAMS))
        out[:, P_KP], out[:, P_KI], out[:, P_U0] = self.Kp, self.Ki, self.u0
        out[:, P_LO], out[:, P_HI] = self.lo, self.hi
        out[:, P_SELECT], out[:, P_SPECIES] = float(self.select), float(self.species)
        return out

    def result_entry(self, raw):
        """resModel["control"] of ONE member from its log [K][4]"""
        raw = np.asarray(raw, dtype=np.float64).reshape(self.K, LOG)
        return {"time": self.times.copy(), "measured": raw[:, 0].copy(), "setpoint": raw[:, 1].copy(),
                "output": raw[:, 2].copy(), "saturated": raw[:, 3] != 0.0}


def _number(what, v, positive=False, e=None):
    who = "" if e is None else " (member %d)" % e
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
            or not np.isfinite(float(v)):
        raise ValueError("solver-config 'control': %r must be a finite number%s (got %r)" % (what, who, v))
    if positive and not float(v) > 0:
        raise ValueError("solver-config 'control': %r must be > 0%s (got %r)" % (what, who, v))
    return float(v)


def _setpoint(sp, e=None):
    """(times, values) of a setpoint: a number, or {"time", "value"} with the rules of schedule 'time'"""
    who = "" if e is None else " (member %d)" % e
    if not isinstance(sp, dict):
        return np.array([0.0]), np.array([_number("setpoint", sp, e=e)])
    if set(sp) != {"time", "value"}:
        raise ValueError("solver-config 'control': 'setpoint' must be a number or {'time': [...], 'value': [...]}%s" % who)
    try:
        T, v = np.array(sp["time"], dtype=np.float64), np.array(sp["value"], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("solver-config 'control': 'setpoint' must hold lists of numbers%s" % who)
    if T.ndim != 1 or len(T) < 1 or T.shape != v.shape or not np.all(np.isfinite(T)) or not np.all(np.isfinite(v)):
        raise ValueError("solver-config 'control': 'setpoint' needs 'time' and 'value' of the same length, finite%s" % who)
    if T[0] != 0.0:
        raise ValueError("solver-config 'control': 'setpoint' 'time' must start at 0 (got %r)%s" % (float(T[0]), who))
    if np.any(np.diff(T) < 0):
        raise ValueError("solver-config 'control': 'setpoint' 'time' must not decrease%s" % who)
    return T, v


def parse(modelInput, members_inputs=None, ivp=None, sched=None, multi_rank=False):
    """(Control, Schedule) of a run - (None, ``sched``) when the base input has no "control" - or ValueError /
    NotImplementedError naming the offending key.  ``sched``: the run's parsed schedule (schedule.parse) or None; the
    returned Schedule is that one, or, without a "schedule" key, a constant schedule of every member's own values.
    ``ivp``: the resolved device stepper; ``members_inputs``: the ensemble members (default: the base input alone)."""
    cfg = modelInput['solver-config']
    spec = cfg.get('control')
    if spec is None:
        return None, sched
    check_model(modelInput)
    if ivp in ("AM", "hip-ab3"):
        raise ValueError("solver-config 'control' cannot be combined with 'ivp': %r - the multistep history does not "
                         "survive a sample (use hip-rk4, hip-rk45, hip-ros4 or 'default')" % (cfg.get('ivp'),))
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise ValueError("solver-config 'control' cannot be combined with 'dtype': 'fp32' (fp64 only)")
    if multi_rank:
        raise NotImplementedError("solver-config 'control' is not available in a multi-rank run: the controller's kernel "
                                  "writes the member rows of ONE process (run the ensemble in a single process)")
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'control' must be a dict with the keys %s" % (KEYS,))
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'control': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    for k in ("measured", "manipulated", "setpoint", "sample-time", "gain", "limits"):
        if k not in spec:
            raise ValueError("solver-config 'control' needs %r" % k)
    iso = modelInput['operating-conditions'].get('process-type') == "iso-thermal"
    shell = list(modelInput['feed']['components']['shell'])
    # what is measured
    meas = spec['measured']
    species = 0
    if isinstance(meas, dict):
        if list(meas) != [MOLE_FRACTION]:
            raise ValueError("solver-config 'control': 'measured' as a dict must be {%r: <shell component>} (got %r)"
                             % (MOLE_FRACTION, meas))
        if meas[MOLE_FRACTION] not in shell:
            raise ValueError("solver-config 'control': 'measured' %r is not a shell component (%s)"
                             % (meas[MOLE_FRACTION], ", ".join(shell)))
        select, species = MEASURED.index(MOLE_FRACTION), shell.index(meas[MOLE_FRACTION])
    elif meas in MEASURED[:2]:
        select = MEASURED.index(meas)
        if iso:
            raise ValueError("solver-config 'control': 'measured' %r needs an energy balance - process-type 'iso-thermal' "
                             "has none" % (meas,))
    else:
        raise ValueError("solver-config 'control': 'measured' must be %r, %r or {%r: <shell component>} (got %r)"
                         % (MEASURED[0], MEASURED[1], MOLE_FRACTION, meas))
    # what is moved
    key = spec['manipulated']
    if key not in ORDER:
        raise ValueError("solver-config 'control': 'manipulated' must be one of %s (got %r)" % (", ".join(ORDER), key))
    if iso and key != "inlet-pressure":
        raise ValueError("solver-config 'control': 'manipulated' %r needs an energy balance - process-type 'iso-thermal' "
                         "has none ('inlet-pressure' is allowed)" % key)
    inputs = list(members_inputs) if members_inputs else [modelInput]
    q = ORDER.index(key)
    if sched is not None and sched.given[q]:
        raise ValueError("solver-config 'control' manipulates %r, which the 'schedule' also gives - a quantity has one "
                         "master (drop it from the schedule)" % key)
    for e, mi in enumerate(inputs):
        own = (mi.get('solver-config') or {}).get('schedule') if mi is not modelInput else None
        if isinstance(own, dict) and key in own:
            raise ValueError("solver-config 'control' manipulates %r, which the 'schedule' of member %d also gives" % (key, e))
    # the times (base input)
    period = float(modelInput['operating-conditions']['period'])
    Ts = _number("sample-time", spec['sample-time'], positive=True)
    start = _number("start", spec.get('start', 0.0))
    if start < 0 or not start < period:
        raise ValueError("solver-config 'control': 'start' must lie in [0, period) (period = %g s, got %g)" % (period, start))
    times = sample_times(start, Ts, period)
    tol = MERGE_TOL*period
    # the members' own loops
    E = len(inputs)
    Kp, Ki, u0, lo, hi = (np.zeros(E) for _ in range(5))
    sp = np.zeros((len(times), E))
    for e, mi in enumerate(inputs):
        own = (mi.get('solver-config') or {}).get('control') if mi is not modelInput else None
        who = None if mi is modelInput else e
        if own is not None:
            if not isinstance(own, dict):
                raise ValueError("solver-config 'control' of member %d must be a dict" % e)
            for k in own:
                if k not in KEYS:
                    raise ValueError("solver-config 'control' of member %d: unknown key %r" % (e, k))
                if k not in MEMBER_KEYS and own[k] != spec.get(k):
                    raise ValueError("solver-config 'control' of member %d: %r differs from the base input's - a member "
                                     "may override %s only" % (e, k, ", ".join(MEMBER_KEYS)))
        get = lambda k, d=None: own[k] if (own is not None and k in own) else spec.get(k, d)      # noqa: E731
        Kp[e] = _number("gain", get("gain"), e=who)
        Ti = get("integral-time")
        Ki[e] = 0.0 if Ti is None else Kp[e]*Ts/_number("integral-time", Ti, positive=True, e=who)
        lim = get("limits")
        try:
            lim = [float(x) for x in lim]
        except (TypeError, ValueError):
            lim = []
        if len(lim) != 2 or not np.all(np.isfinite(lim)) or not 0 < lim[0] < lim[1]:
            raise ValueError("solver-config 'control': 'limits' must be [lo, hi] with 0 < lo < hi%s (got %r)"
                             % ("" if who is None else " (member %d)" % e, get("limits")))
        lo[e], hi[e] = lim
        u0[e] = schedule._own(mi, key)
        if key == "medium-temperature" and u0[e] == 0:
            raise ValueError("solver-config 'control': 'medium-temperature' needs a member with external-heat MeTe > 0 "
                             "(MeTe = 0 is the adiabatic switch); member %d has MeTe = 0" % e)
        T, v = _setpoint(get("setpoint"), who)
        sp[:, e] = [setpoint_at(T, v, t, tol) for t in times]
    if sched is None:          # no "schedule": every member's own values, constant (the forced code object needs its rows)
        values = np.array([[[schedule._own(mi, k)] for k in ORDER] for mi in inputs], dtype=np.float64)
        sched = schedule.Schedule([0.0], values, (False, False, False))
    return Control(times, Kp, Ki, u0, lo, hi, sp, select, species, key, Ts, start), sched
