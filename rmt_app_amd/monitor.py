"""Time series between the output times of the dynamic models N2 and M2 (solver-config "monitor").

    "monitor": {"samples": 20,        # per output interval, int >= 1      (either this ...)
                "times": [..],        # explicit, strictly increasing, in (0, period]   (... or this, not both)
                "residual": False}    # also record max|dy/dt| per variable

* t = 0, the initial state, is always sample 0.
* "samples": m - every output interval [t_i, t_i+1] contributes linspace(t_i, t_i+1, m + 1)[1:], so every output time
  is a sample and there are K = 1 + tNo*m of them.  "times": the samples are exactly {0} and the given times.
* A sample time within schedule.MERGE_TOL * period of an output time or of a schedule breakpoint IS that time.
* The integration is split at the sample times the way "schedule" splits it at its breakpoints: the launch list is the
  sorted union of output times, breakpoints and sample times (launches.merge).  Only launches that end at an output
  time are packed, only launches that end at a sample time are monitored.  A monitored run takes exactly the launches of an
  unmonitored run whose output times are that union - and computes the same states bit for bit.
* At a sample the state stays where it is: a reduction kernel (csrc/monitor_kernels.inc) writes, per member and
  variable, {outlet value, max, argmax, min, max|dy/dt|} into slice k of ONE device buffer [K][E][V][5], which is
  copied to the host once, at the end of the run.

Host side only (numpy): parsing and validation, the sample times and the conversion of the
raw numbers to the result entry resModel["monitor"].
"""
import numpy as np

from .schedule import MERGE_TOL

KEYS = ("samples", "times", "residual")
MODELS = ("N2", "M2")
SLOTS = 5              # doubles per (member, variable): last, max, argmax, min, max|dydt|
LAST, MAX, ARGMAX, MIN, RESIDUAL = range(SLOTS)


def check_model(modelInput):
    """ValueError when the input asks for a monitor on a model that has none (rmtExe, before any device work)."""
    if (modelInput.get('solver-config') or {}).get('monitor') is not None and modelInput.get('model') not in MODELS:
        raise ValueError("solver-config 'monitor' (time series between the output times) is only available for the "
                         "models 'N2' and 'M2' (got model %r)" % (modelInput.get('model'),))


def sample_times(spec, period, tNo):
    """[K] sample times of a validated spec, t = 0 first; samples that coincide with an output time carry that output
    time's value."""
    out = np.linspace(0.0, float(period), int(tNo) + 1)
    if 'samples' in spec:
        m = int(spec['samples'])
        parts = [np.linspace(out[i], out[i + 1], m + 1)[1:] for i in range(int(tNo))]
        return np.concatenate([[0.0]] + parts)
    times = np.array(spec['times'], dtype=np.float64)
    tol = MERGE_TOL*float(period)
    for j, t in enumerate(times):
        k = int(np.argmin(np.abs(out - t)))
        if abs(out[k] - t) <= tol:
            times[j] = out[k]
    return np.concatenate([[0.0], times])


class Monitor:
    """A parsed monitor spec: ``times`` [K] (sample 0 = the initial state at t = 0), ``residual``."""

    def __init__(self, times, residual=False, given="samples"):
        self.times = np.asarray(times, dtype=np.float64)
        self.residual = bool(residual)
        self.given = given
        self.K = len(self.times)

    def check_budget(self, E, V, cap):
        """The device buffer [K][E][V][5] doubles must not exceed ``cap`` bytes (n2.PIPELINE_BYTES)."""
        need = self.K*int(E)*int(V)*SLOTS*8
        if need > cap:
            raise ValueError("solver-config 'monitor': %r asks for %d samples of %d members x %d variables = %d bytes "
                             "of monitor buffer, more than the %d allowed - lower 'samples'"
                             % ("samples" if self.given == "samples" else "times", self.K, E, V, need, cap))


def parse(modelInput, tNo, has_schedule=None):
    """The Monitor of a run (None when the input has no "monitor"), or ValueError naming the offending key."""
    cfg = modelInput['solver-config']
    spec = cfg.get('monitor')
    if spec is None:
        return None
    check_model(modelInput)
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'monitor' must be a dict with the keys %s" % (KEYS,))
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'monitor': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    if ('samples' in spec) == ('times' in spec):
        raise ValueError("solver-config 'monitor' needs either 'samples' (per output interval) or 'times' (explicit), "
                         "not %s" % ("both" if 'samples' in spec else "neither"))
    residual = spec.get('residual', False)
    if not isinstance(residual, (bool, np.bool_)):
        raise ValueError("solver-config 'monitor': 'residual' must be True or False (got %r)" % (residual,))
    if has_schedule is None:
        has_schedule = cfg.get('schedule') is not None
    if residual and has_schedule:
        raise ValueError("solver-config 'monitor': 'residual' cannot be combined with 'schedule' - the residual is "
                         "rmt_n2_rhs at the sample state, which does not evaluate the forcing")
    period = float(modelInput['operating-conditions']['period'])
    if 'samples' in spec:
        m = spec['samples']
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 1:
            raise ValueError("solver-config 'monitor': 'samples' must be an integer >= 1 (got %r)" % (m,))
    else:
        try:
            times = np.array(spec['times'], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("solver-config 'monitor': 'times' must be a list of numbers")
        if times.ndim != 1 or len(times) < 1 or not np.all(np.isfinite(times)):
            raise ValueError("solver-config 'monitor': 'times' must be a non-empty list of finite numbers")
        if np.any(np.diff(times) <= 0):
            raise ValueError("solver-config 'monitor': 'times' must be strictly increasing")
        if times[0] <= 0 or times[-1] > period*(1 + MERGE_TOL):
            raise ValueError("solver-config 'monitor': 'times' must lie in (0, period] (period = %g s, got %g .. %g)"
                             % (period, float(times[0]), float(times[-1])))
    return Monitor(sample_times(spec, period, tNo), residual, "samples" if 'samples' in spec else "times")


def result_entry(raw, times, mech, zNo, named=None, model="N2", length=1.0, residual=False):
    """resModel["monitor"] of ONE member from its raw numbers [K][V][5].

    Units are those of the dataPack entries: model N2 - ``named`` are the member's scaling constants, the outlet is
    the arithmetic of n2.pack_interval on the last column (mole fractions, T in K), concentrations as in dataYCons2,
    temperature as in dataYTemp2, positions as in dataXs; model M2 - the state is dimensional already
    (m2.pack_interval), positions are linspace(0, ``length``, zNo) as in m2.result_lists."""
    raw = np.asarray(raw, dtype=np.float64).reshape(len(times), mech.V, SLOTS)
    S, V = mech.S, mech.V
    thermal = (model == "M2") or not mech.iso

    def units(a):               # [K][V] state values -> result units (monotone per row: extremes stay extremes)
        if model == "M2":
            return a.copy()
        out = a*named["Cmax"]
        if thermal:
            out[:, -1] = a[:, -1]*named["Tf"] + named["Tf"]
        return out
    last = raw[:, :, LAST]
    if model == "M2":
        conc = last[:, :S]
        T = last[:, S:S + 1]
    else:
        conc = (last[:, :-1] if thermal else last)*named["Cmax"]
        T = last[:, -1:]*named["Tf"] + named["Tf"] if thermal else np.zeros((len(times), 1))*named["Tf"] + named["Tf"]
    outlet = np.concatenate((conc/np.sum(conc, axis=1, keepdims=True), T), axis=1)
    xs = np.linspace(0, 1, zNo) if model != "M2" else np.linspace(0, length, zNo)
    idx = raw[:, :, ARGMAX].astype(np.int64)
    res = {
        "time": np.array(times, dtype=np.float64),
        "labelList": list(mech.compList) + ["Temperature"],
        "outlet": outlet,
        "state-max": units(raw[:, :, MAX]),
        "state-min": units(raw[:, :, MIN]),
        "state-argmax": xs[idx],
    }
    if thermal:
        res["peak-temperature"] = res["state-max"][:, V - 1].copy()
        res["peak-position"] = res["state-argmax"][:, V - 1].copy()
    if residual:
        res["residual"] = raw[:, :, RESIDUAL].copy()
    return res


def reduce_numpy(y, dydt=None):
    """What the device kernel computes, in numpy (y: [E][V][N]): the reference of the tests and the monitor of
    host-emulated devices.  [E][V][5]."""
    y = np.asarray(y, dtype=np.float64)
    out = np.zeros(y.shape[:2] + (SLOTS,))
    ok = ~np.isnan(y)
    hi = np.where(ok, y, -np.inf)
    out[..., LAST] = y[..., -1]
    out[..., MAX] = hi.max(axis=-1)
    out[..., ARGMAX] = hi.argmax(axis=-1)
    out[..., MIN] = np.where(ok, y, np.inf).min(axis=-1)
    if dydt is not None:
        d = np.abs(np.asarray(dydt, dtype=np.float64))
        out[..., RESIDUAL] = np.where(np.isnan(d), 0.0, d).max(axis=-1)
    return out
