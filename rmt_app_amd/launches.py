"""The launch list of a dynamic run: where the integration over [0, period] is split (numpy only).

A run is split at its output times, at the breakpoints of "schedule", at the samples of "monitor" and at the samples of
"control".  The marks are merged in that order, in layers, and every layer sees the marks of the ones before it: a time
within MERGE_TOL * period of an existing mark IS that mark (it takes the mark's value, bit for bit), any other time adds a
mark.  This is the one place that rule is written.
"""
from collections import namedtuple

import numpy as np

MERGE_TOL = 1e-12     # relative to the period

# t0, t1 [s]; ``out``: index of the output time the launch ends at, ``sample``: index of the monitor sample it ends at,
# ``control``: index of the control sample taken at its start - each None where there is none
Launch = namedtuple("Launch", "t0 t1 out sample control")
_T, _OUT, _SAMPLE, _CONTROL = range(4)          # a mark: [time, out, sample, control]


def merge(period, tNo, breakpoints=(), samples=None, controls=None):
    """(launches, sample_times, control_times) of a run with the output times linspace(0, period, tNo + 1): the list of
    Launch that covers [0, period], and ``samples`` / ``controls`` with every time that fell on a mark replaced by that
    mark's value (copies; None where None was passed).
    A breakpoint becomes a mark only strictly inside (0, period) and away from every output time: breakpoints add no
    entries to the result, so one that coincides with an output time is that output time."""
    period = float(period)
    tol = MERGE_TOL*period
    out = np.linspace(0.0, period, int(tNo) + 1)
    marks = [[float(t), k, None, None] for k, t in enumerate(out)]
    for b in np.unique(np.asarray(breakpoints, dtype=np.float64)):
        if tol < b < period - tol and np.min(np.abs(out - b)) > tol:
            marks.append([float(b), None, None, None])
    marks.sort(key=lambda m: m[_T])

    def layer(times, slot):
        if times is None:
            return None
        times = np.array(times, dtype=np.float64)
        at = np.array([m[_T] for m in marks])
        extra = []
        for k, t in enumerate(times):
            j = int(np.argmin(np.abs(at - t)))
            if abs(at[j] - t) <= tol:
                marks[j][slot] = k
                times[k] = at[j]
            else:
                extra.append([float(t), None, None, None])
                extra[-1][slot] = k
        marks[:] = sorted(marks + extra, key=lambda m: m[_T])
        return times
    sample_times = layer(samples, _SAMPLE)
    control_times = layer(controls, _CONTROL)
    return ([Launch(a[_T], b[_T], b[_OUT], b[_SAMPLE], a[_CONTROL]) for a, b in zip(marks[:-1], marks[1:])],
            sample_times, control_times)
