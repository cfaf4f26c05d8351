"""launches.merge against the launch lists that three chained passes - one of the schedule, one of the monitor over its
output, one of the controller over the monitor's - computed before it existed (recorded at the parent commit in
tests/golden/g16_launch_lists.json): every field of every launch and both snapped time arrays are equal exactly."""
import json
import os

import numpy as np
import pytest

from rmt_app_amd import launches, schedule

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g16_launch_lists.json")


@pytest.fixture(scope="module")
def cases():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert 300 <= len(doc["cases"]) <= 400 and doc["seed"] and len(doc["parent"]) == 40
    return doc["cases"]


def test_merge_tol_has_one_home():
    assert schedule.MERGE_TOL is launches.MERGE_TOL and launches.MERGE_TOL == 1e-12


def test_merge_equals_the_recorded_lists_exactly(cases):
    for n, c in enumerate(cases):
        args = [None if c[k] is None else list(c[k]) for k in ("breakpoints", "samples", "controls")]
        L, st, ct = launches.merge(c["period"], c["tNo"], () if args[0] is None else args[0], args[1], args[2])
        assert all(type(l.t0) is float and type(l.t1) is float for l in L), n
        assert [(l.t0, l.t1, l.out, l.sample, l.control) for l in L] == [tuple(l) for l in c["launches"]], n
        for got, want in ((st, c["sample_times"]), (ct, c["control_times"])):
            assert (got is None) == (want is None), n
            assert got is None or (got.dtype == np.float64 and got.tolist() == want), n
        # the arguments are left alone
        assert args == [c[k] for k in ("breakpoints", "samples", "controls")], n


def test_merge_copies_arrays_it_is_given():
    samples, controls = np.array([0.0, 0.25*(1 + 3e-13), 0.5]), np.array([0.25*(1 - 3e-13)])
    keep = samples.copy(), controls.copy()
    _, st, ct = launches.merge(0.5, 2, (), samples, controls)
    assert np.array_equal(samples, keep[0]) and np.array_equal(controls, keep[1])
    assert st[1] == 0.25 and ct[0] == 0.25 and st is not samples and ct is not controls


def test_the_fixture_covers_every_kind_of_merge(cases):
    """The recorded cases must keep exercising the rule: at least 5 of each kind."""
    n = dict.fromkeys(("monitor time snapped", "control time snapped", "control sample on a monitor-only mark",
                       "control sample at t = 0", "all three layers", "breakpoint dropped on an output time"), 0)
    for c in cases:
        tol = launches.MERGE_TOL*c["period"]
        out = np.linspace(0.0, c["period"], c["tNo"] + 1)
        L = [launches.Launch(*l) for l in c["launches"]]
        kept = set(c["breakpoints"] or ())
        n["monitor time snapped"] += c["samples"] is not None and c["samples"] != c["sample_times"]
        n["control time snapped"] += c["controls"] is not None and c["controls"] != c["control_times"]
        n["control sample on a monitor-only mark"] += any(
            b.control is not None and a.sample is not None and a.out is None and b.t0 not in kept
            for a, b in zip(L[:-1], L[1:]))
        n["control sample at t = 0"] += L[0].control is not None
        n["all three layers"] += all(c[k] is not None for k in ("breakpoints", "samples", "controls"))
        n["breakpoint dropped on an output time"] += any(
            tol < b < c["period"] - tol and np.min(np.abs(out - b)) <= tol for b in (c["breakpoints"] or ()))
    assert all(v >= 5 for v in n.values()), n
