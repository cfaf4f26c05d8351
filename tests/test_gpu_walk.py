"""The walk over the launches of a run (n2.integrate_intervals) queues them in batches bounded by n2.PIPELINE_BYTES of
pinned memory.  The batch length is host bookkeeping only: it must not change a bit of the result."""
import numpy as np
import pytest

import inputs as INP
from rmt_app_amd import n2, rmtExe

pytestmark = pytest.mark.gpu

ZNO = 20
MEMBERS = [{"operating-conditions": {"temperature": 523.0}}, {"operating-conditions": {"temperature": 531.0}}]
# (id, solver-config beyond the common keys, period, launches the walk makes)
CASES = [
    ("rk45", {"ivp": "hip-rk45", "tNo": 5}, 0.05, 5),
    # breakpoints strictly inside the first and the second output interval: the launch list differs from the output
    # list, and the rows of the forced code object are refreshed between queued launches
    ("ros4-schedule", {"ivp": "hip-ros4", "tNo": 3,
                       "schedule": {"time": [0.0, 0.005, 0.015, 0.03], "inlet-temperature": [0.0, 0.0, 6.0, 6.0],
                                    "relative": True}}, 0.03, 5),
    # every field of a launch in use: output times 0.02 and 0.04, a jump of the coolant at 0.0205, monitor samples at 0.005
    # and 0.012, control samples 0.01, 0.012, .. 0.038 - 15 of them, one on an output time (0.02), one on a monitor sample
    # (0.012), and one launch behind the breakpoint that only rewrites the held value: 18 launches
    ("rk4-schedule-monitor-control",
     {"ivp": "hip-rk4", "dt": 2e-5, "tNo": 2,
      "schedule": {"time": [0, 0.0205, 0.0205, 0.04], "medium-temperature": [523, 523, 533, 533]},
      "monitor": {"times": [0.005, 0.012]},
      "control": {"measured": "outlet-temperature", "manipulated": "inlet-pressure", "sample-time": 0.002, "start": 0.01,
                  "setpoint": 530, "gain": 5e4, "integral-time": 0.005, "limits": [4.9e6, 6.0e6]}}, 0.04, 18),
]


def run(cfg, period):
    mi = INP.dme_notebook_input(ivp=cfg["ivp"], period=period)
    mi["solver-config"].update({"zNo": ZNO, "quiet": True, "ensemble": [dict(m) for m in MEMBERS]})
    mi["solver-config"].update(cfg)
    return rmtExe(mi)["resModel"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def same_entry(a, b):
    """two result entries (dicts of arrays, lists and numbers) are equal bit for bit"""
    return a.keys() == b.keys() and all(
        np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_batch_length_does_not_change_the_result(case, monkeypatch):
    """Batches of one launch, of two (the last batch is short where the launches are five) and the default (one batch)."""
    _, cfg, period, n_launches = case
    per_launch = len(MEMBERS)*7*ZNO*8              # bytes of pinned memory one staged end state takes (V = 7, fp64)
    results = {}
    for batch in (1, 2, None):
        if batch is not None:
            monkeypatch.setattr(n2, "PIPELINE_BYTES", batch*per_launch)
        else:
            monkeypatch.undo()
            assert n2.PIPELINE_BYTES >= n_launches*per_launch
        results[batch] = run(cfg, period)
    ref = results[None]
    assert len(ref["ensemble"]) == len(MEMBERS) and len(ref["dataPack"]) == cfg["tNo"]
    assert ref["device-stats"].get("launches", cfg["tNo"]) == n_launches
    for batch in (1, 2):
        got = results[batch]
        for a, b in zip([ref] + ref["ensemble"], [got] + got["ensemble"]):
            assert len(a["dataPack"]) == len(b["dataPack"]) == cfg["tNo"]
            for pa, pb in zip(a["dataPack"], b["dataPack"]):
                assert pa["dataTime"] == pb["dataTime"]
                arrays = [k for k in pa if isinstance(pa[k], np.ndarray)]
                assert len(arrays) >= 5
                for k in arrays:
                    assert np.array_equal(pa[k], pb[k]), (batch, k)
            for entry in ("monitor", "control"):           # the one-off device buffers: the same samples in the same slices
                assert (entry in a) == (entry in b) == (entry in cfg), (batch, entry)
                if entry in cfg:
                    assert len(a[entry]["time"]) > 1 and same_entry(a[entry], b[entry]), (batch, entry)
        sa, sb = ref["device-stats"], got["device-stats"]
        assert sa["steps"] == sb["steps"] and sa.get("launches") == sb.get("launches")
        assert np.array_equal(sa["accepted"], sb["accepted"]) and np.array_equal(sa["rejected"], sb["rejected"])
