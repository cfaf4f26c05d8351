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
]


def run(cfg, period):
    mi = INP.dme_notebook_input(ivp=cfg["ivp"], period=period)
    mi["solver-config"].update({"zNo": ZNO, "quiet": True, "ensemble": [dict(m) for m in MEMBERS]})
    mi["solver-config"].update(cfg)
    return rmtExe(mi)["resModel"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_batch_length_does_not_change_the_result(case, monkeypatch):
    """Batches of one launch, of two (the last batch is short: five launches) and the default (one batch)."""
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
        sa, sb = ref["device-stats"], got["device-stats"]
        assert sa["steps"] == sb["steps"] and sa.get("launches") == sb.get("launches")
        assert np.array_equal(sa["accepted"], sb["accepted"]) and np.array_equal(sa["rejected"], sb["rejected"])
