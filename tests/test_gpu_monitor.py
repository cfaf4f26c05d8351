"""solver-config "monitor" on the device: the row-reduction kernels against numpy on raw tensors (no mechanism), and
rmtExe with a monitor against the unmonitored run whose output times are the monitor's sample times.

A monitored run takes exactly the launches of that unmonitored run, so tNo = 2 with samples = 3 is compared with tNo = 6
bit for bit: outlet values to 1e-14 (the species sum of <= 12 terms is taken in another order, everything else is the
same operations), extremes and positions exactly.  (The periods used here, 0.5 s, 0.02 s and 10 s, are ones where
linspace(t_i, t_i+1, 4) and linspace(0, period, 7) agree to the last bit.)"""
import copy
import os

import numpy as np
import pytest
import torch

import inputs as INP
from rmt_app_amd import hipbind, monitor, plan, rmtExe
from rmt_app_amd.n2 import N2Device

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2), (3, 7, 20), (5, 7, 64), (5, 7, 65), (2, 13, 1027), (1, 7, 4096), (1, 2, 16385), (2048, 7, 20)]
EDITS = 7          # kinds of edited rows below


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)/np.maximum(np.abs(b), 1e-300)))


@pytest.fixture(scope="module")
def mon():
    m = hipbind.Monitor(torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    yield m
    m.close()


def edited(rng, E, V, N, shift, dtype):
    """random normal rows; row r gets edit (r + shift) % EDITS"""
    y = rng.standard_normal((E*V, N)).astype(dtype)
    for r in range(E*V):
        kind = (r + shift) % EDITS
        if kind == 1:
            y[r] = dtype(0.375)                             # constant: argmax must be 0
        elif kind == 2:
            y[r, 0] = 10.0                                  # the maximum at node 0
        elif kind == 3:
            y[r, N - 1] = 10.0                              # ... and at node N-1
        elif kind == 4:
            y[r] = -np.abs(y[r]) - 1.0                      # everything negative
            y[r, N//3] = -50.0
        elif kind == 5:
            y[r, N//2] = np.nan                             # must not win
        elif kind == 6:
            y[r, [N//3, N - 1]] = 9.0                       # a duplicate maximum: the lower index wins
    return y.reshape(E, V, N)


def reduce_on_device(mon, y, dydt=None, offset=0):
    """y, dydt: numpy [E][V][N]; offset: elements the device copy is shifted by (misaligns every row start)"""
    E, V, N = y.shape
    def dev(a):
        flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
        flat[offset:].copy_(torch.from_numpy(a.ravel()))
        return flat, flat[offset:]
    keep_y, ty = dev(y)
    keep_d, td = dev(dydt) if dydt is not None else (None, None)
    out = torch.full((E, V, 5), -7.0, dtype=torch.float64, device="cuda")
    mon.reduce(torch.cuda.current_stream().cuda_stream, ty.data_ptr(), td.data_ptr() if td is not None else 0,
               E, V, N, y.dtype == np.float32, out.data_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize("shape,dtype", [(s, np.float64) for s in SHAPES]
                         + [((3, 7, 20), np.float32), ((2, 13, 1027), np.float32)])
def test_kernel_equals_numpy(mon, shape, dtype):
    E, V, N = shape
    rng = np.random.default_rng(E*1000 + N)
    size = np.dtype(dtype).itemsize
    N_CUS = torch.cuda.get_device_properties(0).multi_processor_count
    passes = max(1, EDITS - E*V + 1)                           # every kind of edited row occurs, also with 1 or 2 rows
    for shift in range(passes):
        y = edited(rng, E, V, N, shift, dtype)
        d = rng.standard_normal(shape).astype(dtype)
        d[0, 0, N//2] = -11.0 if shift % 2 else np.nan       # a NaN derivative never wins either
        for offset, dydt in ((0, None), (0, d), (1, d)):
            got = reduce_on_device(mon, y, dydt, offset)
            want = monitor.reduce_numpy(y, dydt)
            np.testing.assert_array_equal(got, want, err_msg="%s shift %d offset %d" % (shape, shift, offset))
            if dydt is None:
                assert np.all(got[..., 4] == 0.0)
            else:
                np.testing.assert_array_equal(got[..., 4], np.nanmax(np.abs(d.astype(np.float64)), axis=-1))
            # which path ran: one wave per row, or one workgroup per row
            assert mon.last_rows_per_block() == hipbind.monitor_rows_per_block(E, V, N, size, N_CUS)
    kinds = {(r + s) % EDITS for r in range(E*V) for s in range(passes)}
    assert kinds == set(range(EDITS))


def test_both_paths_are_covered():
    N_CUS = torch.cuda.get_device_properties(0).multi_processor_count
    paths = [hipbind.monitor_rows_per_block(E, V, N, 8, N_CUS) for E, V, N in SHAPES]
    assert paths == [4, 4, 4, 4, 1, 1, 1, 4]


# ----------------------------------------------------------------------------- rmtExe
STEPPERS = {
    "hip-rk4": ({"dt": 2.5e-6}, 0.02),
    "hip-rk45": ({"rtol": 1e-8, "atol": 1e-11}, 0.5),
    "hip-ros4": ({}, 0.5),
    "default": ({}, 0.5),
}


def dme(ivp, tNo, mon=None, zNo=20, period=None, **cfg):
    mi = INP.dme_notebook_input(ivp=ivp, period=STEPPERS[ivp][1] if period is None else period)
    mi["solver-config"].update({"zNo": zNo, "tNo": tNo, "quiet": True})
    mi["solver-config"].update(STEPPERS[ivp][0])
    mi["solver-config"].update(cfg)
    if mon is not None:
        mi["solver-config"]["monitor"] = mon
    return mi


def check_against_fine(mon, coarse, fine, model="N2", xs=None, profile=True):
    assert len(coarse) == 2 and len(fine) == 6 and len(mon["time"]) == 7 and mon["time"][0] == 0.0
    assert np.array_equal(mon["time"][1:], [p["dataTime"] for p in fine])
    worst = 0.0
    for k in range(1, 7):
        pk = fine[k - 1]
        worst = max(worst, relerr(mon["outlet"][k], pk["dataYs"][:, -1]))
        T = pk["dataYTemp2"][0] if model == "N2" else pk["dataYTemp"][0]
        pos = pk["dataXs"] if model == "N2" else xs
        assert mon["peak-temperature"][k] == T.max(), k
        assert mon["peak-position"][k] == pos[np.argmax(T)], k
        conc = pk["dataYCons2"] if model == "N2" else pk["dataYCons"]
        assert np.array_equal(mon["state-max"][k, :conc.shape[0]], conc.max(axis=1))
        assert np.array_equal(mon["state-min"][k, :conc.shape[0]], conc.min(axis=1))
        assert np.array_equal(mon["state-argmax"][k, :conc.shape[0]], pos[conc.argmax(axis=1)])
    print("outlet against the fine run: %.3e" % worst)
    assert worst <= 1e-14
    if profile:
        for a, b in zip(coarse, (fine[2], fine[5])):
            assert a["dataTime"] == b["dataTime"]
            for key in a:
                if isinstance(a[key], np.ndarray):
                    assert np.array_equal(a[key], b[key]), key


def cache_files():
    return set(os.listdir(hipbind.CACHE_DIR))


@pytest.mark.parametrize("ivp", list(STEPPERS))
def test_monitored_run_equals_the_fine_unmonitored_run(ivp):
    fine = rmtExe(dme(ivp, 6))["resModel"]
    before = cache_files()
    res = rmtExe(dme(ivp, 2, {"samples": 3}))["resModel"]
    new = cache_files() - before
    assert all(f.startswith("monitor-") for f in new), new       # the same stepper code object, plus the monitor's
    assert any(f.startswith("monitor-") for f in cache_files())
    assert "monitor" not in fine and not any(k.endswith("raw") for k in res["device-stats"])
    check_against_fine(res["monitor"], res["dataPack"], fine["dataPack"])
    m = res["monitor"]
    assert m["labelList"] == res["dataPack"][0]["labelList"]
    assert np.all(m["state-argmax"][0] == 0.0) and np.array_equal(m["state-max"][0], m["state-min"][0])   # flat start


def test_several_workgroup_reactor_zno_600():
    fine = rmtExe(dme("hip-rk4", 6, zNo=600, period=0.002))["resModel"]
    res = rmtExe(dme("hip-rk4", 2, {"samples": 3}, zNo=600, period=0.002))["resModel"]
    check_against_fine(res["monitor"], res["dataPack"], fine["dataPack"])


def test_model_m2_with_the_stiff_stepper():
    def m2(tNo, mon=None):
        mi = INP.m2_dme_input(ivp="hip-ros4", period=10)
        mi["solver-config"].update({"tNo": tNo, "quiet": True})
        if mon is not None:
            mi["solver-config"]["monitor"] = mon
        return mi
    fine = rmtExe(m2(6))["resModel"]
    res = rmtExe(m2(2, {"samples": 3}))["resModel"]
    zNo = fine["dataPack"][0]["dataYs"].shape[1]
    xs = np.linspace(0, m2(2)["reactor"]["ReLe"], zNo)
    check_against_fine(res["monitor"], res["dataPack"], fine["dataPack"], "M2", xs)


@pytest.mark.parametrize("output", ["profile", "outlet"])
def test_sweep_member_by_member(output):
    sweep = {"temperature": list(np.linspace(503.0, 543.0, 8)), "pressure": [3e6, 4e6, 5e6, 6e6]}
    fine = rmtExe(dme("hip-ros4", 6, ensemble=copy.deepcopy(sweep)))["resModel"]["ensemble"]
    res = rmtExe(dme("hip-ros4", 2, {"samples": 3}, ensemble=copy.deepcopy(sweep),
                     **{"ensemble-output": output}))["resModel"]
    ens = res["ensemble"]
    assert len(ens) == len(fine) == 32
    for e in range(32):
        check_against_fine(ens[e]["monitor"], ens[e]["dataPack"], fine[e]["dataPack"], profile=output == "profile")
    assert res["monitor"] is ens[0]["monitor"]
    # physical sanity: a hotter inlet gives a hotter bed (members are ordered temperature-major, 4 pressures each)
    peak = np.array([m["monitor"]["peak-temperature"][-1] for m in ens]).reshape(8, 4)
    assert np.all(np.diff(peak, axis=0) >= 0), peak


def test_residual_equals_the_rhs_and_decays():
    from rmt_app_amd.n2 import ros4_block
    res = rmtExe(dme("hip-ros4", 2, {"samples": 3, "residual": True}))["resModel"]
    m = res["monitor"]
    assert m["residual"].shape == (7, 7) and np.all(np.isfinite(m["residual"]))
    # at the final time: rmt_n2_rhs at the final state, reduced by numpy (the state is recovered from the dataPack's
    # scaled rows, which are the state itself)
    mi = dme("hip-ros4", 2)
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, 20)
    dev = N2Device(mech, row, 20, block=ros4_block(mech.V, 20), npt=1, features=("ros4",))   # the run's code object
    last = res["dataPack"][-1]
    y = np.concatenate((last["dataYCons1"], last["dataYTemp1"].reshape(1, -1)), axis=0)
    f = dev.rhs(dev.to_device(y)).cpu().numpy().reshape(mech.V, 20)
    dev.close()
    assert np.array_equal(m["residual"][-1], np.abs(f).max(axis=1))
    # the bed settles: the residual at the last sample is below that at the first sample after t = 0
    assert m["residual"][-1].max() < m["residual"][1].max()
    print("residual: first %.3e  last %.3e" % (m["residual"][1].max(), m["residual"][-1].max()))


def test_monitor_with_a_schedule():
    sch = {"time": [0.0, 0.2, 0.2, 0.5], "inlet-temperature": [523.0, 523.0, 533.0, 533.0]}
    t = [0.1, 0.2, 0.25, 0.3, 0.5]
    plainrun = rmtExe(dme("hip-rk45", 2, schedule=copy.deepcopy(sch)))["resModel"]
    res = rmtExe(dme("hip-rk45", 2, {"times": t}, schedule=copy.deepcopy(sch)))["resModel"]
    # launches end at 0.1 | 0.2 (breakpoint and sample, one mark) | 0.25 (output and sample) | 0.3 | 0.5
    assert res["device-stats"]["launches"] == 5 and plainrun["device-stats"]["launches"] == 3
    m = res["monitor"]
    assert np.array_equal(m["time"], [0.0] + t)
    for key in ("time", "inlet-temperature", "inlet-pressure", "medium-temperature"):
        assert np.array_equal(res["schedule"][key], plainrun["schedule"][key])
    for k, pk in ((3, res["dataPack"][0]), (5, res["dataPack"][1])):
        assert m["time"][k] == pk["dataTime"]
        assert relerr(m["outlet"][k], pk["dataYs"][:, -1]) <= 1e-14
        assert m["peak-temperature"][k] == pk["dataYTemp2"].max()
    # splitting the integration at the extra sample times moves the adaptive run within its tolerance only
    for a, b in zip(res["dataPack"], plainrun["dataPack"]):
        assert np.max(np.abs(a["dataYs"][:6] - b["dataYs"][:6])) <= 2e-6
        assert np.max(np.abs(a["dataYs"][6] - b["dataYs"][6])/b["dataYs"][6]) <= 2e-6


def test_rate_domain_error_still_raises_and_returns_no_monitor():
    """The inlet pressure stepped down to 100 Pa (test_gpu_schedule.py): sqrt(KH2 PH2) has no real value inside the bed -
    ValueError('math domain error') with a monitor as without, and no result."""
    mi = dme("hip-rk4", 2, {"samples": 3}, period=0.002,
             schedule={"time": [0.0, 0.001, 0.001, 0.002], "inlet-pressure": [5e6, 5e6, 100.0, 100.0]})
    with pytest.raises(ValueError, match="math domain error"):
        rmtExe(mi)
