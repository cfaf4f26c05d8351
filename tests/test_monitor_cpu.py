"""solver-config "monitor" without a GPU: validation, sample times and refined launch lists, the conversion of the raw
numbers against pack_interval, cross-compilation of the monitor kernels, and the host path end to end on the host
emulation of the generated source (tests/emu_device.py) with a numpy monitor.

The end-to-end tests rest on one equivalence: a monitored run takes the launches of an unmonitored run whose output
times are the union of output and sample times - so tNo = 2 with samples = 3 computes, bit for bit, the states of
tNo = 6 at the same times."""
import copy
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import emu_device
import inputs as INP
from rmt_app_amd import hipbind, isa, launches, monitor, plan, rmtExe, schedule
from rmt_app_amd import m2 as M2
from rmt_app_amd import n2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)/np.maximum(np.abs(b), 1e-300)))


# ----------------------------------------------------------------------------- validation
def _input(model="N2", **mon):
    mi = INP.dme_notebook_input(ivp="hip-rk4", period=0.5) if model != "M2" else INP.m2_dme_input(ivp="hip-rk4", period=0.5)
    mi["model"] = model
    mi["solver-config"].update({"quiet": True, "zNo": 20, "tNo": 2, "display-result": "False"})
    if mon:
        mi["solver-config"]["monitor"] = mon.pop("spec", mon)
    return mi


BAD = [
    ({"samples": 3, "every": 2}, "every"),                       # unknown key
    ({"samples": 3, "times": [0.1]}, "both"),                    # both
    ({"residual": True}, "neither"),                             # neither
    ({"samples": 2.5}, "samples"),
    ({"samples": "3"}, "samples"),
    ({"samples": 0}, "samples"),
    ({"samples": -1}, "samples"),
    ({"samples": True}, "samples"),
    ({"times": [0.2, 0.1]}, "times"),                            # not increasing
    ({"times": [0.1, 0.1]}, "times"),
    ({"times": [0.0, 0.1]}, "times"),                            # 0 is outside (0, period]
    ({"times": [0.1, 0.6]}, "times"),                            # beyond the period
    ({"times": []}, "times"),
    ({"samples": 3, "residual": 1}, "residual"),
]


@pytest.mark.parametrize("spec,word", BAD)
def test_bad_specs_raise_valueerror_naming_the_key(spec, word, capsys):
    mi = _input(spec=spec)
    with pytest.raises(ValueError, match="monitor") as e:
        monitor.parse(mi, 2)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="monitor") as e:       # ... and through rmtExe, before any device work
        rmtExe(mi)                                               # (there is no device here: anything later raises RmtN2Error)
    assert word in str(e.value)
    capsys.readouterr()


def test_residual_with_schedule_other_models_and_the_buffer_cap(capsys):
    mi = _input(samples=3, residual=True)
    mi["solver-config"]["schedule"] = {"time": [0.0, 0.5], "inlet-temperature": [523.0, 533.0]}
    for run in (lambda: monitor.parse(mi, 2), lambda: rmtExe(mi)):
        with pytest.raises(ValueError, match="'residual' cannot be combined with 'schedule'"):
            run()
    for model in ("N1", "M7", "M1", "M9"):
        bad = _input(model, samples=3)
        for run in (lambda: monitor.parse(bad, 2), lambda: rmtExe(bad)):
            with pytest.raises(ValueError, match="'monitor'.*only available for the models 'N2' and 'M2'"):
                run()
    # K*E*V*5*8 bytes against PIPELINE_BYTES: 2048 members x 7 variables hold 1872 samples, not more
    ok = monitor.parse(_input(samples=935), 2)
    ok.check_budget(2048, 7, n2.PIPELINE_BYTES)
    assert ok.K*2048*7*5*8 <= n2.PIPELINE_BYTES
    with pytest.raises(ValueError, match="'samples'"):
        monitor.parse(_input(samples=936), 2).check_budget(2048, 7, n2.PIPELINE_BYTES)
    big = _input(samples=2_000_000)
    with pytest.raises(ValueError, match="'samples'"):           # through rmtExe, one member
        rmtExe(big)
    assert monitor.parse(_input(), 2) is None                     # without the key: nothing
    capsys.readouterr()


# ----------------------------------------------------------------------------- sample times, launch lists
def plain(period, tNo):
    out = np.linspace(0, period, tNo + 1)
    return [(float(out[i]), float(out[i + 1]), i + 1) for i in range(tNo)]


def test_samples_per_interval():
    mon = monitor.parse(_input(samples=3), 2)
    out = np.linspace(0, 0.5, 3)
    want = np.concatenate([[0.0], np.linspace(out[0], out[1], 4)[1:], np.linspace(out[1], out[2], 4)[1:]])
    assert mon.K == 7 and np.array_equal(mon.times, want)
    assert mon.times[3] == out[1] and mon.times[6] == out[2]     # every output time is a sample
    L, times, _ = launches.merge(0.5, 2, (), mon.times)
    assert [(l.out, l.sample) for l in L] == [(None, 1), (None, 2), (1, 3), (None, 4), (None, 5), (2, 6)]
    assert [l.t0 for l in L] == list(mon.times[:-1]) and [l.t1 for l in L] == list(mon.times[1:])
    assert np.array_equal(times, mon.times) and all(l.control is None for l in L)
    # the launches ARE those of an unmonitored run with six output times
    assert [(l.t0, l.t1) for l in L] == [(a, b) for a, b, _ in plain(0.5, 6)]
    assert [l[:3] for l in launches.merge(0.5, 6)[0]] == plain(0.5, 6)


def test_explicit_times_one_on_an_output_time():
    mon = monitor.parse(_input(times=[0.1, 0.25*(1 + 1e-14), 0.4]), 2)
    assert np.array_equal(mon.times, [0.0, 0.1, 0.25, 0.4])     # the near-output sample IS the output time
    L = launches.merge(0.5, 2, (), mon.times)[0]
    assert [l[:4] for l in L] == [(0.0, 0.1, None, 1), (0.1, 0.25, 1, 2), (0.25, 0.4, None, 3), (0.4, 0.5, 2, None)]
    # the period itself may be a sample
    mon = monitor.parse(_input(times=[0.5]), 2)
    assert [l[:4] for l in launches.merge(0.5, 2, (), mon.times)[0]] == [(0.0, 0.25, 1, None), (0.25, 0.5, 2, 1)]


def test_breakpoints_samples_and_outputs_merge_without_duplicates():
    mi = _input(times=[0.1, 0.2*(1 - 1e-13), 0.25, 0.3])
    mi["solver-config"]["schedule"] = {"time": [0.0, 0.2, 0.2, 0.35, 0.5], "inlet-temperature": [523, 523, 533, 533, 533]}
    sched = schedule.parse(mi, None, "hip-rk45")
    base = launches.merge(0.5, 2, sched.times)[0]
    assert [l[:3] for l in base] == [(0.0, 0.2, None), (0.2, 0.25, 1), (0.25, 0.35, None), (0.35, 0.5, 2)]
    mon = monitor.parse(mi, 2)
    given = mon.times.copy()
    L, times, _ = launches.merge(0.5, 2, sched.times, mon.times)
    assert [l[:4] for l in L] == [(0.0, 0.1, None, 1), (0.1, 0.2, None, 2), (0.2, 0.25, 1, 3), (0.25, 0.3, None, 4),
                                  (0.3, 0.35, None, None), (0.35, 0.5, 2, None)]
    assert times[2] == 0.2 and given[2] != 0.2                   # the sample at the jump IS the breakpoint
    assert np.array_equal(mon.times, given)                      # (in the returned copy: the argument is left alone)
    ends = [l.t1 for l in L]
    assert len(set(ends)) == len(ends) and all(l.t1 > l.t0 for l in L)


# ----------------------------------------------------------------------------- conversion
def raw_of(Y):
    """numpy {last, max, argmax, min} of a (V, N) state as the kernel lays them out"""
    return monitor.reduce_numpy(Y[None])[0]


@pytest.mark.parametrize("process_type", ["non-iso-thermal", "iso-thermal"])
def test_conversion_equals_pack_interval(process_type):
    mi = INP.dme_notebook_input(process_type=process_type)
    zNo = 37
    mech = plan.Mechanism(mi)
    named, _ = plan.member_constants(mi, mech, zNo)
    rng = np.random.default_rng(7)
    Y = rng.uniform(0.05, 1.0, (mech.V, zNo))
    if not mech.iso:
        Y[-1] = rng.normal(0.0, 0.02, zNo)                      # scaled temperature around 0
    pk = n2.pack_interval(Y, named, mech, zNo, 0.25, "N2")
    m = monitor.result_entry(raw_of(Y)[None], [0.25], mech, zNo, named, "N2")
    assert m["labelList"] == pk["labelList"] and m["outlet"].shape == (1, mech.S + 1)
    # the rounding of a species sum of <= 12 terms taken in another order; everything else is the same operations
    assert relerr(m["outlet"][0], pk["dataYs"][:, -1]) <= 1e-14
    nC = pk["dataYCons2"].shape[0]
    assert np.array_equal(m["state-max"][0, :nC], pk["dataYCons2"].max(axis=1))
    assert np.array_equal(m["state-min"][0, :nC], pk["dataYCons2"].min(axis=1))
    assert np.array_equal(m["state-argmax"][0, :nC], pk["dataXs"][pk["dataYCons2"].argmax(axis=1)])
    if mech.iso:
        assert "peak-temperature" not in m and "peak-position" not in m and m["state-max"].shape == (1, mech.S)
    else:
        assert m["peak-temperature"][0] == pk["dataYTemp2"].max() == m["state-max"][0, -1]
        assert m["state-min"][0, -1] == pk["dataYTemp2"].min()
        assert m["peak-position"][0] == pk["dataXs"][np.argmax(pk["dataYTemp2"][0])]
    assert "residual" not in m


def test_conversion_equals_m2_pack_interval():
    mi = INP.m2_dme_input()
    zNo = 29
    mech = plan.Mechanism(mi)
    rng = np.random.default_rng(11)
    Y = rng.uniform(0.5, 40.0, (mech.V, zNo))
    Y[-1] = rng.uniform(500.0, 560.0, zNo)
    pk = M2.pack_interval(Y.ravel(), mech, zNo, 1.0)
    ReLe = mi["reactor"]["ReLe"]
    raw = raw_of(Y)
    raw[:, monitor.RESIDUAL] = np.arange(mech.V)
    m = monitor.result_entry(raw[None], [1.0], mech, zNo, None, "M2", ReLe, residual=True)
    assert relerr(m["outlet"][0], pk["dataYs"][:, -1]) <= 1e-14
    assert np.array_equal(m["state-max"][0, :mech.S], pk["dataYCons"].max(axis=1))
    assert m["peak-temperature"][0] == pk["dataYTemp"].max()
    assert m["peak-position"][0] == np.linspace(0, ReLe, zNo)[np.argmax(pk["dataYTemp"][0])]
    assert np.array_equal(m["residual"][0], np.arange(mech.V))


# ----------------------------------------------------------------------------- compilation, exports
def test_monitor_kernels_cross_compile_without_scratch():
    src = hipbind.monitor_source()
    assert src == open(os.path.join(ROOT, "rmt_app_amd", "csrc", "monitor_kernels.inc")).read()
    blob = hipbind.monitor_code("gfx950")
    assert blob[:4] == b"\x7fELF"
    assert any(f.startswith("monitor-") and f.endswith("-gfx950.hsaco") for f in os.listdir(hipbind.CACHE_DIR))
    for k in ("rmt_n2_monitor_rows_f64", "rmt_n2_monitor_rows_f32"):
        res = isa.kernel_resources(blob, k)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (k, res)
        mix = isa.kernel_stats(blob, k)["whole"]
        assert mix["scratch"] == 0 and mix["vmem"] > 0
    L = ctypes.CDLL(hipbind.LIB_PATH)
    for name in ("rmt_n2_monitor_source", "rmt_n2_monitor_create", "rmt_n2_monitor_destroy", "rmt_n2_monitor_reduce",
                 "rmt_n2_monitor_last_rows_per_block"):
        assert hasattr(L, name), name
    assert hipbind.lib().rmt_n2_abi_version() == 2
    # the stepper template is not touched by the monitor: it is a translation unit of its own
    assert "rmt_n2_monitor_rows" not in hipbind.kernel_template()
    # the layout rule (csrc/rmt_n2.cpp): short rows and machine-filling row counts by a wave, a few long rows by a workgroup
    rpb = hipbind.monitor_rows_per_block
    assert rpb(2048, 7, 20, 8, 256) == 4 and rpb(3, 7, 1024, 8, 256) == 4 and rpb(256, 7, 4096, 8, 256) == 4
    assert rpb(64, 7, 4096, 8, 256) == 1 and rpb(1, 7, 16384, 8, 256) == 1 and rpb(2, 13, 1027, 4, 256) == 4


def test_monitor_create_reports_errors_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hipbind.RmtN2Error):
        hipbind.Monitor("gfx950")


def test_reduce_numpy_semantics():
    y = np.array([[[1.0, 1.0, 1.0], [np.nan, 2.0, 2.0], [-3.0, -1.0, -2.0]]])
    r = monitor.reduce_numpy(y, -y)
    assert r[0, 0].tolist() == [1.0, 1.0, 0.0, 1.0, 1.0]          # flat: argmax 0
    assert r[0, 1].tolist() == [2.0, 2.0, 1.0, 2.0, 2.0]          # NaN never wins; the lower of two equal maxima
    assert r[0, 2].tolist() == [-2.0, -1.0, 1.0, -3.0, 3.0]


# ----------------------------------------------------------------------------- host path on the emulated device
MONITOR_CALLS = []


class MonEmu(emu_device.EmuDevice):
    """The host-emulation stand-in with a numpy monitor."""

    def monitor(self, y, out, residual=False):
        assert not residual
        MONITOR_CALLS.append(tuple(out.shape))
        Y = y.numpy().reshape(self.E, self.mech.V, self.N)
        out.copy_(torch.from_numpy(monitor.reduce_numpy(Y)))


def _emu_input(model, tNo, mon=None, ensemble=None):
    if model == "N2":
        mi = INP.dme_notebook_input(ivp="hip-rk4", period=2e-4)
    else:
        mi = INP.m2_dme_input(ivp="hip-rk4", period=2e-4)
    mi["solver-config"].update({"quiet": True, "dt": 2e-6, "zNo": 48, "tNo": tNo, "display-result": "False"})
    if mon is not None:
        mi["solver-config"]["monitor"] = mon
    if ensemble is not None:
        mi["solver-config"]["ensemble"] = copy.deepcopy(ensemble)
    return mi


def _emu_run(mi):
    real, n2.N2Device = n2.N2Device, MonEmu
    try:
        return rmtExe(mi)["resModel"]
    finally:
        n2.N2Device = real


def check_against_fine(mon, coarse, fine, model="N2", xs=None):
    """mon / coarse: monitor and dataPack of the run with tNo = 2, samples = 3; fine: dataPack of the run with tNo = 6."""
    assert len(coarse) == 2 and len(fine) == 6 and len(mon["time"]) == 7
    assert mon["time"][0] == 0.0
    assert np.array_equal(mon["time"][1:], [p["dataTime"] for p in fine])
    for k in range(1, 7):
        pk = fine[k - 1]
        assert relerr(mon["outlet"][k], pk["dataYs"][:, -1]) <= 1e-14, k
        T = pk["dataYTemp2"][0] if model == "N2" else pk["dataYTemp"][0]
        pos = pk["dataXs"] if model == "N2" else xs
        assert mon["peak-temperature"][k] == T.max(), k
        assert mon["peak-position"][k] == pos[np.argmax(T)], k
        conc = pk["dataYCons2"] if model == "N2" else pk["dataYCons"]
        assert np.array_equal(mon["state-max"][k, :conc.shape[0]], conc.max(axis=1))
        assert np.array_equal(mon["state-min"][k, :conc.shape[0]], conc.min(axis=1))
        assert np.array_equal(mon["state-argmax"][k, :conc.shape[0]], pos[conc.argmax(axis=1)])
    for a, b in zip(coarse, (fine[2], fine[5])):
        assert a["dataTime"] == b["dataTime"]
        for key in a:
            if isinstance(a[key], np.ndarray):
                assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("model", ["N2", "M2"])
def test_emulated_run_equals_the_fine_unmonitored_run(model):
    del MONITOR_CALLS[:]
    a = _emu_run(_emu_input(model, 2, {"samples": 3}))
    assert len(MONITOR_CALLS) == 7 and not any(k.endswith("raw") for k in a["device-stats"])
    b = _emu_run(_emu_input(model, 6))
    assert "monitor" not in b and len(MONITOR_CALLS) == 7          # without the key nothing is monitored
    xs = np.linspace(0, INP.m2_dme_input()["reactor"]["ReLe"], 48)
    check_against_fine(a["monitor"], a["dataPack"], b["dataPack"], model, xs)
    m = a["monitor"]
    assert m["labelList"][-1] == "Temperature" and m["outlet"].shape == (7, len(m["labelList"]))
    # sample 0 is the initial state: flat profiles, argmax at node 0 (model M2's too)
    assert np.all(m["state-argmax"][0] == 0.0) and np.array_equal(m["state-max"][0], m["state-min"][0])
    assert "residual" not in m
    # explicit times: the same numbers at the same launches
    t = [float(x) for x in m["time"][1:]]
    c = _emu_run(_emu_input(model, 2, {"times": t}))
    for key in ("time", "outlet", "state-max", "state-min", "state-argmax", "peak-temperature", "peak-position"):
        assert np.array_equal(c["monitor"][key], m[key]), key


ENSEMBLE = [{"operating-conditions": {"temperature": 518.0}}, {"operating-conditions": {"temperature": 531.0}}]


@pytest.mark.parametrize("output", ["profile", "outlet"])
def test_emulated_two_member_ensemble(output):
    mi = _emu_input("N2", 2, {"samples": 3}, ENSEMBLE)
    mi["solver-config"]["ensemble-output"] = output
    a = _emu_run(mi)
    b = _emu_run(_emu_input("N2", 6, None, ENSEMBLE))
    assert len(a["ensemble"]) == 2
    for e in range(2):
        mon = a["ensemble"][e]["monitor"]
        fine = b["ensemble"][e]["dataPack"]
        if output == "profile":
            check_against_fine(mon, a["ensemble"][e]["dataPack"], fine)
        else:
            for k in range(1, 7):
                assert relerr(mon["outlet"][k], fine[k - 1]["dataYs"][:, -1]) <= 1e-14
                assert mon["peak-temperature"][k] == fine[k - 1]["dataYTemp2"].max()
            for a_pk, k in zip(a["ensemble"][e]["dataPack"], (2, 5)):
                assert relerr(a_pk["dataYs"][:, 0], fine[k]["dataYs"][:, -1]) <= 1e-14
    assert a["monitor"] is a["ensemble"][0]["monitor"]              # the base member is member 0
    assert a["ensemble"][0]["monitor"]["peak-temperature"][-1] < a["ensemble"][1]["monitor"]["peak-temperature"][-1]


# ----------------------------------------------------------------------------- two ranks under gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ens = ENSEMBLE + [{"operating-conditions": {"temperature": 525.0}}]
        res = _emu_run(_emu_input("N2", 2, {"samples": 3}, ens))
        if rank == 0:
            assert len(res["ensemble"]) == 3
            np.savez(out_path, **{"%s_%d" % (k, e): m["monitor"][k] for e, m in enumerate(res["ensemble"])
                                  for k in ("time", "outlet", "state-max", "state-argmax", "peak-temperature")})
        else:
            assert res["ensemble"] is None and "monitor" not in res
    finally:
        dist.destroy_process_group()


def test_two_ranks_gather_the_monitor_once(tmp_path):
    """rmtExe under a world-size-2 gloo group (members 0-1 on rank 0, member 2 on rank 1): rank 0 holds every member's
    monitor, equal to the single-process run bit for bit."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "mon.npz")
    mp.start_processes(_rank_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = np.load(out)
    ens = ENSEMBLE + [{"operating-conditions": {"temperature": 525.0}}]
    one = _emu_run(_emu_input("N2", 2, {"samples": 3}, ens))
    for e, m in enumerate(one["ensemble"]):
        for k in ("time", "outlet", "state-max", "state-argmax", "peak-temperature"):
            assert np.array_equal(got["%s_%d" % (k, e)], m["monitor"][k]), (k, e)
