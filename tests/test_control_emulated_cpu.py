"""solver-config "control" without a GPU, on a host build of the controller's kernel (tests/helpers/control_emu.cpp
includes csrc/control_kernels.inc) and the host emulation of the steppers (tests/emu_device.py): the kernel against numpy
bit for bit, and the host walk around it - stream order, hold mode, result entries, open-loop replay, gain 0, ensembles.
The unforced emulation of the steppers is exact here because every slope of a forced row is zero in these runs (checked)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emu_device
import inputs as INP
from rmt_app_amd import control, n2, plan, rmtExe, schedule
from rmt_app_amd.ensemble import expand_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
S = 6


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), None)
    assert cxx, "clang++ (the ROCm one) builds the host form of the kernel"
    out = str(tmp_path_factory.mktemp("control_emu")/"libcontrol_emu.so")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared",
                    "-I" + os.path.join(ROOT, "rmt_app_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "control_emu.cpp"),
                    "-o", out], check=True)
    lib = C.CDLL(out)
    lib.emu_update.argtypes = [DP]*6 + [C.c_int]*9
    return lib


def _p(a):
    return None if a is None else (C.cast(a.data_ptr(), DP) if isinstance(a, torch.Tensor) else a.ctypes.data_as(DP))


def _grid(E):
    return min((E + 3)//4, 32)                 # csrc/rmt_n2.cpp RMT_N2_CONTROL_MAX_GRID


def reference(y, rows, prm, r, state, field, tail_at):
    """numpy: one update of every member -> (log [E][4], state [E][3], rows)"""
    E, V, N = y.shape
    log, state, rows = np.zeros((E, control.LOG)), state.copy(), rows.copy()
    F = plan.MEMBER_FIELDS
    for e in range(E):
        sel, tf = int(prm[e, control.P_SELECT]), rows[e, F["TF"]]
        if sel == 2:
            tot = 0.0
            for i in range(S):
                tot += y[e, i, N - 1]
            pv = y[e, int(prm[e, control.P_SPECIES]), N - 1]/tot
        else:
            row = y[e, V - 1]
            theta = row[N - 1] if sel == 0 else np.max(np.where(np.isnan(row), -np.inf, row))
            pv = theta*tf + tf
        u, sat, I = control.emulate([pv], [r[e]], prm[e, 0], prm[e, 1], prm[e, 2], prm[e, 3], prm[e, 4], I0=state[e, 0])
        log[e] = [pv, r[e], u[0], float(sat[0])]
        state[e] = [I[0], u[0], state[e, 2] + 1.0]
        rows[e, (F["THETA_IN"], F["P0"], F["TM"])[field]] = control.field_value(schedule.ORDER[field], u[0], tf)
        rows[e, tail_at + 1 + field] = 0.0
    return log, state, rows


@pytest.mark.parametrize("E", [3, 130])
def test_host_build_of_the_kernel_equals_numpy(emu, E):
    """The cases of the GPU test of the kernel: N in {1, 2, 63, 64, 65, 600}, aligned and unaligned state rows, the peak at
    node 0, N-1 and in between, a NaN that is not the maximum, all three measurements and row fields, the grid-stride walk
    (E = 130 on 32 workgroups of four waves); then hold mode."""
    rng = np.random.default_rng(15 + E)
    V, width, tail_at = S + 1, 16 + S + schedule.TAIL, 16 + S
    F = plan.MEMBER_FIELDS
    rows0 = rng.random((E, width)) + 1.0
    rows0[:, F["TF"]] = 500.0 + 40.0*rng.random(E)
    seen = set()
    for N in (1, 2, 63, 64, 65, 600):
        for shift in (0, 1):
            for sel, field in ((0, 1), (1, 0), (2, 2)):
                y = 0.2*rng.random((E, V, N)) + 0.05
                for e in range(E):
                    pos = (0, N - 1, N//2)[e % 3]
                    y[e, V - 1, pos] = 0.31 + 0.01*rng.random()
                    if N >= 2 and e % 2 == 0:
                        y[e, V - 1, (pos + 1) % N] = np.nan
                prm = np.zeros((E, control.PARAMS))
                prm[:, control.P_KP] = rng.choice([-1.0, 1.0], E)*(1.0 + rng.random(E))*(0.1, 2.0e3, 20.0)[field]
                prm[:, control.P_KI] = np.where(rng.random(E) < 0.3, 0.0, 0.2*prm[:, control.P_KP])
                prm[:, control.P_U0] = (5.0e6 if field == 1 else 520.0)*(1.0 + 0.02*rng.random(E))
                half = (2.0e5 if field == 1 else 8.0)*np.where(rng.random(E) < 0.5, 0.05, 1.0)
                prm[:, control.P_LO], prm[:, control.P_HI] = prm[:, control.P_U0] - half, prm[:, control.P_U0] + half
                prm[:, control.P_SELECT], prm[:, control.P_SPECIES] = sel, rng.integers(0, S, E)
                sp = (0.15 if sel == 2 else 660.0) + (0.01 if sel == 2 else 6.0)*rng.standard_normal((3, E))
                buf = np.zeros(E*V*N + 2)
                off = shift if buf.ctypes.data % 16 == 0 else 1 - shift
                yd = buf[off:off + E*V*N]
                yd[:] = y.reshape(-1)
                d_rows, d_state, d_log = rows0.copy(), np.zeros((E, 3)), np.zeros((3, E, 4))
                state, rows = np.zeros((E, 3)), rows0.copy()
                for k in range(3):
                    spk = np.ascontiguousarray(sp[k])
                    emu.emu_update(_p(yd), _p(d_rows), _p(prm), _p(spk), _p(d_state), _p(d_log[k]), E, S, V, N, width, tail_at,
                                   field, 0, _grid(E))
                    log, state, rows = reference(y, rows, prm, sp[k], state, field, tail_at)
                    what = (E, N, shift, sel, field, k)
                    assert np.array_equal(d_log[k], log, equal_nan=True), what
                    assert np.array_equal(d_state, state, equal_nan=True), what
                    assert np.array_equal(d_rows, rows, equal_nan=True), what
                    seen |= set(log[:, 3])
                d_rows, before = rows0.copy(), (d_log.copy(), d_state.copy())
                emu.emu_update(None, _p(d_rows), None, None, _p(d_state), None, E, S, V, N, width, tail_at, field, 1, _grid(E))
                assert np.array_equal(d_rows, rows, equal_nan=True)
                assert np.array_equal(d_log, before[0], equal_nan=True) and np.array_equal(d_state, before[1], equal_nan=True)
                d_rows, d_state = rows0.copy(), np.zeros((E, 3))           # not sampled yet: the rows stay
                emu.emu_update(None, _p(d_rows), None, None, _p(d_state), None, E, S, V, N, width, tail_at, field, 1, _grid(E))
                assert np.array_equal(d_rows, rows0)
    assert seen == {0.0, 1.0}


# ----------------------------------------------------------------------------- the host walk on emulated devices
class _Device(emu_device.EmuDevice):
    """EmuDevice with forced rows (every slope zero, so the unforced emulation of the steppers is exact), the
    controller's kernel from the host build, and a record of the order of the calls."""
    kernel = None
    order = []

    def __init__(self, mech, members, N, **kw):
        defs = dict(kw.get("defines") or {})
        assert defs.pop("RMT_FORCING") == "1"
        self.full = np.array(members, dtype=np.float64).reshape(-1, mech.row_width + schedule.TAIL)
        kw.update(defines=defs, specialize=False)
        super().__init__(mech, self.full[:, :mech.row_width].copy(), N, **kw)
        self.block, self.npt = 64, 1

    def set_mode(self, mode):
        pass

    def last_geometry(self):
        return 1, 1

    def set_members(self, rows):
        self.full = np.array(rows, dtype=np.float64).reshape(self.E, -1)
        self.order.append("refresh")

    def rk4(self, y, dt, nsteps, t0=0.0):
        assert np.all(self.full[:, self.mech.row_width + 1:] == 0.0)
        self.members = np.ascontiguousarray(self.full[:, :self.mech.row_width])
        self.order.append("stepper")
        super().rk4(y, dt, nsteps, t0)

    def control(self, y, loop, k=None):
        self.order.append("hold" if k is None else "update")
        hold = k is None
        self.kernel.emu_update(None if hold else _p(y), _p(self.full), _p(loop.params), None if hold else _p(loop.setpoints[k]),
                            _p(loop.state), None if hold else _p(loop.log[k]), self.E, self.mech.S, self.mech.V, self.N,
                            self.full.shape[1], self.mech.row_width, loop.field, int(hold), _grid(self.E))


class _Loop:
    """n2.ControlLoop in host memory"""

    def __init__(self, ctl, dev):
        self.ctl, self.E, self.field, self.taken = ctl, ctl.E, ctl.field, 0
        self.params = torch.from_numpy(ctl.params())
        self.setpoints = torch.from_numpy(np.ascontiguousarray(ctl.setpoints))
        self.state = torch.zeros((ctl.E, control.STATE), dtype=torch.float64)
        self.log = torch.zeros((ctl.K, ctl.E, control.LOG), dtype=torch.float64)

    def close(self):
        pass


@pytest.fixture
def emulated(emu, monkeypatch):
    _Device.kernel, _Device.order = emu, []
    monkeypatch.setattr(n2, "device_cls", lambda: _Device)
    monkeypatch.setattr(n2, "ControlLoop", _Loop)
    return _Device


STEP = 0.0205          # the coolant steps BETWEEN two samples: the launch that starts there runs the kernel in hold mode


def _input(with_control=True, gain=5.0e4, ensemble=False):
    mi = INP.dme_notebook_input(ivp="hip-rk4", period=0.04)
    mi["solver-config"].update({"zNo": 20, "tNo": 2, "quiet": True, "dt": 2e-5, "schedule": {
        "time": [0.0, STEP, STEP, 0.04], "medium-temperature": [523.0, 523.0, 533.0, 533.0]}})
    if with_control:
        mi["solver-config"]["control"] = {
            "measured": "outlet-temperature", "manipulated": "inlet-pressure", "sample-time": 0.002, "start": 0.01,
            "setpoint": {"time": [0.0, 0.025, 0.025, 0.04], "value": [530.0, 530.0, 529.0, 529.0]},
            "gain": gain, "integral-time": 0.005, "limits": [4.9e6, 6.0e6]}
    if ensemble:
        mi["solver-config"]["ensemble"] = {"temperature": [518.0, 528.0], "pressure": [4.8e6, 5.2e6]}
    return mi


def _replay(t, u, own=5.0e6):
    """the logged outputs as a schedule of the inlet pressure with a jump at every sample time (and the coolant's step)"""
    def held(x, right):
        v = own
        for b, new in zip(t, u):
            if b < x or (right and b == x):
                v = float(new)
        return v
    times, P, Tm = [0.0], [own], [523.0]
    for x in sorted(set(float(b) for b in t) | {STEP}):
        times += [x, x]
        P += [held(x, False), held(x, True)]
        Tm += [523.0 if x <= STEP else 533.0, 523.0 if x < STEP else 533.0]
    return {"time": times, "inlet-pressure": P, "medium-temperature": Tm}


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x["dataYs"], y["dataYs"])


def test_closed_loop_stream_order_law_and_replay(emulated):
    res = rmtExe(_input())["resModel"]
    c = res["control"]
    assert set(c) == {"time", "measured", "setpoint", "output", "saturated"} and len(c["time"]) == 15
    assert res["device-stats"]["launches"] == 17 and "schedule" in res
    # refresh, controller, stepper - for every launch; nothing before the first sample, hold where no sample is taken
    order = emulated.order
    assert order[:2] == ["refresh", "stepper"] and order[2:5] == ["refresh", "update", "stepper"]
    assert order.count("update") == 15 and order.count("hold") == 1 and order.count("stepper") == 17
    i = order.index("hold")
    assert order[i - 1] == "refresh" and order[i + 1] == "stepper"
    # the law
    mi = _input()
    ctl = control.parse(mi, None, "hip-rk4", schedule.parse(mi, None, "hip-rk4"))[0]
    u, sat, _ = control.emulate(c["measured"], c["setpoint"], ctl.Kp[0], ctl.Ki[0], ctl.u0[0], ctl.lo[0], ctl.hi[0])
    assert np.array_equal(u, c["output"]) and np.array_equal(sat, c["saturated"])
    assert np.array_equal(c["time"], ctl.times) and np.array_equal(c["setpoint"], ctl.setpoints[:, 0])
    assert np.ptp(c["output"]) > 1e4 and sat.any() and not sat.all()
    # open-loop replay: same launches, same rows, same states bit for bit
    mr = _input(False)
    mr["solver-config"]["schedule"] = _replay(c["time"], c["output"])
    rep = rmtExe(mr)["resModel"]
    assert rep["device-stats"]["launches"] == 17 and "control" not in rep
    _same(res["dataPack"], rep["dataPack"])
    # gain 0: the member's own value, the states of the run without "control" on the same launch list
    zero = rmtExe(_input(gain=0.0))["resModel"]
    assert np.all(zero["control"]["output"] == 5.0e6) and not zero["control"]["saturated"].any()
    mp = _input(False)
    mp["solver-config"]["schedule"] = {k: v for k, v in _replay(c["time"], np.full(15, 5.0e6)).items() if k != "inlet-pressure"}
    plain = rmtExe(mp)["resModel"]
    _same(zero["dataPack"], plain["dataPack"])
    assert not np.array_equal(zero["dataPack"][-1]["dataYs"], res["dataPack"][-1]["dataYs"])


def test_every_member_runs_its_own_loop(emulated):
    base = _input(ensemble=True)
    res = rmtExe(base)["resModel"]
    members = expand_members(base, base["solver-config"]["ensemble"])
    assert len(res["ensemble"]) == 4 and res["control"] is res["ensemble"][0]["control"]
    for e in (0, 3):
        single = dict(members[e])
        single["solver-config"] = {k: v for k, v in base["solver-config"].items() if k != "ensemble"}
        one = rmtExe(single)["resModel"]
        assert np.array_equal(one["control"]["output"], res["ensemble"][e]["control"]["output"])
        assert np.array_equal(one["control"]["measured"], res["ensemble"][e]["control"]["measured"])
        _same(one["dataPack"], res["ensemble"][e]["dataPack"])
    assert len({float(m["control"]["output"][0]) for m in res["ensemble"]}) > 1
