"""GPU: host paths of csrc/rmt_n2.cpp that no other test reaches - a handle's workspace and link buffers growing (and not
growing) between calls of different steppers, rmt_n2_rk4 on a stream that is being captured into a graph, and the release of
the side modules and of a handle whose fallback counter is still on its way back.  Everything is compared bit for bit with
the same call on a fresh handle: the buffers' history must not show in a result."""
import functools

import numpy as np
import pytest

import inputs as INP
from rmt_app_amd import hipbind, plan
from rmt_app_amd.n2 import N2Device

pytestmark = pytest.mark.gpu


def _members(make_input, N, temps):
    mech = plan.Mechanism(make_input())
    rows, named = [], []
    for T in temps:
        mi = make_input()
        mi["operating-conditions"]["temperature"] = T
        nm, row = plan.member_constants(mi, mech, N)
        rows.append(row), named.append(nm)
    return mech, np.array(rows), np.array([plan.initial_state(nm, mech, N) for nm in named])


def _result(dev, y, stats=True):
    """everything a call leaves behind: the state's bytes, the status words and (adaptive steppers) the step counters"""
    return y.cpu().numpy().tobytes(), dev.status().tobytes(), dev._stats.cpu().numpy().tobytes() if stats else b""


# ----------------------------------------------------------------------------- the workspace (rmt_n2_handle work buffer, mask)
# memory mode: rk4 needs 3 state arrays, rk45 10, multistep 8, ros4 8 + V and the mask
WORK_CALLS = {
    "rk4": lambda dev, y: dev.rk4(y, 4e-3, 50),
    "rk45": lambda dev, y: dev.rk45(y, 0.0, 0.2, 1e-6, 1e-9, 1e-6, 10**6),
    "multistep": lambda dev, y: dev.multistep(y, 4e-3, 50),
    "ros4": lambda dev, y: dev.ros4(y, 0.0, 0.2, 1e-6, 1e-9, 1e-5, 10**6),
}
ADAPTIVE = ("rk45", "ros4")          # (the fixed-step ones leave the counters of the call before them)


@functools.lru_cache(maxsize=None)
def _work_case():
    return _members(INP.ch4_input, 20, (973.0, 963.0, 953.0))


def _work_device():
    mech, rows, IV = _work_case()
    dev = N2Device(mech, rows, 20, block=64, npt=1, features=("ros4",), specialize=False)
    dev.set_mode("mem")
    return dev, IV


@functools.lru_cache(maxsize=None)
def _work_fresh(name):
    """the call on a handle that has made no other"""
    dev, IV = _work_device()
    y = dev.to_device(IV)
    WORK_CALLS[name](dev, y)
    out = _result(dev, y, name in ADAPTIVE)
    dev.close()
    assert not np.frombuffer(out[1], dtype=np.uint32).any(), name
    return out


@pytest.mark.parametrize("order", [("rk4", "rk45", "multistep", "ros4", "rk4"), ("rk4", "ros4", "multistep", "rk45", "rk4"),
                                   ("ros4", "multistep", "rk45", "rk4")],
                         ids=["growing", "reverse", "largest-first"])
def test_workspace_regrowth_leaves_no_trace_in_the_results(order):
    """One handle, every memory-resident stepper in turn from the same initial state: the workspace grows 3 -> 10 -> (8) ->
    8 + V arrays and the mask appears late (first order); the reverse order grows once, 3 -> 8 + V, and then serves every
    smaller need; the last order starts at the largest size and never reallocates."""
    dev, IV = _work_device()
    for name in order:
        y = dev.to_device(IV)
        WORK_CALLS[name](dev, y)
        assert _result(dev, y, name in ADAPTIVE) == _work_fresh(name), name
    dev.close()


# ----------------------------------------------------------------------------- the links of the chained stiff stepper
def test_link_buffer_regrowth_leaves_no_trace_in_the_results(monkeypatch):
    """tests/test_gpu_ros4_chain.py's smallest case (1000 nodes in 8 blocks of 128, two reactors): 2 chunks, then 8 - the
    rings of the second call do not fit the first call's allocation."""
    N = 1000
    mech, rows, IV = _members(INP.dme_notebook_input, N, (523, 533))

    def call(dev, chunks):
        monkeypatch.setenv("RMT_N2_ROS4_CHUNKS", str(chunks))
        y = dev.to_device(IV)
        dev.ros4(y, 0.0, 2e-3, 1e-6, 1e-9, 1e-5, 10**6)
        monkeypatch.delenv("RMT_N2_ROS4_CHUNKS")
        assert dev.last_geometry() == (chunks, 2)
        return _result(dev, y)

    def device():
        dev = N2Device(mech, rows, N, block=128, npt=1, features=("ros4",))
        dev.set_mode("chain")
        return dev
    one = device()
    got = [call(one, 2), call(one, 8)]
    one.close()
    for chunks, g in zip((2, 8), got):
        fresh = device()
        want = call(fresh, chunks)
        fresh.close()
        assert not np.frombuffer(want[1], dtype=np.uint32).any()
        assert g == want, chunks


# ----------------------------------------------------------------------------- the caching one-workgroup stepper
@functools.lru_cache(maxsize=None)
def _cached_case():
    """the 512 x 2 unit of tests/test_gpu_kcache.py with 4 members"""
    return _members(INP.dme_notebook_input, 1024, tuple(513.0 + 4.0*e for e in range(4)))


def _cached_device():
    mech, rows, IV = _cached_case()
    dev = N2Device(mech, rows, 1024, block=512, npt=2)
    assert dev.defines.get("RMT_KCACHE") == "1"
    return dev, IV


def test_rk4_on_a_capturing_stream_replays_to_the_eager_result_and_leaves_the_timed_bracket_alone():
    """rmt_n2_rk4 of a caching code object while its stream is captured into a graph: the cached and the plain kernel go
    into the graph; one replay gives the eager call's state bit for bit, the handle's timing events are still the eager
    call's (the captured call recorded none: rmt_n2_last_kernel_ms repeats its figure), and the counter is still readable
    afterwards."""
    import torch
    dev, IV = _cached_device()
    s = torch.cuda.Stream(device=dev.device)
    with torch.cuda.stream(s):
        dev.use_current_stream()
        eager = dev.to_device(IV)
        dev.rk4(eager, 2e-6, 10)
        s.synchronize()
        eager_ms = dev.last_kernel_ms()
        assert eager_ms > 0
        y = dev.to_device(IV)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            dev.rk4(y, 2e-6, 10)
        graph.replay()
        s.synchronize()
        assert dev.last_kernel_ms() == eager_ms
        np.testing.assert_array_equal(y.cpu().numpy(), eager.cpu().numpy())
        assert not np.array_equal(y.cpu().numpy(), np.asarray(IV).reshape(y.shape))
        assert dev.fallbacks() == 0 and not dev.status().any()
    dev.close()


# ----------------------------------------------------------------------------- ownership
def test_side_modules_and_a_handle_with_a_pending_counter_copy_are_released():
    """rmt_n2_{monitor,control,fit}_create / _destroy on the device, and rmt_n2_destroy directly behind a cached launch (its
    counter copy may still be in flight: destroy waits for it).  A clean return is all that is asked."""
    for cls in (hipbind.Monitor, hipbind.Control, hipbind.Fit):
        side = cls()
        assert side.h
        side.close()
        assert side.h is None
    dev, IV = _cached_device()
    y = dev.to_device(IV)
    dev.rk4(y, 2e-6, 10)
    dev.close()
    assert dev.h is None
