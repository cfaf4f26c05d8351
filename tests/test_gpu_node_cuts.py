"""GPU: the N2 node function with its instruction-count cuts (RMT_NODE_CONV_FOLD, RMT_NODE_X_FROM_STATE, RMT_DIV_BATCH;
profiles/node_cuts.md) in the caching one-workgroup RK4 stepper - the bench geometry 512 x 2 on a mesh that leaves the
second wave nearly empty and one lane with a single valid node, and the one-wave geometry 64 x 1.  Members 0, 1000 and
2047 of the bench's inlet-T / pressure sweep plus the notebook's own input, from the reference's initial state with the
product species at the clamp RMT_EPS (the widest range the shared reciprocal of the rate laws meets), 60 steps of 2 us - the cache's
reference point moves ten times.  Against the host emulation's RK4 of the same generated source and against the build
with every cut switched off."""
import numpy as np
import pytest

import bench
import inputs as INP
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, plan
from rmt_app_amd.n2 import N2Device, kc_period

pytestmark = pytest.mark.gpu
OFF = {"RMT_DIV_BATCH": "0", "RMT_NODE_CONV_FOLD": "0", "RMT_NODE_X_FROM_STATE": "0"}
STEPS, DT = 60, 2e-6
PRODUCTS = ("H2O", "CH3OH", "DME")


@pytest.fixture(scope="module")
def emu():
    mech = plan.Mechanism(INP.dme_notebook_input())
    return HostEmu(mech.source(hipbind.kernel_template()), tag="dme_nb_cuts")


def _members(N):
    inputs = [bench.sweep_member_inputs(m, 1)[0] for m in (0, 1000, 2047)] + [INP.dme_notebook_input()]
    mech = plan.Mechanism(inputs[0])
    packed = [plan.member_constants(mi, mech, N) for mi in inputs]
    rows = np.array([row for _, row in packed])
    IV = np.array([plan.initial_state(nm, mech, N) for nm, _ in packed]).reshape(len(inputs), mech.V, N)
    IV[:, [mech.compList.index(s) for s in PRODUCTS]] = 0.0       # below the clamp: the kernels see RMT_EPS
    return mech, rows, IV.reshape(len(inputs), mech.V*N)


def _run(mech, rows, IV, N, block, npt, defines=None):
    dev = N2Device(mech, rows, N, block=block, npt=npt, defines=defines)
    y = dev.to_device(IV)
    dev.rk4(y, DT, STEPS)
    out = (y.cpu().numpy(), dev.status().copy(), dict(dev.defines), dev.fallbacks())
    dev.close()
    return out


@pytest.mark.parametrize("block,npt,N", [(512, 2, 131), (64, 1, 20)])
def test_cached_stepper_with_the_cuts_vs_host_emulation_and_vs_the_cuts_switched_off(block, npt, N, emu):
    mech, rows, IV = _members(N)
    E, V = len(rows), mech.V
    assert E == 4 and int((IV.reshape(E, V, N)[:, :mech.S, 0] == 0.0).sum()) == 3*E     # products at the clamp
    got, flags, defs, fb = _run(mech, rows, IV, N, block, npt)
    assert defs.get("RMT_KCACHE") == "1" and not set(OFF) & set(defs)    # the caching stepper, cuts at their defaults
    assert kc_period(defs, DT) == 6                                      # ten moves of the reference point in 60 steps
    assert not flags.any() and fb == 0
    want, eflags = emu.rk4(IV, rows, N, DT, STEPS)
    assert not eflags.any()
    sc = np.max(np.abs(want.reshape(E, V, N)), axis=2, keepdims=True)
    e_emu = np.max(np.abs(got - want).reshape(E, V, N)/sc)
    off, oflags, odefs, ofb = _run(mech, rows, IV, N, block, npt, defines=OFF)
    assert all(odefs.get(k) == "0" for k in OFF) and odefs.get("RMT_KCACHE") == "1"
    assert not oflags.any() and ofb == 0
    so = np.max(np.abs(off.reshape(E, V, N)), axis=2, keepdims=True)
    e_off = np.max(np.abs(got - off).reshape(E, V, N)/so)
    print("%d x %d, N = %d: vs host emulation %.2e, vs cuts off %.2e" % (block, npt, N, e_emu, e_off))
    assert e_emu < 1e-11
    assert e_off < 2e-13
