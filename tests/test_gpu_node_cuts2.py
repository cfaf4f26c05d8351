"""GPU: the second round of cuts of the N2 node function (RMT_NODE_NO_X, RMT_KC_FOLD, RMT_KIN_FOLD_FM, RMT_KIN_GAIN_RCP,
RMT_NODE_PAIR_RCP; profiles/node_cuts.md) in the caching one-workgroup RK4 stepper.  The bench geometry 512 x 2 on 131
nodes - a partly filled last lane pair, the lane 0 / lane 63 exchanges in three waves, the pair reciprocal with one valid
node in a lane - and 64 x 1 on 20 nodes, where the pair reciprocal is inactive.  Members 0 and 2047 of the bench's
inlet-T / pressure sweep, from the reference's initial state with the product species at the clamp RMT_EPS (the widest
range the shared reciprocal of rate laws and gain meets), 60 steps of 2 us: ten moves of the cache's reference point.
Against the host emulation's RK4 of the generated source and against the same kernel with the new switches off; and
with the cache's range shrunk until every reactor goes to the plain stepper, which returns the plain build's bits."""
import numpy as np
import pytest

import bench
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, plan
from rmt_app_amd.n2 import N2Device, kc_period

pytestmark = pytest.mark.gpu
OFF2 = {"RMT_NODE_NO_X": "0", "RMT_KC_FOLD": "0", "RMT_KIN_FOLD_FM": "0", "RMT_KIN_GAIN_RCP": "0",
        "RMT_NODE_PAIR_RCP": "0"}
STEPS, DT = 60, 2e-6
PRODUCTS = ("H2O", "CH3OH", "DME")


@pytest.fixture(scope="module")
def emu():
    mech = plan.Mechanism(bench.sweep_member_inputs(0, 1)[0])
    return HostEmu(mech.source(hipbind.kernel_template()), tag="dme_nb_cuts2")


def _members(N):
    inputs = [bench.sweep_member_inputs(m, 1)[0] for m in (0, 2047)]
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
def test_cached_stepper_with_the_new_cuts_vs_host_emulation_and_vs_the_switches_off(block, npt, N, emu):
    mech, rows, IV = _members(N)
    E, V = len(rows), mech.V
    assert E == 2 and int((IV.reshape(E, V, N)[:, :mech.S, 0] == 0.0).sum()) == 3*E     # products at the clamp
    got, flags, defs, fb = _run(mech, rows, IV, N, block, npt)
    assert defs.get("RMT_KCACHE") == "1" and not set(OFF2) & set(defs)   # the caching stepper, cuts at their defaults
    assert "RMT_MC_INV_MACOTE" not in defs                               # FM differs between the members, as in the bench
    assert kc_period(defs, DT) == 6                                      # ten moves of the reference point in 60 steps
    assert not flags.any() and fb == 0
    want, eflags = emu.rk4(IV, rows, N, DT, STEPS)
    assert not eflags.any()
    sc = np.max(np.abs(want.reshape(E, V, N)), axis=2, keepdims=True)
    e_emu = np.max(np.abs(got - want).reshape(E, V, N)/sc)
    off, oflags, odefs, ofb = _run(mech, rows, IV, N, block, npt, defines=OFF2)
    assert all(odefs.get(k) == "0" for k in OFF2) and odefs.get("RMT_KCACHE") == "1"
    assert not oflags.any() and ofb == 0
    so = np.max(np.abs(off.reshape(E, V, N)), axis=2, keepdims=True)
    e_off = np.max(np.abs(got - off).reshape(E, V, N)/so)
    print("%d x %d, N = %d: vs host emulation %.2e, vs switches off %.2e" % (block, npt, N, e_emu, e_off))
    assert e_emu < 1e-11
    assert e_off < 2e-13


def test_every_reactor_out_of_range_returns_the_plain_build_bit_for_bit():
    """RMT_KCACHE_THR 1e-12: every stage of every reactor leaves the cache's range, the launch is integrated again by the
    plain stepper of the same code object - which calls the plain rate function, not the caching stepper's."""
    N, block, npt = 131, 512, 2
    mech, rows, IV = _members(N)
    got, flags, defs, fb = _run(mech, rows, IV, N, block, npt, defines={"RMT_KCACHE_THR": "1e-12"})
    assert defs.get("RMT_KCACHE") == "1" and defs["RMT_KCACHE_THR"] == "1e-12" and not set(OFF2) & set(defs)
    assert not flags.any() and fb == len(rows)
    plain, pflags, pdefs, pfb = _run(mech, rows, IV, N, block, npt, defines={"RMT_KCACHE": "0"})
    assert pdefs["RMT_KCACHE"] == "0" and not pflags.any() and pfb == 0
    np.testing.assert_array_equal(got, plain)
