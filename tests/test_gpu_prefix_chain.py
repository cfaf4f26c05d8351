"""GPU: the cross-wave part of the pressure scan with one LDS round trip per batch of records (RMT_PREFIX_MODE 4,
csrc/kernels/25_prefix.inc; profiles/prefix_chain.md) against the scalar loop it replaces in the bench unit
(RMT_PREFIX_MODE=2): the same operations in the same order, so the states agree bit for bit.  Members 0 and 2047 of the
bench's inlet-T / pressure sweep, 60 steps of 2 us.  The caching one-workgroup stepper at 512 x 2 (n2.code_plan selects the new mode
there: dev.defines says so) on 899 nodes - all eight waves hold real nodes, the chain has its full length, the last lane
holds one valid node - and on 131 nodes - identity totals in the waves beyond the reactor's end -, at 256 x 1 on 200 nodes (four waves); the
carry-out form (rmt_prefix_from) in rmt_n2_rhs on 600 nodes at block 256; a reactor chained over two workgroups."""
import numpy as np
import pytest

import bench
from rmt_app_amd import plan
from rmt_app_amd.n2 import N2Device

pytestmark = pytest.mark.gpu
STEPS, DT = 60, 2e-6
MODE2 = {"RMT_PREFIX_MODE": "2"}
MODE4 = {"RMT_PREFIX_MODE": "4"}


def _members(N):
    inputs = [bench.sweep_member_inputs(m, 1)[0] for m in (0, 2047)]
    mech = plan.Mechanism(inputs[0])
    packed = [plan.member_constants(mi, mech, N) for mi in inputs]
    rows = np.array([row for _, row in packed])
    IV = np.array([plan.initial_state(nm, mech, N) for nm, _ in packed])
    return mech, rows, IV


def _run(mech, rows, IV, N, block, npt, defines, what="rk4"):
    dev = N2Device(mech, rows, N, block=block, npt=npt, defines=defines)
    y = dev.to_device(IV)
    if what == "rk4":
        dev.rk4(y, DT, STEPS)
        out = y.cpu().numpy()
    else:
        out = dev.rhs(y).cpu().numpy()
    res = (out, dev.status().copy(), dict(dev.defines), dev.fallbacks())
    dev.close()
    return res


def _pair(N, block, npt, new_defines, what="rk4"):
    mech, rows, IV = _members(N)
    new, nflags, ndefs, nfb = _run(mech, rows, IV, N, block, npt, new_defines, what)
    old, oflags, odefs, ofb = _run(mech, rows, IV, N, block, npt, MODE2, what)
    assert odefs.get("RMT_PREFIX_MODE") == "2" and ndefs.get("RMT_PREFIX_MODE") == "4"      # (the plan's default or the caller's)
    assert not nflags.any() and not oflags.any()
    assert nfb == ofb
    assert np.isfinite(new).all() and new.shape == (2, mech.V*N)
    print("%d x %d, N = %d, %s: max |new - old| = %.3e, fallbacks %d / %d" % (
        block, npt, N, what, float(np.max(np.abs(new - old))), nfb, ofb))
    return new, old, ndefs


@pytest.mark.parametrize("N", [899, 131])
def test_caching_stepper_at_512x2_default_vs_scalar_loop(N):
    new, old, defs = _pair(N, 512, 2, None)
    assert defs.get("RMT_KCACHE") == "1"                      # the unit whose default is the new mode
    assert np.array_equal(new, old)


def test_caching_stepper_at_256x1_four_waves():
    new, old, defs = _pair(200, 256, 1, MODE4)
    assert defs.get("RMT_KCACHE") == "1"
    assert np.array_equal(new, old)


def test_carry_out_kernel_rhs_over_three_blocks():
    """rmt_n2_rhs walks 600 nodes in blocks of 256: every block hands the pressure leaving it (rmt_prefix_from) on"""
    new, old, _ = _pair(600, 256, 1, MODE4, what="rhs")
    assert np.array_equal(new, old)


def test_chained_reactor_two_workgroups():
    new, old, _ = _pair(1100, 512, 2, MODE4)
    assert np.array_equal(new, old)
