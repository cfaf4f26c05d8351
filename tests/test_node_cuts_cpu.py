"""CPU-only: the cuts of the N2 node function's instruction count (profiles/node_cuts.md) - the convective term with a
folded constant (RMT_NODE_CONV_FOLD), mole fractions from the scaled state where the kinetics never read SpCoi
(RMT_NODE_X_FROM_STATE / RMT_KIN_USES_C) and one reciprocal for the independent divisions of the generated rate laws
(lowering.Lowered.div_groups, RMT_DIV_BATCH).  The generated source through the host emulation against the reference
goldens and against the same source with every cut switched off; the division pass itself; the cross-compiled bench
code object."""
import hashlib
import os
import re

import numpy as np
import pytest

import inputs as INP
from oracle import n2_oracle as O
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, isa, lowering, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
OFF = {"RMT_DIV_BATCH": "0", "RMT_NODE_CONV_FOLD": "0", "RMT_NODE_X_FROM_STATE": "0"}
MECHS = {"dme_nb": INP.dme_notebook_input, "dme_script": INP.dme_script_input, "syn12": INP.syn12_input,
         "ch4": INP.ch4_input, "ch4_arrhenius": INP.ch4_arrhenius_input}


def rowwise_err(a, b, V):          # the suite's norm (test_host_cpu.py): per variable row, relative to the row's maximum
    a = np.asarray(a, float).reshape(V, -1)
    b = np.asarray(b, float).reshape(V, -1)
    den = np.max(np.abs(b), axis=1)
    den[den == 0] = 1.0
    return np.max(np.max(np.abs(a - b), axis=1)/den)


@pytest.fixture(scope="module")
def template():
    return hipbind.kernel_template()


def _states_and_reference(name, mi, mech, zNo=20):
    """(states [K][V*zNo], reference RHS [K][V*zNo]): the committed golden g2_rhs.npz (states and right-hand sides of the
    reference itself); ch4_arrhenius has no golden there - its states are the initial one and a perturbed one, the
    right-hand side is the oracle's transcription of the reference (oracle/n2_oracle.py)."""
    if name != "ch4_arrhenius":
        g = np.load(os.path.join(G, "g2_rhs.npz"))
        return g["%s_%d_y" % (name, zNo)], g["%s_%d_f" % (name, zNo)]
    pr = O.setup_n2(mi, zNo)
    f = O.make_rhs_vec(pr)
    y0 = np.array(pr["IV"], dtype=float)
    rng = np.random.default_rng(7)
    y1 = y0.reshape(mech.V, zNo).copy()
    y1[:mech.S] = np.abs(y1[:mech.S]*(1.0 + 0.2*rng.random((mech.S, zNo)))) + 0.01*rng.random((mech.S, zNo))
    y1[mech.S] = 0.02*rng.random(zNo)
    Y = np.array([y0, y1.flatten()])
    return Y, np.array([f(0.0, y) for y in Y])


@pytest.mark.parametrize("name", list(MECHS))
def test_rhs_with_the_cuts_vs_reference_and_vs_the_cuts_switched_off(name, template):
    zNo = 20
    mi = MECHS[name]()
    mech = plan.Mechanism(mi)
    _, row = plan.member_constants(mi, mech, zNo)
    Y, F = _states_and_reference(name, mi, mech, zNo)
    new = HostEmu(mech.source(template), tag=name + "_cuts")
    old = HostEmu(mech.source(template, defines=OFF), tag=name + "_nocuts")
    rows = np.tile(row, (len(Y), 1))
    out, flags = new.rhs(Y, rows, zNo)
    ref, rflags = old.rhs(Y, rows, zNo)
    assert not flags.any() and not rflags.any()
    for k in range(len(Y)):
        e_new, e_old, e_rel = rowwise_err(out[k], F[k], mech.V), rowwise_err(ref[k], F[k], mech.V), \
            rowwise_err(out[k], ref[k], mech.V)
        print("%s state %d: new vs reference %.2e, cuts off vs reference %.2e, new vs cuts off %.2e"
              % (name, k, e_new, e_old, e_rel))
        assert e_new < 1e-12, k
        assert e_rel < 1e-13, k
    # one more state: three species at the clamp (RMT_EPS; the bench's own start has its products there)
    yc = Y[0].reshape(mech.V, zNo).copy()
    clamp = [mech.compList.index(s) for s in ("H2O", "CH3OH", "DME")] if name.startswith("dme") else \
        list(range(mech.S - 3, mech.S))                   # (DME: the product species)
    yc[clamp] = 0.0
    a, fa = new.rhs(yc.flatten(), row, zNo)
    b, fb = old.rhs(yc.flatten(), row, zNo)
    assert (fa == fb).all()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    e = rowwise_err(a[0], b[0], mech.V)
    print("%s clamped state: new vs cuts off %.2e" % (name, e))
    assert e < 1e-13


def _lines_without_groups(src):
    """the emission's lines without the blocks of the groups (their prefix products and reciprocals)"""
    return [ln for ln in src.split("\n") if not re.match(r"\s+const real b\d+_[pti]\d+ = .*;$", ln)]


def _ancestors(dag, i):
    """every node the value of node i depends on (i itself not included)"""
    seen, stack = set(), [i]
    while stack:
        for o in dag.g.operands(stack.pop()):
            if o not in seen:
                seen.add(o)
                stack.append(o)
    return seen


# sha256[:16] of the emission text (plain, with the cached section under the "basis" policy) before the pass existed
PARENT_TEXT = {"dme_nb": ("cc0f9b928e7702ca", "79956f42be6cd312"), "dme_script": ("39245882e70bed40", "de0b11533124942d"),
               "ch4": ("13393a21f8d994e0", "13393a21f8d994e0"), "syn12": ("dd6a014c1251578a", "bcdf8f3eb99b9dc4"),
               "ch4_arrhenius": ("060c6558e82c9bf9", "1fd949c62d50f734")}


@pytest.mark.parametrize("name", list(MECHS))
def test_division_groups_and_the_switch(name, template):
    mech = plan.Mechanism(MECHS[name]())
    dag = mech.device_dag()
    groups = dag.div_groups()
    members = [n for grp in groups for n in grp]
    assert len(members) == len(set(members))
    for grp in groups:
        assert 2 <= len(grp) <= 4 == lowering.Lowered.DIV_BATCH_CAP
        for n in grp:
            assert dag.g.nodes[n][0] in ("div", "rcp")
            anc = _ancestors(dag, dag.denominator(n)) | {dag.denominator(n)}
            assert not anc & set(grp), (grp, n)             # no denominator depends on another member's result
    if name.startswith("dme"):
        assert len(groups) == 1 and len(groups[0]) == 4     # the four divisions of the DME rate laws
    # a smaller cap splits the groups, it never drops the independence
    for grp in dag.div_groups(cap=2):
        assert len(grp) == 2
    # RMT_DIV_BATCH 0: the emission text from before the pass, bit for bit
    plain, cached = dag.emit("rmt_kinetics"), dag.emit("rmt_kinetics", kcache=True, kcache_gen="basis")
    assert (hashlib.sha256(plain.encode()).hexdigest()[:16], hashlib.sha256(cached.encode()).hexdigest()[:16]) \
        == PARENT_TEXT[name]
    assert plain in mech.source(template, defines={"RMT_DIV_BATCH": "0"})
    on = dag.emit("rmt_kinetics", div_batch=True)
    assert on in mech.source(template)                       # the default
    assert (on == plain) == (not groups)
    # every RMT_CHECK_DEN stays, on the same values; one reciprocal per group, none per member
    assert sorted(re.findall(r"RMT_CHECK_DEN\(flag, [^)]*\)", on)) == sorted(re.findall(r"RMT_CHECK_DEN\(flag, [^)]*\)", plain))
    count = lambda s: s.count("rmt_rcp(") + s.count("rmt_div(")
    assert count(on) == count(plain) - sum(len(grp) - 1 for grp in groups)
    assert len(_lines_without_groups(on)) == len(plain.split("\n"))
    # a unit with the gradient DAG of the stiff / steady steppers keeps the plain rates: rmt_kinetics and
    # rmt_kinetics_jac are the same arithmetic there
    for feature in ("RMT_WITH_ROS4", "RMT_WITH_N1"):
        src = mech.source(template, defines={feature: "1"})
        assert plain in src and not re.search(r"\bb\d+_t\d+\b", src)
    # so do fp32 units and units without the Newton-refined reciprocal: 1/overflow is 0 there, not NaN
    assert not re.search(r"\bb\d+_t\d+\b", mech.source(template, fp32=True))
    assert not re.search(r"\bb\d+_t\d+\b", mech.source(template, defines={"RMT_FAST_MATH": "0"}))


def test_division_groups_on_a_dag_with_dependent_denominators():
    """q1 = a/b, q2 = c/(q1 + d) depends on q1: never in q1's group; q3 = 1/e joins q1; six independent ones: 4 + 2."""
    g = lowering.Graph()
    a, b, c, d, e = (g.inp("x%d" % i) for i in range(5))
    q1 = a/b
    q2 = c/(q1 + d)
    q3 = 1.0/e
    low = lowering.Lowered(g, [(q1*q2 + q3).i], 5)
    groups = low.div_groups()
    assert groups == [sorted([q1.i, q3.i])]
    assert q2.i not in groups[0]
    vals = low.evaluate(500.0, 1e5, [0.3, 0.7, 1.1, 0.2, 0.9], [0.0]*5)
    src = low.emit("k", div_batch=True)
    assert src.count("rmt_rcp(") + src.count("rmt_div(") == 2 and vals[0] == pytest.approx(0.3/0.7*1.1/(0.3/0.7 + 0.2) + 1/0.9)
    g = lowering.Graph()
    xs = [g.inp("x%d" % i) for i in range(7)]
    tot = None
    for k in range(6):
        q = xs[6]/xs[k]
        tot = q if tot is None else tot + q
    low = lowering.Lowered(g, [tot.i], 7)
    # (x6/x_k interleaved with the running sum: every denominator is an input, so all six are independent)
    sizes = sorted(len(grp) for grp in low.div_groups())
    assert sizes == [2, 4]
    # a temperature-only denominator and 1/T stay out (they belong to the cached section / come with the node state)
    g = lowering.Graph()
    T, x0, x1 = g.inp("T"), g.inp("x0"), g.inp("x1")
    low = lowering.Lowered(g, [(x0/(T*T + 1.0) + x1/T + 1.0/x0 + 1.0/x1).i], 2)
    grp, = low.div_groups()
    assert [low.g.nodes[low.denominator(n)][:2] for n in grp] == [("in", "x0"), ("in", "x1")]


def test_bench_code_object_with_the_cuts():
    """device_source(dme, rows, 1024): the one-workgroup caching RK4 stepper at 512 x 2 - still at the register limit
    without spills in its step loop, the LDS budget untouched, fewer fp64 instructions and half the reciprocals."""
    from rmt_app_amd.n2 import device_source
    dme = plan.Mechanism(INP.dme_notebook_input())
    _, row = plan.member_constants(INP.dme_notebook_input(), dme, 1024)
    block, npt, defs, src, key = device_source(dme, np.tile(row, (256, 1)), 1024)
    assert (block, npt) == (512, 2) and defs.get("RMT_KCACHE") == "1" and not set(OFF) & set(defs)
    from rmt_app_amd.n2 import compile_options
    blob = hipbind.compile_cached(src, key, "gfx950", compile_options(block, npt, (), "", defs))
    st = isa.kernel_stats(blob, "rmt_n2_rk4_reg")["step_loop"]
    res = isa.kernel_resources(blob, "rmt_n2_rk4_reg")
    print("step loop:", st, "resources:", res)
    assert st["scratch"] == 0
    assert res["vgpr_count"] <= 256
    assert res["group_segment_fixed_size"] == 161072
    # (256 copies of the notebook's row: 2969 fp64 of 3528 VALU, private segment 0 B; the bench's own sweep, whose members
    # differ in inlet temperature and pressure, gives 2966 of 3495 and 12 B, from PyTorch's hipRTC and from the system's alike)
    assert st["valu_f64"] <= 3000                  # 3159 without the cuts
    assert st["rcp_f64"] <= 40                     # 62 without the cuts
