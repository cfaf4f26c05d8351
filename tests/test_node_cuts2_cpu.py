"""CPU-only: the second round of cuts of the N2 node function's instruction count (profiles/node_cuts.md, DESIGN.md
section 3j) - rates and mixture sums from the clamped state (RMT_NODE_NO_X / RMT_KIN_XP_INVARIANT, from the degree
bookkeeping of lowering.Lowered.xp_invariant), literal prefactors and the member literal FM inside the cached constants
(RMT_KC_FOLD, RMT_KIN_FOLD_FM), the gain's reciprocal in the rate laws' division group (RMT_KIN_GAIN_RCP) and one
reciprocal for a lane's two nodes (RMT_NODE_PAIR_RCP, GPU only).  The lowering pass; the generated source through the
host emulation against the reference goldens and against itself with the switches off - the plain unit and the unit of
a caching stepper, whose rmt_kinetics_node the emulation calls without a cache; the cached section itself in a
stand-alone host program; the cross-compiled bench code object."""
import os
import subprocess

import numpy as np
import pytest

import inputs as INP
from oracle import n2_oracle as O
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, isa, lowering, n2, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
OFF2 = {"RMT_NODE_NO_X": "0", "RMT_KC_FOLD": "0", "RMT_KIN_FOLD_FM": "0", "RMT_KIN_GAIN_RCP": "0",
        "RMT_NODE_PAIR_RCP": "0"}
MECHS = {"dme_nb": INP.dme_notebook_input, "dme_script": INP.dme_script_input, "syn12": INP.syn12_input,
         "ch4": INP.ch4_input, "ch4_arrhenius": INP.ch4_arrhenius_input}
INVARIANT = {"dme_nb": True, "dme_script": True, "syn12": True, "ch4": False, "ch4_arrhenius": False}


def rowwise_err(a, b, V):          # the suite's norm (test_host_cpu.py): per variable row, relative to the row's maximum
    a = np.asarray(a, float).reshape(V, -1)
    b = np.asarray(b, float).reshape(V, -1)
    den = np.max(np.abs(b), axis=1)
    den[den == 0] = 1.0
    return np.max(np.max(np.abs(a - b), axis=1)/den)


@pytest.fixture(scope="module")
def template():
    return hipbind.kernel_template()


# ------------------------------------------------------------------ the lowering pass
@pytest.mark.parametrize("name", list(MECHS))
def test_invariance_macro(name, template):
    mech = plan.Mechanism(MECHS[name]())
    assert mech.device_dag().xp_invariant() == INVARIANT[name]
    assert mech.lowered.xp_invariant() == INVARIANT[name]
    assert ("#define RMT_KIN_XP_INVARIANT %d\n" % INVARIANT[name]) in mech.prelude()
    if not INVARIANT[name]:
        return
    # the rates at (x, P) and at (3 x, P / 3)
    mi = MECHS[name]()
    c = np.array(mi['feed']['concentration'], dtype=float)
    x = list(c/np.sum(c))
    T, P = float(mi['operating-conditions']['temperature']), float(mi['operating-conditions']['pressure'])
    for dag in (mech.lowered, mech.device_dag()):
        a = np.array(dag.evaluate(T, P, x, [0.0]*mech.S))
        b = np.array(dag.evaluate(T, P/3.0, [3.0*v for v in x], [0.0]*mech.S))
        err = np.max(np.abs(a - b)/np.abs(a))
        print("%s: rates at (3x, P/3) against (x, P): %.2e" % (name, err))
        assert np.all(a != 0.0) and err < 1e-14


def test_invariance_on_hand_built_dags():
    g = lowering.Graph()
    x0, x1, P, T = g.inp("x0"), g.inp("x1"), g.inp("P"), g.inp("T")
    assert not lowering.Lowered(g, [(x0 + P).i], 2).xp_invariant()              # a sum of unequal degrees
    assert not lowering.Lowered(g, [(x0*x1*P).i], 2).xp_invariant()             # degree +1
    assert not lowering.Lowered(g, [((x0*P)._un("exp", np.exp)*x1).i], 2).xp_invariant()
    assert not lowering.Lowered(g, [(g.inp("C0")*T).i], 2).xp_invariant()       # reads SpCoi
    ok = lowering.Lowered(g, [((x0*P)**2/(1.0 + (x1*P)._un("sqrt", np.sqrt)*(x0*P)._un("sqrt", np.sqrt))*T).i,
                              ((x0*P)._un("exp", np.exp)/(x1/x0)).i], 2)
    assert ok.xp_invariant()
    a = np.array(ok.evaluate(500.0, 2.0, [0.3, 0.7], [0.0, 0.0]))
    b = np.array(ok.evaluate(500.0, 2.0/3.0, [0.9, 2.1], [0.0, 0.0]))
    assert np.max(np.abs(a - b)/np.abs(a)) < 1e-14


# ------------------------------------------------------------------ host emulation
def _states_and_reference(name, mi, mech, zNo=20):
    """as in test_node_cuts_cpu.py: the golden g2_rhs.npz; ch4_arrhenius from the oracle's transcription"""
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


def _caching_defines(mech, row, zNo):
    """the defines of the caching one-wave stepper for this mechanism and ONE member row (every field a literal); None
    where n2.kcache_choice switches no cache on"""
    defs, _ = n2.kcache_choice(mech, zNo, False, 64, 1, None, None)
    if defs.get("RMT_KCACHE") != "1":
        return None
    defs.update(plan.uniform_member_defines(np.asarray(row).reshape(1, -1), mech.S))
    return defs


@pytest.mark.parametrize("unit", ["plain", "caching"])
@pytest.mark.parametrize("name", list(MECHS))
def test_rhs_with_the_new_cuts_vs_reference_and_vs_the_switches_off(name, unit, template):
    zNo = 20
    mi = MECHS[name]()
    mech = plan.Mechanism(mi)
    _, row = plan.member_constants(mi, mech, zNo)
    base = {} if unit == "plain" else _caching_defines(mech, row, zNo)
    if base is None:
        assert name == "ch4"                 # nothing temperature-only to cache: its plain unit is the whole check
        return
    src_new = mech.source(template, block=64, npt=1, defines=dict(base))
    src_old = mech.source(template, block=64, npt=1, defines=dict(base, **OFF2))
    if unit == "caching":            # (the emulation passes no cache: the plain twin's path of such a unit, RMT_NODE_NO_X in it)
        assert "#define RMT_KIN_NODE 1" in src_new and "#define RMT_KIN_NODE 1" not in src_old
        assert "#define RMT_KIN_GAIN_DEN 1" in src_new
        assert ("#define RMT_KIN_RATES_FM 1" in src_new) == (name != "ch4_arrhenius")
    else:
        assert "#define RMT_KIN_NODE 1" not in src_new
    Y, F = _states_and_reference(name, mi, mech, zNo)
    new = HostEmu(src_new, tag="%s_%s_cuts2" % (name, unit))
    old = HostEmu(src_old, tag="%s_%s_nocuts2" % (name, unit))
    rows = np.tile(row, (len(Y), 1))
    out, flags = new.rhs(Y, rows, zNo)
    ref, rflags = old.rhs(Y, rows, zNo)
    assert not flags.any() and not rflags.any()
    for k in range(len(Y)):
        e_new, e_rel = rowwise_err(out[k], F[k], mech.V), rowwise_err(out[k], ref[k], mech.V)
        print("%s %s state %d: new vs reference %.2e, new vs switches off %.2e" % (name, unit, k, e_new, e_rel))
        assert e_new < 1e-12, k
        assert e_rel < 1e-13, k
    # three species at the clamp (RMT_EPS; the bench's own start has its products there)
    yc = Y[0].reshape(mech.V, zNo).copy()
    clamp = [mech.compList.index(s) for s in ("H2O", "CH3OH", "DME")] if name.startswith("dme") else \
        list(range(mech.S - 3, mech.S))
    yc[clamp] = 0.0
    a, fa = new.rhs(yc.flatten(), row, zNo)
    b, fb = old.rhs(yc.flatten(), row, zNo)
    assert (fa == fb).all()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    e = rowwise_err(a[0], b[0], mech.V)
    print("%s %s clamped state: new vs switches off %.2e" % (name, unit, e))
    assert e < 1e-13


def test_switches_off_keep_the_plain_rates_and_the_old_text(template):
    mech = plan.Mechanism(INP.dme_notebook_input())
    _, row = plan.member_constants(INP.dme_notebook_input(), mech, 20)
    base = _caching_defines(mech, row, 20)
    dag = mech.device_dag()
    cached = dag.emit("rmt_kinetics", kcache=True, kcache_gen="basis", div_batch=True)
    assert cached in mech.source(template, block=64, npt=1, defines=dict(base))        # rmt_kinetics itself never changes
    for extra in ({"RMT_WITH_ROS4": "1"}, {"RMT_WITH_N1": "1"}, {"RMT_FAST_MATH": "0"}, OFF2):
        assert "#define RMT_KIN_NODE 1" not in mech.source(template, block=64, npt=1, defines=dict(base, **extra))
    assert "#define RMT_KIN_NODE 1" not in mech.source(template, fp32=True, block=64, npt=1, defines=dict(base))
    # a member field FM read at run time is folded too (multiplied in where the reference point moves)
    norow = {k: v for k, v in base.items() if k != "RMT_MC_INV_MACOTE"}
    assert "#define RMT_KIN_RATES_FM 1" in mech.source(template, block=64, npt=1, defines=norow)
    assert "#define RMT_KIN_RATES_FM 0" in mech.source(template, block=64, npt=1, defines=dict(base, RMT_KIN_FOLD_FM="0"))
    # the fold: every literal prefactor of a cached constant is gone from the tail, slots and range tests unchanged
    node = dag.emit("rmt_kinetics_node", kcache=True, kcache_gen="basis", div_batch=True, kcache_fold=True, head=False)
    tail = lambda s: s[s.rindex("\n    }\n"):]            # behind the cached section
    assert tail(cached).count(" * real(") - tail(node).count(" * real(") == 6
    assert [l for l in cached.split("\n") if "kc.leave" in l or "kc.get" in l] == \
        [l for l in node.split("\n") if "kc.leave" in l or "kc.get" in l]
    assert cached.count("kc.put(") == node.count("kc.put(") == 12


# ------------------------------------------------------------------ the cached section, stand-alone on the host
def _build_kcache_program(tmp, src, fn, extra):
    unit = os.path.join(tmp, "unit_%s.inc" % fn)
    with open(unit, "w") as f:
        f.write(src)
    exe = os.path.join(tmp, "kc_%s" % fn)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DRMT_GENERATED_SOURCE=\"%s\"" % unit,
                    "-DKIN_FN=%s" % fn, "-DKIN_EXTRA=%d" % extra, os.path.join(ROOT, "tests", "helpers", "kcache_emu.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("name", ["dme_nb", "syn12"])
def test_cached_section_on_the_host_with_and_without_the_fold(name, template, tmp_path):
    """MODE 0 at T_ref moves the reference point, MODE 2 at T_ref + 0.05 K against MODE 0 there: 5e-15 relative in every
    rate, with the literals folded into the cached constants (and FM, and the gain's reciprocal) and without."""
    zNo = 20
    mi = MECHS[name]()
    mech = plan.Mechanism(mi)
    _, row = plan.member_constants(mi, mech, zNo)
    base = _caching_defines(mech, row, zNo)
    Y, _ = _states_and_reference(name, mi, mech, zNo)
    c = np.array(mi['feed']['concentration'], dtype=float)
    comps = [c/np.max(c)]
    clamped = comps[0].copy()
    clamped[-3:] = 1e-30                                   # products at RMT_EPS
    if name.startswith("dme"):
        clamped = comps[0].copy()
        clamped[[mech.compList.index(s) for s in ("H2O", "CH3OH", "DME")]] = 1e-30
    comps.append(clamped)
    for y in Y:
        for z in (0, zNo//2, zNo - 1):
            comps.append(np.maximum(y.reshape(mech.V, zNo)[:mech.S, z], 1e-30))
    T, P = float(mi['operating-conditions']['temperature']), float(mi['operating-conditions']['pressure'])
    # (x, P) as the node function hands them over: mole fractions and P without RMT_NODE_NO_X - the rates are the same
    lines = "M " + " ".join(repr(float(v)) for v in row) + "\n"
    lines += "".join("K %r %r %r %s\n" % (T, T + 0.05, P, " ".join(repr(float(v)) for v in cs/np.sum(cs))) for cs in comps)
    fm = float(base["RMT_MC_INV_MACOTE"])
    results = {}
    norow = {k: v for k, v in base.items() if k != "RMT_MC_INV_MACOTE"}        # FM from the member row, as in a sweep
    for tag, defs, fn, extra in (("fold", dict(base), "rmt_kinetics_node", 3),
                                 ("fold, FM at run time", norow, "rmt_kinetics_node", 3),
                                 ("fold off", dict(base, RMT_KC_FOLD="0"), "rmt_kinetics_node", 2),
                                 ("plain", dict(base, **OFF2), "rmt_kinetics", 0)):
        src = mech.source(template, block=64, npt=1, defines=defs)
        assert ("#define RMT_KIN_RATES_FM 1" in src) == (tag in ("fold", "fold, FM at run time"))
        exe = _build_kcache_program(str(tmp_path), src, fn, extra)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == len(comps)
        vals = []
        for k, ln in enumerate(out):
            w = ln.split()
            assert w[0] == "1" and w[1] == "0", (tag, k, ln)          # in range, no flag
            v = np.array([float.fromhex(t) for t in w[2:]])
            r2, r0 = v[:mech.R], v[mech.R:2*mech.R]
            assert np.all(np.isfinite(v))
            live = r0 != 0.0
            err = np.max(np.abs(r2 - r0)[live]/np.abs(r0)[live]) if live.any() else 0.0
            print("%s %s composition %d: cached vs full %.2e" % (name, tag, k, err))
            assert err <= 5e-15, (tag, k)
            assert np.all(r2[~live] == 0.0)
            if extra:
                assert v[-1] == pytest.approx(1.0/1234.5, rel=1e-15) and v[-2] == pytest.approx(1.0/1234.5, rel=1e-15)
            vals.append(r0)
        results[tag] = np.array(vals)
    # the folded function returns FM times the plain rates
    den = np.abs(results["plain"])
    den[den == 0.0] = 1.0
    assert np.max(np.abs(results["fold"] - fm*results["plain"])/(fm*den)) < 1e-14
    assert np.max(np.abs(results["fold, FM at run time"] - fm*results["plain"])/(fm*den)) < 1e-14
    assert np.max(np.abs(results["fold off"] - results["plain"])/den) < 1e-14


@pytest.mark.parametrize("name", ["dme_nb", "dme_script", "syn12", "ch4_arrhenius"])
def test_node_function_with_a_cache_on_the_host(name, template, tmp_path):
    """rmt_node_post as the caching steppers call it (scaled rates, one fma for the species balances, the gain from the
    rate laws' division group) against the same function without a cache, node by node on the golden states: in full and
    from a cache whose reference point lies 0.05 K below; and against the unit with the switches off."""
    zNo = 20
    mi = MECHS[name]()
    mech = plan.Mechanism(mi)
    V, S = mech.V, mech.S
    named, row = plan.member_constants(mi, mech, zNo)
    base = _caching_defines(mech, row, zNo)
    Y, _ = _states_and_reference(name, mi, mech, zNo)
    yc = Y[0].reshape(V, zNo).copy()
    yc[[mech.compList.index(s) for s in ("H2O", "CH3OH", "DME")] if name.startswith("dme") else list(range(S - 3, S))] = 0.0
    states = [y.reshape(V, zNo) for y in Y] + [yc]                       # the last one: three species at the clamp
    F = plan.MEMBER_FIELDS
    inlet = np.concatenate([row[F["CIN"]:F["CIN"] + S], [row[F["THETA_IN"]]]])
    full = np.zeros(RMT_NM(mech))
    full[:len(row)] = row
    recs = ["M " + " ".join(repr(float(v)) for v in full)]
    for y in states:
        for z in range(zNo):
            up = inlet if z == 0 else np.concatenate([np.maximum(y[:S, z - 1], 1e-30), [y[S, z - 1]]])
            yr = y[:, z].copy()
            yr[S] -= 0.05/row[F["TF"]]
            recs.append("N %r %s" % (float(row[F["P0"]])*(1.0 - 1e-3*z),
                                     " ".join(repr(float(v)) for v in np.concatenate([up, yr, y[:, z]]))))
    out = {}
    for tag, defs in (("new", dict(base)), ("off", dict(base, **OFF2))):
        src = mech.source(template, block=64, npt=1, defines=defs)
        exe = _build_kcache_program(str(tmp_path), src, "rmt_kinetics", 0)
        lines = subprocess.run([exe], input="\n".join(recs) + "\n", capture_output=True, text=True,
                               check=True).stdout.strip().split("\n")
        assert len(lines) == len(states)*zNo
        vals = np.array([[float.fromhex(t) for t in ln.split()] for ln in lines])
        assert np.all(vals[:, 0] == 1) and np.all(vals[:, 1] == 0)      # every node in range, no flag
        assert np.all(np.isfinite(vals))
        out[tag] = vals[:, 2:].reshape(len(states), zNo, 3, V).transpose(0, 2, 3, 1)     # [state][plain, full, cached][V][zNo]
    for k in range(len(states)):
        plain, fullk, cached = out["new"][k]
        e_full, e_cached = rowwise_err(fullk, plain, V), rowwise_err(cached, plain, V)
        e_off = rowwise_err(plain, out["off"][k][0], V)
        e_off_c = rowwise_err(cached, out["off"][k][2], V)
        print("%s state %d: with a cache in full vs without %.2e, from the cache vs without %.2e; without a cache vs "
              "switches off %.2e, from the cache vs switches off %.2e" % (name, k, e_full, e_cached, e_off, e_off_c))
        assert e_full < 1e-13 and e_cached < 1e-13 and e_off < 1e-13 and e_off_c < 1e-13, k


def RMT_NM(mech):
    """doubles per member row as the kernels index it (00_config_math.inc, no forcing tail)"""
    return plan.MEMBER_FIXED + mech.S + mech.NU


# ------------------------------------------------------------------ the bench code object
def test_bench_code_object_with_the_new_cuts():
    """device_source(dme, 256 x the notebook's row, 1024) at 512 x 2: no scratch in the step loop, the register and LDS
    budgets untouched, and the counts of profiles/node_cuts.md with a few instructions of slack.  Measured: 3338 VALU,
    2758 fp64, 17 v_rcp_f64 from the hipRTC bundled with PyTorch (the one the suite and every GPU run load), 3305 / 2729 /
    16 from the system's; before the cuts 3462 / 2907 / 30 from both.  The bound is the larger of the two."""
    dme = plan.Mechanism(INP.dme_notebook_input())
    _, row = plan.member_constants(INP.dme_notebook_input(), dme, 1024)
    block, npt, defs, src, key = n2.device_source(dme, np.tile(row, (256, 1)), 1024)
    assert (block, npt) == (512, 2) and defs.get("RMT_KCACHE") == "1" and not set(OFF2) & set(defs)
    assert "#define RMT_KC_SLOTS 12\n" in src and "kc_dp3" in src and "kc_dm3" in src
    assert all(("#define %s 1\n" % m) in src for m in ("RMT_KIN_NODE", "RMT_KIN_RATES_FM", "RMT_KIN_GAIN_DEN",
                                                       "RMT_KIN_XP_INVARIANT"))
    blob = hipbind.compile_cached(src, key, "gfx950", n2.compile_options(block, npt, (), "", defs))
    st = isa.kernel_stats(blob, "rmt_n2_rk4_reg")["step_loop"]
    res = isa.kernel_resources(blob, "rmt_n2_rk4_reg")
    print("step loop:", st, "resources:", res)
    assert st["scratch"] == 0
    assert res["vgpr_count"] <= 256
    assert res["group_segment_fixed_size"] == 161072
    assert st["rcp_f64"] <= 17 < 30
    assert st["valu"] <= 3338 + 10 < 3462
    assert st["valu_f64"] <= 2758 + 10 < 2907
