"""solver-config "schedule" with "inlet-concentration" (time-varying feed composition of model N2), everything that needs no
GPU: parsing and validation, the member rows with their S-wider tail, the golden G14 RHS probes through the oracle and
through the host build of the generated source, the affinity of the right-hand side in the inlet composition under the
member's own scaling, the gfx950 cross-compile of the RMT_FORCING 2 kernels, and the launch walk on the emulated device."""
import copy
import json
import os

import numpy as np
import pytest

import emu_device
import inputs as INP
from oracle import n2_oracle as O
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, isa, launches, n2, plan, rmtExe, schedule
from rmt_app_amd.ensemble import expand_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
KEY = "inlet-concentration"

FEED = [574.8978, 287.4489, 0.0115, 287.4489, 0.0115, 0.0115]
NEW = [574.8978, 250.0, 0.0115, 324.8978, 0.0115, 0.0115]
# hold, ramp over (0.1, 0.2), jump back at 0.3, hold
SPEC = {"time": [0.0, 0.1, 0.2, 0.3, 0.3, 0.4], KEY: [FEED, FEED, NEW, NEW, FEED, FEED]}
S = 6


def rowwise_err(a, b, V):
    a = np.asarray(a, float).reshape(V, -1)
    b = np.asarray(b, float).reshape(V, -1)
    return np.max(np.max(np.abs(a - b), axis=1)/np.maximum(np.max(np.abs(b), axis=1), 1e-300))


def with_schedule(spec, ivp="hip-rk4", **kw):
    mi = INP.dme_notebook_input(ivp=ivp, **kw)
    mi["solver-config"]["schedule"] = copy.deepcopy(spec)
    return mi


@pytest.fixture(scope="module")
def g14():
    with open(os.path.join(G, "g14_feed.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dme():
    mi = INP.dme_notebook_input()
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, 20)
    return mi, mech, named, row


# ----------------------------------------------------------------------------- parsing and semantics
def test_shapes_and_piecewise_linear_composition():
    s = schedule.parse(with_schedule(SPEC))
    assert s.E == 1 and s.conc.shape == (1, S, 6) and s.tail == schedule.TAIL + S == 10 and schedule.TAIL == 4
    assert s.values.shape == (1, 3, 6) and s.given == (False, False, False)        # the three scalars: untouched
    assert s.at(0.15).shape == (1, 3)
    np.testing.assert_array_equal(s.at(0.15)[0], [523.0, 5e6, 523.0])
    v0, sl = s.launch(0.1, 0.2)
    assert v0.shape == sl.shape == (1, 3) and not sl.any()
    np.testing.assert_allclose(s.conc_at(0.05)[0], FEED, rtol=0)                   # hold
    np.testing.assert_allclose(s.conc_at(0.15)[0], 0.5*(np.array(FEED) + np.array(NEW)), rtol=1e-15)      # half way
    np.testing.assert_allclose(s.conc_at(0.25)[0], NEW, rtol=0)
    np.testing.assert_allclose(s.conc_at(0.3, "left")[0], NEW, rtol=0)             # the left value holds up to the jump
    np.testing.assert_allclose(s.conc_at(0.3)[0], FEED, rtol=0)                    # the right value from it on
    np.testing.assert_allclose(s.conc_at(9.0)[0], FEED, rtol=0)                    # after the last breakpoint: held
    c0, cs = s.conc_launch(0.1, 0.2)
    assert c0.shape == cs.shape == (1, S)
    np.testing.assert_allclose(c0[0], FEED, rtol=0)
    np.testing.assert_allclose(cs[0], (np.array(NEW) - np.array(FEED))/0.1, rtol=1e-13)
    c0, cs = s.conc_launch(0.3, 0.4)               # starts AT the jump: the right values, nothing moves
    np.testing.assert_allclose(c0[0], FEED, rtol=0)
    assert not cs.any()
    # inside one launch the composition is ONE linear function of t
    for a, c in [l[:2] for l in launches.merge(0.4, 2, s.times)[0]]:
        c0, cs = s.conc_launch(a, c)
        for t in np.linspace(a, c, 5)[:-1]:
            np.testing.assert_allclose(c0 + cs*(t - a), s.conc_at(t), rtol=1e-13)
        np.testing.assert_allclose(c0 + cs*(c - a), s.conc_at(c, "left"), rtol=1e-13)
    assert [l.out for l in launches.merge(0.4, 2, s.times)[0]] == [None, 1, None, 2]           # 0.1 | 0.2 | 0.3 | 0.4


def test_without_the_key_nothing_is_added():
    spec = {"time": [0.0, 0.1, 0.2], "inlet-temperature": [523.0, 523.0, 533.0]}
    s = schedule.parse(with_schedule(spec))
    assert s.conc is None and s.conc_at(0.1) is None and s.conc_launch(0.0, 0.1) is None and s.tail == schedule.TAIL
    assert s.given == (True, False, False) and len(s.given) == 3 and s.at(0.1).shape == (1, 3)
    assert s.forcing_level == "1"
    s2 = schedule.parse(with_schedule(dict(spec, **{KEY: [FEED, FEED, NEW]})))
    assert s2.given == (True, False, False) and len(s2.given) == 3 and s2.at(0.1).shape == (1, 3)
    assert s2.values.shape == (1, 3, 3) and s2.forcing_level == "2"
    np.testing.assert_array_equal(s2.values, s.values)
    v, sl = s2.launch(0.1, 0.2)
    assert v.shape == (1, 3) and sl.shape == (1, 3)


def test_relative_on_a_sweep_and_list_form():
    off = [0.0, -30.0, 0.0, 30.0, 0.0, 0.0]
    base = with_schedule({"time": [0, 0.2, 0.2, 0.4], KEY: [[0.0]*S, [0.0]*S, off, off], "relative": True})
    members = expand_members(base, {"temperature": [513.0, 533.0], "pressure": [4.0e6, 5.0e6]})
    s = schedule.parse(base, members)
    assert s.E == 4 and s.relative and s.conc.shape == (4, S, 4)
    feeds = np.array([mi["feed"]["concentration"] for mi in members], dtype=float)
    assert len({tuple(f) for f in feeds}) == 4                                     # the members have different feeds
    np.testing.assert_allclose(s.conc_at(0.1), feeds, rtol=0)
    np.testing.assert_allclose(s.conc_at(0.3), feeds + np.array(off), rtol=1e-15)
    sub = s.members(1, 3)
    assert sub.E == 2 and sub.conc.shape == (2, S, 4) and sub.tail == 10
    np.testing.assert_array_equal(sub.conc_at(0.3), s.conc_at(0.3)[1:3])
    np.testing.assert_array_equal(sub.at(0.3), s.at(0.3)[1:3])
    # list form: a member carries its own rows; a member WITHOUT the key keeps its own feed
    base = with_schedule({"time": [0, 0.1, 0.3], "inlet-temperature": [523, 523, 533]})
    members = expand_members(base, [{}, {"solver-config": {"schedule": {KEY: [FEED, FEED, NEW]}}},
                                    {"feed": {"concentration": [500.0, 300.0, 0.02, 200.0, 0.02, 0.02]}}])
    s = schedule.parse(base, members)
    assert s.conc.shape == (3, S, 3)
    np.testing.assert_allclose(s.conc_at(0.3), [FEED, NEW, [500.0, 300.0, 0.02, 200.0, 0.02, 0.02]], rtol=0)
    np.testing.assert_allclose(s.at(0.3)[:, 0], [533, 533, 533])


# ----------------------------------------------------------------------------- member rows
def test_rows_at_changes_only_the_inlet_composition(dme):
    mi, mech, named, row = dme
    F = plan.MEMBER_FIELDS
    cin = list(range(F["CIN"], F["CIN"] + S))
    s = schedule.parse(with_schedule(SPEC))
    r = s.rows_at([row], [named], 0.15)
    assert r.shape == (1, mech.row_width)
    np.testing.assert_allclose(r[0, cin], 0.5*(np.array(FEED) + np.array(NEW))/574.8978, rtol=1e-15)
    other = [i for i in range(mech.row_width) if i not in cin]
    np.testing.assert_array_equal(r[0, other], row[other])                  # CMAX and every scaling constant: the member's own
    np.testing.assert_array_equal(s.rows_at([row], [named], 0.0)[0], row)   # t = 0 of this schedule: the member itself
    # together with a scheduled inlet temperature: CIN and THETA_IN, nothing else
    s = schedule.parse(with_schedule(dict(SPEC, **{"inlet-temperature": [523, 523, 533, 533, 533, 533]})))
    r = s.rows_at([row], [named], 0.25)
    assert r[0, F["THETA_IN"]] == (533.0 - 523.0)/523.0
    np.testing.assert_allclose(r[0, cin], np.array(NEW)/574.8978, rtol=1e-15)
    other = [i for i in range(mech.row_width) if i not in cin + [F["THETA_IN"]]]
    np.testing.assert_array_equal(r[0, other], row[other])


def test_forced_rows_carry_the_wider_tail(dme):
    mi, mech, named, row = dme
    F = plan.MEMBER_FIELDS
    cin = list(range(F["CIN"], F["CIN"] + S))
    s = schedule.parse(with_schedule(dict(SPEC, **{"inlet-temperature": [523, 523, 533, 533, 533, 533]})))
    w = s.forced_rows([row], [named], 0.1, 0.2)
    assert w.shape == (1, mech.row_width + 4 + S)
    np.testing.assert_allclose(w[0, cin], np.array(FEED)/574.8978, rtol=0)           # the values at t_ref
    want = [0.1, 100.0/523.0, 0.0, 0.0] + list((np.array(NEW) - np.array(FEED))/0.1/574.8978)
    np.testing.assert_allclose(w[0, mech.row_width:], want, rtol=1e-13)
    other = [i for i in range(mech.row_width) if i not in cin + [F["THETA_IN"]]]
    np.testing.assert_array_equal(w[0, other], row[other])
    w = s.forced_rows([row], [named], 0.2, 0.3)                                      # a hold: every slope zero
    np.testing.assert_allclose(w[0, cin], np.array(NEW)/574.8978, rtol=1e-15)
    assert w[0, mech.row_width] == 0.2 and not w[0, mech.row_width + 1:].any()
    np.testing.assert_array_equal(plan.forced_composition_slopes([named], [[574.8978, 0, 0, 0, 0, 0]]), [[1, 0, 0, 0, 0, 0]])


def test_rows_without_the_key_are_what_they_were(dme):
    """Without the key: width row_width + schedule.TAIL, and bit for bit the rows of the three-quantity schedule - restated
    here from the member row, the feed temperature and the piecewise-linear functions."""
    mi, mech, named, row = dme
    F = plan.MEMBER_FIELDS
    spec = {"time": [0.0, 0.10, 0.20, 0.20, 0.5], "inlet-temperature": [523, 523, 533, 528, 528],
            "inlet-pressure": [5e6, 5e6, 5e6, 4.9e6, 4.9e6], "medium-temperature": [523, 523, 523, 533, 533]}
    s = schedule.parse(with_schedule(spec))
    for t0, t1, T, P, Tm, sT, sP, sTm in ((0.0, 0.1, 523.0, 5e6, 523.0, 0.0, 0.0, 0.0),
                                          (0.1, 0.2, 523.0, 5e6, 523.0, (533.0 - 523.0)/(0.2 - 0.1), 0.0, 0.0),
                                          (0.2, 0.5, 528.0, 4.9e6, 533.0, 0.0, 0.0, 0.0)):
        w = s.forced_rows([row], [named], t0, t1)
        assert w.shape == (1, mech.row_width + schedule.TAIL)
        want = np.concatenate([row, [t0, sT/523.0, sP, sTm]])
        want[F["THETA_IN"]], want[F["P0"]], want[F["TM"]] = (T - 523.0)/523.0, P, Tm
        assert w[0].tobytes() == want.tobytes(), (t0, t1)


# ----------------------------------------------------------------------------- errors
NEG = [574.8978, -1.0, 0.0115, 287.4489, 0.0115, 0.0115]
BAD = [
    {"time": [0, 0.2], KEY: [FEED]},                                   # wrong row count
    {"time": [0, 0.2], KEY: [FEED, FEED, FEED]},
    {"time": [0, 0.2], KEY: [FEED, FEED[:5]]},                         # ragged
    {"time": [0, 0.2], KEY: [FEED[:5], FEED[:5]]},                     # wrong row width
    {"time": [0, 0.2], KEY: FEED},                                     # not a list of rows
    {"time": [0, 0.2], KEY: [FEED, NEG]},                              # negative
    {"time": [0, 0.2], KEY: [FEED, [0.0]*S]},                          # nothing positive in a row
    {"time": [0, 0.2], KEY: [FEED, [float("nan")] + FEED[1:]]},        # not finite
    {"time": [0, 0.2], KEY: [FEED, [float("inf")] + FEED[1:]]},
    {"time": [0, 0.2], KEY: [[0.0]*S, [0.0, -300.0, 0, 0, 0, 0]], "relative": True},      # negative after the offset
    {"time": [0, 0.2], KEY: [[0.0]*S, [-x for x in FEED]], "relative": True},             # all zero after the offset
]


@pytest.mark.parametrize("spec", BAD)
def test_value_errors_name_the_key(spec):
    mi = with_schedule(spec)
    with pytest.raises(ValueError, match=KEY):
        schedule.parse(mi, None, n2.resolve_ivp(mi["solver-config"]["ivp"]))
    with pytest.raises(ValueError, match=KEY):        # ... and through the public entry point, before any device work
        rmtExe(mi)


def test_value_errors_name_the_member():
    base = with_schedule({"time": [0, 0.2], "inlet-temperature": [523, 530]})
    members = expand_members(base, [{}, {"solver-config": {"schedule": {KEY: [FEED, NEG]}}}])
    with pytest.raises(ValueError, match=KEY + ".*member 1"):
        schedule.parse(base, members)
    with pytest.raises(ValueError, match=KEY + ".*member 0"):
        schedule.parse(with_schedule({"time": [0, 0.2], KEY: [FEED, NEG]}))


def test_isothermal_runs_may_schedule_the_composition():
    mi = with_schedule({"time": [0, 0.2], KEY: [FEED, NEW]}, process_type="iso-thermal")
    s = schedule.parse(mi)
    assert s.conc.shape == (1, S, 2) and s.given == (False, False, False)


def test_result_entry_only_with_the_key():
    s = schedule.parse(with_schedule(SPEC))
    r = schedule.result_entry(s, [0.2, 0.4])
    assert r[KEY].shape == (2, S)
    np.testing.assert_allclose(r[KEY], [NEW, FEED], rtol=0)
    assert r["inlet-temperature"].tolist() == [523.0, 523.0]
    s = schedule.parse(with_schedule({"time": [0, 0.2], "inlet-pressure": [5e6, 4.9e6]}))
    assert KEY not in schedule.result_entry(s, [0.2, 0.4])


# ----------------------------------------------------------------------------- golden G14: RHS probes
def test_g14_probes_vs_oracle():
    """The reference's own modelEquationN2 with only constBC1['SpCoi0'] replaced (one probe set also constBC1['T0']; G14)
    against the oracle with the same overrides: the bound of test_g13_probes_vs_oracle."""
    g = np.load(os.path.join(G, "g14_feed_probes.npz"))
    pr = O.setup_n2(INP.dme_notebook_input(), 20)
    assert g["f"].shape == (len(g["conc"]), 6, 140) and len(g["conc"]) >= 5
    for k, (c, (T0, P0, Tm)) in enumerate(zip(g["conc"], g["forced"])):
        assert np.max(c) == 574.8978                              # the reference's scaling does not move
        fv = O.make_rhs_vec(dict(pr, SpCoi0=np.array(c), T0=float(T0), P0=float(P0), Tm=float(Tm)))
        for j, y in enumerate(g["y"]):
            e = rowwise_err(fv(0.0, y), g["f"][k, j], pr["varNo"])
            assert e < 2e-13, (k, j, e)
    assert len({tuple(v) for v in g["conc"]}) >= 4                # before, inside (twice) and after the ramp / the step
    assert any(T0 != 523.0 for T0, _, _ in g["forced"])           # one of them combined with a forced T0
    assert np.max(np.abs(g["f"][0] - g["f"][3])) > 1e-3           # the probes see the composition


def test_g14_probes_vs_host_build_of_rows_at(g14, dme):
    """schedule.rows_at(t) through the host build of the generated source: the bound of the G13 counterpart."""
    g = np.load(os.path.join(G, "g14_feed_probes.npz"))
    mi, mech, named, row = dme
    emu = HostEmu(mech.source(hipbind.kernel_template()), tag="dme_nb")
    Y = g["y"]
    for k, (case, t) in enumerate(zip(g["case"], g["times"])):
        s = schedule.parse(with_schedule(g14["cases"][str(case)]["schedule"]))
        np.testing.assert_allclose(s.conc_at(float(t))[0], g["conc"][k], rtol=1e-15)
        np.testing.assert_allclose(s.at(float(t))[0], g["forced"][k], rtol=1e-15)
        rows = s.rows_at([row], [named], float(t))
        out, flags = emu.rhs(Y, np.tile(rows[0], (len(Y), 1)), 20)
        for j in range(len(Y)):
            e = rowwise_err(out[j], g["f"][k, j], mech.V)
            assert e < 1e-11, (k, j, e)


def test_rhs_is_affine_in_the_inlet_composition_under_the_members_own_scaling(dme):
    """A disturbance d that RAISES the largest concentration (H2 above 574.8978, where the reference - which rescales by
    the new maximum - has no counterpart): the scaling stays the member's own exactly when the right-hand side of the host
    build is affine in the inlet composition, f(c0 + 2d) - f(c0) = 2 (f(c0 + d) - f(c0)); row-relative <= 1e-12."""
    mi, mech, named, row = dme
    # (every species d moves, it moves by a few percent of Cmax: the differences below are then of the size of f itself
    # and carry its rounding, ~1e-16 relative - a d_i of 1e-3 would leave a difference 1e5 times smaller than the f it is
    # taken from and a floor of 1e-11 that says nothing about affinity)
    d = np.array([60.0, 20.0, 0.0, -30.0, 15.0, 0.0])
    c0 = np.array(FEED)
    s = schedule.parse(with_schedule({"time": [0.0, 1.0, 2.0], KEY: [list(c0), list(c0 + d), list(c0 + 2*d)]}))
    assert np.max(c0 + d) > 574.8978
    F = plan.MEMBER_FIELDS
    r1 = s.rows_at([row], [named], 1.0)[0]
    assert r1[F["CMAX"]] == 574.8978 and r1[F["CIN"]] > 1.0 and r1[F["INV_MACOTE"]] == row[F["INV_MACOTE"]]
    emu = HostEmu(mech.source(hipbind.kernel_template()), tag="dme_nb")
    Y = np.load(os.path.join(G, "g14_feed_probes.npz"))["y"]
    f = [emu.rhs(Y, np.tile(s.rows_at([row], [named], t)[0], (len(Y), 1)), 20)[0] for t in (0.0, 1.0, 2.0)]
    for j in range(len(Y)):
        two = (f[2][j] - f[0][j]).reshape(mech.V, -1)
        one = 2.0*(f[1][j] - f[0][j]).reshape(mech.V, -1)
        assert np.max(np.abs(one[:S, 0])) > 1e-2                  # the disturbance is seen at node 0 ...
        assert not one[:, 1:].any() and not two[:, 1:].any()      # ... and only there (upwind difference)
        for i in range(mech.V):
            if not one[i].any():                                  # a species d leaves alone, and the temperature row
                assert not two[i].any(), (j, i)
                continue
            e = np.max(np.abs(two[i] - one[i]))/np.max(np.abs(one[i]))
            assert e <= 1e-12, (j, i, e)


# ----------------------------------------------------------------------------- generated source, gfx950 cross-compile
FORCED2_KERNELS = [
    ("rk4", 64, 1, {}, ("rmt_n2_rk4_reg", "rmt_n2_rk4_mem")),
    ("rk45", 64, 1, {"RMT_RK45_LDS": "2"}, ("rmt_n2_rk45_reg", "rmt_n2_rk45_mem")),
    ("ros4", 64, 1, {"RMT_WITH_ROS4": "1"}, ("rmt_n2_ros4_mem",)),
]


@pytest.mark.parametrize("name,block,npt,defs,kernels", FORCED2_KERNELS)
def test_forcing_2_kernels_cross_compile(name, block, npt, defs, kernels):
    """RMT_FORCING 2: every kernel that must carry the composition compiles for gfx950 (hipRTC, no GPU), with the member
    row of 16 + S + NU + 4 + S doubles."""
    mech = plan.Mechanism(INP.dme_notebook_input())
    tpl = hipbind.kernel_template()
    d = dict(defs, RMT_FORCING="2")
    src = mech.source(tpl, False, block, npt, None, d)
    blob, _ = hipbind.compile_source(
        src + '\nstatic_assert(RMT_NM == 16 + RMT_S + RMT_NU + 4 + RMT_S && RMT_FORCING == 2, "member row");\n')
    for k in kernels:
        res = isa.kernel_resources(blob, k)
        print(k, "RMT_FORCING 2", res)
        assert res["vgpr_count"] > 0
    assert b"rmt_n2_ros4_chain" not in blob          # a forced reactor stays on one workgroup


def test_a_composition_literal_is_refused_under_forcing_2():
    mech = plan.Mechanism(INP.dme_notebook_input())
    tpl = hipbind.kernel_template()
    lit = "{" + ", ".join(repr(v/574.8978) for v in FEED) + "}"
    hipbind.compile_source(mech.source(tpl, False, 64, 1, None, {"RMT_FORCING": "1", "RMT_MC_CIN": lit}))      # value 1 may
    with pytest.raises(hipbind.RmtN2Error, match="RMT_MC_CIN"):
        hipbind.compile_source(mech.source(tpl, False, 64, 1, None, {"RMT_FORCING": "2", "RMT_MC_CIN": lit}))
    with pytest.raises(hipbind.RmtN2Error, match="RMT_FORCING"):
        hipbind.compile_source(mech.source(tpl, False, 64, 1, None, {"RMT_FORCING": "2", "RMT_MC_TM": "523.0"}))


def test_forcing_defines_are_the_only_difference_of_the_sources():
    mech = plan.Mechanism(INP.dme_notebook_input())
    tpl = hipbind.kernel_template()
    src = mech.source(tpl, False, 64, 1)
    assert mech.source(tpl, False, 64, 1, None, {"RMT_FORCING": "1"}).replace("#define RMT_FORCING 1\n", "") == src
    assert mech.source(tpl, False, 64, 1, None, {"RMT_FORCING": "2"}).replace("#define RMT_FORCING 2\n", "") == src


def test_forced_literals_and_levels():
    lits = {"RMT_MC_UA": "1.0", "RMT_MC_P0": "5e6", "RMT_MC_TM": "523.0", "RMT_MC_THETA_IN": "0.0", "RMT_MC_CIN": "{1.0}"}
    assert set(n2.forced_literals(lits)) == {"RMT_MC_UA", "RMT_MC_CIN"}               # value 1: as before
    assert set(n2.forced_literals(lits, "1")) == {"RMT_MC_UA", "RMT_MC_CIN"}
    assert set(n2.forced_literals(lits, "2")) == {"RMT_MC_UA"}
    assert n2.is_forced({"RMT_FORCING": "1"}) and n2.is_forced({"RMT_FORCING": "2"})
    assert not n2.is_forced({}) and not n2.is_forced({"RMT_FORCING": "0"}) and not n2.is_forced(None)
    # a sweep with ONE feed composition: CIN is uniform, a literal for value 1, withheld for value 2
    base = INP.dme_notebook_input()
    members = expand_members(base, [{}, {"external-heat": {"OvHeTrCo": 60.0}}])
    mech = plan.Mechanism(base)
    rows = np.array([plan.member_constants(mi, mech, 20)[1] for mi in members])
    assert rows[0, plan.MEMBER_FIELDS["UA"]] != rows[1, plan.MEMBER_FIELDS["UA"]]
    for level, tail in (("1", 4), ("2", 4 + S)):
        wide = np.concatenate([rows, np.zeros((2, tail))], axis=1)
        _, _, defs, _, _ = n2.device_source(mech, wide, 20, defines={"RMT_FORCING": level})
        assert "RMT_MC_F1" in defs and "RMT_MC_UA" not in defs and "RMT_MC_P0" not in defs
        assert ("RMT_MC_CIN" in defs) == (level == "1")


# ----------------------------------------------------------------------------- the launch walk on the emulated device
class WalkEmu(emu_device.EmuDevice):
    """The host-emulation stand-in as a forced device: it records the rows every launch runs with, and integrates each
    launch with the rows' values at the launch start (the host build has no forcing; what is under test is the walk)."""
    LOG = []
    block, npt = 64, 1

    def __init__(self, mech, members, N, **kw):
        members = np.ascontiguousarray(members, dtype=np.float64).reshape(-1, np.shape(members)[-1])
        self.forced_defines = dict(kw.get("defines") or {})
        self.rows = members
        kw["defines"] = {k: v for k, v in self.forced_defines.items() if k != "RMT_FORCING"}
        kw["specialize"] = False
        super().__init__(mech, members[:, :mech.row_width], N, **kw)

    def set_mode(self, mode):
        self.mode = mode

    def last_geometry(self):
        return (1, self.E)

    def set_members(self, rows):
        self.rows = np.array(rows, dtype=np.float64).reshape(self.E, -1)
        self.members = np.ascontiguousarray(self.rows[:, :self.mech.row_width])

    def rk4(self, y, dt, nsteps, t0=0.0):
        WalkEmu.LOG.append((float(t0), float(dt)*int(nsteps), self.rows.copy(), self.forced_defines.get("RMT_FORCING")))
        super().rk4(y, dt, nsteps, t0)


def _walk(spec):
    mi = with_schedule(spec, period=4e-4)
    mi["solver-config"].update({"quiet": True, "dt": 4e-6, "zNo": 20, "tNo": 2, "display-result": "False"})
    del WalkEmu.LOG[:]
    real, n2.N2Device = n2.N2Device, WalkEmu
    try:
        res = rmtExe(mi)["resModel"]
    finally:
        n2.N2Device = real
    return res, list(WalkEmu.LOG)


def test_launch_walk_refreshes_the_composition_before_every_launch(dme):
    mi, mech, named, row = dme
    T = [0.0, 1e-4, 2e-4, 3e-4, 3e-4, 4e-4]
    temp = {"time": T, "inlet-temperature": [523, 523, 533, 533, 533, 533]}
    res0, log0 = _walk(temp)
    res2, log2 = _walk(dict(temp, **{KEY: SPEC[KEY]}))
    assert [(a, round(b, 15)) for a, b, _, _ in log2] == [(a, round(b, 15)) for a, b, _, _ in log0]      # the same launch list
    assert len(log2) == 4 and [lv for _, _, _, lv in log2] == ["2"]*4 and [lv for _, _, _, lv in log0] == ["1"]*4
    W = mech.row_width
    cin = slice(plan.MEMBER_FIELDS["CIN"], plan.MEMBER_FIELDS["CIN"] + S)
    s = schedule.parse(with_schedule(dict(temp, **{KEY: SPEC[KEY]})))
    for (t0, span, rows, _), (_, _, rows0, _) in zip(log2, log0):
        assert rows.shape == (1, W + 4 + S) and rows0.shape == (1, W + 4)
        c0, cs = s.conc_launch(t0, t0 + span)
        np.testing.assert_array_equal(rows[0, cin], c0[0]/574.8978)                  # CIN at the launch start ...
        np.testing.assert_array_equal(rows[0, W + 4:], cs[0]/574.8978)               # ... and the S slopes
        np.testing.assert_array_equal(rows[0, W:W + 4], rows0[0, W:W + 4])           # t_ref and the three slopes: as without
        keep = np.ones(W, dtype=bool)
        keep[cin] = False
        np.testing.assert_array_equal(rows[0, :W][keep], rows0[0, :W][keep])
    assert [bool(r[0, W + 4:].any()) for _, _, r, _ in log2] == [False, True, False, False]
    assert len(res2["dataPack"]) == 2                                                # breakpoints add no entries
    np.testing.assert_allclose(res2["schedule"][KEY], [NEW, FEED], rtol=0)
    assert KEY not in res0["schedule"]
