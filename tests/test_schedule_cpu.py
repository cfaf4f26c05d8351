"""solver-config "schedule" (time-varying inlet and coolant conditions of model N2), everything that needs no GPU:
parsing and validation, launch boundaries, the forced member rows, the golden G13 RHS probes through the oracle and
through the host build of the generated source, the order of the non-autonomous RODAS4 step, and the gfx950
cross-compile of the forced kernels."""
import copy
import json
import os

import numpy as np
import pytest

import inputs as INP
from oracle import n2_oracle as O
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, isa, launches, n2, plan, rmtExe, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

STEP = {"time": [0.0, 0.10, 0.20, 0.20, 0.5], "inlet-temperature": [523, 523, 533, 528, 528],
        "inlet-pressure": [5e6, 5e6, 5e6, 4.9e6, 4.9e6], "medium-temperature": [523, 523, 523, 533, 533]}


def rowwise_err(a, b, V):
    a = np.asarray(a, float).reshape(V, -1)
    b = np.asarray(b, float).reshape(V, -1)
    return np.max(np.max(np.abs(a - b), axis=1)/np.maximum(np.max(np.abs(b), axis=1), 1e-300))


def with_schedule(spec, ivp="hip-rk4", **kw):
    mi = INP.dme_notebook_input(ivp=ivp, **kw)
    mi["solver-config"]["schedule"] = copy.deepcopy(spec)
    return mi


@pytest.fixture(scope="module")
def g13():
    with open(os.path.join(G, "g13_schedule.json")) as f:
        return json.load(f)


# ----------------------------------------------------------------------------- parsing and semantics
def test_absent_schedule_is_none():
    assert schedule.parse(INP.dme_notebook_input()) is None


def test_piecewise_linear_jumps_and_holds():
    s = schedule.parse(with_schedule(STEP))
    assert s.E == 1 and s.given == (True, True, True) and not s.relative
    np.testing.assert_allclose(s.at(0.05)[0], [523, 5e6, 523])
    np.testing.assert_allclose(s.at(0.15)[0], [528, 5e6, 523])                  # half way up the ramp
    np.testing.assert_allclose(s.at(0.2, "left")[0], [533, 5e6, 523])           # the left value holds up to the jump
    np.testing.assert_allclose(s.at(0.2)[0], [528, 4.9e6, 533])                 # the right value from it on
    np.testing.assert_allclose(s.at(0.35)[0], [528, 4.9e6, 533])
    np.testing.assert_allclose(s.at(7.0)[0], [528, 4.9e6, 533])                 # after the last breakpoint: held
    # a quantity that is not given stays the member's constant
    s2 = schedule.parse(with_schedule({"time": [0, 0.1], "inlet-pressure": [5e6, 4e6]}))
    assert s2.given == (False, True, False)
    np.testing.assert_allclose(s2.at(0.05)[0], [523, 4.5e6, 523])


def test_launch_boundaries_and_pieces():
    s = schedule.parse(with_schedule(STEP))
    b = launches.merge(0.5, 2, s.times)[0]    # outputs 0.25, 0.5; breakpoints 0.1, 0.2 inside
    assert [(round(l.t0, 12), round(l.t1, 12), l.out) for l in b] == [
        (0.0, 0.1, None), (0.1, 0.2, None), (0.2, 0.25, 1), (0.25, 0.5, 2)]
    # a breakpoint ON an output time adds no launch, whatever linspace rounds it to
    b = launches.merge(0.3, 6, s.times)[0]
    assert len(b) == 6 and [l.out for l in b] == [1, 2, 3, 4, 5, 6]
    v0, sl = s.launch(0.1, 0.2)
    np.testing.assert_allclose(v0[0], [523, 5e6, 523])
    np.testing.assert_allclose(sl[0], [100.0, 0.0, 0.0])
    v0, sl = s.launch(0.2, 0.25)              # starts AT the jump: the right values, nothing moves
    np.testing.assert_allclose(v0[0], [528, 4.9e6, 533])
    assert not sl.any()
    v0, sl = s.launch(0.5, 0.7)               # beyond the last breakpoint
    np.testing.assert_allclose(v0[0], [528, 4.9e6, 533])
    assert not sl.any()
    # inside one launch the forcing is ONE linear function: start value + slope (t - t0) reproduces at()
    for a, c in [l[:2] for l in launches.merge(0.5, 2, s.times)[0]]:
        v0, sl = s.launch(a, c)
        for t in np.linspace(a, c, 5)[:-1]:
            np.testing.assert_allclose(v0 + sl*(t - a), s.at(t), rtol=1e-14)
        np.testing.assert_allclose(v0 + sl*(c - a), s.at(c, "left"), rtol=1e-14)


def test_relative_and_per_member_values():
    from rmt_app_amd.ensemble import expand_members
    base = with_schedule({"time": [0, 0.2, 0.2, 0.4], "inlet-temperature": [0, 0, 5, 5],
                          "inlet-pressure": [0, 0, -1e5, -1e5], "medium-temperature": [0, 0, 10, 10], "relative": True})
    members = expand_members(base, {"temperature": [513.0, 533.0], "pressure": [4.0e6, 5.0e6]})
    s = schedule.parse(base, members)
    assert s.E == 4 and s.relative
    np.testing.assert_allclose(s.at(0.1), [[513, 4e6, 523], [513, 5e6, 523], [533, 4e6, 523], [533, 5e6, 523]])
    np.testing.assert_allclose(s.at(0.3), [[518, 3.9e6, 533], [518, 4.9e6, 533], [538, 3.9e6, 533], [538, 4.9e6, 533]])
    assert s.members(1, 3).E == 2
    np.testing.assert_allclose(s.members(1, 3).at(0.3), s.at(0.3)[1:3])
    # list form: a member carries its own values, the times come from the base input
    base = with_schedule({"time": [0, 0.1, 0.3], "inlet-temperature": [523, 523, 533]})
    members = expand_members(base, [{}, {"solver-config": {"schedule": {"inlet-temperature": [523, 523, 543]}}}])
    s = schedule.parse(base, members)
    np.testing.assert_allclose(s.at(0.3)[:, 0], [533, 543])
    members = expand_members(base, [{}, {"solver-config": {"schedule": {"time": [0, 0.2, 0.3]}}}])
    with pytest.raises(ValueError, match="time"):
        schedule.parse(base, members)


def test_forced_rows_and_rows_at():
    mi = with_schedule(STEP)
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, 20)
    s = schedule.parse(mi)
    F = plan.MEMBER_FIELDS
    r = s.rows_at([row], [named], 0.15)
    assert r.shape == (1, mech.row_width)
    assert r[0, F["THETA_IN"]] == (528.0 - 523.0)/523.0 and r[0, F["P0"]] == 5e6 and r[0, F["TM"]] == 523.0
    untouched = [i for i in range(mech.row_width) if i not in (F["THETA_IN"], F["P0"], F["TM"])]
    np.testing.assert_array_equal(r[0, untouched], row[untouched])          # only the boundary values change
    w = s.forced_rows([row], [named], 0.1, 0.2)
    assert w.shape == (1, mech.row_width + schedule.TAIL)
    np.testing.assert_array_equal(w[0, untouched], row[untouched])
    assert w[0, F["THETA_IN"]] == 0.0 and w[0, F["P0"]] == 5e6 and w[0, F["TM"]] == 523.0
    np.testing.assert_allclose(w[0, mech.row_width:], [0.1, 100.0/523.0, 0.0, 0.0], rtol=1e-15)
    np.testing.assert_array_equal(s.rows_at([row], [named], 0.0)[0], row)   # t = 0 of this schedule: the member itself


BAD = [
    ({"time": [0.1, 0.2], "inlet-temperature": [523, 530]}, {}, "time"),
    ({"time": [0, 0.2, 0.1], "inlet-temperature": [523, 530, 530]}, {}, "time"),
    ({"inlet-temperature": [523, 530]}, {}, "time"),
    ({"time": [0, 0.2], "inlet-temperature": [523, 530, 531]}, {}, "inlet-temperature"),
    ({"time": [0, 0.2], "inlet-pressure": [5e6]}, {}, "inlet-pressure"),
    ({"time": [0, 0.2], "medium-temperature": [523, 530, 531]}, {}, "medium-temperature"),
    ({"time": [0, 0.2], "medium-temperature": [523, 0]}, {}, "medium-temperature"),
    ({"time": [0, 0.2], "medium-temperature": [523, -5]}, {}, "medium-temperature"),
    ({"time": [0, 0.2], "inlet-temperature": [523, -1]}, {}, "inlet-temperature"),
    ({"time": [0, 0.2], "inlet-pressure": [5e6, 0]}, {}, "inlet-pressure"),
    ({"time": [0, 0.2], "inlet-pressure": [0, -6e6], "relative": True}, {}, "inlet-pressure"),
    ({"time": [0, 0.2], "inlet-temperature": [523, 530]}, {"ivp": "AM"}, "ivp"),
    ({"time": [0, 0.2], "inlet-temperature": [523, 530]}, {"ivp": "hip-ab3"}, "ivp"),
    ({"time": [0, 0.2], "inlet-temperature": [523, 530]}, {"dtype": "fp32"}, "dtype"),
    ({"time": [0, 0.2], "inlet-temperture": [523, 530]}, {}, "inlet-temperture"),
]


@pytest.mark.parametrize("spec,cfg,key", BAD)
def test_value_errors_name_the_key(spec, cfg, key):
    mi = with_schedule(spec)
    mi["solver-config"].update(cfg)
    with pytest.raises(ValueError, match=key):
        schedule.parse(mi, None, n2.resolve_ivp(mi["solver-config"]["ivp"]))
    with pytest.raises(ValueError, match=key):        # ... and through the public entry point, before any device work
        rmtExe(mi)


def test_value_errors_adiabatic_isothermal_and_other_models():
    mi = INP.ch4_input(ivp="hip-rk4")                 # MeTe = 0: the reference's adiabatic switch
    mi["solver-config"]["schedule"] = {"time": [0, 1], "medium-temperature": [900, 910]}
    with pytest.raises(ValueError, match="medium-temperature"):
        rmtExe(mi)
    for key in ("inlet-temperature", "medium-temperature"):
        mi = with_schedule({"time": [0, 0.2], key: [523, 530]}, process_type="iso-thermal")
        with pytest.raises(ValueError, match=key):
            rmtExe(mi)
    mi = with_schedule({"time": [0, 0.2], "inlet-pressure": [5e6, 4.9e6]}, process_type="iso-thermal")
    assert schedule.parse(mi).given == (False, True, False)               # stays allowed there
    for fn in (INP.n1_notebook_input, INP.m2_dme_input):
        mi = fn()
        mi["solver-config"]["schedule"] = {"time": [0, 0.2], "inlet-pressure": [5e6, 4.9e6]}
        with pytest.raises(ValueError, match="schedule"):
            rmtExe(mi)


def test_forced_kernel_form_is_chosen_by_the_host():
    assert n2.forced_mode("hip-rk4", 20, 64, 1) == "reg"
    assert n2.forced_mode("hip-rk4", 600, 512, 2) == "reg"
    assert n2.forced_mode("hip-rk4", 4096, 512, 2) == "mem"          # never the chained form
    assert n2.forced_mode("hip-rk45", 600, 512, 2, "mem") == "mem"
    assert n2.forced_mode("hip-ros4", 20, 64, 1) == "mem"
    with pytest.raises(ValueError, match="device-mode"):
        n2.forced_mode("hip-rk4", 600, 512, 2, "chain")
    with pytest.raises(ValueError, match="device-mode"):
        n2.forced_mode("hip-rk4", 4096, 512, 2, "reg")


# ----------------------------------------------------------------------------- golden G13: RHS probes
def test_g13_probes_vs_oracle():
    """The reference's own modelEquationN2 with only constBC1['T0'], constBC1['P0'] and ExHe['MeTe'] replaced (G13)
    against the oracle with the same overrides: the bound of test_oracle_golden.py for the RHS."""
    g = np.load(os.path.join(G, "g13_schedule_probes.npz"))
    pr = O.setup_n2(INP.dme_notebook_input(), 20)
    assert g["f"].shape == (7, 6, 140)
    for k, (T0, P0, Tm) in enumerate(g["forced"]):
        fv = O.make_rhs_vec(dict(pr, T0=float(T0), P0=float(P0), Tm=float(Tm)))
        for j, y in enumerate(g["y"]):
            e = rowwise_err(fv(0.0, y), g["f"][k, j], pr["varNo"])
            assert e < 2e-13, (k, j, e)
    assert len({tuple(v) for v in g["forced"]}) >= 4          # before, inside and after the ramp, and behind the pressure step


def test_g13_probes_vs_host_build_of_rows_at(g13):
    """schedule.rows_at(t) through the host build of the generated source: the project's bound for the host build."""
    g = np.load(os.path.join(G, "g13_schedule_probes.npz"))
    mi = INP.dme_notebook_input()
    mech = plan.Mechanism(mi)
    named, row = plan.member_constants(mi, mech, 20)
    emu = HostEmu(mech.source(hipbind.kernel_template()), tag="dme_nb")
    Y = g["y"]
    for k, (case, t) in enumerate(zip(g["case"], g["times"])):
        mi_s = with_schedule(g13["cases"][str(case)]["schedule"])
        s = schedule.parse(mi_s)
        np.testing.assert_allclose(s.at(float(t))[0], g["forced"][k], rtol=1e-15)
        rows = s.rows_at([row], [named], float(t))
        out, flags = emu.rhs(Y, np.tile(rows[0], (len(Y), 1)), 20)
        for j in range(len(Y)):
            e = rowwise_err(out[j], g["f"][k, j], mech.V)
            assert e < 1e-11, (k, j, e)


# ----------------------------------------------------------------------------- order of the non-autonomous RODAS4 step
RODAS_A = [[], [1.544], [0.9466785280815826, 0.2557011698983284],
           [3.314825187068521, 2.896124015972201, 0.9986419139977817],
           [1.221224509226641, 6.019134481288629, 12.53708332932087, -0.6878860361058950],
           [1.221224509226641, 6.019134481288629, 12.53708332932087, -0.6878860361058950, 1.0]]
RODAS_C = [[], [-5.6688], [-2.430093356833875, -0.2063599157091915],
           [-0.1073529058151375, -9.594562251023355, -20.47028614809616],
           [7.496443313967647, -10.24680431464352, -33.99990352819905, 11.70890893206160],
           [8.083246795921522, -7.981132988064893, -31.52159432874371, 16.31930543123136, -6.058818238834054]]
RODAS_CT = [0.0, 0.386, 0.21, 0.63, 1.0, 1.0]                 # kernels/11_forcing.inc rmt_rodas_t
RODAS_D = [0.25, -0.1043, 0.1035, -0.3620000000000023e-01, 0.0, 0.0]
RODAS_GAM = 0.25


def rodas4_step(f, jac, ft, t, y, h, d=RODAS_D):
    """The kernel's stage loop (60_ros4.inc rmt_rodas_bs: Y_i = y + sum a_ij G_j, (I/(gamma h) - J) G_i = f(t + c_i h, Y_i)
    + sum c_ij G_j / h + h d_i f_t, y_new = Y_6 + G_6) with dense linear algebra."""
    A = np.eye(len(y))/(RODAS_GAM*h) - jac(t, y)
    dfdt = ft(t, y)
    Gs = []
    for i in range(6):
        Y = y + sum(a*g for a, g in zip(RODAS_A[i], Gs))
        rhs = f(t + RODAS_CT[i]*h, Y) + sum(c*g for c, g in zip(RODAS_C[i], Gs))/h + h*d[i]*dfdt
        Gs.append(np.linalg.solve(A, rhs))
    return Y + Gs[5]


def test_nonautonomous_rodas4_order():
    """Stiff two-variable problem with a linearly ramped source, fixed steps: with c_i AND d_i the observed order is
    above 3.5 (the method's is 4); with d_i = 0 it collapses below 1.5 - so the test can see the term."""
    from scipy.integrate import solve_ivp

    def u(t):
        return 1.0 + 2.0*t

    def f(t, y):
        return np.array([-40.0*(y[0] - u(t)) + y[1]**2, -y[1] + 0.5*y[0]*u(t)])

    def jac(t, y):
        return np.array([[-40.0, 2.0*y[1]], [0.5*u(t), -1.0]])

    def ft(t, y):
        return np.array([40.0*2.0, 0.5*y[0]*2.0])

    y0 = np.array([1.0, 0.5])
    exact = solve_ivp(f, (0.0, 1.0), y0, method="Radau", rtol=1e-13, atol=1e-13, jac=jac).y[:, -1]

    def errors(d):
        out = []
        for n in (20, 40, 80, 160, 320):
            y, h = y0.copy(), 1.0/n
            for k in range(n):
                y = rodas4_step(f, jac, ft, k*h, y, h, d)
            out.append(np.max(np.abs(y - exact)))
        return np.array(out)

    e = errors(RODAS_D)
    orders = np.log2(e[:-1]/e[1:])
    print("non-autonomous RODAS4: errors", e, "orders", orders)
    assert np.all(orders > 3.5), orders
    e0 = errors([0.0]*6)
    orders0 = np.log2(e0[:-1]/e0[1:])
    print("without the d_i f_t term: errors", e0, "orders", orders0)
    assert np.all(orders0 < 1.5), orders0


# ----------------------------------------------------------------------------- cross-compile for gfx950
FORCED_KERNELS = [
    ("rk4", 64, 1, {}, ("rmt_n2_rk4_reg", "rmt_n2_rk4_mem")),
    ("rk45", 64, 1, {"RMT_RK45_LDS": "2"}, ("rmt_n2_rk45_reg", "rmt_n2_rk45_mem")),
    ("ros4", 64, 1, {"RMT_WITH_ROS4": "1"}, ("rmt_n2_ros4_mem",)),
]


@pytest.mark.parametrize("name,block,npt,defs,kernels", FORCED_KERNELS)
def test_forced_kernels_cross_compile(name, block, npt, defs, kernels):
    """The forced DME build of every kernel that must carry the forcing compiles for gfx950 (hipRTC, no GPU)."""
    mech = plan.Mechanism(INP.dme_notebook_input())
    tpl = hipbind.kernel_template()
    d = dict(defs, RMT_FORCING="1")
    blob = hipbind.compile_cached(mech.source(tpl, False, block, npt, None, d), mech.digest(tpl, False, block, npt, None, d),
                                  "gfx950")
    for k in kernels:
        res = isa.kernel_resources(blob, k)
        print(k, "forced", res)
        assert res["vgpr_count"] > 0
    assert b"rmt_n2_ros4_chain" not in blob          # a forced reactor stays on one workgroup


def test_unforced_build_has_no_forcing():
    """A build without the define contains no forcing symbol and has the unchanged member row."""
    mech = plan.Mechanism(INP.dme_notebook_input())
    tpl = hipbind.kernel_template()
    src = mech.source(tpl, False, 64, 1)
    assert "#define RMT_FORCING" not in src.split("// generated by", 1)[1].split("typedef", 1)[0]     # the prelude
    # (compiled with the assertion appended: the row of an unforced code object is 16 + S + NU doubles)
    blob, _ = hipbind.compile_source(src + '\nstatic_assert(RMT_NM == 16 + RMT_S + RMT_NU && !RMT_FORCING, "member row");\n')
    assert b"rmt_forcing" not in blob and b"rmt_n2_ros4_chain" not in blob
    blob = hipbind.compile_cached(src, mech.digest(tpl, False, 64, 1), "gfx950")
    assert b"rmt_forcing" not in blob
    forced = mech.source(tpl, False, 64, 1, None, {"RMT_FORCING": "1"})
    assert forced.replace("#define RMT_FORCING 1\n", "") == src        # the define is the ONLY difference of the sources


def test_wide_mechanism_with_the_stiff_stepper_is_refused():
    """More than 8 variables per node: the stiff stepper's four-lane form does not carry the forcing."""
    for ivp in ("hip-ros4", "default"):
        mi = INP.syn12_input(ivp=ivp)
        mi["solver-config"].update({"quiet": True, "schedule": {"time": [0, 0.1], "inlet-pressure": [
            mi["operating-conditions"]["pressure"], 0.98*mi["operating-conditions"]["pressure"]]}})
        with pytest.raises(NotImplementedError, match="schedule"):
            rmtExe(mi)


def test_forced_build_keeps_the_other_literals():
    """A forced code object of a sweep takes the sweep-invariant fields as literals, except the three its schedule moves."""
    from rmt_app_amd.ensemble import expand_members
    base = INP.dme_notebook_input()
    members = expand_members(base, {"temperature": [513.0, 533.0]})
    mech = plan.Mechanism(base)
    rows = np.array([plan.member_constants(mi, mech, 20)[1] for mi in members])
    wide = np.concatenate([rows, np.zeros((2, schedule.TAIL))], axis=1)
    _, _, defs, src, _ = n2.device_source(mech, wide, 20, defines={"RMT_FORCING": "1"})
    assert "RMT_MC_UA" in defs and "RMT_MC_P0" not in defs and "RMT_MC_TM" not in defs and "RMT_MC_THETA_IN" not in defs
    _, _, plain, _, _ = n2.device_source(mech, rows, 20)
    assert "RMT_MC_P0" in plain and "RMT_MC_TM" in plain          # (uniform over this sweep: literals of the unforced build)
