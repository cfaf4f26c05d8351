"""CPU tests of the steady packed-bed models M7 (runM3) and M1 (runM1): the member rows against the reference's setup
(golden G12, tools/make_golden.py m7 m1), the generated node functions (host build of the same source the GPU gets)
against the reference's model functions, the analytic Jacobians against forward differences, the public API on a
machine without a GPU, and the gfx950 cross-compilation of both modules."""
import json
import os

import numpy as np
import pytest

import inputs_steady as INS
from oracle.hostemu import HostEmu
from rmt_app_amd import hipbind, isa, plan
from rmt_app_amd.n2 import compile_options, device_source
from rmt_app_amd.steady import SS_MODEL_DEFINE, output_points, result_dict
from rmt_app_amd.settings import solverSetting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
MODELS = ("M7", "M1")


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)/np.maximum(np.abs(b), 1e-300))


def golden(model):
    g = np.load(os.path.join(G, "g12_%s.npz" % model.lower()))
    with open(os.path.join(G, "g12_%s_setup.json" % model.lower())) as f:
        setup = json.load(f)
    return g, setup


def case(model):
    mi = INS.STEADY_INPUTS[(model, "dme")]()
    mech = plan.Mechanism(mi)
    named, row = getattr(plan, "member_constants_" + model.lower())(mi, mech)
    return mi, mech, named, row


@pytest.fixture(scope="module")
def template():
    return hipbind.kernel_template()


def emu_for(model, template, mech, openmp=True):
    return HostEmu(mech.source(template, defines={"RMT_WITH_N1": "1", "RMT_SS_MODEL": SS_MODEL_DEFINE[model]}),
                   tag="ss_%s" % model.lower(), openmp=openmp)


def unscale_rate(dU, named, model, S):
    """d u/d z* of the kernel -> d y/d z of the reference's variables (affine scalings: only the factors count)."""
    one = plan.unscale_steady(np.ones(dU.shape[-1]), named, model, S)
    zero = plan.unscale_steady(np.zeros(dU.shape[-1]), named, model, S)
    return dU*(one - zero)/named["ReLe"]


@pytest.mark.parametrize("model", MODELS)
def test_member_constants_match_reference_setup(model):
    mi, mech, named, row = case(model)
    _, setup = golden(model)
    assert relerr(named["IV"], setup["IV"]) <= 1e-14
    c = setup["const"]
    assert relerr(named["CrSeAr"], c["CrSeAr"]) <= 1e-14
    assert relerr(named["MoWei"], c["MoWei"]) <= 1e-14
    assert relerr(named["StHeRe25"], c["StHeRe25"]) <= 1e-14
    assert relerr(named["GaMiVi"], c["GaMiVi"]) <= 1e-14
    assert relerr(named["OvHeTrCo"], setup["ExHe"]["OvHeTrCo"]) <= 1e-14
    assert relerr(named["EfHeTrAr"], setup["ExHe"]["EfHeTrAr"]) <= 1e-14          # M1: 4/ReInDi (pbReactor.py:211)
    assert relerr(named["MeTe"], setup["ExHe"]["MeTe"]) <= 1e-14
    if model == "M7":
        bc = setup["constBC1"]
        for k in ("VoFlRa0", "SpCoi0", "SpCo0", "P0", "T0"):
            assert relerr(named[k], bc[k]) <= 1e-14, k
    # the packed row's initial state is the reference's IV after scaling
    u0 = np.concatenate([row[plan.MEMBER_FIXED:plan.MEMBER_FIXED + mech.S],
                         [0.0, 1.0] if model == "M7" else [1.0, 0.0, 1.0]])
    assert relerr(plan.unscale_steady(u0, named, model, mech.S), setup["IV"]) <= 1e-14
    assert row.shape == (mech.row_width,)


@pytest.mark.parametrize("model", MODELS)
def test_generated_node_function_vs_reference(model, template):
    """rmt_n1_rhs generated for RMT_SS_MODEL 7 / 1 against modelEquationM3 / modelEquationM1 at the G12 states (the
    feed, three states of the reference's run, a hot perturbed state, a species at 1e-12 of the total)."""
    mi, mech, named, row = case(model)
    g, _ = golden(model)
    Y, F, equil = g["rhs_y"], g["rhs_f"], g["rhs_equil"]
    U = plan.scale_steady(Y, named, model, mech.S)
    du, flags = emu_for(model, template, mech).n1_rhs(U, np.tile(row, (len(U), 1)))
    assert not flags.any()
    got = unscale_rate(du, named, model, mech.S)
    for k in range(len(Y)):
        # the run states sit close to chemical equilibrium: rates there are differences of nearly equal terms
        tol = 1e-7 if equil[k] else 1e-11
        assert relerr(got[k], F[k]) <= tol, (k, relerr(got[k], F[k]))


@pytest.mark.parametrize("model", MODELS)
def test_analytic_jacobian_vs_forward_differences(model, template):
    mi, mech, named, row = case(model)
    g, _ = golden(model)
    U = plan.scale_steady(g["rhs_y"], named, model, mech.S)
    jan, jfd, fan, fref = emu_for(model, template, mech, openmp=False).n1_jac(U, np.tile(row, (len(U), 1)))
    assert jan.shape[1:] == (mech.S + (2 if model == "M7" else 3),)*2
    assert np.max(np.abs(fan - fref)/np.maximum(np.abs(fref), 1e-300)) <= 1e-12
    for k in range(len(U)):
        scale = np.max(np.abs(jfd[k]), axis=1, keepdims=True)
        assert np.max(np.abs(jan[k] - jfd[k])/scale) <= 1e-4, (k, np.max(np.abs(jan[k] - jfd[k])/scale))


@pytest.mark.parametrize("model", MODELS)
def test_result_dict_layout_matches_reference(model):
    """result_dict applied to the reference's own solve_ivp output rebuilds the dict rmtExe returned (G12 default)."""
    mi, mech, named, row = case(model)
    g, setup = golden(model)
    res = result_dict(g["default_sol_y"], named, mech, model)
    assert relerr(res["dataYs"], g["default_dataYs"]) <= 1e-15
    assert np.allclose([xy[0] for xy in res["XYList"]], g["default_x"], rtol=1e-15, atol=0)
    assert relerr([xy[1] for xy in res["XYList"]], g["default_XY_y"]) <= 1e-15
    assert [d["leg"] for d in res["dataList"]] == [str(s) for s in g["default_legends"]]
    assert relerr([d["y"] for d in res["dataList"]], g["default_dataList_y"]) <= 1e-15
    assert relerr(res["XYList"][0][0], setup["t_eval"]) <= 1e-15
    assert output_points(model, {}) == len(setup["t_eval"])


def test_solver_settings_mirror_the_reference():
    assert solverSetting["S3"]["timesNo"] == 25
    assert solverSetting["M9"]["zNo"] == 30
    assert output_points("M7", {"zNo": 12}) == 12 and output_points("M1", {"zNo": 7}) == 7


@pytest.mark.parametrize("model", MODELS)
def test_rmtexe_without_gpu_raises_device_error(model):
    """M7 and M1 are built: without a GPU rmtExe reaches the device and raises RmtN2Error (not NotImplementedError)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from rmt_app_amd import rmtExe
    with pytest.raises(hipbind.RmtN2Error):
        rmtExe(INS.STEADY_INPUTS[(model, "dme")]())


def test_bad_ivp_and_other_models():
    from rmt_app_amd import rmtExe
    mi = INS.m7_dme_input(ivp="Euler")
    with pytest.raises(ValueError, match="ivp"):
        rmtExe(mi)
    with pytest.raises(NotImplementedError):
        rmtExe(INS.m7_dme_input(model="M8"))


@pytest.mark.parametrize("model", MODELS)
def test_steady_modules_cross_compile_for_gfx950(model):
    """The module steady.run_steady loads (hipRTC, no GPU): its rmt_n1_ros4 with V1 = S+2 (M7) or S+3 (M1) unknowns
    keeps every value in registers - no scratch."""
    mi, mech, named, row = case(model)
    kw = dict(block=64, npt=1, specialize=False, features=("n1",), defines={"RMT_SS_MODEL": SS_MODEL_DEFINE[model]})
    block, npt, defs, src, key = device_source(mech, row, 64, **kw)
    assert defs["RMT_SS_MODEL"] == SS_MODEL_DEFINE[model] and defs["RMT_WITH_N1"] == "1"
    blob = hipbind.compile_cached(src, key, "gfx950", compile_options(block, npt, ("n1",), "", kw["defines"]))
    res = isa.kernel_resources(blob, "rmt_n1_ros4")
    assert res["private_segment_fixed_size"] == 0, res
    assert res["vgpr_count"] <= 512
