"""The lowering is three modules, imported in one direction: dag (tracing front end) <- emit (HIP text of a DAG) <-
lowering (analyses and rewrites).  What one emission needs lives in an emit.Emission, never on the DAG: the DAG a
mechanism caches and shares between every source() / digest() call is only read, so the text of an emission does not
depend on what was emitted before.  The walkers every pass shares (Graph.operands, Lowered.users / t_only / order) against
the rule they replace; the node creation order of the two rewrites, pinned by digests taken before the passes shared one
copy helper.  On the DME notebook mechanism and on the 12-species one, which has "gen" / "basis" exponents."""
import ast
import math

import pytest

import inputs as INP
from rmt_app_amd import dag as dagmod
from rmt_app_amd import emit, lowering, plan

NODE = dict(const_table=True, kcache=True, kcache_gen="basis", kcache_thr=1e-4, div_batch=True, kcache_fold=True,
            rate_scale=True, extra_den=True, head=False)


@pytest.fixture(scope="module", params=["dme_nb", "syn12"])
def dag(request):
    return plan.Mechanism(INP.ALL_N2_INPUTS[request.param]()).device_dag()


def test_emission_leaves_the_dag_alone(dag):
    grad = dag.gradient()
    for d, run in ((dag, lambda: dag.emit("rmt_kinetics")), (dag, lambda: dag.emit("rmt_kinetics_node", **NODE)),
                   (dag, lambda: emit.Emission(dag, "rmt_kinetics_node", **NODE)),
                   (grad, lambda: grad.emit_jac("rmt_kinetics_jac"))):
        attrs, nodes, live, order = set(vars(d)), list(d.g.nodes), set(d.live), list(d.order)
        run()
        assert set(vars(d)) == attrs and d.g.nodes == nodes and d.live == live and d.order == order
    assert not hasattr(dag, "rates_scaled") and not hasattr(grad, "rates_scaled")
    assert set(vars(dag)) == {"g", "outputs", "S", "live", "order"}


def test_emission_does_not_depend_on_what_ran_before(dag):
    runs = {"A": lambda d: (d.emit("rmt_kinetics"), None),
            "B": lambda d: (lambda em: (em.text, em.rates_scaled))(emit.Emission(d, "rmt_kinetics_node", **NODE)),
            "C": lambda d: (d.emit("rmt_kinetics", kcache=True, kcache_gen="basis"), None)}
    first = {k: run(lowering.Lowered(dag.g, dag.outputs, dag.S)) for k, run in runs.items()}     # each on a fresh DAG
    assert len({t for t, _ in first.values()}) == 3
    assert "rmt_exp_sel<KC::enabled>(" in first["B"][0] and "rmt_exp_sel<KC::enabled>(" in first["C"][0]
    assert ", const real gden, real& ginv" in first["B"][0] and "gden" not in first["A"][0] + first["C"][0]
    assert first["B"][1] == (", const real rscale" in first["B"][0])
    for seq in ("ABC", "CBA", "ABA", "BBC"):
        for k in seq:                                          # ... and one after the other on the shared one
            assert runs[k](dag) == first[k], (seq, k)


def _old_operands(g, i):
    """the operand rule as every pass used to spell it"""
    op, a, b = g.nodes[i]
    if op in ("const", "in"):
        return []
    return [a] + ([b] if (b is not None and op != "powi") else [])


def test_walkers_on_a_hand_built_graph():
    g = lowering.Graph()
    T, x0 = g.inp("T"), g.inp("x0")
    p4 = T**4                              # powi: its second field (4) is an exponent - and the id of the next node
    e = p4._un("exp", math.exp)            # unary; read by the division, the sum, the product and an output
    q = x0/e
    s = e + q
    h = e*2.0
    two = h.g.nodes[h.i][2]
    assert g.nodes[p4.i] == ("powi", T.i, 4) and e.i == 4 and g.is_const(two)
    low = lowering.Lowered(g, [e.i, s.i, h.i], 1)
    assert low.order == sorted(low.live) == [T.i, x0.i, p4.i, e.i, q.i, s.i, two, h.i]     # (the lifted exponent is dead)
    for i in low.order:
        assert g.operands(i) == _old_operands(g, i), i
    assert g.operands(p4.i) == [T.i] and g.operands(q.i) == [x0.i, e.i] and g.operands(two) == g.operands(T.i) == []
    assert low.users() == {T.i: [(p4.i, 0)], p4.i: [(e.i, 0)], x0.i: [(q.i, 0)],
                           e.i: [(q.i, 1), (s.i, 0), (h.i, 0), (-1, 0)], q.i: [(s.i, 1)], two: [(h.i, 1)],
                           s.i: [(-1, 0)], h.i: [(-1, 0)]}
    assert low.t_only() == {T.i: True, x0.i: False, p4.i: True, e.i: True, q.i: False, s.i: False, two: True, h.i: True}
    # a node nobody reads is not walked
    dead = lowering.Lowered(g, [q.i], 1)
    assert dead.order == [T.i, x0.i, p4.i, e.i, q.i] and dead.users()[e.i] == [(q.i, 1)]


# trace(...).optimize().digest() before optimize, reassociate and gradient shared one copy helper: node ids appear in the
# emitted text as v<N>, so the creation order of the rewritten nodes is part of the result
OPTIMIZED_DIGEST = {"dme_nb": "92a30aad613bfe59e3c2a21f127228f0be61dbd4f776a42b8ed94eeb56dcb487",
                    "dme_script": "9019a9d2c51f8686e6aa282a9e2dcb30e1923d74b0c3e35314e40673ffd0fd6a",
                    "ch4": "3069372e4d3a5ded7206d42bcb3df01c91a5449f2ce28df95fb45cc6f65596d3",
                    "syn12": "0c65007f80d88f185e9ab27ff6ab35bbccea10782e8f0bdb19241e0c79755a2a"}


@pytest.mark.parametrize("name", sorted(INP.ALL_N2_INPUTS))
def test_rewrites_create_their_nodes_in_the_same_order(name):
    mi = INP.ALL_N2_INPUTS[name]()
    rr = mi["reaction-rates"]
    low = lowering.trace(rr["VARS"], rr["RATES"], len(mi["feed"]["components"]["shell"]))
    assert low.optimize().digest() == OPTIMIZED_DIGEST[name]
    opt = low.optimize()
    grad = opt.gradient()                    # the primal part of a gradient DAG is a plain copy: nothing sorted or rewritten
    assert [grad.g.nodes[i][0] for i in range(grad.n_primal)] == [opt.g.nodes[i][0] for i in opt.order]


def test_lowering_re_exports_the_tracing_front_end():
    """Product modules and tests import the flags, Graph, LoweringError, trace and is_scalar_constant from
    rmt_app_amd.lowering; they are the objects of rmt_app_amd.dag.  emit never imports lowering, dag imports neither."""
    for name in ("FLAG_DOMAIN", "FLAG_DIV0", "FLAG_OVERFLOW", "FLAG_NONFINITE", "FLAG_STEP", "Graph", "LoweringError", "Sym",
                 "SymVector", "rebind", "is_scalar_constant"):
        assert getattr(lowering, name) is getattr(dagmod, name), name
    assert callable(lowering.trace) and lowering.Gradient.__mro__[1] is lowering.Lowered
    assert plan.trace is lowering.trace and plan.Emission is emit.Emission

    def imported(mod):
        tree = ast.parse(open(mod.__file__).read())
        return {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level == 1}
    assert imported(dagmod) == set() and imported(emit) == {"dag"} and imported(lowering) == {"dag", "emit"}
