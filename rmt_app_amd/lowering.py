"""Lowering of PyREMOT ``reaction-rates`` lambdas to a HIP device function.

The reference evaluates the user's VARS / RATES dicts node by node in Python
(reactionRateExe, PyREMOT/docs/rmtReaction.py:11-61): VARS entries are evaluated in insertion
order into one namespace that already holds ``R_CONST, T, P, MoFri, SpCoi``; entries that are
functions are called with the partially filled namespace, everything else is copied as a
constant; then every RATES lambda is called with the full namespace.

Here the same ordered evaluation is performed ONCE, symbolically (``trace``, on the symbols of dag.py).  The result is an
expression DAG over ``T, P, MoFri[i], SpCoi[i]`` with hash-consed common subexpressions and folded constants - a
``Lowered``, which holds the analyses and rewrites of the DAG - and is printed as straight-line HIP C++ (one
``const real vN = ...;`` per node, emit.py) for the fused RHS kernel.  Three modules, imported in one direction:
dag <- emit <- lowering.
"""
import hashlib
import math
import types

from .dag import (  # noqa: F401  (also the re-exports: the tracing front end stays importable from here)
    _EXP_MAX, FLAG_DIV0, FLAG_DOMAIN, FLAG_NONFINITE, FLAG_OVERFLOW, FLAG_STEP, Graph, LoweringError, Sym, SymVector, _num,
    _pow, is_scalar_constant, rebind)
from .emit import Emission, JacEmission


class Lowered:
    """Result of trace(): DAG + output node ids + op statistics."""

    def __init__(self, graph, outputs, nspecies):
        self.g, self.outputs, self.S = graph, outputs, nspecies
        self.live = self._live()
        self.order = sorted(self.live)      # creation order = a topological one: every pass walks the DAG in it

    def _live(self):
        live, stack = set(), list(self.outputs)
        while stack:
            i = stack.pop()
            if i not in live:
                live.add(i)
                stack.extend(self.g.operands(i))
        return live

    # ---- the walks every pass shares
    def users(self):
        """node -> [(user, slot)] over the live DAG, in the user's id order; an output counts as user (-1, 0)"""
        users = {}
        for i in self.order:
            for slot, o in enumerate(self.g.operands(i)):
                users.setdefault(o, []).append((i, slot))
        for o in self.outputs:
            users.setdefault(o, []).append((-1, 0))
        return users

    def t_only(self):
        """node -> True when its value depends on nothing but the temperature (constants included)"""
        g, mark = self.g, {}
        for i in self.order:
            op, a, b = g.nodes[i]
            m = (a == "T") if op == "in" else True
            for o in g.operands(i):
                m = m and mark[o]
            mark[i] = m
        return mark

    def _copy(self, g2, rule=None, sort=()):
        """Copy the live DAG into the fresh Graph ``g2``, node by node in id order (the creation order of the new nodes is
        part of the result: ids appear in the emitted text as v<N>) -> {node: its Sym in g2}.  ``rule(i, new)`` may put
        something else in a node's place - a Sym, or None for a node that only lives on inside its users - and returns
        NotImplemented for the plain copy; the binary ops named in ``sort`` get their operands in id order."""
        g, new = self.g, {}
        for i in self.order:
            op, a, b = g.nodes[i]
            r = rule(i, new) if rule else NotImplemented
            if r is not NotImplemented:
                new[i] = r
            elif op == "const":
                new[i] = g2.const(g.cval(i))
            elif op == "in":
                new[i] = g2.inp(a)
            elif op == "powi":
                new[i] = g2._mk("powi", new[a].i, b)
            elif b is None:
                new[i] = g2._mk(op, new[a].i)
            else:
                x, y = new[a].i, new[b].i
                new[i] = g2._mk(op, *((y, x) if (op in sort and x > y) else (x, y)))
        return new

    def stats(self):
        st = {}
        for i in self.order:
            op = self.g.nodes[i][0]
            st[op] = st.get(op, 0) + 1
        return st

    def uses(self, name):
        return any(self.g.nodes[i][:2] == ("in", name) for i in self.live)

    def digest(self):
        h = hashlib.sha256()
        for i in self.order:
            h.update(repr(self.g.nodes[i]).encode())
        h.update(repr(self.outputs).encode())
        return h.hexdigest()

    # ---- evaluation on the host (used by tests to check the trace itself, not by the product path)
    def evaluate(self, T, P, x, C, U=()):
        env = {}
        for i in self.order:
            op, a, b = self.g.nodes[i]
            if op == "const":
                env[i] = self.g.cval(i)
            elif op == "in":
                env[i] = {"T": T, "P": P}.get(a) if a in ("T", "P") else (
                    x[int(a[1:])] if a[0] == "x" else (U[int(a[1:])] if a[0] == "u" else C[int(a[1:])]))
            elif op == "powi":
                env[i] = env[a]**b
            elif op in ("add", "sub", "mul", "div", "pow", "min", "max"):
                u, v = env[a], env[b]
                env[i] = {"add": lambda: u + v, "sub": lambda: u - v, "mul": lambda: u*v,
                          "div": lambda: u/v, "pow": lambda: math.pow(u, v),
                          "min": lambda: min(u, v), "max": lambda: max(u, v)}[op]()
            else:
                fn = {"neg": lambda u: -u, "abs": abs, "exp10": lambda u: 10.0**u,
                      "exp2": lambda u: 2.0**u, "rcp": lambda u: 1.0/u,
                      "expn": lambda u: math.exp(-u), "exp10n": lambda u: 10.0**(-u),
                      "exp2n": lambda u: 2.0**(-u), "sign": lambda u: (u > 0) - (u < 0),
                      "step": lambda u: 1.0 if u >= 0 else 0.0}.get(op) or getattr(math, op)
                env[i] = fn(env[a])
        return [env[o] for o in self.outputs]

    # ---- algebraic strength reduction (device build only; changes results by a few ulp)
    def optimize(self):
        """Cheaper but equivalent forms for the fp64 VALU (costs measured on gfx950):
          a/exp(z)           -> a*exp(-z)            when exp(z) is only ever a divisor
          a/b, c/b, ...      -> a*r, c*r, r = 1/b    when b divides at least twice
          log10(x)           -> log(x)*(1/ln 10)     (one log serves both bases)
        The Python-exception conditions of the original expressions are still flagged."""
        g = self.g
        uses = self.users()
        def only_divides(n):
            return bool(uses.get(n)) and all(u >= 0 and g.nodes[u][0] == "div" and slot == 1
                                             for (u, slot) in uses[n])
        # b "divides" directly (x/b) or through an integer power that itself only divides (x/b^n)
        div_uses = {}
        for n, us in uses.items():
            c = 0
            for (u, slot) in us:
                if u < 0:
                    continue
                uop = g.nodes[u][0]
                if uop == "div" and slot == 1:
                    c += 1
                elif uop == "powi" and g.nodes[u][2] > 0 and only_divides(u):
                    c += len(uses[u])
            div_uses[n] = c
        g2 = Graph()
        LOG10E = 1.0/math.log(10.0)
        NEGEXP = {"exp": "expn", "exp10": "exp10n", "exp2": "exp2n"}

        def mul(x, y):
            return x._bin("mul", x, y, lambda p, q: p*q)

        def shared_base(n, e):
            """y^e, e > 0, whose base divides at least twice: x/y^e goes through the reciprocal of y"""
            return e > 0 and div_uses.get(n, 0) >= 2 and not g.is_const(n)

        def rule(i, new):
            op, a, b = g.nodes[i]
            if op == "powi" and only_divides(i) and shared_base(a, b):
                return None            # x/y^n is emitted as x*(1/y)^n at its uses
            if op == "div":
                bop, ba, bb = g.nodes[b]
                if bop in NEGEXP and only_divides(b):
                    return mul(new[a], g2._mk(NEGEXP[bop], new[ba].i))
                if bop == "powi" and (new[b] is None or shared_base(ba, bb)):
                    r = g2._mk("rcp", new[ba].i)          # 1/y exists anyway: x/y^n = x*(1/y)^n
                    return mul(new[a], g2._mk("powi", r.i, bb))
                if div_uses.get(b, 0) >= 2 and not g.is_const(b):
                    return mul(new[a], g2._mk("rcp", new[b].i))
            elif op == "log10":
                return mul(g2._mk("log", new[a].i), g2.const(LOG10E))
            elif op in NEGEXP and only_divides(i):
                return None            # 1/exp(z) is emitted as exp(-z) at its uses
            return NotImplemented
        new = self._copy(g2, rule, sort=("add", "mul", "min", "max"))
        return Lowered(g2, [new[o].i for o in self.outputs], self.S).reassociate()

    def reassociate(self):
        """Products only: flatten every multiplication tree whose inner products have no other
        user, fold ALL its constant factors into one, drop factors 1.0, and rebuild it as
        ((K * inputs...) * others...) so that sub-products such as 1e-5*P are shared between the
        species (hash-consing).  Changes rounding at the 1e-16 level, never the exception
        behaviour (Python's float product does not raise)."""
        g = self.g
        nuse = {n: len(us) for n, us in self.users().items()}

        def factors(i, root):
            op, a, b = g.nodes[i]
            if op == "mul" and (root or nuse.get(i, 0) == 1):
                return factors(a, False) + factors(b, False)
            return [i]

        inner = set()        # mul nodes absorbed into a parent product
        for i in self.order:
            op, a, b = g.nodes[i]
            if op == "mul":
                for c in (a, b):
                    if g.nodes[c][0] == "mul" and nuse.get(c, 0) == 1:
                        inner.add(c)
        g2 = Graph()

        def product(new, fs, acc=None):
            for f in fs:
                acc = new[f] if acc is None else acc._bin("mul", acc, new[f], lambda p, q: p*q)
            return acc

        def rule(i, new):
            op, a, b = g.nodes[i]
            if op == "mul":
                if i in inner:
                    return None
                fs = factors(i, True)
                K, rest = 1.0, []
                for f in fs:
                    if g.is_const(f):
                        K *= g.cval(f)
                    else:
                        rest.append(f)
                if not math.isfinite(K) or K == 0.0 or not rest:
                    if new[a] is None or new[b] is None:          # operands were absorbed: rebuild plainly
                        return product(new, fs)
                    return g2._mk("mul", min(new[a].i, new[b].i), max(new[a].i, new[b].i))
                ins = sorted([f for f in rest if g.nodes[f][0] == "in"], key=lambda f: g.nodes[f][1])
                oth = [f for f in rest if g.nodes[f][0] != "in"]
                return product(new, ins + oth, None if K == 1.0 else g2.const(K))
            if op == "rcp" and g2.nodes[new[a].i][0] == "mul":
                # 1/(K*T) -> (1/K)*(1/T): the kernel hands 1/T to the kinetics for free (it needs it
                # for M/T anyway), so this reciprocal becomes one multiplication
                mo, ma, mb = g2.nodes[new[a].i]
                kk, xx = (ma, mb) if g2.is_const(ma) else (mb, ma)
                if g2.is_const(kk) and g2.nodes[xx] == ("in", "T", None) and g2.cval(kk) != 0.0:
                    rt = g2._mk("rcp", xx)
                    return rt._bin("mul", g2.const(1.0/g2.cval(kk)), rt, lambda p, q: p*q)
            return NotImplemented
        new = self._copy(g2, rule, sort=("add", "min", "max"))
        return Lowered(g2, [new[o].i for o in self.outputs], self.S)

    # ---- symbolic gradient (sparse forward mode on the DAG)
    def gradient(self, wrt=None):
        """d outputs / d inputs as a DAG: every node carries the dict {input: derivative node} of its
        NON-ZERO partials (one-hot seeds, so an expression that does not depend on an input never gets
        a tangent for it), built with constant folding and the identities x*0, x*1, x+0 - the result
        is close to what one would write by hand.  ``wrt``: input names to differentiate by (default:
        T and every x_i / C_i the expressions use; P is a frozen parameter of the node Jacobian).
        Returns a ``Gradient`` (primal outputs + partials) for emission / evaluation."""
        g = self.g
        g2 = Graph()
        new = self._copy(g2)      # primal part first: its node ids stay below n_primal, where the exception tests are kept
        n_primal = len(g2.nodes)
        if wrt is None:
            wrt = sorted({g.nodes[i][1] for i in self.live if g.nodes[i][0] == "in" and g.nodes[i][1] != "P"
                          and g.nodes[i][1][0] != "u"})        # u<k>: per-reactor parameters, frozen like P
        wrt = list(wrt)

        def c(v):
            return g2.const(v)

        def isc(x, v=None):
            return g2.is_const(x.i) and (v is None or g2.cval(x.i) == v)

        def add(x, y):
            if x is None:
                return y
            if y is None:
                return x
            if isc(x, 0.0):
                return y
            if isc(y, 0.0):
                return x
            return x._bin("add", x, y, lambda p, q: p + q)

        def sub(x, y):
            if y is None:
                return x
            if x is None:
                return neg(y)
            if isc(y, 0.0):
                return x
            return x._bin("sub", x, y, lambda p, q: p - q)

        def mul(x, y):
            if x is None or y is None:
                return None
            if isc(x, 0.0) or isc(y, 0.0):
                return None
            if isc(x, 1.0):
                return y
            if isc(y, 1.0):
                return x
            if isc(x, -1.0):
                return neg(y)
            if isc(y, -1.0):
                return neg(x)
            return x._bin("mul", x, y, lambda p, q: p*q)

        def neg(x):
            if x is None:
                return None
            if g2.nodes[x.i][0] == "neg":
                return Sym(g2, g2.nodes[x.i][1])
            return x._un("neg", lambda p: -p)

        def un(op, x):
            return g2._mk(op, x.i)

        LN10, LN2 = math.log(10.0), math.log(2.0)
        d = {}
        for i in self.order:
            op, a, b = g.nodes[i]
            u = new[i]
            if op == "const":
                d[i] = {}
                continue
            if op == "in":
                d[i] = {a: c(1.0)} if a in wrt else {}
                continue
            A = new[a]
            da = d[a]
            if op == "powi":
                n = b
                f = mul(c(float(n)), A if n == 2 else (c(1.0) if n == 1 else g2._mk("powi", A.i, n - 1)))
                d[i] = {k: mul(f, v) for k, v in da.items()}
                continue
            if b is not None:
                B = new[b]
                db = d[b]
                keys = list(dict.fromkeys(list(da) + list(db)))
                out = {}
                for k in keys:
                    x, y = da.get(k), db.get(k)
                    if op == "add":
                        v = add(x, y)
                    elif op == "sub":
                        v = sub(x, y)
                    elif op == "mul":
                        v = add(mul(x, B), mul(A, y))
                    elif op == "div":
                        v = mul(sub(x, mul(u, y)), un("rcp", B)) if (x is not None or y is not None) else None
                    elif op == "pow":
                        t1 = mul(y, un("log", A))
                        t2 = mul(mul(B, x), un("rcp", A))
                        v = mul(u, add(t1, t2))
                    elif op in ("max", "min"):
                        sel = un("step", sub(A, B) if op == "max" else sub(B, A))
                        v = add(mul(sel, x), mul(sub(c(1.0), sel), y))
                    else:
                        raise LoweringError("no derivative rule for op %r" % op)
                    if v is not None and not isc(v, 0.0):
                        out[k] = v
                d[i] = out
                continue
            # unary
            if op == "neg":
                f = c(-1.0)
            elif op == "abs":
                f = un("sign", A)
            elif op == "rcp":
                f = neg(mul(u, u))
            elif op == "sqrt":
                f = mul(c(0.5), un("rcp", u))
            elif op == "exp":
                f = u
            elif op == "exp10":
                f = mul(c(LN10), u)
            elif op == "exp2":
                f = mul(c(LN2), u)
            elif op == "expn":
                f = neg(u)
            elif op == "exp10n":
                f = mul(c(-LN10), u)
            elif op == "exp2n":
                f = mul(c(-LN2), u)
            elif op == "log":
                f = un("rcp", A)
            elif op == "log10":
                f = mul(c(1.0/LN10), un("rcp", A))
            elif op == "log2":
                f = mul(c(1.0/LN2), un("rcp", A))
            elif op == "log1p":
                f = un("rcp", add(c(1.0), A))
            elif op == "expm1":
                f = add(u, c(1.0))
            elif op == "sin":
                f = un("cos", A)
            elif op == "cos":
                f = neg(un("sin", A))
            elif op == "tan":
                f = add(c(1.0), mul(u, u))
            elif op == "tanh":
                f = sub(c(1.0), mul(u, u))
            elif op == "sinh":
                f = un("cosh", A)
            elif op == "cosh":
                f = un("sinh", A)
            elif op == "atan":
                f = un("rcp", add(c(1.0), mul(A, A)))
            elif op in ("sign", "step"):
                f = None
            else:
                raise LoweringError("no derivative rule for op %r" % op)
            out = {}
            for k, v in da.items():
                w = mul(f, v)
                if w is not None and not isc(w, 0.0):
                    out[k] = w
            d[i] = out
        partial = [{k: v.i for k, v in d[o].items()} for o in self.outputs]
        return Gradient(g2, [new[o].i for o in self.outputs], partial, self.S, n_primal, wrt)

    # ---- homogeneity in (x, P): may the node function hand over the unnormalised composition?
    def xp_invariant(self):
        """True when every rate is unchanged under (x, P) -> (lambda x, P/lambda), lambda > 0, and SpCoi is not read: the
        rates then depend on the composition only through the partial pressures x_i P, and the node function may pass
        the clamped state for x and P/sum(state) for P without ever forming the mole fractions (csrc/kernels/20_node_n2.inc,
        RMT_NODE_NO_X).  Degree bookkeeping over the DAG: x_i has degree +1, P degree -1, constants, T and the user
        parameters degree 0; products and quotients add and subtract degrees, sums (and min / max) need equal degrees,
        integer powers and square roots scale them, every other function needs degree 0."""
        from fractions import Fraction
        g = self.g
        deg = {}
        for i in self.order:
            op, a, b = g.nodes[i]
            if op == "const":
                d = Fraction(0)
            elif op == "in":
                if a[0] == "C":
                    return False
                d = Fraction(1) if a[0] == "x" else (Fraction(-1) if a == "P" else Fraction(0))
            elif op == "mul":
                d = deg[a] + deg[b]
            elif op == "div":
                d = deg[a] - deg[b]
            elif op == "rcp":
                d = -deg[a]
            elif op in ("neg", "abs"):
                d = deg[a]
            elif op in ("add", "sub", "min", "max"):
                if deg[a] != deg[b]:
                    return False
                d = deg[a]
            elif op == "powi":
                d = deg[a]*b
            elif op == "sqrt":
                d = deg[a]/2
            elif op == "pow":
                if deg[b] != 0 or (deg[a] != 0 and not g.is_const(b)):
                    return False
                d = deg[a]*Fraction(g.cval(b)) if g.is_const(b) else Fraction(0)
            else:                                         # exp, log, trigonometric functions, sign, step, ...
                if deg[a] != 0:
                    return False
                d = Fraction(0)
            deg[i] = d
        return all(deg[o] == 0 for o in self.outputs)

    # ---- one reciprocal for independent divisions
    DIV_BATCH_CAP = 4

    def div_groups(self, cap=None):
        """Divisions of the DAG that can share ONE reciprocal: lists of ``div`` / ``rcp`` node ids (id order, at least two,
        at most ``cap`` = DIV_BATCH_CAP each).  v_rcp_f64 issues at a quarter of the FMA rate and every reciprocal carries
        its Newton steps, so n reciprocals 1/d_1 .. 1/d_n are cheaper as a prefix-product inversion: p_k = d_1 .. d_k,
        t = 1/p_n, then 1/d_k = t_k p_(k-1), t_(k-1) = t_k d_k going down - one reciprocal and 3(n-1) multiplications.

        A division joins a group only when its denominator exists before the group's FIRST division (node ids are
        creation-ordered, so such a denominator cannot depend on any member's result); the group's reciprocals are
        printed right there, at its first division - no denominator is evaluated earlier than in the plain emission.
        Left alone: constant denominators, 1/T (comes with the node state) and temperature-only denominators (they
        belong to the cached section of a caching stepper, see kcache_plan).

        Dynamic range: the product of up to four denominators can overflow or underflow where each quotient alone
        would not.  With the fp64 device rmt_rcp (its Newton steps turn rcp(inf) and rcp(0) into NaN) the rates are then
        non-finite and the reactor ends in FLAG_NONFINITE.  A plain 1.0/b (host emulation, RMT_FAST_MATH 0) and
        v_rcp_f32 return 0 for an overflowed product: finite, wrong rates without a flag - which is why
        plan.Mechanism.source never asks for the pass in fp32 (include/rmt_n2.h has the figures).
        ``emit(div_batch=False)`` (plan.Mechanism.source with RMT_DIV_BATCH 0 among its defines: a switch of the
        generator, the kernel source never reads it) keeps one reciprocal per division."""
        cap = self.DIV_BATCH_CAP if cap is None else int(cap)
        tonly = self.t_only()
        groups = []
        for i in self.order:
            if self.g.nodes[i][0] not in ("div", "rcp"):
                continue
            d = self.denominator(i)
            if tonly[d]:
                continue
            for grp in groups:
                if len(grp) < cap and d < grp[0]:
                    grp.append(i)
                    break
            else:
                groups.append([i])
        return [grp for grp in groups if len(grp) >= 2]

    def denominator(self, i):
        """the node a ``div`` / ``rcp`` node divides by"""
        op, a, b = self.g.nodes[i]
        if op not in ("div", "rcp"):
            raise ValueError("node %d is no division" % i)
        return b if op == "div" else a

    # ---- cache of the temperature-only transcendentals ("K-cache")
    KC_THR = 2.0**-9      # |d| <= 2^-9: the degree-4 Taylor sum of e^d is exact to 2.4e-16, log1p to degree 5 to 1e-17
    _EXP_ROOTS = {"exp": (1.0, 1.0), "expn": (-1.0, 1.0), "exp10": (1.0, math.log(10.0)),
                  "exp10n": (-1.0, math.log(10.0)), "exp2": (1.0, math.log(2.0)), "exp2n": (-1.0, math.log(2.0))}

    def kcache_plan(self, gen=True):
        """Which nodes of the DAG are worth caching per mesh node between right-hand-side evaluations.

        Rate and equilibrium constants depend on the temperature only - K = exp(f(T)), Arrhenius f = -E/(R T) - and
        they are the expensive part of a kinetics evaluation (9 of the 13 transcendentals of the DME mechanism, 29 % of
        the bench kernel's time), while T at a mesh node moves by millikelvins between RK stages and time steps.  With
        K_ref = K(T_ref) kept per node,  K(T) = K_ref e^d,  d = f(T) - f(T_ref)  is a 4-term Taylor sum as long as
        |d| <= 2^-9 (5 fp64 operations instead of 10 + a dependent table look-up); log(T) likewise through log1p.  A
        wave whose lanes all pass that test takes the short path, otherwise the wave evaluates in full and moves its
        reference point (cache refresh) - so the result never depends on the cache beyond the 2.4e-16 of the Taylor
        remainder and the rounding of d (|f| 2e-16 absolute, i.e. ~1e-14 relative in K).

        Returns None when there is nothing to cache, else a dict: ``roots`` (node ids, creation order), ``kind`` per
        root ("log", ("lin", coef) = exponent linear in 1/T with that coefficient, or "gen" = exponent stored),
        ``slot`` / ``fslot`` (cache slot of the value / of a "gen" exponent), ``slots`` (doubles per mesh node),
        ``branch`` (nodes evaluated inside the cached section, roots included), ``prologue`` (their root-free
        T-only ancestors, evaluated before it).  ``gen=False`` leaves the "gen" constants (two slots each) out of the
        cache: they are evaluated in full on either path (their log(T) still comes from the cache).

        ``gen="basis"``: an exponent that is a LINEAR COMBINATION of T^n (|n| <= 4) and log T - the usual form of an
        equilibrium constant, ln K = a/T + b ln T + c T + d T^2 + ... - needs no stored exponent: f(T) - f(T_ref) is the
        same combination of the differences of the basis functions, which follow from T - T_ref, 1/T - 1/T_ref and
        log1p(T/T_ref - 1) in a handful of operations shared by all such constants.  kind = ("basis", {key: coef}) with
        keys ("p", n) / ("log",), one slot each; ``tslot`` = slot of T_ref (when a positive power occurs).  Exponents that
        do not decompose stay out of the cache.  ``outside_exp``: True when some exp-family node of the DAG is NOT a
        root (its evaluation needs the exp table whatever the path)."""
        g, live, operands = self.g, self.order, self.g.operands
        tonly = self.t_only()
        def lin_in_invT(i):
            """coefficient c if node i is exactly c/T through products with constants and negations, else None."""
            op, a, b = g.nodes[i]
            if op == "rcp" and g.nodes[a] == ("in", "T", None):
                return 1.0
            if op == "neg":
                c = lin_in_invT(a)
                return None if c is None else -c
            if op == "mul":
                for k, x in ((a, b), (b, a)):
                    if g.is_const(k):
                        c = lin_in_invT(x)
                        if c is not None:
                            return g.cval(k)*c
            if op == "div" and g.is_const(a) and g.nodes[b] == ("in", "T", None):
                return g.cval(a)
            return None
        memo = {}
        def basis(i):
            """{key: coef} if node i is a linear combination of T^n and log T (constant term under ("c",)), else None."""
            if i in memo:
                return memo[i]
            op, a, b = g.nodes[i]
            out = None
            mono = lambda d: d is not None and len(d) == 1 and next(iter(d))[0] in ("p", "c")
            def scaled(d, c):
                return None if d is None else {k: v*c for k, v in d.items()}
            def times(x, y):                      # monomial x monomial
                (kx, cx), (ky, cy) = next(iter(x.items())), next(iter(y.items()))
                n = (kx[1] if kx[0] == "p" else 0) + (ky[1] if ky[0] == "p" else 0)
                return {(("p", n) if n else ("c",)): cx*cy}
            if op == "const":
                out = {("c",): g.cval(i)}
            elif op == "in":
                out = {("p", 1): 1.0} if a == "T" else None
            elif op == "log":
                out = {("log",): 1.0} if g.nodes[a] == ("in", "T", None) else None
            elif op == "neg":
                out = scaled(basis(a), -1.0)
            elif op in ("add", "sub"):
                x, y = basis(a), basis(b)
                if x is not None and y is not None:
                    out = dict(x)
                    for k, v in y.items():
                        out[k] = out.get(k, 0.0) + (v if op == "add" else -v)
            elif op == "mul":
                x, y = basis(a), basis(b)
                if x is not None and y is not None:
                    if set(x) == {("c",)}:
                        out = scaled(y, x[("c",)])
                    elif set(y) == {("c",)}:
                        out = scaled(x, y[("c",)])
                    elif mono(x) and mono(y):
                        out = times(x, y)
                    elif mono(x) and all(k[0] in ("p", "c") for k in y):
                        out = {}
                        for k, v in y.items():
                            out.update(times(x, {k: v}))
                    elif mono(y) and all(k[0] in ("p", "c") for k in x):
                        out = {}
                        for k, v in x.items():
                            out.update(times(y, {k: v}))
            elif op in ("rcp", "div"):
                den = basis(a if op == "rcp" else b)
                num = {("c",): 1.0} if op == "rcp" else basis(a)
                if mono(den) and num is not None and next(iter(den.values())) != 0.0 \
                        and all(k[0] in ("p", "c") for k in num):
                    (kd, cd), = den.items()
                    inv = {(("p", -kd[1]) if kd[0] == "p" else ("c",)): 1.0/cd}
                    out = {}
                    for k, v in num.items():
                        out.update(times(inv, {k: v}))
            elif op == "powi":
                x = basis(a)
                if mono(x):
                    (kx, cx), = x.items()
                    n = (kx[1] if kx[0] == "p" else 0)*b
                    out = {(("p", n) if n else ("c",)): cx**b}
            if out is not None and not all(math.isfinite(v) for v in out.values()):
                out = None
            memo[i] = out
            return out
        roots = []
        bases, lins = {}, {}
        for i in live:
            op, a, b = g.nodes[i]
            if op in self._EXP_ROOTS and tonly[a] and not g.is_const(a):
                d = basis(a)                      # (an additive constant in the exponent drops out of every difference)
                d = None if d is None else {k: v for k, v in d.items() if k != ("c",) and v != 0.0}
                c = lin_in_invT(a)
                if c in (None, 0.0) and d and set(d) == {("p", -1)}:
                    c = d[("p", -1)]              # c/T + const: Arrhenius written relative to a reference temperature
                if c not in (None, 0.0) and math.isfinite(c):
                    lins[i] = c
                    roots.append(i)
                elif gen is True:
                    roots.append(i)
                elif gen == "basis" and d and all(k == ("log",) or 1 <= abs(k[1]) <= 4 for k in d):
                    bases[i] = d
                    roots.append(i)
            elif op == "log" and g.nodes[a] == ("in", "T", None):
                roots.append(i)
        if not roots:
            return None
        rootset = set(roots)
        dep = {}                      # depends on a root (strictly below it)
        for i in live:
            dep[i] = any(dep[o] or o in rootset for o in operands(i))
        need, stack = set(), [g.nodes[r][1] for r in roots]
        while stack:                  # ancestors of the roots' arguments
            i = stack.pop()
            if i in need:
                continue
            need.add(i)
            stack.extend(operands(i))

        kind, slot, fslot, nslots = {}, {}, {}, 1          # slot 0: 1/T_ref
        for r in roots:
            op, a, b = g.nodes[r]
            slot[r] = nslots
            nslots += 1
            if op == "log":
                kind[r] = "log"
                continue
            if r in lins:
                kind[r] = ("lin", lins[r])
            elif r in bases:
                kind[r] = ("basis", bases[r])
            else:
                kind[r] = "gen"
                fslot[r] = nslots
                nslots += 1
        tslot = None
        if any(k[0] == "p" and k[1] > 0 for d in bases.values() for k in d):
            tslot = nslots
            nslots += 1
        branch = [i for i in live if i in rootset or (i in need and dep[i] and not g.is_const(i))]
        prologue = [i for i in live if i in need and not dep[i] and i not in rootset]
        outside = any(g.nodes[i][0] in self._EXP_ROOTS and i not in rootset for i in live)
        return {"roots": roots, "kind": kind, "slot": slot, "fslot": fslot, "slots": nslots, "branch": branch,
                "prologue": prologue, "tslot": tslot, "outside_exp": outside}

    def emit(self, fname="rmt_kinetics", const_table=False, kcache=False, kcache_gen=True, kcache_thr=None,
             div_batch=False, kcache_fold=False, rate_scale=False, extra_den=False, head=True):
        """The text of the device function of the rates; the switches are those of emit.Emission."""
        return Emission(self, fname, const_table, kcache, kcache_gen, kcache_thr, div_batch, kcache_fold, rate_scale,
                        extra_den, head).text

    def fold_plan(self, plan, rate_scale=False):
        """Emission(kcache_fold=True) -> ({cached constant: literal applied before kc.put}, {node: node it copies}, the
        cached constants that carry `rscale`).  ``rate_scale``: look for one such constant per rate; the last set is
        empty when some rate has none (nothing is scaled then) and without the switch."""
        g = self.g
        users = {n: [u for u, _ in us] for n, us in self.users().items()}
        kinds, branch = plan["kind"], set(plan["branch"])
        cached = [r for r in plan["roots"] if kinds[r] != "log"]
        scale, copy, scaled = {}, {}, set()

        def literal_of(u, r):
            """(literal, {node: copied node}) if consumer u multiplies r by a literal, directly or as r * (X * c)"""
            op, a, b = g.nodes[u]
            if op != "mul" or a == b or u in branch:
                return None
            o = b if a == r else a
            if g.is_const(o):
                return g.cval(o), {u: r}
            oop, oa, ob = g.nodes[o]
            if oop == "mul" and users.get(o) == [u] and o not in branch and g.is_const(oa) != g.is_const(ob):
                c, X = (oa, ob) if g.is_const(oa) else (ob, oa)
                return g.cval(c), {o: X}
            return None
        for r in cached:
            us = users.get(r, [])
            found = [literal_of(u, r) if u >= 0 else None for u in us]
            if not found or any(f is None for f in found) or len({f[0] for f in found}) != 1:
                continue
            c = found[0][0]
            if not math.isfinite(c) or c == 0.0:
                continue
            scale[r] = c
            for f in found:
                copy.update(f[1])
        if rate_scale:
            def carrier(n):
                """the cached constant at the end of a chain of single-use products below node n"""
                if n in cached:
                    return n
                op, a, b = g.nodes[n]
                if op != "mul" or n in branch:
                    return None
                for o in (a, b):
                    if len(users.get(o, [])) == 1 and not g.is_const(o):
                        r = carrier(o)
                        if r is not None:
                            return r
                return None
            carriers = [carrier(o) if users.get(o) == [-1] else None for o in self.outputs]
            if carriers and all(r is not None for r in carriers) and len(set(carriers)) == len(carriers):
                scaled = set(carriers)
                for r in carriers:
                    scale.setdefault(r, 1.0)
        return scale, copy, scaled


class Gradient(Lowered):
    """Rates and their non-zero partial derivatives with respect to the node inputs (T, x_i, C_i)."""

    def __init__(self, graph, outputs, partial, nspecies, n_primal, wrt):
        self.partial, self.n_primal, self.wrt = partial, n_primal, wrt
        self.n_rates = len(outputs)
        flat = list(outputs)
        for p in partial:
            flat.extend(p.values())
        Lowered.__init__(self, graph, flat, nspecies)
        self.rate_outputs = list(outputs)

    def evaluate_all(self, T, P, x, C, U=()):
        """(rates, [{input: d rate / d input}]) on the host - for the tests of the gradient itself."""
        vals = self.evaluate(T, P, x, C, U)
        R = self.n_rates
        out, pos = [], R
        for p in self.partial:
            out.append({k: vals[pos + n] for n, k in enumerate(p)})
            pos += len(p)
        return vals[:R], out

    def emit_jac(self, fname="rmt_kinetics_jac", with_p=False, with_u=None):
        """The text of the device function of the rates and their partials (emit.JacEmission)."""
        return JacEmission(self, fname, with_p, with_u).text


def trace(VARS, RATES, nspecies, R_CONST=8.314472, fixed=None, params=()):
    """Symbolic run of reactionRateExe (rmtReaction.py:27-58).  ``fixed`` optionally binds inputs
    (e.g. {"T": 523.0}) to literals so that everything depending only on them is folded.
    ``params``: names of scalar VARS entries that stay SYMBOLIC - input ``u<k>`` for params[k] - instead of
    being folded as literals: per-reactor kinetic parameters of an ensemble (a sweep over a catalyst density,
    a pre-exponential factor, an activation energy), read by the kernel from the member row."""
    g = Graph()
    fixed = fixed or {}
    params = list(params)
    for nm in params:
        if nm not in VARS or not is_scalar_constant(VARS[nm]):
            raise LoweringError("VARS[%r] cannot be a per-reactor parameter: it is not a scalar constant" % (nm,))

    def leaf(nm):
        return g.const(fixed[nm]) if nm in fixed else g.inp(nm)

    loopDict = {
        "R_CONST": R_CONST,
        "T": leaf("T"),
        "P": leaf("P"),
        "MoFri": SymVector([g.inp("x%d" % i) for i in range(nspecies)]),
        "SpCoi": SymVector([g.inp("C%d" % i) for i in range(nspecies)]),
    }
    merged = {**loopDict, **VARS}
    memo = {}
    exe = {}
    for k, v in merged.items():
        if isinstance(v, types.FunctionType):
            try:
                exe[k] = rebind(v, memo)(exe)
            except LoweringError:
                raise
            except Exception as e:
                raise LoweringError("cannot trace VARS[%r]: %s: %s" % (k, type(e).__name__, e)) from e
        elif k in params:
            exe[k] = g.inp("u%d" % params.index(k))
        else:
            exe[k] = v
    outs = []
    for k, fn in RATES.items():
        try:
            val = rebind(fn, memo)(exe)
        except LoweringError:
            raise
        except Exception as e:
            raise LoweringError("cannot trace RATES[%r]: %s: %s" % (k, type(e).__name__, e)) from e
        if not isinstance(val, Sym):
            if not _num(val):
                raise LoweringError("RATES[%r] returned %r" % (k, type(val)))
            val = g.const(float(val))
        outs.append(val.i)
    return Lowered(g, outs, nspecies)
