"""HIP C++ text of a lowered DAG (lowering.Lowered / lowering.Gradient, taken as arguments): straight-line code, one
``const real vN = ...;`` per node, as the device functions `rmt_kinetics`, `rmt_kinetics_node` and `rmt_kinetics_jac`.

Everything that belongs to ONE emission - the constant table, the division groups and the names of their reciprocals, the
caller's extra denominator, the fold plan, the Taylor range, the tests already printed - lives in an ``Emission``; the DAG
it prints is only read, so one DAG serves any number of emissions in any order."""
import math

from .dag import FLAG_DIV0, FLAG_DOMAIN, LoweringError

_INLINE = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0)      # hardware inline constants: never through the table
_TAYLOR = ("k_ + (k_ * d_) * (real(1) + d_ * (real(0.5) + d_ * (real(%r) + d_ * real(%r))))" % (1.0/6.0, 1.0/24.0))


def _lit(v, table):
    if math.isnan(v):
        return "real(__builtin_nan(\"\"))"
    if math.isinf(v):
        return "real(__builtin_inf())" if v > 0 else "real(-__builtin_inf())"
    v = float(v)
    # experiment (const_table): constants that are not hardware inline constants come from a __constant__ table
    # (scalar loads) instead of s_mov literal pairs
    if table is not None and v not in _INLINE:
        return "real(RMT_KTAB[%d])" % table.setdefault(v, len(table))
    return "real(%s)" % repr(v)


class _Lines:
    """The per-node emitter and its state.  ``table``: the constant table (None: literals), ``groups``: the division
    groups that share a reciprocal, ``extra``: (denominator, out-parameter) of the caller, see Emission extra_den.  Nodes
    with an id >= ``nocheck_from`` (the derivative part of a gradient DAG) are printed without the Python-exception
    tests: they are not expressions the reference evaluates."""

    def __init__(self, dag, table=None, groups=(), extra=None, nocheck_from=None):
        self.dag, self.table, self.extra, self.nocheck_from = dag, table, extra, nocheck_from
        self.name = {}                 # node -> its C expression
        self.seen_checks = set()
        self.batch = {n: grp for grp in groups for n in grp}      # division node -> its group (div_batch only)
        self.inv = {}                  # division node -> name of the reciprocal of its denominator
        self.extra_done = False        # (extra: (denominator, out-parameter) of the caller, see extra_den)

    def group_lines(self, grp):
        """the prefix-product inversion of a group (div_groups), printed at its first division"""
        den = [self.name[self.dag.denominator(n)] for n in grp]
        ride = self.extra and not self.extra_done         # the caller's own denominator rides along (extra_den)
        if ride:
            den.append(self.extra[0])
        tag, n = "b%d" % grp[0], len(den)
        out, prod = [], den[0]
        for k in range(1, n):                             # p_k = d_1 .. d_(k+1)
            out.append("    const real %s_p%d = %s * %s;" % (tag, k, prod, den[k]))
            prod = "%s_p%d" % (tag, k)
        out.append("    const real %s_t%d = rmt_rcp(%s);" % (tag, n - 1, prod))
        for k in range(n - 1, 0, -1):                     # 1/d_(k+1) = t_k p_(k-1),  t_(k-1) = t_k d_(k+1)
            below = den[0] if k == 1 else "%s_p%d" % (tag, k - 1)
            out.append("    const real %s_i%d = %s_t%d * %s;" % (tag, k, tag, k, below))
            if k > 1:
                out.append("    const real %s_t%d = %s_t%d * %s;" % (tag, k - 1, tag, k, den[k]))
            else:
                out.append("    const real %s_i0 = %s_t1 * %s;" % (tag, tag, den[1]))
            if k < len(grp):
                self.inv[grp[k]] = "%s_i%d" % (tag, k)
        self.inv[grp[0]] = "%s_i0" % tag
        if ride:
            out.append("    %s = %s_i%d;" % (self.extra[1], tag, n - 1))
            self.extra_done = True
        return out

    def node(self, i, indent="    ", declare=True, nocheck=False, exp_sel=False):
        """Lines of HIP C++ for live node i (its C expression goes to ``name``).  ``declare`` False prints an assignment
        to an already declared ``v<i>`` instead of a ``const real`` definition (nodes evaluated inside a branch and used
        after it).  ``exp_sel``: the table-driven exp goes through rmt_exp_sel<KC::enabled> (00_config_math.inc) - a full
        evaluation made on behalf of a cache, whose kernel may keep a smaller exp table than the rest."""
        g, name, inv = self.dag.g, self.name, self.inv
        lines = []
        op, a, b = g.nodes[i]
        if op == "const":
            name[i] = _lit(g.cval(i), self.table)
            return lines
        if op == "in":
            name[i] = a if a in ("T", "P") else ("x[%s]" % a[1:] if a[0] == "x" else (
                "U[%s]" % a[1:] if a[0] == "u" else "C[%s]" % a[1:]))
            return lines
        v = "v%d" % i
        A = name[a]
        B = name[b] if (b is not None and op != "powi") else None
        sel = "_sel<KC::enabled>" if exp_sel else ""
        pre = []
        if i in self.batch and i not in inv:              # the first division of a group: its reciprocals, all at once
            if not declare:
                raise LoweringError("a batched division inside the cached section")
            lines.extend(self.group_lines(self.batch[i]))
        if op == "add":
            e = "%s + %s" % (A, B)
        elif op == "sub":
            e = "%s - %s" % (A, B)
        elif op == "mul":
            e = "%s * %s" % (A, B)
        elif op == "div":
            pre.append("RMT_CHECK_DEN(flag, %s);" % B)
            e = "%s * %s" % (A, inv[i]) if i in inv else "rmt_div(%s, %s)" % (A, B)
        elif op == "rcp":
            pre.append("RMT_CHECK_DEN(flag, %s);" % A)
            e = "invT" if A == "T" else (inv[i] if i in inv else "rmt_rcp(%s)" % A)     # 1/T comes with the node state
        elif op == "expn":      # stands for 1/exp(A): Python raises if exp(A) overflows or is 0
            pre.append("RMT_CHECK_EXP(flag, rmt_abs(%s));" % A)
            e = "rmt_exp%s(-%s)" % (sel, A)
        elif op in ("exp10n", "exp2n"):
            k = {"exp10n": math.log(10.0), "exp2n": math.log(2.0)}[op]
            pre.append("RMT_CHECK_EXP(flag, rmt_abs(%s) * real(%r));" % (A, k))
            e = "rmt_%s%s(-%s)" % (op[:-1], sel, A)
        elif op == "neg":
            e = "-%s" % A
        elif op == "abs":
            e = "rmt_abs(%s)" % A
        elif op == "powi":
            # binary powering with named squares
            terms, sq, k, sqname = [], abs(b), 0, A
            while sq:
                if sq & 1:
                    terms.append(sqname)
                sq >>= 1
                if sq:
                    k += 1
                    nm = "%s_s%d" % (v, k)
                    pre.append("const real %s = %s * %s;" % (nm, sqname, sqname))
                    sqname = nm
            prod = " * ".join(terms)
            if b < 0:
                pre.append("RMT_CHECK_DEN(flag, %s);" % A)
                e = "rmt_rcp(%s)" % prod
            else:
                e = prod
        elif op == "pow":
            pre.append("RMT_CHECK(flag, %s < real(0) && %s != trunc(%s), %du);" % (A, B, B, FLAG_DOMAIN))
            pre.append("RMT_CHECK(flag, %s == real(0) && %s < real(0), %du);" % (A, B, FLAG_DIV0))
            e = "rmt_pow(%s, %s)" % (A, B)
        elif op in ("log", "log10", "log2", "log1p"):
            pre.append("RMT_CHECK_POS(flag, %s);" % (A if op != "log1p" else "(%s + real(1))" % A))
            e = "rmt_%s(%s)" % (op, A)
        elif op == "sqrt":
            pre.append("RMT_CHECK_NONNEG(flag, %s);" % A)
            e = "rmt_sqrt(%s)" % A
        elif op in ("exp", "exp10", "exp2", "expm1", "sinh", "cosh"):
            # one running maximum against exp's limit 709.78: scale the other bases' arguments
            scale = {"exp10": math.log(10.0), "exp2": math.log(2.0)}.get(op)
            arg = A if op not in ("sinh", "cosh") else "rmt_abs(%s)" % A
            pre.append("RMT_CHECK_EXP(flag, %s);" % (arg if scale is None else "%s * real(%r)" % (arg, scale)))
            e = "rmt_%s%s(%s)" % (op, sel if op in ("exp", "exp10", "exp2") else "", A)
        elif op in ("sin", "cos", "tan", "tanh", "atan"):
            e = "rmt_%s(%s)" % (op, A)
        elif op in ("min", "max"):
            e = "rmt_%s(%s, %s)" % (op, A, B)
        elif op == "sign":
            e = "(%s > real(0) ? real(1) : (%s < real(0) ? real(-1) : real(0)))" % (A, A)
        elif op == "step":
            e = "(%s >= real(0) ? real(1) : real(0))" % A
        else:
            raise LoweringError("no device emission for op %r" % op)
        for p in pre:
            if p.startswith("RMT_CHECK"):
                if nocheck or p in self.seen_checks or (self.nocheck_from is not None and i >= self.nocheck_from):
                    continue
                if declare:               # (a check printed inside a branch does not cover the code after it)
                    self.seen_checks.add(p)
            lines.append(indent + p)
        lines.append(indent + ("const real %s = %s;" if declare else "%s = %s;") % (v, e))
        name[i] = v
        return lines

    def body(self):
        """straight-line code for every live node"""
        lines = []
        for i in self.dag.order:
            lines.extend(self.node(i))
        return lines


class Emission(_Lines):
    """The device function of the rates: ``text``, with ``slots`` (doubles per mesh node its cached section keeps, 0
    without one) and ``rates_scaled`` (whether the function has the parameter `rscale`, see below).

    ``kcache``: with the cached section of kcache_plan() for callers that pass a cache (template parameter KC with
    KC::enabled; every other caller passes rmt_nocache_t and gets the plain evaluation - the section is discarded at
    compile time).  ``div_batch``: independent divisions share one reciprocal (div_groups; plan.Mechanism.source switches
    it on unless RMT_DIV_BATCH 0 is among its defines).

    Three more, for the node function of a caching stepper (plan.Mechanism.node_kinetics, `rmt_kinetics_node`), each off
    by default - the text of the calls above does not change:
    ``kcache_fold``: a literal factor that every consumer of a cached constant multiplies onto it is applied ONCE, in
    the full evaluation before `kc.put` (K c obeys the same Taylor update as K); the consumer becomes a copy.  Covers
    a chain of literal factors behind the constant, v19 * (v116 * c), too.  Slots and range tests do not change.
    ``rate_scale`` (with kcache_fold): one more parameter `const real rscale`; every rate leaves multiplied by it,
    through one cached constant of the rate's product chain (its literal times rscale goes in before `kc.put`, so the
    cached evaluations pay nothing; rscale must not change while a cache is in use) - if some rate has no such chain
    nothing is scaled, there is no such parameter and ``rates_scaled`` is False.
    ``extra_den``: two more parameters `const real gden, real& ginv` (behind rscale); 1/gden joins the first division group as one
    more member of its prefix-product inversion (a plain reciprocal where there is no group).  gden must exist before
    the call and be positive; the product's range is the caller's business."""

    def __init__(self, dag, fname="rmt_kinetics", const_table=False, kcache=False, kcache_gen=True, kcache_thr=None,
                 div_batch=False, kcache_fold=False, rate_scale=False, extra_den=False, head=True):
        _Lines.__init__(self, dag, {} if const_table else None, dag.div_groups() if div_batch else (),
                        ("gden", "ginv") if extra_den else None)
        plan = dag.kcache_plan(kcache_gen) if kcache else None
        self.thr = dag.KC_THR
        if kcache_thr is not None:        # (tests: a smaller range makes the callers' out-of-range handling run)
            if not 0.0 < float(kcache_thr) <= dag.KC_THR:
                raise ValueError("the cache's Taylor range must lie in (0, 2^-9]")
            self.thr = float(kcache_thr)
        self.scale, self.copy, self.scaled = dag.fold_plan(plan, rate_scale) if (plan and kcache_fold) else ({}, {}, set())
        self.rates_scaled = bool(self.scaled)
        self.slots = plan["slots"] if plan else 0
        lines = self.body() if plan is None else self.cached(plan)
        if self.extra and not self.extra_done:            # no division group to join
            lines.insert(0, "    ginv = rmt_rcp(gden);")
        body, decl = "\n".join(lines), ""
        if self.table:
            vals = sorted(self.table, key=self.table.get)
            body = "    // literals through the scalar cache\n" + body
            decl = "__constant__ double RMT_KTAB[%d] = {%s};\n" % (len(vals), ", ".join(repr(v) for v in vals))
        outs = "\n".join("    r[%d] = %s;" % (k, self.name[o]) for k, o in enumerate(dag.outputs))
        self.text = ("#define RMT_KC_SLOTS %d\n" % self.slots if head else "") + decl + (
            "template <typename FL, typename KC, int MODE = 0>\n"
            "__device__ __forceinline__ void %s(const real T, const real invT, const real P,\n"
            "        const real* __restrict__ x, const real* __restrict__ C, const real* __restrict__ U,\n"
            "        real* __restrict__ r, FL& flag, KC& kc%s) {\n"
            "    (void)invT; (void)U; (void)kc;\n%s\n%s\n}\n"
            % (fname, (", const real rscale" if self.rates_scaled else "") + (", const real gden, real& ginv" if extra_den else ""),
               body, outs))

    def cached(self, plan):
        """Body with the cached section: MODE 2 takes every cached constant from its reference value by a Taylor step
        and tests the range that step serves - |d| <= KC_THR in every exponent, |T/T_ref - 1| <= KC_THR for log(T) - a
        lane out of range only marks its cache (`kc.leave`: there is no second code path, the CALLER discards what it
        computed from such an evaluation, see csrc/kernels/50_rk4.inc rmt_rk4_reg_body); MODE 0 evaluates in full and
        (with a cache) stores the new reference point."""
        dag, g, name = self.dag, self.dag.g, self.name
        lines = []
        for i in dag.order:                               # constants and inputs have no code: name them first
            if g.nodes[i][0] in ("const", "in"):
                self.node(i)
        done = set(name)
        for i in plan["prologue"]:
            if i not in done:
                lines.extend(self.node(i))
                done.add(i)
        for i in plan["branch"]:                          # values that leave the cached section
            lines.append("    real v%d;" % i)
        thr = repr(self.thr)
        kinds, slot, fslot = plan["kind"], plan["slot"], plan["fslot"]

        def factor(r):
            """d(exponent of e) / d(argument) of the exp-family root r"""
            sg, lnb = dag._EXP_ROOTS[g.nodes[r][0]]
            return sg*lnb
        lin = [abs(factor(r)*kinds[r][1]) for r in plan["roots"] if isinstance(kinds[r], tuple) and kinds[r][0] == "lin"]
        bases = {r: kinds[r][1] for r in plan["roots"] if isinstance(kinds[r], tuple) and kinds[r][0] == "basis"}
        powers = sorted({k[1] for d in bases.values() for k in d if k[0] == "p"})
        want_log = any(k == "log" for k in kinds.values()) or any(("log",) in d for d in bases.values())
        L = lines.append
        L("    if constexpr (KC::enabled && MODE == 2) {      // every constant from its cached value: K = K_ref e^d, d = f(T) - f(T_ref)")
        L("        const real kc_it = kc.get(0);")
        L("        const real kc_di = invT - kc_it;")
        L("        (void)kc_di;")
        tests = []                                        # the range test sits next to the values it shares with the Taylor steps
        if lin:
            tests.append("!(rmt_abs(kc_di) <= real(%r))" % (self.thr/max(lin)))
        if want_log:
            L("        const real kc_s = T * kc_it - real(1);")
            L("        const real kc_dl = kc_s * (real(1) + kc_s * (real(-0.5) + kc_s * (real(%r) + kc_s * (real(-0.25) + kc_s * real(0.2)))));      // log(T) - log(T_ref) = log1p(T/T_ref - 1)"
              % (1.0/3.0))
            tests.append("!(rmt_abs(kc_s) <= real(%r))" % self.thr)
        if tests:
            L("        kc.leave(%s);" % " || ".join(tests))
        # differences of the basis functions of the ("basis", ...) exponents: T^n - T_ref^n from (T - T_ref) or (1/T - 1/T_ref)
        dname = {("log",): "kc_dl"}
        if any(n > 0 for n in powers):
            L("        const real kc_tr = kc.get(%d);" % plan["tslot"])
            L("        const real kc_dt = T - kc_tr;")
        for n in powers:
            x, xr, dx = ("T", "kc_tr", "kc_dt") if n > 0 else ("invT", "kc_it", "kc_di")
            m = abs(n)
            nm = "kc_d%s%d" % ("p" if n > 0 else "m", m)
            dname[("p", n)] = nm
            if m == 1:
                L("        const real %s = %s;" % (nm, dx))
            elif m == 2:
                L("        const real %s = %s * (%s + %s);" % (nm, dx, x, xr))
            elif m == 3:
                L("        const real %s = %s * (%s * (%s + %s) + %s * %s);" % (nm, dx, x, x, xr, xr, xr))
            else:
                L("        const real %s = (%s * (%s + %s)) * (%s * %s + %s * %s);" % (nm, dx, x, xr, x, x, xr, xr))
        # ... consumed at once: only the exponents' changes stay live (one value per constant), with ONE range test for all
        # of them (a NaN exponent implies a NaN temperature, which the tests above catch)
        dmax = []
        for i, d in bases.items():
            terms = " + ".join("real(%r) * %s" % (factor(i)*c, dname[key]) for key, c in d.items())
            L("        const real kc_e%d = %s;" % (i, terms))
            dmax.append("rmt_abs(kc_e%d)" % i)
        if dmax:
            big = dmax[0]
            for t in dmax[1:]:
                big = "rmt_max(%s, %s)" % (big, t)
            L("        kc.leave(!(%s <= real(%s)));" % (big, thr))
        for i in plan["branch"]:
            v = "v%d" % i
            if i not in kinds:
                lines.extend(self.node(i, "        ", declare=False, nocheck=True))
                continue
            k = kinds[i]
            if k == "log":
                L("        %s = kc.get(%d) + kc_dl;" % (v, slot[i]))
            else:
                L("        {")
                if k[0] == "lin":
                    L("            const real d_ = real(%r) * kc_di;" % (factor(i)*k[1]))
                elif k[0] == "basis":
                    L("            const real d_ = kc_e%d;" % i)
                else:
                    L("            const real d_ = real(%r) * (%s - kc.get(%d));" % (factor(i), name[g.nodes[i][1]], fslot[i]))
                    L("            kc.leave(!(rmt_abs(d_) <= real(%s)));" % thr)
                L("            const real k_ = kc.get(%d);" % slot[i])
                L("            %s = %s;" % (v, _TAYLOR))
                L("        }")
            name[i] = v
        L("    } else {                 // full evaluation; with a cache its reference point moves here (every constant is")
        L("        if constexpr (KC::enabled) kc.put(0, invT);      // stored as soon as it exists: short live ranges)")
        if plan.get("tslot") is not None:
            L("        if constexpr (KC::enabled) kc.put(%d, T);" % plan["tslot"])
        for i in plan["branch"]:                          # (a cached exp: the table-driven exp of whoever owns the table)
            lines.extend(self.node(i, "        ", declare=False, exp_sel=i in kinds and kinds[i] != "log"))
            done.add(i)
            if i in self.scale:                               # the literal its consumers would multiply onto it
                c = "real(%r)" % self.scale[i]
                if i in self.scaled:
                    c = "rscale" if self.scale[i] == 1.0 else "(%s * rscale)" % c
                L("        v%d = v%d * %s;" % (i, i, c))
            if i in slot:
                L("        if constexpr (KC::enabled) {")
                L("            kc.put(%d, v%d);" % (slot[i], i))
                if i in fslot:
                    L("            kc.put(%d, %s);" % (fslot[i], name[g.nodes[i][1]]))
                L("        }")
        L("    }")
        if self.rates_scaled:
            L("    // (the rates leave scaled by rscale)")
        for i in dag.order:
            if i not in done:
                if i in self.copy:                            # its literal sits in the cached constant
                    name[i] = name[self.copy[i]]
                else:
                    lines.extend(self.node(i))
                done.add(i)
        return lines


class JacEmission(_Lines):
    """The device function of a Gradient: rates r[R] and the partials drdT[R], drdx[R][S], drdC[R][S] (zeros written as
    literals, which the compiler then removes from the chain rule of the node Jacobian); with_p: also drdP[R] (model N1,
    where the pressure is a state variable - the gradient must have been taken by "P" too); with_u = NU (not None): also
    drdU[R][max(NU, 1)], the partials by the per-reactor inputs u<k> (the sensitivity sweep - the gradient must have been
    taken by them too)."""

    def __init__(self, grad, fname="rmt_kinetics_jac", with_p=False, with_u=None):
        _Lines.__init__(self, grad, nocheck_from=grad.n_primal)
        lines, name = self.body(), self.name
        S = grad.S
        outs = ["    r[%d] = %s;" % (k, name[o]) for k, o in enumerate(grad.rate_outputs)]

        def d(p, key):
            return name[p[key]] if key in p else "real(0)"
        for q, p in enumerate(grad.partial):
            outs.append("    drdT[%d] = %s;" % (q, d(p, "T")))
            if with_p:
                outs.append("    drdP[%d] = %s;" % (q, d(p, "P")))
            for i in range(S):
                outs.append("    drdx[%d][%d] = %s;" % (q, i, d(p, "x%d" % i)))
                outs.append("    drdC[%d][%d] = %s;" % (q, i, d(p, "C%d" % i)))
            for k in range(max(with_u, 1) if with_u is not None else 0):
                outs.append("    drdU[%d][%d] = %s;" % (q, k, d(p, "u%d" % k)))
        self.text = (
            "template <typename FL>\n"
            "__device__ __forceinline__ void %s(const real T, const real invT, const real P,\n"
            "        const real* __restrict__ x, const real* __restrict__ C, const real* __restrict__ U,\n"
            "        real* __restrict__ r,\n"
            "        real* __restrict__ drdT, real (*__restrict__ drdx)[RMT_S], real (*__restrict__ drdC)[RMT_S],%s FL& flag) {\n"
            "    (void)invT; (void)U;\n%s\n%s\n}\n"
            % (fname, (" real* __restrict__ drdP," if with_p else "")
               + (" real (*__restrict__ drdU)[RMT_NU > 0 ? RMT_NU : 1]," if with_u is not None else ""),
               "\n".join(lines), "\n".join(outs)))
