"""Stage-function emission: from a module stack (plugin.py protocol) to the HIP/C++ header the solve kernel compiles.

What CasADi + acados do for the reference at solver-generation time (generate_acados_solver.py:27-65: `cost_expr_ext_cost`,
`con_h_expr`, EXACT Hessian) is done here with sympy: the stage cost and every inequality row are differentiated exactly
(gradient + Hessian), all outputs go through one common-subexpression elimination, and the result is printed as
straight-line C++ that is valid both for hipcc (`__host__ __device__`) and for a host compiler (tests).

Conventions of the emitted code (namespace tmpc_gen):
  * z = [a, w, x, y, psi, v, spline] are the 7 QP variables; with the slack model the 8th model variable `slack` is a
    per-trajectory constant argument;
  * every row is normalised to  g(z) <= 0  (lower-bounded rows h >= lb become lb - h <= 0): the kernel then has
    NH upper-bounded rows and no lower-bounded ones;
  * rows may depend on (x, y, psi) and on the slack only -- true for every constraint module the reference ships;
    the generator refuses anything else, because the kernels keep 3 Jacobian entries per row;
  * the stage cost may depend on all 7 variables (dense 7x7 Hessian, packed lower triangle, index i(i+1)/2 + j).
"""
import re

import numpy as np
import sympy as sp
from sympy.printing.c import C99CodePrinter

from . import plugin
from .jets import JetEmitter, _lit

class UnsupportedStack(ValueError):
    """The module stack / model asks for something the solve kernels do not implement (message says what)."""


class logistic(sp.Function):
    """1 / (1 + exp(-x)) as an atomic function: its derivatives are polynomials in itself, so the emitted gradient and
    Hessian never form exp(u)^k / (1 + exp(u))^m quotients that overflow for the glue sigmoids of spline.py:37
    (|u| reaches ~200 one segment away from a knot)."""
    nargs = 1

    def fdiff(self, argindex=1):
        return self * (1 - self)


def _stabilise(expr):
    """1 / (1 + c exp(w))  ->  logistic(-(w + log c))   (the glue sigmoids; sympy folds exp(u + 0.2) into 1.22 exp(u))."""
    def split(e):
        if not (e.is_Pow and e.exp == -1 and e.base.is_Add and len(e.base.args) == 2):
            return None
        a, b = e.base.args
        one = lambda q: q.is_Number and float(q) == 1.0
        if not one(a):
            a, b = b, a
        if not one(a):
            return None
        coeff, rest = b.as_coeff_Mul()
        if rest.func == sp.exp and coeff.is_Number and coeff > 0:
            return rest.args[0] + sp.log(coeff)
        return None

    return sp.sympify(expr).replace(lambda e: split(e) is not None, lambda e: logistic(-split(e)))


CORE = ["a", "w", "x", "y", "psi", "v", "spline"]
ROW_VARS = (2, 3, 4)            # x, y, psi


class _Printer(C99CodePrinter):
    def _print_Pow(self, expr):
        b, e = expr.as_base_exp()
        if e.is_Integer and 2 <= abs(int(e)) <= 4:
            s = "*".join([self.parenthesize(b, 50)] * abs(int(e)))      # x*x instead of pow(x, 2)
            return f"({s})" if e > 0 else f"(1.0/({s}))"        # always parenthesised: the result may be a denominator
        if e == sp.Rational(1, 2):
            return f"sqrt({self._print(b)})"
        if e == -sp.Rational(1, 2):
            return f"(1.0/sqrt({self._print(b)}))"
        return super()._print_Pow(expr)

    def _print_logistic(self, expr):
        return f"tmpc_gen_logistic({self._print(expr.args[0])})"

    def _print_Max(self, expr):
        a = list(expr.args)
        out = self._print(a[0])
        for x in a[1:]:
            out = f"fmax({out}, {self._print(x)})"
        return out

    def _print_Min(self, expr):
        a = list(expr.args)
        out = self._print(a[0])
        for x in a[1:]:
            out = f"fmin({out}, {self._print(x)})"
        return out


_printer = _Printer({"precision": 17})


def _c(expr):
    s = _printer.doprint(expr)
    s = re.sub(r"\bP_(\d+)_\b", r"p[(size_t)\1 * ps]", s)
    s = re.sub(r"\bZ_(\d+)_\b", r"z[\1]", s)
    return s


def _cse_block(outputs, prefix):
    """outputs: list of (lhs string, expr).  Returns C statements (temporaries + assignments).

    Statement order: every output is followed back through the temporaries it needs (depth first), and a temporary is
    emitted right before its first consumer -- values are born late and die early, which is what keeps the kernels'
    linearisation phase inside the register file (sympy's own order defines all temporaries up front)."""
    exprs = [sp.sympify(e) for _, e in outputs]
    repl, red = sp.cse(exprs, symbols=sp.numbered_symbols(prefix), optimizations="basic", order="none")
    defs = {s_: e for s_, e in repl}
    emitted, lines = set(), []

    def need(expr):
        for s_ in sorted(expr.free_symbols & defs.keys(), key=lambda q: int(str(q)[len(prefix):])):
            if s_ not in emitted:
                need(defs[s_])
                emitted.add(s_)
                lines.append(f"    const double {_c(s_)} = {_c(defs[s_])};")

    for (lhs, _), e in zip(outputs, red):
        need(e)
        lines.append(f"    {lhs} = {_c(e)};")
    return lines


def generate(modules, model, settings, name="generated", method="symbolic", row_shares=False, tick_kernels=3, tick_split=1):
    """Returns dict(header=<C++ text>, params=<plugin.Parameters>, npar, nh, slack, rows=[(module row index, kind)]).
    method: "symbolic" = sympy derivatives + one common-subexpression elimination over all outputs (default: the fastest
    kernels -- 8 % off the hand-written cfg 2 kernel -- but ~30 s of generation for a contouring stack); "jets" = sparse
    forward-mode second-order differentiation at code level (jets.py: under a second of generation, kernels 18 % off the
    hand-written one).  The two are independent implementations and are checked against each other in the tests.
    row_shares: the header a solver LIBRARY is compiled around (build.py): the emitted `rows` takes a share (first, step) and evaluates the row
    blocks k % step == first -- the default (0, 1) is every row --, and the header carries the two constants below.  False: `rows` evaluates
    every row (the header as it was before the tick kernels: stage-function checks on the host, the recorded digest of the reference's scripts).
    tick_kernels: the horizon ranges for which a library compiled around this header instantiates the control-tick kernels (latency mode 3):
    bit 0 = N <= 20, bit 1 = 21 <= N <= 31 (build.py chooses; 0 = none).  tick_split: 1 = the four-wave tick kernels split the stage
    linearisation over their waves (csrc/tmpc_kernels.hpp, the four-wave form of linearise); 0 is for A/B measurements of the split."""
    params = plugin.Parameters()
    plugin.define_parameters(modules, params, settings)
    settings = dict(settings); settings["params"] = params
    npar = params.length()
    nvar = model.get_nvar()
    slack_model = "slack" in model.states
    # model 0: ContouringSecondOrderUnicycleModel (+ slack variant); model 1: SecondOrderUnicycleModel (solver_model.py:170-191: no spline
    # state) -- same unicycle, the kernels' fifth state slot is inert for it (csrc/tmpc_stage.hpp Dims::model); nothing may depend on that slot,
    # which holds by construction here: the model has no name for it, so no module expression can contain Z_6_
    second_order_unicycle = model.inputs + model.states == CORE[:6]
    if not second_order_unicycle and model.inputs + model.states[:5] != CORE:
        raise UnsupportedStack("the kernels integrate the (contouring) second-order unicycle (solver_model.py:170-214); got "
                               f"inputs {model.inputs}, states {model.states}")
    z = [sp.Symbol(f"Z_{i}_", real=True) for i in range(7)]
    slack = sp.Symbol("slack", real=True)
    zfull = (z[:6] if second_order_unicycle else z) + ([slack] if slack_model else [])
    if len(zfull) != nvar:
        raise UnsupportedStack(f"model has {nvar} variables; the kernels support the unicycle (6), the contouring unicycle (7) and its slack variant (8)")
    lb7 = list(model.lower_bound[:6 if second_order_unicycle else 7]) + ([-1.0] if second_order_unicycle else [])
    ub7 = list(model.upper_bound[:6 if second_order_unicycle else 7]) + ([10000.0] if second_order_unicycle else [])
    p = [sp.Symbol(f"P_{i}_", real=True) for i in range(npar)]

    cost = _stabilise(plugin.objective(modules, np.array(zfull, dtype=object), p, model, settings, 1))
    hs = [_stabilise(h) for h in plugin.constraints(modules, np.array(zfull, dtype=object), p, model, settings, 1)]
    lb, ub = plugin.constraint_bounds(modules)
    if not len(hs) == len(lb) == len(ub):
        raise UnsupportedStack(f"{len(hs)} constraint rows but {len(lb)} lower / {len(ub)} upper bounds")

    # ---- cost: value, gradient, packed Hessian ------------------------------------------------------------------
    if slack_model:
        for v in z:
            if sp.simplify(sp.diff(cost, v, slack)) != 0:
                raise UnsupportedStack("cost couples the slack with another variable: not supported (DESIGN.md U9)")
    if method == "jets":
        em = JetEmitter(z, _c, "c")
        j = em.jet(cost)
        cost_full = em.lines + [f"    *val = {_lit(j.v)};"] + [f"    g[{i}] = {_lit(j.g.get(i, 0.0))};" for i in range(7)] + \
                    [f"    H[{i * (i + 1) // 2 + k}] = {_lit(j.h.get((i, k), 0.0))};" for i in range(7) for k in range(i + 1)]
    else:
        g = [sp.diff(cost, v) for v in z]
        H = [[sp.diff(g[i], z[j]) for j in range(i + 1)] for i in range(7)]
        outs = [("*val", cost)] + [(f"g[{i}]", g[i]) for i in range(7)] + \
               [(f"H[{i * (i + 1) // 2 + j}]", H[i][j]) for i in range(7) for j in range(i + 1)]
        cost_full = _cse_block(outs, "c")
    cost_value = _cse_block([("*val", cost)], "v")

    # ---- rows, normalised to g(z) <= 0 ----------------------------------------------------------------------------
    rows = []
    for r, h in enumerate(hs):
        has_lo, has_up = np.isfinite(lb[r]), np.isfinite(ub[r])
        if has_up:
            rows.append((r, "upper", h - ub[r]))
        if has_lo:
            rows.append((r, "lower", lb[r] - h))
        if not (has_lo or has_up):
            raise UnsupportedStack(f"row {r} is unbounded on both sides")
    row_lines = []
    block_open = (lambda k: f"    if ({k} % step == first) {{") if row_shares else (lambda k: "    {")
    for k, (r, kind, gexpr) in enumerate(rows):
        for i, v in enumerate(z):
            if i not in ROW_VARS:
                if sp.diff(gexpr, v) != 0:
                    raise UnsupportedStack(f"constraint row {r} depends on `{CORE[i]}`: only x, y, psi (and slack) are supported")
        if method == "jets":
            em = JetEmitter([z[i] for i in ROW_VARS], _c, "r")
            j = em.jet(gexpr)
            G = lambda a: _lit(j.g.get(a, 0.0))
            Hh = lambda a, b: _lit(j.h.get((a, b), 0.0))
            row_lines += [block_open(k)] + ["    " + l for l in em.lines] + \
                         [f"        sink({k}, {_lit(j.v)}, {G(0)}, {G(1)}, {G(2)}, {Hh(0, 0)}, {Hh(1, 0)}, {Hh(1, 1)}, {Hh(2, 0)}, {Hh(2, 1)}, {Hh(2, 2)});", "    }"]
            continue
        gx, gy, gp = (sp.diff(gexpr, z[i]) for i in ROW_VARS)
        outs_k = [("const double h_", gexpr), ("const double gx_", gx), ("const double gy_", gy), ("const double gp_", gp),
                  ("const double hxx_", sp.diff(gx, z[2])), ("const double hxy_", sp.diff(gx, z[3])),
                  ("const double hyy_", sp.diff(gy, z[3])), ("const double hxp_", sp.diff(gx, z[4])),
                  ("const double hyp_", sp.diff(gy, z[4])), ("const double hpp_", sp.diff(gp, z[4]))]
        # one block per row (own common subexpressions, values dead after the sink call): keeps the register footprint of
        # the kernel independent of the number of rows; the compiler still shares sin/cos(psi) across blocks
        row_lines += [block_open(k)] + ["    " + l for l in _cse_block(outs_k, "r")] + \
                     [f"        sink({k}, h_, gx_, gy_, gp_, hxx_, hxy_, hyy_, hxp_, hyp_, hpp_);", "    }"]
    nh = len(rows)
    src_rows = ", ".join(str(r) for r, _, _ in rows)
    sgn = ", ".join("1" if kind == "upper" else "-1" for _, kind, _ in rows)
    off = ", ".join(repr(float(ub[r])) if kind == "upper" else repr(float(lb[r])) for r, kind, _ in rows)
    tick_macro = tick_const = ""
    rows_head = """// sink(k, g_k, dg/dx, dg/dy, dg/dpsi, d2g/dxdx, dxdy, dydy, dxdpsi, dydpsi, dpsidpsi) for k = 0..NH-1
template <class Sink>
TMPC_GEN_FN void rows(const double *z, const double *p, int ps, double slack, Sink &&sink)
{
    (void)z; (void)p; (void)ps; (void)slack; (void)sink;"""
    if row_shares:
        tick_macro = ("// horizon ranges whose control-tick kernels (latency mode 3) a library around this header instantiates: bit 0 = N <= 20, "
                      f"bit 1 = 21 <= N <= 31\n#define GENERATED_STAGE_TICK_KERNELS {int(tick_kernels)}\n")
        tick_const = (f"constexpr int TICK_SPLIT = {int(tick_split)};   // control-tick kernels (four waves per trajectory): 1 = the stage "
                      "linearisation is split over the waves\n")
        rows_head = """// sink(k, g_k, dg/dx, dg/dy, dg/dpsi, d2g/dxdx, dxdy, dydy, dxdpsi, dydpsi, dpsidpsi) for k = 0..NH-1.
// (first, step): this call's share -- the row blocks with k % step == first, each exactly as the unshared call evaluates it
// (the four-wave tick kernels give the shares to different waves); the default (0, 1) is every row.
template <class Sink>
TMPC_GEN_FN void rows(const double *z, const double *p, int ps, double slack, Sink &&sink, int first = 0, int step = 1)
{
    (void)z; (void)p; (void)ps; (void)slack; (void)sink; (void)first; (void)step;"""
    header = f"""// Generated by mpc_planner_amd.codegen.emit for solver "{name}" -- do not edit.
// Stage cost and inequality rows of the configured module stack with exact first and second derivatives.
// z = [a, w, x, y, psi, v, spline]; p = one stage's parameter row, element i at p[i * ps]; slack = the trajectory's
// constant slack value (0 without the slack model).  Rows are normalised to g(z) <= 0:
//   g_k = SIGN[k] * (h_SRC[k](z) - BOUND[k]),  SIGN = +1 for an upper bound, -1 for a lower bound of module row SRC[k].
#pragma once
#include <math.h>
#include <stddef.h>
#if defined(__HIPCC__)
#define TMPC_GEN_FN __host__ __device__ inline
#else
#define TMPC_GEN_FN inline
#endif

// 1 / (1 + exp(-x)), evaluated without overflow for either sign of x
TMPC_GEN_FN double tmpc_gen_logistic(double x) {{ const double e = exp(-fabs(x)); return (x >= 0.0 ? 1.0 : e) / (1.0 + e); }}
{tick_macro}namespace tmpc_gen {{
constexpr int NPAR = {npar};
constexpr int NH = {nh};
constexpr int SLACK = {1 if slack_model else 0};
{tick_const}constexpr int MODEL = {1 if second_order_unicycle else 0};   // 0: contouring unicycle (spline' = v); 1: SecondOrderUnicycleModel (z[6] is an inert padding slot)
constexpr double LB[7] = {{{", ".join(repr(float(v)) for v in lb7)}}};   // the model's bounds, order [a, w, x, y, psi, v, spline / padding]
constexpr double UB[7] = {{{", ".join(repr(float(v)) for v in ub7)}}};
constexpr int ROW_SRC[{max(nh, 1)}] = {{{src_rows or "0"}}};
constexpr int ROW_SIGN[{max(nh, 1)}] = {{{sgn or "0"}}};
constexpr double ROW_BOUND[{max(nh, 1)}] = {{{off or "0.0"}}};

TMPC_GEN_FN void cost_value(const double *z, const double *p, int ps, double slack, double *val)
{{
    (void)slack;
{chr(10).join(cost_value)}
}}

// g[7]; H[28] = packed lower triangle, H[i (i + 1) / 2 + j] = d2 cost / dz_i dz_j  (i >= j)
TMPC_GEN_FN void cost_full(const double *z, const double *p, int ps, double slack, double *val, double *g, double *H)
{{
    (void)slack;
{chr(10).join(cost_full)}
}}

{rows_head}
{chr(10).join(row_lines)}
}}
}}  // namespace tmpc_gen
"""
    return dict(header=header, params=params, npar=npar, nh=nh, slack=int(slack_model), model=int(second_order_unicycle),
                rows=[(r, kind) for r, kind, _ in rows], name=name)
