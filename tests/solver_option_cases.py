"""Model bounds that bind and solver options off their defaults (helper, no tests): the option cases, the kernel families that run them, the bound
values and scenes per shape, and the oracle runs both sides share.  tests/test_solver_option_cases.py (no GPU) holds every (shape, option case) named
here to its preconditions on the oracle alone; tests/test_gpu_solver_options.py runs the matrix on the device; tests/test_gpu_carried_state.py,
tests/test_gpu_generated_tick.py and tests/test_lanes_twin.py take single cases from here.

Variable order of lb / ub (tmpc_dims, the oracle's orc_problem): a, w, x, y, psi, v, s.  Stage 0 boxes the controls only (x_0 is fixed), the terminal
node is not boxed (oracle/sqp_rti.c), so a side counts as active when a control of stages 0 .. N-1 or a state of stages 1 .. N-1 is within ACTIVE
of it."""
import functools
import math

import numpy as np

VARS = ("a", "w", "x", "y", "psi", "v", "s")
DEFAULT_LB = (-2.0, -0.8, -2000.0, -2000.0, -4.0 * math.pi, -0.01, -1.0)      # tmpc_default_dims*, orc_problem_init* (checked by the CPU module)
DEFAULT_UB = (2.0, 0.8, 2000.0, 2000.0, 4.0 * math.pi, 3.0, 10000.0)
ACTIVE, INACTIVE, VIOLATED = 1e-4, 1e-2, 1e-6
THRESHOLD_GUARD = 2e-7          # no entry's distance to a bound it is asked about may be this close to ACTIVE: the 1e-8 line times the largest stage scale (< 20)
MATTERS = 1e-7                  # 100 x the 1.3e-9 worst device-oracle distance the README records
B_PER_SCENE = 16
DRAWS = 4                       # ulp-moved copies of the inputs per (shape, option case)
THREADS = 16
VERDICT = ("exit_code", "qp_status", "sqp_iter", "qp_iter_total")

# bounds asymmetric inactive: all 14 changed, no two of one magnitude, none active.  Far bounds are not free: their barrier terms move the interior-point count
# of some entries by one, so which set (and scene) leaves the oracle's integers at those of its default-bounds run is derived per shape like the other values
ASYM_SETS = {
    "near": (dict(a=-1.7, w=-0.7, x=-30.0, y=-40.0, psi=-3.0, v=-0.02, s=-0.5), dict(a=1.3, w=0.9, x=50.0, y=20.0, psi=2.0, v=2.6, s=45.0)),
    "mid": (dict(a=-1.8, w=-0.75, x=-300.0, y=-400.0, psi=-6.0, v=-0.03, s=-0.6), dict(a=1.9, w=0.65, x=500.0, y=200.0, psi=5.0, v=2.8, s=450.0)),
    "far": (dict(a=-2.3, w=-0.9, x=-1900.0, y=-2200.0, psi=-12.0, v=-0.05, s=-1.5), dict(a=2.1, w=0.85, x=2100.0, y=1800.0, psi=13.0, v=3.2, s=9000.0)),
}
ALL_OFF = dict(erk_steps=2, dt=0.25, reg_eps=1e-3, ipm_mu0=0.1, ipm_thr0=0.05, n_sqp=7)


def option(oid, opts=None, baseline=None, bounds=None, active=(), inactive=False):
    """opts: tmpc_dims / orc_problem fields off their defaults; baseline: the fields of the run the option is told apart from (default: none -- every
    default); bounds: the option case whose per-shape lb / ub values (VALUES) this case takes, or "asym"; active: the (side, variable) pairs the values
    must make active."""
    return dict(id=oid, opts=opts or {}, baseline=baseline or {}, bounds=bounds, active=tuple(active), inactive=inactive)


OPTION_CASES = [
    option("bounds upper", bounds="bounds upper", active=(("ub", "a"), ("ub", "v"), ("ub", "s"))),
    option("bounds x", bounds="bounds x", active=(("ub", "x"),)),
    option("bounds psi lower", bounds="bounds psi lower", active=(("lb", "psi"),)),
    option("bounds w lower", bounds="bounds w lower", active=(("lb", "w"),)),
    option("bounds w upper", bounds="bounds w upper", active=(("ub", "w"),)),
    option("bounds a lower", bounds="bounds a lower", active=(("lb", "a"),)),
    option("bounds asymmetric inactive", bounds="asym", inactive=True),
    option("dt 0.25", dict(dt=0.25)),
    option("erk 1 at dt 0.4", dict(dt=0.4, erk_steps=1), baseline=dict(dt=0.4)),
    option("reg 1e-6", dict(reg_eps=1e-6)),
    option("reg 1e-2", dict(reg_eps=1e-2)),
    option("mu0 only 0.1", dict(ipm_mu0=0.1)),
    option("thr0 only 0.1", dict(ipm_thr0=0.1)),
    option("mu0 thr0 (1, 1)", dict(ipm_mu0=1.0, ipm_thr0=1.0)),
    option("n_sqp 3", dict(n_sqp=3)),
    option("n_sqp 25", dict(n_sqp=25)),
    # (its own values: at dt 0.25 the horizon is a second longer, and the bounds that bind at dt 0.2 need not)
    option("all off + bounds upper", dict(ALL_OFF), bounds="all off + bounds upper", active=(("ub", "a"), ("ub", "v"), ("ub", "s"))),
]
OPTION = {o["id"]: o for o in OPTION_CASES}
LOWER_CASES = ("bounds w lower", "bounds psi lower", "bounds a lower")       # every family runs the first of these its shape has values for
EVERY_FAMILY = ("bounds upper", "lower", "bounds asymmetric inactive", "all off + bounds upper")

# ids of test_gpu_dispatch_matrix.DISPATCH_CASES: the closed-loop list of test_gpu_carried_state plus the generic kernel at both ends of its regime
EXTRA_FAMILIES = ["m0 N=21 nr=40 generic", "generic N=33 (8,8)"]
# one per code copy and team: these run every option case
REDUCED = ["m0 (8,8) N=20", "m0 (8,8) N=20 compact", "m0 (20,8) N=30", "m2 (8,8) N=20", "m3 (8,8) N=21", "sqrt <-1,13,3> N=20", "generic N=33 (8,8)"]


def families():
    import test_gpu_carried_state as CS
    return list(CS.LOOP_CASES) + EXTRA_FAMILIES


def dispatch_case(fid):
    """The row of DISPATCH_CASES, without its doomed entries and at this matrix's launch size."""
    import test_gpu_dispatch_matrix as T
    (c,) = [c for c in T.DISPATCH_CASES if c["id"] == fid]
    assert isinstance(c["B"], int) and not c["refused"] and not c["disc_offset"], fid
    return dict(c, doomed=())


def shape_of(fid):
    """The oracle problem of a family, the Riccati form aside: families of one shape share bound values, scenes and oracle runs."""
    c = dispatch_case(fid)
    rows = f"({c['n_lin']},{c['M']})" + (f"+{c['n_slk']}" if c["n_slk"] else "")
    return f"N={c['N']} {rows} S={c['S']}" + (" ca" if c["cm"] else "") + (" g" if c["gauss"] else "")


def shapes():
    """{shape: the first family of that shape}."""
    out = {}
    for fid in families():
        out.setdefault(shape_of(fid), fid)
    return out


# ---- values per shape ------------------------------------------------------------------------------------------------------------------------------
# VALUES[shape][bound case] = (scenes, {variable: bound}): derived on the CPU from the oracle's default solution of the shape's batches (a bound inside
# the range the default solution spans, loosened until the preconditions of tests/test_solver_option_cases.py hold).  SCENES[shape]: the scenes of the
# cases without bound values.
VALUES = {
    'N=20 (8,8) S=5': {
        'bounds upper': ((1, 2), {'v': 1.94, 's': 6.65, 'a': 0.46}),
        'all off + bounds upper': ((1, 2), {'v': 1.81, 's': 7.76, 'a': 0.21}),
        'bounds w lower': ((1, 2), {'w': -0.38}),
        'bounds psi lower': ((1, 2), {'psi': -0.43}),
        'bounds a lower': ((8,), {'a': -0.06}),
        'bounds x': ((1, 2), {'x': 6.56}),
        'bounds w upper': ((1, 2), {'w': 0.32}),
        'asym': ((21,), 'mid'),
    },
    'N=30 (8,8) S=5': {
        'bounds upper': ((1, 2), {'v': 1.95, 's': 10.59, 'a': 0.5}),
        'all off + bounds upper': ((1, 2), {'v': 1.89, 's': 12.05, 'a': 0.34}),
        'bounds w lower': ((1, 2), {'w': -0.27}),
        'asym': ((7,), 'far'),
    },
    'N=32 (8,8) S=5': {
        'bounds upper': ((1, 2), {'v': 1.96, 's': 11.38, 'a': 0.5}),
        'all off + bounds upper': ((1, 2), {'v': 1.97, 's': 13.29, 'a': 0.32}),
        'bounds w lower': ((1, 2), {'w': -0.27}),
        'asym': ((5,), 'near'),
    },
    'N=20 (12,12) S=5': {
        'bounds upper': ((1, 2), {'v': 1.95, 's': 6.82, 'a': 0.71}),
        'all off + bounds upper': ((1, 2), {'v': 1.86, 's': 7.33, 'a': 0.29}),
        'bounds w lower': ((1, 2), {'w': -0.31}),
        'asym': ((25,), 'near'),
    },
    'N=30 (8,8)+12 S=5': {
        'bounds upper': ((1, 2), {'v': 1.93, 's': 10.58, 'a': 0.46}),
        'all off + bounds upper': ((1, 2), {'v': 1.87, 's': 12.03, 'a': 0.36}),
        'bounds w lower': ((1, 2), {'w': -0.24}),
        'bounds psi lower': ((1, 2), {'psi': -0.25}),
        'bounds a lower': ((2, 3), {'a': -0.16}),
        'bounds x': ((1, 2), {'x': 10.41}),
        'bounds w upper': ((1, 2), {'w': 0.27}),
        'asym': ((0,), 'near'),
    },
    'N=20 (12,13) S=5': {
        'bounds upper': ((1, 2), {'v': 1.69, 's': 6.21, 'a': 0.39}),
        'all off + bounds upper': ((1, 2), {'v': 1.64, 's': 6.89, 'a': 0.25}),
        'bounds w lower': ((1, 2), {'w': -0.33}),
        'asym': ((7,), 'mid'),
    },
    'N=20 (7,9) S=5': {
        'bounds upper': ((1, 2), {'v': 1.91, 's': 6.44, 'a': 0.29}),
        'all off + bounds upper': ((1, 2), {'v': 1.82, 's': 7.23, 'a': 0.24}),
        'bounds w lower': ((1, 2), {'w': -0.43}),
        'asym': ((26,), 'near'),
    },
    'N=20 (14,14)+12 S=5': {
        'bounds upper': ((1, 2), {'v': 1.76, 's': 6.25, 'a': 0.36}),
        'all off + bounds upper': ((1, 2), {'v': 1.64, 's': 7.24, 'a': 0.23}),
        'bounds w lower': ((1, 2), {'w': -0.23}),
        'asym': ((3,), 'near'),
    },
    'N=31 (11,11)+12 S=5': {
        'bounds upper': ((1, 2), {'v': 1.93, 's': 10.5, 'a': 0.48}),
        'all off + bounds upper': ((1, 2), {'v': 1.46, 's': 8.68, 'a': 0.23}),
        'bounds w lower': ((1, 2), {'w': -0.29}),
        'asym': ((5,), 'near'),
    },
    'N=30 (5,5) S=3': {
        'bounds upper': ((1, 2), {'v': 1.98, 's': 10.49, 'a': 0.49}),
        'all off + bounds upper': ((1, 2), {'v': 1.9, 's': 12.11, 'a': 0.3}),
        'bounds w lower': ((1, 2), {'w': -0.33}),
        'asym': ((3,), 'near'),
    },
    'N=31 (8,8) S=5': {
        'bounds upper': ((1, 2), {'v': 1.94, 's': 10.98, 'a': 0.5}),
        'all off + bounds upper': ((1, 2), {'v': 1.96, 's': 12.82, 'a': 0.32}),
        'bounds w lower': ((1, 2), {'w': -0.27}),
        'asym': ((0,), 'near'),
    },
    'N=21 (8,8) S=5': {
        'bounds upper': ((1, 2), {'v': 1.94, 's': 7.03, 'a': 0.46}),
        'all off + bounds upper': ((1, 2), {'v': 1.83, 's': 8.09, 'a': 0.2}),
        'bounds w lower': ((1, 2), {'w': -0.41}),
        'bounds psi lower': ((1, 2), {'psi': -0.41}),
        'bounds a lower': ((8,), {'a': -0.1}),
        'bounds x': ((1, 2), {'x': 6.95}),
        'bounds w upper': ((1, 2), {'w': 0.32}),
        'asym': ((8,), 'near'),
    },
    'N=30 (8,8)+12 S=5 ca': {
        'bounds upper': ((1, 2), {'v': 1.97, 's': 10.72, 'a': 0.61}),
        'all off + bounds upper': ((1, 2), {'v': 1.95, 's': 12.82, 'a': 0.43}),
        'bounds w lower': ((1, 2), {'w': -0.26}),
        'asym': ((2,), 'near'),
    },
    'N=30 (5,5) S=3 g': {
        'bounds upper': ((1, 2), {'v': 1.62, 's': 8.32, 'a': 0.41}),
        'all off + bounds upper': ((1, 2), {'v': 1.52, 's': 9.24, 'a': 0.35}),
        'bounds w lower': ((1, 2), {'w': -0.45}),
        'asym': ((2,), 'near'),
    },
    'N=30 (5,5) S=3 ca g': {
        'bounds upper': ((1, 2), {'v': 1.81, 's': 9.09, 'a': 0.53}),
        'all off + bounds upper': ((1, 2), {'v': 1.79, 's': 10.69, 'a': 0.46}),
        'bounds w lower': ((1, 2), {'w': -0.56}),
        'asym': ((10,), 'near'),
    },
    'N=2 (8,8) S=5': {
        'bounds upper': ((26, 27), {'v': 0.55, 's': 0.13, 'a': 0.04}),
        'all off + bounds upper': ((26, 27), {'v': 0.53, 's': 0.16, 'a': -0.03}),
    },
    'N=21 (13,13) S=5': {
        'bounds upper': ((1, 2), {'v': 1.72, 's': 6.61, 'a': 0.4}),
        'all off + bounds upper': ((1, 2), {'v': 1.88, 's': 7.73, 'a': 0.28}),
        'bounds w lower': ((1, 2), {'w': -0.44}),
        'asym': ((16,), 'mid'),
    },
    'N=33 (8,8) S=5': {
        'bounds upper': ((1, 2), {'v': 1.99, 's': 11.77, 'a': 0.5}),
        'all off + bounds upper': ((1, 2), {'v': 1.95, 's': 13.78, 'a': 0.32}),
        'bounds w lower': ((1, 2), {'w': -0.27}),
        'bounds psi lower': ((2, 3), {'psi': -0.43}),
        'bounds a lower': ((1, 2), {'a': -0.05}),
        'bounds x': ((1, 2), {'x': 11.59}),
        'bounds w upper': ((1, 2), {'w': 0.29}),
        'asym': ((5,), 'near'),
    },
}
# scenes of the cases without bound values, where (1, 2) does not meet the preconditions
SCENES = {
    'N=21 (8,8) S=5': {'reg 1e-6': (5, 7)},
}
# (shape, option case) pairs without a value and scene in 0 .. 31 that meet the preconditions, and why
_N2_LOWER = "at N = 2 no lower bound on w, psi or a that every entry of a scene in 0 .. 31 survives pulls two entries within 1e-4 of it: the default solution spans 1e-4 in these variables, the bound's multiplier stays small and the interior point stays further than that from the bound"
EXCLUDED = {
    ("N=2 (8,8) S=5", "bounds w lower"): _N2_LOWER,
    ("N=2 (8,8) S=5", "bounds psi lower"): _N2_LOWER,
    ("N=2 (8,8) S=5", "bounds a lower"): _N2_LOWER,
    ("N=2 (8,8) S=5", "bounds asymmetric inactive"): "at N = 2 bounds that stay inactive move no entry of the oracle's result by 1e-7 (0 of 16 in each of the 69 scene and "
                                                     "set pairs tried): the discrimination rule would have nothing to tell apart",
}
# (kind, lanes per stage, threads, team) tuples of the pick functions without a family here: those of test_gpu_carried_state.EXCLUDED
FAMILY_EXCLUDED = {}


def lower_case_of(shape):
    for oid in LOWER_CASES:
        if oid in VALUES.get(shape, {}):
            return oid
    return None


def options_of(fid):
    """The option cases a family runs."""
    shape = shape_of(fid)
    ids = [lower_case_of(shape) if oid == "lower" else oid for oid in EVERY_FAMILY]
    if fid in REDUCED:
        ids = [o["id"] for o in OPTION_CASES]
    return [oid for oid in ids if oid is not None and (shape, oid) not in EXCLUDED and (OPTION[oid]["bounds"] is None or OPTION[oid]["bounds"] in VALUES.get(shape, {}))]


def matrix():
    return [(fid, oid) for fid in families() for oid in options_of(fid)]


def shape_matrix():
    """(shape, option case) pairs of the matrix, each once."""
    seen = {}
    for fid, oid in matrix():
        seen.setdefault((shape_of(fid), oid), fid)
    return [(s, o, f) for (s, o), f in seen.items()]


def _box(lb, ub):
    l, u = list(DEFAULT_LB), list(DEFAULT_UB)
    for k, v in lb.items():
        l[VARS.index(k)] = v
    for k, v in ub.items():
        u[VARS.index(k)] = v
    return dict(lb=tuple(l), ub=tuple(u))


def resolve(shape, oid):
    """(scenes, overrides of the option run, overrides of its baseline run)."""
    o = OPTION[oid]
    opts, base = dict(o["opts"]), dict(o["baseline"])
    ids = SCENES.get(shape, {}).get(oid, (1, 2))
    if o["bounds"] == "asym":
        ids, name = VALUES[shape]["asym"]
        opts.update(_box(*ASYM_SETS[name]))
    elif o["bounds"] is not None:
        ids, vals = VALUES[shape][o["bounds"]]
        side = {s for s, _ in o["active"]}
        assert len(side) == 1
        opts.update(_box(vals, {}) if side == {"lb"} else _box({}, vals))
    return tuple(ids), opts, base


def scene_batch(fid, ids):
    import test_gpu_dispatch_matrix as T
    return T._scenes(dict(dispatch_case(fid), ids=tuple(ids)), B_PER_SCENE * len(ids))


def oracle_solve(fid, sc, opts, rf=None, moved=None):
    """The oracle on the family's problem under `opts`; rf: another Riccati form; moved: a seed -- every input times 1 + 2^-50 N(0,1)."""
    import oracle_lib as O
    import test_gpu_dispatch_matrix as T
    c = dispatch_case(fid)
    pb = T._problem(c if rf is None else dict(c, rf=rf))
    for k, v in opts.items():
        setattr(pb, k, v)
    xinit, x0, params = sc["xinit"], sc["x0"], sc["params"]
    if moved is not None:
        rng = np.random.default_rng(moved)
        xinit, x0, params = (a * (1.0 + 2.0 ** -50 * rng.standard_normal(a.shape)) for a in (xinit, x0, params))
    n = xinit.shape[0]
    assert params.shape[2] == pb.npar
    xt, ut, info = O.solve_batch(pb, xinit, x0.reshape(n, -1), params.reshape(n, -1), num_threads=THREADS)
    return xt, ut, info


def distance(xa, ua, xb, ub):
    """Per entry: the worst relative difference per stage of two results (the scale of _compare: the stage's largest entry of the second, at least 1)."""
    sx = np.maximum(np.abs(xb).max(axis=2, keepdims=True), 1.0); su = np.maximum(np.abs(ub).max(axis=2, keepdims=True), 1.0)
    return np.maximum((np.abs(xa - xb) / sx).max(axis=(1, 2)), (np.abs(ua - ub) / su).max(axis=(1, 2)))


def gaps(xt, ut, lb, ub):
    """Per entry and variable: (distance to the lower bound, to the upper bound), the smallest over the boxed stages; negative: violated."""
    N = ut.shape[1]
    z = [ut[:, :N, 0], ut[:, :N, 1]] + [xt[:, 1:N, j] for j in range(5)]
    lo = np.stack([(zj - lb[j]).min(axis=1) for j, zj in enumerate(z)], axis=1)
    hi = np.stack([(ub[j] - zj).min(axis=1) for j, zj in enumerate(z)], axis=1)
    return lo, hi


def active_entries(xt, ut, opts, side, var):
    """Mask of the entries with that side active at some stage."""
    lo, hi = gaps(xt, ut, opts.get("lb", DEFAULT_LB), opts.get("ub", DEFAULT_UB))
    return np.abs((lo if side == "lb" else hi)[:, VARS.index(var)]) < ACTIVE


@functools.lru_cache(maxsize=None)
def oracle_runs(shape, oid, rf=0):
    """What both sides share, computed once and never written to: the batch, the oracle under the option and under its baseline (in Riccati form rf), and the
    mask of the entries on which the option matters -- they differ by MATTERS or more, or in an integer."""
    fid = shapes()[shape]
    ids, opts, base = resolve(shape, oid)
    sc = scene_batch(fid, ids)
    xt, ut, info = oracle_solve(fid, sc, opts, rf=rf)
    xb, ub, ib = oracle_solve(fid, sc, base, rf=rf)
    moved = distance(xb, ub, xt, ut)
    ints = np.zeros(len(moved), bool)
    for k in VERDICT:
        ints |= info[k] != ib[k]
    out = dict(ids=ids, opts=opts, base=base, sc=sc, xt=xt, ut=ut, info=info, xb=xb, ub=ub, ib=ib, moved=moved, ints_differ=ints, mask=(moved >= MATTERS) | ints)
    for v in (xt, ut, xb, ub, moved, ints, out["mask"], *info.values(), *ib.values(), sc["xinit"], sc["x0"], sc["params"]):
        v.setflags(write=False)
    return out
