"""The wave and workgroup reductions of the solve kernels (csrc/tmpc_kernels.hpp: wave_max, wave_min, wave_sum, blk_max / blk_min / blk_sum,
blk_residuals) and the stage pre-reductions of the row passes (stage_sum3, stage_sum_quad), run on chosen lane values through the lab library's
tmpc_lab_reductions (csrc/tmpc_capi.hip, -DTMPC_LAB_SWITCHES only) at 64, 128 and 256 threads and compared BIT FOR BIT with a numpy
restatement of the same pairing order:

    row_shr:1, 2, 4, 8 inside every 16-lane row, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3, lane 63 is the wave's result;
    workgroups combine the waves' results in the order wave 0, 1, ...

The reductions move no identity value into the lanes a row shift vacates (those read 0) and leave the rows a row broadcast does not write undefined:
lane 63's result never contains such a lane.  They take v_max_f64 / v_min_f64 on the operands as they are, without fmax's canonicalising move.
The kernel also returns maximum, minimum and sum in the form the reductions had before -- identity (-Inf, +Inf, 0.0) moved into the vacated
lanes, fmax / fmin -- and the two forms must agree on every input below.

Special values, recorded from the identity-filled form and asserted for both (test_documented_special_values): fmax / fmin drop a quiet NaN
operand, so wave_max / wave_min of a wave with one NaN lane are the maximum / minimum of the other 63 lanes; a sum with a NaN lane is that NaN
(0x7ff8000000000000 stays 0x7ff8000000000000).  All lanes -0.0: wave_max, wave_min AND wave_sum return -0.0 (lane 63 adds no vacated lane's +0.0)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALARS = 32
LANES = np.arange(64)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def net(x, op, ident):
    """Lane 63 of the DPP network on one wave (64 values)."""
    x = np.array(x, dtype=np.float64)
    for n in (1, 2, 4, 8):
        src = np.where(LANES % 16 >= n, x[np.maximum(LANES - n, 0)], ident)
        x = op(x, src)
    y = x.copy()
    for row in (1, 3):
        y[16 * row:16 * row + 16] = op(x[16 * row:16 * row + 16], x[16 * row - 1])
    x = y.copy()
    x[32:] = op(y[32:], y[31])
    return x[63]


ADD = lambda a, b: a + b            # noqa: E731
MAX = np.fmax                       # drops a NaN operand, like fmax
MIN = np.fmin


def combine(per_wave, op):
    r = per_wave[0]
    for v in per_wave[1:]:
        r = op(r, v)
    return r


def shl1(x):                        # wave_shl:1, the last lane reads 0
    return np.concatenate([x[1:], [0.0]])


def sum3(x):
    return x + shl1(x + shl1(x))


def quad(x, fold8):
    x = x + x[LANES ^ 1]
    x = x + x[LANES ^ 2]
    if fold8:                       # row_shl:4, lanes 12 .. 15 of a row read 0
        x = x + np.where(LANES % 16 < 12, x[np.minimum(LANES + 4, 63)], 0.0)
    return x


def cases(threads, rng):
    """[(name, array[5][threads], nonneg)]: arrays 0 .. 3 feed blk_residuals' maxima (and array 0 everything else), array 4 its sum."""
    out = []

    def add(name, a, nonneg):
        a = np.asarray(a, dtype=np.float64)
        five = np.stack([a, np.roll(a, 7) * 0.5, np.roll(a, 19) * 0.25, np.roll(a, 40) * 2.0, np.roll(a, 3)])
        out.append((name, five, nonneg))

    add("zeros", np.zeros(threads), True)
    for lane in (0, 15, 16, 31, 32, 63):
        for w in range(threads // 64):
            a = np.zeros(threads); a[64 * w + lane] = 3.5 + lane
            add(f"single lane {lane} wave {w}", a, True)
            add(f"single negative lane {lane} wave {w}", -a, False)
    a = np.abs(rng.standard_normal(threads)); a[threads // 3] = np.inf
    add("+Inf in one lane", a, True)
    a = rng.standard_normal(threads); a[threads - 5] = np.nan
    add("NaN in one lane", a, False)
    a = rng.standard_normal(threads); a[0] = np.nan
    add("NaN in lane 0", a, False)
    add("-0.0 everywhere", np.full(threads, -0.0), False)
    a = np.abs(rng.standard_normal(threads)) * 1e-310; a[::5] = 5e-324
    add("denormals", a, True)
    add("signed denormals", a * np.where(rng.random(threads) < 0.5, -1.0, 1.0), False)
    a = np.ones(threads) * 1e-16; a[::9] = 1.0; a[4::13] = 1e16; a[5::13] = -1e16
    add("sum depends on association", a, False)
    add("sum depends on association, non-negative", np.abs(a), True)
    add("random", rng.standard_normal(threads) * 10.0 ** rng.integers(-8, 8, threads), False)
    add("random non-negative", np.abs(rng.standard_normal(threads)) * 10.0 ** rng.integers(-8, 8, threads), True)
    return out


@pytest.fixture(scope="module")
def lab():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    lib = C.CDLL(solver.LAB_LIB_PATH)
    assert lib.tmpc_has_lab_switches() == 1
    lib.tmpc_lab_reductions.restype = C.c_int
    lib.tmpc_lab_reductions.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("threads", [64, 128, 256])
def test_reductions_bitwise(lab, threads):
    rng = np.random.default_rng(1234 + threads)
    cs = cases(threads, rng)
    nw = threads // 64
    inp = np.ascontiguousarray(np.stack([c[1] for c in cs]))
    out = np.full((len(cs), SCALARS + 3 * threads), -777.0)
    assert lab.tmpc_lab_reductions(threads, len(cs), inp.ctypes.data, out.ctypes.data) == 0
    with np.errstate(all="ignore"):
        for (name, five, nonneg), o in zip(cs, out):
            a = five[0]
            waves = [a[64 * w:64 * w + 64] for w in range(nw)]
            wmax = [net(x, MAX, -np.inf) for x in waves]
            wmin = [net(x, MIN, np.inf) for x in waves]
            wsum = [net(x, ADD, 0.0) for x in waves]
            exp = {"wave_max": (o[0:nw], wmax), "wave_min": (o[8:8 + nw], wmin), "wave_sum": (o[12:12 + nw], wsum),
                   "wave_max, identity-filled": (o[4:4 + nw], wmax), "wave_min, identity-filled": (o[28:28 + nw], wmin),
                   "wave_sum, identity-filled": (o[24:24 + nw], wsum),
                   "blk_max": (o[16:17], [combine(wmax, MAX)]), "blk_min": (o[18:19], [combine(wmin, MIN)]), "blk_sum": (o[19:20], [combine(wsum, ADD)]),
                   "stage_sum3": (o[SCALARS:SCALARS + threads], np.concatenate([sum3(x) for x in waves])),
                   "stage_sum_quad": (o[SCALARS + threads:SCALARS + 2 * threads], np.concatenate([quad(x, False) for x in waves])),
                   "stage_sum_quad, fold 8": (o[SCALARS + 2 * threads:SCALARS + 3 * threads], np.concatenate([quad(x, True) for x in waves]))}
            for ident in (0.0, np.nan):                                                 # (the restatement itself: the fill never reaches lane 63)
                assert np.array_equal(bits([net(x, MAX, ident) for x in waves]), bits(wmax)), name
                assert np.array_equal(bits([net(x, ADD, ident) for x in waves]), bits(wsum)), name
            g, b, dd, m = five[:4]                                                       # (no case mixes +0.0 with -0.0, the one pair fmax leaves open)
            lane_max = MAX(MAX(g, b), MAX(dd, m))
            worst = combine([net(lane_max[64 * w:64 * w + 64], MAX, -np.inf) for w in range(nw)], MAX)
            exp["blk_residuals worst"] = (o[20:21], [worst])
            exp["blk_residuals mu"] = (o[21:22], [combine([net(five[4][64 * w:64 * w + 64], ADD, 0.0) for w in range(nw)], ADD)])
            for what, (got, want) in exp.items():
                assert np.array_equal(bits(got), bits(want)), (threads, name, what, got, want)
            assert np.all(o[nw:4] == -777.0) and np.all(o[12 + nw:16] == -777.0) and o[17] == -777.0      # waves the block does not have: untouched


def test_documented_special_values(lab):
    """The behaviours the module docstring states, on the device."""
    a = np.arange(64.0) - 20.0
    nan = a.copy(); nan[40] = np.nan
    neg0 = np.full(64, -0.0)
    inp = np.ascontiguousarray(np.stack([np.stack([x] * 5) for x in (nan, neg0)]))
    out = np.zeros((2, SCALARS + 3 * 64))
    assert lab.tmpc_lab_reductions(64, 2, inp.ctypes.data, out.ctypes.data) == 0
    b = bits(out)
    assert out[0, 0] == 43.0 == out[0, 4] and out[0, 8] == -20.0 == out[0, 28]            # the NaN lane is dropped
    assert b[0, 12] == 0x7ff8000000000000 == b[0, 24]
    neg0 = 0x8000000000000000
    assert b[1, 0] == neg0 == b[1, 4] and b[1, 8] == neg0 == b[1, 28] and b[1, 12] == neg0 == b[1, 24]
