"""The stores of the sequential Riccati stage loops (csrc/tmpc_riccati.hpp) at the smallest shapes at which a re-ordered or re-addressed store can go wrong.

What the loops do:
  factorisation    the P row of lanes 2..6 (and the extra row's p of lane 7) is stored without a select for the entries above the diagonal: every lane stores
                   five entries in DESCENDING order of the entry index, and the junk a lane puts above its diagonal lands on an entry of a later row, whose
                   owner overwrites it in a later instruction of the same wave; the three store groups (P row, Lxu / y pair, lane 1's pivots) are stores of
                   every lane through per-lane (offset, stride) pairs, one straight-line region per stage, and the lanes outside a group write to a dummy
                   slot of L.scr
  backward sweep   q rides in lanes 8..12 of the gh load (a per-lane pointer and stride) and one row shift hands it to lanes 2..6
A store that lands on the wrong stage or slot, junk that survives, or a q from the wrong stage shows as a wrong iterate, so every shape below is solved by
the fast kernel and by its compact twin (another LDS layout -- another stride per lane, L.pr aliases L.dpi --, the same arithmetic), which must agree bit
for bit, and both are compared with the CPU oracle as tests/test_gpu_parity._compare does: no mismatch in exit codes, SQP counts, QP status and
interior-point counts, iterates and objectives within 1e-8 relative.  B = 16 per case.  The shapes are those of tests/test_gpu_sweep_operands.py (its
helpers run them) and two more short horizons:
  (8,8) N = 2, 3, 4, 5   the first and the last stage of these paths and the by-two loops' remainder: N = 2 is one pass of the by-two loops and no
                         remainder, 3 adds the odd remainder, 4 and 5 are the same with a second pass; the per-lane strides are multiplied by every stage
                         index from the terminal node's P row down to stage 0
  (8,8) N = 20           the benchmark's shape
  (12,12) N = 20         compact layout 3: y lives inside the stage's 30-double block (the extra row's pair store has another base and stride)
  (0,4) N = 20           no packed topology rows
  <-1,7,3> N = 20        a runtime-shape instantiation
  <-1,6,4> N = 22        two waves per trajectory (NTH = 128): the sweeping wave alternates
  (8,8) N = 20, riccati_form = 1    the square-root form stores Lxx through the same P-row store (fast kernels only: no compact twin to compare with)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_dispatch_matrix import CP0, FIELDS, case
from test_gpu_sweep_operands import B, SHAPES as OPERAND_SHAPES, _oracle, _run

# (case of the fast kernel, instantiation of the compact twin or None, lab switches that make the twin run at B = 16)
SHAPES = OPERAND_SHAPES[:2] + [
    (case("(8,8) N=4", "fast<8,8,3,64,Solo,0>", 4, 8, 8, B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=5", "fast<8,8,3,64,Solo,0>", 5, 8, 8, B=B), "compact<8,8,3,64,0>", CP0),
] + OPERAND_SHAPES[2:]


@pytest.mark.parametrize("c,twin,lab", SHAPES, ids=[s[0]["id"] for s in SHAPES])
def test_riccati_stage_stores(c, twin, lab, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, xt, ut, info = _oracle(c)
    ok = info["exit_code"] == 1
    assert ok.sum() >= B / 2, (int(ok.sum()), B)                   # the comparison is not made on failures alone
    fast = _run(c, sc, c["expect"])
    worst = max(_compare(fast, xt, ut, info))
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        compact = _run(c, sc, twin)
        for f in FIELDS:
            assert np.array_equal(fast[f], compact[f], equal_nan=True), f
        worst = max(worst, *_compare(compact, xt, ut, info))
    print(f"[stage stores] {c['id']}: successes {int(ok.sum())}/{B}, worst rel diff {worst:.2e}, twin {twin}")
