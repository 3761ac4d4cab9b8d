"""Control-tick kernels of generated solvers without a GPU: the build records the run-time-shape tick instantiations of a generated library with
their registers and scratch, and the emitted `rows` evaluates a share (first, step) of its row blocks -- what the four-wave tick kernel gives its
two row waves -- exactly as the unshared call evaluates those rows.

Latency mode 3 (four waves per trajectory) is what generated libraries carry.  The two-wave instantiations of mode 2 were built and measured
(profiles/generated_tick_kernels.json): every run was above the default kernel's (tmpc_cfg2 N = 20, 64 trajectories: 1.084 - 1.089 ms against
1.007 - 1.009 ms; jackal_tmpc N = 30, 64: 1.303 - 1.307 against 1.220 - 1.222), so by the project's rule their slot stays empty and they are not
compiled: the tests assert their absence."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TICK_NAMES = {"fast<-1,4,12,256,ScanQuad,0>", "fast<-1,6,8,256,ScanQuadT<2>,0>"}           # mode 3: N <= 20, 21 <= N <= 31


def _meta(name):
    path = os.path.join(ROOT, "build", "generated", f"{name}_meta.json")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build_generated_demo()
    with open(path) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", ["tmpc_cfg2", "jackal_tmpc"])
def test_meta_names_the_tick_kernels_without_scratch(name):
    meta = _meta(name)
    tick = meta["tick_kernels"]
    assert set(tick) == TICK_NAMES, sorted(tick)
    for k, v in tick.items():
        assert v["scratch"] == 0 and 0 < v["vgprs"] <= 512, (k, v)
    # the back end is still chosen by the production wave kernels alone: no tick kernel is counted among them
    from mpc_planner_amd.codegen import build as gb
    assert meta["wave_kernel_scratch"] == gb.wave_kernel_scratch(meta["kernel_resources"])
    assert not any(gb._is_tick_kernel(k) for k in meta["wave_kernel_scratch"])
    assert sum(gb._is_tick_kernel(k) for k in meta["kernel_resources"]) == 2
    assert not any("ScanSolo" in k for k in meta["kernel_resources"])           # mode 2's two-wave instantiations: measured slower, not compiled


def test_tick_kernels_are_outside_the_back_end_choice():
    from mpc_planner_amd.codegen import build as gb
    tick = "_ZN4tmpc22tmpc_solve_fast_kernelILin1ELi4ELi12ELi256ELb0ENS_9ScanQuadTILi3EEELi0EEEvNS_4DimsEi"
    wave = "_ZN4tmpc22tmpc_solve_fast_kernelILi16ELi0ELi3ELi64ELb0ENS_5SoloTILb0EEELi0EEEvNS_4DimsEi"
    usage = {tick: dict(vgprs=256, agprs=256, scratch=48), wave: dict(vgprs=256, agprs=0, scratch=0)}
    assert gb.wave_kernel_scratch(usage) == {}
    assert gb.tick_kernel_resources(usage) == {"fast<-1,4,12,256,ScanQuad,0>": dict(vgprs=512, scratch=48)}
    assert gb.tick_kernel_resources(usage, ranges=2) == {} and gb.tick_kernel_resources(usage, ranges=0) == {}
    usage[wave]["scratch"] = 8
    assert gb.wave_kernel_scratch(usage) == {wave: 8}


def _stack(name):
    from mpc_planner_amd.codegen import stacks
    if name == "tmpc":
        st = stacks.settings(N=20, max_obstacles=8)
        return stacks.tmpc(st) + (st,)
    st = stacks.settings(N=20, max_obstacles=4)
    return stacks.goal_gaussian(st) + (st,)


@pytest.mark.parametrize("method", ["jets", "symbolic"])
@pytest.mark.parametrize("name", ["tmpc", "goal_gaussian"])
def test_row_shares_equal_the_unshared_rows_bit_for_bit(name, method):
    """rows(first, step) evaluates the row blocks k % step == first and nothing else; the shares (0, 2) + (1, 2) and (0, 3) + (1, 3) + (2, 3)
    together are the unshared call: values, Jacobians and Hessians bit for bit, at several points."""
    from mpc_planner_amd.codegen import emit
    from mpc_planner_amd.codegen.hostlib import HostStageFunctions
    model, mm, st = _stack(name)
    gen = emit.generate(mm, model, st, name, method=method, row_shares=True)           # the header a library is compiled around
    assert "int first = 0, int step = 1" in gen["header"]
    hs = HostStageFunctions(gen["header"])
    assert hs.nh >= 4
    rng = np.random.default_rng(11)
    for _ in range(4):
        z = rng.uniform(-1.0, 1.0, 7); z[5] = rng.uniform(0.2, 2.0); z[6] = rng.uniform(0.1, 3.0)
        p = rng.uniform(0.1, 0.9, hs.npar)                                   # (a risk level among them: inside (0, 1))
        slack = 0.1 if hs.slack else 0.0
        h, D, H = hs.rows(z, p, slack)
        assert np.isfinite(h).all() and np.abs(D).sum(axis=1).all()         # every row is really evaluated (none has a zero Jacobian)
        for step in (2, 3):
            hsum, Dsum, Hsum = np.zeros_like(h), np.zeros_like(D), np.zeros_like(H)
            for first in range(step):
                hf, Df, Hf = hs.rows(z, p, slack, first, step)
                mine = np.arange(hs.nh) % step == first
                assert np.array_equal(hf[mine], h[mine]) and np.array_equal(Df[mine], D[mine]) and np.array_equal(Hf[mine], H[mine]), (first, step)
                assert not hf[~mine].any() and not Df[~mine].any() and not Hf[~mine].any(), (first, step)      # the other rows are not touched
                hsum += hf; Dsum += Df; Hsum += Hf
            assert np.array_equal(hsum, h) and np.array_equal(Dsum, D) and np.array_equal(Hsum, H)
