"""The fifth C header, include/tmpc_hip_episode.h (the plant step, obstacle motion and episode log of a closed loop), without a GPU: it names
exactly one function and one struct; every library build exports the function, the generated libraries among them;
mpc_planner_amd/episode.py's signature table and struct agree with the header; the four older headers and their tables know nothing of it."""
import ctypes as C
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_binding_signatures import header_prototypes, header_structs, header_text, layout, prototype_mismatches  # noqa: E402
from test_stack_scenario_header import GENERATED  # noqa: E402

NAME = "tmpc_episode_step"


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    text = _header("tmpc_hip_episode.h")
    protos = header_prototypes(text)
    assert list(protos) == [NAME]
    assert [NAME] == sorted(set(re.findall(r"\b(tmpc_[a-z0-9_]+)\s*\(", text)))                        # the expression misses no function the header names
    generated = sorted(glob.glob(os.path.join(ROOT, "build", "generated", "libtmpc_hip_*.so")))
    assert {f"libtmpc_hip_{n}.so" for n in GENERATED} <= {os.path.basename(p) for p in generated}
    for path in [solver.LIB_PATH, solver.LAB_LIB_PATH] + generated:
        assert hasattr(C.CDLL(path), NAME), f"{os.path.basename(path)} does not export {NAME}"


def test_signature_table_and_struct_match_the_header():
    from mpc_planner_amd import episode
    text = _header("tmpc_hip_episode.h")
    assert prototype_mismatches(text, episode._SIGNATURES) == []
    assert episode.EXPORTS == list(episode._SIGNATURES) == [NAME]
    assert len(episode.ARRAYS) == 21 and set(episode.OPTIONAL) <= set(episode.ARRAYS)
    proto = re.search(r"int tmpc_episode_step\(([^()]*)\)", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")][5:] == list(episode.ARRAYS)           # the pointer arguments, in the header's order
    structs = header_structs(text)
    assert list(structs) == ["tmpc_episode_options"]
    assert layout(structs["tmpc_episode_options"]) == layout(episode.TmpcEpisodeOptions) and C.sizeof(episode.TmpcEpisodeOptions) == 56
    opt = episode.episode_options(substeps=4, timeout_ticks=7, max_episodes=3, control_dt=0.04, max_acceleration=2.5, max_angular_velocity=1.5,
                                  robot_radius=0.3, goal_x=9.0)
    assert [getattr(opt, n) for n, _ in opt._fields_] == [56, 4, 7, 3, 0.04, 2.5, 1.5, 0.3, 9.0]
    # and the check sees a wrong row
    ret, args = episode._SIGNATURES[NAME]
    assert prototype_mismatches(text, {NAME: (ret, args[:-1])}) == [f"{NAME}: 26 arguments in the header, 25 in the table"]


def test_the_older_headers_and_their_tables_are_unchanged():
    from mpc_planner_amd import solver, stack_env, stack_scenario, stack_writers
    older = [header_text(), _header("tmpc_hip_stack.h"), _header("tmpc_hip_stack_env.h"), _header("tmpc_hip_stack_scenario.h")]
    assert not any(NAME in text or "tmpc_episode_options" in text for text in older)
    for module in (solver, stack_writers, stack_env, stack_scenario):
        assert NAME not in module.EXPORTS and NAME not in module._SIGNATURES
    with open(os.path.join(HERE, "golden", "binding_calls.json")) as fh:
        assert sorted(solver.EXPORTS) == sorted(json.load(fh)["bound"])
    assert len(stack_writers.EXPORTS) == 3 and len(stack_env.EXPORTS) == 4 and len(stack_scenario.EXPORTS) == 2
    assert '#include "tmpc_hip.h"' in open(os.path.join(ROOT, "include", "tmpc_hip_episode.h")).read()
