"""The sixth C header, include/tmpc_hip_guidance_search.h (the guidance search on device), without a GPU: it names exactly one function and
one struct; every library build exports the function, the generated libraries among them; mpc_planner_amd/guidance_search.py's signature
table and struct agree with the header; the five older headers and their tables know nothing of it."""
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

NAME, STRUCT, HEADER = "tmpc_guidance_search", "tmpc_guidance_search_options", "tmpc_hip_guidance_search.h"


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    text = _header(HEADER)
    protos = header_prototypes(text)
    assert list(protos) == [NAME]
    assert [NAME, STRUCT] == sorted(set(re.findall(r"\b(tmpc_guidance_[a-z0-9_]+)\b", text)))           # the expression misses no name the header declares
    generated = sorted(glob.glob(os.path.join(ROOT, "build", "generated", "libtmpc_hip_*.so")))
    assert {f"libtmpc_hip_{n}.so" for n in GENERATED} <= {os.path.basename(p) for p in generated}
    for path in [solver.LIB_PATH, solver.LAB_LIB_PATH] + generated:
        assert hasattr(C.CDLL(path), NAME), f"{os.path.basename(path)} does not export {NAME}"


def test_signature_table_and_struct_match_the_header():
    from mpc_planner_amd import guidance_search as gs
    text = _header(HEADER)
    assert prototype_mismatches(text, gs._SIGNATURES) == []
    assert gs.EXPORTS == list(gs._SIGNATURES) == [NAME]
    assert len(gs.ARRAYS) == 15 and set(gs.OPTIONAL) <= set(gs.ARRAYS)
    proto = re.search(r"int tmpc_guidance_search\(([^()]*)\)", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")][5:] == list(gs.ARRAYS)                  # the pointer arguments, in the header's order
    structs = header_structs(text)
    assert list(structs) == [STRUCT]
    assert layout(structs[STRUCT]) == layout(gs.TmpcGuidanceSearchOptions) and C.sizeof(gs.TmpcGuidanceSearchOptions) == 64
    opt = gs.guidance_search_options(n_paths=3, n_samples=17, seed=2 ** 63 + 5, n_nodes_max=9, max_expansions=11, robot_radius=0.3,
                                     max_velocity=2.5, margin=0.75, weight_length=1.5)
    assert [getattr(opt, n) for n, _ in opt._fields_] == [64, 3, 17, 0, 2 ** 63 + 5, 9, 11, 0.3, 2.5, 0.75, 1.5]
    # and the check sees a wrong row
    ret, args = gs._SIGNATURES[NAME]
    assert prototype_mismatches(text, {NAME: (ret, args[:-1])}) == [f"{NAME}: 20 arguments in the header, 19 in the table"]


def test_the_older_headers_and_their_tables_are_unchanged():
    from mpc_planner_amd import episode, solver, stack_env, stack_scenario, stack_writers
    older = [header_text(), _header("tmpc_hip_stack.h"), _header("tmpc_hip_stack_env.h"), _header("tmpc_hip_stack_scenario.h"),
             _header("tmpc_hip_episode.h")]
    assert not any(re.search(r"\b%s\b" % NAME, text) or STRUCT in text for text in older)
    for module in (solver, stack_writers, stack_env, stack_scenario, episode):
        assert NAME not in module.EXPORTS and NAME not in module._SIGNATURES
    with open(os.path.join(HERE, "golden", "binding_calls.json")) as fh:
        assert sorted(solver.EXPORTS) == sorted(json.load(fh)["bound"])
    assert len(stack_writers.EXPORTS) == 3 and len(stack_env.EXPORTS) == 4 and len(stack_scenario.EXPORTS) == 2 and len(episode.EXPORTS) == 1
    assert '#include "tmpc_hip.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
