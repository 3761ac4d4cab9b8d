"""Drop-in check of the generator's plugin surface against the reference's OWN, unmodified module scripts: what those scripts
generate through mpc_planner_amd.codegen (symbolic registered as `casadi`, assembled exactly like generate_jackalsimulator_solver.py:92-101,
handed to emit.generate) is recorded in tests/golden/reference_scripts.json -- parameter maps, row count, sha256 of the emitted stage-function
header and of the C++ wiring files (made by tests/golden/make_golden_reference_scripts.py) -- and this repository's library stacks of the
same configurations must reproduce it byte for byte."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _sha256(text):
    return hashlib.sha256(text.encode()).hexdigest()


def test_unmodified_reference_module_scripts_generate_the_same_stage_functions():
    with open(os.path.join(HERE, "golden", "reference_scripts.json")) as fh:
        rec = json.load(fh)
    from mpc_planner_amd.codegen import cpp_glue, emit, stacks
    from mpc_planner_amd.codegen.hostlib import HostStageFunctions
    st = stacks.settings()                                  # N = 20, 8 obstacles, 5 segments: the configuration the reference's scripts were assembled in
    model, mm = stacks.tmpc(st)
    gen = emit.generate(mm, model, st, "reference_scripts_tmpc", method="jets")
    ref = rec["tmpc"]
    # the emitted header is the one the reference's own scripts produce, byte for byte
    assert _sha256(gen["header"]) == ref["header_sha256"]
    with open(os.path.join(HERE, "golden", "stage_functions.json")) as fh:
        cases = [c for c in json.load(fh)["cases"] if c["config"] == "cfg2_tmpc_M8"]
    assert ref["parameter_map"] == cases[0]["parameter_map"] and ref["nh"] == 16
    assert dict(gen["params"]._params) == ref["parameter_map"] and gen["nh"] == ref["nh"]
    hs = HostStageFunctions(gen["header"])
    for c in cases:
        v, g, H = hs.cost(c["z"], c["p"])
        np.testing.assert_allclose(v, c["cost"], rtol=1e-12)
        np.testing.assert_allclose(g, c["cost_grad"], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(H, c["cost_hess"], rtol=1e-9, atol=1e-10)
        h, D, Hr = hs.rows(c["z"], c["p"])
        hh, J = np.array(c["h"]), np.array(c["h_jac"])
        for k in range(hs.nh):
            r, s = hs.row_src[k], hs.row_sign[k]
            np.testing.assert_allclose(h[k], s * (hh[r] - hs.row_bound[k]), rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(D[k], s * J[r][[2, 3, 4]], rtol=1e-10, atol=1e-11)
    # the C++ wiring files (modules.h / definitions.h / modules.cmake) written for the reference's own module objects are
    # identical to those written for this repo's library stack of the same configuration
    assert _sha256(cpp_glue.modules_header(mm)) == ref["modules_h_sha256"]
    assert _sha256(cpp_glue.definitions_header(mm)) == ref["definitions_h_sha256"]
    assert _sha256(cpp_glue.modules_cmake(mm)) == ref["modules_cmake_sha256"]
    # the stack of the reference's generation test (test_acados.py:30-46): same parameter map and wiring files from the
    # reference's own Parameters / module objects and from this repo's library
    from mpc_planner_amd.codegen import plugin as P
    ref2 = rec["acados_test_stack"]
    st2 = stacks.settings(N=20, max_obstacles=12, num_segments=8)
    _, mm2 = stacks.contouring_path_velocity_ellipsoids(st2)
    assert dict(P.define_parameters(mm2, P.Parameters(), st2)._params) == ref2["parameter_map"]
    assert _sha256(cpp_glue.modules_header(mm2)) == ref2["modules_h_sha256"] and _sha256(cpp_glue.definitions_header(mm2)) == ref2["definitions_h_sha256"]
