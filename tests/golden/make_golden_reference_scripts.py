#!/usr/bin/env python3
"""Writes tests/golden/reference_scripts.json: what the reference's OWN, unmodified module scripts (solver_generator,
mpc_planner_modules/scripts) generate when they are imported with mpc_planner_amd.codegen.symbolic registered as `casadi`,
assembled exactly like generate_jackalsimulator_solver.py:92-101 does and handed to emit.generate -- recorded as data only: the
parameter maps, the row count and sha256 digests of the emitted stage-function header and of the C++ wiring files (modules.h /
definitions.h / modules.cmake).  tests/test_codegen_reference_scripts.py checks this repository's own library stacks against them.
A subprocess with bytecode writing disabled keeps the reference checkout untouched.
Run from the repository root:  python tests/golden/make_golden_reference_scripts.py <path of a checkout of the reference project>"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SCRIPT = r'''
import sys, json
sys.dont_write_bytecode = True
sys.path.insert(0, %(root)r)
from mpc_planner_amd.codegen import symbolic, emit, cpp_glue
symbolic.install_as_casadi()
sys.path.insert(0, %(ref)r + "/solver_generator"); sys.path.insert(0, %(ref)r + "/mpc_planner_modules/scripts")
from control_modules import ModuleManager
from solver_model import ContouringSecondOrderUnicycleModel
from mpc_base import MPCBaseModule
from contouring import ContouringModule
from ellipsoid_constraints import EllipsoidConstraintModule
from guidance_constraints import GuidanceConstraintModule
settings = {"N": 20, "integrator_step": 0.2, "n_discs": 1, "max_obstacles": 8, "linearized_constraints": {"add_halfspaces": 0},
            "contouring": {"num_segments": 5, "dynamic_velocity_reference": False}}
modules = ModuleManager(); model = ContouringSecondOrderUnicycleModel()
base = modules.add_module(MPCBaseModule(settings))
base.weigh_variable(var_name="a", weight_names="acceleration"); base.weigh_variable(var_name="w", weight_names="angular_velocity")
base.weigh_variable(var_name="v", weight_names=["velocity", "reference_velocity"], cost_function=lambda x, w: w[0] * (x - w[1]) ** 2)
modules.add_module(ContouringModule(settings))
modules.add_module(GuidanceConstraintModule(settings, constraint_submodule=EllipsoidConstraintModule))
gen = emit.generate(modules, model, settings, "reference_scripts_tmpc", method="jets")
# second configuration: the reference's own generation test stack (solver_generator/test/test_acados.py:30-46)
from path_reference_velocity import PathReferenceVelocityModule
from solver_definition import define_parameters
from util.parameters import Parameters
st2 = {"N": 20, "integrator_step": 0.2, "n_discs": 1, "max_obstacles": 12, "contouring": {"num_segments": 8, "dynamic_velocity_reference": False}}
m2 = ModuleManager()
b2 = m2.add_module(MPCBaseModule(st2))
b2.weigh_variable(var_name="a", weight_names="acceleration"); b2.weigh_variable(var_name="w", weight_names="angular_velocity")
m2.add_module(ContouringModule(st2)); m2.add_module(PathReferenceVelocityModule(st2)); m2.add_module(EllipsoidConstraintModule(st2))
p2 = define_parameters(m2, Parameters(), st2)
json.dump(dict(header=gen["header"], pmap=dict(gen["params"]._params), nh=gen["nh"], modules_h=cpp_glue.modules_header(modules),
               pmap2=dict(p2._params), modules_h2=cpp_glue.modules_header(m2), definitions_h2=cpp_glue.definitions_header(m2),
               definitions_h=cpp_glue.definitions_header(modules), modules_cmake=cpp_glue.modules_cmake(modules)), open(sys.argv[1], "w"))
'''


def sha256(text):
    return hashlib.sha256(text.encode()).hexdigest()


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "gen.json")
        subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, ref=os.path.abspath(ref)), out], check=True, timeout=600, cwd=tmp,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), stdout=subprocess.DEVNULL)
        gen = json.load(open(out))
    rec = {"what": "outputs of the reference's unmodified module scripts through mpc_planner_amd.codegen (made by make_golden_reference_scripts.py)",
           "tmpc": {"settings": "N = 20, 1 disc, 8 obstacles, 5 spline segments: MPCBase (a, w, v weights) + Contouring + GuidanceConstraints(EllipsoidConstraints)",
                    "parameter_map": gen["pmap"], "nh": gen["nh"], "header_sha256": sha256(gen["header"]),
                    "modules_h_sha256": sha256(gen["modules_h"]), "definitions_h_sha256": sha256(gen["definitions_h"]),
                    "modules_cmake_sha256": sha256(gen["modules_cmake"])},
           "acados_test_stack": {"settings": "N = 20, 1 disc, 12 obstacles, 8 spline segments: MPCBase (a, w) + Contouring + PathReferenceVelocity + "
                                             "EllipsoidConstraints (the reference's solver_generator/test/test_acados.py:30-46)",
                                 "parameter_map": gen["pmap2"], "modules_h_sha256": sha256(gen["modules_h2"]),
                                 "definitions_h_sha256": sha256(gen["definitions_h2"])}}
    with open(os.path.join(HERE, "reference_scripts.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
