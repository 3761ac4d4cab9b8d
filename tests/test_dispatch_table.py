"""The solve-kernel dispatch table without a GPU: every instantiation the pick_*_kernel functions of csrc/tmpc_capi.hip can return has a
case in tests/test_gpu_dispatch_matrix.py (or a reason in its EXCLUDED), so that a new instantiation without a parity case fails here; and the
C-ABI unit compiles in every optional configuration (lane family, lab switches), which no default build exercises."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CAPI = os.path.join(os.path.dirname(HERE), "mpc_planner_amd", "csrc", "tmpc_capi.hip")

# the naming macros of tmpc_capi.hip and the name each writes (the C side builds the same text by stringizing the arguments)
_MACROS = {
    "TMPC_FAST": lambda a: "fast<%s,%s,%s,%s,Solo,0>" % tuple(a),
    "TMPC_FASTP": lambda a: "fast<%s,%s,%s,%s,%s,0>" % tuple(a),
    "TMPC_FASTX": lambda a: "fast<%s,%s,%s,%s,%s,%s>" % tuple(a),
    "TMPC_CP": lambda a: "compact<%s,%s,%s,64,%s>" % tuple(a),
    "TMPC_CP2": lambda a: "compact<%s,%s,%s,128,%s>" % tuple(a),
}
_ARITY = {"TMPC_FAST": 4, "TMPC_FASTP": 5, "TMPC_FASTX": 6, "TMPC_CP": 4, "TMPC_CP2": 4}


def _pick_bodies(src):
    """{function name: body text} of every pick_*_kernel function."""
    out = {}
    for m in re.finditer(r"static SolveKernel (pick_\w+_kernel)\([^)]*\)\s*\{", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        out[m.group(1)] = src[m.end():i - 1]
    return out


def pick_instantiations(path=CAPI):
    """{name: (macro, pick function)} of every instantiation expression in the pick_*_kernel functions.  TMPC_FAST / TMPC_FASTP name a shape with a
    profiled twin (tmpc_debug_profile runs it), the others production instantiations only."""
    src = open(path).read()
    found = {}
    for fn, body in _pick_bodies(src).items():
        raw = re.findall(r"tmpc_solve_(?:fast_|compact_)?kernel\s*<[^;]*", body)
        assert not raw, f"{fn}: instantiation written without a naming macro (tmpc_kernel_info could not report it): {raw}"
        for m in re.finditer(r"\b(TMPC_FASTP|TMPC_FASTX|TMPC_FAST|TMPC_CP2|TMPC_CP)\(([^()]*)\)", body):
            args = [a.strip() for a in m.group(2).split(",")]
            assert len(args) == _ARITY[m.group(1)], m.group(0)
            found.setdefault(_MACROS[m.group(1)](args), (m.group(1), fn))
    return found


def test_pick_functions_are_found():
    found = pick_instantiations()
    fns = {fn for _, fn in found.values()}
    assert fns == {"pick_fast_kernel", "pick_sqrt_kernel", "pick_compact_kernel", "pick_compact2_kernel", "pick_latency_kernel",
                   "pick_scan_kernel", "pick_quad_kernel"}, fns
    assert len(found) >= 55, len(found)


def test_every_instantiation_has_a_dispatch_case():
    """Coverage ratchet: an instantiation named in pick_*_kernel must be the expected name of a case of DISPATCH_CASES or be listed in EXCLUDED."""
    import test_gpu_dispatch_matrix as T
    found = pick_instantiations()
    covered = T.expected_names()
    orphans = sorted(set(found) - covered - set(T.EXCLUDED))
    assert not orphans, "instantiations without a case in tests/test_gpu_dispatch_matrix.py DISPATCH_CASES (or EXCLUDED): " + ", ".join(orphans)
    stale = sorted((covered | set(T.EXCLUDED)) - set(found) - {n for n in covered if n.startswith("generic<")})
    assert not stale, "names in DISPATCH_CASES / EXCLUDED that no pick_*_kernel function returns: " + ", ".join(stale)
    assert all(reason.strip() for reason in T.EXCLUDED.values())
    assert {f"generic<{cm}>" for cm in range(4)} <= covered                       # the generic kernel of every stage model


def _hipcc():
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.exists(h) else shutil.which("hipcc")


@pytest.mark.parametrize("flags", [[], ["-DTMPC_LAB_SWITCHES"], ["-DTMPC_WITH_LANES"], ["-DTMPC_WITH_LANES", "-DTMPC_LAB_SWITCHES"]],
                         ids=["product", "lab", "lanes", "lanes_lab"])
def test_capi_unit_compiles_in_every_configuration(flags):
    """build(with_lanes=True) and the lab library compile the C-ABI unit with these switches; a host-side syntax check catches what breaks one of them
    (e.g. a helper defined in only one branch of #ifdef TMPC_WITH_LANES)."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not available")
    inc = os.path.join(os.path.dirname(HERE), "include")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "--cuda-host-only", *flags, "-I", inc, CAPI],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
