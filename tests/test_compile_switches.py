"""Compile-time switches without a GPU: the kernel sources test no TMPC_* macro outside ALLOWED (the build structure and the four measurement
instruments), and no build script or tool passes a -D for a TMPC_* name outside it.  A -D for a name that no source reads compiles the product
form without a word, and an A/B run of it measures two identical builds; here it fails instead.  A new compile-time experiment is added to
ALLOWED on purpose (an instrument also to INTEGRATION.md section 7)."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

BUILD_STRUCTURE = {
    "TMPC_TU_FAST", "TMPC_TU_COMPACT", "TMPC_TU_PROF", "TMPC_TU_CP2", "TMPC_TU_SQRT", "TMPC_TU_QUAD", "TMPC_TU_QUADW",
    "TMPC_SINGLE_KERNEL", "TMPC_SINGLE_COMPACT", "TMPC_SINGLE_TU",
    "TMPC_GENERATED_STAGE", "TMPC_GEN_FAST", "TMPC_GEN_FAST2",
    "TMPC_WITH_LANES", "TMPC_LAB_SWITCHES",
}
INSTRUMENTS = {"TMPC_SWEEP_PROFILE", "TMPC_SCAN_PROFILE", "TMPC_POLY_PROFILE", "TMPC_LANES_PROF"}
ALLOWED = BUILD_STRUCTURE | INSTRUMENTS

SOURCE_SUFFIXES = (".hip", ".hpp", ".h", ".cpp", ".cc", ".c")
_DIRECTIVE = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")
_DEFINED = re.compile(r"\bdefined\s*\(?\s*(TMPC_\w+)")
# -DTMPC_NAME, -D TMPC_NAME, -D${VAR:-TMPC_NAME}; a following $ or { (shell / f-string substitution) makes the name a prefix
_DASH_D = re.compile(r"-D\s*(?:\$\{\w+:-)?(TMPC_\w*)([${]?)")


def _sources():
    files = glob.glob(os.path.join(ROOT, "mpc_planner_amd", "csrc", "*")) + glob.glob(os.path.join(HERE, "cpu_twin", "*"))
    return sorted(f for f in files if f.endswith(SOURCE_SUFFIXES))


def switches_tested():
    """{name: [file:line, ...]} of every TMPC_* macro that a preprocessor condition of the kernel sources tests."""
    out = {}
    for path in _sources():
        for i, line in enumerate(open(path, errors="replace"), 1):
            m = _DIRECTIVE.match(line)
            names = set()
            if m:
                names |= set(re.findall(r"\bTMPC_\w+", m.group(1).split("//")[0]))
            names |= set(_DEFINED.findall(line.split("//")[0]))
            for n in names:
                out.setdefault(n, []).append(f"{os.path.relpath(path, ROOT)}:{i}")
    return out


def switches_passed():
    """{(name, is_prefix): [file:line, ...]} of every -DTMPC_* that the build, the code generator and tools/ pass."""
    files = [os.path.join(ROOT, "__graft_entry__.py")] + glob.glob(os.path.join(ROOT, "mpc_planner_amd", "codegen", "*.py"))
    files += [f for f in glob.glob(os.path.join(ROOT, "tools", "*")) if os.path.isfile(f)]
    out = {}
    for path in sorted(files):
        for i, line in enumerate(open(path, errors="replace"), 1):
            for name, subst in _DASH_D.findall(line):
                out.setdefault((name, bool(subst)), []).append(f"{os.path.relpath(path, ROOT)}:{i}")
    return out


def test_sources_test_only_allowed_switches():
    tested = switches_tested()
    bad = {n: where for n, where in tested.items() if n not in ALLOWED}
    assert not bad, f"compile-time switches outside the allowed list: {bad}"
    # the list holds nothing the sources no longer read
    stale = sorted(ALLOWED - set(tested))
    assert not stale, f"allowed switches that no source tests: {stale}"


def test_scripts_pass_only_allowed_switches():
    passed = switches_passed()
    assert ("TMPC_TU_FAST", False) in passed and ("TMPC_GENERATED_STAGE", False) in passed, "the -D scan found none of the build's own flags"
    bad = {}
    for (name, prefix), where in passed.items():
        ok = any(a.startswith(name) for a in ALLOWED) if prefix else name in ALLOWED
        if not ok:
            bad[name + ("*" if prefix else "")] = where
    assert not bad, f"-D flags for names the sources do not read: {bad}"


def test_instruments_documented():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 7\..*?(?=^## |\Z)", text, re.S | re.M)
    assert m, "INTEGRATION.md has no section 7"
    missing = sorted(n for n in INSTRUMENTS if n not in m.group(0))
    assert not missing, f"instruments not named in INTEGRATION.md section 7: {missing}"
