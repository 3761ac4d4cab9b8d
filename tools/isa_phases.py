"""Static view of the interior-point loop of a solve kernel's ISA (hipcc -S), split into its phases.

The Riccati calls of an interior-point iteration raise the wave's issue priority (s_setprio 3 ... s_setprio 2, csrc/tmpc_riccati.hpp TMPC_PRIO_*), so
the s_setprio pairs are landmarks in the listing: the interior-point loop is the smallest loop (backward branch) that holds every `s_setprio 3`, and
its text falls into the stretches between the pairs -- the code OUTSIDE the stage loops, which tools/isa_loops.py does not look at -- and the
stretches inside them.  The stretches are named by their place in the TEXT (outside A, stage loops 1, outside B, ...).  The compiler rotates the loop and
orders its blocks freely, so which phase of the iteration a stretch holds is read from its contents; for compact<8,8,3,64,0> today:

    outside A   node residuals, Hh <- W, row pass R, residual reduction, exit tests          (27 ds_add_f64: the stage sums of row pass R)
    outside B   pivot verdict, affine step length, mu_aff, corrector right-hand side         (8 ds_add_f64: the right-hand side's sums)
    outside C   step length, update of t / lam / v / pi                                      (the only stretch with stores and no ds_add_f64)
    outside D   the back branch

Counts are static and follow the compiler's block layout: a divergent block the compiler placed behind another phase is counted where it stands.
Per stretch: VALU, f64, DPP, v_cndmask, v_mov (b32 / b64, DPP moves not included), v_max/v_min f64, readlane, SALU, VMEM, LDS and LDS by opcode.

Usage: python tools/isa_phases.py file.s kernel-name-prefix [--json]
One kernel per call; the listings come from tools/kernel_probe.sh, one instantiation each (EMIT=-S EXT=s):
    COMPACT=1 EMIT=-S EXT=s OUT=/tmp/c883 tools/kernel_probe.sh 8,8,3,false          compact<8,8,3,64,0>
    COMPACT=1 EMIT=-S EXT=s OUT=/tmp/c884 tools/kernel_probe.sh 8,8,4,false,128      compact<8,8,4,128,0>
    COMPACT=1 EMIT=-S EXT=s OUT=/tmp/c12 tools/kernel_probe.sh 12,12,3,false         compact<12,12,3,64,0>
    EMIT=-S EXT=s OUT=/tmp/f883 tools/kernel_probe.sh 8,8,3,64,false                 fast<8,8,3,64,Solo,0>
    python tools/isa_phases.py /tmp/c883.s _ZN4tmpc
DESIGN.md section 7 holds the tables of these four before and after the interior-point phases were slimmed."""
import collections
import json
import re
import sys


def kernel_body(path, prefix):
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if l.startswith(prefix)]              # (labels stand in column 0)
    if not starts:
        raise SystemExit(f"{path}: no kernel whose symbol starts with {prefix!r} (symbols are mangled: _ZN4tmpc25tmpc_solve_compact_kernel..., _ZN4tmpc22tmpc_solve_fast_kernel...)")
    st = starts[0]
    body = []
    for l in lines[st:]:
        body.append(l)
        if "s_endpgm" in l:
            break
    return body


def is_instr(l):
    s = l.strip()
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":")


def loops_of(body):
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
    out = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in label_at and label_at[tgt] < i:
                out.append((label_at[tgt], i))
    return out


def mix(body, a, b):
    c = collections.OrderedDict(valu=0, f64=0, dpp=0, cndmask=0, mov=0, maxmin64=0, readlane=0, salu=0, vmem=0, lds=0)
    lds = collections.Counter()
    for l in body[a:b + 1]:
        if not is_instr(l):
            continue
        op = l.strip().split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
            if "_f64" in op: c["f64"] += 1
            if "dpp" in l: c["dpp"] += 1
            if op.startswith("v_cndmask"): c["cndmask"] += 1
            if op.startswith(("v_mov_b32", "v_mov_b64")) and "dpp" not in l: c["mov"] += 1
            if op.startswith(("v_max_f64", "v_min_f64")): c["maxmin64"] += 1
            if "readlane" in op or "readfirstlane" in op: c["readlane"] += 1
        elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop")):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
            lds[op] += 1
        elif op.startswith(("global_", "scratch_", "buffer_", "flat_")):
            c["vmem"] += 1
    c["lds_by_opcode"] = dict(sorted(lds.items()))
    return c


def phases(path, prefix):
    body = kernel_body(path, prefix)
    hi = [i for i, l in enumerate(body) if re.match(r"\s*s_setprio\s+3\b", l)]
    lo = [i for i, l in enumerate(body) if re.match(r"\s*s_setprio\s+2\b", l)]
    if not hi:
        raise SystemExit("no s_setprio 3 in this kernel: no landmarks")
    holding = [lp for lp in loops_of(body) if lp[0] <= hi[0] and hi[-1] <= lp[1]]
    a, b = min(holding, key=lambda lp: lp[1] - lp[0])
    pairs = []
    for h in hi:                                           # every raise with the first lowering behind it
        l = min((x for x in lo if x > h), default=b)
        pairs.append((h, min(l, b)))
    out, at = [], a
    for n, (h, l) in enumerate(pairs):
        out.append((f"outside {chr(ord('A') + n)}", at, h - 1))
        out.append((f"stage loops {n + 1}", h, l))
        at = l + 1
    out.append((f"outside {chr(ord('A') + len(pairs))}", at, b))
    return body, (a, b), out


if __name__ == "__main__":
    body, (a, b), segs = phases(sys.argv[1], sys.argv[2])
    rows = [dict(phase=name, lines=[x, y], **mix(body, x, y)) for name, x, y in segs]
    if "--json" in sys.argv:
        print(json.dumps(dict(loop_lines=[a, b], phases=rows)))
        raise SystemExit(0)
    print(f"interior-point loop: lines {a}-{b}")
    keys = ["valu", "f64", "dpp", "cndmask", "mov", "maxmin64", "readlane", "salu", "vmem", "lds"]
    print(f"{'phase':<14}{'lines':>13}" + "".join(f"{k:>9}" for k in keys) + "  lds by opcode")
    for r in rows:
        print(f"{r['phase']:<14}{r['lines'][0]:>6}-{r['lines'][1]:<6}" + "".join(f"{r[k]:>9}" for k in keys) + "  " +
              ", ".join(f"{k} {v}" for k, v in r["lds_by_opcode"].items()))
    out = [r for r in rows if r["phase"].startswith("outside")]
    print(f"{'outside, sum':<27}" + "".join(f"{sum(r[k] for r in out):>9}" for k in keys))
