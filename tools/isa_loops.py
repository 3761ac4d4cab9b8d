"""Static view of a kernel's ISA (hipcc -S): innermost loops (backward branches) with their instruction mix.
A loop's SIDE BLOCKS -- code placed outside the loop's line range that the loop branches out to and that branches (or falls) back into it, as the
compiler lays out divergent regions (s_cbranch_exec* to a block behind the loop, s_branch back) -- are found and added: every loop is printed with the
mix of its line range and -- innermost loops only --, where it has side blocks, with the mix including them (every side block counted once: an upper bound of one trip).
Two fields follow the address arithmetic of the sequential stage loops: `int` counts the VALU integer and move instructions (everything on the vector
side that is neither floating point nor a cross-lane move: the index / address arithmetic, selects and register copies) and `quarter` the quarter-rate
integer forms among them (the 32-bit multiplies v_mul_lo / v_mul_hi and the 64-bit multiply-adds v_mad_u64_u32 / v_mad_i64_i32: 16 issue cycles where
v_mul_u32_u24 / v_mad_u32_u24 take 4; csrc/tmpc_kernels.hpp, mul24).
Two more follow the row broadcasts: `dpp` counts every DPP instruction, `fused` those among them that compute (v_fmac_f64_dpp: the broadcast folded into
the multiply-add, fmac_bcast16 of csrc/tmpc_kernels.hpp; dpp - fused = the plain v_mov_b64_dpp), and `nop` / `nop_states` the s_nop instructions and the
wait states they stand for (s_nop n = n + 1 states), the price of the fused form's hazard pad.
Usage: python tools/isa_loops.py file.s kernel-name-prefix"""
import re
import sys

lines = open(sys.argv[1]).read().split("\n")
st = [i for i, l in enumerate(lines) if l.startswith(sys.argv[2])][0]
body = []
for l in lines[st:]:
    body.append(l)
    if "s_endpgm" in l:
        break
label_at = {}
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        label_at[m.group(1)] = i
loops = []
for i, l in enumerate(body):
    m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", l)
    if m:
        tgt = m.group(1) or m.group(2)
        if tgt in label_at and label_at[tgt] < i:
            loops.append((label_at[tgt], i))
def is_instr(l):
    s = l.strip()
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":")
FLOAT = re.compile(r"_(f|bf)(16|32|64)|_pk_f")
QUARTER = ("v_mul_lo_u32", "v_mul_lo_i32", "v_mul_hi_u32", "v_mul_hi_i32", "v_mad_u64_u32", "v_mad_i64_i32")
def mix(a, b):
    c = dict(valu=0, f64=0, salu=0, lds=0, vmem=0, readlane=0, dpp=0, fused=0, nop=0, nop_states=0, wait=0, trans=0, int=0, quarter=0, total=0)
    for l in body[a:b + 1]:
        if not is_instr(l):
            continue
        op = l.strip().split()[0]
        c["total"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
            if "_f64" in op: c["f64"] += 1
            if "readlane" in op or "readfirstlane" in op: c["readlane"] += 1
            if "dpp" in l: c["dpp"] += 1
            if "dpp" in l and not op.startswith("v_mov"): c["fused"] += 1
            if op.startswith(("v_rsq", "v_rcp", "v_sqrt", "v_sin", "v_cos", "v_exp", "v_log")): c["trans"] += 1
            if not FLOAT.search(op) and "lane" not in op and "dpp" not in l: c["int"] += 1
            if op.startswith(QUARTER): c["quarter"] += 1
        elif op.startswith("s_nop"):
            c["nop"] += 1
            c["nop_states"] += int(l.split()[1], 0) + 1
        elif op.startswith("s_waitcnt"): c["wait"] += 1
        elif op.startswith("s_"): c["salu"] += 1
        elif op.startswith("ds_"): c["lds"] += 1
        elif op.startswith(("global_", "scratch_", "buffer_", "flat_")): c["vmem"] += 1
    return c
BRANCH = re.compile(r"^\s*(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")
def side_blocks(a, b, limit=400):
    """[(first, last)] line ranges outside [a, b] that the loop a..b branches to and that return into it."""
    inside = lambda i: a <= i <= b
    todo = [label_at[m.group(2)] for l in body[a:b + 1] for m in [BRANCH.match(l)] if m and m.group(2) in label_at and not inside(label_at[m.group(2)])]
    seen, blocks = set(), []
    while todo:
        t = todo.pop()
        if t in seen or any(x <= t <= y for x, y in blocks):
            continue
        seen.add(t)
        pending, end = [], None
        for j in range(t, min(t + limit, len(body))):
            l = body[j]
            if "s_endpgm" in l:
                break
            if j > t and j == a:                      # fell through into the loop's header
                end = j - 1
                break
            m = BRANCH.match(l)
            if not m or m.group(2) not in label_at:
                continue
            tgt = label_at[m.group(2)]
            if m.group(1) == "s_branch":
                if inside(tgt) or any(x <= tgt <= y for x, y in blocks) or tgt in seen:
                    end = j
                break
            if inside(tgt):
                end = j                                 # a conditional return; the block may go on
            else:
                pending.append(tgt)
        if end is not None:
            blocks.append((t, end))
            todo += pending
    merged = []                                        # (a block reached twice at different entry points is counted once)
    for x, y in sorted(blocks):
        if merged and x <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(merged[-1][1], y))
        else:
            merged.append((x, y))
    return merged
def add(c, d):
    return {k: c[k] + d[k] for k in c}
# innermost: loops that contain no other loop
inner = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
print(f"kernel lines {len(body)}, total {mix(0, len(body) - 1)}")
for a, b in sorted(set(loops)):
    tag = "inner" if (a, b) in inner else "outer"
    print(f"{tag} loop lines {a}-{b} ({b - a}): {mix(a, b)}")
    sb = side_blocks(a, b) if (a, b) in inner else []   # (an outer loop's "blocks" would be the enclosing loop's fall-through code, not divergent regions)
    if sb:
        tot = mix(a, b)
        for x, y in sb:
            tot = add(tot, mix(x, y))
        print(f"    with side blocks {', '.join(f'{x}-{y}' for x, y in sb)}: {tot}")
