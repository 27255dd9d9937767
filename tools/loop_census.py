#!/usr/bin/env python3
"""Instruction census of a kernel's Newton loop, block by block, priced in issue slots.

    python3 tools/loop_census.py [--rates FILE] [--min-block N] [--ticks-per-iteration T] OBJ_OR_ASM KERNEL

OBJ_OR_ASM is an object of the library's build (flow-sim_amd/csrc/build/fs_part_nodiag.o: the gfx950 code object is taken out
of it as tools/isa_digest.py does) or the output of `hipcc -S --offload-arch=gfx950 --cuda-device-only` of one instantiation.
KERNEL is a substring of the demangled name in tools/isa_digest.py's short form, e.g. "step<double, 0, 16, 4, false, 5, false".

The flagship's fold runs at its lone-wave issue cost, so a change to it is judged by the VALU slots it
removes BEFORE it is taken to a GPU.  The census is a histogram of whatever mnemonics it meets, grouped by the classes the rates
file prices (profiles/round4/issue_rates.txt, relative to v_fma_f64): an fp64 reciprocal / reciprocal square root seed, an fp32
transcendental, everything else on the vector ALU (AGPR and DPP moves included) one slot.  Scalar, LDS and memory instructions
issue beside the vector ALU and are counted but not priced.

The Newton loop is the largest loop nested inside another one (the time loop); a kernel with a single loop is reported for
that loop.  Blocks are split at branch targets and behind branches and listed in text order with their offset in the loop.  The
totals price the loop TEXT: a block behind a branch (the flagship's level pass, once per level and not per iteration; the
boundary rows, one lane) counts as if it ran every time, so compare two builds block by block.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("FS_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
RATES = os.path.join(ROOT, "profiles", "round4", "issue_rates.txt")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def short(name):
    return (name.replace("fs::preissmann_step_kernel", "step").replace("(fs::KernelArgs<double>)", "")
            .replace("(fs::KernelArgs<float>)", "").replace("void ", ""))


def read_rates(path):
    """slot costs relative to v_fma_f64 and the ticks of one slot"""
    rel, tick = {}, 4.85
    section = False
    for line in open(path):
        m = re.match(r"v_fma_f64\s+[\d.]+ s_memtime ticks.*?: ([\d.]+) ticks", line)
        if m:
            tick = float(m.group(1))
        if line.startswith("relative to"):
            section = True
            continue
        m = re.match(r"\s+(\S.*?)\s{2,}([\d.]+)\s*$", line)
        if section and m:
            rel[m.group(1)] = float(m.group(2))
    return rel, tick


# (class, pattern on the mnemonic): the first match wins
CLASSES = [
    ("rcp/rsq f64", r"v_(rcp|rsq)_f64"),
    ("trans f32", r"v_(rcp|rsq|sqrt|log|exp|sin|cos)(_iflag|_legacy)?_f32"),
    ("agpr move", r"v_accvgpr_"),
    ("dpp move", r"v_mov_b(32|64)_dpp|v_\w+_dpp"),
    ("select", r"v_cndmask_"),
    # (v_fmac_f64 is the two-address fma the register allocator picks where the addend dies: the same arithmetic.  Until round 9 it was
    # missing here and counted as "other valu" - 244 of the flagship fold's "292 other" in the census files of rounds 5 and 6)
    ("fp64 arith", r"v_(fma|fmac|mul|add|sub|max|min|ldexp|trunc|rndne|frexp\w*|div_\w+)_f64"),
    ("fp32 arith", r"v_(fma|fmac|mul|add|sub|max|min)_f32"),
    ("lds read", r"ds_read|ds_load"),
    ("lds write", r"ds_write|ds_store"),
    ("s_nop", r"s_nop"),
]
VALU_CLASSES = ("rcp/rsq f64", "trans f32", "agpr move", "dpp move", "select", "fp64 arith", "fp32 arith", "other valu")


def classify(mn, dpp):
    if dpp and mn.startswith("v_"):
        return "dpp move"
    for name, pat in CLASSES:
        if re.match(pat, mn):
            return name
    if mn.startswith("v_"):
        return "other valu"
    if mn.startswith("s_"):
        return "scalar"
    return "memory"


def slot_cost(cls, rel):
    if cls == "rcp/rsq f64":
        return rel.get("v_rcp_f64", 3.42)
    if cls == "trans f32":
        return rel.get("v_log_f32", 1.77)
    return 1.0 if cls in VALU_CLASSES else 0.0


def metadata(text, mangled):
    """registers and spills of one kernel from the code object's metadata (the same YAML in an object's note and in a .s file)"""
    for entry in re.split(r"\n\s*- \.agpr_count:", "\n" + text)[1:]:
        if re.search(r"\.name:\s+" + re.escape(mangled) + r"\s", entry):
            entry = ".agpr_count:" + entry
            return {k: int(v) for k, v in re.findall(r"\.(agpr_count|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|"
                                                     r"private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", entry)}
    return {}


def from_object(obj):
    """{mangled: [(label or None, mnemonic, operands)]}, metadata text"""
    with tempfile.TemporaryDirectory() as tmp:
        bundle, co = os.path.join(tmp, "f.bundle"), os.path.join(tmp, "f.co")
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={bundle}", obj, os.path.join(tmp, "copy.o"))
        run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={bundle}", f"--output={co}")
        dis = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--symbolize-operands", co)
        meta = run(f"{LLVM}/llvm-readelf", "--notes", co)
    kernels, name, label = {}, None, None
    for line in dis.splitlines():
        s = line.split("//")[0].strip()
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", s)
        if m:
            if re.match(r"L\d+$", m.group(1)):
                label = m.group(1)
            else:
                name, label = m.group(1), None
                kernels[name] = []
            continue
        if name and s:
            parts = s.split(None, 1)
            kernels[name].append((label, parts[0], parts[1] if len(parts) > 1 else ""))
            label = None
    return kernels, meta


def from_asm(path):
    text = open(path).read()
    kernels, name, label = {}, None, None
    for line in text.splitlines():
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", s)
        if m:
            if m.group(1).startswith(".L"):
                label = m.group(1)
            elif m.group(1).startswith("_Z"):
                name, label = m.group(1), None
                kernels[name] = []
            continue
        if s.startswith(".") or name is None:
            if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".rodata"):
                name = None
            continue
        parts = s.split(None, 1)
        kernels[name].append((label, parts[0], parts[1] if len(parts) > 1 else ""))
        label = None
    return kernels, text


def blocks_of(body):
    """basic blocks [(first index, last index + 1, label)] and the branch edges (from index, to label)"""
    starts, edges = {0}, []
    for i, (label, mn, ops) in enumerate(body):
        if label:
            starts.add(i)
        if mn.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            starts.add(i + 1)
            if mn.startswith(("s_cbranch", "s_branch")):
                edges.append((i, ops.strip().split()[-1]))
    starts = sorted(s for s in starts if s < len(body))
    return [(s, e, body[s][0]) for s, e in zip(starts, starts[1:] + [len(body)])], edges


def census(body, rel):
    where = {label: i for i, (label, _, _) in enumerate(body) if label}
    blocks, edges = blocks_of(body)
    loops = sorted({(where[t], i) for i, t in edges if t in where and where[t] <= i})
    nested = [lp for lp in loops if any(o != lp and o[0] <= lp[0] and lp[1] <= o[1] for o in loops)]
    pool = nested or loops
    if not pool:
        return None
    loop = max(pool, key=lambda lp: lp[1] - lp[0])
    rows = []
    for s, e, label in blocks:
        if s < loop[0] or s > loop[1]:
            continue
        hist = collections.Counter()
        for _, mn, ops in body[s:e]:
            hist[classify(mn, "dpp" in mn or "row_" in ops or "wave_" in ops or "quad_perm" in ops)] += 1
        rows.append((label or "-", s - loop[0], e - s, hist))
    return loop, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source")
    ap.add_argument("kernel")
    ap.add_argument("--rates", default=RATES)
    ap.add_argument("--min-block", type=int, default=0, help="list only blocks of at least this many instructions (totals count all)")
    ap.add_argument("--ticks-per-iteration", type=float, default=None,
                    help="measured s_memtime ticks of one Newton iteration of THIS kernel (the flagship: 15600, "
                         "profiles/round3/stamps_flagship_final.txt): the loop text's ticks are then also printed as a share of it")
    args = ap.parse_args()
    rel, tick = read_rates(args.rates)
    kernels, meta_text = from_asm(args.source) if args.source.endswith((".s", ".S", ".asm")) else from_object(args.source)
    kernels = {k: v for k, v in kernels.items() if v}           # (a .s file labels its constant tables too)
    demangled = dict(zip(kernels, run("c++filt", *kernels.keys()).splitlines())) if kernels else {}
    hits = [k for k in kernels if args.kernel in short(demangled[k]) or args.kernel in k]
    if len(hits) != 1:
        print(f"{len(hits)} kernels match {args.kernel!r}:")
        for k in (hits or kernels):
            print("   ", short(demangled[k]))
        return 1
    k = hits[0]
    body = kernels[k]
    print(f"kernel   {short(demangled[k])}")
    md = metadata(meta_text, k)
    if md:
        print(f"registers  vgpr+agpr {md.get('vgpr_count', -1)} (agpr {md.get('agpr_count', -1)})  sgpr {md.get('sgpr_count', -1)}   "
              f"spilled: vgpr {md.get('vgpr_spill_count', -1)} sgpr {md.get('sgpr_spill_count', -1)}   scratch {md.get('private_segment_fixed_size', -1)} B/lane   "
              f"LDS {md.get('group_segment_fixed_size', -1)} B")
    res = census(body, rel)
    if res is None:
        print("no loop found")
        return 1
    loop, rows = res
    cols = ["fp64 arith", "fp32 arith", "rcp/rsq f64", "trans f32", "agpr move", "dpp move", "select", "other valu", "lds read", "lds write", "s_nop", "scalar", "memory"]
    print(f"whole kernel {len(body)} instructions; Newton loop: instructions {loop[0]} .. {loop[1]} ({loop[1] - loop[0] + 1})")
    print(f"{'block':>8s} {'at':>6s} {'instr':>6s} " + " ".join(f"{c:>11s}" for c in cols) + f" {'valu slots':>11s}")
    total, tslots = collections.Counter(), 0.0
    for label, at, n, hist in rows:
        slots = sum(slot_cost(c, rel) * v for c, v in hist.items())
        total.update(hist)
        tslots += slots
        if n >= args.min_block:
            print(f"{label:>8s} {at:6d} {n:6d} " + " ".join(f"{hist.get(c, 0):11d}" for c in cols) + f" {slots:11.1f}")
    n = sum(total.values())
    print(f"{'loop':>8s} {'':>6s} {n:6d} " + " ".join(f"{total.get(c, 0):11d}" for c in cols) + f" {tslots:11.1f}")
    valu = sum(total[c] for c in VALU_CLASSES)
    share = ""
    if args.ticks_per_iteration:
        share = (f" ({100.0 * tslots * tick / args.ticks_per_iteration:.1f} % of a {args.ticks_per_iteration:.0f}-tick iteration "
                 "if every block ran once)")
    print(f"loop text: {n} instructions, {valu} on the vector ALU, {tslots:.1f} issue slots = {tslots * tick:.0f} ticks at {tick} ticks per slot" + share)
    return 0


if __name__ == "__main__":
    sys.exit(main())
