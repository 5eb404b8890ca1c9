#!/usr/bin/env python3
"""Device code of two checkouts, kernel by kernel (no GPU needed): the check of a refactor that must not change a kernel.

    python tools/codegen_compare.py PARENT_TREE CHANGE_TREE fused fused_bwd sweep_mv ... > profiles/<name>_codegen.txt
    python tools/codegen_compare.py PARENT_TREE CHANGE_TREE bf16=bf16_sweeps+bf16_color+bf16_dw backward dw

An argument is a unit both trees have, or PARENT_UNITS=CHANGE_UNITS ('+' between units) where kernels moved between units:
the kernels are then matched by symbol across the union of the units of each side.
Compiles csrc/<unit>.hip of both trees with the library's flags (buildid.py: COMMON_FLAGS + the unit's EXTRA_FLAGS) plus
`--cuda-device-only -S`, and compares per kernel: the resource counts of the code object's metadata (registers, spills, LDS,
scratch) and the number of MFMA, vector-memory load / store, LDS and barrier instructions — any difference there is a FAIL.
Where the instruction streams differ beyond that (labels and register numbers set aside) the line says how much and in which
opcodes; `identical` = the same instructions in the same order with the same operands."""
import collections
import concurrent.futures
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size"]
CLASSES = [("mfma", r"v_mfma"), ("vmem_ld", r"(buffer|global)_load"), ("vmem_st", r"(buffer|global)_(store|atomic)"),
           ("ds", r"ds_"), ("barrier", r"s_barrier")]


def compile_unit(tree, unit, out):
    pkg = os.path.join(tree, "rnb-neus-fork_amd")
    spec = importlib.util.spec_from_file_location("bid", os.path.join(pkg, "buildid.py"))
    bid = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bid)
    os.makedirs(os.path.join(pkg, "build"), exist_ok=True)
    idh = os.path.join(pkg, "build", "build_id.h")   # (api.hip includes it; its value is no device code)
    if not os.path.exists(idh):
        open(idh, "w").write('#define RNB_BUILD_ID "0"\n')
    cmd = (["hipcc"] + bid.COMMON_FLAGS + bid.EXTRA_FLAGS.get(unit + ".hip", []) +
           ["--cuda-device-only", "-S", os.path.join(pkg, "csrc", unit + ".hip"), "-o", out])
    subprocess.run(cmd, check=True, capture_output=True)


def parse(path):
    """-> ({symbol: {key: value}}, {symbol: [instruction, ...]})"""
    txt = open(path).read()
    meta, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == ".agpr_count":
            cur = {}
        if cur is None:
            continue
        if k in KEYS:
            cur[k] = v
        if k == ".symbol":
            cur["sym"] = v[:-3]
        if k == ".wavefront_size":
            meta[cur["sym"]] = cur
            cur = None
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        ins = []
        for ln in m.group(2).split("\n"):
            ln = ln.split(";")[0].strip()
            if ln and not ln.startswith(".") and not ln.endswith(":"):
                ins.append(re.sub(r"\.LBB\d+_\d+", "L", re.sub(r"\s+", " ", ln)))
        bodies[m.group(1)] = ins
    return meta, bodies


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n"))) if r.returncode == 0 else {n: n for n in names}


def main():
    parent, change = sys.argv[1], sys.argv[2]
    groups = []   # (parent units, change units)
    for arg in sys.argv[3:]:
        pu, _, cu = arg.partition("=")
        groups.append((pu.split("+"), (cu or pu).split("+")))
    tmp = tempfile.mkdtemp()
    jobs = [(t, u, os.path.join(tmp, f"{tag}_{u}.s")) for g in groups for tag, t, us in (("p", parent, g[0]), ("c", change, g[1]))
            for u in us]
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))

    def parse_union(tag, units):
        meta, bodies = {}, {}
        for u in units:
            m, b = parse(os.path.join(tmp, f"{tag}_{u}.s"))
            meta.update(m)
            bodies.update(b)
        return meta, bodies

    bad = 0
    for punits, cunits in groups:
        pm, pb = parse_union("p", punits)
        cm, cb = parse_union("c", cunits)
        same_syms = sorted(pm) == sorted(cm)
        name = lambda us: " + ".join(u + ".hip" for u in us)
        print(f"== {name(cunits) if punits == cunits else name(punits) + ' -> ' + name(cunits)}: {len(pm)} kernels at the parent, "
              f"{len(cm)} at the change; sorted symbol lists {'identical' if same_syms else 'DIFFER'}")
        if not same_syms:
            bad += 1
            for n in sorted(set(pm) ^ set(cm)):
                print("   only at the", "parent:" if n in pm else "change:", n)
        dm = demangle(sorted(set(pm) | set(cm)))
        for n in sorted(set(pm) & set(cm)):
            rp, rc = [pm[n].get(k) for k in KEYS], [cm[n].get(k) for k in KEYS]
            count = lambda b: [sum(1 for i in b if re.match(rx, i)) for _, rx in CLASSES]
            kp, kc = count(pb[n]), count(cb[n])
            ok = rp == rc and kp == kc
            if pb[n] == cb[n]:
                note = "identical"
            else:
                strip = lambda b: [re.sub(r"\b([sv])\[?\d+(:\d+)?\]?", r"\1N", i) for i in b]
                sp, sc = strip(pb[n]), strip(cb[n])
                ch = [(sp[a:b], sc[c:d]) for t, a, b, c, d in
                      difflib.SequenceMatcher(None, sp, sc, autojunk=False).get_opcodes() if t != "equal"]
                ops = collections.Counter(i.split(" ")[0] for x, y in ch for i in x + y)
                note = (f"{len(pb[n])} -> {len(cb[n])} instructions; register numbers aside, {sum(len(x) for x, _ in ch)} "
                        f"removed / {sum(len(y) for _, y in ch)} added: " + ", ".join(f"{k} x{v}" for k, v in ops.most_common(5)))
            print(f" {'ok  ' if ok else 'FAIL'} {dm[n]}")
            print(f"      vgpr/agpr/sgpr {rc[0]}/{rc[1]}/{rc[2]}  spills {rc[3]}/{rc[4]}  lds {rc[5]}  scratch {rc[6]} | "
                  + "  ".join(f"{c[0]} {v}" for c, v in zip(CLASSES, kc)) + f" | {note}")
            if not ok:
                bad += 1
                print(f"      AT THE PARENT: {rp} {kp}")
    print("RESULT:", "every resource and instruction-class count equal" if bad == 0 else f"{bad} FAILURES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
