#!/usr/bin/env python3
"""Where a kernel's waves wait on vector memory, read from the generated code (no GPU needed).

    python tools/vm_trace.py UNIT [KERNEL_SUBSTRING ...] [--tree DIR]
    python tools/vm_trace.py color_h2 color_bwd_h2_kernel
    python tools/vm_trace.py fused 'fused_forward_kernel<2, true, 4, true, true>'

Compiles csrc/UNIT.hip device-only to assembly with the library's flags (buildid.py: COMMON_FLAGS + the unit's EXTRA_FLAGS)
and prints, for every kernel whose demangled name contains one of the substrings (all kernels when none is given):

  * registers, scratch, LDS and occupancy as the compiler reports them, and
  * the run-length trace of the instruction classes that matter for the vector-memory counter, basic block by basic block:

        L<n>   n vector loads (buffer_load / global_load)          sL<n>  n scratch loads (spill reloads)
        S<n>   n vector stores or atomics                          sS<n>  n scratch stores (spills)
        W(k)   s_waitcnt with vmcnt(k)                             B      s_barrier
        M<n>   n MFMAs

gfx950 has ONE counter, vmcnt, for vector loads and vector stores, retired in issue order: W(k) waits until at most k of the
loads AND stores issued before it are outstanding.  A wait for a load therefore also waits for every store issued before that
load — `S2 W(2)` behind a load is a wait for the two stores that precede the load in the stream.  Every other instruction
class is left out of the trace; nothing else is looked at."""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the compiler prints behind every kernel of the assembly
RESOURCES = [("NumVgprs", "vgprs"), ("NumAgprs", "agprs"), ("TotalNumSgprs", "sgprs"), ("ScratchSize", "scratch"),
             ("LDSByteSize", "lds"), ("Occupancy", "occupancy")]
CLASSES = [("sL", re.compile(r"scratch_load")), ("sS", re.compile(r"scratch_store")),
           ("L", re.compile(r"(buffer|global|flat)_load")), ("S", re.compile(r"(buffer|global|flat)_(store|atomic)")),
           ("M", re.compile(r"v_mfma")), ("B", re.compile(r"s_barrier"))]
VMCNT = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")


def compile_unit(unit, tree=ROOT, out=None):
    """csrc/<unit>.hip of `tree` -> device assembly (path returned)"""
    pkg = os.path.join(tree, "rnb-neus-fork_amd")
    spec = importlib.util.spec_from_file_location("rnb_buildid", os.path.join(pkg, "buildid.py"))
    bid = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bid)
    if out is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vm_trace_"), unit + ".s")
    cmd = (["hipcc"] + bid.COMMON_FLAGS + bid.EXTRA_FLAGS.get(unit + ".hip", []) +
           ["--cuda-device-only", "-S", os.path.join(pkg, "csrc", unit + ".hip"), "-o", out])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {unit}.hip:\n{r.stderr}")
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n"))) if r.returncode == 0 else {n: n for n in names}


def parse(path):
    """-> {symbol: {"name", "res": {vgprs, agprs, sgprs, scratch, lds, occupancy}, "blocks": [(label, [token, ...])]}}"""
    txt = open(path).read()
    kernels = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^_Z\w+:\s*; @|\Z)", txt, re.S | re.M):
        sym, body, tail = m.group(1), m.group(2), m.group(3)
        res = {}
        for key, name in RESOURCES:
            r = re.search(r";\s*" + key + r":\s*(\d+)", tail)
            if r:
                res[name] = int(r.group(1))
        if "occupancy" not in res:
            continue   # (a device function, not a kernel)
        blocks, cur = [], ("entry", [])
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith("."):
                lab = re.match(r"(\.LBB\d+_\d+):", ln)
                if lab:
                    blocks.append(cur)
                    cur = (lab.group(1), [])
                continue
            w = VMCNT.match(ln)
            if w:
                cur[1].append(f"W({w.group(1)})")
                continue
            for tok, rx in CLASSES:
                if rx.match(ln):
                    cur[1].append(tok)
                    break
        blocks.append(cur)
        kernels[sym] = {"res": res, "blocks": blocks}
    dm = demangle(sorted(kernels))
    for sym, k in kernels.items():
        k["name"] = re.sub(r"^void ", "", dm[sym])
    return kernels


def run_length(tokens):
    out, i = [], 0
    while i < len(tokens):
        j = i
        while j < len(tokens) and tokens[j] == tokens[i]:
            j += 1
        t = tokens[i]
        if t.startswith("W") or t == "B":
            out.append(t if j - i == 1 else f"{t}x{j - i}")
        else:
            out.append(f"{t}{j - i}")
        i = j
    return out


def kernels_of(unit, substrings=(), tree=ROOT):
    """the parsed kernels of one unit whose demangled names contain one of `substrings` (every kernel when empty)"""
    ks = parse(compile_unit(unit, tree))
    return {s: k for s, k in ks.items() if not substrings or any(x in k["name"] for x in substrings)}


def report(kernels, out=sys.stdout):
    for sym in sorted(kernels, key=lambda s: kernels[s]["name"]):
        k = kernels[sym]
        r = k["res"]
        toks = [t for _, b in k["blocks"] for t in b]
        n = lambda p: sum(1 for t in toks if t == p)
        waits = [int(t[2:-1]) for t in toks if t.startswith("W")]
        print(f"== {k['name']}", file=out)
        print(f"   vgprs {r.get('vgprs')}  agprs {r.get('agprs')}  sgprs {r.get('sgprs')}  scratch {r.get('scratch')} B/lane  "
              f"lds {r.get('lds')} B  occupancy {r.get('occupancy')} waves/SIMD", file=out)
        print(f"   loads {n('L')}  stores {n('S')}  scratch loads {n('sL')}  scratch stores {n('sS')}  mfma {n('M')}  "
              f"barriers {n('B')}  vmcnt waits {len(waits)} (of them vmcnt(0): {sum(1 for w in waits if w == 0)})", file=out)
        for label, b in k["blocks"]:
            if b:
                line = " ".join(run_length(b))
                print(f"   {label + ':':<12}{line}", file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", help="csrc/<unit>.hip")
    ap.add_argument("kernel", nargs="*", help="substring of the demangled kernel name")
    ap.add_argument("--tree", default=ROOT, help="checkout to compile (default: this one)")
    a = ap.parse_args()
    ks = kernels_of(a.unit, a.kernel, a.tree)
    if not ks:
        print("no kernel matches", file=sys.stderr)
        return 1
    report(ks)
    return 0


if __name__ == "__main__":
    sys.exit(main())
