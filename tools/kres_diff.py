#!/usr/bin/env python3
"""What the compiler made of every kernel of one .hip source, before and after a change, as a markdown table: registers, spills,
scratch, LDS and occupancy from -Rpass-analysis=kernel-resource-usage, opcode classes counted in the gfx950 listing.

    tools/kres_diff.py BEFORE AFTER [-I include-dir]

BEFORE / AFTER: a .hip source, compiled here with the library's flags (--cuda-device-only -S; no GPU needed), or a prefix P whose
P.s and P.remarks (the compiler's stderr) are already there.  A cell with one number: equal; `a / b`: before / after.  Classes,
counted in operations (a v_pk_* instruction counts as two): fp = v_{add,sub,mul,max,min,exp,log,rcp,rsq,sqrt,cmp*}_f32 and their
packed forms; fma = v_fma*, v_fmac*, v_pk_fma*; cvt = v_cvt_*; scalar load = s_load_*, s_buffer_load_*; the rest as named.  Every other opcode whose count differs is listed."""
import collections
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
RES = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"), ("VGPR spill", "VGPRs Spill"), ("SGPR spill", "SGPRs Spill"),
       ("scratch B/lane", "ScratchSize [bytes/lane]"), ("LDS B", "LDS Size [bytes/block]"), ("occupancy", "Occupancy [waves/SIMD]")]
CLASSES = [("mfma", r"v_mfma_"), ("LDS", r"ds_"), ("global load", r"global_load_"), ("global store", r"global_store_"), ("scalar load", r"s_(buffer_)?load_"), ("scratch", r"scratch_"),
           ("fp", r"v_(pk_)?(add|sub|subrev|mul|max|min|exp|log|rcp|rsq|sqrt|cmp[a-z_]*)_f32"), ("fma", r"v_(pk_)?(fma|fmac)"), ("cvt", r"v_cvt_")]


def listing(arg, inc):
    if not arg.endswith(".hip"):
        return open(arg + ".s").read(), open(arg + ".remarks").read()
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I", inc or os.path.dirname(os.path.abspath(arg)), arg, "-o", os.path.join(d, "a.s")],
                           capture_output=True, text=True, check=True)
        return open(os.path.join(d, "a.s")).read(), r.stderr


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    clean = lambda n: re.sub(r"\(.*$", "", n.replace("(anonymous namespace)::", "").replace("void ", ""))
    return {m: clean(d) for m, d in zip(names, out)}


def kernels(arg, inc):
    asm, remarks = listing(arg, inc)
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(Function Name|[A-Za-z /\[\]]+?):\s+(.*?) \[-Rpass", line)
        if m and m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2).strip(), {})
        elif m and cur is not None:
            cur[m.group(1).strip()] = m.group(2).strip()
    ops, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = ops.setdefault(m.group(1), collections.Counter()) if m.group(1) in res else None
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            m = re.match(r"^\s+([a-z][a-z0-9_]*)(\s|$)", line)
            if m:
                cur[m.group(1)] += 1
    names = demangle(sorted(res))
    return {names[k]: (res[k], ops.get(k, collections.Counter())) for k in res}


def classes(ops):
    out, rest = collections.Counter(), collections.Counter()
    for op, n in ops.items():
        for name, pat in CLASSES:
            if re.match(pat, op):
                out[name] += n * (2 if op.startswith("v_pk_") else 1)
                break
        else:
            rest[op] += n
    return out, rest


def main():
    args = [a for a in sys.argv[1:]]
    inc = args.pop(args.index("-I") + 1) if "-I" in args else None
    args = [a for a in args if a != "-I"]
    before, after = kernels(args[0], inc), kernels(args[1], inc)
    cell = lambda a, b: str(a) if a == b else f"{a} / {b}"
    print(f"{len(before)} functions before, {len(after)} after" + ("" if sorted(before) == sorted(after) else "; NOT the same set: "
          + ", ".join(sorted(set(before) ^ set(after)))))
    heads = [h for h, _ in RES] + [c for c, _ in CLASSES] + ["instructions", "other opcodes that differ"]
    print("| kernel | " + " | ".join(heads) + " |")
    print("|" + "---|" * (len(heads) + 1))
    for k in sorted(set(before) & set(after)):
        (ra, oa), (rb, ob) = before[k], after[k]
        (ca, xa), (cb, xb) = classes(oa), classes(ob)
        other = [f"`{op}` {xa[op]}/{xb[op]}" for op in sorted(set(xa) | set(xb)) if xa[op] != xb[op]]
        row = [cell(ra.get(key, "?"), rb.get(key, "?")) for _, key in RES] + [cell(ca[c], cb[c]) for c, _ in CLASSES]
        row += [cell(sum(oa.values()), sum(ob.values())), ", ".join(other) or "none"]
        print(f"| `{k}` | " + " | ".join(row) + " |")


if __name__ == "__main__":
    main()
