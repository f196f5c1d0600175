#!/usr/bin/env python3
"""Per-block table of the eight Linear launches of a CSWinBlock that a DropPath sample order reaches (four forward Linears, three
data gradients, the block tail), one tree against another, as profiles/drop_path_skip_notes.md shows it:
    block_linear_table.py BEFORE_sequence.txt AFTER_sequence.txt kept.txt
The sequence files are tools/rocpd_last_step.py's ordered lists of one replayed step of bench.py (26 blocks); kept.txt has one line
`<block name> <kept by rs1> <kept by rs2>` per block in forward order (read from the blocks' factors after an identical run).  The
launches are found by their place around each block's attention kernels."""
import re
import sys



def load(path):
    rows = []
    for ln in open(path):
        m = re.match(r"\s*([\d.]+) us\s+\+\s*([\d.]+)\s+gap\s+(-?[\d.]+)\s+(.*)", ln)
        rows.append((float(m.group(2)), m.group(4).strip()))
    return rows


def blocks(rows):
    fwd = [i for i, (_, n) in enumerate(rows) if "attn_fwd3" in n]
    bwd = [i for i, (_, n) in enumerate(rows) if "attn_bwd3" in n]
    assert len(fwd) == len(bwd) == 26
    out, used = [], set()
    for k, f in enumerate(fwd):
        b = bwd[25 - k]
        idx = dict(qkv=f - 1, proj=f + 1, fc1=f + 3, fc2=f + 4, dfc2=b - 4, dfc1=b - 3, dproj=b - 1, tail=b + 1)
        assert "ln_fwd" in rows[f + 2][1] and "ln_bwd" in rows[b - 2][1] and "tail" in rows[b + 1][1], (k, rows[f + 2], rows[b - 2], rows[b + 1])
        for i in idx.values():
            assert "gemm" in rows[i][1], rows[i]
            used.add(i)
        out.append({k2: rows[i][0] for k2, i in idx.items()})
    other = sum(t for i, (t, _) in enumerate(rows) if i not in used)
    return out, other, len(rows) - len(used)


P, B = load(sys.argv[1]), load(sys.argv[2])
bp, op, np_ = blocks(P)
bb, ob, nb_ = blocks(B)
kept = [ln.split() for ln in open(sys.argv[3]) if "stage" in ln and len(ln.split()) == 3]
assert len(kept) == 26
keys = ["qkv", "proj", "fc1", "fc2", "dfc2", "dfc1", "dproj", "tail"]
print("| # | block | kept rs1 / rs2 | " + " | ".join(keys) + " | parent sum | branch sum | drop |")
print("|---|---|---|" + "---|" * (len(keys) + 3))
tot = {k: [0.0, 0.0] for k in keys}
S = 0.0
prop = 0.0
for i, (name, k1, k2) in enumerate(kept):
    p, b = bp[i], bb[i]
    sp, sb = sum(p.values()), sum(b.values())
    S += sp - sb
    cells = []
    for k in keys:
        tot[k][0] += p[k]; tot[k][1] += b[k]
        cells.append(f"{p[k]:.1f} / {b[k]:.1f}")
    d1, d2 = 1 - int(k1) / 24, 1 - int(k2) / 24
    prop += d1 * (p["qkv"] + p["proj"] + p["dproj"]) + d2 * (p["fc1"] + p["fc2"] + p["dfc2"] + p["dfc1"])
    print(f"| {i + 1} | {name.replace('cswin_unet.', '')} | {k1} / {k2} | " + " | ".join(cells) + f" | {sp:.1f} | {sb:.1f} | {sp - sb:+.1f} |")
print(f"| sum | | | " + " | ".join(f"{tot[k][0]:.1f} / {tot[k][1]:.1f}" for k in keys) +
      f" | {sum(v[0] for v in tot.values()):.1f} | {sum(v[1] for v in tot.values()):.1f} | {S:+.1f} |")
print()
print(f"S = {S:.1f} us; proportional share of the seven stand-alone launches by this step's draws = {prop:.1f} us")
for k in keys:
    print(f"class {k}: parent {tot[k][0]:.1f} us, branch {tot[k][1]:.1f} us, drop {tot[k][0] - tot[k][1]:+.1f}")
# per class, the proportional share by draws
share = {k: 0.0 for k in keys}
for i, (name, k1, k2) in enumerate(kept):
    d1, d2 = 1 - int(k1) / 24, 1 - int(k2) / 24
    for k in keys:
        share[k] += (d1 if k in ("qkv", "proj", "dproj") else d2 if k != "tail" else 0.0) * bp[i][k]
for k in keys:
    if share[k]:
        print(f"class {k}: proportional {share[k]:.1f} us, realised {(tot[k][0] - tot[k][1]) / share[k] * 100:.0f} %")
print(f"other launches: parent {np_} launches {op:.1f} us, branch {nb_} launches {ob:.1f} us")
for rows, t in ((P, "parent"), (B, "branch")):
    for i, (tm, n) in enumerate(rows):
        if "distribution" in n or "drop_path_order" in n or "uniform" in n.lower():
            print(t, i, [(round(a, 1), b[:90]) for a, b in rows[i:i + 5]])
            break
