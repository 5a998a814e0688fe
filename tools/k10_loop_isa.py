"""Dev tool: static instruction counts of kernel 10's steady-state loop from a `hipcc -S` gfx950 .s file.

The loop is the innermost backward branch whose span holds the two unrolled tiles' MFMAs.  Inside it, the
basic blocks that hold an MFMA, an LDS-DMA or a stage barrier are the steady state (every wave runs them
at every tile); the others are the slow path and the slot-table refresh, reported apart.

    python tools/k10_loop_isa.py k10_768.s ILi10ELi768ELb0E
"""
import re
import sys
from collections import Counter


def classify(op):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def kernel_body(text, pat):
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\s*s_endpgm", text, re.S | re.M):
        if pat in m.group(1):
            return m.group(1), m.group(2)
    raise SystemExit(f"no kernel matching {pat}")


def main():
    text = open(sys.argv[1]).read()
    name, body = kernel_body(text, sys.argv[2] if len(sys.argv) > 2 else "")
    lines = [ln.strip() for ln in body.split("\n")]
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    n_mfma_all = sum(1 for ln in lines if ln.startswith("v_mfma"))
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)|^s_branch\s+(\.LBB\d+_\d+)", ln)
        if not m:
            continue
        tgt = label_at.get(m.group(1) or m.group(2))
        if tgt is None or tgt >= i:
            continue
        n = sum(1 for x in lines[tgt:i] if x.startswith("v_mfma"))
        if n >= 48 and (best is None or i - tgt < best[1] - best[0]):
            best = (tgt, i, n)
    if best is None:
        raise SystemExit("no loop found")
    lo, hi, n_mfma = best
    blocks, cur = [], []
    for ln in lines[lo:hi + 1]:
        if re.match(r"^\.LBB\d+_\d+:", ln) and cur:
            blocks.append(cur)
            cur = []
        cur.append(ln)
    blocks.append(cur)
    steady, other = Counter(), Counter()
    nops = 0
    for b in blocks:
        ins = [ln.split()[0] for ln in b if ln and not ln.startswith((";", ".", "//")) and not ln.endswith(":")]
        hot = any(o.startswith("v_mfma") or o == "s_barrier" for o in ins) or any(" lds" in ln for ln in b)
        for o in ins:
            (steady if hot else other)[classify(o)] += 1
            if hot and o == "s_nop":
                nops += 1
    md = re.search(r"\.name:\s+" + re.escape(name) + r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    sg = re.search(r"\.name:\s+" + re.escape(name) + r".*?\.sgpr_spill_count:\s+(\d+)", text, re.S)
    print(name[:100])
    print(f"  MFMAs in the kernel {n_mfma_all}, in the loop {n_mfma}; loop lines {hi - lo}")
    print(f"  steady-state blocks: {dict(steady)} (s_nop among SALU: {nops})")
    for k in ("VALU", "SALU", "LDS", "VMEM"):
        print(f"    {k} per MFMA {steady[k] / max(steady['MFMA'], 1):.3f}")
    print(f"  other blocks in the loop (slow path, refresh): {dict(other)}")
    if md:
        print(f"  vgpr_count {md.group(1)} vgpr_spill_count {md.group(2)} sgpr_spill_count {sg.group(1) if sg else '?'}")


if __name__ == "__main__":
    main()
