#!/usr/bin/env python3
"""What the compiler made of the local pass (CPU only, no GPU needed):
compile numamma_amd/csrc/nmg_route.hip to gfx950 assembly with the Makefile's
HIPFLAGS and print, per local_kernel instance,

  * VGPRs, SGPR spills, VGPR spills, scratch bytes, LDS bytes, occupancy;
  * for the chunk loop: the instruction classes by prefix, the number of
    exec-region opens (s_*_saveexec), conditional branches, s_nop and
    lane reloads of spilled SGPRs (v_readlane_b32);
  * the chunk loop's LDS read groups: the reads issued back to back before
    the first s_waitcnt lgkmcnt that follows them.  A step of the common path
    that serves both chunks of a pair with one round trip shows as a group of
    kLC (or a multiple) reads of one width; a group with a single read of a
    width is a round trip that serves one chunk only ("single").

The chunk loop is found from the loop notes the compiler writes into the
assembly ("Loop Header: Depth=N", "Child Loop BBx_y Depth N"): the item loop
is the depth-1 loop with the most loops inside it, the chunk loop its depth-2
child with the largest extent.  A loop's extent runs from its header label to the
last branch back to that label; cold blocks the compiler placed behind the
latch, and their jumps back into the loop, are not part of it.

  tools/isa_stats.py [--kernel SUBSTR] [--src FILE] [--asm FILE]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "numamma_amd")
KLC = 2  # chunks per group (nmg_route.hip kLC)


def makefile_flags():
    """HIPCC and HIPFLAGS as numamma_amd/Makefile gives them (ARCH = gfx950)."""
    var = {}
    for line in open(os.path.join(PKG, "Makefile")):
        m = re.match(r"^(\w+)\s*[:?]?=\s*(.*)$", line.rstrip("\n"))
        if m:
            var.setdefault(m.group(1), m.group(2))
    var["ARCH"] = "gfx950"

    def expand(s):
        for _ in range(4):
            s = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
        return s

    return os.environ.get("HIPCC", expand(var["HIPCC"])), expand(var["HIPFLAGS"]).split()


def compile_asm(src, out):
    hipcc, flags = makefile_flags()
    cmd = [hipcc, *flags, "-x", "hip", "--offload-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, cwd=PKG, stderr=subprocess.DEVNULL)


def kernel_meta(text):
    """name -> dict of the amdhsa.kernels metadata block's scalar fields."""
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        d = dict(re.findall(r"\.(\w+):\s+(\S+)", blk.split("\namdhsa.", 1)[0]))
        if "name" in d:
            meta[d["name"]] = d
    return meta


def kernel_bodies(text):
    """name -> (instruction / label lines of the function, loop headers).  Headers: label -> (depth,
    [(child label, child depth)], [labels of blocks noted "in Loop: Header=" this one]), from the compiler's
    loop notes on the label's comment lines."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines, heads, cur, inloop = [], {}, None, []
        for raw in m.group(2).split("\n"):
            code, _, note = raw.partition(";")
            ln = code.strip()
            lab = re.match(r"^(\.LBB\d+_\d+):", ln)
            if lab:
                cur = lab.group(1)
            elif ln:
                cur = None
            if cur:
                h = re.search(r"Loop Header: Depth=(\d+)", note)
                if h:
                    heads[cur] = (int(h.group(1)), [], [])
                b = re.search(r"in Loop: Header=(BB\d+_\d+) ", note)
                if b:
                    inloop.append((cur, ".L" + b.group(1)))
                c = re.search(r"Child Loop (BB\d+_\d+) Depth (\d+)", note)
                if c and cur in heads:
                    heads[cur][1].append((".L" + c.group(1), int(c.group(2))))
            if ln and not ln.startswith(".") or lab:
                lines.append(ln)
        for lab, head in inloop:
            if head in heads:
                heads[head][2].append(lab)
        out[m.group(1)] = (lines, heads)
    return out


def extent(lines, heads, label):
    """(start, end) line indices of the loop headed by `label`, to the last branch back to it.  A rotated loop's
    latch jumps to a block of the loop laid out ahead of the header: the extent starts there."""
    at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    head = at[label]
    entry = {label} | {b for b in heads[label][2] if at[b] < head}
    back = [(i, m.group(1)) for i, ln in enumerate(lines) if i > head
            for m in [re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)$", ln)] if m and m.group(1) in entry]
    return (min(at[t] for _, t in back), max(i for i, _ in back)) if back else None


def chunk_loop(lines, heads):
    size = lambda e: e[1] - e[0] if e else -1
    items = [l for l, (d, kids, _) in heads.items() if d == 1 and kids]
    if not items:
        return None
    item = max(items, key=lambda l: len(heads[l][1]))  # (its own back-edge may go through a block ahead of its header)
    kids = [extent(lines, heads, l) for l, d in heads[item][1] if d == 2]
    kids = [k for k in kids if k]
    return max(kids, key=size) if kids else None


def klass(op):
    if op.startswith(("ds_", "lds_")):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vector-memory"
    if op.startswith("s_load") or op.startswith("s_buffer_load") or op.startswith("s_memtime"):
        return "scalar-memory"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("v_"):
        return "vector-ALU"
    return "other"


def read_groups(body):
    """Runs of LDS reads up to the first lgkmcnt wait after them: list of Counter(opcode)."""
    groups, cur = [], collections.Counter()
    for ln in body:
        op = ln.split()[0]
        if re.match(r"ds_read|ds_load", op):
            cur[op] += 1
        elif cur and (ln.endswith(":") or op.startswith(("s_cbranch", "s_branch")) or
                      (op == "s_waitcnt" and "lgkmcnt" in ln)):
            # (a block edge ends a group too: what follows is another exec region)
            groups.append(cur)
            cur = collections.Counter()
    if cur:
        groups.append(cur)
    return groups


def report(name, meta, lines, heads, out):
    d = meta.get(name, {})
    vg = int(d.get("vgpr_count", 0))
    occ = min(8, 512 // max(vg, 1)) if vg else 0
    print(f"{name}", file=out)
    print(f"  vgprs {vg}  occupancy {occ}  sgpr_spills {d.get('sgpr_spill_count')}  vgpr_spills "
          f"{d.get('vgpr_spill_count')}  scratch_bytes {d.get('private_segment_fixed_size')}  "
          f"lds_bytes {d.get('group_segment_fixed_size')}", file=out)
    cl = chunk_loop(lines, heads)
    if cl is None:
        print("  chunk loop: not found", file=out)
        return
    body = [ln for ln in lines[cl[0]:cl[1] + 1] if not ln.endswith(":")]
    ops = [ln.split()[0] for ln in body]
    by = collections.Counter(klass(op) for op in ops)
    print(f"  chunk loop {lines[cl[0]][:-1]}: {len(body)} instructions  " + "  ".join(f"{k} {v}" for k, v in sorted(by.items())), file=out)
    cnt = lambda pred: sum(1 for op in ops if pred(op))
    print(f"  exec_opens {cnt(lambda o: '_saveexec' in o)}"
          f"  cbranch {cnt(lambda o: o.startswith('s_cbranch'))}"
          f"  cbranch_execz {cnt(lambda o: o.startswith('s_cbranch_execz') or o.startswith('s_cbranch_execnz'))}"
          f"  s_nop {cnt(lambda o: o == 's_nop')}  lane_reloads {cnt(lambda o: o == 'v_readlane_b32')}"
          f"  lane_spills {cnt(lambda o: o == 'v_writelane_b32')}"
          f"  scratch_ops {cnt(lambda o: o.startswith('scratch_'))}", file=out)
    vm = sorted({m.group(1) for ln in body for m in [re.search(r"vmcnt\((\d+)\)", ln)] if m}, key=int)
    print(f"  vmcnt waits seen: {' '.join(vm)}", file=out)
    gs = read_groups(lines[cl[0]:cl[1] + 1])
    single = sum(1 for g in gs if any(v % KLC for v in g.values()))
    print(f"  LDS read groups {len(gs)}  with an unpaired read {single}", file=out)
    for g in gs:
        tag = "single" if any(v % KLC for v in g.values()) else "paired"
        print("    " + tag + "  " + "  ".join(f"{k} x{v}" for k, v in sorted(g.items())), file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="local_kernel", help="substring of the (mangled) kernel names to report")
    ap.add_argument("--src", default=os.path.join(PKG, "csrc", "nmg_route.hip"))
    ap.add_argument("--asm", help="read this assembly file, compile nothing")
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "nmg_route.s")
            compile_asm(os.path.abspath(args.src), path)
            text = open(path).read()
    meta, bodies = kernel_meta(text), kernel_bodies(text)
    names = sorted(n for n in bodies if args.kernel in n and n in meta)
    if not names:
        sys.exit(f"no kernel matching {args.kernel!r}")
    for n in names:
        report(n, meta, *bodies[n], sys.stdout)


if __name__ == "__main__":
    main()
