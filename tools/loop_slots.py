#!/usr/bin/env python3
"""Issue slots per pass of the marked loops of a kernel, by instruction class (CPU, static).

    bash tools/isa.sh out.s && python tools/loop_slots.py out.s [--kernel SUBSTR] [--json F] [--hash]

One wave alone issues an instruction every few cycles whatever its class, so the length of a single
wave's loop is its instruction count, all classes, not its VALU count.  This tool reads the assembly
text tools/isa.sh writes and counts, per marked loop, the instructions of one pass on the hot path.

Markers are empty asm statements in the source whose comment the assembler text keeps
(D2D_LOOP_MARK in d2d_device.h):

    ; D2D_LOOP begin NAME   a block on the cycle of loop NAME (one report per occurrence: an inlined
                            loop appears once per call site)
    ; D2D_LOOP cold WHAT    a block that is not on the hot path (the knot scan)
    ; D2D_LOOP opt WHAT     a block only some passes take (the parabolic candidate): counted in the
                            `full` row, left out of the `skip` row

The hot path of a loop is the longest pass (a cycle through the `begin` block in the kernel's
control-flow graph, by instruction count) that enters no `cold` block; `skip` is the longest that
also enters no `opt` block.  Instructions are told apart by mnemonic prefix only:

    valu_f64      v_*  with _f64 in the mnemonic         scalar   s_* other than the three below
    valu_cndmask  v_cndmask*                             wait     s_waitcnt*
    valu_mov      v_mov*                                 nop      s_nop
    valu_other    every other v_*                        branch   s_branch, s_cbranch*, s_setpc*, s_endpgm
    lds           ds_*                                   vmem     global_* flat_* buffer_* scratch_*

--hash prints, per kernel, the body hash of tools/isa.sh's last column with the marker statements
taken out: equal to the unmarked tree's column exactly when the markers changed nothing else.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import re
import sys

CLASSES = ["valu_f64", "valu_cndmask", "valu_mov", "valu_other", "scalar", "lds", "vmem", "wait", "nop", "branch"]
VALU = CLASSES[:4]
MARK = re.compile(r"^\s*;\s*D2D_LOOP\s+(begin|cold|opt)\s+(\w+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
FALL = re.compile(r"^; %bb\.(\d+):")
DEFAULT_KERNEL = "d2d_step_kernelILb1ELb1ELb0E"


def classify(mn: str) -> str:
    """Class of an instruction from its mnemonic's prefix."""
    if mn.startswith("v_"):
        if mn.startswith("v_cndmask"):
            return "valu_cndmask"
        if mn.startswith("v_mov"):
            return "valu_mov"
        return "valu_f64" if "_f64" in mn else "valu_other"
    if mn.startswith("s_"):
        if mn.startswith("s_waitcnt"):
            return "wait"
        if mn == "s_nop":
            return "nop"
        if mn.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm")):
            return "branch"
        return "scalar"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "other"


def kernels(text: str) -> dict:
    """name -> body lines of every function of the file (label line to .Lfunc_end)."""
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        out[m.group(1)] = m.group(2).split("\n")
    return out


class Block:
    def __init__(self, name):
        self.name, self.ins, self.marks, self.succ = name, [], [], []


def blocks(lines) -> dict:
    """Basic blocks of a function body: a label, a `; %bb.N:` comment or the instruction after a
    branch starts one; successors from the terminating branch and the fall-through."""
    bl, order = {}, []

    def new(name):
        b = Block(name)
        bl[name] = b
        order.append(b)
        return b

    cur, n_anon = new("entry"), 0
    for ln in lines:
        s = ln.strip()
        m = LABEL.match(s) or FALL.match(s)
        if m:
            cur = new(m.group(1))
            continue
        mk = MARK.match(s)
        if mk:
            cur.marks.append((mk.group(1), mk.group(2)))
            continue
        if not s or s[0] in ";.":
            continue
        if cur.ins and classify(cur.ins[-1][0]) == "branch":
            n_anon += 1
            cur = new(f"after{n_anon}")
        tok = s.split(None, 1)
        cur.ins.append((tok[0], tok[1].split(";")[0].strip() if len(tok) > 1 else ""))
    for i, b in enumerate(order):
        nxt = order[i + 1].name if i + 1 < len(order) else None
        last = b.ins[-1] if b.ins else None
        if last and classify(last[0]) == "branch":
            mn, arg = last
            if mn == "s_branch":
                b.succ = [arg]
            elif mn.startswith("s_cbranch"):
                b.succ = [arg] + ([nxt] if nxt else [])
        elif nxt:
            b.succ = [nxt]
        b.succ = [x for x in b.succ if x in bl]
    return bl


def loop_nodes(bl, head):
    """The blocks on some cycle through `head`: reachable from it and reaching it."""
    def reach(start, edges):
        seen, todo = {start}, [start]
        while todo:
            for y in edges(todo.pop()):
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        return seen
    pred = {}
    for b in bl.values():
        for y in b.succ:
            pred.setdefault(y, []).append(b.name)
    return reach(head, lambda x: bl[x].succ) & reach(head, lambda x: pred.get(x, []))


def longest_pass(bl, head, banned, budget=2_000_000):
    """The longest simple cycle head -> ... -> head by instruction count that enters no banned block."""
    nodes = loop_nodes(bl, head) - banned
    best, steps = (-1, None), [0]

    def go(x, path, n):
        nonlocal best
        steps[0] += 1
        if steps[0] > budget:
            raise RuntimeError("loop too branchy for an exhaustive walk")
        for y in bl[x].succ:
            if y == head:
                if n > best[0]:
                    best = (n, list(path))
            elif y in nodes and y not in path:
                path.append(y)
                go(y, path, n + len(bl[y].ins))
                path.pop()
    go(head, [head], len(bl[head].ins))
    return best[1]


def count(bl, path) -> dict:
    c = dict.fromkeys(CLASSES + ["other"], 0)
    for x in path:
        for mn, _ in bl[x].ins:
            c[classify(mn)] += 1
    c["valu"] = sum(c[k] for k in VALU)
    c["total"] = sum(c[k] for k in CLASSES + ["other"])
    c["blocks"] = len(path)
    if not c["other"]:
        del c["other"]
    return c


def report(text: str, kernel: str = DEFAULT_KERNEL) -> list:
    """[{kernel, loop, occurrence, full: {...}, skip: {...}}] for every `begin` marker of the kernels
    whose name contains `kernel`."""
    out = []
    for name, lines in sorted(kernels(text).items()):
        if kernel not in name:
            continue
        bl = blocks(lines)
        cold = {b.name for b in bl.values() if any(k == "cold" for k, _ in b.marks)}
        opt = {b.name for b in bl.values() if any(k == "opt" for k, _ in b.marks)}
        seen = {}
        for b in bl.values():
            for kind, loop in b.marks:
                if kind != "begin":
                    continue
                seen[loop] = seen.get(loop, 0) + 1
                row = {"kernel": name, "loop": loop, "occurrence": seen[loop]}
                for tag, ban in (("full", cold), ("skip", cold | opt)):
                    p = longest_pass(bl, b.name, ban - {b.name})
                    row[tag] = count(bl, p) if p else None
                out.append(row)
    return out


def body_hashes(text: str) -> dict:
    """tools/isa.sh's body hash per d2dk kernel, the marker statements (and the asm brackets left
    empty by them) removed first."""
    res = {}
    for name in re.findall(r"^(_ZN4d2dk\w+):", text, re.M):
        blk = text[text.index("\n" + name + ":") + 1:]
        body = blk[:re.search(r"^\.Lfunc_end\d+:", blk, re.M).start()]
        body = re.sub(r"[ \t]*;;#ASMSTART\n[ \t]*; D2D_LOOP[^\n]*\n[ \t]*;;#ASMEND\n", "", body)
        body = re.sub(r"BB\d+_", "BB_", re.sub(r"__hip_cuid_\w+", "__hip_cuid", body))
        body = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", body)
        body = re.sub(r"[ \t]+", " ", body)
        res[name] = hashlib.sha256(body.encode()).hexdigest()[:12]
    return res


def fmt(rows) -> str:
    cols = ["total", "valu"] + CLASSES
    out = [f"{'loop':14s} {'path':5s} " + " ".join(f"{c[:9]:>9s}" for c in cols)]
    for r in rows:
        for tag in ("full", "skip"):
            c = r[tag]
            if c is None:
                continue
            out.append(f"{r['loop'] + '#' + str(r['occurrence']):14s} {tag:5s} " + " ".join(f"{c[k]:9d}" for k in cols))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, help="substring of the (mangled) kernel name")
    ap.add_argument("--json", default=None)
    ap.add_argument("--hash", action="store_true", help="body hashes with the markers removed, as tools/isa.sh prints them")
    a = ap.parse_args()
    text = open(a.asm).read()
    if a.hash:
        for k, v in sorted(body_hashes(text).items()):
            print(f"{k:60s} {v}")
        return
    rows = report(text, a.kernel)
    if not rows:
        sys.exit(f"no `; D2D_LOOP begin` marker in a kernel matching {a.kernel!r}")
    for k in sorted({r["kernel"] for r in rows}):
        print("#", k)
        print(fmt([r for r in rows if r["kernel"] == k]))
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
