#!/usr/bin/env python3
"""Per-basic-block instruction classes of one kernel's code IN FRONT of its first loop, from the compiler's assembly.

    hipcc <build._flags(SRC)> --cuda-device-only -S splatloc_amd/csrc/SRC -o SRC.s
    tools/isa_blocks.py SRC.s MANGLED_NAME_PREFIX [--off BLOCK,BLOCK,...]

Prints, for every basic block from the kernel's entry up to the first label that a LATER branch jumps BACK to (the header of
the first loop: in composite_bwd_kernel the chunk loop), the number of vector-ALU, matrix, scalar-ALU, scalar-memory,
vector-memory and LDS instructions, waits, lane moves between the register files (v_readlane / v_writelane: spill traffic
of scalar registers) and branches, then the totals.  Static counts: a wave runs one path through these blocks; --off names
the blocks a given launch does not run (read off the branches) and adds the total without them.
"""
import re
import sys


def classify(op):
    if op.startswith(("v_readlane", "v_writelane")):
        return "lane"
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return None


def main():
    path, prefix = sys.argv[1], sys.argv[2]
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(rf"{re.escape(prefix)}\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start + 1:end + 1]
    cols = ["valu", "mfma", "salu", "smem", "vmem", "lds", "wait", "lane", "branch"]
    # basic blocks: a label starts one, a branch ends one
    blocks, order = {}, []

    def open_block(name):
        blocks[name] = {"n": dict.fromkeys(cols, 0), "succ": [], "fall": True, "vm0": 0}
        order.append(name)
        return name

    cur, anon = open_block("entry"), 0
    for l in body:
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            if blocks[cur]["fall"]:
                blocks[cur]["succ"].append(m.group(1))
            cur = open_block(m.group(1))
            continue
        m = re.match(r"\s+([a-z_0-9]+)(?:\s+(\S+))?", l)
        k = classify(m.group(1)) if m else None
        if not k:
            continue
        if not blocks[cur]["fall"]:      # code behind an unconditional branch without a label: unreachable padding
            continue
        blocks[cur]["n"][k] += 1
        blocks[cur]["vm0"] += bool(re.search(r"s_waitcnt.*vmcnt\(0\)", l))
        if k == "branch":
            op, tgt = m.group(1), m.group(2)
            if op.startswith("s_cbranch"):
                anon += 1
                nxt = f"{cur}+{anon}"
                blocks[cur]["succ"] += [tgt, nxt]
                blocks[cur]["fall"] = False
                cur = open_block(nxt)
            else:
                if op == "s_branch":
                    blocks[cur]["succ"].append(tgt)
                blocks[cur]["fall"] = False
    # loop headers = targets of back edges (depth-first search from the entry)
    headers, state = set(), {}

    def dfs(root):
        stack = [(root, iter(blocks[root]["succ"]))]
        state[root] = 1
        while stack:
            node, it = stack[-1]
            for t in it:
                if t not in blocks:
                    continue
                if state.get(t) == 1:
                    headers.add(t)
                elif t not in state:
                    state[t] = 1
                    stack.append((t, iter(blocks[t]["succ"])))
                    break
            else:
                state[node] = 2
                stack.pop()

    dfs("entry")
    # the set-up: everything reachable from the entry without entering a loop
    seen, todo = set(), ["entry"]
    while todo:
        b = todo.pop()
        if b in seen or b in headers or b not in blocks:
            continue
        seen.add(b)
        todo += blocks[b]["succ"]
    # (a conditional branch splits a labelled block into pieces NAME, NAME+k, k counting the kernel's conditional branches)
    off = set(sys.argv[sys.argv.index("--off") + 1].split(",")) if "--off" in sys.argv else set()
    blocks = [(b + (" (off)" if b in off else ""), dict(blocks[b]["n"], vm0=blocks[b]["vm0"])) for b in order if b in seen]
    vm0 = sum(c["vm0"] for _, c in blocks)
    print(f"{'block':16s}" + "".join(f"{c:>8s}" for c in cols))
    for n, c in blocks:
        if any(c.values()):
            print(f"{n:16s}" + "".join(f"{c[k]:8d}" for k in cols))
    tot = {k: sum(c[k] for _, c in blocks) for k in cols}
    print(f"{'total':16s}" + "".join(f"{tot[k]:8d}" for k in cols))
    if off:
        on = {k: sum(c[k] for n, c in blocks if not n.endswith("(off)")) for k in cols}
        print(f"{'without (off)':16s}" + "".join(f"{on[k]:8d}" for k in cols))
    print(f"blocks: {sum(1 for _, c in blocks if any(c.values()))}   s_waitcnt with vmcnt(0) in front of the loop: {vm0}")


if __name__ == "__main__":
    main()
