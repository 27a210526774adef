#!/usr/bin/env python3
"""Instructions between two barriers of the lean sweeps, from a gfx950 listing of pg_kernels.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S pangenie_amd/csrc/pg_kernels.hip -o pg_kernels.s
    python tools/lean_step_listing.py pg_kernels.s [kernel-symbol-substring ...]

For every kernel named (default: the sparse phase-1 and phase-3 sweeps, k_sweep_lean<1,16,false> and <3,16,false>) it prints,
for every s_barrier in text order, the SHORTEST path from it to the next barrier over the kernel's branches — the rare bodies (a
zero-sum column, the upkeep of a block) only lengthen a path, so the shortest one is the common path of the step: the number of
instructions on it, and how many of them are fp64 arithmetic / LDS / scalar / branches / s_nop / global stores, and the wait states
the path's pads stand for (the sum of N + 1 over its `s_nop N`: work moved into a pad's place shortens the pad and leaves the
count of instructions as it was).  The store-free steps of the sparse loops are the paths with 80 or more fp64 operations and no
global store."""
import re
import sys

DEFAULT = ("_Z12k_sweep_leanILi1ELi16ELb0EE", "_Z12k_sweep_leanILi3ELi16ELb0EE")


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        body.append(line.rstrip("\n"))


def stretches(body):
    """per s_barrier: the SHORTEST path from it to the next barrier over the kernel's branches"""
    ins, label_at = [], {}
    for line in body:
        s = line.strip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            label_at[m.group(1)] = len(ins)
            continue
        if not s or s.startswith(";") or s.startswith("."):
            continue
        ins.append(s.split(";")[0].split())
    out = []
    for start, tok in enumerate(ins):
        if tok[0] != "s_barrier":
            continue
        # breadth-first from the instruction behind the barrier: every edge is one instruction
        prev, frontier, goal = {start + 1: None}, [start + 1], None
        while frontier and goal is None:
            nxt = []
            for pc in frontier:
                if pc >= len(ins):
                    continue
                op = ins[pc][0]
                if op in ("s_barrier", "s_endpgm"):
                    goal = pc
                    break
                succ = []
                if op != "s_branch":
                    succ.append(pc + 1)
                if (op == "s_branch" or op.startswith("s_cbranch")) and ins[pc][1] in label_at:
                    succ.append(label_at[ins[pc][1]])
                for q in succ:
                    if q not in prev:
                        prev[q] = pc
                        nxt.append(q)
            frontier = nxt
        cur = dict(n=0, f64=0, lds=0, salu=0, branch=0, nop=0, wait=0, store=0, end="no barrier" if goal is None else ("barrier" if ins[goal][0] == "s_barrier" else "end"))
        pc = prev.get(goal) if goal is not None else None
        while pc is not None:
            op = ins[pc][0]
            cur["n"] += 1
            cur["f64"] += op.endswith("_f64") or "_f64_" in op
            cur["lds"] += op.startswith("ds_")
            cur["branch"] += op.startswith("s_cbranch") or op == "s_branch"
            cur["salu"] += op.startswith("s_") and not op.startswith(("s_cbranch", "s_branch", "s_nop", "s_waitcnt"))
            cur["nop"] += op == "s_nop"
            if op == "s_nop":
                cur["wait"] += int(ins[pc][1], 0) + 1
            cur["store"] += op.startswith("global_store")
            pc = prev[pc]
        out.append(cur)
    return out


def main():
    path, want = sys.argv[1], tuple(sys.argv[2:]) or DEFAULT
    for name, body in kernels(path):
        if not any(w in name for w in want):
            continue
        print(name)
        for i, s in enumerate(stretches(body)):
            print(f"  stretch {i:3d}: {s['n']:4d} instructions  fp64 {s['f64']:3d}  lds {s['lds']:3d}  scalar {s['salu']:3d}  branches {s['branch']:2d}"
                  f"  s_nop {s['nop']:2d}  wait states {s['wait']:3d}  global stores {s['store']:2d}  ends at: {s['end']}")


if __name__ == "__main__":
    main()
