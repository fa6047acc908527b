#!/usr/bin/env python3
"""The wait ledger of a kernel's prologue: what a wave waits for before its first step.

Compiles one translation unit of csrc/ to gfx950 assembly with the flags the Makefile gives it (no GPU needed) and, for every
kernel whose demangled name contains one of the given patterns, prints in program order

  * every s_waitcnt before the header of the main loop, with the memory operations it waits for (vector memory retires in order,
    so vmcnt(n) leaves the last n; scalar loads return in any order, so only lgkmcnt(0) retires them), and what kind of wait it is:
    a DEPENDENT ROUND TRIP (it waits for an operation that was issued after the previous round trip had been waited for), a wait
    for operations that were in flight together with the previous round trip, a scalar load of kernel-argument lines that an
    earlier load has already brought into the scalar cache, or a wait on LDS operations alone;
  * the waits inside the first pass of the main loop, with their counts and the number of operations left in flight.

The main loop is the first loop (a label the compiler remarks as a loop header) of at least --min-loop instructions: the step loop of
a rollout, the refill-batch loop of the fused sweep (its first pass is listed up to the first loop nested in it).  Block order in
the text stands for execution order, which holds for the straight-line prologues this is for.  A development aid: compiler versions move its output.

usage: scripts/list_prologue_waits.py UNIT PATTERN [PATTERN ...] [--csrc DIR] [--keep FILE.s] [--min-loop K]
  e.g. scripts/list_prologue_waits.py rollout_quad 'simulate_quad_kernel<false>' 'linesearch_quad_kernel<false>'
"""
import argparse
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quattro-transformer-ilqr_amd", "csrc")

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
FUNC = re.compile(r"^(_Z\w+):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
BRANCH = re.compile(r"^s_c?branch\w*$")
WAIT_FIELD = re.compile(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)")


def assembly(unit, csrc, keep):
    """The unit's device assembly, through the Makefile's own compile line."""
    line = None
    out = subprocess.run(["make", "-C", csrc, "-n", "-B", unit + ".o"], check=True, capture_output=True, text=True).stdout
    for l in out.splitlines():
        if " -c " in l and unit + ".hip" in l:
            line = l
    if line is None:
        sys.exit(f"no compile line for {unit}.o in the Makefile")
    words = shlex.split(line)
    i = words.index("-o")
    del words[i:i + 2]
    words.remove("-c")
    tmp = tempfile.mkdtemp()
    s_path = os.path.join(tmp, unit + ".s")
    try:
        subprocess.run(words + ["-S", "--cuda-device-only", "-o", s_path], check=True, cwd=csrc)
        if keep:
            shutil.copy(s_path, keep)
        return open(s_path).read().splitlines()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(tool):
        tool = shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool] + names, check=True, capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def functions(lines):
    """{mangled name: [(label or None, mnemonic, operands)]} for every function of the unit."""
    fns, cur = {}, None
    for l in lines:
        m = FUNC.match(l)
        if m:
            cur = fns.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
            continue
        m = LABEL.match(l)
        if m:
            cur.append((m.group(1), None, "loop" if "Loop Header" in l else ""))
            continue
        if "Loop Header" in l and l.lstrip().startswith(";") and cur and cur[-1][0]:   # (a nested header: the remark has a line of its own)
            cur[-1] = (cur[-1][0], None, "loop")
            continue
        m = INSN.match(l)
        if m and not l.lstrip().startswith((".", ";")):
            cur.append((None, m.group(1), m.group(2).split(";")[0].strip()))
    return fns


def loops(body):
    """[(index of the header label, index of the last branch back to it)] in the order of the headers."""
    where = {lab: i for i, (lab, _, mark) in enumerate(body) if lab and mark == "loop"}   # (the compiler's own loop remarks)
    found = {}
    for i, (_, op, args) in enumerate(body):
        if op and BRANCH.match(op):
            tgt = args.split(",")[-1].strip()
            if tgt in where and where[tgt] < i:
                found[where[tgt]] = i
    return sorted(found.items())


def main_loop(body, min_insns):
    """The first loop of at least min_insns instructions, and the header of the first loop nested in it (or its back branch)."""
    ls = loops(body)
    for head, back in ls:
        if sum(1 for x in body[head:back] if x[1]) >= min_insns:
            inner = [h for h, _ in ls if head < h < back]
            return head, back, (inner[0] if inner else back)
    return None


def kind(op):
    """'vm' / 'lgkm' for an instruction that one of the two counters tracks, else None."""
    if op.startswith(("s_load", "s_buffer_load")):
        return "lgkm"
    if op.startswith("ds_") and not op.startswith(("ds_nop",)):
        return "lgkm"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")) and not op.startswith(("buffer_wbl2", "buffer_inv", "buffer_gl")):
        return "vm"
    return None


def brief(op, args):
    a = args.replace(" ", "")
    return f"{op} {a}" if len(a) <= 44 else f"{op} {a[:41]}..."


SLOAD = re.compile(r"^s_load_dword(x\d+)?$")
KBASE_ADD = re.compile(r"^(s\d+),\s*s0,\s*(0x[0-9a-f]+|\d+)$")


class Op:
    def __init__(self, at, text, lines=None, lds=False):
        self.at, self.text, self.lines, self.lds = at, text, lines, lds   # lines: kernel-argument lines a scalar load touches


def ledger(name, body, min_insns):
    loop = main_loop(body, min_insns)
    if loop is None:
        print(f"{name}: no loop found")
        return
    head, back, stop = loop
    print(f"== {name}")
    print(f"   main loop: {body[head][0]}, {sum(1 for x in body[head:back] if x[1])} instructions; "
          f"{sum(1 for x in body[:head] if x[1])} instructions before it")
    vm, lgkm = [], []
    # the kernel-argument segment is s[0:1] at entry; a copy advanced by a constant (s_add_u32 sN, s0, K with its s_addc) is followed
    kbase = {"s[0:1]": 0}
    cached = set()          # 64-byte lines of the segment that a finished scalar load has brought into the scalar cache
    trips = hits = lds_waits = waits = 0
    last_trip = -1          # where the last counted round trip was waited for
    print("   -- before the loop")
    for i, (lab, op, args) in enumerate(body[:stop + 1]):
        if i == head:
            print(f"   prologue: {waits} waits: {trips} dependent memory round trips, {hits} on kernel-argument lines fetched before "
                  f"(scalar-cache hits), {lds_waits} on LDS alone, {waits - trips - hits - lds_waits} with nothing new to wait for")
            print(f"   pending at the loop header: vm {len(vm)}, lgkm {len(lgkm)}")
            print("   -- first pass of the loop")
        if op is None:
            continue
        m = KBASE_ADD.match(args) if op == "s_add_u32" else None
        if m:
            n = int(m.group(1)[1:])
            kbase[f"s[{n}:{n + 1}]"] = int(m.group(2), 0)
        k = kind(op)
        if k == "vm":
            vm.append(Op(i, brief(op, args)))
        elif k == "lgkm":
            lines = None
            m = SLOAD.match(op)
            parts = [x.strip() for x in args.split(",")]
            if m and len(parts) == 3 and parts[1] in kbase and re.fullmatch(r"0x[0-9a-f]+|\d+", parts[2]):
                lo = kbase[parts[1]] + int(parts[2], 0)
                hi = lo + 4 * int((m.group(1) or "x1")[1:]) - 1
                lines = set(range(lo // 64, hi // 64 + 1))
            lgkm.append(Op(i, brief(op, args), lines, op.startswith("ds_")))
        elif op == "s_waitcnt":
            f = dict((a, int(b)) for a, b in WAIT_FIELD.findall(args))
            done = []
            if "vmcnt" in f and len(vm) > f["vmcnt"]:
                done += vm[:len(vm) - f["vmcnt"]]
                vm = vm[len(vm) - f["vmcnt"]:]
            if "lgkmcnt" in f and len(lgkm) > f["lgkmcnt"]:   # (scalar loads return in any order: only a count of 0 says they are back)
                done += lgkm if f["lgkmcnt"] == 0 else [x for x in lgkm[:len(lgkm) - f["lgkmcnt"]] if x.lds]
                lgkm = [] if f["lgkmcnt"] == 0 else [x for x in lgkm if x not in done]
            if i >= head:
                print(f"   s_waitcnt {args:<24} in flight after it: vm {len(vm)}, lgkm {len(lgkm)}")
                continue
            waits += 1
            mem = [x for x in done if not x.lds and not (x.lines is not None and x.lines <= cached)]
            if not done:
                what = "nothing to wait for"
            elif mem and any(x.at > last_trip for x in mem):
                trips += 1
                last_trip = i
                what = f"ROUND TRIP {trips}"
            elif mem:
                what = "issued before the last round trip's wait: in flight with it"
            elif all(x.lds for x in done):
                lds_waits += 1
                what = "LDS only"
            else:
                hits += 1
                what = "kernel-argument lines fetched before: scalar-cache hits"
            print(f"   s_waitcnt {args:<24} {what}")
            for x in done:
                print(f"        {x.text}")
            for x in done:
                if x.lines:
                    cached |= x.lines
    print()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit")
    ap.add_argument("patterns", nargs="+")
    ap.add_argument("--csrc", default=CSRC, help="the csrc directory to compile from (another checkout's, for a comparison)")
    ap.add_argument("--keep", help="also leave the assembly in this file")
    ap.add_argument("--min-loop", type=int, default=100, help="instructions a loop must have to count as the main loop")
    a = ap.parse_args()
    fns = functions(assembly(a.unit, os.path.abspath(a.csrc), a.keep))
    names = demangle(list(fns))
    found = False
    for pat in a.patterns:
        for mangled, body in fns.items():
            if pat in names[mangled]:
                found = True
                ledger(names[mangled], body, a.min_loop)
    if not found:
        sys.exit("no kernel matches: " + ", ".join(a.patterns))


if __name__ == "__main__":
    main()
