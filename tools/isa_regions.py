"""Developer tool: static instruction counts of one kernel variant per PVT_MARK section of the step, by opcode CLASS -- f64 VALU, moves and selects, other VALU, exec-mask SALU, branches, literal s_mov, other SALU, waits, nops, LDS, memory.  No GPU needed.
usage: isa_regions.py [variant substring] [--asm file.s] [--md] [--all-variants]     (default variant: the lean headline kernel)

The tree is compiled to gfx950 assembly with build()'s flags plus -gline-tables-only (or --asm names an assembly made
that way) -- the plain-scene kernels alone (-DPVT_DEV_VARIANTS=1, half a minute; the same text kernel for kernel) unless
--all-variants asks for the whole library.  An instruction belongs to the section of the last line of the step loop's body that the `.loc` stream has
named: helpers inlined from above the loop and from pvt_math.h carry their own lines and inherit the section of their
caller this way (the line table has no inlined-at chain; the block layout makes this an approximation of a few per cent).
Sections are the source ranges between the `PVT_MARK(k);` lines of trace_body; the `tally_flush` lambda and
`tally_flush_call` are sections of their own.  Classes are prefixes and substrings of the mnemonic, never a list of opcodes."""
import collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_H = os.path.join(ROOT, "pvtrace_amd", "csrc", "pvt_trace_kernel.h")
CLASSES = ["f64 VALU", "v_mov + cndmask", "other VALU", "exec-mask SALU", "branches", "s_mov (literal)", "other SALU",
           "waits", "nops", "LDS", "memory"]
MARK_NAMES = {0: "refill + drain", 1: "node loop", 2: "absorption + emission", 3: "frame + normal", 4: "cosines",
              5: "Fresnel / reflect / refract", 6: "tally trip"}


def classify(op, operands):
    if op.startswith("v_"):
        if "_f64" in op:
            return "f64 VALU"
        if op.startswith(("v_mov_", "v_cndmask_", "v_accvgpr_")):
            return "v_mov + cndmask"
        return "other VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load_", "s_buffer_load_")):
        return "memory"
    if op.startswith("s_"):
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")):
            return "branches"
        if op.startswith("s_waitcnt"):
            return "waits"
        if op.startswith("s_nop"):
            return "nops"
        # lane-mask bookkeeping: every saveexec form, 64-bit mask logic, and moves to or from exec / vcc
        if "saveexec" in op or re.match(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor|not)_b64$", op) or \
                (op.startswith("s_mov_b64") and re.search(r"\b(exec|vcc)\b", operands)):
            return "exec-mask SALU"
        if op == "s_mov_b32" and re.search(r",\s*(0x[0-9a-f]+|-?\d+)\s*$", operands):
            v = operands.rsplit(",", 1)[1].strip()
            n = int(v, 16) if v.startswith("0x") else int(v)
            if not -16 <= n <= 64:   # (an inline constant is part of the instruction: not a literal)
                return "s_mov (literal)"
        return "other SALU"
    return None


def sections_of_source():
    """[(first line, last line, name)] of trace_body's step sections, from the PVT_MARK lines of the header."""
    lines = open(KERNEL_H).read().split("\n")
    marks = [(i + 1, int(m.group(1))) for i, l in enumerate(lines) for m in [re.search(r"^\s+PVT_MARK\((\d)\);", l)] if m]
    loop0 = max(i + 1 for i, l in enumerate(lines) if re.match(r"    for \(;;\) \{$", l) and i + 1 < marks[0][0])
    out, start = [], loop0
    for ln, k in marks:
        out.append((start, ln, MARK_NAMES.get(k, f"mark {k}")))
        start = ln + 1
    body_end = next(i + 1 for i, l in enumerate(lines) if i + 1 > marks[-1][0] and re.match(r"    tally_flush", l))
    out.append((start, body_end - 1, "loop end: lane retires, drain exit"))
    for pat, name in ((r"\s+auto tally_flush = \[&\]", "tally_flush"), (r"__device__ .*\btally_flush_call\(", "tally_flush_call")):
        for i, l in enumerate(lines):
            if re.match(pat, l):
                depth, j = 0, i
                while True:   # to the brace that closes it
                    depth += lines[j].count("{") - lines[j].count("}")
                    if depth == 0 and "{" in "".join(lines[i:j + 1]):
                        break
                    j += 1
                out.append((i + 1, j + 1, name))
    return out


def main():
    args = sys.argv[1:]
    asm = args[args.index("--asm") + 1] if "--asm" in args else None
    md = "--md" in args
    pos = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--asm")]
    variant = pos[0] if pos else "trace_kernel_lean_w4ILb0ELb0ELb1E"
    if asm is None:
        sys.path.insert(0, ROOT)
        import __graft_entry__   # build()'s own flags
        flags = [f for f in __graft_entry__.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
        asm = os.path.join(tempfile.mkdtemp(prefix="isar_"), "k.s")
        if "--all-variants" not in args:
            flags.append("-DPVT_DEV_VARIANTS=1")
        subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-gline-tables-only", "--cuda-device-only", "-S",
                               os.path.join(ROOT, "pvtrace_amd", "csrc", "pvt_trace.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    s = open(asm).read()
    files = dict(re.findall(r'\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', s)) or dict(re.findall(r'\.file\s+(\d+)\s+"([^"]+)"', s))
    secs = sections_of_source()

    def section_of(line):
        for a, b, name in secs:
            if a <= line <= b:
                return name
        return None

    # functions of the assembly: `name:  ; @name` ... `.Lfunc_end`; the kernel, and tally_flush_call where it exists
    funcs = [(m.group(1), s[m.end():s.index(".Lfunc_end", m.end())]) for m in re.finditer(r"^(\w+):\s+; @\1\s*$", s, re.M)]
    # (the tail functions too: `tail_runILb0ELi1ELi1ELb0ELb0ELi0ELi2E`, `tail_run_soloILi2E`)
    kernels = [(n, b) for n, b in funcs if variant in n and ("trace_kernel" in n or "tail_kernel" in n or "tail_run" in n)]
    called = [b for n, b in funcs if "tally_flush_call" in n]
    for name, body in kernels:
        body = "\n".join([body] + called)
        cur = "outside the loop"
        table = collections.defaultdict(collections.Counter)
        for line in body.split("\n"):
            line = line.strip()
            m = re.match(r"\.loc\s+(\d+)\s+(\d+)", line)
            if m:
                if os.path.basename(files.get(m.group(1), "")) == "pvt_trace_kernel.h":
                    sec = section_of(int(m.group(2)))
                    if sec:
                        cur = sec
                continue
            m = re.match(r"^([a-z][a-z_0-9]+)(?:\s+(.*?))?\s*(?:;.*)?$", line)
            if m:
                c = classify(m.group(1), m.group(2) or "")
                if c:
                    table[cur][c] += 1
        order = ["outside the loop"] + [n for _, _, n in secs]
        rows = [(n, table[n]) for n in order if sum(table[n].values())]
        total = collections.Counter()
        for _, c in rows:
            total.update(c)
        rows.append(("whole kernel", total))
        print(f"{'# ' if md else ''}{name}")
        if md:
            print("| section | " + " | ".join(CLASSES) + " | total |")
            print("|---|" + "---|" * (len(CLASSES) + 1))
            for n, c in rows:
                print(f"| {n} | " + " | ".join(str(c[k]) for k in CLASSES) + f" | {sum(c.values())} |")
        else:
            print(f"{'section':36s}" + "".join(f"{k[:11]:>12s}" for k in CLASSES) + f"{'total':>8s}")
            for n, c in rows:
                print(f"{n[:36]:36s}" + "".join(f"{c[k]:12d}" for k in CLASSES) + f"{sum(c.values()):8d}")


if __name__ == "__main__":
    main()
