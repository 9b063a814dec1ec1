#!/usr/bin/env python3
"""Vector-memory operations and vmcnt waits of one kernel in a hipcc -S listing, in listing order, per basic block.

Usage: tools/isa_waits.py <listing.s> <kernel-substring> [--all] [--meta]
For the first kernel whose mangled name contains the substring, prints every basic block that holds a vector-memory
operation or a wait on vmcnt as one line: label, line range, then the sequence of
    Ln  n consecutive vector-memory loads      Sn  n consecutive vector-memory stores
    w(k) an s_waitcnt that carries vmcnt(k)    |   an s_cbranch / s_branch (with its target)
--all also lists blocks with neither; --meta prints the kernel's NumVgprs, ScratchSize, Occupancy and LDSByteSize
(hipcc's own comment block behind the kernel) and nothing else.
profiles/load_queue_notes.md reads the source loop of k_hrtf_multi with it: between a trip's row request (the L8 after
the history store at F = 512) and the next trip's, no wait may carry a vmcnt below the number of rows just requested.
tools/isa_blocks.py counts the instructions of the same blocks.
"""
import re
import sys


def kernel_span(lines, sub):
    start = None
    for i, l in enumerate(lines):
        if re.match(r"^_Z\w*:", l) and sub in l.split(":")[0]:
            start = i
            break
    if start is None:
        raise SystemExit(f"no kernel matching {sub!r}")
    end = len(lines)
    for i in range(start + 1, len(lines)):
        if lines[i].startswith(".Lfunc_end"):
            end = i
            break
    return start, end


def meta(lines, end):
    out = {}
    for l in lines[end : end + 80]:
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize|NumSgprs): (\d+)", l)
        if m and m.group(1) not in out:
            out[m.group(1)] = int(m.group(2))
    return out


def main():
    path, sub = sys.argv[1], sys.argv[2]
    show_all = "--all" in sys.argv
    lines = open(path).read().splitlines()
    start, end = kernel_span(lines, sub)
    name = lines[start].split(":")[0]
    if "--meta" in sys.argv:
        print(name, " ".join(f"{k}={v}" for k, v in meta(lines, end).items()))
        return
    print("kernel", name)
    label, first, seq = "entry", start + 1, []

    def flush(last):
        if seq and (show_all or any(not t.startswith("|") for t in seq)):
            print(f"{label:12s} {first:6d}-{last:<6d} " + " ".join(seq))

    def bump(kind):
        if seq and seq[-1][0] == kind and seq[-1][1:].isdigit():
            seq[-1] = kind + str(int(seq[-1][1:]) + 1)
        else:
            seq.append(kind + "1")

    for i in range(start + 1, end):
        l = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            flush(i)
            label, first, seq = m.group(1), i + 1, []
            continue
        s = l.strip()
        if not s or s.startswith((";", ".", "//")):
            continue
        op = s.split()[0]
        if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            bump("S" if "_store" in op or "_atomic" in op else "L")
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                seq.append(f"w({m.group(1)})")
        elif op.startswith(("s_cbranch", "s_branch")):
            seq.append("|" + s.split()[-1])
    flush(end)


if __name__ == "__main__":
    main()
