#!/usr/bin/env python3
"""tools/isa_identity.py OLD NEW

Device code of two versions of the library, kernel by kernel.  OLD / NEW: a source tree (a directory that holds omok-ai_amd/csrc) or a git revision of this
repository.  net_kernels.hip, tree_kernels.hip and train_kernels.hip of both are compiled device-only with the Makefile's flags (tools/isa_hist.py: compile_code_object; tree_kernels.hip
with -ffp-contract=off) and the gfx950 code objects compared per demangled symbol:
  * the instruction sequence (mnemonics and operands; branch / call targets and address comments masked): identical or differing,
  * VGPR / AGPR / SGPR counts, LDS and scratch bytes from the code object's notes,
  * for differing kernels, side by side: the counts of MFMA, global / buffer loads and stores, LDS-DMA, ds_read, ds_write and s_barrier instructions and of
    s_waitcnt by immediate.
A kernel whose parameter list changed (another mangled name) is compared with its namesake and marked "signature changed".
Needs hipcc and the LLVM tools of ROCm, no GPU.  Exit status 0 whatever differs: the report is for reading."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_hist  # noqa: E402

FILES = (("net_kernels.hip", False), ("tree_kernels.hip", True), ("train_kernels.hip", False))  # (source, -ffp-contract=off)
COUNTED = [  # first match wins
    ("mfma", re.compile(r"^v_s?mfma")),
    ("lds-dma", re.compile(r"^(global|buffer)_load_lds")),
    ("vmem load", re.compile(r"^(global|buffer|flat)_load")),
    ("vmem store", re.compile(r"^(global|buffer|flat)_(store|atomic)")),
    ("scratch", re.compile(r"^scratch_")),
    ("ds_read", re.compile(r"^ds_read")),
    ("ds_write", re.compile(r"^ds_write")),
    ("s_barrier", re.compile(r"^s_barrier")),
]
NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def source_tree(arg):
    """directory of omok-ai_amd/csrc of a tree, or of a git revision unpacked into a temporary directory"""
    if os.path.isdir(os.path.join(arg, "omok-ai_amd", "csrc")):
        return os.path.join(os.path.abspath(arg), "omok-ai_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix="isa_identity_")
    tar = subprocess.run(["git", "-C", isa_hist.ROOT, "archive", arg, "omok-ai_amd/csrc", "include"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    return os.path.join(tmp, "omok-ai_amd", "csrc")


def kernels_of(co):
    """demangled name -> (masked instruction list, notes tuple or None for a device function)"""
    text = isa_hist.objdump(co)
    body, cur = collections.OrderedDict(), None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = body.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins or ins.endswith(":"):
            continue
        op = ins.split()[0]
        if op.startswith(("s_branch", "s_cbranch", "s_call")):
            ins = op + " <target>"
        cur.append(re.sub(r"<[^>]+>", "<sym>", ins))
    notes, entry = {}, None  # the notes' kernel list: entries start with "  - .key:", their own keys sit at that depth
    for line in subprocess.run([os.path.join(isa_hist.LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"^  (- |  )(\.[a-z_]+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            entry = {}
        if entry is not None:
            entry[m.group(2)] = m.group(3)
            if m.group(2) == ".name":
                notes[m.group(3)] = entry
    pretty = isa_hist.demangle(list(body))
    return {pretty[k]: (v, tuple(int(notes[k].get(key, 0)) for key in NOTE_KEYS) if k in notes else None) for k, v in body.items() if v}


def counts(ins):
    c = collections.Counter()
    for i in ins:
        op = i.split()[0]
        if op == "s_waitcnt":
            c[i] += 1
            continue
        for name, rx in COUNTED:
            if rx.match(op):
                c[name] += 1
                break
    return c


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old_dir, new_dir = source_tree(sys.argv[1]), source_tree(sys.argv[2])
    print(f"old: {sys.argv[1]}   new: {sys.argv[2]}   (vgpr, agpr, sgpr, lds bytes, scratch bytes)")
    for src, contract_off in FILES:
        old = kernels_of(isa_hist.compile_code_object(os.path.join(old_dir, src), "", contract_off))
        new = kernels_of(isa_hist.compile_code_object(os.path.join(new_dir, src), "", contract_off))
        # a symbol whose parameter list changed has another mangled name: it is compared with the old symbol of the same name in front of the parameter
        # list (template arguments included) if there is exactly one on either side, and listed as "signature changed"
        stem = lambda k: k.split("(")[0]
        lone_old, lone_new = [k for k in old if k not in new], [k for k in new if k not in old]
        resigned = []
        for k in lone_new:
            match = [o for o in lone_old if stem(o) == stem(k)]
            if len(match) == 1 and sum(stem(x) == stem(k) for x in lone_new) == 1:
                old[k] = old.pop(match[0])
                resigned.append(k)
        same = [k for k in new if k in old and new[k] == old[k]]
        differ = [k for k in new if k in old and new[k] != old[k]]
        print(f"\n{src}: old {len(old)} kernels and device functions, new {len(new)}: identical {len(same)}, differing {len(differ)}, "
              f"only in new {len(set(new) - set(old))}, only in old {len(set(old) - set(new))}, signature changed {len(resigned)}")
        for k in resigned:
            print(f"   signature changed: {stem(k)}")
        for k in sorted(set(new) - set(old)):
            print(f"   only in new: {k[:150]}")
        for k in sorted(set(old) - set(new)):
            print(f"   only in old: {k[:150]}")
        for k in same:
            print(f"   identical  {k.split('(')[0]}: {len(new[k][0])} instructions, {new[k][1]}")
        for k in differ:
            (io, no), (inn, nn) = old[k], new[k]
            print(f"   DIFFERS    {k.split('(')[0]}: instructions {len(io)} -> {len(inn)}, same sequence: {io == inn}, {no} -> {nn}")
            co, cn = counts(io), counts(inn)
            for name in sorted(set(co) | set(cn), key=lambda s: (s.startswith("s_waitcnt"), s)):
                print(f"      {name:40s} {co[name]:6d} {cn[name]:6d}{'' if co[name] == cn[name] else '   <--'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
