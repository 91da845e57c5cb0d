#!/usr/bin/env python3
"""Diff of two builds of libpscv.so, per kernel symbol: the gfx950 instruction streams (addresses and comments dropped) and the
resource rows of kernel_resources.py.  One line per kernel whose name contains a given substring (default: conv3d), "identical" or the
instruction-class counts and resource rows of both; every other kernel of the library is only counted, and named if it differs.
Usage: python scripts/dev/isa_diff.py before.so after.so [substring ...]"""
import os, re, shutil, subprocess, sys, tempfile
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lint_isa
import kernel_resources

CLASSES = [("mfma", r"v_s?mfmac?_"), ("buf_ld", r"buffer_load"), ("buf_st", r"buffer_store"), ("glb_ld", r"global_load"),
           ("glb_st", r"global_store"), ("lds_rd", r"ds_(read|load)"), ("lds_wr", r"ds_(write|store)"), ("wait", r"s_waitcnt")]


def streams(lib_path):
    """{kernel symbol: [instruction text]} over every gfx950 code object of the library."""
    od, out = lint_isa.objdump(), {}
    with tempfile.TemporaryDirectory() as td:
        lib = os.path.join(td, "lib.so")
        shutil.copy(lib_path, lib)
        subprocess.run([od, "--offloading", lib], cwd=td, capture_output=True, check=True)
        for f in sorted(x for x in os.listdir(td) if "amdgcn" in x):
            cur = None
            for line in subprocess.run([od, "-d", "--no-show-raw-insn", os.path.join(td, f)], capture_output=True, text=True, check=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif cur is not None and line.startswith(("\t", " ")) and line.strip():
                    cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())
    return out


def counts(ins):
    return " ".join(f"{k}={sum(1 for i in ins if re.match(p, i))}" for k, p in CLASSES)


def main():
    before, after, pats = sys.argv[1], sys.argv[2], sys.argv[3:] or ["conv3d"]
    sa, sb = streams(before), streams(after)
    ra, rb = ({r[0]: " / ".join(r[1:6]) for r in kernel_resources.resources(p)} for p in (before, after))
    names = dict(zip(sorted(set(sa) | set(sb)), kernel_resources.demangle(sorted(set(sa) | set(sb)))))
    others = other_diff = 0
    for sym, name in sorted(names.items(), key=lambda kv: kv[1]):
        if sym not in ra and sym not in rb:
            continue                                    # not a kernel (a device function kept out of line)
        same = sa.get(sym) == sb.get(sym) and ra.get(sym) == rb.get(sym)
        if not any(p in name for p in pats):
            others += 1
            other_diff += not same
            if not same:
                print(f"DIFFERS (outside the selection): {name}")
            continue
        if same:
            print(f"identical  [{ra[sym]}]  {name}")
        elif sym not in sa or sym not in sb:
            print(f"{'only before' if sym in sa else 'only after'}  {name}")
        else:
            print(f"differs    {name}\n    before: {len(sa[sym])} instr, {counts(sa[sym])}, vgpr / agpr / sgpr / lds_static / scratch = {ra[sym]}\n"
                  f"    after:  {len(sb[sym])} instr, {counts(sb[sym])}, vgpr / agpr / sgpr / lds_static / scratch = {rb[sym]}")
    print(f"{others} kernels outside the selection: {other_diff} differ")


if __name__ == "__main__":
    main()
