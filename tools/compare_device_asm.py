#!/usr/bin/env python3
"""Is a translation unit's device code the same before and after a change?  Compares two gfx950 assembly files
(hipcc <the Makefile's flags> --cuda-device-only -S x.hip -o x.s), kernel by kernel, keyed by demangled name:
the instructions between the kernel's label and its last s_endpgm, and its .amdhsa_ resource lines.

    tools/compare_device_asm.py OLD.s NEW.s [--allow REGEX ...] [--shrunk REGEX ...] [--gone REGEX ...]

A kernel is named without its parameter list (template arguments stay), so one that lost a parameter is still paired.
--allow: kernels that may differ; the figures that decide occupancy (VGPRs, LDS and scratch bytes) must still be equal and
the instruction count must not grow; the differing lines are printed.  --shrunk: kernels that lost instrumentation: those
figures and the count may fall, none may grow.  --gone: kernels of OLD that NEW may lack.  Exit status 0 iff everything
else is identical and NEW has no kernel OLD lacks.  Needs no GPU: it reads two text files."""
import argparse
import difflib
import re
import subprocess
import sys

KEPT = ("next_free_vgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    res = {}
    for name, d in zip(names, out.splitlines()):
        depth, i = 0, len(d)
        while True:                                      # cut the parameter list: the last top-level (...)
            i -= 1
            depth += (d[i] == ")") - (d[i] == "(")
            if depth == 0:
                break
        res[name] = d[:i].removeprefix("void ")
    assert len(set(res.values())) == len(names), "overloaded kernels: key by the full signature"
    return res


def kernels(path):
    lines = open(path).read().split("\n")
    res, cur = {}, None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
        elif ln.strip() == ".end_amdhsa_kernel":
            cur = None
        elif cur:
            k, v = ln.split()
            res[cur][k[len(".amdhsa_"):]] = v
    body = {}
    for name in res:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        text = []
        for ln in lines[start + 1:end]:
            ln = ln.split(";")[0].strip()
            if ln and not ln.startswith("."):            # instructions only: no directives
                text.append(ln)
            elif re.match(r"\.LBB\d+_\d+:", ln):
                text.append(ln)
        # block labels carry the kernel's position in the file; string it out of labels and branch targets
        text = [re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t) for t in text]
        while text and text[-1] != "s_endpgm":           # padding after the last s_endpgm
            text.pop()
        body[name] = text
    names = demangle(list(res))
    return {names[k]: (res[k], body[k]) for k in res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", action="append", default=[])
    ap.add_argument("--shrunk", action="append", default=[])
    ap.add_argument("--gone", action="append", default=[])
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    bad = 0
    print(f"{a.old}: {len(old)} kernels; {a.new}: {len(new)} kernels")
    for k in sorted(set(new) - set(old)):
        print("ADDED   ", k)
        bad += 1
    for k in sorted(set(old) - set(new)):
        ok = any(re.search(r, k) for r in a.gone)
        print("gone (allowed)" if ok else "MISSING ", k)
        bad += not ok
    same = 0
    for k in sorted(set(old) & set(new)):
        (ro, bo), (rn, bn) = old[k], new[k]
        if ro == rn and bo == bn:
            same += 1
            continue
        shrunk = any(re.search(r, k) for r in a.shrunk)
        if not shrunk and not any(re.search(r, k) for r in a.allow):
            print("DIFFERS ", k, f"({len(bo)} -> {len(bn)} instructions)")
            bad += 1
            continue
        ok = all(int(rn[f]) <= int(ro[f]) if shrunk else rn[f] == ro[f] for f in KEPT) and len(bn) <= len(bo)
        print("allowed " if ok else "ALLOWED BUT OUT OF BOUNDS ", k, f"({len(bo)} -> {len(bn)} instructions)")
        bad += not ok
        for f in sorted(set(ro) | set(rn)):
            if ro.get(f) != rn.get(f):
                print(f"    .amdhsa_{f}: {ro.get(f)} -> {rn.get(f)}")
        diff = [d for d in difflib.unified_diff(bo, bn, lineterm="", n=0) if not d.startswith(("---", "+++"))]
        for d in diff[:16]:
            print("    " + d)
        if len(diff) > 16:
            print(f"    ... {len(diff) - 16} more diff lines")
    print(f"identical (instructions and resources): {same} kernels")
    print("VERDICT:", "FAIL" if bad else "ok")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
