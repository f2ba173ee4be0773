#!/usr/bin/env python3
"""kernel_diff.py <a.s> <b.s> -- per-kernel diff of two device assembly files (hipcc -S --cuda-device-only of the same
translation unit at two revisions, e.g. before and after a refactor that should only have moved code).

Per kernel, compared: the text of its body (from its label to its end label, the kernel descriptor included) after dropping
comments and renumbering the function ordinal in local labels (.LBB<n>_k, .Lfunc_end<n>: they change when kernels change
order in the file), and its metadata (register, spill, LDS, private-segment and kernarg sizes).  Prints one line per kernel;
exit status 1 if any kernel differs or exists on one side only."""
import difflib
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")
LOCAL = re.compile(r"(\.L[A-Za-z_]+?)\d+(_\d+)?\b")


def kernels(path):
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    start = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln and not ln[0].isspace() and ln.split(":")[0] in set(names)}
    out = {}
    for name in names:
        body = []
        for ln in lines[start[name] + 1:]:
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].strip()
            if ln:
                body.append(LOCAL.sub(lambda m: m.group(1) + "#" + (m.group(2) or ""), ln))
        out[name] = {"body": body, "meta": {}}
    for block in re.split(r"\n  - (?=\.agpr_count)", "\n".join(lines)[("\n".join(lines)).index("amdhsa.kernels:"):]):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and m.group(1) in out:
            out[m.group(1)]["meta"] = {k: re.search(re.escape(k) + r":\s+(\S+)", block).group(1) for k in META}
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("ONLY IN %s  %s" % (a_path if name in a else b_path, name))
            bad += 1
            continue
        same_body, same_meta = a[name]["body"] == b[name]["body"], a[name]["meta"] == b[name]["meta"]
        print("%-9s %6d lines  %s" % ("identical" if same_body and same_meta else "DIFFERS", len(a[name]["body"]), name))
        if not same_meta:
            for k in META:
                if a[name]["meta"].get(k) != b[name]["meta"].get(k):
                    print("    %s: %s -> %s" % (k, a[name]["meta"].get(k), b[name]["meta"].get(k)))
        if not same_body:
            for ln in list(difflib.unified_diff(a[name]["body"], b[name]["body"], a_path, b_path, lineterm="", n=2))[:60]:
                print("    " + ln)
        bad += not (same_body and same_meta)
    print("%d kernels in %s, %d in %s, %d differ" % (len(a), a_path, len(b), b_path, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
