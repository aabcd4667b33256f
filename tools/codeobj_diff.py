"""Which kernels differ between two builds of libm3p2i_hip.so (no GPU needed): per kernel of the gfx950 code objects,
whether the instruction text is the same once addresses, encodings, symbol names and the padding behind the last instruction are
dropped, and whether the metadata
is (VGPRs, AGPRs, SGPRs, spill counts, scratch, LDS, kernarg size).  A kernel whose name exists on one side only is matched
to a kernel of the other side with the same instructions and metadata, and reported as RENAMED; what is left is NEW or
REMOVED.  It only compares.

    python tools/codeobj_diff.py parent/libm3p2i_hip.so m3p2i_aip_amd/lib/libm3p2i_hip.so > kernels_changed_vs_parent.txt
"""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj_info as info   # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size")


def bodies(co):
    """symbol -> the instruction lines of its disassembly: mnemonic and operands, without the address / encoding comment."""
    out = subprocess.run([f"{info.LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    res, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = res.setdefault(m.group(1), [])
        elif cur is not None and line.startswith(("\t", " ")):
            text = line.split("//")[0].strip()
            if text:
                cur.append(re.sub(r"\s+", " ", text))
    for lines in res.values():   # the padding between a function's last instruction and the next function is not its code
        while lines and lines[-1] in ("s_nop 0", "..."):
            lines.pop()
    return res


def load(lib):
    """mangled name -> (demangled name, metadata tuple, sha256 of the instruction text, instruction count)"""
    tmp, cos = info.extract(lib)
    res = {}
    try:
        for co in cos:
            ks = info.kernels(co)
            body = bodies(co)
            for k, d in zip(ks, info.demangle([k["name"] for k in ks])):
                lines = body.get(k["name"], [])
                res[k["name"]] = (re.sub(r"\(.*$", "", d), tuple(k.get(m) for m in META),
                                  hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    old, new = load(argv[0]), load(argv[1])
    rows, counts = [], collections.Counter()
    only_new = collections.defaultdict(list)   # (metadata, instructions) -> names that exist in the second library only
    for name in sorted(set(new) - set(old)):
        only_new[new[name][1:3]].append(name)
    for name in sorted(old):
        dem, meta, text, n = old[name]
        twin, verdict = name, "IDENTICAL"
        if name not in new:
            if not only_new[(meta, text)]:
                rows.append(("REMOVED", dem, ""))
                counts["removed"] += 1
                continue
            twin, verdict = only_new[(meta, text)].pop(0), "RENAMED"
        what = []
        if new[twin][2] != text:
            what.append("instructions %d -> %d" % (n, new[twin][3]))
        what += ["%s %s -> %s" % (m, a, b) for m, a, b in zip(META, meta, new[twin][1]) if a != b]
        if what:
            verdict = "CHANGED"
        counts[verdict.lower()] += 1
        rows.append((verdict, dem, ("-> " + new[twin][0] if twin != name else "") + ("  [" + "; ".join(what) + "]" if what else "")))
    for names in only_new.values():
        for name in names:
            rows.append(("NEW", new[name][0], ""))
            counts["new"] += 1
    print("per-kernel llvm-objdump -d of the gfx950 code objects: instruction text (addresses, encodings and symbol names dropped) and")
    print("metadata (%s)" % ", ".join(META))
    print("first library %d kernels, second %d: identical %d, renamed with identical code %d, changed %d, new %d, removed %d"
          % (len(old), len(new), counts["identical"], counts["renamed"], counts["changed"], counts["new"], counts["removed"]))
    order = {"CHANGED": 0, "REMOVED": 1, "NEW": 2, "RENAMED": 3, "IDENTICAL": 4}
    for verdict, dem, rest in sorted(rows, key=lambda r: (order[r[0]], r[1])):
        print(("%s %s %s" % (verdict, dem[:150], rest)).rstrip())
    return 1 if counts["changed"] or counts["new"] or counts["removed"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
