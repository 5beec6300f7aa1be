#!/usr/bin/env python3
"""What the compiler makes of the same translation units at two checkouts, kernel by kernel: each .hip file is compiled to gfx950
assembly at both (tools/isa_round_trips.py's command) and, per kernel instantiation, the table of profiles/*_shared_code_ab.txt is
printed — VGPRs (.amdhsa_next_free_vgpr: it counts the AGPRs of the unified file), SGPRs, scratch and LDS bytes, instructions in the
body, and every opcode whose count changed as (parent, branch).  The opcodes are whatever occurs in the bodies; the tool knows none.
    python tools/isa_ab.py PARENT_ROOT BRANCH_ROOT FILE.hip [FILE.hip ...] [--same REGEX] [--counts REGEX] [--text SUBSTRING] [--jobs N]
FILE is relative to both roots.  --same REGEX (repeatable): a class of opcodes whose counts must not move in any kernel, e.g.
'^(global_|ds_|buffer_)' or '_f64' (the two encodings of one opcode, _e32 and _e64, count together there); --counts REGEX (repeatable): kernels whose name matches must keep the count of EVERY opcode;
--text SUBSTRING (repeatable): kernels whose name contains it must be the same text line for line.
After the table: symbol sets, scratch / LDS gained, waves per SIMD (512 / the VGPR count rounded up to 8, at most 8), the classes and
the texts, each as ok or as the list of kernels that miss it.  Exit status 1 when one is missed."""
import argparse
import collections
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_round_trips import compile_to_asm

FIELDS = (("VGPR", "next_free_vgpr"), ("SGPR", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"), ("LDS", "group_segment_fixed_size"))


def kernels(asm_text):
    """{demangled kernel name: {"VGPR", "SGPR", "scratch", "LDS": int, "body": [instruction lines], "ops": Counter of opcodes}}"""
    out = {}
    blocks = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm_text, re.S)
    names = [n for n, _ in blocks]
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    for (n, desc), d in zip(blocks, demangled):
        i = asm_text.find("\n" + n + ":")
        j = asm_text.find("\n.Lfunc_end", i)
        body = [l.split(";")[0].strip() for l in asm_text[i:j].splitlines()[2:]]
        body = [l for l in body if l and not l.startswith(".") and not l.endswith(":")]
        k = {f: int(re.search(r"\.amdhsa_" + key + r" (\d+)", desc).group(1)) for f, key in FIELDS}
        k["body"] = body
        k["ops"] = collections.Counter(l.split()[0] for l in body)
        out[d.replace("mrl::(anonymous namespace)::", "").replace("void ", "").split("(")[0]] = k
    return out


def waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--same", action="append", default=[])
    ap.add_argument("--counts", action="append", default=[])
    ap.add_argument("--text", action="append", default=[])
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    with ThreadPoolExecutor(max_workers=a.jobs) as pool:
        asm = list(pool.map(lambda p: kernels(compile_to_asm(p)), [os.path.join(r, f) for f in a.files for r in (a.parent, a.branch)]))
    missed = collections.defaultdict(list)
    texts = {t: 0 for t in a.text}
    total = 0
    for n, f in enumerate(a.files):
        p, b = asm[2 * n], asm[2 * n + 1]
        print(f"== {f}: {len(p)} kernels at the parent, {len(b)} at the branch, symbol sets {'equal' if p.keys() == b.keys() else 'DIFFERENT'}")
        if p.keys() != b.keys():
            missed["symbol sets"].append(f"{f}: {sorted(p.keys() ^ b.keys())}")
        same = 0
        for name in sorted(p.keys() & b.keys()):
            kp, kb = p[name], b[name]
            changed = {op: (kp["ops"][op], kb["ops"][op]) for op in sorted(kp["ops"].keys() | kb["ops"].keys()) if kp["ops"][op] != kb["ops"][op]}
            same += not changed
            print(f"{name}: " + " ".join(f"{fl} {kp[fl]}->{kb[fl]}" for fl, _ in FIELDS) + f" instr {len(kp['body'])}->{len(kb['body'])} changed: {changed or 'none'}")
            if kb["scratch"] > kp["scratch"] or kb["LDS"] > kp["LDS"]:
                missed["no scratch or LDS gained"].append(name)
            if waves(kp["VGPR"]) != waves(kb["VGPR"]):
                missed["waves per SIMD"].append(f"{name}: {waves(kp['VGPR'])} -> {waves(kb['VGPR'])}")
            for rx in a.same:                                    # per opcode whatever its encoding: v_x_e32 and v_x_e64 are one opcode
                moved = collections.Counter()
                for op, (x, y) in changed.items():
                    if re.search(rx, op):
                        moved[re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)] += y - x
                if any(moved.values()):
                    missed[f"counts of {rx}"].append(name)
            for rx in a.counts:
                if changed and re.search(rx, name):
                    missed[f"every count of {rx}"].append(name)
            for t in a.text:
                if t in name:
                    texts[t] += 1
                    if kp["body"] != kb["body"]:
                        missed[f"text of {t}"].append(name)
        total += len(p.keys() & b.keys())
        print(f"-- {same} of {len(p.keys() & b.keys())} bodies identical in every opcode count")
    for t, hits in texts.items():
        if not hits:
            missed[f"text of {t}"].append("no kernel of that name")
    print(f"== conditions over {total} kernels")
    for cond in ["symbol sets", "no scratch or LDS gained", "waves per SIMD"] + [f"counts of {rx}" for rx in a.same] + [f"every count of {rx}" for rx in a.counts] + [f"text of {t}" for t in a.text]:
        print(f"{cond}: " + ("ok" if cond not in missed else "MISSED by " + "; ".join(missed[cond])))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
