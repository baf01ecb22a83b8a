#!/usr/bin/env python
"""Did a refactor keep the machine code?  Compiles one csrc/ file to gfx950 ISA (no GPU needed) from the working tree and from a git
revision, with the file's flags from unimedvl_amd/build.py, and prints per kernel: VGPRs / occupancy / scratch on both sides and whether
the instruction streams are identical (comments, .loc / .file / .cfi lines dropped, basic-block labels renumbered).

usage: python tools/isa_diff.py attention_prefill.hip [--rev HEAD] [--must-match REGEX]     exit 1 when a --must-match kernel differs
       --renamed OLD=NEW (repeatable): a kernel whose symbol changed - one that became a template instantiation, say - is compared
       under its two names (each a regex that matches exactly one symbol of its side) and must be identical"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimedvl_amd import build as product  # noqa: E402


def kernels(root, src, out):
    """{symbol: (normalised instruction lines, 'vgprs/occupancy/scratch')} of every kernel of root/unimedvl_amd/csrc/<src>"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + product.FLAGS + product.FILE_FLAGS.get(src, []) +
                          ["-S", "--cuda-device-only", "-o", out, os.path.join(root, "unimedvl_amd", "csrc", src)])
    s = open(out).read()
    res = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, re.M):
        b = s.index("\n" + name + ":")
        e = s.index(".Lfunc_end", b)
        labels, lines = {}, []
        for ln in s[b:e].split("\n")[2:]:
            ln = ln.split(";")[0].strip()
            if ln and not re.match(r"\.(loc|file|cfi)", ln):
                lines.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln))
        res[name] = (lines, "/".join(re.compile(r"; %s: (\d+)" % k).search(s, e).group(1) for k in ("NumVgprs", "Occupancy", "ScratchSize")))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", help="file name under unimedvl_amd/csrc/")
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--must-match", default=None, help="regex over kernel symbols whose instruction streams must be identical")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW", help="compare a kernel of the revision with a differently named one of the tree")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call("git archive %s unimedvl_amd/csrc include | tar -x -C %s" % (a.rev, tmp), shell=True, cwd=ROOT)
        old, new = kernels(tmp, a.source, os.path.join(tmp, "old.s")), kernels(ROOT, a.source, os.path.join(tmp, "new.s"))
    bad = 0
    print("%-9s %-14s %-14s %s" % ("stream", a.rev + " v/o/s", "tree v/o/s", "kernel"))
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "removed" if name in old else "added"
        else:
            verdict = "identical" if old[name][0] == new[name][0] else "differs"
        must = a.must_match is not None and re.search(a.must_match, name) is not None
        bad += must and verdict != "identical"
        print("%-9s %-14s %-14s %s%s" % (verdict, old.get(name, (0, "-"))[1], new.get(name, (0, "-"))[1], name, "  (must match)" if must else ""))
    for pair in a.renamed:
        sides = []
        for rx, side in zip(pair.split("=", 1), (old, new)):
            hit = [n for n in side if re.search(rx, n)]
            if len(hit) != 1:
                sys.exit("--renamed %s: %r matches %d kernels" % (pair, rx, len(hit)))
            sides.append((hit[0], [ln.replace(hit[0], "<kernel>") for ln in side[hit[0]][0] if not re.match(r"\.(text|section)\b", ln)], side[hit[0]][1]))
        same = sides[0][1] == sides[1][1]
        bad += not same
        print("%-9s %-14s %-14s %s -> %s  (renamed, must match)" % ("identical" if same else "differs", sides[0][2], sides[1][2], sides[0][0], sides[1][0]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
