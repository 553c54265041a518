#!/usr/bin/env python3
"""Dump what the kernel generator emits over the whole matrix, for diffing two builds.

    tools/gen_dump_matrix.py <gen_dump binary> <output dir> [--default-only] [--serial]

Matrix: every energies/*.t and its UsePreconditioner("block") variant where the file
accepts one (the substitution of tests/test_block_preconditioner_frontend.py), each in
{float, double} x {off32 off, on}, under the default knobs and each OPT_AMD_GEN_* setting
below alone. `diff -r` of two output directories compares two builds of the generator.
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = [("default", {})] + [
    ("%s=%s" % (k, v), {"OPT_AMD_GEN_" + k: v})
    for k, v in [("STRIP32", "0"), ("STRIP32", "1"), ("STRIP32", "2"), ("WIDU", "0"), ("WIDU", "1"), ("FACTOR", "0"),
                 ("PRED", "0"), ("GRAPH_CACHE", "0"), ("NB_PREFETCH", "0"), ("EDGE_UNROLL", "1"), ("SAMPLE_CACHE", "0")]]


def block_variant(text):
    if "UsePreconditioner(true)" in text:
        text = text.replace("UsePreconditioner(true)", 'UsePreconditioner("block")')
    elif "UsePreconditioner" not in text:
        text = text.replace("Exclude(", 'UsePreconditioner("block")\nExclude(', 1)
    return text if text.count('UsePreconditioner("block")') == 1 else None


def main():
    tool, out = sys.argv[1], sys.argv[2]
    knobs = KNOBS[:1] if "--default-only" in sys.argv[3:] else KNOBS
    src = os.path.join(out, "_energies")
    os.makedirs(src, exist_ok=True)
    files = []
    for path in sorted(glob.glob(os.path.join(ROOT, "energies", "*.t"))):
        files.append(path)
        blk = block_variant(open(path).read())
        if blk is not None:
            files.append(os.path.join(src, os.path.basename(path)[:-2] + "_block.t"))
            open(files[-1], "w").write(blk)
    env0 = {k: v for k, v in os.environ.items() if not k.startswith("OPT_AMD_GEN_")}
    jobs = []
    for kname, kenv in knobs:
        os.makedirs(os.path.join(out, kname), exist_ok=True)
        for path in files:
            for flags in ([], ["--off32"], ["--double"], ["--double", "--off32"]):
                name = os.path.basename(path)[:-2] + "".join(f.replace("--", ".") for f in flags) + ".txt"
                jobs.append(([tool, path] + flags, dict(env0, **kenv), os.path.join(out, kname, name)))

    def run(job):
        cmd, env, dst = job
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0 or r.stderr:
            return "%s: exit %d\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode(errors="replace"))
        open(dst, "wb").write(r.stdout)
        return None

    serial = "--serial" in sys.argv[3:]   # one process at a time: for timing the generator
    with ThreadPoolExecutor(1 if serial else min(16, os.cpu_count() or 1)) as pool:
        bad = [e for e in pool.map(run, jobs) if e]
    for e in bad:
        sys.stderr.write(e + "\n")
    print("%d energy files, %d dumps, %d failed" % (len(files), len(jobs), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
