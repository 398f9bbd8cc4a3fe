#!/usr/bin/env python3
"""Registers, scratch and occupancy of every kernel of the given HIP sources.

Compiles each file's device code with the library's own flags (ar_slam_amd/build.py
hip_flags) plus -Rpass-analysis=kernel-resource-usage and prints one line per kernel, in the
layout of profiles/*/resource_usage.txt.  No GPU needed.

    python tools/resource_table.py lm_linearize.hip lm_step.hip debug_rows.hip
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ar_slam_amd import build as B   # noqa: E402

FIELDS = [("VGPR", r" VGPRs: (\d+)"), ("SGPR", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"),
          ("sspill", r"SGPRs Spill: (\d+)")]


def table(src):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [B.hipcc()] + B.hip_flags(ROOT, "resource-table") + \
            ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(B.CSRC, src),
             "-o", os.path.join(tmp, "dev.o")]
        out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode:
        raise SystemExit(out.stderr)
    rows, cur = [], None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = name.replace("arslam::(anonymous namespace)::", "")
            name = re.sub(r"^void ", "", name).split("(")[0]
            cur = {"name": name}
            rows.append(cur)
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def main():
    srcs = sys.argv[1:] or ["lm_linearize.hip", "lm_step.hip", "debug_rows.hip", "localize.hip"]
    bad = 0
    for src in srcs:
        print(f"== {src}")
        for r in sorted(table(src), key=lambda r: r["name"]):
            print(f"{r['name']:44s} VGPR {r['VGPR']:4d} SGPR {r['SGPR']:4d} scratch {r['scratch']:3d} "
                  f"occ {r['occ']} vspill {r['vspill']} sspill {r.get('sspill', 0)}")
            bad += r["scratch"] > 0
    print(f"kernels with scratch: {bad}")


if __name__ == "__main__":
    main()
