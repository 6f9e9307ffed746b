#!/usr/bin/env python3
"""Per-kernel resource table from the compiler's own remarks (no GPU).

Compiles the HIP sources with the flags of dpo_amd/ops/build.py plus
-Rpass-analysis=kernel-resource-usage into a temporary directory and
writes one CSV row per kernel, sorted by name:

    python scripts/kernel_resources.py OUT.csv [SRC_DIR]

SRC_DIR defaults to dpo_amd/ops/hip; point it at another checkout's
directory to tabulate that revision (e.g. before/after a refactor).
"""
import csv
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpo_amd.ops.build import ARCH, HIP_DIR, SOURCES  # noqa: E402

FIELDS = [("name", "Function Name"), ("vgprs", "VGPRs"), ("agprs", "AGPRs"),
          ("sgprs", "TotalSGPRs"), ("scratch_bytes_per_lane", "ScratchSize"),
          ("occupancy_waves_per_simd", "Occupancy"), ("lds_bytes", "LDS Size")]
REMARK = re.compile(r"remark: (?:\S+:\d+:\d+: )?\s*([A-Za-z ]+?)"
                    r"(?: \[[^\]]*\])?: "
                    r"(\S+) \[-Rpass-analysis=kernel-resource-usage\]")


def main():
    out_csv = sys.argv[1]
    src_dir = sys.argv[2] if len(sys.argv) > 2 else HIP_DIR
    hipcc = os.environ.get("HIPCC", "hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-shared",
               "-fPIC", "-Rpass-analysis=kernel-resource-usage",
               "-o", os.path.join(tmp, "out.so")]
        cmd += [os.path.join(src_dir, s) for s in SOURCES]
        log = subprocess.run(cmd, check=True, stderr=subprocess.PIPE,
                             text=True).stderr
    want = {label: key for key, label in FIELDS}
    rows = []
    for label, value in REMARK.findall(log):
        if label == "Function Name":
            rows.append({})
        if label in want and rows:
            rows[-1][want[label]] = value
    names = subprocess.run(["c++filt"], capture_output=True, text=True,
                           input="\n".join(r["name"] for r in rows),
                           check=True).stdout
    for row, name in zip(rows, names.splitlines()):
        row["name"] = name
    rows.sort(key=lambda r: r["name"])
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, [k for k, _ in FIELDS])
        w.writeheader()
        w.writerows(rows)
    print(f"{len(rows)} kernels -> {out_csv}")


if __name__ == "__main__":
    main()
