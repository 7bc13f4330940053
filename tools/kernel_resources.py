#!/usr/bin/env python3
"""Registers, scratch, occupancy and LDS of every kernel of one .hip file, from the compiler's own resource remarks.

  tools/kernel_resources.py schwarz-lib_amd/csrc/spmv_stream.hip [--filter stream_kernel] [--json out.json]

The file is compiled device-only with the Makefile's flags (`make hipflags`) plus
-Rpass-analysis=kernel-resource-usage; nothing is linked, nothing runs.  Headers named with quotes come from the
file's own directory first, so a file of another checkout is measured with that checkout's headers.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "schwarz-lib_amd")
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def kernel_resources(path, pattern=""):
    """{demangled kernel name without its parameter list: {vgprs, sgprs, agprs, scratch, occupancy, lds}}"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = subprocess.run(["make", "-s", "-C", LIB, "hipflags"], check=True, capture_output=True, text=True).stdout.split()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.abspath(path),
               "-o", os.path.join(tmp, "device.out")]
        run = subprocess.run(cmd, capture_output=True, text=True)
    if run.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), run.stderr[-4000:]))
    mangled, table = [], []
    for line in run.stderr.splitlines():
        m = re.search(r"remark: +([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            mangled.append(m.group(2))
            table.append({})
        elif m.group(1) in FIELDS and table:
            table[-1][FIELDS[m.group(1)]] = int(m.group(2))
    filt = os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "llvm-cxxfilt")
    names = subprocess.run([filt if os.path.exists(filt) else "c++filt", *mangled], check=True, capture_output=True,
                           text=True).stdout.splitlines() if mangled else []
    out = {}
    for name, row in zip(names, table):
        name = re.sub(r"^void ", "", name)
        name = name[:name.rindex(">") + 1] if ">(" in name else name.split("(")[0]
        if pattern in name:
            out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("hip_file")
    ap.add_argument("--filter", default="", help="only kernels whose name contains this")
    ap.add_argument("--json", help="write the table to this file as well")
    args = ap.parse_args()
    table = kernel_resources(args.hip_file, args.filter)
    print("%-64s %5s %5s %7s %4s %6s" % ("kernel", "VGPR", "SGPR", "scratch", "occ", "LDS"))
    for name, r in table.items():
        print("%-64s %5d %5d %7d %4d %6d" % (name, r["vgprs"] + r["agprs"], r["sgprs"], r["scratch"], r["occupancy"], r["lds"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
