#!/usr/bin/env python3
"""Launch timeline of the z-sweep walk kernels: where a walk launch spends the time that does not depend on its bytes.

Needs a measurement build of spmv_pair.hip (make -C schwarz-lib_amd variant NAME=stamp DEFS=-DSCHWZ_WITH_PROBES),
selected with SCHWZ_HIP_LIB: there lane 0 of every walk workgroup stores the 100 MHz wall clock at seven points of
its life (kernel entry, segment and chain rows known, first windows requested -- landed with
-DSCHWZ_WALK_STAMP_WAIT=1 --, tables and fold done, end of the first step, end of the last step, after the final
reduction).  This tool runs a few solves of the default configuration of bench.py (256^3, one subdomain, 10 CG
iterations per solve) and prints, for each of the four walk forms, the medians over the launches of

  entry spread     last workgroup entry - first workgroup entry of a launch
  prologue stages  per workgroup, median over the workgroups of a launch
  steady step      (end of last step - end of first step) / (positions - 1)
  drain            end of last step -> partial sums written
  exit spread      last exit - median exit, and how much of a workgroup's lateness repeats from launch to launch
  dispatch rounds  per round of workgroups on a CU (block index // CUs): median prologue, steady step, positions and exit
  gap              last exit of the launch before -> first entry of this one (kernel end + dispatch of the next)

  python3 tools/walk_timeline.py [--solves 3] [--size 256] [--trace DIR]

--trace DIR: a rocprofv3 --kernel-trace output directory of a SEPARATE run of the same workload (tools/walk_timeline.sh
makes both runs); the mean duration of each form's kernel is set against the first-entry-to-last-exit span of the
stamps: the difference is kernel begin -> first entry plus last exit -> kernel end."""
import argparse
import csv
import ctypes as C
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "schwarz-lib_amd"))

FORMS = {1: "update", 2: "start", 3: "fused direction", 4: "first direction"}
STAGES = ["entry -> segment and chain rows", "-> windows %s", "-> tables and fold", "-> end of first step"]
TICK_US = 0.01  # wall_clock64 counts at 100 MHz


def trace_durations(d):
    """form -> mean kernel duration in us (steady state: last 60 % of the trace)"""
    f = glob.glob(d + "/**/*_kernel_trace.csv", recursive=True)
    if not f:
        return {}
    rows = list(csv.DictReader(open(f[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[int(len(rows) * 0.4):]
    acc = {k: [] for k in FORMS}
    for r in rows:
        n = r["Kernel_Name"]
        args = n[n.find("<") + 1:].split(",")
        if "spmv_pair_dirdot_sweep_kernel<" in n:
            form = 4 if args[2].strip() in ("true", "1") else 3
        elif "spmv_pair_sweep_kernel<" in n:
            form = 2 if args[3].strip() in ("true", "1") else 1
        else:
            continue
        acc[form].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (float(np.mean(v)), float(np.min(v)), len(v)) for k, v in acc.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--no-stamps", action="store_true", help="run the solves only (the rocprofv3 leg)")
    ap.add_argument("--summarize-trace", default=None, metavar="DIR", help="print the per-form kernel durations of a kernel trace and leave")
    a = ap.parse_args()
    if a.summarize_trace:
        for form, t in sorted(trace_durations(a.summarize_trace).items()):
            print("  %-16s %7.2f us mean, %.2f min, %d launches" % (FORMS[form], t[0], t[1], t[2]))
        return 0
    import torch
    import schwz_amd as S
    import bench
    lib = S.capi.lib
    n = a.size
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    solver, _ = bench.make_solver(S, S.InProcessComm(1), (n, n, n), 10, 1e-30, 200, 0.0, 0)
    solver.begin_run()
    for _ in range(4):
        solver.step()
    torch.cuda.synchronize()
    if a.no_stamps:
        for _ in range(a.solves):
            solver.step()
        torch.cuda.synchronize()
        return 0
    if not hasattr(lib, "schwz_walk_probe_set"):
        sys.exit("walk_timeline: %s is no measurement build (make variant NAME=stamp DEFS=-DSCHWZ_WITH_PROBES)" % S.capi.LIB_PATH)
    words, recs = lib.schwz_walk_probe_record_words(), lib.schwz_walk_probe_launch_records()
    cap = 32 * a.solves
    buf = torch.zeros(cap * recs * words, dtype=torch.int64, device="cuda")
    lib.schwz_walk_probe_set.argtypes = [C.c_void_p, C.c_int]
    lib.schwz_walk_probe_set.restype = None
    torch.cuda.synchronize()
    lib.schwz_walk_probe_set(buf.data_ptr(), cap)
    for _ in range(a.solves):
        solver.step()
    torch.cuda.synchronize()
    used = lib.schwz_walk_probe_used()
    lib.schwz_walk_probe_set(None, 0)
    h = buf.cpu().numpy().reshape(cap, recs, words)[:used]
    trace = trace_durations(a.trace) if a.trace else {}
    landed = "landed" if "stampw" in os.path.basename(S.capi.LIB_PATH) else "requested"
    print("walk timeline: %s, %d^3, %d solves, %d walk launches stamped" % (os.path.basename(S.capi.LIB_PATH), n, a.solves, used))
    per_form = {k: [] for k in FORMS}
    prev_exit = None
    for l in range(used):
        r = h[l]
        r = r[r[:, 0] != 0]
        if not len(r):
            prev_exit = None
            continue
        form = int(r[0, 0] & 0xff)
        xcc = (r[:, 0] >> 40) & 0xf
        blk = (r[:, 0] >> 8) & 0xffffffff
        st = r[:, 2:].astype(np.float64) * TICK_US
        walked = r[:, 1] > 0   # workgroups with an empty segment stamp entry and exit only
        entry, done = st[:, 0], st[:, 6]
        w = st[walked]
        npos = r[walked, 1].astype(np.float64)
        m = dict(wgs=len(r), entry_spread=entry.max() - entry.min(), entry_med=np.median(entry) - entry.min(),
                 stages=[np.median(w[:, k + 1] - w[:, k]) for k in range(4)],
                 prologue=np.median(w[:, 4] - w[:, 0]),
                 step=np.median((w[:, 5] - w[:, 4])[npos > 1] / (npos[npos > 1] - 1)),
                 steps=np.median(npos), drain=np.median(w[:, 6] - w[:, 5]),
                 life=np.median(done - entry), exit_spread=done.max() - np.median(done),
                 span=done.max() - entry.min(), gap=(entry.min() - prev_exit) if prev_exit is not None else np.nan,
                 late=dict(zip(blk.tolist(), (done - np.median(done)).tolist())),
                 wg=dict(zip(blk[walked].tolist(), zip(npos.tolist(), ((w[:, 5] - w[:, 4]) / np.maximum(npos - 1, 1)).tolist(),
                                                       (w[:, 4] - w[:, 0]).tolist(), (w[:, 6] - entry.min()).tolist()))),
                 late_xcc=[float(np.mean((done - np.median(done))[xcc == x])) if (xcc == x).any() else np.nan for x in range(8)])
        per_form[form].append(m)
        prev_exit = done.max()
    for form, name in FORMS.items():
        ms = per_form[form]
        if not ms:
            continue
        med = lambda key: float(np.nanmedian([m[key] for m in ms]))
        print("\n%s walk: %d launches, %d workgroups, %.0f positions per segment (median)" % (name, len(ms), ms[0]["wgs"], med("steps")))
        print("  entry spread (last - first entry)        %7.2f us   (median entry - first %.2f)" % (med("entry_spread"), med("entry_med")))
        for k, s in enumerate(STAGES):
            print("  %-40s %7.2f us" % (s % landed if "%s" in s else s, float(np.median([m["stages"][k] for m in ms]))))
        print("  prologue in all (entry -> end of first step) %5.2f us" % med("prologue"))
        print("  steady step                              %7.2f us   x (positions - 1)" % med("step"))
        print("  drain (end of last step -> sums written) %7.2f us" % med("drain"))
        print("  workgroup life (median)                  %7.2f us" % med("life"))
        print("  exit spread (last - median exit)         %7.2f us" % med("exit_spread"))
        print("  first entry -> last exit                 %7.2f us" % med("span"))
        print("  last exit of the launch before -> first entry %5.2f us" % med("gap"))
        if form in trace:
            t = trace[form]
            print("  kernel duration (separate kernel trace)  %7.2f us mean, %.2f min, %d launches: begin -> first entry + last exit -> end = %.2f us"
                  % (t[0], t[1], t[2], t[0] - med("span")))
        # does a workgroup's lateness repeat?  variance of the per-workgroup mean lateness over the launches / total variance
        keys = sorted(set.intersection(*[set(m["late"]) for m in ms]))
        if len(ms) > 1 and keys:
            L = np.array([[m["late"][k] for k in keys] for m in ms])
            tot = L.var()
            rep = L.mean(axis=0).var()
            worst = np.argsort(L.mean(axis=0))[-5:][::-1]
            print("  lateness at exit that repeats per workgroup: %.0f %% of its variance; latest on average: %s"
                  % (100.0 * rep / tot if tot > 0 else 0.0, ", ".join("wg %d (+%.1f us)" % (keys[i], L.mean(axis=0)[i]) for i in worst)))
            # what sets the latest twentieth apart: more positions, slower steps or a longer prologue?
            order = np.argsort(L.mean(axis=0))
            late_keys = [keys[i] for i in order[-max(len(keys) // 20, 1):]]

            def mean_of(ks, j):
                return float(np.mean([m["wg"][k][j] for m in ms for k in ks if k in m["wg"]]))
            print("  the latest twentieth of the workgroups (indices %d ... %d, median %d) / all: positions %.1f / %.1f, steady step %.2f / %.2f us, prologue %.2f / %.2f us"
                  % (min(late_keys), max(late_keys), int(np.median(late_keys)), mean_of(late_keys, 0), mean_of(keys, 0),
                     mean_of(late_keys, 1), mean_of(keys, 1), mean_of(late_keys, 2), mean_of(keys, 2)))
        # by dispatch round: block b reads table entry b and is the (b // 8)-th workgroup of its XCD, so with `cus` CUs the
        # blocks [r cus, (r + 1) cus) are the r-th workgroup to arrive on their CU -- what the plan's trim acts on
        # (SCHWZ_SWEEP_TRIM, walk_segment_table): equal lives need prologue_r + positions_r x step_r equal over r
        all_keys = sorted(set().union(*[set(m["wg"]) for m in ms]))
        for rnd in range((max(all_keys) // cus + 1) if all_keys else 0):
            ks = [k for k in all_keys if k // cus == rnd]
            if not ks:
                continue

            def median_of(j):
                return float(np.median([m["wg"][k][j] for m in ms for k in ks if k in m["wg"]]))
            print("  dispatch round %d (indices %d ... %d): prologue %.2f us, steady step %.3f us, positions %.0f, exit %.2f us after the first entry (latest %.2f)"
                  % (rnd, min(ks), max(ks), median_of(2), median_of(1), median_of(0), median_of(3),
                     float(np.median([max(m["wg"][k][3] for k in ks if k in m["wg"]) for m in ms]))))
        print("  mean exit - median exit by XCC id: %s" % " ".join("%.1f" % float(np.nanmean([m["late_xcc"][x] for m in ms])) for x in range(8)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
