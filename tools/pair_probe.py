#!/usr/bin/env python3
"""--device-pairs against the host path, file to file, on the bench's reads written as two FASTQ files of mates:

    python tools/pair_probe.py [--reads N] [--runs R] [--bgzf] [--other-exe PATH] [--kernel-trace] [--out profiles/pair_probe.json]

The bench's reads (tools/device_parse_probe.py's input) are split in two halves of equal count: read r of the first half is
mate 1 of pair r, read r of the second half its mate 2.  --bgzf writes both files as BGZF (the driver's bgzf-dump tap) and
adds --device-inflate to the device leg.  Every run is a fresh process of the driver (-m 1024 -n 16 --jsonl -v,
KASA_HOST_TIMING=1) under a `timeout` of its own; a run that fails ends the probe.  Legs: `other` (--other-exe: the driver
of the parent commit, host path), `host` (this driver without the flag) and `device` (--device-pairs).  Per leg: "Time
file", wall time and the child's peak resident set of every run, their medians, and the median KASA_HOST_TIMING split.
--kernel-trace: one more `device` run under `rocprofv3 --kernel-trace --stats` for pair_gather_kernel / pair_layout_kernel,
and one single-end --device-parse run on file 1 for the copy kernels behind kasa_parse_take (a device-to-device copy of the
same letters, half as many bytes): time, calls, bytes, GB/s.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from device_parse_probe import TIMING, write_fastq
from kasa_amd import build, formats, synth
from kasa_amd.reads import ReadBatch

STEP_LIMIT_S = 600
PEAK_OF_CHILD = "import resource, subprocess, sys; rc = subprocess.call(sys.argv[1:]); print('PEAK_RSS_KIB', resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss, flush=True); sys.exit(rc)"


def run_once(exe, d, inputs, extra, wrap=None):
    """One driver process under `timeout`; -> "Time file", wall seconds, peak resident set (KiB), host timing split, notes."""
    for name in ("out.jsonl", "prof.csv"):
        try:
            os.unlink(os.path.join(d, name))
        except OSError:
            pass
    cmd = [exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx")] + inputs + \
          ["-q", os.path.join(d, "out.jsonl"), "-p", os.path.join(d, "prof.csv"), "--jsonl", "-v", "-m", "1024", "-n", "16"] + extra
    log = os.path.join(d, "run.log")
    t0 = time.perf_counter()
    # The peak resident set is read by a small process of its own: a child forked by THIS process starts with this process's
    # peak (the reads and the index were made here), which is what wait4 would report for it.
    with open(log, "w") as f:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, "-c", PEAK_OF_CHILD] + (wrap or []) + cmd, stdout=f, stderr=subprocess.STDOUT,
                           env=dict(os.environ, KASA_HOST_TIMING="1"))
    wall = time.perf_counter() - t0
    text = open(log).read()
    if r.returncode != 0:
        raise RuntimeError("exit %d: %s" % (r.returncode, text[-2000:]))
    out = {"wall_s": wall}
    for line in text.splitlines():
        if line.startswith("PEAK_RSS_KIB "):
            out["peak_rss_kib"] = int(line.split()[1])
        elif line.startswith("OUT: Time file:"):
            out["time_file_s"] = float(line.split()[3])
        elif "host timing:" in line:
            out["host"] = {k.strip(" ,;()"): float(v) for k, v in TIMING.findall(line.split("host timing:")[1])}
        elif line.startswith(("OUT: --device-pairs", "OUT: --device-parse", "OUT: --device-inflate")):
            out.setdefault("notes", []).append(line)
    return out


def kernel_rows(td, wanted):
    rows = {}
    for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if any(w in name for w in wanted):
                rows[name.split("(")[0]] = {"calls": int(row["Calls"]), "total_ns": int(row["TotalDurationNs"])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000, help="reads of the bench; half as many pairs")
    ap.add_argument("--taxa", type=int, default=1400)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--bgzf", action="store_true")
    ap.add_argument("--other-exe", default=None)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_probe.json"))
    a = ap.parse_args()
    L, n = 150, a.reads // 2
    g = synth.genomes(a.taxa, 300_000, seed=11)
    ix = synth.index_from_genomes(g)
    reads = synth.reads_from_genomes(g, 2 * n, L, seed=1000)
    d = tempfile.mkdtemp(prefix="kasa_pair_", dir="/dev/shm")
    res = {"pairs": n, "read_length": L, "runs": a.runs, "bgzf": a.bgzf, "legs": {}}
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        exe = build.build_host()
        files = []
        for m in range(2):
            half = ReadBatch(reads.bases[m * n * L:(m + 1) * n * L], reads.offsets[:n + 1], None, reads.lengths[:n])
            path = os.path.join(d, "mates_%d.fastq" % (m + 1))
            res["fastq_bytes_each"] = write_fastq(path, half, L)
            if a.bgzf:
                subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), exe, "bgzf-dump", path, path + ".gz"], check=True, stdout=subprocess.DEVNULL)
                os.unlink(path)
                path += ".gz"
            files.append(path)
        del ix, reads, g
        pair_in = ["-1", files[0], "-2", files[1]]
        dev_flags = ["--device-pairs"] + (["--device-inflate"] if a.bgzf else [])
        legs = ([("other", a.other_exe, [])] if a.other_exe else []) + [("host", exe, []), ("device", exe, dev_flags)]
        runs = {name: [] for name, *_ in legs}
        for i in range(a.runs):                                  # the legs take turns, so that drift hits all of them alike
            for name, e, extra in legs:
                runs[name].append(run_once(e, d, pair_in, extra))
                print(name, i, runs[name][-1].get("time_file_s"), runs[name][-1]["peak_rss_kib"], flush=True)
        for name, rs in runs.items():
            t = [r["time_file_s"] for r in rs]
            keys = sorted({k for r in rs for k in r.get("host", {})})
            res["legs"][name] = {"time_file_s": t, "median_s": statistics.median(t), "wall_median_s": statistics.median([r["wall_s"] for r in rs]),
                                 "pairs_per_s_median": n / statistics.median(t), "peak_rss_kib_median": statistics.median([r["peak_rss_kib"] for r in rs]),
                                 "host_median_s": {k: statistics.median([r["host"].get(k, 0.0) for r in rs]) for k in keys},
                                 "notes": sorted({x for r in rs for x in r.get("notes", [])})}
        if a.kernel_trace:
            letters = 2 * n * L
            trace = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv"]
            td = tempfile.mkdtemp(prefix="kasa_pair_trace_")
            run_once(exe, d, pair_in, dev_flags, wrap=trace + ["-d", td, "--"])
            kern = kernel_rows(td, ("pair_gather_kernel", "pair_layout_kernel"))
            names = 2 * n * 10                                   # write_fastq's names: nine digits and the space, per mate
            for k, v in kern.items():
                if "gather" in k:                                # (its launches: the takes' letters and the fetches' names; every byte is read once and written once)
                    v["letters"] = letters; v["name_bytes"] = names; v["out_gb_per_s"] = (letters + names) / v["total_ns"] if v["total_ns"] else None
            shutil.rmtree(td, ignore_errors=True)
            td = tempfile.mkdtemp(prefix="kasa_pair_trace_")
            run_once(exe, d, ["-i", files[0]], ["--device-parse"] + (["--device-inflate"] if a.bgzf else []), wrap=trace + ["-d", td, "--"])
            for k, v in kernel_rows(td, ("copyBuffer", "CopyBuffer", "copy_buffer")).items():
                v["letters"] = letters // 2; v["letters_gb_per_s"] = (letters // 2) / v["total_ns"] if v["total_ns"] else None
                kern["kasa_parse_take (single-end, file 1): " + k] = v      # (every copy kernel of that run: an upper bound for the take's copy)
            shutil.rmtree(td, ignore_errors=True)
            res["kernels"] = kern
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
