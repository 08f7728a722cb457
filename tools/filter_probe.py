#!/usr/bin/env python3
"""--filter file to file on the bench's reads as one FASTQ: the host's filterReads against --device-filter.

    python tools/filter_probe.py [--reads N] [--runs R] [--modes plain,gzip] [--other-exe PATH] [--kernel-trace] [--out profiles/filter_probe.json]

Every run is a fresh process of the driver (--filter <clean> <contaminants> -m 1024 -n 16 --jsonl -v, no -q,
KASA_HOST_TIMING=1) under a `timeout` of its own; a run that fails ends the probe.  Legs, each plain and with --gzip:
`other` (--other-exe: the driver of the parent commit), `host` (this driver, --filter), `host-parser` (this driver,
--device-parse --filter: the flag that keeps the host parser) and `device` (--device-filter).  The legs take turns.  Per leg:
"Time file", wall time and the child's peak resident set of every run, min / median / max, the median KASA_HOST_TIMING
split, and the sizes of the two files.  --kernel-trace: one more `device` run (plain) under `rocprofv3 --kernel-trace
--stats` for the kernels the feature adds: time, calls, record bytes, GB/s written (the same bytes are read).  --markdown prints the table of
DESIGN.md section 8h from a result file.
"""
import argparse
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
from pair_probe import PEAK_OF_CHILD, STEP_LIMIT_S, kernel_rows
from kasa_amd import build, formats, synth

KERNELS = ("pair_gather_kernel", "flt_mark_kernel", "flt_list_kernel", "prs_gather_kernel", "prs_recsize_kernel", "prs_recindex_kernel", "prs_recoff_kernel")


def run_once(exe, d, infile, extra, wrap=None):
    for name in os.listdir(d):
        if name.startswith(("clean.", "cont.")) or name == "prof.csv":
            os.unlink(os.path.join(d, name))
    cmd = [exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", infile, "-p", os.path.join(d, "prof.csv"),
           "--filter", os.path.join(d, "clean"), os.path.join(d, "cont"), "--jsonl", "-v", "-m", "1024", "-n", "16"] + extra
    log = os.path.join(d, "run.log")
    t0 = time.perf_counter()
    with open(log, "w") as f:                                    # (the peak resident set is read by a small process of its own, as in pair_probe)
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, "-c", PEAK_OF_CHILD] + (wrap or []) + cmd, stdout=f, stderr=subprocess.STDOUT,
                           env=dict(os.environ, KASA_HOST_TIMING="1"))
    wall = time.perf_counter() - t0
    text = open(log).read()
    if r.returncode != 0:
        raise RuntimeError("exit %d: %s" % (r.returncode, text[-2000:]))
    out = {"wall_s": wall, "host": {}, "files": {n: os.path.getsize(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.startswith(("clean.", "cont."))}}
    for line in text.splitlines():
        if line.startswith("PEAK_RSS_KIB "):
            out["peak_rss_kib"] = int(line.split()[1])
        elif line.startswith("OUT: Time file:"):
            out["time_file_s"] = float(line.split()[3])
        elif "host timing:" in line:
            out["host"].update({k.strip(" ,;()"): float(v) for k, v in TIMING.findall(line.split("host timing:")[1])})
        elif line.startswith(("OUT: --device-filter", "OUT: --device-parse")):
            out.setdefault("notes", []).append(line)
    return out


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def markdown(res):
    rows = ["| leg | Time file s (min / median / max) | wall s | peak RSS MB | clean + contaminants bytes | filter split / fetch / write s |", "|---|---|---|---|---|---|"]
    for mode, legs in res["modes"].items():
        for name, leg in legs.items():
            t, h = leg["time_file_s"], leg["host_median_s"]
            rows.append("| %s, %s | %.2f / %.2f / %.2f | %.2f | %.0f | %s | %s |" % (
                name, mode, t["min"], t["median"], t["max"], leg["wall_s"]["median"], leg["peak_rss_kib"]["median"] / 1024, " + ".join(str(v) for v in leg["files"].values()),
                " / ".join("%.3f" % h[k] for k in ("filter split", "filter fetch", "filter write")) if "filter split" in h else "-"))
    for k, v in res.get("kernels", {}).items():
        rows.append("| `%s` | %d calls, %.3f ms%s | | | | |" % (k, v["calls"], v["total_ns"] / 1e6, ", %.0f GB/s written, as much read" % v["gb_per_s"] if v.get("gb_per_s") else ""))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--taxa", type=int, default=1400)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="plain,gzip")
    ap.add_argument("--other-exe", default=None)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--markdown", default=None, help="print the table of a result file and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_probe.json"))
    a = ap.parse_args()
    if a.markdown:
        print(markdown(json.load(open(a.markdown))))
        return
    L, n = 150, a.reads
    g = synth.genomes(a.taxa, 300_000, seed=11)
    ix = synth.index_from_genomes(g)
    reads = synth.reads_from_genomes(g, n, L, seed=1000)
    d = tempfile.mkdtemp(prefix="kasa_filter_", dir="/dev/shm")
    res = {"reads": n, "read_length": L, "runs": a.runs, "modes": {}}
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        exe = build.build_host()
        infile = os.path.join(d, "reads.fastq")
        write_fastq(infile, reads, L)
        res["fastq_bytes"] = os.path.getsize(infile)
        del ix, reads, g
        legs = ([("other", a.other_exe, [])] if a.other_exe else []) + [("host", exe, []), ("host-parser", exe, ["--device-parse"]), ("device", exe, ["--device-filter"])]
        for mode in a.modes.split(","):
            gz = ["--gzip"] if mode == "gzip" else []
            runs = {name: [] for name, *_ in legs}
            for i in range(a.runs):                              # the legs take turns, so that drift hits all of them alike
                for name, e, extra in legs:
                    runs[name].append(run_once(e, d, infile, extra + gz))
                    print(mode, name, i, runs[name][-1].get("time_file_s"), runs[name][-1]["peak_rss_kib"], runs[name][-1]["files"], flush=True)
            res["modes"][mode] = {}
            for name, rs in runs.items():
                keys = sorted({k for r in rs for k in r["host"]})
                res["modes"][mode][name] = {"time_file_s": spread([r["time_file_s"] for r in rs]), "wall_s": spread([r["wall_s"] for r in rs]),
                                            "peak_rss_kib": spread([r["peak_rss_kib"] for r in rs]), "files": rs[-1]["files"],
                                            "host_median_s": {k: statistics.median([r["host"].get(k, 0.0) for r in rs]) for k in keys},
                                            "notes": sorted({x for r in rs for x in r.get("notes", [])})}
        if a.kernel_trace:
            td = tempfile.mkdtemp(prefix="kasa_filter_trace_")
            r = run_once(exe, d, infile, ["--device-filter"], wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--"])
            records = sum(r["files"].values())                   # plain files: every record byte is in one of them
            kern = kernel_rows(td, KERNELS)
            for k, v in kern.items():
                if "gather" in k and ("FilterOffsets" in k or "<2>" in k or "GATHER_RECORDS" in k):   # the split's copy; the pool's record flavour: each reads and writes every record byte once
                    v["record_bytes"] = records; v["gb_per_s"] = records / v["total_ns"] if v["total_ns"] else None
            res["kernels"] = kern
            shutil.rmtree(td, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print(markdown(res))


if __name__ == "__main__":
    main()
