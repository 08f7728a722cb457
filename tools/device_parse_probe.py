#!/usr/bin/env python3
"""--device-parse against the host parser, file to file, on the bench's FASTQ (tools/f2f_probe.py's input, made once):

    python tools/device_parse_probe.py [--reads N] [--runs R] [--other-exe PATH] [--out profiles/device_parse_probe.json]

Every run is a fresh process of the driver (-m 1024 -n 16 --jsonl -v, KASA_HOST_TIMING=1).  Legs: `other` (--other-exe: a
driver built from another commit, for the "nothing changed without the flag" comparison), `host` (this driver), `device`
(this driver with --device-parse: the text goes up straight from the reader's buffer) and `device_pinned`
(KASA_PARSE_STAGE=pinned: copied to a page-locked staging buffer first).  Per leg: "Time file" and reads/s of every run, their median, and the median host breakdown.
--kernel-trace: one more `device` run under `rocprofv3 --kernel-trace --stats` for the parser's kernels (time, bytes, GB/s).
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from kasa_amd import build, formats, synth

TIMING = re.compile(r"([a-z][a-z +-]*?) ([0-9][0-9.e+-]*) s")


def write_fastq(path, reads, L):
    rec = np.empty((reads.n, 2 * L + 15), dtype=np.uint8)
    rec[:, 0] = ord("@")
    ids = np.arange(reads.n, dtype=np.int64)
    for c in range(9):
        rec[:, 9 - c] = (ord("0") + (ids // 10 ** c) % 10).astype(np.uint8)
    rec[:, 10] = 10
    rec[:, 11:11 + L] = reads.bases.reshape(reads.n, L)
    rec[:, 11 + L:14 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 14 + L:14 + 2 * L] = ord("I")
    rec[:, 14 + 2 * L] = 10
    with open(path, "wb") as f:
        f.write(rec.tobytes())
    return rec.nbytes


def run_once(exe, d, extra, env_extra, wrap=None):
    for name in ("out.jsonl", "prof.csv"):
        try:
            os.unlink(os.path.join(d, name))
        except OSError:
            pass
    cmd = [exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, "reads.fastq"),
           "-q", os.path.join(d, "out.jsonl"), "-p", os.path.join(d, "prof.csv"), "--jsonl", "-v", "-m", "1024", "-n", "16"] + extra
    r = subprocess.run((wrap or []) + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=dict(os.environ, KASA_HOST_TIMING="1", **env_extra))
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("OUT: Time file:"):
            out["time_file_s"] = float(line.split()[3])
        elif "host timing:" in line:
            out["host"] = {k.strip(" ,;()"): float(v) for k, v in TIMING.findall(line.split("host timing:")[1])}
        elif line.startswith("OUT: --device-parse"):
            out.setdefault("notes", []).append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--other-exe", default=None)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_parse_probe.json"))
    a = ap.parse_args()
    L = 150
    g = synth.genomes(1400, 300_000, seed=11)
    ix = synth.index_from_genomes(g)
    reads = synth.reads_from_genomes(g, a.reads, L, seed=1000)
    d = tempfile.mkdtemp(prefix="kasa_dpp_", dir="/dev/shm")
    res = {"reads": a.reads, "read_length": L, "runs": a.runs, "legs": {}}
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        res["fastq_bytes"] = write_fastq(os.path.join(d, "reads.fastq"), reads, L)
        del ix, reads, g
        exe = build.build_host()
        legs = ([("other", a.other_exe, [], {})] if a.other_exe else []) + [("host", exe, [], {}), ("device", exe, ["--device-parse"], {}),
                                                                              ("device_pinned", exe, ["--device-parse"], {"KASA_PARSE_STAGE": "pinned"})]
        runs = {name: [] for name, *_ in legs}
        for i in range(a.runs):                                  # the legs take turns, so that drift hits all of them alike
            for name, e, extra, env in legs:
                runs[name].append(run_once(e, d, extra, env))
                print(name, i, runs[name][-1].get("time_file_s"), flush=True)
        for name, rs in runs.items():
            t = [r["time_file_s"] for r in rs]
            keys = sorted({k for r in rs for k in r.get("host", {})})
            res["legs"][name] = {"time_file_s": t, "median_s": statistics.median(t), "min_s": min(t), "max_s": max(t),
                                 "reads_per_s_median": a.reads / statistics.median(t),
                                 "host_median_s": {k: statistics.median([r["host"].get(k, 0.0) for r in rs]) for k in keys},
                                 "notes": sorted({n for r in rs for n in r.get("notes", [])})}
        if a.kernel_trace:
            td = tempfile.mkdtemp(prefix="kasa_dpp_trace_")
            run_once(exe, d, ["--device-parse"], {}, wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--"])
            kern = {}
            for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "prs_" in row.get("Name", ""):
                        ns = int(row["TotalDurationNs"])                  # text_gb_per_s: the rate at which the kernel gets through the file's text
                        kern[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ns": ns, "text_gb_per_s": res["fastq_bytes"] / ns if ns else None}
            res["kernels"] = kern
            shutil.rmtree(td, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
