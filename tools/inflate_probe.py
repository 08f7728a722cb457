#!/usr/bin/env python3
"""--device-inflate against gzread, file to file, on the bench's FASTQ as plain text and as BGZF (tools/bgzf_probe.py's
layout; the .gz is made with the driver's `bgzf-dump` tap):

    python tools/inflate_probe.py [--reads N] [--runs R] [--other-exe PATH] [--kernel-trace] [--out profiles/inflate_probe.json]
    python tools/inflate_probe.py --table-from profiles/inflate_probe.json    # only rewrite DESIGN.md's table from a result

Every run is a fresh process of the driver (-m 1024 -n 16 --jsonl -v, KASA_HOST_TIMING=1).  Legs, taking turns:
    other-plain, other-gz      --other-exe (the driver of the parent commit) on the plain file and on the .gz
    gz                         this driver on the .gz without a flag (gzread; the new code is not reached)
    gz-device-parse            this driver on the .gz with --device-parse (gzread, text up, parsed on the device)
    gz-device-inflate          this driver on the .gz with --device-inflate (compressed bytes up, inflated and parsed there)
Per leg: "Time file" of every run, min / median / max, and the medians of the host breakdown (`read`, `upload-text`,
`inflate`, `device-parse`, ...); the plain and the compressed size.  --kernel-trace: one more gz-device-inflate run under
`rocprofv3 --kernel-trace --stats`, in a run of its own, for inflate_kernel's total and its GB/s of text.
The result goes to --out and, as a table, between the two `inflate_probe` marker lines of DESIGN.md section 8f (--design).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kasa_amd import build, formats, synth
from device_parse_probe import TIMING, write_fastq

BEGIN, END = "<!-- inflate_probe: table begin (tools/inflate_probe.py writes it) -->", "<!-- inflate_probe: table end -->"
LEGS = [("other-plain", "parent commit's driver, plain file"), ("other-gz", "parent commit's driver, `.gz`"), ("gz", "this driver, `.gz`"),
        ("gz-device-parse", "this driver, `.gz`, `--device-parse`"), ("gz-device-inflate", "this driver, `.gz`, `--device-inflate`")]
HOST = ("read", "cut", "parse", "upload-text", "inflate", "device-parse")


def run_once(exe, d, infile, extra, wrap=None):
    for name in ("out.jsonl", "prof.csv"):
        try:
            os.unlink(os.path.join(d, name))
        except OSError:
            pass
    cmd = [exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, infile),
           "-q", os.path.join(d, "out.jsonl"), "-p", os.path.join(d, "prof.csv"), "--jsonl", "-v", "-m", "1024", "-n", "16"] + extra
    r = subprocess.run((wrap or []) + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=dict(os.environ, KASA_HOST_TIMING="1"))
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("OUT: Time file:"):
            out["time_file_s"] = float(line.split()[3])
        elif "host timing:" in line:
            out["host"] = {k.strip(" ,;()"): float(v) for k, v in TIMING.findall(line.split("host timing:")[1])}
        elif line.startswith("OUT: --device-parse") or line.startswith("OUT: --device-inflate"):
            out.setdefault("notes", []).append(line)
    return out


def table(res):
    if not res.get("legs"):
        return "not measured"
    rows = ["%d reads of %d bases, `--jsonl`, %d runs a leg, fresh processes taking turns; seconds, host entries are medians; plain file %d bytes, `.gz` %d bytes (%.3f):"
            % (res["reads"], res["read_length"], res["runs"], res["fastq_bytes"], res["gz_bytes"], res["gz_bytes"] / res["fastq_bytes"]), "",
            "| leg | Time file min / median / max | " + " | ".join("`%s`" % h for h in HOST) + " |", "|---|---|" + "---|" * len(HOST)]
    for leg, name in LEGS:
        if leg in res["legs"]:
            r = res["legs"][leg]
            cells = ["%.3f" % r["host_median_s"][h] if h in r["host_median_s"] else "-" for h in HOST]
            rows.append("| %s | %.3f / %.3f / %.3f | %s |" % (name, r["min_s"], r["median_s"], r["max_s"], " | ".join(cells)))
    for k, v in sorted(res.get("kernels", {}).items()):
        rows.append("")
        rows.append("`%s`: %d calls, %.1f ms in all, %.1f GB/s of text." % (k, v["calls"], v["total_ms"], v["text_gb_per_s"] or 0.0))
    return "\n".join(rows)


def write_table(res, design):
    text = open(design).read()
    if BEGIN not in text or END not in text:
        return False
    head, rest = text.split(BEGIN, 1)
    with open(design, "w") as f:
        f.write(head + BEGIN + "\n" + table(res) + "\n" + END + rest.split(END, 1)[1])
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--design", default=os.path.join(ROOT, "DESIGN.md"))
    ap.add_argument("--table-from", default=None)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--other-exe", default=None)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_probe.json"))
    a = ap.parse_args()
    if a.table_from:
        if not write_table(json.load(open(a.table_from)), a.design):
            sys.exit("no inflate_probe marker lines in " + a.design)
        return
    L = 150
    g = synth.genomes(1400, 300_000, seed=11)
    ix = synth.index_from_genomes(g)
    reads = synth.reads_from_genomes(g, a.reads, L, seed=1000)
    d = tempfile.mkdtemp(prefix="kasa_inf_", dir="/dev/shm")
    res = {"reads": a.reads, "read_length": L, "runs": a.runs, "legs": {}}
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        res["fastq_bytes"] = write_fastq(os.path.join(d, "reads.fastq"), reads, L)
        del ix, reads, g
        exe = build.build_host()
        subprocess.check_call([exe, "bgzf-dump", os.path.join(d, "reads.fastq"), os.path.join(d, "reads.fastq.gz")], stdout=subprocess.DEVNULL)
        res["gz_bytes"] = os.path.getsize(os.path.join(d, "reads.fastq.gz"))
        print("input made:", res["fastq_bytes"], "bytes of FASTQ,", res["gz_bytes"], "as BGZF", flush=True)
        legs = ([("other-plain", a.other_exe, "reads.fastq", []), ("other-gz", a.other_exe, "reads.fastq.gz", [])] if a.other_exe else []) + \
               [("gz", exe, "reads.fastq.gz", []), ("gz-device-parse", exe, "reads.fastq.gz", ["--device-parse"]), ("gz-device-inflate", exe, "reads.fastq.gz", ["--device-inflate"])]
        runs = {name: [] for name, *_ in legs}
        for i in range(a.runs):                                  # the legs take turns, so that drift hits all of them alike
            for name, e, infile, extra in legs:
                runs[name].append(run_once(e, d, infile, extra))
                print(name, i, runs[name][-1].get("time_file_s"), runs[name][-1].get("notes", ""), flush=True)
        for name, rs in runs.items():
            t = [r["time_file_s"] for r in rs]
            keys = sorted({k for r in rs for k in r.get("host", {})})
            res["legs"][name] = {"time_file_s": t, "median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "reads_per_s_median": a.reads / statistics.median(t),
                                 "host_median_s": {k: statistics.median([r["host"].get(k, 0.0) for r in rs]) for k in keys}, "notes": rs[0].get("notes", [])}
        if a.kernel_trace:                                       # counters and traces never share a run: this one traces kernels only
            td = tempfile.mkdtemp(prefix="kasa_inf_trace_")
            run_once(exe, d, "reads.fastq.gz", ["--device-inflate"], wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--"])
            kern = {}
            for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "kasa_inflate" in row.get("Name", ""):
                        ns = int(row["TotalDurationNs"])          # text_gb_per_s: the rate at which the kernel writes the plain text
                        kern[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": ns * 1e-6, "text_gb_per_s": res["fastq_bytes"] / ns if ns else None}
            res["kernels"] = kern
            shutil.rmtree(td, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not write_table(res, a.design):
        print("no inflate_probe marker lines in", a.design, "-- table not written", file=sys.stderr)


if __name__ == "__main__":
    main()
