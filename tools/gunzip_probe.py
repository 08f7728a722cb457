#!/usr/bin/env python3
"""--device-gunzip against gzread, file to file, on the bench's FASTQ as ONE gzip member of level 6 (what gzip writes) and, for
scale, as BGZF with --device-inflate (tools/inflate_probe.py's layout):

    python tools/gunzip_probe.py [--reads N] [--runs R] [--kernel-trace] [--sweep] [--out profiles/gunzip_probe.json]
    python tools/gunzip_probe.py --table-from profiles/gunzip_probe.json    # only rewrite DESIGN.md's table from a result

Every run is a fresh process of the driver (-m 1024 -n 16 --jsonl -v, KASA_HOST_TIMING=1).  Legs, taking turns:
    gz                   this driver on the .gz without a flag: gzread on the reader thread -- what the user has today, and the
                         code of the parent commit (the new code is not reached)
    gz-device-gunzip     this driver on the .gz with --device-gunzip (compressed bytes up, chunks, chain, windows, parsed there)
    bgzf-device-inflate  this driver on the BGZF form with --device-inflate
Per leg: "Time file" of every run, min / median / max, the medians of the host breakdown, and the -v line with the chunk
statistics.  --sweep: one more gz-device-gunzip run per chunk size (KASA_GUNZIP_CHUNK) from 16 KiB to 512 KiB, from which the
default is chosen.  --kernel-trace: one more gz-device-gunzip run under `rocprofv3 --kernel-trace --stats`, in a run of its
own, for every kasa_gunzip kernel's total, its GB/s of compressed bytes and of text, and the chain's share.
The result goes to --out and, as a table, between the two `gunzip_probe` marker lines of DESIGN.md section 8n (--design).
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
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kasa_amd import build, formats, synth
from device_parse_probe import TIMING, write_fastq

BEGIN, END = "<!-- gunzip_probe: table begin (tools/gunzip_probe.py writes it) -->", "<!-- gunzip_probe: table end -->"
LEGS = [("gz", "`.gz`, no flag (`gzread`)"), ("gz-device-gunzip", "`.gz`, `--device-gunzip`"), ("bgzf-device-inflate", "BGZF, `--device-inflate`")]
HOST = ("read", "cut", "parse", "upload-text", "inflate", "device-parse")
SWEEP = (16384, 32768, 65536, 131072, 262144, 524288)


def run_once(exe, d, infile, extra, wrap=None, env=None):
    for name in ("out.jsonl", "prof.csv"):
        try:
            os.unlink(os.path.join(d, name))
        except OSError:
            pass
    cmd = [exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", os.path.join(d, infile),
           "-q", os.path.join(d, "out.jsonl"), "-p", os.path.join(d, "prof.csv"), "--jsonl", "-v", "-m", "1024", "-n", "16"] + extra
    r = subprocess.run((wrap or []) + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=dict(os.environ, KASA_HOST_TIMING="1", **(env or {})))
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("OUT: Time file:"):
            out["time_file_s"] = float(line.split()[3])
        elif "host timing:" in line:
            out["host"] = {k.strip(" ,;()"): float(v) for k, v in TIMING.findall(line.split("host timing:")[1])}
        elif line.startswith("OUT: --device-parse") or line.startswith("OUT: --device-inflate") or line.startswith("OUT: --device-gunzip"):
            out.setdefault("notes", []).append(line)
    return out


def gzip_one_member(src, dst, level=6):
    z = zlib.compressobj(level, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(dst, "wb") as o:
        while True:
            b = f.read(8 << 20)
            if not b:
                break
            o.write(z.compress(b))
        o.write(z.flush())
    return os.path.getsize(dst)


def table(res):
    if not res.get("legs"):
        return "not measured"
    rows = ["%d reads of %d bases, `--jsonl`, %d runs a leg, fresh processes taking turns; seconds, host entries are medians; plain file %d bytes, `.gz` (one member, level 6) %d bytes (%.3f), BGZF %d bytes:"
            % (res["reads"], res["read_length"], res["runs"], res["fastq_bytes"], res["gz_bytes"], res["gz_bytes"] / res["fastq_bytes"], res["bgzf_bytes"]), "",
            "| leg | Time file min / median / max | " + " | ".join("`%s`" % h for h in HOST) + " |", "|---|---|" + "---|" * len(HOST)]
    for leg, name in LEGS:
        if leg in res["legs"]:
            r = res["legs"][leg]
            cells = ["%.3f" % r["host_median_s"][h] if h in r["host_median_s"] else "-" for h in HOST]
            rows.append("| %s | %.3f / %.3f / %.3f | %s |" % (name, r["min_s"], r["median_s"], r["max_s"], " | ".join(cells)))
    for note in res["legs"].get("gz-device-gunzip", {}).get("notes", []):
        if "chunks" in note:
            rows += ["", "`" + note[5:] + "`"]
    if res.get("sweep"):
        rows += ["", "| `KASA_GUNZIP_CHUNK` | Time file | `inflate` |", "|---|---|---|"]
        rows += ["| %d | %.3f | %.3f |" % (int(k), v["time_file_s"], v.get("host", {}).get("inflate", 0.0)) for k, v in sorted(res["sweep"].items(), key=lambda kv: int(kv[0]))]
    if res.get("kernels"):
        total = sum(v["total_ms"] for v in res["kernels"].values())
        rows += ["", "| kernel | calls | ms | share | GB/s compressed | GB/s text |", "|---|---|---|---|---|---|"]
        for k, v in sorted(res["kernels"].items(), key=lambda kv: -kv[1]["total_ms"]):
            rows.append("| `%s` | %d | %.1f | %.0f %% | %.2f | %.2f |" % (k, v["calls"], v["total_ms"], 100.0 * v["total_ms"] / total, v["compressed_gb_per_s"], v["text_gb_per_s"]))
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
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_probe.json"))
    a = ap.parse_args()
    if a.table_from:
        if not write_table(json.load(open(a.table_from)), a.design):
            sys.exit("no gunzip_probe marker lines in " + a.design)
        return
    L = 150
    g = synth.genomes(1400, 300_000, seed=11)
    ix = synth.index_from_genomes(g)
    reads = synth.reads_from_genomes(g, a.reads, L, seed=1000)
    d = tempfile.mkdtemp(prefix="kasa_gun_", dir="/dev/shm")
    res = {"reads": a.reads, "read_length": L, "runs": a.runs, "legs": {}}
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        res["fastq_bytes"] = write_fastq(os.path.join(d, "reads.fastq"), reads, L)
        del ix, reads, g
        exe = build.build_host()
        res["gz_bytes"] = gzip_one_member(os.path.join(d, "reads.fastq"), os.path.join(d, "reads.fastq.gz"))
        subprocess.check_call([exe, "bgzf-dump", os.path.join(d, "reads.fastq"), os.path.join(d, "reads.bgzf.gz")], stdout=subprocess.DEVNULL)
        res["bgzf_bytes"] = os.path.getsize(os.path.join(d, "reads.bgzf.gz"))
        print("input made:", res["fastq_bytes"], "bytes of FASTQ,", res["gz_bytes"], "as gzip,", res["bgzf_bytes"], "as BGZF", flush=True)
        legs = [("gz", "reads.fastq.gz", []), ("gz-device-gunzip", "reads.fastq.gz", ["--device-gunzip"]), ("bgzf-device-inflate", "reads.bgzf.gz", ["--device-inflate"])]
        runs = {name: [] for name, *_ in legs}
        for i in range(a.runs):                                  # the legs take turns, so that drift hits all of them alike
            for name, infile, extra in legs:
                runs[name].append(run_once(exe, d, infile, extra))
                print(name, i, runs[name][-1].get("time_file_s"), runs[name][-1].get("notes", ""), flush=True)
        for name, rs in runs.items():
            t = [r["time_file_s"] for r in rs]
            keys = sorted({k for r in rs for k in r.get("host", {})})
            res["legs"][name] = {"time_file_s": t, "median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "reads_per_s_median": a.reads / statistics.median(t),
                                 "host_median_s": {k: statistics.median([r["host"].get(k, 0.0) for r in rs]) for k in keys}, "notes": rs[0].get("notes", [])}
        if a.sweep:
            res["sweep"] = {}
            for c in SWEEP:
                res["sweep"][str(c)] = run_once(exe, d, "reads.fastq.gz", ["--device-gunzip"], env={"KASA_GUNZIP_CHUNK": str(c)})
                print("chunk", c, res["sweep"][str(c)].get("time_file_s"), res["sweep"][str(c)].get("notes", ""), flush=True)
        if a.kernel_trace:                                       # counters and traces never share a run: this one traces kernels only
            td = tempfile.mkdtemp(prefix="kasa_gun_trace_")
            run_once(exe, d, "reads.fastq.gz", ["--device-gunzip"], wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--"])
            kern = {}
            for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "kasa_gunzip" in row.get("Name", ""):
                        ns = int(row["TotalDurationNs"])
                        kern[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": ns * 1e-6, "compressed_gb_per_s": res["gz_bytes"] / ns if ns else 0.0,
                                                           "text_gb_per_s": res["fastq_bytes"] / ns if ns else 0.0}
            res["kernels"] = kern
            shutil.rmtree(td, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not write_table(res, a.design):
        print("no gunzip_probe marker lines in", a.design, "-- table not written", file=sys.stderr)


if __name__ == "__main__":
    main()
