#!/usr/bin/env python3
"""--bgzf against the plain per-read file, file to file, on the bench's FASTQ (tools/device_parse_probe.py's input):

    python tools/bgzf_probe.py [--reads N] [--runs R] [--other-exe PATH] [--kernel-trace] [--out profiles/bgzf_probe.json]
    python tools/bgzf_probe.py --table-from profiles/bgzf_probe.json      # only rewrite DESIGN.md's table from a result

Every run is a fresh process of the driver (-m 1024 -n 16 --jsonl -v, KASA_HOST_TIMING=1).  Legs, taking turns: `other`
(--other-exe: the driver of the parent commit, for "nothing changes without the flag"), `plain` (this driver), `bgzf`
(this driver with --bgzf) and `dynamic` (this driver with --bgzf-dynamic: a Huffman table per batch).  Per leg: "Time file" of every run, min / median / max, and the median host breakdown (`output
write`, `text fetch`, `text`, `deflate`, ...).  The sizes: plain bytes, compressed bytes, their ratio -- and what zlib level 1
makes of the same text block by block on the CPU with the fixed Huffman code (Z_FIXED: the gap to ours is the matcher's
cost) and with its own tables (what a Huffman table per batch would buy), on a sample of blocks spread over the file.
--kernel-trace: one more `bgzf` and one more `dynamic` run under `rocprofv3 --kernel-trace --stats` for the kernels of each
(total ms, GB/s of text; `dynamic`: the count pass, the table's build and the coded pass apart).
Only `kasa_bgzf::` kernels are counted there: the rocPRIM scan of the member sizes (4097 values per 256 MiB of text) and the
memset of as many bytes carry the names the other stages' scans and memsets carry, so the statistics cannot tell them apart;
the result says so in `kernels_left_out`.
The result goes to --out and, as a table, between the two `bgzf_probe` marker lines of DESIGN.md section 8e (--design).
"""
import argparse
import csv
import glob
import gzip
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kasa_amd import build, formats, synth
from device_parse_probe import run_once, write_fastq


def zlib_blockwise(path, sample_blocks):
    """bytes zlib level 1 makes of `sample_blocks` blocks of 65 280 bytes spread over the file (26 bytes of framing each):
    fixed Huffman code and default strategy, with the plain bytes they stand for"""
    size = os.path.getsize(path)
    n_blocks = (size + formats.BGZF_BLOCK - 1) // formats.BGZF_BLOCK
    step = max(1, n_blocks // sample_blocks)
    plain = fixed = dynamic = 0
    with open(path, "rb") as f:
        for b in range(0, n_blocks, step):
            f.seek(b * formats.BGZF_BLOCK)
            block = f.read(formats.BGZF_BLOCK)
            plain += len(block)
            for strategy in (zlib.Z_FIXED, zlib.Z_DEFAULT_STRATEGY):
                z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
                n = len(z.compress(block) + z.flush()) + 26
                if strategy == zlib.Z_FIXED:
                    fixed += n
                else:
                    dynamic += n
    return {"blocks_sampled": len(range(0, n_blocks, step)), "plain_bytes": plain, "zlib1_fixed_ratio": fixed / plain, "zlib1_dynamic_ratio": dynamic / plain}


def digest(f):
    h = hashlib.blake2b()
    for chunk in iter(lambda: f.read(1 << 24), b""):
        h.update(chunk)
    return h.hexdigest()


BEGIN, END = "<!-- bgzf_probe: table begin (tools/bgzf_probe.py writes it) -->", "<!-- bgzf_probe: table end -->"


def table(res):
    """the result as the markdown table of DESIGN.md section 8e"""
    names = {"other": "parent commit's driver", "plain": "this driver", "bgzf": "this driver, `--bgzf`", "dynamic": "this driver, `--bgzf-dynamic`"}
    host = ("output write", "text fetch", "text", "deflate")
    rows = ["%d reads of %d bases, `--jsonl`, %d runs a leg, fresh processes taking turns; seconds, host entries are medians:" % (res["reads"], res["read_length"], res["runs"]), "",
            "| leg | Time file min / median / max | " + " | ".join("`%s`" % h for h in host) + " | file bytes |", "|---|---|" + "---|" * (len(host) + 1)]
    for leg in ("other", "plain", "bgzf", "dynamic"):
        if leg in res["legs"]:
            r = res["legs"][leg]
            cells = ["%.3f" % r["host_median_s"][h] if h in r["host_median_s"] else "-" for h in host]
            rows.append("| %s | %.3f / %.3f / %.3f | %s | %d |" % (names[leg], r["min_s"], r["median_s"], r["max_s"], " | ".join(cells), r["file_bytes"]))
    z = res.get("zlib_on_the_cpu", {})
    rows += ["", "Ratio (compressed / plain bytes): %.3f on the device with the fixed code%s; zlib level 1 block by block on %s sampled blocks of the same text: %s with the fixed code, %s with its own tables." %
             (res["ratio"], ", %.3f with a table per batch (%.3f of the fixed code's file)" % (res["dynamic_ratio"], res["dynamic_bytes"] / res["bgzf_bytes"]) if "dynamic_ratio" in res else "",
              z.get("blocks_sampled", "no"), "%.3f" % z["zlib1_fixed_ratio"] if z else "-", "%.3f" % z["zlib1_dynamic_ratio"] if z else "-")]
    for key, flag in (("bgzf_file", "--bgzf"), ("dynamic_file", "--bgzf-dynamic")):
        if key in res:
            rows.append("The `%s` file decompresses to the plain file: %s; it ends with the EOF block: %s." % (flag, res[key]["decompresses_to_the_plain_file"], res[key]["ends_with_eof_block"]))
    for leg, flag in (("kernels", "--bgzf"), ("kernels_dynamic", "--bgzf-dynamic")):
        for k, v in sorted(res.get(leg, {}).items()):
            rows.append("`%s`, `%s`: %d calls, %.1f ms in all, %.1f GB/s of text." % (flag, k, v["calls"], v["total_ms"], v["text_gb_per_s"] or 0.0))
    if "kernels_left_out" in res:
        rows.append("Left out of the kernels' total: " + res["kernels_left_out"])
    return "\n".join(rows)


def write_table(res, design):
    """puts table(res) between DESIGN.md's marker lines; False when the file has none"""
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
    ap.add_argument("--sample-blocks", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_probe.json"))
    a = ap.parse_args()
    if a.table_from:
        if not write_table(json.load(open(a.table_from)), a.design):
            sys.exit("no bgzf_probe marker lines in " + a.design)
        return
    L = 150
    g = synth.genomes(1400, 300_000, seed=11)
    ix = synth.index_from_genomes(g)
    reads = synth.reads_from_genomes(g, a.reads, L, seed=1000)
    d = tempfile.mkdtemp(prefix="kasa_bgz_", dir="/dev/shm")
    res = {"reads": a.reads, "read_length": L, "runs": a.runs, "legs": {}}
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        res["fastq_bytes"] = write_fastq(os.path.join(d, "reads.fastq"), reads, L)
        del ix, reads, g
        print("input made:", res["fastq_bytes"], "bytes of FASTQ", flush=True)
        exe = build.build_host()
        legs = ([("other", a.other_exe, [])] if a.other_exe else []) + [("plain", exe, []), ("bgzf", exe, ["--bgzf"]), ("dynamic", exe, ["--bgzf-dynamic"])]
        runs = {name: [] for name, *_ in legs}
        out = os.path.join(d, "out.jsonl")
        for i in range(a.runs):                                  # the legs take turns, so that drift hits all of them alike
            for name, e, extra in legs:
                runs[name].append(run_once(e, d, extra, {}))
                runs[name][-1]["file_bytes"] = os.path.getsize(out)
                print(name, i, runs[name][-1].get("time_file_s"), runs[name][-1]["file_bytes"], flush=True)
                if name == "plain" and i == 0:
                    res["zlib_on_the_cpu"] = zlib_blockwise(out, a.sample_blocks)
                    with open(out, "rb") as f:
                        plain_digest = digest(f)
                if name in ("bgzf", "dynamic") and i == 0:       # the file rule, at full size: the same bytes, the EOF block at the end
                    with gzip.open(out, "rb") as z:
                        same = digest(z) == plain_digest
                    with open(out, "rb") as f:
                        f.seek(-28, os.SEEK_END)
                        res[name + "_file"] = {"decompresses_to_the_plain_file": same, "ends_with_eof_block": f.read() == formats.BGZF_EOF}
        for name, rs in runs.items():
            t = [r["time_file_s"] for r in rs]
            keys = sorted({k for r in rs for k in r.get("host", {})})
            res["legs"][name] = {"time_file_s": t, "median_s": statistics.median(t), "min_s": min(t), "max_s": max(t),
                                 "reads_per_s_median": a.reads / statistics.median(t), "file_bytes": rs[0]["file_bytes"],
                                 "host_median_s": {k: statistics.median([r["host"].get(k, 0.0) for r in rs]) for k in keys}}
        res["plain_bytes"] = res["legs"]["plain"]["file_bytes"]
        res["bgzf_bytes"] = res["legs"]["bgzf"]["file_bytes"]
        res["ratio"] = res["bgzf_bytes"] / res["plain_bytes"]
        res["dynamic_bytes"] = res["legs"]["dynamic"]["file_bytes"]
        res["dynamic_ratio"] = res["dynamic_bytes"] / res["plain_bytes"]
        for key, flag in (("kernels", "--bgzf"), ("kernels_dynamic", "--bgzf-dynamic")) if a.kernel_trace else ():
            td = tempfile.mkdtemp(prefix="kasa_bgz_trace_")
            run_once(exe, d, [flag], {}, wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--"])
            kern = {}
            for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "kasa_bgzf" in row.get("Name", ""):
                        ns = int(row["TotalDurationNs"])          # text_gb_per_s: the rate at which the kernel gets through the plain text
                        kern[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": ns * 1e-6, "text_gb_per_s": res["plain_bytes"] / ns if ns else None}
            res[key] = kern
            shutil.rmtree(td, ignore_errors=True)
        if a.kernel_trace:
            res["kernels_left_out"] = "the rocPRIM scan of the member sizes and the memset before it (4097 values per 256 MiB of text): the statistics list them under names the other stages share"
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not write_table(res, a.design):
        print("no bgzf_probe marker lines in", a.design, "-- table not written", file=sys.stderr)


if __name__ == "__main__":
    main()
