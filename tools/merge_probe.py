#!/usr/bin/env python3
"""How long `kasa_index merge | redundancy` take on the bench's index, and where the time goes (the companion of
tools/edit_probe.py, same columns).

merge       bench.py's database (synth.genomes(1400, 300_000, seed=11)) split by taxon into two halves that share 10 % of
            the taxa (taxa 0-769 and 630-1399), each built with `kasa_identify build`, then merged once.
redundancy  on the whole bench index and on the crowded one (synth.genomes_crowded, same size), each once plainly and once
            under `rocprofv3 --kernel-trace --stats`: the device time of the histogram pass (the head scan + edit_taxa_hist_kernel)
            next to edit_load_kernel's, the existing streaming pass over the same records.

One JSON line.   python tools/merge_probe.py [--out profiles/merge_probe.json] [--taxa 1400]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTH, SEED = 300_000, 11
MERGE_TIMING = re.compile(r"merge timing: read (\S+) s, upload (\S+) s, finish (\S+) s, write (\S+) s, total (\S+) s; device ms load (\S+) merge (\S+) emit (\S+)")
RED_TIMING = re.compile(r"redundancy timing: read (\S+) s, upload (\S+) s, histogram (\S+) s, total (\S+) s")


def write_fasta(path, content, g, taxa):
    import numpy as np
    lines = g.reshape(g.shape[0], LENGTH // 80, 80)
    block = np.concatenate([lines, np.full((g.shape[0], LENGTH // 80, 1), ord("\n"), np.uint8)], axis=2).reshape(g.shape[0], -1)
    with open(path, "wb") as f, open(content, "w") as c:
        for t in taxa:
            f.write(b">SYN%04d.1 synthetic taxon %d\n" % (t, t))
            f.write(block[t].tobytes())
            c.write("Taxon %d\t%d\t%d\tSYN%04d.1\n" % (t, 100 + t, 100 + t, t))


def run(cmd, timeout=600, **env):
    t = time.time()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=dict(os.environ, **env))
    return r, round(time.time() - t, 3)


def build(exe, d, name, res):
    r, wall = run([exe, "build", "-i", d + "/" + name + ".fasta", "-c", d + "/" + name + "_content.txt", "-d", d + "/" + name, "-n", "16"])
    if r.returncode != 0:
        res["stderr"] = r.stderr[-2000:]
        raise SystemExit(json.dumps(res))
    os.remove(d + "/" + name + ".fasta")
    return {"build_wall_s": wall, "records": int(re.search(r"Index: (\d+) entries", r.stdout).group(1)), "index_bytes": os.path.getsize(d + "/" + name)}


def kernel_ms(stats_dir):
    """device ms per kernel family from a rocprofv3 kernel_stats.csv"""
    out = {"edit_load_kernel": 0.0, "edit_taxa_hist_kernel": 0.0, "head_scan": 0.0, "other": 0.0}
    for f in glob.glob(stats_dir + "/**/*kernel_stats.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            ms = float(row["TotalDurationNs"]) / 1e6
            name = row["Name"]
            if "edit_load_kernel" in name:
                out["edit_load_kernel"] += ms
            elif "edit_taxa_hist_kernel" in name:
                out["edit_taxa_hist_kernel"] += ms
            elif "EditHeadPos" in name:
                out["head_scan"] += ms
            else:
                out["other"] += ms
    return {k: round(v, 3) for k, v in out.items()}


def redundancy(tool, d, name, res):
    st = {}
    r, wall = run([tool, "redundancy", "-d", d + "/" + name, "-c", d + "/" + name + "_content.txt", "-v"], KASA_BUILD_TIMING="1")
    st["wall_s"], st["rc"] = wall, r.returncode
    if r.returncode != 0:
        st["stderr"] = r.stderr[-2000:]
        return st
    m = RED_TIMING.search(r.stdout)
    if m:
        v = [float(x) for x in m.groups()]
        st.update({"read_s": v[0], "upload_s": v[1], "histogram_call_s": v[2], "total_s": v[3]})
    rows = re.findall(r"^(\d+) (\d+) (\S+)$", r.stdout, re.M)
    st["distinct_kmers"] = sum(int(c) for _, c, _ in rows)
    st["longest_run"] = max(int(i) for i, _, _ in rows)
    st["share_of_records_in_runs_over_50"] = round(sum(float(p) for i, _, p in rows if int(i) > 50), 3)
    st["out_line"] = r.stdout.strip().splitlines()[-1]
    prof = tempfile.mkdtemp(prefix="prof_", dir=d)
    r, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--", tool, "redundancy", "-d", d + "/" + name,
                "-c", d + "/" + name + "_content.txt"])
    if r.returncode == 0:
        st["device_ms"] = kernel_ms(prof)
    else:
        st["rocprof_stderr"] = r.stderr[-500:]
    shutil.rmtree(prof, ignore_errors=True)
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--taxa", type=int, default=1400)
    a = ap.parse_args()
    from kasa_amd import build as hipbuild, synth
    exe, tool = hipbuild.build_host(), hipbuild.build_index_tool()
    n = a.taxa
    lo_end, hi_start = n * 55 // 100, n * 45 // 100                      # 10 % of the taxa in both halves
    shm = "/dev/shm"
    where = shm if os.path.isdir(shm) and shutil.disk_usage(shm).free > (30 << 30) else None
    d = tempfile.mkdtemp(prefix="kasa_merge_probe_", dir=where)
    res = {"probe": "merge_probe", "database": {"taxa": n, "length": LENGTH, "seed": SEED, "first": [0, lo_end], "second": [hi_start, n]},
           "files_on": "tmpfs" if where else "disk", "indices": {}, "steps": {}}
    try:
        g = synth.genomes(n, LENGTH, SEED)
        write_fasta(d + "/a.fasta", d + "/a_content.txt", g, range(0, lo_end))
        write_fasta(d + "/b.fasta", d + "/b_content.txt", g, range(hi_start, n))
        write_fasta(d + "/idx.fasta", d + "/idx_content.txt", g, range(n))
        del g
        for name in ("a", "b", "idx"):
            res["indices"][name] = build(exe, d, name, res)
        r, wall = run([tool, "merge", "--firstIndex", d + "/a", "--secondIndex", d + "/b", "-o", d + "/m", "-v"], KASA_BUILD_TIMING="1")
        st = {"wall_s": wall, "rc": r.returncode}
        if r.returncode != 0:
            st["stderr"] = r.stderr[-2000:]
        m = MERGE_TIMING.search(r.stdout)
        if m:
            v = [float(x) for x in m.groups()]
            st.update({"read_s": v[0], "upload_s": v[1], "finish_s": v[2], "write_s": v[3], "total_s": v[4], "device_ms": {"load": v[5], "merge": v[6], "emit": v[7]}})
        m = re.search(r"Index: (\d+) entries, trie: (\d+) entries; (\d+) read from the two indices, (\d+) in both", r.stdout)
        if m:
            st.update({"records_out": int(m.group(1)), "trie": int(m.group(2)), "index_in": int(m.group(3)), "in_both": int(m.group(4))})
        if r.returncode == 0:
            st["equals_whole_build"] = all(open(d + "/m" + s, "rb").read() == open(d + "/idx" + s, "rb").read() for s in ("_info.txt", "_trie", "_trie.txt", "_f.txt")) and \
                subprocess.run(["cmp", "-s", d + "/m", d + "/idx"]).returncode == 0
        res["steps"]["merge_two_halves"] = st
        for s in ("", "_info.txt", "_trie", "_trie.txt", "_f.txt", "_content.txt"):
            for p in ("m", "a", "b"):
                if os.path.exists(d + "/" + p + s):
                    os.remove(d + "/" + p + s)
        res["steps"]["redundancy_bench"] = redundancy(tool, d, "idx", res)
        for s in ("", "_info.txt", "_trie", "_trie.txt", "_f.txt"):
            os.remove(d + "/idx" + s)
        g = synth.genomes_crowded(n, LENGTH, seed=SEED)
        write_fasta(d + "/crowded.fasta", d + "/crowded_content.txt", g, range(n))
        del g
        res["indices"]["crowded"] = build(exe, d, "crowded", res)
        res["steps"]["redundancy_crowded"] = redundancy(tool, d, "crowded", res)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
