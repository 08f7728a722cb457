#!/usr/bin/env python3
"""How long `kasa_identify update | delete | shrink | getFrequency` take on the bench's index, and where the time goes.

The index is built from bench.py's database (synth.genomes(1400, 300_000, seed=11): 420 Mbp, 4.2e8 records, 5 GB) with
`kasa_identify build`, on tmpfs when it has room.  Then each edit runs once on it: update with 70 more genomes, delete 140
taxa, shrink -s 1 -g 50, -s 3, -s 2, getFrequency.  One JSON line: per step the wall time, the reading of the old index,
its upload (kasa_build_add_index), the device milliseconds per stage (kasa_build_stats / kasa_build_edit_stats) and the
writing of the outputs.

    python tools/edit_probe.py [--out profiles/edit_probe.json]
"""
import argparse
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

N_TAXA, LENGTH, SEED = 1400, 300_000, 11
N_NEW, SEED_NEW = 70, 12
TIMING = re.compile(r"edit timing: read (\S+) s, upload (\S+) s, parse (\S+) s, add (\S+) s, finish (\S+) s, write (\S+) s, total (\S+) s; "
                    r"device ms load\+filters (\S+) encode (\S+) sort\+unique (\S+) merge (\S+) emit (\S+)")


def write_fasta(path, content, g, first, append_content=None):
    import numpy as np
    n = g.shape[0]
    lines = g.reshape(n, LENGTH // 80, 80)
    block = np.concatenate([lines, np.full((n, LENGTH // 80, 1), ord("\n"), np.uint8)], axis=2).reshape(n, -1)
    with open(path, "wb") as f:
        for t in range(n):
            f.write(b">SYN%04d.1 synthetic taxon %d\n" % (first + t, first + t))
            f.write(block[t].tobytes())
    with open(content, "w") as c:
        for t in range(first + n if append_content else n):
            c.write("Taxon %d\t%d\t%d\tSYN%04d.1\n" % (t, 100 + t, 100 + t, t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kasa_amd import build as hipbuild, synth
    exe = hipbuild.build_host()
    shm = "/dev/shm"
    where = shm if os.path.isdir(shm) and shutil.disk_usage(shm).free > (20 << 30) else None
    d = tempfile.mkdtemp(prefix="kasa_edit_probe_", dir=where)
    res = {"probe": "edit_probe", "database": {"taxa": N_TAXA, "length": LENGTH, "seed": SEED, "new_taxa": N_NEW, "new_seed": SEED_NEW},
           "files_on": "tmpfs" if where else "disk", "steps": {}}
    try:
        write_fasta(d + "/db.fasta", d + "/content.txt", synth.genomes(N_TAXA, LENGTH, SEED), 0)
        write_fasta(d + "/new.fasta", d + "/content_all.txt", synth.genomes(N_NEW, LENGTH, SEED_NEW), N_TAXA, append_content=True)
        with open(d + "/delnodes.dmp", "w") as f:
            for t in range(0, N_TAXA, 10):
                f.write("%d\t|\n" % (100 + t))
        t = time.time()
        r = subprocess.run([exe, "build", "-i", d + "/db.fasta", "-c", d + "/content.txt", "-d", d + "/idx", "-n", "16"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        res["build_wall_s"] = round(time.time() - t, 3)
        if r.returncode != 0:
            res["build_stderr"] = r.stderr[-2000:]
            raise SystemExit(json.dumps(res))
        m = re.search(r"Index: (\d+) entries", r.stdout)
        res["records"], res["index_bytes"] = int(m.group(1)), os.path.getsize(d + "/idx")
        steps = {
            "update_70_genomes": ["update", "-d", d + "/idx", "-o", d + "/out", "-i", d + "/new.fasta", "-c", d + "/content_all.txt", "-n", "16"],
            "delete_140_taxa": ["delete", "-d", d + "/idx", "-o", d + "/out", "-l", d + "/delnodes.dmp", "-c", d + "/content.txt"],
            "shrink_s1_g50": ["shrink", "-d", d + "/idx", "-o", d + "/out", "-c", d + "/content.txt", "-s", "1", "-g", "50"],
            "shrink_s3": ["shrink", "-d", d + "/idx", "-o", d + "/out", "-c", d + "/content.txt", "-s", "3"],
            "shrink_s2": ["shrink", "-d", d + "/idx", "-o", d + "/out", "-c", d + "/content.txt", "-s", "2"],
            "getFrequency": ["getFrequency", "-d", d + "/idx", "-c", d + "/content.txt"],
        }
        for name, args in steps.items():
            t = time.time()
            r = subprocess.run([exe] + args + ["-v"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                               env=dict(os.environ, KASA_BUILD_TIMING="1"))
            st = {"wall_s": round(time.time() - t, 3), "rc": r.returncode}
            if r.returncode != 0:
                st["stderr"] = r.stderr[-2000:]
                res["steps"][name] = st
                break
            m = TIMING.search(r.stdout)
            if m:
                v = [float(x) for x in m.groups()]
                st.update({"read_s": v[0], "upload_s": v[1], "parse_s": v[2], "add_s": v[3], "finish_s": v[4], "write_s": v[5], "total_s": v[6],
                           "device_ms": {"load_filters": v[7], "encode": v[8], "sort_unique": v[9], "merge": v[10], "emit": v[11]}})
            m = re.search(r"Index: (\d+) entries, trie: (\d+) entries; (\d+) read from the index, (\d+) deleted, (\d+) shrunk away", r.stdout)
            if m:
                st.update({"records_out": int(m.group(1)), "trie": int(m.group(2)), "index_in": int(m.group(3)), "deleted": int(m.group(4)),
                           "shrunk": int(m.group(5))})
            res["steps"][name] = st
            for s in ("", "_info.txt", "_trie", "_trie.txt", "_f.txt"):
                if os.path.exists(d + "/out" + s):
                    os.remove(d + "/out" + s)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
