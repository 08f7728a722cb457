#!/usr/bin/env python3
"""How long `kasa_identify build` takes on the bench's database, and where the time goes.

The database is bench.py's (synth.genomes(1400, 300_000, seed=11): 420 Mbp), written as FASTA (80-letter lines) with a
four-column content file to tmpfs when it has room.  One JSON line: the build's wall time and its split (parse, the
device stages of kasa_build_stats, file write), the bricks, and the same database through the old path (the device
encoder's pairs + numpy's formats.make_index) under a time limit.

    python tools/build_probe.py [--limit-numpy 120] [--out profiles/build_probe.json] [--resident-records N] [--runs R] [--no-numpy]

--resident-records N builds under a resident budget of N input records per slab (KASA_BUILD_RESIDENT_RECORDS: the runs go to host
memory, the index is finished in key-range slabs); "records/8" sizes N from an in-core build made first.  --runs R repeats the
build and lists every run; --driver names another build of kasa_identify (a parent commit's, for comparison).
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


def write_db(d):
    import numpy as np
    from kasa_amd import synth
    g = synth.genomes(N_TAXA, LENGTH, SEED)
    lines = g.reshape(N_TAXA, LENGTH // 80, 80)
    block = np.concatenate([lines, np.full((N_TAXA, LENGTH // 80, 1), ord("\n"), np.uint8)], axis=2).reshape(N_TAXA, -1)
    with open(os.path.join(d, "db.fasta"), "wb") as f, open(os.path.join(d, "content.txt"), "w") as c:
        for t in range(N_TAXA):
            f.write(b">SYN%04d.1 synthetic taxon %d\n" % (t, t))
            f.write(block[t].tobytes())
            c.write("Taxon %d\t%d\t%d\tSYN%04d.1\n" % (t, 100 + t, 100 + t, t))


# the old path in two children: the device part (encoder pairs, saved), then numpy alone under the time limit
PAIRS_LEG = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from kasa_amd import capi, formats, reads
d = %r
content = formats.read_content(d + "/content.txt")
db = reads.parse_reads(d + "/db.fasta")
boot = formats.make_index(np.array([1], dtype=np.uint64), content.taxids[1:2].copy(), content)
dix = capi.DeviceIndex(boot, 0, check_trie=False)
ctx = capi.Context(dix, 12, 1, 3)
ctx.upload(db.bases, db.offsets); ctx.encode(); ctx.sort_and_range()
km, seq = ctx.queries(); ctx.close(); dix.close()
np.save(d + "/km.npy", km); np.save(d + "/tax.npy", content.taxids[seq + 1])
"""
NUMPY_LEG = r"""
import sys, time
sys.path.insert(0, %r)
import numpy as np
from kasa_amd import formats
d = %r
content = formats.read_content(d + "/content.txt")
km, tax = np.load(d + "/km.npy"), np.load(d + "/tax.npy")
t = time.time()
ix = formats.make_index(km, tax, content)
print("NUMPY", time.time() - t, ix.n)
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit-numpy", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident-records", default=None, help="a number, or records/D: the D-th part of the index's records")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--driver", default=None)
    a = ap.parse_args()
    from kasa_amd import build as hipbuild
    exe = a.driver or hipbuild.build_host()
    shm = "/dev/shm"
    where = shm if os.path.isdir(shm) and shutil.disk_usage(shm).free > (16 << 30) else None
    d = tempfile.mkdtemp(prefix="kasa_build_probe_", dir=where)
    res = {"probe": "build_probe", "database": {"taxa": N_TAXA, "length": LENGTH, "seed": SEED, "bases": N_TAXA * LENGTH},
           "files_on": "tmpfs" if where else "disk"}
    try:
        t = time.time()
        write_db(d)
        res["fasta_write_s"] = round(time.time() - t, 2)
        env = dict(os.environ)
        resident = a.resident_records
        if resident and resident.startswith("records/"):               # an in-core build first: its records size the budget
            r = subprocess.run([exe, "build", "-i", d + "/db.fasta", "-c", d + "/content.txt", "-d", d + "/idx", "-n", "16"],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
            resident = str(int(re.search(r"Index: (\d+) entries", r.stdout).group(1)) // int(resident.split("/")[1]))
        if resident:
            env["KASA_BUILD_RESIDENT_RECORDS"] = res["resident_records"] = resident
        runs = []
        for _ in range(a.runs):
            t = time.time()
            r = subprocess.run([exe, "build", "-i", d + "/db.fasta", "-c", d + "/content.txt", "-d", d + "/idx", "-n", "16", "-v"],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
            wall = round(time.time() - t, 3)
            m = re.search(r"finish (\S+) s, write (\S+) s", r.stdout)
            runs.append({"wall_s": wall, "finish_s": float(m.group(1)) if m else None, "write_s": float(m.group(2)) if m else None})
        if a.runs > 1:
            res["runs"] = runs
        res["build_wall_s"] = wall
        res["build_rc"] = r.returncode
        if r.returncode != 0:
            res["build_stderr"] = r.stderr[-2000:]
        m = re.search(r"build timing: parse (\S+) s, add (\S+) s, finish (\S+) s, write (\S+) s, total (\S+) s; pairs (\d+), bricks (\d+), merges (\d+), "
                      r"device ms encode (\S+) sort\+unique (\S+) merge (\S+) emit ([^\s;]+)", r.stdout)
        if m:
            v = m.groups()
            res.update({"parse_s": float(v[0]), "add_s": float(v[1]), "finish_s": float(v[2]), "write_s": float(v[3]), "total_s": float(v[4]),
                        "pairs": int(v[5]), "bricks": int(v[6]), "merges": int(v[7]),
                        "device_ms": {"encode": float(v[8]), "sort_unique": float(v[9]), "merge": float(v[10]), "emit": float(v[11])}})
        m = re.search(r"spilled runs (\d+), slabs (\d+), copy ms up (\S+) down (\S+)", r.stdout)
        if m:
            res["spill"] = {"runs_spilled": int(m.group(1)), "slabs": int(m.group(2)), "upload_ms": float(m.group(3)), "download_ms": float(m.group(4))}
        m = re.search(r"Index: (\d+) entries, trie: (\d+) entries", r.stdout)
        if m:
            res["records"], res["trie"] = int(m.group(1)), int(m.group(2))
            res["index_bytes"] = os.path.getsize(d + "/idx")
        if os.path.exists(d + "/idx"):
            res["index_sha256"] = subprocess.run(["sha256sum", d + "/idx"], stdout=subprocess.PIPE, text=True).stdout.split()[0]
            os.remove(d + "/idx")
        p = None if a.no_numpy else subprocess.run([sys.executable, "-c", PAIRS_LEG % (ROOT, d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if p is None:
            pass
        elif p.returncode != 0:
            res["numpy_path"] = {"error": p.stderr[-1000:]}
        else:
            try:                                                   # (no device in this child: a time limit ends CPU work only)
                p = subprocess.run([sys.executable, "-c", NUMPY_LEG % (ROOT, d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                   timeout=a.limit_numpy)
                m = re.search(r"NUMPY (\S+) (\d+)", p.stdout)
                res["numpy_path"] = ({"make_index_s": round(float(m.group(1)), 2), "records": int(m.group(2))} if m else {"error": p.stderr[-1000:]})
            except subprocess.TimeoutExpired:
                res["numpy_path"] = {"make_index_timed_out_after_s": a.limit_numpy}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
