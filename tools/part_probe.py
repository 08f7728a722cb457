"""kasa_identify over the bench's synthetic index (4.2e8 records) as ONE index object and as range partitions of at most
--part-records records (KASA_INDEX_PART_RECORDS): same bytes out, and what the partitions cost.  Files in /dev/shm.
    python tools/part_probe.py [--reads 2000000] [--part-records 100000000] [--coherence] [--partition-devices 0,0]
--coherence: both runs with --coherence; the JSON then carries the time of the coherence step (the driver's clock around
kasa_batch_coherence, or around begin + one kasa_batch_match_depth_device per partition + finish: every one of these calls
returns with the device idle) and of the same runs' other device work.
--partition-devices a,b,...: a third run with the same partitions spread over these device slots, every partition once
(kasa_identify --partition-devices).  On ONE card (0,0) its figures beside the in-device partitions' show only what the copies
(slices, records, depth bytes, profile tables -- from the device to itself) and the host thread per partition cost; they say
nothing about a link between devices.  The JSON is also written to --out (default profiles/partition_devices_probe.json).
Prints one JSON object."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--part-records", type=int, default=100_000_000)
    ap.add_argument("--memory", type=int, default=1024)
    ap.add_argument("--coherence", action="store_true")
    ap.add_argument("--partition-devices", default=None, help="device slots, e.g. 0,0: one more run with the partitions spread over them")
    ap.add_argument("--out", default=None, help="with --partition-devices: where the JSON goes as well (default profiles/partition_devices_probe.json)")
    args = ap.parse_args()
    import numpy as np
    from kasa_amd import build, formats, synth
    g = synth.genomes(1400, 300_000, seed=11)
    ix = synth.index_from_genomes(g, device=0, K=12)
    reads = synth.reads_from_genomes(g, args.reads, 150, seed=1000)
    exe = build.build_host()
    d = tempfile.mkdtemp(prefix="kasa_part_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
    try:
        formats.write_index(ix, os.path.join(d, "idx"), os.path.join(d, "content.txt"))
        fq = os.path.join(d, "reads.fastq")
        with open(fq, "wb") as f:
            bases = reads.bases.reshape(reads.n, 150)
            for a in range(0, reads.n, 200000):
                blk = bases[a:a + 200000]
                f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (a + i, blk[i].tobytes(), b"I" * 150) for i in range(blk.shape[0])))
        res = {"reads": reads.n, "index_records": int(ix.n), "coherence": bool(args.coherence)}
        sums = {}
        runs = [("one_index", {}, []), ("partitions", {"KASA_INDEX_PART_RECORDS": str(args.part_records)}, [])]
        if args.partition_devices:
            runs.append(("partition_devices", {"KASA_INDEX_PART_RECORDS": str(args.part_records)}, ["--partition-devices", args.partition_devices]))
            res["partition_devices"] = args.partition_devices
        for name, env, extra in runs:
            out, prof = os.path.join(d, "out_%s.jsonl" % name), os.path.join(d, "prof_%s.csv" % name)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "identify", "-c", os.path.join(d, "content.txt"), "-d", os.path.join(d, "idx"), "-i", fq, "-q", out, "-p", prof,
                                "--jsonl", "-v", "-m", str(args.memory)] + (["--coherence"] if args.coherence else []) + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200,
                               env=dict(os.environ, KASA_HOST_TIMING="1", **env))
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                res[name] = {"error": r.stdout[-600:]}
                continue
            t = {}
            for line in r.stdout.splitlines():
                for key in ("Time compare", "Time file"):
                    if line.startswith("OUT: " + key + ":"):
                        t[key] = float(line.split(":")[2].split()[0])
                if line.startswith("OUT: Index of"):
                    t["partitions"] = int(line.split()[6])
                if line.startswith("OUT: Batches per owner:"):
                    t["batches_per_owner"] = [int(x) for x in line.split(":", 2)[2].split()]
                if line.startswith("OUT: coherence"):
                    w = line.replace(",", " ").replace(")", " ").split()
                    t["coherence_s"] = float(w[2])
                    if "begin" in w:                                  # partitions: begin / one depth call per partition / finish
                        t["coherence_parts_s"] = {"begin": float(w[w.index("begin") + 1]), "depth": float(w[w.index("partitions") + 1]), "finish": float(w[w.index("finish") + 1])}
                if line.startswith("OUT: device stages"):
                    t["device_stages_ms"] = line.split(":", 2)[2].strip()
            sums[name] = [hashlib.sha256(open(p, "rb").read()).hexdigest() for p in (out, prof)]
            res[name] = {"file_s": t.get("Time file"), "device_s": t.get("Time compare"), "partitions": t.get("partitions", 1), "wall_s_incl_index_load": round(wall, 2),
                         "device_stages_ms": t.get("device_stages_ms")}
            if "batches_per_owner" in t:
                res[name]["batches_per_owner"] = t["batches_per_owner"]
            if args.coherence:
                res[name]["coherence_s"] = t.get("coherence_s")
                if "coherence_parts_s" in t:
                    res[name]["coherence_parts_s"] = t["coherence_parts_s"]
            os.unlink(out)
        res["same_bytes"] = len(sums) == len(runs) and all(s == sums["one_index"] for s in sums.values())
        print(json.dumps(res))
        if args.partition_devices:
            path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "partition_devices_probe.json")
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
