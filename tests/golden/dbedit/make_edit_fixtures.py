#!/usr/bin/env python3
"""Generate the `update` / `delete` / `shrink` / `getFrequency` fixtures under tests/golden/dbedit/ by RUNNING THE REFERENCE's
shipped binary, as tests/golden/dbindex/make_build_fixtures.py does for `build`.

Runs only in the development container, where the reference checkout exists (binaries/kASA_linux, v1.4.9, started through the
dynamic loader).  The old indices are the `build` fixtures of tests/golden/dbindex/ (and a 128-bit build of its `headers`
database, stored here as update128/old); every output is trimmed of the zero padding the reference writes after the
records and the trie.  Only data is kept: inputs and outputs.

    python tests/golden/dbedit/make_edit_fixtures.py
"""
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

REF = "/root/reference"
KASA = ["/lib64/ld-linux-x86-64.so.2", os.path.join(REF, "binaries", "kASA_linux")]
HERE = os.path.dirname(os.path.abspath(__file__))
DBINDEX = os.path.join(os.path.dirname(HERE), "dbindex")
SUFFIXES = ("", "_info.txt", "_trie", "_trie.txt", "_f.txt")
PROV = {}


def run(args, cwd, key):
    tmp = os.path.join(cwd, "tmp")
    os.makedirs(tmp, exist_ok=True)
    p = subprocess.run(KASA + args + ["-t", tmp + "/"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    shutil.rmtree(tmp, ignore_errors=True)
    for junk in ("stxxl.log", "stxxl.errlog"):
        if os.path.exists(os.path.join(cwd, junk)):
            os.remove(os.path.join(cwd, junk))
    if p.returncode != 0:
        sys.stderr.write(p.stdout)
        raise SystemExit("reference failed: " + " ".join(args))
    PROV[key] = args
    return p.stdout


def genome(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def lines(s, width):
    return "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))


def copy_index(src, dst):
    for s in SUFFIXES:
        if os.path.exists(src + s):
            shutil.copyfile(src + s, dst + s)


def keep(work, prefix, out_dir, name, rec_bytes):
    """the five files of `prefix` (in work) -> out_dir/name*, records and trie trimmed to the counts of the text files"""
    os.makedirs(out_dir, exist_ok=True)
    n = int(open(os.path.join(work, prefix + "_info.txt")).read().split()[0])
    m = int(open(os.path.join(work, prefix + "_trie.txt")).read().split()[0])
    for s in SUFFIXES:
        with open(os.path.join(work, prefix + s), "rb") as f:
            data = f.read()
        if s == "":
            data = data[:n * rec_bytes]
        elif s == "_trie":
            data = data[:m * 12]
        with open(os.path.join(out_dir, name + s), "wb") as f:
            f.write(data)


def first_sequence(path):
    seq, on = [], False
    for line in open(path):
        if line.startswith(">"):
            if on:
                break
            on = True
            continue
        seq.append(line.strip())
    return "".join(seq)


def new_database(out, rng, old_fasta, width):
    """two new genomes of new taxa and one that repeats a stretch of the old database (duplicates to drop)"""
    old = first_sequence(old_fasta)
    g = [genome(rng, 900), genome(rng, 700)]
    with open(os.path.join(out, "new.fasta"), "w") as f:
        f.write(">NEW_A.1 new taxon\n" + lines(g[0], width))
        f.write(">NEW_B.1 another new taxon\n" + lines(g[1], width))
        f.write(">NEW_C.1 overlaps the old index\n" + lines(old[100:500] + genome(rng, 200), width))


def main():
    if not os.path.exists(KASA[1]):
        raise SystemExit("needs the reference checkout (development container only)")
    rng = random.Random(900)
    headers = os.path.join(DBINDEX, "headers")
    hcontent = open(os.path.join(headers, "content.txt")).read()
    for d in ("update64", "update128", "update_one", "delete64", "delete128", "shrink", "getfreq"):
        if os.path.isdir(os.path.join(HERE, d)):
            shutil.rmtree(os.path.join(HERE, d))
    with tempfile.TemporaryDirectory() as work:
        # update, 64-bit: the `headers` index + new sequences (one repeats part of the old database)
        out = os.path.join(HERE, "update64")
        os.makedirs(out)
        new_database(out, rng, os.path.join(headers, "db.fasta"), 60)
        with open(os.path.join(out, "content.txt"), "w") as c:
            c.write(hcontent + "NewA\t901\t901\tNEW_A.1\nNewB\t902\t902\tNEW_B.1;NEW_C.1\n")
        copy_index(os.path.join(headers, "idx"), os.path.join(work, "old"))
        for f in ("new.fasta", "content.txt"):
            shutil.copyfile(os.path.join(out, f), os.path.join(work, f))
        run(["update", "-d", "old", "-o", "idx", "-i", "new.fasta", "-c", "content.txt", "-m", "4", "-n", "1"], work, "update64")
        keep(work, "idx", out, "idx", 12)
        # update, 128-bit: a --kH 25 build of the `headers` database (stored as old*) + the same kind of new sequences
        out = os.path.join(HERE, "update128")
        os.makedirs(out)
        shutil.copyfile(os.path.join(headers, "db.fasta"), os.path.join(work, "db.fasta"))
        shutil.copyfile(os.path.join(headers, "content.txt"), os.path.join(work, "hcontent.txt"))
        run(["build", "-c", "hcontent.txt", "-d", "old", "-i", "db.fasta", "--kH", "25", "-m", "4", "-n", "1"], work, "update128_old")
        keep(work, "old", out, "old", 20)
        new_database(out, rng, os.path.join(headers, "db.fasta"), 70)
        with open(os.path.join(out, "content.txt"), "w") as c:
            c.write(hcontent + "NewA\t901\t901\tNEW_A.1\nNewB\t902\t902\tNEW_B.1;NEW_C.1\n")
        for f in ("new.fasta", "content.txt"):
            shutil.copyfile(os.path.join(out, f), os.path.join(work, f))
        run(["update", "-d", "old", "-o", "idx", "-i", "new.fasta", "-c", "content.txt", "-m", "4", "-n", "1"], work, "update128")
        keep(work, "idx", out, "idx", 20)
        # update --one: every new sequence within one 20-line chunk of the reference's reader
        out = os.path.join(HERE, "update_one")
        os.makedirs(out)
        g = [genome(rng, 1000), genome(rng, 640)]
        with open(os.path.join(out, "new.fasta"), "w") as f:
            f.write(">NO0.1\n" + lines(g[0], 60) + ">NO1.1\n" + lines(g[1], 60))
        with open(os.path.join(out, "content.txt"), "w") as c:
            c.write(open(os.path.join(DBINDEX, "one", "content.txt")).read() + "OneNew\t33\t33\tNO0.1;NO1.1\n")
        copy_index(os.path.join(DBINDEX, "one", "idx"), os.path.join(work, "old"))
        for f in ("new.fasta", "content.txt"):
            shutil.copyfile(os.path.join(out, f), os.path.join(work, f))
        run(["update", "-d", "old", "-o", "idx", "-i", "new.fasta", "-c", "content.txt", "--one", "-m", "4", "-n", "1"], work, "update_one")
        keep(work, "idx", out, "idx", 12)
        # delete, 64-bit: the `multiline` index without taxon 1002 (and an ID no record carries)
        out = os.path.join(HERE, "delete64")
        os.makedirs(out)
        with open(os.path.join(out, "delnodes.dmp"), "w") as f:
            f.write("1002\t|\n\n424242\t|\n")
        copy_index(os.path.join(DBINDEX, "multiline", "idx"), os.path.join(work, "old"))
        shutil.copyfile(os.path.join(DBINDEX, "multiline", "content.txt"), os.path.join(work, "content.txt"))
        shutil.copyfile(os.path.join(out, "delnodes.dmp"), os.path.join(work, "delnodes.dmp"))
        run(["delete", "-d", "old", "-o", "idx", "-l", "delnodes.dmp", "-c", "content.txt", "-m", "4", "-n", "1"], work, "delete64")
        keep(work, "idx", out, "idx", 12)
        # delete, 128-bit: update128/old without taxon 77 (the reference's _info.txt lacks the "128" line)
        out = os.path.join(HERE, "delete128")
        os.makedirs(out)
        with open(os.path.join(out, "delnodes.dmp"), "w") as f:
            f.write("77\t|\n")
        copy_index(os.path.join(HERE, "update128", "old"), os.path.join(work, "old"))
        shutil.copyfile(os.path.join(headers, "content.txt"), os.path.join(work, "content.txt"))
        shutil.copyfile(os.path.join(out, "delnodes.dmp"), os.path.join(work, "delnodes.dmp"))
        with open(os.path.join(work, "old_info.txt"), "w") as f:
            f.write(open(os.path.join(HERE, "update128", "old_info.txt")).read())
        run(["delete", "-d", "old", "-o", "idx", "-l", "delnodes.dmp", "-c", "content.txt", "-m", "4", "-n", "1"], work, "delete128")
        keep(work, "idx", out, "idx", 20)
        # shrink: strategies 1 and 3 on the update results, 3 on `fivecol`, 3 without -c
        out = os.path.join(HERE, "shrink")
        os.makedirs(out)
        cases = [("s1_30", "update64", ["-s", "1", "-g", "30"], 12), ("s1_333", "update64", ["-s", "1", "-g", "33.3"], 12),
                 ("s1_150", "update64", ["-s", "1", "-g", "150"], 12), ("s1_333w", "update128", ["-s", "1", "-g", "33.3"], 20),
                 ("s3", "update64", ["-s", "3"], 12), ("s3w", "update128", ["-s", "3"], 20)]
        for name, src, args, rb in cases:
            copy_index(os.path.join(HERE, src, "idx"), os.path.join(work, "in"))
            shutil.copyfile(os.path.join(HERE, src, "content.txt"), os.path.join(work, "content.txt"))
            run(["shrink", "-d", "in", "-o", name, "-c", "content.txt", "-m", "4", "-n", "1"] + args, work, "shrink_" + name)
            keep(work, name, out, name, rb)
        copy_index(os.path.join(DBINDEX, "fivecol", "idx"), os.path.join(work, "in"))
        shutil.copyfile(os.path.join(DBINDEX, "fivecol", "content.txt"), os.path.join(work, "content.txt"))
        run(["shrink", "-d", "in", "-o", "s3_five", "-c", "content.txt", "-s", "3", "-m", "4", "-n", "1"], work, "shrink_s3_five")
        keep(work, "s3_five", out, "s3_five", 12)
        copy_index(os.path.join(HERE, "update64", "idx"), os.path.join(work, "in"))
        shutil.copyfile(os.path.join(HERE, "update64", "content.txt"), os.path.join(work, "in_content.txt"))
        run(["shrink", "-d", "in", "-s", "3", "-m", "4", "-n", "1"], work, "shrink_noc")
        keep(work, "in_s", out, "s_noc", 12)
        shutil.copyfile(os.path.join(work, "in_s_content.txt"), os.path.join(out, "s_noc_content.txt"))
        # getFrequency: _f.txt of the 64-bit update result, rewritten in place
        out = os.path.join(HERE, "getfreq")
        os.makedirs(out)
        copy_index(os.path.join(HERE, "update64", "idx"), os.path.join(work, "gf"))
        os.remove(os.path.join(work, "gf_f.txt"))
        shutil.copyfile(os.path.join(HERE, "update64", "content.txt"), os.path.join(work, "content.txt"))
        run(["getFrequency", "-d", "gf", "-c", "content.txt"], work, "getfreq")
        shutil.copyfile(os.path.join(work, "gf_f.txt"), os.path.join(out, "idx_f.txt"))
    ver = subprocess.run(KASA, stdout=subprocess.PIPE, text=True, timeout=60).stdout.splitlines()[0]
    with open(os.path.join(HERE, "PROVENANCE.json"), "w") as f:
        json.dump({"reference_binary": "binaries/kASA_linux", "banner": ver.split(" ran on")[0],
                   "generator": "tests/golden/dbedit/make_edit_fixtures.py", "old_indices": "tests/golden/dbindex/{headers,one,multiline,fivecol}/idx",
                   "runs": PROV}, f, indent=1)
    for r, _, fs in os.walk(HERE):
        print(r, sum(os.path.getsize(os.path.join(r, x)) for x in fs) // 1024, "KiB")


if __name__ == "__main__":
    main()
