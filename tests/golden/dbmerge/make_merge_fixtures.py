#!/usr/bin/env python3
"""Generate the `merge` / `redundancy` fixtures under tests/golden/dbmerge/ by RUNNING THE REFERENCE's shipped binary, as
tests/golden/dbedit/make_edit_fixtures.py does for the edit modes.

Runs only in the development container, where the reference checkout exists (binaries/kASA_linux, v1.4.9, started through the
dynamic loader).  Only data is kept: inputs and outputs, the records and the trie trimmed of the zero padding the reference
writes after them.

  merge64, merge128   a/, b/: two small random databases built by the reference (db.fasta, content.txt sorted by tax ID,
                      idx*).  They share taxon 500 (accession SH_1.1, the same columns 3 and 4 in both content files), whose
                      sequences overlap in one stretch (duplicates to drop); a second stretch lies in a genome of taxon 101
                      in a and of taxon 202 in b (k-mers whose taxa come from both sides).  m*: the reference's `merge`.  It
                      writes no m_info.txt and an m_f.txt of zeros, so the record count is asserted against the numpy union
                      of the two record sets, and m_f.txt is made by the reference's `getFrequency` on the merged index once
                      an m_info.txt has been written by hand.
  merge_lists         content files only: taxon 500 has different accession and species lists in the two files (the reference
                      joins them in hash-table order; tests compare those columns as sets).
  redundancy          stdout of `redundancy` with and without -v (without STXXL's own messages: the lines from "Number of
                      unique" on, or from the last "OUT:" line on) for dbindex/headers, dbindex/multiline,
                      dbedit/update128/old and clones6, a new index of six taxa that share one genome (redundancy/clones6/).

    python tests/golden/dbmerge/make_merge_fixtures.py
"""
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REF = "/root/reference"
KASA = ["/lib64/ld-linux-x86-64.so.2", os.path.join(REF, "binaries", "kASA_linux")]
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
DBINDEX = os.path.join(GOLDEN, "dbindex")
DBEDIT = os.path.join(GOLDEN, "dbedit")
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


def lines(s, width=60):
    return "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))


def copy_index(src, dst):
    for s in SUFFIXES:
        if os.path.exists(src + s):
            shutil.copyfile(src + s, dst + s)


def keep_built(work, prefix, out_dir, rec_bytes):
    """the five files of a reference build `prefix` (in work) -> out_dir/idx*, records and trie trimmed"""
    n = int(open(os.path.join(work, prefix + "_info.txt")).read().split()[0])
    m = int(open(os.path.join(work, prefix + "_trie.txt")).read().split()[0])
    for s in SUFFIXES:
        with open(os.path.join(work, prefix + s), "rb") as f:
            data = f.read()
        if s == "":
            data = data[:n * rec_bytes]
        elif s == "_trie":
            data = data[:m * 12]
        with open(os.path.join(out_dir, "idx" + s), "wb") as f:
            f.write(data)
    return n


def rec_dtype(rec_bytes):
    if rec_bytes == 12:
        return np.dtype([("kmer", "<u8"), ("tax", "<u4")])
    return np.dtype([("lo", "<u8"), ("hi", "<u8"), ("tax", "<u4")])


def union(a, b, rec_bytes):
    """the sorted unique union of two record arrays under (k-mer, tax ID) order"""
    x = np.concatenate([a, b])
    keys = (x["tax"], x["kmer"]) if rec_bytes == 12 else (x["tax"], x["lo"], x["hi"])
    x = x[np.lexsort(keys)]
    same = np.zeros(x.shape[0], dtype=bool)
    same[1:] = x[1:] == x[:-1]
    return x[~same]


def merge_case(name, rng, extra, rec_bytes, work):
    out = os.path.join(HERE, name)
    os.makedirs(os.path.join(out, "a"))
    os.makedirs(os.path.join(out, "b"))
    shared500, shared_x = genome(rng, 240), genome(rng, 210)
    dbs = {
        "a": ([("A1.1 first of a", genome(rng, 300) + shared_x + genome(rng, 150)), ("A2.1", genome(rng, 420)),
               ("SH_1.1 the shared taxon", genome(rng, 180) + shared500)],
              "TaxA1\t101\t101\tA1.1\nTaxA2\t102\t102\tA2.1\nShared\t500\t500\tSH_1.1\n"),
        "b": ([("B1.1 first of b", genome(rng, 200) + shared_x + genome(rng, 260)), ("SH_1.1 the shared taxon", shared500 + genome(rng, 200)),
               ("B2.1", genome(rng, 380))],
              "TaxB1\t202\t202\tB1.1\nShared\t500\t500\tSH_1.1\nTaxB2\t777\t777\tB2.1\n"),
    }
    counts = {}
    for side, (seqs, content) in dbs.items():
        d = os.path.join(out, side)
        with open(os.path.join(d, "db.fasta"), "w") as f:
            for head, seq in seqs:
                f.write(">" + head + "\n" + lines(seq))
        with open(os.path.join(d, "content.txt"), "w") as f:
            f.write(content)
        shutil.copyfile(os.path.join(d, "db.fasta"), os.path.join(work, side + ".fasta"))
        shutil.copyfile(os.path.join(d, "content.txt"), os.path.join(work, side + "_content.txt"))
        run(["build", "-c", side + "_content.txt", "-d", side, "-i", side + ".fasta", "-m", "4", "-n", "1"] + extra, work, name + "_build_" + side)
        counts[side] = keep_built(work, side, d, rec_bytes)
    for s in ("", "_trie", "_trie.txt", "_content.txt", "_f.txt", "_info.txt"):
        if os.path.exists(os.path.join(work, "m" + s)):
            os.remove(os.path.join(work, "m" + s))
    run(["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "m", "-m", "4", "-n", "1"], work, name + "_merge")
    assert not os.path.exists(os.path.join(work, "m_info.txt")), "the reference wrote an info file after all"
    dt = rec_dtype(rec_bytes)
    a = np.fromfile(os.path.join(out, "a", "idx"), dtype=dt)
    b = np.fromfile(os.path.join(out, "b", "idx"), dtype=dt)
    u = union(a, b, rec_bytes)
    assert u.shape[0] < a.shape[0] + b.shape[0], "no duplicate between the two indices"
    with open(os.path.join(work, "m"), "rb") as f:
        data = f.read()
    got = np.frombuffer(data[:u.shape[0] * rec_bytes], dtype=dt)
    assert np.array_equal(got, u), "the reference's merge is not the sorted unique union"
    assert not any(data[u.shape[0] * rec_bytes:]), "records after the union"
    m = int(open(os.path.join(work, "m_trie.txt")).read().split()[0])
    with open(os.path.join(out, "m"), "wb") as f:
        f.write(data[:u.shape[0] * rec_bytes])
    with open(os.path.join(work, "m_trie"), "rb") as f, open(os.path.join(out, "m_trie"), "wb") as g:
        g.write(f.read()[:m * 12])
    for s in ("_trie.txt", "_content.txt"):
        shutil.copyfile(os.path.join(work, "m" + s), os.path.join(out, "m" + s))
    zeros = open(os.path.join(work, "m_f.txt")).read()
    assert all(int(x) == 0 for line in zeros.splitlines() for x in line.split("\t")[1:]), "the reference's m_f.txt is not all zeros"
    # the true frequencies: an info file by hand, then the reference's getFrequency on the merged index
    with open(os.path.join(work, "m_info.txt"), "w") as f:
        f.write(str(u.shape[0]) + ("\n128" if rec_bytes == 20 else ""))
    PROV[name + "_info_by_hand"] = "m_info.txt = '%d%s' written by this script before getFrequency" % (u.shape[0], "\\n128" if rec_bytes == 20 else "")
    run(["getFrequency", "-d", "m", "-c", "m_content.txt"], work, name + "_getfreq")
    shutil.copyfile(os.path.join(work, "m_f.txt"), os.path.join(out, "m_f.txt"))
    return counts, u.shape[0]


def merge_lists(work):
    """the reference's content merge alone, on the indices merge128 left in `work`"""
    out = os.path.join(HERE, "merge_lists")
    os.makedirs(out)
    ca = "TaxA1\t101\t101\tA1.1\nTaxA2\t102\t102\tA2.1\nShared in a\t500\t500;501\tSH_1.1;SH_2.1;SH_3.1\n"
    cb = "TaxB1\t202\t202\tB1.1\nShared in b\t500\t502;500\tSH_4.1;SH_1.1;SH_3.1\nTaxB2\t777\t777\tB2.1\n"
    for name, text in (("a_content.txt", ca), ("b_content.txt", cb)):
        with open(os.path.join(out, name), "w") as f:
            f.write(text)
        with open(os.path.join(work, "l" + name), "w") as f:
            f.write(text)
    for s in ("", "_trie", "_trie.txt", "_f.txt"):
        if os.path.exists(os.path.join(work, "ml" + s)):
            os.remove(os.path.join(work, "ml" + s))
    run(["merge", "--firstIndex", "a", "--secondIndex", "b", "-o", "ml", "-c1", "la_content.txt", "-c2", "lb_content.txt", "-co", "ml_content.txt", "-m", "4", "-n", "1"],
        work, "merge_lists")
    shutil.copyfile(os.path.join(work, "ml_content.txt"), os.path.join(out, "m_content.txt"))


def report(stdout, verbose):
    ls = [x for x in stdout.splitlines() if "STXXL-MSG" not in x]      # (the disk-file messages name a temporary path)
    if verbose:
        first = next(i for i, x in enumerate(ls) if x.startswith("Number of unique"))
    else:
        first = max(i for i, x in enumerate(ls) if x.startswith("OUT:"))
    return "\n".join(ls[first:]) + "\n"


def redundancy_cases(rng, work):
    out = os.path.join(HERE, "redundancy")
    os.makedirs(os.path.join(out, "clones6"))
    g = genome(rng, 600)
    d = os.path.join(out, "clones6")
    with open(os.path.join(d, "db.fasta"), "w") as f:
        for i in range(6):
            f.write(">CL%d.1 clone %d\n" % (i, i) + lines(g))
    with open(os.path.join(d, "content.txt"), "w") as f:
        for i in range(6):
            f.write("Clone%d\t%d\t%d\tCL%d.1\n" % (i, 300 + i, 300 + i, i))
    shutil.copyfile(os.path.join(d, "db.fasta"), os.path.join(work, "clones.fasta"))
    shutil.copyfile(os.path.join(d, "content.txt"), os.path.join(work, "clones_content.txt"))
    run(["build", "-c", "clones_content.txt", "-d", "clones", "-i", "clones.fasta", "-m", "4", "-n", "1"], work, "clones6_build")
    keep_built(work, "clones", d, 12)
    cases = [("headers", os.path.join(DBINDEX, "headers", "idx"), os.path.join(DBINDEX, "headers", "content.txt")),
             ("multiline", os.path.join(DBINDEX, "multiline", "idx"), os.path.join(DBINDEX, "multiline", "content.txt")),
             ("wide", os.path.join(DBEDIT, "update128", "old"), os.path.join(DBINDEX, "headers", "content.txt")),
             ("clones6", os.path.join(d, "idx"), os.path.join(d, "content.txt"))]
    for name, idx, content in cases:
        copy_index(idx, os.path.join(work, "r_" + name))
        shutil.copyfile(content, os.path.join(work, "r_" + name + "_content.txt"))
        for verbose in (False, True):
            so = run(["redundancy", "-d", "r_" + name, "-c", "r_" + name + "_content.txt"] + (["-v"] if verbose else []), work,
                     "redundancy_" + name + ("_v" if verbose else ""))
            with open(os.path.join(out, name + ("_v" if verbose else "") + ".txt"), "w") as f:
                f.write(report(so, verbose))


def main():
    if not os.path.exists(KASA[1]):
        raise SystemExit("needs the reference checkout (development container only)")
    rng = random.Random(1409)
    for d in ("merge64", "merge128", "merge_lists", "redundancy"):
        if os.path.isdir(os.path.join(HERE, d)):
            shutil.rmtree(os.path.join(HERE, d))
    sizes = {}
    with tempfile.TemporaryDirectory() as work:
        sizes["merge64"] = merge_case("merge64", rng, [], 12, work)
        sizes["merge128"] = merge_case("merge128", rng, ["--kH", "25"], 20, work)
        merge_lists(work)
        redundancy_cases(rng, work)
    ver = subprocess.run(KASA, stdout=subprocess.PIPE, text=True, timeout=60).stdout.splitlines()[0]
    with open(os.path.join(HERE, "PROVENANCE.json"), "w") as f:
        json.dump({"reference_binary": "binaries/kASA_linux", "banner": ver.split(" ran on")[0],
                   "generator": "tests/golden/dbmerge/make_merge_fixtures.py",
                   "old_indices": "tests/golden/dbindex/{headers,multiline}/idx, tests/golden/dbedit/update128/old",
                   "records": {k: {"a": v[0]["a"], "b": v[0]["b"], "union": v[1]} for k, v in sizes.items()},
                   "runs": PROV}, f, indent=1)
    for r, _, fs in os.walk(HERE):
        print(r, sum(os.path.getsize(os.path.join(r, x)) for x in fs) // 1024, "KiB")


if __name__ == "__main__":
    main()
