#!/usr/bin/env python3
"""Generate the `build` fixtures under tests/golden/dbindex/ by RUNNING THE REFERENCE's shipped binary.

Runs only in the development container, where the reference checkout exists (binaries/kASA_linux, v1.4.9; started through
the dynamic loader because its mount drops the x bit, as tests/golden/make_fixtures.py does).  Every case is a small
database + content file, built with `kASA build`; the index files it wrote (records and trie trimmed of the zero padding
the reference adds, as in make_fixtures.py) are stored next to the inputs.  Only data is kept: inputs and outputs.

    python tests/golden/dbindex/make_build_fixtures.py        # regenerates every case
"""
import gzip
import json
import os
import random
import shutil
import subprocess
import sys

REF = "/root/reference"
KASA = ["/lib64/ld-linux-x86-64.so.2", os.path.join(REF, "binaries", "kASA_linux")]
HERE = os.path.dirname(os.path.abspath(__file__))

# the cases: name -> extra arguments of `build`; the input is db/ (a folder) where it exists, else db.fasta
CASES = {
    "folder": [],
    "headers": [],
    "multiline": [],
    "protein": [],
    "one": ["--one"],
    "fivecol": [],
}


def run(args, cwd):
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
    return p.stdout


def genome(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def lines(s, width):
    return "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))


def trim(d, rec_bytes):
    n = int(open(os.path.join(d, "idx_info.txt")).read().split()[0])
    m = int(open(os.path.join(d, "idx_trie.txt")).read().split()[0])
    for name, nbytes in (("idx", n * rec_bytes), ("idx_trie", m * 12)):
        p = os.path.join(d, name)
        with open(p, "rb") as f:
            data = f.read(nbytes)
        with open(p, "wb") as f:
            f.write(data)


def case_folder(out, rng):
    """Three FASTA files in a folder, one of them gzipped."""
    os.makedirs(os.path.join(out, "db"))
    g = [genome(rng, 900) for _ in range(4)]
    with open(os.path.join(out, "db", "a.fasta"), "w") as f:
        f.write(">ACC_A.1 first\n" + lines(g[0], 60) + ">ACC_B.1 second\n" + lines(g[1], 60))
    with open(os.path.join(out, "db", "b.fasta"), "w") as f:
        f.write(">ACC_C.1 third\n" + lines(g[2], 70))
    with gzip.open(os.path.join(out, "db", "c.fasta.gz"), "wt") as f:
        f.write(">ACC_D.1 fourth, shares a region with the first\n" + lines(g[3][:400] + g[0][100:500], 80))
    with open(os.path.join(out, "content.txt"), "w") as c:
        c.write("Alpha\t11\t11\tACC_A.1;ACC_D.1\nBeta\t12\t12\tACC_B.1\nGamma\t13\t13\tACC_C.1\n")


def case_headers(out, rng):
    """'|'-separated headers, a header matched only as a whole, an accession the content file does not list."""
    g = [genome(rng, 700) for _ in range(5)]
    with open(os.path.join(out, "db.fasta"), "w") as f:
        f.write(">gi|123|ref|NC_000913.3| Escherichia coli\n" + lines(g[0], 60))
        f.write(">emb|XY12|AB000001.2|extra words here\n" + lines(g[1], 60))
        f.write(">plain_header_without_dot some words\n" + lines(g[2], 60))
        f.write(">gi|999|ref|NOT_LISTED.1| unknown\n" + lines(g[3], 60))
        f.write(">XZ_5.1\n" + lines(g[4][:300] + g[0][:300], 60))
    with open(os.path.join(out, "content.txt"), "w") as c:
        c.write("Ecoli\t562\t562\tNC_000913.3\nOther\t77\t77\tAB000001.2;XZ_5.1\n"
                "Whole\t88\t88\tplain_header_without_dot some words\n")


def case_multiline(out, rng):
    """Sequences longer than the reader's 20-line chunk, N runs, lowercase letters, sequences shorter than K."""
    a = genome(rng, 2600)
    a = a[:700] + "N" * 25 + a[725:1500] + "nnnnn" + a[1505:]
    b = genome(rng, 1900).lower()
    b = b[:300] + b[300:900].upper() + b[900:]
    with open(os.path.join(out, "db.fasta"), "w") as f:
        f.write(">M1.1 long\n" + lines(a, 50))
        f.write(">M2.1 long lowercase\n" + lines(b, 37))
        f.write(">M3.1 short\n" + "ACGTACGTAC\n")
        f.write(">M4.1 shorter than three codons of K\n" + "ACGTTGCAACGTTGCAACGTTGCAACGTTGCA\n")
        f.write(">M5.1 tiny\nACG\n")
    with open(os.path.join(out, "content.txt"), "w") as c:
        c.write("One\t1001\t1001\tM1.1;M3.1\nTwo\t1002\t1002\tM2.1;M4.1\nThree\t1003\t1003\tM5.1\n")


def case_protein(out, rng):
    """An amino-acid database."""
    aa = "ACDEFGHIKLMNPQRSTVWY"
    p = ["".join(rng.choice(aa) for _ in range(n)) for n in (400, 350, 20, 8)]
    p[1] = p[1][:100] + p[0][50:150] + p[1][200:]
    with open(os.path.join(out, "db.fasta"), "w") as f:
        for i, s in enumerate(p):
            f.write(">P%d.1 protein %d\n%s" % (i, i, lines(s, 60)))
    with open(os.path.join(out, "content.txt"), "w") as c:
        c.write("ProtA\t21\t21\tP0.1;P2.1\nProtB\t22\t22\tP1.1\nProtC\t23\t23\tP3.1\n")


def case_one(out, rng):
    """--one: one frame.  Every sequence fits one chunk of the reference's reader (fewer than 20 lines): where a sequence goes on
    past one, the reference carries the last 3K - 1 bases over to the next chunk and its one frame continues from there, a
    frame that depends on where the chunk ended -- the device build's one frame runs through the whole sequence."""
    g = [genome(rng, n) for n in (1100, 1130, 700)]
    with open(os.path.join(out, "db.fasta"), "w") as f:
        for i, s in enumerate(g):
            f.write(">O%d.1\n%s" % (i, lines(s, 60)))
    with open(os.path.join(out, "content.txt"), "w") as c:
        c.write("OneA\t31\t31\tO0.1\nOneB\t32\t32\tO1.1;O2.1\n")


def case_fivecol(out, rng):
    """A content file with five columns: the tax ID is column 5."""
    g = [genome(rng, 800) for _ in range(3)]
    with open(os.path.join(out, "db.fasta"), "w") as f:
        for i, s in enumerate(g):
            f.write(">F%d.1\n%s" % (i, lines(s, 60)))
    with open(os.path.join(out, "content.txt"), "w") as c:
        c.write("FiveA\t1\t1\tF0.1\t4001\nFiveB\t2\t2\tF1.1\t4002\nFiveC\t3\t3\tF2.1\t4003\n")


def main():
    if not os.path.exists(KASA[1]):
        raise SystemExit("needs the reference checkout (development container only)")
    only = sys.argv[1:]
    for i, (name, extra) in enumerate(CASES.items()):
        if only and name not in only:
            continue
        out = os.path.join(HERE, name)
        if os.path.isdir(out):
            shutil.rmtree(out)
        os.makedirs(out)
        globals()["case_" + name](out, random.Random(500 + i))
        src = "db/" if os.path.isdir(os.path.join(out, "db")) else "db.fasta"
        run(["build", "-c", "content.txt", "-d", "idx", "-i", src, "-m", "4", "-n", "1"] + extra, out)
        trim(out, 12)
        print("wrote", out, sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(out) for f in fs) // 1024, "KiB")
    ver = subprocess.run(KASA, stdout=subprocess.PIPE, text=True, timeout=60).stdout.splitlines()[0]
    with open(os.path.join(HERE, "PROVENANCE.json"), "w") as f:
        json.dump({"reference_binary": "binaries/kASA_linux", "banner": ver.split(" ran on")[0],
                   "generator": "tests/golden/dbindex/make_build_fixtures.py",
                   "cases": {k: ["build", "-c", "content.txt", "-d", "idx", "-i", "db/" if k == "folder" else "db.fasta"] + v
                             for k, v in CASES.items()}}, f, indent=1)


if __name__ == "__main__":
    main()
