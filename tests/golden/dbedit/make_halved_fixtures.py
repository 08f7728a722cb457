#!/usr/bin/env python3
"""Generate tests/golden/dbedit/halved_pads/ by RUNNING THE REFERENCE's shipped binary, as make_edit_fixtures.py does: a small
amino-acid database whose sequences hold '^' and '~' (both encode to the padding letter 30), built (`build`) and halved
(`shrink -s 2`).  Its k-mers hold a '^' at letter 5 over real letters, six '^' under a real letter, and trailing padding.

Runs only in the development container, where the reference checkout exists (binaries/kASA_linux, v1.4.9, started through the
dynamic loader).  Every output is trimmed of the zero padding the reference writes after the records and the trie.  Only data
is kept: inputs and outputs.

    python tests/golden/dbedit/make_halved_fixtures.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

REF = "/root/reference"
KASA = ["/lib64/ld-linux-x86-64.so.2", os.path.join(REF, "binaries", "kASA_linux")]
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "halved_pads")
SUFFIXES = ("", "_info.txt", "_trie", "_trie.txt", "_f.txt")

A = [("P0.1 protein 0", "MKVLAAGIWQ^ERTYHDNPFSCMKVLAAGIWQ"), ("P2.1 protein 2", "GHIKLM^^^^^^NPQRSTVWY"), ("P5.1 protein 5", "HIKLM^^^^^^NPQRSTV")]
B = [("P1.1 protein 1", "MKVLAAGIWQ^ERTYHD~CCDDEEFFGGHH"), ("P3.1 protein 3", "GHIKLM^^^^^^NPQRSTVWYAC"), ("P4.1 protein 4", "WYACDEFGHIKLMNPQRS^TVW")]
A_CONTENT = "ProtA\t21\t21\tP0.1;P2.1\nProtB\t22\t22\tP5.1\n"
B_CONTENT = "ProtB\t22\t22\tP1.1;P3.1\nProtC\t23\t23\tP4.1\n"


def fasta(seqs):
    return "".join(">%s\n%s\n" % (h, s) for h, s in seqs)


def run(args, cwd, prov, key):
    tmp = os.path.join(cwd, "tmp")
    os.makedirs(tmp, exist_ok=True)
    p = subprocess.run(KASA + args + ["-t", tmp + "/", "-m", "4", "-n", "1"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    shutil.rmtree(tmp, ignore_errors=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout)
        raise SystemExit("reference failed: " + " ".join(args))
    prov[key] = args
    return p.stdout


def keep(work, prefix, rec_bytes):
    n = int(open(os.path.join(work, prefix + "_info.txt")).read().split()[0])
    m = int(open(os.path.join(work, prefix + "_trie.txt")).read().split()[0])
    for s in SUFFIXES:
        with open(os.path.join(work, prefix + s), "rb") as f:
            data = f.read()
        if s == "":
            data = data[:n * rec_bytes]
        elif s == "_trie":
            data = data[:m * 12]
        with open(os.path.join(OUT, prefix + s), "wb") as f:
            f.write(data)


def main():
    os.makedirs(OUT, exist_ok=True)
    texts = {"a.fasta": fasta(A), "b.fasta": fasta(B), "u.fasta": fasta(A + B), "a_content.txt": A_CONTENT, "b_content.txt": B_CONTENT,
             "u_content.txt": "ProtA\t21\t21\tP0.1;P2.1\nProtB\t22\t22\tP5.1;P1.1;P3.1\nProtC\t23\t23\tP4.1\n"}
    prov = {"reference_binary": "binaries/kASA_linux", "generator": "tests/golden/dbedit/make_halved_fixtures.py", "runs": {}}
    with tempfile.TemporaryDirectory() as work:
        for name, text in texts.items():
            for d in (work, OUT):
                with open(os.path.join(d, name), "w") as f:
                    f.write(text)
        run(["build", "-c", "u_content.txt", "-d", "idx", "-i", "u.fasta"], work, prov["runs"], "build")
        run(["shrink", "-c", "u_content.txt", "-d", "idx", "-o", "idx_half", "-s", "2"], work, prov["runs"], "shrink")
        keep(work, "idx", 12)
        keep(work, "idx_half", 6)
    with open(os.path.join(OUT, "PROVENANCE.json"), "w") as f:
        json.dump(prov, f, indent=1)


if __name__ == "__main__":
    main()
