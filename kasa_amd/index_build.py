"""`kASA build` for the device path: a reference FASTA + content file -> the index
files `identify` reads, built on the device by kasa_build_* (kasa_amd/csrc/kasa_build.h, capi.Builder).

What the reference's build mode leaves on disk (source/modes/Build.hpp:305-477, Trie.hpp:365-394,
kASA.hpp:449-575) is, per database sequence, every 3-frame window of K codons *including* the windows that run
over the end of the sequence (padded with '^' letters, down to a single real letter), tagged with the
sequence's tax ID, sorted by (k-mer, tax ID) and made unique.  That is exactly what the read encoder emits for
kLow = 1 (marker of 3(K-1) `X` bases), so the build is: encode with kLow = 1 -> sort -> unique -> trie + frequencies,
all on the device.
"""
from __future__ import annotations

import numpy as np

from . import capi, formats, reads


def accession_map(content_path: str) -> dict:
    """Accession -> tax ID as the reference's build reads the content file (Read.hpp:2958-3006): column 4 holds the
    accessions, ';'-separated; the tax ID is column 2, or column 5 from the first line that has five columns on; the
    first line that names an accession keeps it."""
    acc_to_tax = {}
    as_str = False
    with open(content_path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line == "":
                continue
            cols = line.split("\t")
            if len(cols) >= 5:
                as_str = True
            if len(cols) < 4:
                raise RuntimeError("Content file contains less than 4 columns, it may be damaged... "
                                   "The faulty line was: " + line + "\n")
            if as_str and len(cols) < 5:
                raise RuntimeError("Content file: tax IDs are in column 5 from an earlier line on, this line has 4 columns: " + line)
            tid = int(cols[4]) if as_str else int(cols[1])
            for acc in cols[3].split(";"):
                acc_to_tax.setdefault(acc, tid)
    return acc_to_tax


def accession_of(header: str, acc_to_tax: dict):
    """Tax ID of a database sequence from its header (without '>'), Read.hpp:2343-2366: the first word is split at '|',
    the first field that contains a '.' is the accession; if that is not listed, the whole header is looked up.  None:
    not listed at all (the reference skips the sequence)."""
    acc = ""
    for field in header.split(" ")[0].split("|"):
        if "." in field:
            acc = field
            break
    if acc in acc_to_tax:
        return acc_to_tax[acc]
    return acc_to_tax.get(header)


def build_index(fasta_path: str, content_path: str, device: int = 0, K: int = formats.K64, codon_lut=None,
                frames: int = 3, max_pairs_per_brick: int = 0, max_resident_records: int = 0) -> formats.Index:
    content = formats.read_content(content_path)
    acc_to_tax = accession_map(content_path)
    db = reads.parse_reads(fasta_path)
    keep, tax = [], []
    for i, name in enumerate(db.names):
        t = accession_of(name[:-1] if name.endswith(" ") else name, acc_to_tax)   # (names carry the reader's trailing space)
        if t is not None:
            keep.append(i)
            tax.append(t)
    lens = np.diff(db.offsets)[keep] if keep else np.zeros(0, np.int64)
    off = np.zeros(len(keep) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    bases = np.concatenate([db.bases[db.offsets[i]:db.offsets[i + 1]] for i in keep]) if keep else np.zeros(0, np.uint8)
    b = capi.Builder(content.taxids, K, frames, codon_lut, max_pairs_per_brick, device, max_resident_records)
    try:
        b.add(bases, off, np.asarray(tax, dtype=np.uint32), db.protein)
        b.finish()
        km, taxid, tp, tc, freq = b.fetch()
    finally:
        b.close()
    return formats.Index(km, taxid, formats.dense_tax(taxid, content), tp, tc, content, freq)
