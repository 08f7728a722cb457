"""`kASA update | delete | shrink | getFrequency | merge | redundancy | trie` for the device path: an existing index edited by the builder
(kasa_amd/csrc/kasa_edit.h behind kasa_build_add_index / drop_taxa / shrink, capi.Builder).

Every function loads the index's records as a sorted run of a builder, lets the device merge and filter them, and returns
the result as a formats.Index (or writes the five index files with formats.write_index / write_index_halved).  The host
helpers below are the reference's own rules, shared with the C++ driver (kasa_amd/host/kasa_identify.cpp).
"""
from __future__ import annotations

import math

import numpy as np

from . import capi, formats, index_build, reads


def _records(ix: formats.Index) -> np.ndarray:
    if formats.is_wide(ix.kmer):
        rec = np.zeros(ix.n, dtype=formats.REC128_DTYPE)
        rec["lo"], rec["hi"] = ix.kmer["lo"], ix.kmer["hi"]
    else:
        rec = np.zeros(ix.n, dtype=formats.REC_DTYPE)
        rec["kmer"] = ix.kmer
    rec["tax"] = ix.taxid
    return rec


def _run(ix: formats.Index, content: formats.Content, edit, device: int = 0, chunk: int = 0, sequences=None,
         frames: int = 3, codon_lut=None, max_pairs_per_brick: int = 0) -> formats.Index:
    b = capi.Builder(content.taxids, ix.K, frames, codon_lut, max_pairs_per_brick, device)
    try:
        if sequences is not None:
            b.add(*sequences)
        b.add_index(_records(ix), chunk)
        edit(b)
        b.finish()
        km, taxid, tp, tc, freq = b.fetch()
        stats = b.edit_stats()
    finally:
        b.close()
    out = formats.Index(km, taxid, formats.dense_tax(taxid, content), tp, tc, content, freq)
    out.edit_stats = stats
    return out


def update_index(ix: formats.Index, fasta_path: str, content_path: str, device: int = 0, frames: int = 3, codon_lut=None,
                 chunk: int = 0, max_pairs_per_brick: int = 0) -> formats.Index:
    """update (Update.hpp:99-180): the sorted union of the index's records and those `build` makes of fasta_path with the
    content file content_path (which lists the old taxa and the new ones)."""
    content = formats.read_content(content_path)
    acc_to_tax = index_build.accession_map(content_path)
    db = reads.parse_reads(fasta_path)
    keep, tax = [], []
    for i, name in enumerate(db.names):
        t = index_build.accession_of(name[:-1] if name.endswith(" ") else name, acc_to_tax)
        if t is not None:
            keep.append(i)
            tax.append(t)
    lens = np.diff(db.offsets)[keep] if keep else np.zeros(0, np.int64)
    off = np.zeros(len(keep) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    bases = np.concatenate([db.bases[db.offsets[i]:db.offsets[i + 1]] for i in keep]) if keep else np.zeros(0, np.uint8)
    seqs = (bases, off, np.asarray(tax, dtype=np.uint32), db.protein)
    return _run(ix, content, lambda b: None, device, chunk, seqs, frames, codon_lut, max_pairs_per_brick)


def delete_taxa(ix: formats.Index, taxids, device: int = 0, chunk: int = 0) -> formats.Index:
    """delete (Update.hpp:28-90): the records whose tax ID is not in taxids, in the same order."""
    ids = np.asarray(list(taxids), dtype=np.uint32)
    return _run(ix, ix.content, lambda b: b.drop_taxa(ids), device, chunk)


def shrink_index(ix: formats.Index, strategy: int = 2, percentage: float = 0.0, device: int = 0, chunk: int = 0) -> formats.Index:
    """shrink -s strategy [-g percentage] (Shrink.hpp:152-370).  Strategy 2's Index keeps the full index's frequencies;
    write it with formats.write_index_halved."""
    return _run(ix, ix.content, lambda b: b.shrink(strategy, percentage), device, chunk)


def frequencies(ix: formats.Index, device: int = 0) -> np.ndarray:
    """getFrequency (main.cpp:1336-1362, kASA.hpp:449-575): the `_f.txt` rows of the index, recomputed on the device."""
    return _run(ix, ix.content, lambda b: None, device).freq


def merge_indices(ix1: formats.Index, ix2: formats.Index, content: formats.Content, device: int = 0, chunk: int = 0) -> formats.Index:
    """merge (Build.hpp:153-290): the sorted unique union of the records of two indices of the same width; content lists the
    taxa of both (merge_content writes its file).  Each index is a run of its own, the finish merges them."""
    if ix1.K != ix2.K:
        raise ValueError("Indices are not of the same format! One of them was created with a k larger than 12, unlike the other.")
    b = capi.Builder(content.taxids, ix1.K, 3, None, 0, device)
    try:
        b.add_index(_records(ix1), chunk)
        b.add_index(_records(ix2), chunk)
        b.finish()
        km, taxid, tp, tc, freq = b.fetch()
        stats = b.edit_stats()
    finally:
        b.close()
    out = formats.Index(km, taxid, formats.dense_tax(taxid, content), tp, tc, content, freq)
    out.edit_stats = stats
    return out


def redundancy(ix: formats.Index, device: int = 0):
    """redundancy (main.cpp:1364-1420, Shrink.hpp:35-72): (hist, cutoff) with hist[c] = the distinct k-mers of c taxa, counted
    on the device, and cutoff = redundancy_cutoff(hist, ix.n)."""
    b = capi.Builder(ix.content.taxids, ix.K, 3, None, 0, device)
    try:
        b.add_index(_records(ix))
        b.finish()
        hist, _ = b.taxa_histogram()
    finally:
        b.close()
    return hist, redundancy_cutoff(hist, ix.n)


def rebuild_trie(ix: formats.Index, device: int = 0):
    """trie (main.cpp:1422-1460): (prefix, count) of the `_trie` file, from the index's k-mers alone."""
    b = capi.Builder(ix.content.taxids, ix.K, 3, None, 0, device)
    try:
        b.add_index(_records(ix))
        b.finish()
        return b.fetch_trie()
    finally:
        b.close()


# ---- host rules -------------------------------------------------------------------------------------------------------

def read_delnodes(path: str) -> np.ndarray:
    """delnodes.dmp (Update.hpp:36-45): the first tab field of every non-empty line is a tax ID."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n").rstrip("\r")
            if line == "":
                continue
            out.append(int(line.split("\t")[0]))
    return np.asarray(out, dtype=np.uint32)


def shrink_thresholds(percentage: float, max_ordinal: int) -> np.ndarray:
    """The ordinals j <= max_ordinal that `shrink -s 1 -g percentage` drops from every taxon (Shrink.hpp:270-308): the
    percentage is a float (stof), step = 100.0 / fabsf(P) in double, d_1 = step, d_m+1 = d_m + step; j goes iff
    j == (uint64_t)d_m.  With step < 1 (|P| > 100) or P = 0 the first threshold, 0, is never met and nothing goes."""
    a = abs(float(np.float32(percentage)))
    out = []
    if a == 0.0:
        return np.zeros(0, np.uint64)
    step = 100.0 / a
    if not step >= 1.0:
        return np.zeros(0, np.uint64)
    d = step
    while int(d) <= max_ordinal:
        out.append(int(d))
        d += step
    return np.asarray(out, dtype=np.uint64)


def memory_percentage(memory_gib: int, n_records: int, record_bytes: int) -> float:
    """shrink -m without -g (main.cpp:839-857): the percentage that makes the index fit `memory_gib` GiB, in float."""
    mem = np.float32(float(memory_gib * 1024 ** 3))
    size = np.float32(float(n_records * record_bytes))
    return float(np.float32(np.float32(100.0) - np.float32(np.float32(100.0) * mem) / size))


def entropy_keeps(counts, K: int) -> bool:
    """The reference's entropy rule (Shrink.hpp:152-236) for a k-mer whose letters occur `counts` times: float terms
    float(c) / K * log2f(float(c) / K) summed in double, scaled by ln 2 / ln 22, kept iff > 0.5."""
    h = 0.0
    for c in counts:
        p = np.float32(np.float32(c) / np.float32(K))
        h += float(np.float32(p * np.log2(p, dtype=np.float32)))
    return (-h * math.log(2) / math.log(22)) > 0.5


def redundancy_cutoff(hist, n_records: int) -> int:
    """Shrink.hpp:60-71, literally: double(hist[i]) * i / n_records summed over i = 1, 2, ... in that order; the first i at
    which the sum is >= 0.99, 0 if it never is."""
    percentage = 0.0
    for i in range(1, len(hist)):
        percentage += float(int(hist[i])) * i / n_records
        if percentage >= 0.99:
            return i
    return 0


def _cout_double(x: float) -> str:
    """a double as std::cout writes it: precision 6, %g"""
    return "%g" % x


def redundancy_report(hist, n_records: int, verbose: bool = False) -> str:
    """The text `redundancy [-v]` prints (Shrink.hpp:55-65, main.cpp:1409-1419).  "Number of unique k-mers" is the distinct
    k-mers MINUS ONE, as the reference prints it: its loop counts a k-mer when the next one begins, so the last k-mer is
    never counted, while the histogram below it holds every k-mer."""
    out = []
    if verbose:
        distinct = sum(int(x) for x in hist[1:])
        out.append("Number of unique k-mers: %d" % max(distinct - 1, 0))
        out.append("Histogram")
        out.append("Frequency Counts Percentage")
        for i in range(1, len(hist)):
            if int(hist[i]) != 0:
                out.append("%d %d %s" % (i, int(hist[i]), _cout_double(100.0 * float(int(hist[i])) * i / n_records)))
    cut = redundancy_cutoff(hist, n_records)
    if cut == 1:
        out.append("OUT: 99% of the k-mers in your index have only one taxon. Using unique frequencies makes sense.")
    elif cut < 4:
        out.append("OUT: 99%% of the k-mers in your index have %d or less taxa. Using unique frequencies could make sense." % cut)
    else:
        out.append("OUT: 99%% of the k-mers in your index have %d or less taxa. You should consider looking at the non-unique frequencies as well." % cut)
    return "\n".join(out) + "\n"


def _join_lists(a: str, b: str) -> str:
    out = []
    for e in a.split(";") + b.split(";"):
        if e not in out:
            out.append(e)
    return ";".join(out)


def merge_content(path1: str, path2: str, out_path: str) -> None:
    """The content file of a merged index (GenerateContentFile.hpp:449-611): the rows of both files keyed by the numeric tax
    ID of column 2, ascending.  That is the reference's output whenever both inputs are sorted, as its two-pointer merge
    assumes; for unsorted inputs the reference interleaves wrongly, here the result is the sorted union all the same.  A taxon
    of both files takes the second file's name, and its columns 3 and 4 are the ';'-joined lists without repeats: the first
    file's entries in their order, then the second's new ones (the reference: in the order of a hash table).  Refused: a
    leading empty line, fewer than 4 columns, five columns (--taxidasstr) and EWAN dummy taxa, which the reference
    renumbers so that the dummies of the two indices collide."""
    rows = {}
    for path in (path1, path2):
        with open(path) as f:
            lines = f.read().split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        if not lines or lines[0].rstrip("\r") == "":
            raise ValueError("Invalid content files! %s has a leading empty line." % path)
        for line in lines:
            line = line.rstrip("\r")
            if line == "":
                continue
            cols = line.split("\t")
            if len(cols) < 4:
                raise ValueError("Content file contains less than 4 columns, it may be damaged... The faulty line was: " + line)
            if len(cols) >= 5:
                raise ValueError("merge reads the tax ID from column 2 of the content files: a content file with five columns is not supported (%s)" % path)
            if "EWAN" in cols[0]:
                raise ValueError("merge does not renumber dummy taxa: %s lists %s; give the sequences a taxon first" % (path, cols[0]))
            if not cols[1].isdigit():
                raise ValueError("Content file: the tax ID in column 2 is not a number: " + line)
            tid = int(cols[1])
            if tid in rows:
                old = rows[tid]
                rows[tid] = [cols[0], old[1], _join_lists(old[2], cols[2]), _join_lists(old[3], cols[3])]
            else:
                rows[tid] = cols[:4]
    with open(out_path, "w") as f:
        for tid in sorted(rows):
            f.write("\t".join(rows[tid]) + "\n")
