"""What --filter writes for a read, and the split of a batch's reads into the two files, stated in plain Python: the
specification of kasa_pool_keep_records / kasa_batch_filter (kasa_amd/csrc/kasa_parse.h, kasa_filter.h).  It restates what
filterReads of kasa_amd/host/kasa_identify.cpp (and report.filter_reads) write once at least one read is flagged.

Record text of a read: every non-empty line of its record, each followed by one line feed.  A FASTA record runs from its
header line ('>' first) up to the next header or the text's end; a FASTQ record is four lines.  A '\\r' stays part of its
line (a line that is only "\\r" is not empty); a last line without a line feed gets one."""
import numpy as np


def lines_of(text: bytes):
    ls = text.split(b"\n")
    if ls and ls[-1] == b"":
        ls.pop()                                                   # nothing follows the last line feed
    return ls


def records(text: bytes, fasta: bool):
    """The record texts of the reads of `text` (whole records, as the device parser takes them), in order."""
    out = []
    ls = lines_of(text)
    if fasta:
        for l in ls:
            if l == b"":
                continue
            if l[:1] == b">":
                out.append(b"")
            out[-1] += l + b"\n"                                    # (a text of whole records starts with a header)
    else:
        assert len(ls) % 4 == 0, "a FASTQ text of whole records has four lines per record"
        for i in range(0, len(ls), 4):
            assert all(ls[i:i + 4]), "no empty line in a FASTQ record"
            out.append(b"".join(l + b"\n" for l in ls[i:i + 4]))
    return out


def offsets(recs):
    """u64[n + 1] running offsets of the records back to back."""
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    if recs:
        off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    return off


def split(recs, flags):
    """(clean bytes, contaminant bytes, clean reads, contaminant reads): record r goes to side 1 where flags[r] is not 0."""
    assert len(recs) == len(flags)
    clean = [r for r, f in zip(recs, flags) if not f]
    cont = [r for r, f in zip(recs, flags) if f]
    return b"".join(clean), b"".join(cont), len(clean), len(cont)


def header_of(rec: bytes) -> bytes:
    return rec.split(b"\n", 1)[0]
