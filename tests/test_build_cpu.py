"""CPU-only checks of `build`'s host side: the reference's accession rule (Read.hpp:2343-2366), the content file as the
build reads it (Read.hpp:2958-3006), and the flags the device build refuses before any device work."""
import os
import subprocess

import pytest

from kasa_amd import build as hipbuild, index_build
from tests import helpers

BUILD = os.path.join(helpers.GOLDEN, "dbindex")


def test_accession_rule_header_forms():
    acc = {"NC_000913.3": 562, "AB000001.2": 77, "plain_header_without_dot some words": 88, "XZ_5.1": 77}
    assert index_build.accession_of("gi|123|ref|NC_000913.3| Escherichia coli", acc) == 562
    assert index_build.accession_of("emb|XY12|AB000001.2|extra words here", acc) == 77
    assert index_build.accession_of("XZ_5.1", acc) == 77
    assert index_build.accession_of("plain_header_without_dot some words", acc) == 88       # no '.': the whole header
    assert index_build.accession_of("plain_header_without_dot", acc) is None
    assert index_build.accession_of("gi|999|ref|NOT_LISTED.1| unknown", acc) is None        # the reference skips it
    # the first field with a '.' decides, even when a later one is listed
    assert index_build.accession_of("x.1|NC_000913.3", acc) is None
    # the old rule (first word as a whole) does not find these
    assert "gi|123|ref|NC_000913.3|" not in acc


def test_content_four_and_five_columns(tmp_path):
    four = tmp_path / "c4.txt"
    four.write_text("A\t11\t11\tX.1;Y.1\nB\t12\t12\tZ.1\n\nC\t13\t13\tX.1\n")
    assert index_build.accession_map(str(four)) == {"X.1": 11, "Y.1": 11, "Z.1": 12}        # first line keeps X.1
    five = tmp_path / "c5.txt"
    five.write_text("A\t1\t1\tF0.1\t4001\nB\t2\t2\tF1.1\t4002\n")
    assert index_build.accession_map(str(five)) == {"F0.1": 4001, "F1.1": 4002}
    mixed = tmp_path / "cm.txt"                                                              # column 5 from the first 5-column line on
    mixed.write_text("A\t1\t1\tF0.1\nB\t2\t2\tF1.1\t4002\nC\t3\t3\tF2.1\n")
    with pytest.raises(RuntimeError, match="column 5"):
        index_build.accession_map(str(mixed))
    bad = tmp_path / "bad.txt"
    bad.write_text("A\t1\t1\n")
    with pytest.raises(RuntimeError, match="less than 4 columns"):
        index_build.accession_map(str(bad))
    assert index_build.accession_map(os.path.join(BUILD, "fivecol", "content.txt"))["F2.1"] == 4003


def _host(args, tmp_path):
    exe = hipbuild.build_host()
    return subprocess.run([exe, "build"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))


@pytest.mark.parametrize("flag,extra", [("-g", ["50"]), ("--percentage", ["50"]), ("--continue", []), ("--spaced", []),
                                        ("-y", ["tax/"]), ("-f", ["acc2tax/"])])
def test_build_refuses_unsupported_flags(flag, extra, tmp_path):
    d = os.path.join(BUILD, "headers")
    r = _host(["-i", os.path.join(d, "db.fasta"), "-c", os.path.join(d, "content.txt"), "-d", str(tmp_path / "x"), flag] + extra, tmp_path)
    assert r.returncode == 1
    assert r.stderr.startswith("ERROR: ") and "not supported" in r.stderr
    assert not os.path.exists(str(tmp_path / "x"))


def test_build_needs_a_content_file(tmp_path):
    d = os.path.join(BUILD, "headers")
    r = _host(["-i", os.path.join(d, "db.fasta"), "-d", str(tmp_path / "x")], tmp_path)
    assert r.returncode == 1 and "content file" in r.stderr
    r = _host(["-i", os.path.join(d, "db.fasta"), "-c", str(tmp_path / "missing.txt"), "-d", str(tmp_path / "x")], tmp_path)
    assert r.returncode == 1 and r.stderr.strip() == "ERROR: Content file not found."
