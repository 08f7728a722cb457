"""`kasa_identify --partition-devices a,b,...`: what is wrong with the flag is said before any device call, so these
run without a device (the golden index is only read from disk)."""
import os
import subprocess

import pytest

from kasa_amd import build as hipbuild
from tests import helpers

PAIRS = os.path.join(helpers.GOLDEN, "pairs")


def _identify(extra):
    exe = hipbuild.build_host()
    cmd = [exe, "identify", "-c", os.path.join(PAIRS, "content.txt"), "-d", os.path.join(PAIRS, "idx"), "-i", os.path.join(PAIRS, "reads.fastq"),
           "-n", "1"] + list(extra)
    env = {k: v for k, v in os.environ.items() if k != "KASA_INDEX_PART_RECORDS"}
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=env)


def _refused(r):
    errors = [line for line in r.stderr.splitlines() if line.startswith("ERROR: ")]
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert len(errors) == 1 and "--partition-devices" in errors[0], r.stderr
    return errors[0]


@pytest.mark.parametrize("slots", ["", "0,x", "0,,1", ",0", "0,", "-1", "0 1"], ids=["empty", "0,x", "gap", "leading", "trailing", "negative", "blank"])
def test_a_malformed_slot_list_is_an_error(slots):
    _refused(_identify(["--partition-devices", slots]))


def test_the_flag_needs_its_list():
    _refused(_identify(["--partition-devices"]))


@pytest.mark.parametrize("other", [["--devices", "0"], ["--device", "0"]], ids=["devices", "device"])
@pytest.mark.parametrize("first", [True, False], ids=["before", "after"])
def test_the_flag_excludes_device_and_devices(other, first):
    mine = ["--partition-devices", "0,0"]
    msg = _refused(_identify(other + mine if first else mine + other))
    assert "--devices" in msg


def test_more_slots_than_the_index_has_trie_entries_is_said_so():
    """Partitions are cut between `_trie` entries: an index of m entries gives at most m partitions, and every slot needs one."""
    m = int(open(os.path.join(PAIRS, "idx_trie.txt")).read().split()[0])
    msg = _refused(_identify(["--partition-devices", ",".join(["0"] * (m + 1))]))
    assert "at least one partition" in msg and str(m + 1) + " device slots" in msg
