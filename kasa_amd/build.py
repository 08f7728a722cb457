"""Build the HIP extension in-tree (kasa_amd/libkasa_hip.so) for gfx950 with hipcc."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "kasa_hip.hip")
HOST_SRCS = [os.path.join(HERE, "csrc", "kasa_refbatch.cpp")]   # host-only parts of the C ABI
SO = os.path.join(HERE, "libkasa_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "kasa_hip.h")
CSRC_HEADERS = [os.path.join(HERE, "csrc", "stdsort_order.h"), os.path.join(HERE, "csrc", "kasa_radix.h"), os.path.join(HERE, "csrc", "kasa_text.h"), os.path.join(HERE, "csrc", "kasa_replay.h"),
                os.path.join(HERE, "csrc", "kasa_build.h"), os.path.join(HERE, "csrc", "kasa_edit.h"), os.path.join(HERE, "csrc", "kasa_spill.h"), os.path.join(HERE, "csrc", "kasa_spill_plan.h"), os.path.join(HERE, "csrc", "kasa_parse.h"), os.path.join(HERE, "csrc", "kasa_bgzf.h"), os.path.join(HERE, "csrc", "kasa_inflate.h"), os.path.join(HERE, "csrc", "kasa_gunzip.h"), os.path.join(HERE, "csrc", "kasa_filter.h"), os.path.join(HERE, "csrc", "kasa_pager.h"),
                os.path.join(HERE, "host", "grisu_powers.inc")]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required)")


def build(force: bool = False) -> str:
    newest = max(os.path.getmtime(p) for p in [SRC, HEADER] + HOST_SRCS + CSRC_HEADERS)
    if not force and os.path.exists(SO) and os.path.getmtime(SO) >= newest:
        return SO
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
           "-Wall", "-Wno-unused-result", "-o", SO, SRC] + HOST_SRCS + ["-ldl", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return SO


HOST_SRC = os.path.join(HERE, "host", "kasa_identify.cpp")
HOST_BIN = os.path.join(HERE, "host", "kasa_identify")
INDEX_BIN = os.path.join(HERE, "host", "kasa_index")          # the same source with -DKASA_INDEX_TOOL: merge | redundancy | trie


def build_host(force: bool = False) -> str:
    """The C++ host driver (kASA's `identify` CLI over the C ABI).  KASA_IDENTIFY: another build of it (tools/asan_run.sh)."""
    other = os.environ.get("KASA_IDENTIFY")
    if other and os.path.exists(other):
        return other
    build()
    newest = max(os.path.getmtime(p) for p in (HOST_SRC, HEADER, os.path.join(HERE, "host", "grisu_powers.inc")))
    if not force and os.path.exists(HOST_BIN) and os.path.getmtime(HOST_BIN) >= newest:
        return HOST_BIN
    cmd = ["g++", "-O2", "-std=c++17", "-pthread", "-o", HOST_BIN, HOST_SRC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + HERE, "-lkasa_hip", "-lz", "-L/opt/rocm/lib", "-lrccl",
           "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return HOST_BIN


def build_index_tool(force: bool = False) -> str:
    """kasa_index (`merge`, `redundancy`, `trie`): kasa_identify.cpp compiled with -DKASA_INDEX_TOOL."""
    build()
    newest = max(os.path.getmtime(p) for p in (HOST_SRC, HEADER, os.path.join(HERE, "host", "grisu_powers.inc")))
    if not force and os.path.exists(INDEX_BIN) and os.path.getmtime(INDEX_BIN) >= newest:
        return INDEX_BIN
    cmd = ["g++", "-O2", "-std=c++17", "-pthread", "-DKASA_INDEX_TOOL", "-o", INDEX_BIN, HOST_SRC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + HERE, "-lkasa_hip", "-lz",
           "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return INDEX_BIN


INFLATE_CHECK_SRC = os.path.join(os.path.dirname(HERE), "tools", "inflate_host_check.cpp")
INFLATE_CHECK_BIN = os.path.join(os.path.dirname(HERE), "tools", "inflate_host_check")


def build_inflate_check(force: bool = False) -> str:
    """tools/inflate_host_check: the decoder body of csrc/kasa_inflate.h for the CPU under AddressSanitizer + UBSan (a
    stand-alone program; nothing is preloaded)."""
    newest = max(os.path.getmtime(p) for p in (INFLATE_CHECK_SRC, HEADER, os.path.join(HERE, "csrc", "kasa_inflate.h")))
    if not force and os.path.exists(INFLATE_CHECK_BIN) and os.path.getmtime(INFLATE_CHECK_BIN) >= newest:
        return INFLATE_CHECK_BIN
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", INFLATE_CHECK_BIN, INFLATE_CHECK_SRC])
    return INFLATE_CHECK_BIN


GUNZIP_CHECK_SRC = os.path.join(os.path.dirname(HERE), "tools", "gunzip_host_check.cpp")
GUNZIP_CHECK_BIN = os.path.join(os.path.dirname(HERE), "tools", "gunzip_host_check")


def build_gunzip_check(force: bool = False) -> str:
    """tools/gunzip_host_check: the bodies and the rounds of csrc/kasa_gunzip.h for the CPU under AddressSanitizer + UBSan (a
    stand-alone program; nothing is preloaded)."""
    newest = max(os.path.getmtime(p) for p in (GUNZIP_CHECK_SRC, HEADER, os.path.join(HERE, "csrc", "kasa_inflate.h"), os.path.join(HERE, "csrc", "kasa_gunzip.h")))
    if not force and os.path.exists(GUNZIP_CHECK_BIN) and os.path.getmtime(GUNZIP_CHECK_BIN) >= newest:
        return GUNZIP_CHECK_BIN
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", GUNZIP_CHECK_BIN, GUNZIP_CHECK_SRC])
    return GUNZIP_CHECK_BIN


SPILL_PLAN_CHECK_SRC = os.path.join(os.path.dirname(HERE), "tools", "spill_plan_check.cpp")
SPILL_PLAN_CHECK_BIN = os.path.join(os.path.dirname(HERE), "tools", "spill_plan_check")


def build_spill_plan_check(force: bool = False) -> str:
    """tools/spill_plan_check: the slab plan of csrc/kasa_spill_plan.h for the CPU under AddressSanitizer + UBSan (a stand-alone
    program; nothing is preloaded)."""
    newest = max(os.path.getmtime(p) for p in (SPILL_PLAN_CHECK_SRC, os.path.join(HERE, "csrc", "kasa_spill_plan.h")))
    if not force and os.path.exists(SPILL_PLAN_CHECK_BIN) and os.path.getmtime(SPILL_PLAN_CHECK_BIN) >= newest:
        return SPILL_PLAN_CHECK_BIN
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
                           "-o", SPILL_PLAN_CHECK_BIN, SPILL_PLAN_CHECK_SRC])
    return SPILL_PLAN_CHECK_BIN


if __name__ == "__main__":
    print(build(force=True))
    print(build_host(force=True))
    print(build_index_tool(force=True))
