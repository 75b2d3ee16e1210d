"""The staging loop of the host-array ray queries (csrc/query_staging.h) on the CPU: tests/query_staging_probe.cpp drives the real loop with memcpy as its device
side, under AddressSanitizer and UBSan, through one column set per query family -- trace, trace + resolve with hits = NULL, pixel footprints with and without their
optional arrays, bounces with one output, chains of 8 segments, layers (walk + weigh, and weigh alone: the strided gather on the way up) at 16 and 3 layers -- at
counts 1, cap - 1, cap, cap + 1 and 3 cap + 2.  The header needs no HIP, so the probe is compiled against it alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sm64rt-legacy-renderer_amd", "csrc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("query_staging") / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "query_staging_probe.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("cap", [7, 1, 64])
def test_every_column_set_comes_back_whole(probe, cap):
    """Every caller output holds the expected record at every index and block, the guard bytes behind every caller array are intact, the copies stay inside a pin
    buffer of chunk x max(up, down) bytes and inside device buffers of chunk x record x blocks, a column without a caller array is never copied, and a chunk is
    up copies, one launch, down copies, one wait."""
    r = subprocess.run([probe, str(cap)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0
    assert r.stdout.strip().split("\n")[-1].endswith("cap %d, 0 failures" % cap)


def test_the_header_includes_no_hip():
    with open(os.path.join(CSRC, "query_staging.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<c") or i == "<algorithm>" for i in includes), includes
