"""Where the frame calls behind Regions stage Regions' and Anchors' products (infur_amd/csrc/region_layout.h), swept by
tests/cpp/region_layout_test.cpp: every offset on a 256-byte boundary, slots in order, disjoint and large enough for what is copied
into and out of them, rows == min(table_rows, npix), min(n, rows) rows copied back, nothing wrapping in 64 bits, and a total that is
the sum of the parts' aligned sizes -- what the nine hand-written layouts came to.  The program is plain g++ -- the header includes
no HIP -- and runs a second time built with the address and undefined-behaviour sanitizers; both must print the same."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "region_layout_test.cpp")
INC = os.path.join(ROOT, "infur_amd", "csrc")


def _run(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", INC, SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("region_layout")
    plain = _run(tmp, "region_layout_test", [])
    san = _run(tmp, "region_layout_test_san", ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return plain, san


def test_every_property_holds_in_both_builds(printed):
    plain, san = printed
    assert san == plain
    lines = plain.splitlines()
    assert "FAILED" not in plain and lines[-1].endswith(" checks, 0 failed") and int(lines[-1].split()[0]) > 10000
    # the grid: the eight planes, each from three starts with five table-row requests, alone and with three anchor-row requests
    swept = [ln for ln in lines if " layouts, " in ln]
    assert [ln.split(":")[0] for ln in swept] == ["0x0", "1x1", "1x63", "63x1", "1x64", "1x65", "61x97", "1x4097"]
    assert all(int(ln.split()[1]) == 3 * 5 * (1 + 3) for ln in swept)
    assert any(ln.startswith("largest: ") for ln in lines)


def test_the_header_includes_only_the_egress_layout():
    with open(os.path.join(INC, "region_layout.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert includes == ['"egress_layout.h"']
