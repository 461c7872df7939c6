"""The staging layout and the row rules of the egress stages' host-pointer calls (infur_amd/csrc/egress_layout.h), swept by
tests/cpp/egress_layout_test.cpp: every offset on a 256-byte boundary, slots disjoint, in order and large enough, requests clamped
to what a frame can produce, nothing wrapping in 64 bits, and the rows-to-copy-back rule.  The program is plain g++ -- the header
includes no HIP -- and runs a second time built with the address and undefined-behaviour sanitizers; both must print the same."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "egress_layout_test.cpp")
INC = os.path.join(ROOT, "infur_amd", "csrc")


def _run(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", INC, SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("egress_layout")
    plain = _run(tmp, "egress_layout_test", [])
    san = _run(tmp, "egress_layout_test_san", ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return plain, san


def test_every_property_holds_in_both_builds(printed):
    plain, san = printed
    assert san == plain
    lines = plain.splitlines()
    assert "FAILED" not in plain and lines[-1].endswith(" checks, 0 failed") and int(lines[-1].split()[0]) > 100000
    # the grid: sixteen planes of the six sizes, 1 x n and n x 1 among them, each with every combination of rows, classes and bytes
    swept = [ln for ln in lines if " layouts, " in ln]
    assert len(swept) == 16 and all(int(ln.split()[1]) == 2 * 5 * 5 * 5 * 3 * 3 * 3 for ln in swept)
    assert {ln.split(":")[0] for ln in swept} >= {"0x0", "1x1", "1x63", "63x1", "1x64", "64x1", "1x65", "65x1", "1x4097", "4097x1"}


def test_the_header_includes_nothing_of_the_project():
    with open(os.path.join(INC, "egress_layout.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>"]
