"""The table of conv forms the library is built from (infur_amd/csrc/conv_forms.h), printed by tests/cpp/conv_forms_test.cpp, against
the hand-written restatements the GPU tests are driven by: tests/forms.py (names and index sets per mode) and
tests/test_tune_db_cpu.py (the three-byte mode's forms and N tiles).  The program is plain g++ -- the header includes no HIP -- and
runs a second time built with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import forms as F  # noqa: E402
import test_tune_db_cpu as T  # noqa: E402

SRC = os.path.join(F.ROOT, "tests", "cpp", "conv_forms_test.cpp")
INC = os.path.join(F.ROOT, "infur_amd", "csrc")
MODE_NO = {"f32": 0, "f16": 1, "f32s": 2, "f32x": 3, "i8": 4, "f16hl": 5}  # ConvMode
# what the tuner's tie-break compares, per configuration number, in EVERY mode that has the number: BM x BN of the number's
# f16 form (for f16hl's 15 and 16 twice the tile that runs -- kept as it always was, see conv_forms.h)
TIE_AREA = {0: 16384, 1: 8192, 2: 8192, 3: 4096, 4: 8192, 5: 32768, 6: 32768, 7: 16384, 8: 8192, 9: 8192, 10: 4096, 11: 65536,
            12: 32768, 13: 65536, 14: 32768, 15: 32768, 16: 65536, 17: 32768, 18: 32768, 19: 32768, 20: 65536, 21: 65536}


def _run(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", INC, SRC, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("conv_forms")
    plain = _run(tmp, "conv_forms_test", [])
    san = _run(tmp, "conv_forms_test_san", ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert san == plain
    return plain


@pytest.fixture(scope="module")
def table(printed):
    """(mode number, cfg) -> dict of the admitted rows, in printed order; names: (mode number, cfg) -> (name, plain) of every pair"""
    rows, names = {}, {}
    for ln in printed.splitlines():
        p = ln.split()
        if p[0] == "#":  # no form: the name the library would still report
            names[(int(p[1]), int(p[2]))] = (p[3], p[4])
            continue
        mode, cfg, name, plain, bm, bn, area, tunable = int(p[0]), int(p[1]), p[2], p[3], int(p[4]), int(p[5]), int(p[6]), int(p[7])
        assert (mode, cfg) not in rows
        rows[(mode, cfg)] = dict(name=name, plain=plain, bm=bm, bn=bn, area=area, tunable=tunable)
        names[(mode, cfg)] = (name, plain)
    return rows, names


def test_forms_table_matches_the_library(table):
    """every name of tests/forms.py is the name the library reports for that (mode, configuration), and the index sets are the
    ones its table admits (formerly test_gpu_forms.py::test_forms_table_matches_the_sources, over the text of conv_igemm.hip)"""
    rows, names = table
    for mode, no in MODE_NO.items():
        for cfg, name in F.FORMS[mode].items():
            assert rows[(no, cfg)]["name"] == name, (mode, cfg, name)
            if mode == "f16hl" and cfg != F.HL_AREG:
                assert rows[(no, cfg)]["plain"] == name + ",plain", (cfg, name)
            else:  # no other form ever says ",plain"
                assert rows[(no, cfg)]["plain"] == name, (mode, cfg)
        # the index sets, from the table itself
        assert sorted(k for m, k in rows if m == no) == sorted(F.FORMS[mode]), mode
    assert [mk for mk in rows] == sorted(rows)  # printed in the order of the configuration numbers
    # all 22 numbers have a name in modes 0-4, a candidate there or not: the f32x / i8 names are the f32s ones with the tag replaced
    for cfg in range(22):
        f32s = names[(MODE_NO["f32s"], cfg)][0]
        assert "f32s<" in f32s
        for mode in ("f32", "f16", "f32x", "i8"):
            assert names[(MODE_NO[mode], cfg)][0] == f32s.replace("f32s", mode), (mode, cfg)
            assert F.FORMS[mode].get(cfg, f32s.replace("f32s", mode)) == f32s.replace("f32s", mode), (mode, cfg)
        assert F.FORMS["f32s"].get(cfg, f32s) == f32s
    # what is in no table
    for mode in range(-1, 7):
        for cfg in (-1, 22):
            assert names[(mode, cfg)] == (("conv_hl<?>",) * 2 if mode == 5 else ("conv_igemm<?>",) * 2)
    assert all(names[(m, k)] == ("conv_igemm<?>",) * 2 for m in (-1, 6) for k in range(22))
    assert all(names[(5, k)] == ("conv_hl<?>",) * 2 for k in range(22) if k not in F.FORMS["f16hl"])
    assert sorted(F.FORMS["f32"]) == sorted(F.FORMS["f32s"]) == sorted(F.FORMS["f32x"]) == list(range(13))
    assert sorted(F.FORMS["f16"]) == list(range(18)) + [19, 20, 21]
    assert sorted(F.FORMS["f16hl"]) == [0, 5, 6, 11, 12, 13, 14, 15, 16, 17]
    assert {15, 18, 19, 20} <= set(F.FORMS["i8"]) and 21 not in F.FORMS["i8"]
    assert all(len(n) + len(",plain") < 32 for n in F.FORMS["f16hl"].values())  # infur_kernel_record::kernel is char[32]
    assert all(len(n) < 32 and len(p) < 32 for n, p in names.values())
    n_hl = len(F.FORMS["f16hl"])
    assert len(F.cases()) == sum(len(v) for v in F.FORMS.values()) + n_hl == len(rows) + n_hl


def test_tie_break_areas_and_tunable_flags(table):
    rows, _ = table
    assert sorted(TIE_AREA) == list(range(22))
    for (mode, cfg), r in rows.items():
        assert r["area"] == TIE_AREA[cfg], (mode, cfg)
        assert r["tunable"] == (0 if cfg == 20 else 1), (mode, cfg)  # (INFUR_TUNE_HALO256 lifts it)
    # ... which is the tile itself everywhere but on the two rows conv_forms.h names
    odd = sorted((m, k) for (m, k), r in rows.items() if r["bm"] * r["bn"] != r["area"])
    assert odd == [(5, 15), (5, 16)]


def test_tune_db_tests_restate_the_three_byte_rows(table):
    rows, _ = table
    hl = {k: r for (m, k), r in rows.items() if m == MODE_NO["f16hl"]}
    assert set(hl) == T.HL_FORMS
    assert {k: r["bn"] for k, r in hl.items() if k != F.HL_AREG} == T.HL_BN
