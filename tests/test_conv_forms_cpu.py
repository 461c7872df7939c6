"""The table of conv forms the library is built from (infur_amd/csrc/conv_forms.h), printed by tests/cpp/conv_forms_test.cpp, against
the hand-written restatements the GPU tests are driven by: tests/forms.py (names and index sets per mode) and
tests/test_tune_db_cpu.py (the three-byte mode's forms and N tiles).  The program is plain g++ -- the header includes no HIP -- and
runs a second time built with the address and undefined-behaviour sanitizers.

The same program prints the SUB-forms: the size rules by which a launcher picks a kernel inside one configuration (conv_forms.h:
areg_small_rule, b2b_form_rule, halo_bn_rule, q8_nsplit_rule) at the values the sources' comments state and at each threshold +- 1,
and every word a profile record's variant tag can hold (kVariantWords).  tests/forms.py: SUBFORM_CASES, the cases of
tests/test_gpu_subforms.py, must name every one of those words: a new sub-form without a case fails here."""
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
        if p[0] in ("R", "V", "T"):  # the sub-forms: `subforms`
            continue
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


# ---- the sub-forms inside a configuration ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subforms(printed):
    """rules: (rule, arguments...) -> value; words: the variant words; tags: the composed tags"""
    rules, words, tags = {}, [], []
    for ln in printed.splitlines():
        p = ln.split()
        if p[0] == "R":
            rules[(p[1],) + tuple(int(x) for x in p[2:-1])] = int(p[-1])
        elif p[0] == "V":
            words.append(p[1])
        elif p[0] == "T":
            tags.append(p[1])
    return rules, words, tags


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def maps(h, w):
    """the stride-4 map (stem + max-pool) and the stride-8 map (layer2; layer3, layer4 and the heads are dilated) of an h x w frame"""
    s4 = tuple(conv_out(conv_out(n, 7, 2, 3), 3, 2, 1) for n in (h, w))
    return s4, tuple(conv_out(n, 3, 2, 1) for n in s4)


def test_size_rules_at_the_values_the_sources_state(subforms):
    rules, _, _ = subforms
    # conv1x1_areg.hip / conv1x1_b2b.hip: more than 170 workgroups of 256 pixels
    for m, small in ((1, 1), (104, 1), (4096, 1), (34 * 61, 1), (43519, 1), (43520, 1), (43521, 0), (135 * 240, 1), (270 * 480, 0)):
        assert rules[("areg_small", m)] == small, m
        assert rules[("b2b_form", m)] == (3 if small else 1), m
    # conv3x3_halo.hip: "layer2 conv2 at 1080p: 128 tiles x ONE N tile" runs BN = 64; Cout 256 on the same map BN = 128
    assert rules[("halo_bn", 135, 240, 128)] == 64 and rules[("halo_bn", 135, 240, 256)] == 128 and rules[("halo_bn", 135, 240, 512)] == 128
    for hw in ((1, 1), (17, 31), (34, 61)):  # the maps of forms.SIZES: always the small side
        assert all(rules[("halo_bn",) + hw + (c,)] == 64 for c in (64, 128, 256, 512)), hw
    assert all(rules[("halo_bn", h, w, 64)] == 64 for h, w in ((98, 113), (195, 225), (135, 240)))
    # conv1x1_q8.hip: "M = 32400 alone gives 254 workgroups": split 2; 480 workgroups = two per CU
    assert rules[("q8_nsplit", 32400, 2048)] == 2
    assert [rules[("q8_nsplit", 1, c)] for c in (128, 256, 512, 1024, 2048)] == [0, 2, 4, 8, 16]
    assert [rules[("q8_nsplit", 17 * 31, c)] for c in (128, 256, 512, 1024, 2048)] == [0, 2, 4, 8, 16]
    assert rules[("q8_nsplit", 30592, 2048)] == 4 and rules[("q8_nsplit", 30593, 2048)] == 2  # 239 / 240 M tiles of 128 pixels
    assert rules[("q8_nsplit", 61312, 2048)] == 2 and rules[("q8_nsplit", 61313, 2048)] == 0  # 479 / 480
    assert all(rules[("q8_nsplit", m, 128)] == 0 for m in (1, 32400, 61313))  # a single N tile


def test_the_natural_size_flips_both_f16_rules(subforms):
    """forms.NATURAL_SIZES: the figures its comment states, through the library's own rules"""
    rules, _, _ = subforms
    assert F.NATURAL_SIZES == [(777, 897)]
    s4, s8 = maps(777, 897)
    assert s4 == (195, 225) and s8 == (98, 113)
    assert rules[("areg_small", s4[0] * s4[1])] == 0 and rules[("areg_small", s8[0] * s8[1])] == 1  # 172 tiles of 256 pixels; 44
    assert -(-s4[0] * s4[1] // 256) == 172 and -(-s8[0] // 16) * -(-s8[1] // 16) == 56
    assert rules[("halo_bn",) + s8 + (512,)] == 128 and rules[("halo_bn",) + s8 + (256,)] == 64 and rules[("halo_bn",) + s8 + (128,)] == 64
    assert rules[("halo_bn",) + s4 + (64,)] == 64
    # ragged against every tile
    assert all((s[0] * s[1]) % t for s in (s4, s8) for t in (64, 128, 256)) and all(n % 16 and n % 8 and n % 6 for n in s4 + s8)
    # the sizes of forms.SIZES stay on the small side of both rules, which is why this size exists
    for h, w in F.SIZES:
        for m in maps(h, w):
            assert rules.get(("areg_small", m[0] * m[1]), 1) == 1
    assert maps(135, 241) == ((34, 61), (17, 31)) and maps(64, 256) == ((16, 64), (8, 32))


def test_subform_cases_name_every_variant_word(subforms):
    """a word the library can put into a variant tag and no case of tests/test_gpu_subforms.py must see: a sub-form nobody forces"""
    _, words, tags = subforms
    assert len(words) == len(set(words)) >= 26
    covered = set().union(*(c.words() for c in F.SUBFORM_CASES))
    assert not set(words) - covered, f"variant words without a case in forms.SUBFORM_CASES: {sorted(set(words) - covered)}"
    assert not covered - set(words), f"forms.SUBFORM_CASES expects words the library never says: {sorted(covered - set(words))}"
    for c in F.SUBFORM_CASES:
        assert not set(c.never) - set(words) and not set(c.never) & c.words(), c.id
    # every composed tag is made of the words (the N split of a Cout that is no power of two times 128 is a number like the others)
    for t in tags:
        for w in t.split(","):
            assert w in words or (w.startswith("nsplit") and w[6:].isdigit() and 2 <= int(w[6:]) <= 16), t
        assert len(t) < 24
    # each case has its baseline, each baseline is a case, ids are unique, hooks are the ones run_child clears
    ids = [c.id for c in F.SUBFORM_CASES]
    assert len(set(ids)) == len(ids)
    for c in F.SUBFORM_CASES:
        assert F.subform_baseline(c).key == c.key and set(c.env) <= set(F.SUBFORM_HOOKS) and c.sizes in F.SIZE_SETS, c.id
        assert c.mode in F.MODES and c.cfg in F.FORMS[c.mode] and c.tile in (0, 2, 4, 6)
    # the forced cases the sub-forms were found by
    have = {(c.mode, c.cfg, tuple(sorted(c.env.items())), c.tile, c.sizes) for c in F.SUBFORM_CASES}
    for want in [("f16", 15, (("INFUR_AREG_BM", "256"),), 0, "edge"), ("i8", 18, (("INFUR_Q8_NSPLIT", "2"),), 0, "edge"),
                 ("i8", 18, (("INFUR_Q8_NSPLIT", "4"),), 0, "edge"), ("i8", 18, (("INFUR_Q8_NSPLIT", "8"),), 0, "edge"),
                 ("f16", 19, (("INFUR_HALO_BN", "128"),), 0, "edge"), ("f32", 0, (("INFUR_WINO_LDS", "0"),), 0, "edge"),
                 ("f32", 0, (("INFUR_WINO_VEC", "1"),), 0, "edge"), ("f32", 0, (("INFUR_WINO_VEC", "2"),), 2, "edge"),
                 ("f32", 0, (("INFUR_WINO_VEC", "2"),), 4, "edge"), ("f32", 0, (("INFUR_WINO_VEC", "2"),), 0, "edge"),
                 ("f16", 0, (("INFUR_B2B", "1"), ("INFUR_B2B_DMA", "0")), 0, "edge"), ("f16", 0, (("INFUR_B2B", "1"), ("INFUR_B2B_DMA", "1")), 0, "edge"),
                 ("f16", 0, (("INFUR_STEM_F32", "1"),), 0, "edge"), ("f32s", 0, (("INFUR_STEM_F32", "1"),), 0, "edge"),
                 ("f16", 0, (), 0, "natural"), ("f16", 15, (), 0, "natural"), ("f16", 19, (), 0, "natural")]:
        assert want in have, want
