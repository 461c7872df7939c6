"""Every forced conv form, sub-form and Winograd tile of every mode at the frame sizes tests/edge_cover.py DERIVES: the sizes that put
a kernel into the tile, border and tail cases forms.SIZES, NATURAL_SIZES and GEOM_SIZES never reach (the one-row tail tile and the
tail tile one row short of every BM, d < dim <= 2d at dilation 2, Winograd phases of 0 (mod 6), halo patches on 2 to 7 rows, ...;
tests/test_edge_cover_cpu.py proves the cover on the CPU).  The children are forms.run_child's, under its FATAL latch: after a child
that ends by signal, abort, time limit or a reported memory fault nothing more is started.

Baselines -- INFUR_CONV_CFG=0, arrays kept, one child per (mode, Winograd tile) of BASELINES: every tile test_gpu_own_error.VARIANTS
forces (F(6x6) is the context's default, tile 0) and the default of every mode, which the forced runs are compared with.  One case per
(baseline, size): every layer graded ALONE on the inputs the device stored (own_error.forced_taps / scope_of on the child's arrays
and the records of the launches that made them) under the own/* and own16/* bars of tests/accuracy.py, the product path's logits
under "edge" -- a (mode, kind) whose layers exceed the own row at these maps of 12 to 63 pixels for reasons of arithmetic (the mean error
of so few elements; where the worst elements sit is printed for every such layer) has a cover/<kind> row there, at 1.3 x measured, and
is graded under it (cover_scope; LAB_NOTES.md has the readings) --; i8: every layer's bytes, the logits and the mask equal oracle.infur_qoracle.qforward.

Forced runs -- one child per (mode, cfg, K loop) of forms.cases() and per forms.SUBFORM_CASES entry at the edge sizes, digests only:
all L/ and P/ digests equal the baseline's; a sub-form case whose `compare` is "stem" or "layers" keeps its arrays and is graded like
a baseline.

Proof that it ran -- from each child's product-path profile and the layer dimensions, edge_cover.met_classes: the classes the forced
form's OWN kernel met.  They must equal the literal edge_cover.REQUIRED[case]; a class the box reaches on a layer the form ran on
(edge_cover.reachable_on) that REQUIRED omits must carry a reason in edge_cover.OMITTED[case].  What every run meets whatever its
form (stem / pool parities, decode widths, Winograd phase lengths of the tile) is held per baseline in edge_cover.REQUIRED_WIDE.

INFUR_EDGE_COVER_LOG names a file that gets one JSON line per case (what was met, which layers carried the form, the child's time):
how REQUIRED is made, as INFUR_ACCURACY_LOG makes accuracy.MEASURED.
"""
import json
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import accuracy as A  # noqa: E402
import edge_cover as E  # noqa: E402
import forms as F  # noqa: E402
import own_error as OE  # noqa: E402
import test_gpu_forms as TF  # noqa: E402
from test_gpu_own_error import VARIANTS  # noqa: E402

from infur_amd import weights as W  # noqa: E402

gpu = pytest.mark.gpu
_LOG = os.environ.get("INFUR_EDGE_COVER_LOG", "")

# A cover child: two model loads, twelve frames up to 241x258, the read-back of 6 x 57 layers.  Measured on an MI355X: 2.9 s the first
# child of a run, 2.3 to 3.2 s the 130 of it; the limit is five times the first one's time, the factor beside forms.CHILD_TIMEOUT.
FIRST_CHILD_SECONDS = 2.9
COVER_TIMEOUT = round(5 * FIRST_CHILD_SECONDS)

SIZES = E.COVER_SIZES
# (mode, Winograd tile; 0: the default, F(6x6))
BASELINES = sorted({(m, 0) for m in F.MODES} | {(v[0], 0 if v[3] == 6 else v[3]) for v in VARIANTS if v[3]})
EDGE_SUBFORMS = [c for c in F.SUBFORM_CASES if c.sizes == "edge" and not c.baseline]


def log_line(**kw):
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(json.dumps(kw, sort_keys=True) + "\n")


class Shared:
    def __init__(self, tmp):
        self.tmp, self.base, self.digests, self.qblob_path = tmp, {}, {}, ""
        self.model64 = self.model16 = None
        self.ref, self.qref, self.taps = {}, {}, {}
        self.t0 = time.perf_counter()

    def qblob(self):
        if not self.qblob_path:
            from oracle import infur_qoracle as Q

            self.qblob_path = str(self.tmp / "qblob.bin")
            with open(self.qblob_path, "wb") as f:
                f.write(Q.synth_qblob())
        return self.qblob_path

    def child(self, name, mode, cfg, plain=False, env=None, tile=0, keep=False):
        t = time.perf_counter()
        run = F.run_child(mode, cfg, plain, str(self.tmp / (name + ".npz")), self.qblob() if mode == "i8" else "", extra_env=env, tile=tile,
                          sizes=SIZES, digest=not keep, timeout=COVER_TIMEOUT, records=keep)
        run.seconds = time.perf_counter() - t
        print(f"{name}: child took {run.seconds:.1f} s")
        return run

    def baseline(self, mode, tile):
        if (mode, tile) not in self.base:
            self.base[(mode, tile)] = self.child(f"base_{mode}_F{tile}", mode, 0, tile=tile, keep=True)
        return self.base[(mode, tile)]

    def baseline_digests(self, mode, tile):
        if (mode, tile) not in self.digests:
            self.digests[(mode, tile)] = F.digests(self.baseline(mode, tile))
        return self.digests[(mode, tile)]

    def models(self):
        if self.model64 is None:
            from oracle.infur_oracle import TorchModel

            self.model64 = TorchModel(W.synth_blob(), float64=True)
            self.model16 = OE.f16_weight_model(self.model64)
        return self.model64, self.model16

    def chw(self, oracle, size):
        return oracle.pack_normalize(W.synth_frame(size[0], size[1], index=size[0] + size[1]))

    def logits(self, oracle, size):
        """float64 out_low / aux_low of the reference's own chain, made once per size"""
        if size not in self.ref:
            lo, la = self.models()[0].forward_lowres(self.chw(oracle, size))
            self.ref[size] = {"out_low": lo.numpy(), "aux_low": la.numpy()}
        return self.ref[size]

    def quant(self, oracle, size):
        if size not in self.qref:
            from oracle import infur_qoracle as Q

            t = {}
            lo, la = Q.qforward(open(self.qblob(), "rb").read(), self.chw(oracle, size), t)
            t["out_low"], t["aux_low"] = lo, la
            self.qref[size] = t
        return self.qref[size]


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    s = Shared(tmp_path_factory.mktemp("edge_cover"))
    yield s
    print(f"\ntest_gpu_edge_cover.py: {time.perf_counter() - s.t0:.0f} s from the first case to the last")


def not_after_a_bad_end():
    if F.FATAL:
        pytest.fail(f"not started: an earlier child of this module ended badly ({F.FATAL[0]})")


# ---- grading --------------------------------------------------------------------------------------------------------------------------
def cover_scope(mode, scope):
    """own/<kind> -> cover/<kind> where tests/accuracy.py has such a row for the mode (a (mode, kind) whose layers at the cover sizes
    exceed the own row for reasons of arithmetic), else the own row itself"""
    cover = scope.replace("own", "cover", 1)
    return cover if (mode, cover) in A.MEASURED else scope


def where_worst(got, ref):
    """where the error of one layer sits: the pixel of the worst element, the share of the squared error on the map's border ring against
    the ring's share of the pixels, and the mean error of the last row of pixels (a tail tile's) against the map's"""
    d = np.asarray(got, np.float64) - ref
    c, y, x = np.unravel_index(int(np.abs(d).argmax()), d.shape)
    hh, ww = d.shape[1:]
    ring = np.ones((hh, ww), bool)
    ring[1:-1, 1:-1] = False
    e2 = (d * d).sum(0)
    flat = d.reshape(d.shape[0], -1)
    return (f"worst element at channel {c}, pixel ({y}, {x}) of {hh} x {ww}; border ring holds {e2[ring].sum() / max(e2.sum(), 1e-300):.0%} of the squared "
            f"error on {ring.mean():.0%} of the pixels; mean error of the last pixel {flat[:, -1].mean():.2e}, of the map {flat.mean():.2e}")


def grade_float_size(run, mode, size, shared, oracle, what):
    """one size of a run that kept its arrays: every layer alone, the product path's logits, the mask given its logits"""
    m64, m16 = shared.models()
    tag, (h, w) = F.tag(size), size
    acts = {s.name: run[f"L/{tag}/{s.name}"] for s in m64.specs}
    for spec, _, _, oh, ow in W.plan(h, w):
        assert acts[spec.name].shape == (spec.cout, oh, ow), (tag, spec.name, acts[spec.name].shape)
    chw = shared.chw(oracle, size)
    taps64 = OE.forced_taps(m64, chw, acts)
    taps16 = OE.forced_taps(m16, chw, acts) if mode == "f16" else None
    rows = OE.grade_rows(acts, taps64, run.layer_records[tag], m64.specs, mode, f"{what} {tag}", taps16)
    print(OE.format_table(rows, f"{what} {tag}"))
    assert len(rows) == 57
    worst, bad = {}, []
    for row in rows:
        for key, scope0 in (("r", row["scope"]), ("r16", row["scope"].replace("own/", "own16/"))):
            if key not in row:
                continue
            worst[scope0] = [max(a, b) for a, b in zip(worst.get(scope0, (0, 0, 0, 0)), row[key])]
            scope = cover_scope(mode, scope0)
            cap = row["cap"] if key == "r" else None
            missed = A.failures(row[key], mode, scope, cap)
            if missed or A.failures(row[key], mode, scope0, cap):  # over its own row: say where the worst elements sit
                print(f"{what} {tag} {row['name']} {scope0} {A.fmt(row[key])}: {where_worst(acts[row['name']], (taps64 if key == 'r' else taps16)[row['name']])}")
            if missed:
                bad.append(A.message(row[key], mode, scope, f"{what} {tag} {row['name']}", cap, missed))
    for scope in sorted(worst):
        print(f"{what} {tag}: worst {scope} {A.fmt(worst[scope])}, bars {A.fmt(A.effective_bars(mode, cover_scope(mode, scope)))} ({cover_scope(mode, scope)})")
    cap = (TF.mode_bars()[mode], None, None, None)
    ref = shared.logits(oracle, size)
    for name in ("out_low", "aux_low"):
        r = A.grade(run[f"P/{tag}/{name}"], ref[name], mode, "edge", f"{what} {tag} product path {name}", cap=cap, check=False)
        print(f"{what} {tag}: product path {name} {A.fmt(r)}, edge bars {A.fmt(A.effective_bars(mode, 'edge', cap))}")
        if A.failures(r, mode, "edge", cap):
            bad.append(A.message(r, mode, "edge", f"{what} {tag} product path {name}", cap))
    assert (run[f"P/{tag}/rgba"] == oracle.colorcode(oracle.upsample_bilinear(run[f"P/{tag}/out_low"], h, w))).all(), (what, tag)
    log_line(kind="own", what=what, size=tag, worst=worst)
    assert not bad, "\n".join(bad)


def grade_quant_size(run, size, shared, oracle):
    """as test_gpu_forms.grade_quant, one size: every layer's bytes, the dequantised logits and the mask equal the integer oracle's"""
    tag, (h, w) = F.tag(size), size
    ref = shared.quant(oracle, size)
    n = 0
    for spec in W.graph(50):
        if spec.role in ("cls", "auxcls"):
            continue  # the logit convs leave the stack dequantised: compared below
        got, want = run[f"L/{tag}/{spec.name}"], ref[spec.name]
        assert got.shape[1:] == want.shape[1:] and got.shape[0] >= want.shape[0], (tag, spec.name)
        assert (got[: want.shape[0]] == want.astype(np.float32)).all(), (tag, spec.name, int((got[: want.shape[0]] != want).sum()))
        assert (got[want.shape[0]:] == 0).all(), (tag, spec.name)  # channel padding of the 64-channel tensors
        n += 1
    assert n == 55
    for path in ("L", "P"):
        lo, la = run[f"{path}/{tag}/out_low"], run[f"{path}/{tag}/aux_low"]
        assert (lo.view(np.uint32) == ref["out_low"].view(np.uint32)).all() and (la.view(np.uint32) == ref["aux_low"].view(np.uint32)).all(), (path, tag)
    assert (run[f"P/{tag}/rgba"] == oracle.colorcode(oracle.upsample_bilinear(ref["out_low"], h, w))).all(), tag
    print(f"i8 {tag}: 55 layers, logits and mask bit-exact against the integer oracle")


def check_digests(base_digests, run, what, prefixes=("L/", "P/")):
    mine = {k[2:]: bytes(run[k]).hex() for k in run.keys() if k.startswith("D/")}
    if not mine:  # a run that kept its arrays
        mine = F.digests(run)
    assert sorted(mine) == sorted(base_digests), what
    bad = [k for k in sorted(mine) if k.startswith(prefixes) and mine[k] != base_digests[k]]
    assert not bad, f"{what}: differs from configuration 0 in {bad[:12]} ({len(bad)} tensors)"


# ---- proof that the form ran, and on what -----------------------------------------------------------------------------------------------
def check_met(case_id, mode, cfg, plain, run):
    met, carried = E.met_classes(mode, cfg, plain, run.variants)
    layers = sorted({n for v in carried.values() for n in v})
    print(f"{case_id} {F.expected_kernel(mode, cfg, plain)}: " + ", ".join(f"{t}: {len(v)} launches" for t, v in carried.items()))
    print(f"   layers: {' '.join(layers)}")
    print(f"   met: {' '.join(sorted(met))}")
    wrong_word = E.tiling_mismatches(mode, cfg, plain, run.variants)
    assert not wrong_word, f"{case_id}: the tiling a record names is not the one edge_cover.halo_tiling restates: {wrong_word[:8]}"
    log_line(kind="met", id=case_id, mode=mode, cfg=cfg, plain=plain, met=sorted(met), carried=carried, seconds=getattr(run, "seconds", None),
             other={t: sorted({(n, k) for n, k, _ in recs if E.record_layer(n) in layers}) for t, recs in run.variants.items()})
    assert layers, f"{case_id}: the forced form ran on no layer at any of {SIZES}"
    assert case_id in E.REQUIRED, f"{case_id}: no entry in edge_cover.REQUIRED; met {sorted(met)}"
    want = set(E.REQUIRED[case_id])
    assert met == want, f"{case_id}: classes met and not required {sorted(met - want)}, required and not met {sorted(want - met)}"
    could = E.reachable_on(layers, E.forms_table()[(mode, cfg)], mode=mode)
    unexplained = sorted(could - want - set(E.omitted(case_id)))
    assert not unexplained, f"{case_id}: classes the box reaches on {layers} that REQUIRED omits without a reason: {unexplained}"


def check_wide(mode, tile, run):
    met = E.frame_wide_classes(run.variants, tile)
    print(f"{mode} F{tile}: met whatever the form: {' '.join(sorted(met))}")
    log_line(kind="wide", mode=mode, tile=tile, met=sorted(met))
    assert (mode, tile) in E.REQUIRED_WIDE, f"no entry in edge_cover.REQUIRED_WIDE; met {sorted(met)}"
    want = set(E.REQUIRED_WIDE[(mode, tile)])
    assert met == want, f"{mode} F{tile}: met and not required {sorted(met - want)}, required and not met {sorted(want - met)}"


def all_of(checks):
    """every check runs, whatever the ones before it found"""
    found = []
    for check in checks:
        try:
            check()
        except AssertionError as e:
            found.append(str(e))
    assert not found, "\n".join(found)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("size", SIZES, ids=[F.tag(s) for s in SIZES])
@pytest.mark.parametrize("mode,tile", BASELINES, ids=[f"{m}-F{t}" for m, t in BASELINES])
def test_baseline_every_layer_alone(shared, oracle, mode, tile, size):
    not_after_a_bad_end()
    run = shared.baseline(mode, tile)
    if mode == "i8":
        grade_quant_size(run, size, shared, oracle)
    else:
        grade_float_size(run, mode, size, shared, oracle, f"{mode} F{tile}")


@gpu
@pytest.mark.parametrize("mode,tile", BASELINES, ids=[f"{m}-F{t}" for m, t in BASELINES])
def test_baseline_met_its_frame_wide_classes(shared, mode, tile):
    not_after_a_bad_end()
    check_wide(mode, tile, shared.baseline(mode, tile))


@gpu
@pytest.mark.parametrize("mode,cfg,plain", F.cases(), ids=[f"{m}-cfg{k}{'-plain' if p else ''}" for m, k, p in F.cases()])
def test_forced_form_at_the_cover_sizes(shared, mode, cfg, plain):
    not_after_a_bad_end()
    case_id = f"{mode}-cfg{cfg}{'-plain' if plain else ''}"
    is_base = cfg == 0 and not plain
    base = shared.baseline_digests(mode, 0)
    run = shared.baseline(mode, 0) if is_base else shared.child(case_id, mode, cfg, plain)
    try:
        checks = [lambda: check_met(case_id, mode, cfg, plain, run)] + ([] if is_base else [lambda: check_digests(base, run, case_id)])
        all_of(checks)
    finally:
        if not is_base:
            run.discard()


@gpu
@pytest.mark.parametrize("case", EDGE_SUBFORMS, ids=[c.id for c in EDGE_SUBFORMS])
def test_subform_at_the_cover_sizes(shared, oracle, case):
    not_after_a_bad_end()
    case_id = "sub:" + case.id
    base = shared.baseline_digests(case.mode, case.tile)
    graded = case.compare != "bytes"
    run = shared.child(case.id, case.mode, case.cfg, env=case.env, tile=case.tile, keep=graded)
    try:
        # the variant words of the case, at THESE sizes: the words it excludes appear on no record; the words it must see are
        # printed with their layers (which of them a map this small reaches is part of REQUIRED through met_classes)
        seen = {w for recs in run.variants.values() for _, _, v in recs for w in filter(None, v.split(","))}
        print(f"{case_id}: variant words seen {sorted(seen)}")
        assert not seen & set(case.never), (case_id, sorted(seen & set(case.never)))
        assert seen & case.words() or not case.words(), (case_id, sorted(seen))
        checks = [lambda: check_met(case_id, case.mode, case.cfg, False, run)]
        if case.compare == "bytes":
            checks.append(lambda: check_digests(base, run, case_id))
        else:
            if case.compare == "stem":
                checks.append(lambda: check_digests(base, run, case_id, prefixes=("L/",)))
            checks += [lambda size=size: grade_float_size(run, case.mode, size, shared, oracle, case.id) for size in SIZES]
        all_of(checks)
    finally:
        run.discard()
