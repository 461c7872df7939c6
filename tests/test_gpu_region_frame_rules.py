"""What the eighteen fused frame entry points behind Regions -- ``infur_frame_{regions,tracks,anchors,sieve,shapes,split,skeleton,
centrelines,expand}`` and their ``_dev`` forms -- agree on, one table over all of them:

  * with every output wanted the host-pointer form and the ``_dev`` form write identical bytes, and both equal the chain of the
    separate ``_dev`` stage calls on the same decoded plane (``infur_frame_regions_dev``, then ``infur_anchors_dev`` and so on);
  * for a list of output subsets every unwanted buffer keeps its poison and every wanted one holds the bytes of the full call;
  * one table of faults -> status code, ``infur_last_error`` text, whether ``*ow, *oh`` were written, and the next valid call is OK;
  * without a model: E_MODEL_NOT_LOADED, the scaled frame written, nothing else touched, whatever a stage's own capacities are.

The frames: 48 x 64 at 1.0 and at 0.5, and 61 x 97 (5917 pixels: neither npix nor 4 npix is a multiple of the staging alignment, so
two slots of a wrong staging layout overlap).  Region tables of 64 rows and of 1 row (fewer rows than regions).

Rows that are not uniform over the eighteen are pinned per entry point as they are (EXCEPTIONS):
  * ``infur_frame_centrelines`` (host pointers) has no connectivity / flags check of its own: the one of the calls below it answers,
    after the dimensions were written;
  * ``infur_frame_sieve_dev`` checks ``klass_out`` against ``plane_cap`` itself, before it delegates: no dimensions;
  * ``infur_frame_tracks`` rejects "no tracker output wanted" before it looks at the frame: no dimensions."""
import ctypes as C

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context

pytestmark = pytest.mark.gpu

STAGES = ("regions", "tracks", "anchors", "sieve", "shapes", "split", "skeleton", "centrelines", "expand")
UNSET = 0xDEAD  # what *ow, *oh hold before every call
POISON = 0xA5
ROWS = 64  # the larger region table; the buffers are sized for it
MIN_PIXELS, FLAGS, CONN = 4, _lib.REGIONS_SKIP_BACKGROUND, _lib.CONNECT_8
LOOP_ROWS, VERTEX_ROWS, SHAPE_ROWS = 128, 2048, 128  # Shapes
SPLIT_ROWS, SPLIT_CORE = 128, 4
SKEL_ROWS, RECORD_ROWS, CL_VERTEX_ROWS = 64, 128, 2048
EXPAND_ROWS, REACH = 64, 3
NP_MAX = 61 * 97


class Frame:
    def __init__(self, h, w, factor, index):
        self.h, self.w, self.factor = h, w, factor
        self.oh, self.ow = (h, w) if factor == 1.0 else (int(h * factor), int(w * factor))
        self.npix = self.oh * self.ow
        self.pixels = W.synth_frame(h, w, index=index)


FRAMES = {"48x64": lambda: Frame(48, 64, 1.0, 1), "48x64 at 0.5": lambda: Frame(48, 64, 0.5, 1), "61x97": lambda: Frame(61, 97, 1.0, 2)}

REG_OUT = ("klass", "conf", "labels", "table", "n")
ANCH_OUT = ("dist2", "anchors")
SKEL_OUT = ANCH_OUT + ("kind", "skel_table", "skel_counts")
# the outputs of a stage behind Regions' own
OWN = {
    "regions": (),
    "tracks": ("tor", "tplane", "ttab", "summary"),
    "anchors": ANCH_OUT,
    "sieve": ("klass_out", "scounts"),
    "shapes": ("loops_out", "vertices_out", "shapes", "values", "counts_out"),
    "split": ANCH_OUT + ("split_labels", "split_table", "split_counts"),
    "skeleton": SKEL_OUT,
    "centrelines": SKEL_OUT + ("records", "vertices", "cl_counts"),
    "expand": ("grown", "dist2", "source", "etable", "ecounts"),
}
SIZES = {
    "frame": NP_MAX * 3, "scaled": NP_MAX * 3, "klass": NP_MAX, "conf": NP_MAX, "labels": NP_MAX * 4, "table": ROWS * _lib.REGION_WORDS * 8, "n": 4,
    "tor": ROWS * 4, "tplane": NP_MAX * 4, "ttab": ROWS * _lib.TRACK_WORDS * 8, "summary": _lib.TRACKS_SUMMARY_WORDS * 4,
    "dist2": NP_MAX * 4, "anchors": ROWS * _lib.ANCHOR_WORDS * 4,
    "klass_out": NP_MAX, "scounts": _lib.SIEVE_COUNT_WORDS * 4,
    "loops_out": LOOP_ROWS * 16, "vertices_out": VERTEX_ROWS * 4, "shapes": SHAPE_ROWS * _lib.SHAPE_WORDS * 8, "values": ROWS * _lib.SHAPE_WORDS * 8,
    "counts_out": _lib.SHAPES_COUNT_WORDS * 4,
    "split_labels": NP_MAX * 4, "split_table": SPLIT_ROWS * _lib.SPLIT_WORDS * 4, "split_counts": _lib.SPLIT_COUNT_WORDS * 4,
    "kind": NP_MAX, "skel_table": SKEL_ROWS * _lib.SKELETON_WORDS * 4, "skel_counts": _lib.SKELETON_COUNT_WORDS * 4,
    "records": RECORD_ROWS * _lib.CENTRELINE_WORDS * 4, "vertices": CL_VERTEX_ROWS * 4, "cl_counts": _lib.CENTRELINES_COUNT_WORDS * 4,
    "grown": NP_MAX * 4, "source": NP_MAX * 4, "etable": EXPAND_ROWS * _lib.EXPAND_WORDS * 4, "ecounts": _lib.EXPAND_COUNT_WORDS * 4,
}
# what only the chain of separate calls needs: Sieve's first Regions pass, Outlines in front of Shapes
SCRATCH = {"s_labels": NP_MAX * 4, "s_table": NP_MAX * _lib.REGION_WORDS * 8, "s_n": 4, "s_loops": NP_MAX * 16, "s_vertices": NP_MAX * 16, "s_counts": 64}
OUTPUTS = tuple(k for k in SIZES if k not in ("frame", "scaled"))


class Bufs:
    """the frame and every output of the eighteen calls: numpy arrays for the host-pointer calls ("host"), device buffers for the
    _dev ones ("dev"), a second set of device buffers for the chain of separate calls ("ref")"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.host = {name: np.zeros(n, np.uint8) for name, n in SIZES.items()}
        self.dev, self.ref = {}, {}
        for name, n in list(SIZES.items()) + list(SCRATCH.items()):
            for where in (self.dev, self.ref):
                if name in SCRATCH and where is self.dev:
                    continue
                d = C.c_void_p(None)
                ctx.check(ctx.L.infur_dev_alloc(ctx.h, n, C.byref(d)))
                where[name] = d
        self.fill = np.full(max(SIZES.values()), POISON, np.uint8)

    def set_frame(self, fr):
        flat = fr.pixels.ravel()
        self.host["frame"][: flat.size] = flat
        for where in (self.dev, self.ref):
            self.ctx.check(self.ctx.L.infur_memcpy_h2d(self.ctx.h, where["frame"], self.host["frame"].ctypes.data, flat.size))

    def poison(self):
        self.ctx.synchronize()
        for name in OUTPUTS + ("scaled",):
            self.host[name][:] = POISON
            for where in (self.dev, self.ref):
                self.ctx.check(self.ctx.L.infur_memcpy_h2d(self.ctx.h, where[name], self.fill.ctypes.data, SIZES[name]))

    def ptr(self, name, where):
        return self.host[name].ctypes.data if where == "host" else getattr(self, where)[name]

    def read(self, name, where):
        if where == "host":
            return self.host[name].copy()
        out = np.empty(SIZES[name], np.uint8)
        self.ctx.synchronize()
        self.ctx.check(self.ctx.L.infur_memcpy_d2h(self.ctx.h, out.ctypes.data, getattr(self, where)[name], SIZES[name]))
        return out

    def free(self):
        self.ctx.synchronize()
        for where in (self.dev, self.ref):
            for d in where.values():
                self.ctx.check(self.ctx.L.infur_dev_free(self.ctx.h, d))


@pytest.fixture(scope="module")
def bufs(ctx, model):
    b = Bufs(ctx)
    yield b
    b.free()


@pytest.fixture(scope="module")
def frames():
    return {name: make() for name, make in FRAMES.items()}


class FreshTracker:
    """a tracker that has seen no frame, for the one call made inside the block (the frame counter behind TRACK_BORN survives
    infur_tracker_reset, so equal bytes want equal histories); None for the stages that take none"""

    def __init__(self, ctx, stage):
        self.ctx, self.t = ctx, C.c_void_p(None) if stage == "tracks" else None

    def __enter__(self):
        if self.t is not None:
            self.ctx.check(self.ctx.L.infur_tracker_create(self.ctx.h, 0, 0, C.byref(self.t)))
        return self.t

    def __exit__(self, *exc):
        if self.t is not None:
            self.ctx.L.infur_tracker_destroy(self.t)  # (synchronises the context's stream first)


VALID = dict(mode=0, frame=True, w=None, factor=None, conn=CONN, flags=FLAGS, short=None, scaled=False)


def tail_args(stage, p, cap, npix, rows, trk):
    """the arguments behind oh: p(name) the pointer or None, cap(name, full) the capacity"""
    anch = (p("dist2"), cap("dist2", npix * 4), p("anchors"))
    skel = anch + (0, p("kind"), cap("kind", npix), p("skel_table"), SKEL_ROWS, p("skel_counts"))
    return {
        "regions": (),
        "tracks": (trk, 1, p("tor"), p("tplane"), p("ttab"), p("summary")),
        "anchors": anch,
        "sieve": (0, 0, p("klass_out"), p("scounts")),
        "shapes": (0, p("loops_out"), LOOP_ROWS, p("vertices_out"), VERTEX_ROWS, p("shapes"), SHAPE_ROWS, p("values"), p("counts_out")),
        "split": anch + (SPLIT_CORE, 0, p("split_labels"), cap("split_labels", npix * 4), p("split_table"), SPLIT_ROWS, p("split_counts")),
        "skeleton": skel,
        "centrelines": skel + (_lib.CENTRELINES_CORNERS, 0, p("records"), RECORD_ROWS, p("vertices"), CL_VERTEX_ROWS, p("cl_counts")),
        "expand": (REACH, p("grown"), cap("grown", npix * 4), p("dist2"), cap("dist2", npix * 4), p("source"), cap("source", npix * 4), p("etable"),
                   EXPAND_ROWS, p("ecounts")),
    }[stage]


def invoke(b, stage, where, fr, rows, want, ow, oh, **changes):
    """one fused call of `stage`: where = "host" for the host-pointer form, "dev" / "ref" for the _dev form on that buffer set"""
    s = dict(VALID, **changes)
    L, h = b.ctx.L, b.ctx.h
    p = lambda name: b.ptr(name, where) if name in want else None  # noqa: E731
    cap = lambda name, full: full - (1 if s["short"] == name else 0)  # noqa: E731
    head = (h, b.ptr("frame", where) if s["frame"] else None, fr.w if s["w"] is None else s["w"], fr.h, fr.factor if s["factor"] is None else s["factor"],
            s["mode"], _lib.DECODE_RAW, s["conn"], MIN_PIXELS, s["flags"], p("klass"), p("conf"), cap("plane", fr.npix), p("labels"),
            cap("labels", fr.npix * 4), p("table"), rows, p("n"), b.ptr("scaled", where) if s["scaled"] else None, C.byref(ow), C.byref(oh))
    ow.value = oh.value = UNSET
    fn = getattr(L, "infur_frame_" + stage + ("" if where == "host" else "_dev"))
    with FreshTracker(b.ctx, stage) as trk:
        return fn(*head, *tail_args(stage, p, cap, fr.npix, rows, trk))


def chain(b, stage, fr, rows, ow, oh):
    """the separate _dev calls on the "ref" buffers that the fused call of `stage` stands for, every output wanted"""
    L, h, r, ck = b.ctx.L, b.ctx.h, b.ref, b.ctx.check
    H, Wd, NONE = fr.oh, fr.ow, _lib.REGION_NONE
    head = (h, r["frame"], fr.w, fr.h, fr.factor, 0, _lib.DECODE_RAW, CONN)
    if stage == "sieve":  # Regions of the plane as decoded, everything; Sieve; Regions of the cleaned plane
        rows1 = min(fr.npix, 1 << 20)
        ck(L.infur_frame_regions_dev(*head, 0, 0, r["klass"], r["conf"], fr.npix, r["s_labels"], fr.npix * 4, r["s_table"], rows1, r["s_n"], None,
                                     C.byref(ow), C.byref(oh)))
        ck(L.infur_sieve_dev(h, r["klass"], r["s_labels"], r["s_table"], rows1, r["s_n"], H, Wd, MIN_PIXELS, 0, 0, r["klass_out"], None, r["scounts"]))
        ck(L.infur_regions_dev(h, r["klass_out"], r["conf"], H, Wd, CONN, 0, FLAGS, r["labels"], r["table"], rows, r["n"]))
        return
    ck(L.infur_frame_regions_dev(*head, MIN_PIXELS, FLAGS, r["klass"], r["conf"], fr.npix, r["labels"], fr.npix * 4, r["table"], rows, r["n"], None,
                                 C.byref(ow), C.byref(oh)))
    if stage == "tracks":
        with FreshTracker(b.ctx, stage) as trk:
            ck(L.infur_tracks_dev(trk, r["labels"], r["table"], rows, r["n"], H, Wd, 1, r["tor"], r["tplane"], r["ttab"], r["summary"]))
    if stage == "shapes":
        ck(L.infur_outlines_dev(h, r["labels"], 4, H, Wd, _lib.OUTLINES_SKIP | _lib.OUTLINES_CONN8, NONE, 0, r["s_loops"], fr.npix, r["s_vertices"],
                                fr.npix * 4, r["s_counts"]))
        ck(L.infur_shapes_dev(h, r["s_loops"], fr.npix, r["s_vertices"], fr.npix * 4, r["s_counts"], H, Wd, r["loops_out"], LOOP_ROWS, r["vertices_out"],
                              VERTEX_ROWS, r["shapes"], SHAPE_ROWS, r["values"], rows, r["counts_out"]))
    if stage == "expand":
        ck(L.infur_expand_dev(h, r["labels"], 4, H, Wd, 0, NONE, REACH, r["grown"], r["dist2"], r["source"], r["etable"], EXPAND_ROWS, r["ecounts"]))
    if stage in ("anchors", "split", "skeleton", "centrelines"):
        ck(L.infur_anchors_dev(h, r["labels"], 4, H, Wd, _lib.ANCHORS_SKIP, NONE, r["dist2"], r["anchors"], rows))
    if stage == "split":
        ck(L.infur_split_dev(h, r["labels"], 4, r["dist2"], H, Wd, _lib.SPLIT_SKIP, NONE, SPLIT_CORE, 0, r["split_labels"], r["split_table"], SPLIT_ROWS,
                             r["split_counts"]))
    if stage in ("skeleton", "centrelines"):
        ck(L.infur_skeleton_dev(h, r["labels"], 4, r["dist2"], H, Wd, _lib.SKELETON_SKIP, NONE, 0, r["kind"], r["skel_table"], SKEL_ROWS, r["skel_counts"]))
    if stage == "centrelines":
        ck(L.infur_centrelines_dev(h, r["labels"], 4, r["kind"], r["dist2"], H, Wd, _lib.CENTRELINES_CORNERS | _lib.CENTRELINES_SKIP, NONE, 0, r["records"],
                                   RECORD_ROWS, r["vertices"], CL_VERTEX_ROWS, r["cl_counts"]))


def outputs(stage):
    return REG_OUT + OWN[stage]


def diff(a, b_):
    bad = np.flatnonzero(a != b_)
    return f"{bad.size} bytes differ, the first at {bad[0]}: {a[bad[0]]:#x} and {b_[bad[0]]:#x}" if bad.size else ""


@pytest.mark.parametrize("stage", STAGES)
def test_full_outputs_host_dev_and_the_chain_of_separate_calls_agree(ctx, model, bufs, frames, stage):
    """every output wanted: the host-pointer form, the _dev form and the chain of the separate _dev calls write the same bytes, on
    every frame and with a region table of 64 rows and of 1; the table's rows beyond n keep their poison"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    bad = []
    for fname, fr in frames.items():
        bufs.set_frame(fr)
        for rows in (ROWS, 1):
            bufs.poison()
            want = set(outputs(stage))
            for where in ("host", "dev"):
                rc = invoke(bufs, stage, where, fr, rows, want, ow, oh)
                assert rc == _lib.OK and (ow.value, oh.value) == (fr.ow, fr.oh), (stage, where, fname, rows, rc, ctx.last_error())
            chain(bufs, stage, fr, rows, ow, oh)
            assert (ow.value, oh.value) == (fr.ow, fr.oh)
            got = {where: {name: bufs.read(name, where) for name in outputs(stage)} for where in ("host", "dev", "ref")}
            n = int(got["dev"]["n"].view(np.uint32)[0])
            print(f"{stage:11s} {fname:12s} rows {rows:2d}: {n} regions")
            assert n > 1, "the frame has fewer regions than the test wants"
            for name in outputs(stage):
                for where in ("host", "ref"):
                    d = diff(got[where][name], got["dev"][name])
                    if d:
                        bad.append((fname, rows, name, where + " against dev", d))
            for where in ("host", "dev"):
                beyond = got[where]["table"][min(n, rows) * _lib.REGION_WORDS * 8:]
                if not (beyond == POISON).all():
                    bad.append((fname, rows, "table", where, "rows beyond n were written"))
            if not (got["dev"]["labels"][: fr.npix * 4] != POISON).any() or not (got["dev"]["klass"][fr.npix:] == POISON).all():
                bad.append((fname, rows, "labels / klass", "dev", "not written, or written beyond the plane"))
    assert not bad, bad


def subsets(stage):
    own = OWN[stage]
    full = set(outputs(stage))
    return [full] + [{name} for name in own] + [set(REG_OUT), {"labels", "n"}, {"table"}]


@pytest.mark.parametrize("stage", STAGES)
def test_output_subsets_leave_every_unwanted_buffer_alone(ctx, model, bufs, frames, stage):
    """on the 61 x 97 frame: whatever subset of the outputs is wanted, the unwanted buffers keep their poison and the wanted ones
    hold what the call with every output wrote.  (Tracks answers E_INVALID_ARG where none of the tracker's outputs is wanted, and
    touches nothing.)"""
    fr = frames["61x97"]
    bufs.set_frame(fr)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    bad = []
    for rows in (ROWS, 1):
        full = {}
        for want in subsets(stage):
            bufs.poison()
            refused = stage == "tracks" and not (want & set(OWN["tracks"]))
            for where in ("host", "dev"):
                rc = invoke(bufs, stage, where, fr, rows, want, ow, oh)
                if rc != (_lib.E_INVALID_ARG if refused else _lib.OK):
                    bad.append((rows, sorted(want), where, "rc", rc, ctx.last_error()))
                    continue
                for name in OUTPUTS:
                    got = bufs.read(name, where)
                    if name not in want or refused:
                        if not (got == POISON).all():
                            bad.append((rows, sorted(want), where, name, "unwanted and written"))
                    elif (where, name) not in full:
                        full[(where, name)] = got  # (the first subset is everything)
                    else:
                        d = diff(got, full[(where, name)])
                        if d:
                            bad.append((rows, sorted(want), where, name, d))
    assert not bad, bad


NOUN = {"dist2": "distance", "split_labels": "segment", "kind": "kind", "grown": "grown", "source": "source"}
OWN_PLANES = {"anchors": ("dist2",), "split": ("dist2", "split_labels"), "skeleton": ("dist2", "kind"), "centrelines": ("dist2", "kind"),
              "expand": ("grown", "dist2", "source")}


def faults(stage, npix, h):
    """fault -> (changes to VALID, code, message of infur_last_error or None where the code is returned without one,
                 are *ow, *oh written: by the host-pointer call, by the _dev call)"""
    t = {
        "negative factor": (dict(factor=-1.0), _lib.E_INVALID_SCALE, "Cannot scale by negative number", False, False),
        "unknown scale mode": (dict(mode=2), _lib.E_INVALID_ARG, "unknown scale mode 2", True, False),
        "null frame": (dict(frame=False), _lib.E_INVALID_ARG, None, True, True),
        "zero width": (dict(w=0), _lib.E_SHAPE, f"couldn't transform image: 0x{h}", True, True),
        "connectivity 5": (dict(conn=5), _lib.E_INVALID_ARG, "connectivity 5: 4 or 8", False, False),
        "regions flags 2": (dict(flags=2), _lib.E_INVALID_ARG, "unknown regions flags 0x2", False, False),
        "plane one byte short": (dict(short="plane"), _lib.E_CAPACITY, f"a plane needs {npix} bytes, buffer has {npix - 1}", True, True),
        "labels one byte short": (dict(short="labels"), _lib.E_CAPACITY, f"the label plane needs {npix * 4} bytes, buffer has {npix * 4 - 1}", True, False),
        "all outputs null": (dict(outs=False), _lib.E_INVALID_ARG, None, True, False),
    }
    for name in OWN_PLANES.get(stage, ()):
        need = npix if name == "kind" else npix * 4
        t[name + " one byte short"] = (dict(short=name), _lib.E_CAPACITY, f"the {NOUN[name]} plane needs {need} bytes, buffer has {need - 1}", True, False)
    return t


# the rows that are not uniform (module docstring): (fault, entry) -> are *ow, *oh written
EXCEPTIONS = {
    ("connectivity 5", "centrelines"): True,
    ("regions flags 2", "centrelines"): True,
    ("plane one byte short", "sieve_dev"): False,
    ("all outputs null", "tracks"): False,
}


@pytest.mark.parametrize("stage", STAGES)
def test_fault_table(ctx, model, bufs, frames, stage):
    """every fault answers its code on both forms, with the message of the check that found it; *ow, *oh hold the scaled dimensions
    exactly where the call got past infur_scale_out_dims before the check; and the next valid call on the same context is OK"""
    fr = frames["48x64"]
    bufs.set_frame(fr)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    everything = set(outputs(stage))
    bad = []
    for where in ("host", "dev"):
        entry = stage + ("" if where == "host" else "_dev")
        assert invoke(bufs, stage, where, fr, ROWS, everything, ow, oh) == _lib.OK and (ow.value, oh.value) == (fr.ow, fr.oh), entry
        for name, (changes, code, msg, dims_host, dims_dev) in faults(stage, fr.npix, fr.h).items():
            dims = EXCEPTIONS.get((name, entry), dims_dev if where == "dev" else dims_host)
            changes = dict(changes)
            want = everything if changes.pop("outs", True) else set()
            rc = invoke(bufs, stage, where, fr, ROWS, want, ow, oh, **changes)
            got = (rc, (ow.value, oh.value), ctx.last_error())
            print(f"{entry:16s} {name:28s} rc {rc:3d}  ow x oh {ow.value} x {oh.value}  last_error {got[2]!r}")
            want_dims = (changes.get("w", fr.ow), fr.oh) if dims else (UNSET, UNSET)
            if rc != code or got[1] != want_dims or (msg is not None and got[2] != msg):
                bad.append((entry, name, got, (code, want_dims, msg)))
            # the context is not poisoned
            if invoke(bufs, stage, where, fr, ROWS, everything, ow, oh) != _lib.OK or (ow.value, oh.value) != (fr.ow, fr.oh):
                bad.append((entry, name, "the next valid call failed", ctx.last_error()))
    assert not bad, bad


def test_no_model_rule(frames):
    """no model: E_MODEL_NOT_LOADED from all eighteen, after the Scale stage has run -- the scaled frame is written, the bytes
    infur_frame_regions writes; nothing else is touched; and a stage's own plane that is too short does not change the answer"""
    fr = frames["48x64 at 0.5"]
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    bad = []
    with Context(device=0) as c:
        b = Bufs(c)
        b.set_frame(fr)
        ref = None
        for stage in STAGES:
            for where in ("host", "dev"):
                entry = stage + ("" if where == "host" else "_dev")
                for short in (None,) + OWN_PLANES.get(stage, ()):
                    b.poison()
                    rc = invoke(b, stage, where, fr, ROWS, set(outputs(stage)), ow, oh, scaled=True, short=short)
                    if rc != _lib.E_MODEL_NOT_LOADED or (ow.value, oh.value) != (fr.ow, fr.oh) or c.last_error() != "no model loaded":
                        bad.append((entry, short, rc, (ow.value, oh.value), c.last_error()))
                        continue
                    scaled = b.read("scaled", where)
                    if ref is None:  # (the first entry is infur_frame_regions)
                        ref = scaled
                        assert (ref[: fr.npix * 3] != POISON).any() and (ref[fr.npix * 3:] == POISON).all()
                    if diff(scaled, ref):
                        bad.append((entry, short, "scaled", diff(scaled, ref)))
                    for name in OUTPUTS:
                        if not (b.read(name, where) == POISON).all():
                            bad.append((entry, short, name, "written without a model"))
        b.free()
    assert not bad, bad
