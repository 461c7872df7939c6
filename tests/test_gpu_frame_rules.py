"""What the six fused frame entry points -- ``infur_frame_advance``, ``infur_frame_segments``, ``infur_frame_regions`` and their
``_dev`` forms -- agree on: one table of faults -> status code, the scaled dimensions they report, the no-model rule (the Scale
stage still runs), the order of the profile records, and that a failing call leaves the context usable.

Two rows are not uniform over the six, and are pinned per entry point as they are:
  * all outputs NULL: ``infur_frame_advance`` (host pointers) decodes into its own staging and answers OK; the five others
    answer E_INVALID_ARG;
  * ``infur_frame_regions_dev`` checks its own outputs and the label capacity BEFORE it delegates to the Segments call, so for
    those two faults ``*ow, *oh`` are not written."""
import ctypes as C

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd

pytestmark = pytest.mark.gpu

H, WID = 48, 64
NPIX = H * WID
ROWS = 64
UNSET = 0xDEAD  # what *ow, *oh hold before every call
ENTRIES = ("advance", "advance_dev", "segments", "segments_dev", "regions", "regions_dev")
CAPS = {"advance": ("mask",), "segments": ("plane", "mask"), "regions": ("plane", "labels")}
VALID = dict(factor=1.0, mode=0, frame=True, w=WID, outs=True, short=None, scaled=False)

# fault -> (changes to VALID, code, message of infur_last_error or None where the code is returned without one,
#           are *ow, *oh written: by the host-pointer calls, by the _dev calls)
FAULTS = {
    "negative factor": (dict(factor=-1.0), _lib.E_INVALID_SCALE, "Cannot scale by negative number", False, False),
    "unknown scale mode": (dict(mode=2), _lib.E_INVALID_ARG, "unknown scale mode 2", True, False),
    "null frame": (dict(frame=False), _lib.E_INVALID_ARG, None, True, True),
    "zero width": (dict(w=0), _lib.E_SHAPE, "couldn't transform image: 0x48", True, True),
    "plane one byte short": (dict(short="plane"), _lib.E_CAPACITY, "a plane needs 3072 bytes, buffer has 3071", True, True),
    "mask one byte short": (dict(short="mask"), _lib.E_CAPACITY, "mask needs 12288 bytes, buffer has 12287", True, True),
    "labels one byte short": (dict(short="labels"), _lib.E_CAPACITY, "the label plane needs 12288 bytes, buffer has 12287", True, True),
    "all outputs null": (dict(outs=False), _lib.E_INVALID_ARG, None, True, True),
}
# the rows that are not uniform (module docstring): (fault, entry) -> (code, message, dims written)
EXCEPTIONS = {
    ("all outputs null", "advance"): (_lib.OK, None, True),
    ("all outputs null", "regions_dev"): (_lib.E_INVALID_ARG, None, False),
    ("labels one byte short", "regions_dev"): (_lib.E_CAPACITY, "the label plane needs 12288 bytes, buffer has 12287", False),
}


class Bufs:
    """the frame and every output of the six calls: numpy arrays for the host-pointer calls, device buffers for the _dev ones"""

    SIZES = {"frame": NPIX * 3, "mask": NPIX * 4, "klass": NPIX, "conf": NPIX, "stats": 21 * 64, "labels": NPIX * 4,
             "table": ROWS * _lib.REGION_WORDS * 8, "n": 4, "scaled": NPIX * 3}

    def __init__(self, ctx, frame):
        self.ctx = ctx
        self.host = {name: np.zeros(n, np.uint8) for name, n in self.SIZES.items()}
        self.host["frame"][:] = frame.ravel()
        self.dev = {}
        for name, n in self.SIZES.items():
            d = C.c_void_p(None)
            ctx.check(ctx.L.infur_dev_alloc(ctx.h, n, C.byref(d)))
            self.dev[name] = d
        ctx.check(ctx.L.infur_memcpy_h2d(ctx.h, self.dev["frame"], frame.ctypes.data, frame.nbytes))

    def ptr(self, name, dev):
        return self.dev[name] if dev else self.host[name].ctypes.data

    def read(self, name, dev, n):
        if not dev:
            return self.host[name][:n].copy()
        out = np.empty(n, np.uint8)
        self.ctx.synchronize()
        self.ctx.check(self.ctx.L.infur_memcpy_d2h(self.ctx.h, out.ctypes.data, self.dev[name], n))
        return out

    def free(self):
        for d in self.dev.values():
            self.ctx.check(self.ctx.L.infur_dev_free(self.ctx.h, d))


def invoke(b, entry, k, ow, oh, **changes):
    s = dict(VALID, **changes)
    dev = entry.endswith("_dev")
    kind = entry.split("_")[0]
    L, h = b.ctx.L, b.ctx.h
    out = lambda name: b.ptr(name, dev) if s["outs"] else None  # noqa: E731
    cap = lambda name, full: full - (1 if s["short"] == name else 0)  # noqa: E731
    head = (h, b.ptr("frame", dev) if s["frame"] else None, s["w"], H, s["factor"], s["mode"])
    tail = (b.ptr("scaled", dev) if s["scaled"] else None, C.byref(ow), C.byref(oh))
    ow.value = oh.value = UNSET
    if kind == "advance":
        return getattr(L, "infur_frame_" + entry)(*head, out("mask"), cap("mask", NPIX * 4), *tail)
    if kind == "segments":
        return getattr(L, "infur_frame_" + entry)(*head, _lib.DECODE_RAW, out("klass"), out("conf"), cap("plane", NPIX), out("stats"), k,
                                                  out("mask"), cap("mask", NPIX * 4), *tail)
    return getattr(L, "infur_frame_" + entry)(*head, _lib.DECODE_RAW, _lib.CONNECT_8, 0, 0, out("klass"), out("conf"), cap("plane", NPIX),
                                              out("labels"), cap("labels", NPIX * 4), out("table"), ROWS, out("n"), *tail)


@pytest.fixture(scope="module")
def frame():
    return W.synth_frame(H, WID, index=1)


def test_fault_table_over_the_six_entry_points(ctx, model, frame):
    """every fault answers its code on every entry point that has the argument, with the message of the check that found it;
    *ow, *oh hold the scaled dimensions whenever the call got past infur_scale_out_dims; and the next valid call on the same
    context is OK"""
    k = model.get_info().num_classes
    assert k * 64 <= Bufs.SIZES["stats"]
    b = Bufs(ctx, frame)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    bad = []
    for entry in ENTRIES:
        assert invoke(b, entry, k, ow, oh) == _lib.OK and (ow.value, oh.value) == (WID, H), entry
        for name, (changes, code, msg, dims_host, dims_dev) in FAULTS.items():
            if changes.get("short") and changes["short"] not in CAPS[entry.split("_")[0]]:
                continue  # (the entry point has no such capacity)
            dims = dims_dev if entry.endswith("_dev") else dims_host
            code, msg, dims = EXCEPTIONS.get((name, entry), (code, msg, dims))
            rc = invoke(b, entry, k, ow, oh, **changes)
            got = (rc, (ow.value, oh.value), ctx.last_error())
            print(f"{entry:13s} {name:22s} rc {rc:3d}  ow x oh {ow.value} x {oh.value}  last_error {got[2]!r}")
            want_dims = (changes.get("w", WID), H) if dims else (UNSET, UNSET)
            if rc != code or got[1] != want_dims or (msg is not None and got[2] != msg) or (rc != _lib.OK and msg is not None and not got[2]):
                bad.append((entry, name, got, (code, want_dims, msg)))
            # the context is not poisoned
            if invoke(b, entry, k, ow, oh) != _lib.OK or (ow.value, oh.value) != (WID, H):
                bad.append((entry, name, "the next valid call failed", ctx.last_error()))
    b.free()
    assert not bad, bad


def test_no_model_rule_over_the_six_entry_points(frame, blob50, oracle):
    """no model: E_MODEL_NOT_LOADED from all six, after the Scale stage has run -- the scaled frame is written, the same bytes on
    every path; loading a model afterwards makes the same context answer OK"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    with Context(device=0) as c:
        b = Bufs(c, frame)
        scaled = {}
        for entry in ENTRIES:
            dev = entry.endswith("_dev")
            assert invoke(b, entry, 21, ow, oh) == _lib.E_MODEL_NOT_LOADED, entry
            assert (ow.value, oh.value) == (WID, H) and c.last_error() == "no model loaded", entry
            for name in ("scaled", "mask", "klass", "labels"):
                b.host[name][:] = 0xA5
                c.check(c.L.infur_memcpy_h2d(c.h, b.dev[name], b.host[name].ctypes.data, b.SIZES[name]))
            assert invoke(b, entry, 21, ow, oh, factor=0.5, scaled=True) == _lib.E_MODEL_NOT_LOADED, entry
            assert (ow.value, oh.value) == (WID // 2, H // 2) and c.last_error() == "no model loaded", entry
            scaled[entry] = b.read("scaled", dev, NPIX // 4 * 3)
            for name in ("mask", "klass", "labels"):  # nothing else is produced
                assert (b.read(name, dev, b.SIZES[name]) == 0xA5).all(), (entry, name)
        rc, ref = oracle.scale(frame, 0.5, 0)
        assert rc == 0
        for entry in ENTRIES:
            assert (scaled[entry] == ref.ravel()).all(), entry
        Model(c).control(ModelCmd.LoadBlob(blob50))
        for entry in ENTRIES:
            assert invoke(b, entry, 21, ow, oh, factor=0.5, scaled=True) == _lib.OK and (ow.value, oh.value) == (WID // 2, H // 2), entry
            assert (b.read("scaled", entry.endswith("_dev"), NPIX // 4 * 3) == ref.ravel()).all(), entry
        b.free()


def test_profile_records_keep_their_order(frame, blob50):
    """the scale records first, the decode kernel last; Regions' record follows the one Segments record"""
    with Context(device=0, profile=True) as c:
        Model(c).control(ModelCmd.LoadBlob(blob50))
        fp = FramePath(c)
        fp.advance(frame, 0.5)
        kernels = [r["kernel"] for r in c.profile()]
        assert kernels[0].startswith("scale") and kernels[-1] == "upsample_argmax_shade" and kernels.count("upsample_argmax_shade") == 1
        assert sum(kn.startswith("scale") for kn in kernels) == 1
        fp.advance_regions(frame, 0.5)
        kernels = [r["kernel"] for r in c.profile()]
        assert kernels[0].startswith("scale") and kernels.count("upsample_argmax_segments") == 1
        assert kernels[-2:] == ["upsample_argmax_segments", "regions"] and "upsample_argmax_shade" not in kernels
