"""Host-side mirror of the reference's ``Processor`` plugin surface over the C ABI.

The reference defines one trait, ``Processor`` (infur/src/processing.rs:23-60), and the
per-frame path instantiates it three times: ``Scale`` (processing.rs:179-282),
``Model<f32>`` (infur/src/predict_onnx.rs:146-345) and ``ColorCode``
(infur/src/decode_predict.rs:38-84), wired together by ``ProcessingApp::advance``
(infur/src/app.rs:107-153).  The classes below keep the same names, commands, argument
meaning and error behaviour; the arithmetic happens in ``libinfur_hip.so`` (hand-written
gfx950 kernels).  There is no CPU fallback.

Rust ``&mut Output`` parameters become mutable holders: ``Slot`` for ``Option<T>``
outputs, a plain ``list`` for ``Vec<ArrayD<f32>>``.  Typed ``Result`` errors become
exceptions carrying the status code of include/infur_hip.h.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Generic, List, NamedTuple, Optional, TypeVar

import numpy as np

from . import _lib

T = TypeVar("T")

# tile configurations measured on MI355X for the BASELINE configs (scripts/tune.py writes it)
TUNE_DB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_tune_gfx950.txt")


# --------------------------------------------------------------------------- #
# errors (thiserror enums of the reference)
# --------------------------------------------------------------------------- #
class InfurError(Exception):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        self.detail = detail
        super().__init__(detail or _lib.status_string(code))


class ValidScaleError(InfurError):
    """processing.rs:145-168 -- "Cannot scale by negative number"."""


class ScaleProcError(InfurError):
    """processing.rs:201-211 -- ZeroSizeIn / ZeroSizeOut."""

    @property
    def kind(self) -> str:
        return {_lib.E_ZERO_SIZE_IN: "ZeroSizeIn", _lib.E_ZERO_SIZE_OUT: "ZeroSizeOut"}.get(self.code, "Other")


class ModelCmdError(InfurError):
    """predict_onnx.rs:41-48 -- the model could not be loaded."""


class ModelProcError(InfurError):
    """predict_onnx.rs:33-39 -- ShapeError / RuntimeError while processing."""


class Slot(Generic[T]):
    """A mutable ``Option<T>`` the callee may fill or reuse (Rust ``&mut Option<T>``)."""

    def __init__(self, value: Optional[T] = None):
        self.value = value

    def is_some(self) -> bool:
        return self.value is not None

    def take(self) -> Optional[T]:
        v, self.value = self.value, None
        return v


@dataclass
class Frame:
    """processing.rs:9-18: frame id + packed BGR image ([h, w, 3] u8, row-major, no padding)."""

    id: int
    img: np.ndarray

    def __eq__(self, other):  # PartialEq compares ids only (processing.rs:14-18)
        return isinstance(other, Frame) and self.id == other.id


def bgr_image(w: int, h: int) -> np.ndarray:
    """``BgrImage::new(w, h)``: zero-filled packed BGR."""
    return np.zeros((h, w, 3), np.uint8)


def _check_bgr(img: np.ndarray) -> np.ndarray:
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ModelProcError(_lib.E_SHAPE, f"expected packed BGR u8 [h,w,3], got {img.dtype} {img.shape}")
    return np.ascontiguousarray(img)


def _ptr(a: Optional[np.ndarray]):
    """the address of an array, NULL for None"""
    return a.ctypes.data if a is not None else None


def _ptr_some(a: Optional[np.ndarray]):
    """the address of an array that holds something, NULL for None and for an empty one"""
    return a.ctypes.data if a is not None and a.size else None


# --------------------------------------------------------------------------- #
# context
# --------------------------------------------------------------------------- #
class HlRange(NamedTuple):
    """What the splits of an "f16hl" context saw since its monitor was enabled or last read (``infur_hl_range``)."""

    act_amax: float    # largest |activation| stored in three bytes (a ReLU layer's max(x, 0)); the f32 logits are not included
    wino_amax: float   # largest |Winograd-domain input| (unscaled)
    saturated: bool    # a value was changed by the upper clamp (beyond 65520; +inf included): re-run the frame on "f32" / "f32s"
    nan_seen: bool     # a split received a NaN (stored as the layer's lower bound)


class Context:
    """One GPU + one HIP stream + device arena (``infur_ctx``).  Not thread-safe."""

    def __init__(self, device: int = 0, compute_aux: bool = True, profile: bool = False,
                 keep_activations: bool = False, stream: Optional[int] = None, dtype: str = "f32",
                 winograd_min_cin: int = 0, winograd_tile: int = 0, autotune: bool = True, fuse_downsample: bool = True,
                 fuse_stem_pool: bool = True, fuse_b2b: bool = True, graph_replay: bool = False, hl_monitor: bool = False):
        L = self.L = _lib.load()
        o = _lib.Options()
        L.infur_options_default(C.byref(o))
        o.device = device
        o.compute_dtype = {"f32": _lib.DTYPE_F32, "f16": _lib.DTYPE_F16, "f32s": _lib.DTYPE_F32_SPLIT, "f32x": _lib.DTYPE_F32_SPLIT_FP8,
                           "f16hl": _lib.DTYPE_F16_HL}[dtype]
        self.dtype = dtype
        o.compute_aux = 1 if compute_aux else 0
        o.profile = 1 if profile else 0
        o.keep_activations = 1 if keep_activations else 0
        o.winograd_min_cin = winograd_min_cin  # 0 = default (256), 0xFFFFFFFF = direct convs only
        o.winograd_tile = winograd_tile  # 0 = default F(6x6,3x3); 2 / 4 / 6 = forced
        o.no_autotune = 0 if autotune else 1
        o.no_fuse_downsample = 0 if fuse_downsample else 1
        o.no_fuse_stem_pool = 0 if fuse_stem_pool else 1
        o.no_fuse_b2b = 0 if fuse_b2b else 1  # f16 mode: conv3 + residual and the next block's conv1 as one launch
        o.stream = stream
        h = C.c_void_p(None)
        rc = L.infur_ctx_create(C.byref(o), C.byref(h))
        if rc != _lib.OK:
            raise InfurError(rc, f"infur_ctx_create(device={device}) failed: {_lib.status_string(rc)} "
                                 f"({L.infur_device_count()} HIP devices visible; there is no CPU fallback)")
        self.h = h
        self.device = device
        if autotune and os.path.exists(TUNE_DB):  # measured tile configurations for the common shapes
            self.load_tuning(TUNE_DB)
        if graph_replay:  # the fused frame path as a hipGraph once a frame shape has settled (small frames: launch-bound)
            self.check(L.infur_ctx_set_graph_replay(h, 1))
        if hl_monitor:  # dtype "f16hl" only: the range monitor of the three-byte mode (InfurError otherwise)
            self.set_hl_monitor(True)

    def graph_stats(self):
        """(graphs captured so far, frames replayed from a graph, graphs cached now)"""
        a, b, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self.check(self.L.infur_ctx_graph_stats(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def load_tuning(self, path: str) -> None:
        txt = open(path, "rb").read()
        self.check(self.L.infur_tune_import(self.h, txt, len(txt)))

    def split_range(self):
        """dtype "f32s" only: (max |activation| fed to a GEMM, max |Winograd-domain input|, saturated) of the last frame."""
        a, w, sat = C.c_float(0), C.c_float(0), C.c_uint32(0)
        self.check(self.L.infur_split_range(self.h, C.byref(a), C.byref(w), C.byref(sat)))
        return a.value, w.value, bool(sat.value)

    def set_hl_monitor(self, on: bool) -> None:
        """dtype "f16hl" only (InfurError otherwise): switch the opt-in range monitor on / off."""
        self.check(self.L.infur_hl_monitor_enable(self.h, 1 if on else 0))

    def hl_range(self) -> HlRange:
        """The monitor's values accumulated over every frame since it was enabled or last read; reading clears them."""
        a, w, sat, nan = C.c_float(0), C.c_float(0), C.c_uint32(0), C.c_uint32(0)
        self.check(self.L.infur_hl_range(self.h, C.byref(a), C.byref(w), C.byref(sat), C.byref(nan)))
        return HlRange(a.value, w.value, bool(sat.value), bool(nan.value))

    def tuning_text(self) -> str:
        n = C.c_size_t(0)
        self.check(self.L.infur_tune_export(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        self.check(self.L.infur_tune_export(self.h, buf, n.value, C.byref(n)))
        return buf.raw[: n.value].decode()

    def last_error(self) -> str:
        return self.L.infur_last_error(self.h).decode()

    def check(self, rc: int, exc=InfurError):
        if rc != _lib.OK:
            raise exc(rc, self.last_error() or _lib.status_string(rc))

    def synchronize(self):
        self.check(self.L.infur_ctx_synchronize(self.h))

    @property
    def stream(self) -> int:
        return self.L.infur_ctx_stream(self.h) or 0

    def profile(self) -> List[dict]:
        """Kernel records of the last advance (needs ``profile=True``)."""
        n = C.c_uint32(0)
        self.check(self.L.infur_profile_count(self.h, C.byref(n)))
        out = []
        rec = _lib.KernelRecord()
        variant = C.create_string_buffer(32)
        for i in range(n.value):
            self.check(self.L.infur_profile_get(self.h, i, C.byref(rec)))
            self.check(self.L.infur_debug_profile_variant(self.h, i, variant, len(variant)))
            out.append({"name": rec.name.decode(), "kernel": rec.kernel.decode(), "ms": rec.ms,
                        "flops": rec.flops, "bytes": rec.bytes, "algo_flops": rec.algo_flops,
                        "variant": variant.value.decode()})  # the size-picked kernel inside the configuration ("" = one form)
        return out

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.infur_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# --------------------------------------------------------------------------- #
# the trait
# --------------------------------------------------------------------------- #
class Processor:
    """processing.rs:23-60."""

    def control(self, cmd):
        raise NotImplementedError

    def advance(self, inp, out):
        raise NotImplementedError

    def is_dirty(self) -> bool:
        raise NotImplementedError


class Scale(Processor):
    """Scale frames by a constant factor (processing.rs:179-282).

    Command = f32, Input = Output = Option<Frame>.  ``mode`` selects the resampler:
    nearest is the reference's (processing.rs:189); bilinear is the north-star extension.
    """

    def __init__(self, ctx: Context, mode: int = _lib.SCALE_NEAREST):
        self.ctx = ctx
        self.mode = mode
        self.factor = np.float32(1.0)  # Default, processing.rs:185-193
        self.dirty = True

    def control(self, cmd: float) -> "Scale":
        factor = np.float32(cmd)
        rc = self.ctx.L.infur_scale_validate(float(factor))
        if rc != _lib.OK:
            raise ValidScaleError(rc)  # state untouched, like `cmd.try_into()?` (processing.rs:221)
        self.dirty = bool(factor != self.factor)  # processing.rs:222 (NaN != NaN -> dirty)
        self.factor = factor
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def is_unit_scale(self) -> bool:
        return bool(self.factor == np.float32(1.0))

    def advance(self, inp: Optional[Frame], out: Slot) -> None:
        self.dirty = False  # processing.rs:233
        if inp is None:
            return
        if self.is_unit_scale():  # clone, processing.rs:238-242
            out.value = Frame(inp.id, inp.img.copy())
            return
        img = _check_bgr(inp.img)
        h, w = img.shape[:2]
        L = self.ctx.L
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        rc = L.infur_scale_out_dims(w, h, float(self.factor), C.byref(ow), C.byref(oh))
        if rc != _lib.OK:
            raise ScaleProcError(rc)
        nw, nh = ow.value, oh.value
        # get or create the output frame; re-allocate only on size change (processing.rs:260-268)
        fr = out.value
        if fr is None or fr.img.shape[0] != nh or fr.img.shape[1] != nw or not fr.img.flags["C_CONTIGUOUS"]:
            fr = Frame(inp.id, bgr_image(nw, nh))
            out.value = fr
        fr.id = inp.id
        rc = L.infur_scale(self.ctx.h, img.ctypes.data, w, h, float(self.factor), self.mode,
                           fr.img.ctypes.data, fr.img.nbytes, C.byref(ow), C.byref(oh))
        self.ctx.check(rc, ScaleProcError)


@dataclass
class ModelCmd:
    """predict_onnx.rs:267-270: ``ModelCmd::Load(path)``; empty path unloads."""

    path: str = ""
    blob: Optional[bytes] = None  # extension: load an in-memory INFURW01 blob

    @staticmethod
    def Load(path: str) -> "ModelCmd":
        return ModelCmd(path=path)

    @staticmethod
    def LoadBlob(blob: bytes) -> "ModelCmd":
        return ModelCmd(blob=blob)


@dataclass
class ModelInfo:
    """predict_onnx.rs:56-62."""

    input_names: List[str]
    input0_dtype: str
    output_names: List[str]
    num_classes: int = 0
    depth: int = 0
    weight_bytes: int = 0
    quantised: bool = False        # a QOperator / QDQ int8 model: runs on the i8 MFMA whatever the context's dtype
    resize_u8_heads: bool = False  # ... whose file resizes the u8 logits before DequantizeLinear


class Model(Processor):
    """Segmentation model session (predict_onnx.rs:146-345).

    Command = ModelCmd, Input = BgrImage, Output = Vec<ArrayD<f32>> (a ``list`` here).
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def control(self, cmd: ModelCmd) -> "Model":
        L, h = self.ctx.L, self.ctx.h
        if cmd.blob is not None:
            rc = L.infur_model_load_blob(h, cmd.blob, len(cmd.blob))
        else:
            rc = L.infur_model_load(h, cmd.path.encode())  # "" unloads (predict_onnx.rs:310-312)
        self.ctx.check(rc, ModelCmdError)
        return self

    def is_dirty(self) -> bool:
        return False  # predict_onnx.rs:336-338

    def get_info(self) -> Optional[ModelInfo]:
        mi = _lib.ModelInfoC()
        rc = self.ctx.L.infur_model_info_get(self.ctx.h, C.byref(mi))
        if rc == _lib.E_MODEL_NOT_LOADED:
            return None
        self.ctx.check(rc)
        outs = [bytes(mi.output_names[i]).split(b"\0", 1)[0].decode() for i in range(mi.n_outputs)]
        return ModelInfo([mi.input_name.decode()], mi.input0_dtype.decode(), outs, mi.num_classes, mi.depth,
                         mi.weight_bytes, bool(mi.quantised), bool(mi.resize_u8_heads))

    def advance(self, img: np.ndarray, out: list) -> None:
        """Fills ``out`` with the model's outputs, each [num_classes, h, w] f32 -- [out, aux], or [out] alone for a
        model without the aux head / a context created with ``compute_aux=False`` (``get_info().output_names``);
        untouched when no model is loaded."""
        info = self.get_info()
        if info is None:
            return  # Ok(()) with `out` untouched (predict_onnx.rs:318,333)
        img = _check_bgr(img)
        h, w = img.shape[:2]
        k = info.num_classes
        bufs = [np.empty((k, h, w), np.float32) for _ in info.output_names]
        n = C.c_uint32(0)
        rc = self.ctx.L.infur_model_advance(self.ctx.h, img.ctypes.data, w, h, bufs[0].ctypes.data,
                                            bufs[1].ctypes.data if len(bufs) > 1 else None, C.byref(n))
        self.ctx.check(rc, ModelProcError)
        assert n.value == len(bufs)
        out.clear()  # predict_onnx.rs:326
        out.extend(bufs)

    def warmup(self, w: int, h: int) -> None:
        """Allocate the arena and pick tile configurations for w x h frames before the first real one."""
        self.ctx.check(self.ctx.L.infur_model_warmup(self.ctx.h, w, h), ModelProcError)

    def lowres(self):
        """Output-stride-8 logits of the last advance: (out_low, aux_low) [K, lh, lw] f32; aux_low is None for a
        one-output model."""
        info = self.get_info()
        L, h = self.ctx.L, self.ctx.h
        lh, lw = C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(L.infur_model_read_lowres(h, None, None, C.byref(lh), C.byref(lw)))
        o = np.empty((info.num_classes, lh.value, lw.value), np.float32)
        a = np.empty_like(o) if len(info.output_names) > 1 else None
        self.ctx.check(L.infur_model_read_lowres(h, o.ctypes.data, a.ctypes.data if a is not None else None,
                                                 C.byref(lh), C.byref(lw)))
        return o, a


class ColorCode(Processor):
    """Per-pixel argmax + confidence-shaded RGBA (decode_predict.rs:38-84).

    Input = Array3<f32> [K, H, W]; Output = Option<ColorImage> (``Slot`` of [H, W, 4] u8,
    premultiplied r,g,b,a -- the memory layout of epaint's ``Color32``).
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def control(self, cmd=None) -> "ColorCode":
        return self

    def is_dirty(self) -> bool:
        return False

    def advance(self, inp: np.ndarray, out: Slot) -> None:
        if inp.ndim != 3:
            raise InfurError(_lib.E_SHAPE, f"expected [K,H,W], got {inp.shape}")
        khw = np.ascontiguousarray(inp, np.float32)
        k, h, w = khw.shape
        img = out.value
        if img is None or img.shape[:2] != (h, w):  # re-create only on size change (decode_predict.rs:58-65)
            img = np.zeros((h, w, 4), np.uint8)
            img[..., 3] = 255  # Color32::BLACK
            out.value = img
        self.ctx.check(self.ctx.L.infur_colorcode(self.ctx.h, khw.ctypes.data, k, h, w, img.ctypes.data))


class SegmentsOut:
    """``Segments``' ``&mut Output``: what to produce (``want_*``) and, after ``advance``, the results -- ``klass`` / ``conf``
    [H, W] u8, ``stats`` [K, 8] uint64 (columns ``_lib.STAT_*``), ``rgba`` [H, W, 4] u8; None where not wanted."""

    def __init__(self, want_klass: bool = True, want_conf: bool = True, want_stats: bool = True, want_rgba: bool = False):
        self.want_klass, self.want_conf, self.want_stats, self.want_rgba = want_klass, want_conf, want_stats, want_rgba
        self.klass = self.conf = self.stats = self.rgba = None


class Segments(Processor):
    """ColorCode's sibling for a host without a display: per-pixel argmax class, confidence byte, per-class statistics and
    (optionally) the RGBA overlay shaded by that confidence.

    Command = decode mode (``_lib.DECODE_RAW``: the reference's loop, decode_predict.rs:67-78; ``_lib.DECODE_SOFTMAX``: the
    same loop over logits with the softmax probability of the winner as confidence -- the reference's README.md:76 todo).
    Input = Array3<f32> [K, H, W]; Output = ``SegmentsOut``.
    """

    def __init__(self, ctx: Context, decode: int = _lib.DECODE_RAW):
        self.ctx = ctx
        self.decode = decode
        self.dirty = True

    def control(self, cmd: int) -> "Segments":
        if cmd not in (_lib.DECODE_RAW, _lib.DECODE_SOFTMAX):
            raise InfurError(_lib.E_INVALID_ARG, f"unknown decode mode {cmd}")  # state untouched
        self.dirty = cmd != self.decode
        self.decode = cmd
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: np.ndarray, out: SegmentsOut) -> None:
        self.dirty = False
        if inp.ndim != 3:
            raise InfurError(_lib.E_SHAPE, f"expected [K,H,W], got {inp.shape}")
        khw = np.ascontiguousarray(inp, np.float32)
        k, h, w = khw.shape

        def buf(want, old, shape, dtype):
            if not want:
                return None
            return old if old is not None and old.shape == shape and old.dtype == dtype and old.flags.c_contiguous else np.zeros(shape, dtype)

        out.klass = buf(out.want_klass, out.klass, (h, w), np.uint8)
        out.conf = buf(out.want_conf, out.conf, (h, w), np.uint8)
        out.stats = buf(out.want_stats, out.stats, (k, _lib.STAT_WORDS), np.uint64)
        out.rgba = buf(out.want_rgba, out.rgba, (h, w, 4), np.uint8)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_segments(self.ctx.h, khw.ctypes.data, k, h, w, self.decode, ptr(out.klass), ptr(out.conf),
                                                 ptr(out.stats), ptr(out.rgba)))


class SegmentsFrame(NamedTuple):
    """``FramePath.advance_segments``: class plane and confidence plane [oh, ow] u8, statistics [K, 8] uint64, RGBA overlay
    [oh, ow, 4] u8 or None, scaled BGR frame or None"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    stats: Optional[np.ndarray]
    rgba: Optional[np.ndarray]
    scaled: Optional[np.ndarray]


def voc_class_name(ctx_or_lib, k: int) -> Optional[str]:
    """The Pascal-VOC name torchvision's FCN heads give class ``k`` (None beyond the 21)."""
    L = getattr(ctx_or_lib, "L", ctx_or_lib)
    s = L.infur_voc_class_name(k)
    return s.decode() if s is not None else None


def class_summary(stats: np.ndarray, ow: int, oh: int, names=None) -> List[dict]:
    """The caption records of a frame: one dict per class that occurs, largest first -- ``klass``, ``name``, ``pixels``,
    ``share`` of the ow x oh mask, ``centroid`` (x, y), ``box`` (min_x, min_y, max_x, max_y; inclusive) and
    ``mean_confidence`` in [0, 1].  ``names``: class index -> label (default: the library's Pascal-VOC names)."""
    if names is None:
        L = _lib.load()
        names = lambda k: voc_class_name(L, k)  # noqa: E731
    elif not callable(names):
        table = list(names)
        names = lambda k: table[k] if k < len(table) else None  # noqa: E731
    recs = []
    total = float(ow) * float(oh)
    for k, row in enumerate(np.asarray(stats, np.uint64)):
        n = int(row[_lib.STAT_PIXELS])
        if n == 0:
            continue
        recs.append({
            "klass": k,
            "name": names(k) or f"class{k}",
            "pixels": n,
            "share": n / total if total else 0.0,
            "centroid": (int(row[_lib.STAT_SUM_X]) / n, int(row[_lib.STAT_SUM_Y]) / n),
            "box": (int(row[_lib.STAT_MIN_X]), int(row[_lib.STAT_MIN_Y]), int(row[_lib.STAT_MAX_X]), int(row[_lib.STAT_MAX_Y])),
            "mean_confidence": int(row[_lib.STAT_SUM_CONF]) / (255.0 * n),
        })
    recs.sort(key=lambda r: (-r["pixels"], r["klass"]))
    return recs


@dataclass
class RegionsCmd:
    """``Regions``' command: exactly one of connectivity (``_lib.CONNECT_4`` / ``_lib.CONNECT_8``), min_pixels, flags."""

    connectivity: Optional[int] = None
    min_pixels: Optional[int] = None
    flags: Optional[int] = None

    @staticmethod
    def Connectivity(v: int) -> "RegionsCmd":
        return RegionsCmd(connectivity=v)

    @staticmethod
    def MinPixels(v: int) -> "RegionsCmd":
        return RegionsCmd(min_pixels=v)

    @staticmethod
    def Flags(v: int) -> "RegionsCmd":
        return RegionsCmd(flags=v)


class RegionsOut:
    """``Regions``' ``&mut Output``: what to produce (``want_labels``, ``table_rows``) and, after ``advance``, the results --
    ``labels`` [H, W] u32 (``_lib.REGION_NONE``: no kept region) or None, ``table`` [min(n, table_rows), 10] uint64 (columns
    ``_lib.STAT_*``, ``_lib.REGION_CLASS``, ``_lib.REGION_FIRST``) or None, ``n`` the number of kept regions."""

    def __init__(self, want_labels: bool = True, table_rows: int = 1024):
        self.want_labels, self.table_rows = want_labels, table_rows
        self.labels = self.table = None
        self.n = 0


class Regions(Processor):
    """The third decode stage: the connected components of a class plane, one table row per object.

    Command = ``RegionsCmd``.  Input = (klass [H, W] u8, conf [H, W] u8 or None), e.g. ``SegmentsOut``'s planes;
    Output = ``RegionsOut``.  Regions are numbered in ascending order of their first pixel; the results are integers and
    identical from run to run.
    """

    def __init__(self, ctx: Context, connectivity: int = _lib.CONNECT_8, min_pixels: int = 0, flags: int = 0):
        self.ctx = ctx
        self.connectivity, self.min_pixels, self.flags = connectivity, min_pixels, flags
        self.dirty = True

    def control(self, cmd: RegionsCmd) -> "Regions":
        given = [v for v in (cmd.connectivity, cmd.min_pixels, cmd.flags) if v is not None]
        if len(given) != 1:
            raise InfurError(_lib.E_INVALID_ARG, "a RegionsCmd sets exactly one of connectivity, min_pixels, flags")
        if cmd.connectivity is not None and cmd.connectivity not in (_lib.CONNECT_4, _lib.CONNECT_8):
            raise InfurError(_lib.E_INVALID_ARG, f"connectivity {cmd.connectivity}: 4 or 8")  # state untouched
        if cmd.flags is not None and cmd.flags & ~_lib.REGIONS_SKIP_BACKGROUND:
            raise InfurError(_lib.E_INVALID_ARG, f"unknown regions flags {cmd.flags:#x}")
        if cmd.min_pixels is not None and not 0 <= cmd.min_pixels <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"min_pixels {cmd.min_pixels}")
        new = (cmd.connectivity if cmd.connectivity is not None else self.connectivity,
               cmd.min_pixels if cmd.min_pixels is not None else self.min_pixels, cmd.flags if cmd.flags is not None else self.flags)
        self.dirty = self.dirty or new != (self.connectivity, self.min_pixels, self.flags)
        self.connectivity, self.min_pixels, self.flags = new
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp, out: RegionsOut) -> None:
        self.dirty = False
        klass, conf = inp
        if klass.ndim != 2 or (conf is not None and conf.shape != klass.shape):
            raise InfurError(_lib.E_SHAPE, f"expected [H,W] planes, got {klass.shape}")
        klass = np.ascontiguousarray(klass, np.uint8)
        conf = np.ascontiguousarray(conf, np.uint8) if conf is not None else None
        h, w = klass.shape
        rows = max(0, min(int(out.table_rows), h * w))
        labels = np.empty((h, w), np.uint32) if out.want_labels else None
        table = np.zeros((rows, _lib.REGION_WORDS), np.uint64) if rows else None
        n = C.c_uint32(0)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_regions(self.ctx.h, ptr(klass), ptr(conf), h, w, self.connectivity, self.min_pixels, self.flags,
                                                ptr(labels), ptr(table), rows, C.addressof(n)))
        out.labels, out.n = labels, n.value
        out.table = table[:min(n.value, rows)] if table is not None else None


class RegionsFrame(NamedTuple):
    """``FramePath.advance_regions``: class / confidence planes [oh, ow] u8 (None where not wanted), label plane [oh, ow] u32,
    region table [min(n, table_rows), 10] uint64, the number of kept regions, scaled BGR frame or None"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    table: Optional[np.ndarray]
    n: Optional[int]
    scaled: Optional[np.ndarray]


def region_summary(table: np.ndarray, n: int, ow: int, oh: int, names=None, anchors=None) -> List[dict]:
    """The caption records of a frame's objects: one dict per table row, in id order -- ``id``, ``klass``, ``name``, ``pixels``,
    ``share`` of the ow x oh mask, ``centroid`` (x, y), ``box`` (min_x, min_y, max_x, max_y; inclusive), ``mean_confidence``
    in [0, 1] and ``first`` (x, y), the region's first pixel in raster order.  ``n`` may exceed the rows the table holds (a
    truncated table): the rows there are are summarised.  ``names`` as in ``class_summary``.  ``anchors`` (Anchors' rows, row i
    for region i) adds ``anchor`` [x, y], the region's most interior pixel, and ``radius``, the distance from there to the nearest
    pixel of anything else, to two decimals; both are None for a row without an anchor."""
    if names is None:
        L = _lib.load()
        names = lambda k: voc_class_name(L, k)  # noqa: E731
    elif not callable(names):
        lookup = list(names)
        names = lambda k: lookup[k] if k < len(lookup) else None  # noqa: E731
    recs = []
    total = float(ow) * float(oh)
    rows = np.asarray(table, np.uint64).reshape(-1, _lib.REGION_WORDS)
    for i, row in enumerate(rows[:min(int(n), len(rows))]):
        px, k, first = int(row[_lib.STAT_PIXELS]), int(row[_lib.REGION_CLASS]), int(row[_lib.REGION_FIRST])
        recs.append({
            "id": i,
            "klass": k,
            "name": names(k) or f"class{k}",
            "pixels": px,
            "share": px / total if total else 0.0,
            "centroid": (int(row[_lib.STAT_SUM_X]) / px, int(row[_lib.STAT_SUM_Y]) / px),
            "box": (int(row[_lib.STAT_MIN_X]), int(row[_lib.STAT_MIN_Y]), int(row[_lib.STAT_MAX_X]), int(row[_lib.STAT_MAX_Y])),
            "mean_confidence": int(row[_lib.STAT_SUM_CONF]) / (255.0 * px),
            "first": (first % ow, first // ow) if ow else (0, 0),
        })
    if anchors is not None:
        arows = np.asarray(anchors, np.uint32).reshape(-1, _lib.ANCHOR_WORDS)
        for i, rec in enumerate(recs):
            at = int(arows[i, _lib.ANCHOR_PIXEL]) if i < len(arows) else _lib.ANCHOR_NONE
            have = at != _lib.ANCHOR_NONE and ow
            rec["anchor"] = [at % ow, at // ow] if have else None
            rec["radius"] = round(math.sqrt(int(arows[i, _lib.ANCHOR_DIST2])), 2) if have else None
    return recs


@dataclass
class TracksCmd:
    """``Tracks``' command: exactly one of min_overlap, or reset (the first id of the tracks that follow; the frame is forgotten)."""

    min_overlap: Optional[int] = None
    reset: Optional[int] = None

    @staticmethod
    def MinOverlap(v: int) -> "TracksCmd":
        return TracksCmd(min_overlap=v)

    @staticmethod
    def Reset(first_id: int = 0) -> "TracksCmd":
        return TracksCmd(reset=first_id)


class TracksOut:
    """``Tracks``' ``&mut Output``: what to produce (``want_plane``) and, after ``advance``, the results -- ``track_of_region``
    [min(n, rows)] u32 (``_lib.TRACK_NONE``: not tracked), ``table`` [min(n, rows), 8] uint64 (columns ``_lib.TRACK_*``),
    ``plane`` [H, W] u32 or None, ``summary`` [4] u32 (``_lib.TRACKS_SUMMARY_*``) and its fields ``status`` (``_lib.TRACKS_*``
    bits), ``continued``, ``new``, ``ended``.  On a tracker with memory also ``gap_of_region`` [min(n, rows)] u32 and ``memory``
    [4] u32 (``_lib.TRACK_MEMORY_*``: revived, lost, expired, held); both are None without memory."""

    def __init__(self, want_plane: bool = False):
        self.want_plane = want_plane
        self.track_of_region = self.table = self.plane = self.summary = None
        self.gap_of_region = self.memory = None
        self.status = self.continued = self.new = self.ended = 0

    def _set(self, tor, table, plane, summary, n):
        self.track_of_region = tor[:n] if tor is not None else None
        self.table = table[:n] if table is not None else None
        self.plane, self.summary = plane, summary
        self.status, self.continued, self.new, self.ended = (int(v) for v in summary)


class Tracks(Processor):
    """The fourth decode stage: region identities carried from frame to frame.  Owns its tracker (one remembered frame on the
    device): ``close()`` it, or let it go with its context.

    Command = ``TracksCmd``.  Input = (labels [H, W] u32, table [rows, 10] uint64, n), i.e. ``RegionsOut``'s fields;
    Output = ``TracksOut``.  A region inherits the track of the remembered region of its class it overlaps most (when that
    region prefers it too), otherwise it starts a new one; integers throughout, identical from run to run.
    """

    def __init__(self, ctx: Context, max_regions: int = 0, pair_slots: int = 0, min_overlap: int = 1, max_lost: int = 0, reach: int = 0,
                 gallery_rows: int = 0):
        self.ctx = ctx
        self.min_overlap = min_overlap
        self.dirty = True
        self.max_lost = 0
        t = C.c_void_p()
        ctx.check(ctx.L.infur_tracker_create(ctx.h, max_regions, pair_slots, C.byref(t)))
        self.t = t
        if max_lost:
            self.set_memory(max_lost, reach, gallery_rows)

    def set_memory(self, max_lost: int, reach: int = 0, gallery_rows: int = 0) -> "Tracks":
        """Keep lost tracks for up to ``max_lost`` steps (0: memory off): a region that would start a new track takes a lost
        track of its class back when its box meets that track's last box grown by ``reach`` pixels per step of absence.  Forgets
        the remembered frame and the gallery."""
        self.ctx.check(self.ctx.L.infur_tracker_set_memory(self.t, max_lost, reach, gallery_rows))
        self.max_lost = max_lost
        self.dirty = True
        return self

    def memory(self, rows: int):
        """-> (gap_of_region [rows] u32, memory summary [4] u32) of the last step, or (None, None) without memory"""
        if not getattr(self, "max_lost", 0):
            return None, None
        gap, msum = np.zeros(rows, np.uint32), np.zeros(_lib.TRACK_MEMORY_WORDS, np.uint32)
        self.ctx.check(self.ctx.L.infur_tracker_memory(self.t, gap.ctypes.data if rows else None, rows, msum.ctypes.data, None, 0))
        return gap, msum

    def lost(self, lost_rows: Optional[int] = None) -> Optional[np.ndarray]:
        """-> the gallery as the last step left it, [min(HELD, lost_rows), 12] uint64 (columns ``_lib.LOST_*``) in gallery
        order; None without memory"""
        if not getattr(self, "max_lost", 0):
            return None
        msum = np.zeros(_lib.TRACK_MEMORY_WORDS, np.uint32)
        self.ctx.check(self.ctx.L.infur_tracker_memory(self.t, None, 0, msum.ctypes.data, None, 0))
        held = int(msum[_lib.TRACK_MEMORY_HELD])
        rows = held if lost_rows is None else min(held, int(lost_rows))
        table = np.zeros((rows, _lib.LOST_WORDS), np.uint64)
        if rows:
            self.ctx.check(self.ctx.L.infur_tracker_memory(self.t, None, 0, None, table.ctypes.data, rows))
        return table

    def control(self, cmd: TracksCmd) -> "Tracks":
        given = [v for v in (cmd.min_overlap, cmd.reset) if v is not None]
        if len(given) != 1 or not 0 <= given[0] <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, "a TracksCmd sets exactly one of min_overlap, reset, each a u32")
        if cmd.reset is not None:
            self.ctx.check(self.ctx.L.infur_tracker_reset(self.t, cmd.reset))
            self.dirty = True
        else:
            self.dirty = self.dirty or cmd.min_overlap != self.min_overlap
            self.min_overlap = cmd.min_overlap
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp, out: TracksOut) -> None:
        self.dirty = False
        labels, table, n = inp
        if labels.ndim != 2:
            raise InfurError(_lib.E_SHAPE, f"expected an [H,W] label plane, got {labels.shape}")
        labels = np.ascontiguousarray(labels, np.uint32)
        h, w = labels.shape
        table = np.ascontiguousarray(table if table is not None else np.zeros((0, _lib.REGION_WORDS)), np.uint64).reshape(-1, _lib.REGION_WORDS)
        rows = len(table)
        tor = np.empty(rows, np.uint32)
        ttab = np.empty((rows, _lib.TRACK_WORDS), np.uint64)
        plane = np.empty((h, w), np.uint32) if out.want_plane else None
        summary = np.zeros(_lib.TRACKS_SUMMARY_WORDS, np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_tracks(self.t, ptr(labels), ptr(table), rows, int(n), h, w, self.min_overlap, ptr(tor), ptr(plane),
                                               ptr(ttab), summary.ctypes.data))
        k = min(int(n), rows) if h * w else 0
        out._set(tor, ttab, plane, summary, k)
        out.gap_of_region, out.memory = self.memory(k)

    def close(self):
        if getattr(self, "t", None):
            self.ctx.L.infur_tracker_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TracksFrame(NamedTuple):
    """``FramePath.advance_tracks``: the fields of ``RegionsFrame``, then ``track_of_region`` [min(n, table_rows)] u32, the track
    table [min(n, table_rows), 8] uint64, the track plane [oh, ow] u32 or None and the summary [4] u32; on a tracker with memory
    also ``gap_of_region`` [min(n, table_rows)] u32 and the memory summary [4] u32 (None without memory)"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    table: Optional[np.ndarray]
    n: Optional[int]
    scaled: Optional[np.ndarray]
    track_of_region: Optional[np.ndarray]
    track_table: Optional[np.ndarray]
    track_plane: Optional[np.ndarray]
    summary: Optional[np.ndarray]
    gap_of_region: Optional[np.ndarray] = None
    memory: Optional[np.ndarray] = None


def track_summary(table: np.ndarray, track_table: np.ndarray, n: int, ow: int, oh: int, names=None, gap=None) -> List[dict]:
    """``region_summary``'s records joined with the track table, one dict per row both tables hold, in region order: added are
    ``track`` (None for an untracked region), ``age``, ``born``, ``prev_region`` (None for a new track), ``overlap`` and
    ``step`` -- this frame's centroid minus the inherited region's, (dx, dy), or None for a new or untracked region."""
    recs = region_summary(table, n, ow, oh, names)
    rows = np.asarray(track_table, np.uint64).reshape(-1, _lib.TRACK_WORDS)
    recs = recs[:len(rows)]
    for rec, row in zip(recs, rows):
        tid, prev, ppx = int(row[_lib.TRACK_ID]), int(row[_lib.TRACK_PREV_REGION]), int(row[_lib.TRACK_PREV_PIXELS])
        rec["track"] = tid if tid != _lib.TRACK_NONE else None
        rec["age"], rec["born"] = int(row[_lib.TRACK_AGE]), int(row[_lib.TRACK_BORN])
        rec["prev_region"] = prev if prev != _lib.REGION_NONE else None
        rec["overlap"] = int(row[_lib.TRACK_OVERLAP])
        rec["step"] = None
        if rec["prev_region"] is not None and ppx:
            cx, cy = rec["centroid"]
            rec["step"] = (cx - int(row[_lib.TRACK_PREV_SUM_X]) / ppx, cy - int(row[_lib.TRACK_PREV_SUM_Y]) / ppx)
    if gap is not None:  # a tracker with memory: the steps a revived track was absent (0 for every other region)
        for rec, g in zip(recs, gap):
            rec["gap"] = int(g)
    return recs


@dataclass
class RunsCmd:
    """``Runs``' command: ``Skip(value)`` drops the runs of that value (``Skip(None)``: every run is emitted again)."""

    skip: Optional[int] = None

    @staticmethod
    def Skip(v: Optional[int]) -> "RunsCmd":
        return RunsCmd(skip=v)


class RunsOut:
    """``Runs``' ``&mut Output``: what to produce (``runs_rows`` records at most, ``want_row_start``) and, after ``advance``, the
    results -- ``runs`` [min(n, runs_rows), 3] u32 (columns ``_lib.RUN_START``, ``_lib.RUN_END``, ``_lib.RUN_VALUE``) or None,
    ``row_start`` [H + 1] u32 or None, ``n`` the number of runs (above ``len(runs)``: truncated)."""

    def __init__(self, runs_rows: int = 1 << 16, want_row_start: bool = True):
        self.runs_rows, self.want_row_start = runs_rows, want_row_start
        self.runs = self.row_start = None
        self.n = 0


class Runs(Processor):
    """The egress stage: a class / confidence plane (u8) or a label / track plane (u32) as raster-ordered runs.

    Command = ``RunsCmd``.  Input = a plane [H, W] of u8 or u32; Output = ``RunsOut``.  A run is a maximal sequence of equal
    values within one row; integers throughout, identical from run to run.
    """

    def __init__(self, ctx: Context, skip: Optional[int] = None):
        self.ctx = ctx
        self.skip = skip
        self.dirty = True

    def control(self, cmd: RunsCmd) -> "Runs":
        if cmd.skip is not None and not 0 <= cmd.skip <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"skip value {cmd.skip}: a u32")
        self.dirty = self.dirty or cmd.skip != self.skip
        self.skip = cmd.skip
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: np.ndarray, out: RunsOut) -> None:
        self.dirty = False
        if inp.ndim != 2 or inp.dtype.itemsize not in (1, 4) or inp.dtype.kind not in "ui":
            raise InfurError(_lib.E_SHAPE, f"expected an [H,W] plane of 1- or 4-byte integers, got {inp.shape} {inp.dtype}")
        plane = np.ascontiguousarray(inp)
        h, w = plane.shape
        rows = max(0, min(int(out.runs_rows), h * w))
        runs = np.empty((rows, _lib.RUN_WORDS), np.uint32) if rows else None
        row_start = np.empty(h + 1, np.uint32) if out.want_row_start else None
        n = C.c_uint32(0)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_runs(self.ctx.h, ptr(plane), plane.dtype.itemsize, h, w, _lib.RUNS_SKIP if self.skip is not None else 0,
                                             self.skip or 0, ptr(runs), rows, ptr(row_start), C.addressof(n)))
        out.n, out.row_start = n.value, row_start
        out.runs = runs[:min(n.value, rows)] if runs is not None else None


class RunsFrame(NamedTuple):
    """``FramePath.advance_runs``: the records [min(n, runs_rows), 3] u32 of the class plane, the per-row index [oh + 1] u32, the
    number of runs, the per-class statistics [k, 8] uint64 or None, the scaled BGR frame or None"""

    runs: Optional[np.ndarray]
    row_start: Optional[np.ndarray]
    n: Optional[int]
    stats: Optional[np.ndarray]
    scaled: Optional[np.ndarray]


@dataclass
class AnchorsCmd:
    """``Anchors``' command: ``Skip(value)`` takes the pixels of that value out of every region (``Skip(None)``: every value is
    a region again)."""

    skip: Optional[int] = None

    @staticmethod
    def Skip(v: Optional[int]) -> "AnchorsCmd":
        return AnchorsCmd(skip=v)


class AnchorsOut:
    """``Anchors``' ``&mut Output``: what to produce (``rows`` anchor rows, ``want_dist2``) and, after ``advance``, the results --
    ``dist2`` [H, W] u32 or None, ``anchors`` [rows, 2] u32 (columns ``_lib.ANCHOR_PIXEL``, ``_lib.ANCHOR_DIST2``; a value no
    pixel holds reads ``(_lib.ANCHOR_NONE, 0)``) or None."""

    def __init__(self, rows: int = 256, want_dist2: bool = True):
        self.rows, self.want_dist2 = rows, want_dist2
        self.dist2 = self.anchors = None


class Anchors(Processor):
    """The stage that measures how thick a region is: the exact squared distance transform of a class plane (u8) or a label /
    track plane (u32) by value, the frame counting as a border, and per value its most interior pixel.

    Command = ``AnchorsCmd``.  Input = a plane [H, W] of u8 or u32; Output = ``AnchorsOut``.  Integers throughout, identical
    from run to run.
    """

    def __init__(self, ctx: Context, skip: Optional[int] = None):
        self.ctx = ctx
        self.skip = skip
        self.dirty = True

    def control(self, cmd: AnchorsCmd) -> "Anchors":
        if cmd.skip is not None and not 0 <= cmd.skip <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"skip value {cmd.skip}: a u32")
        self.dirty = self.dirty or cmd.skip != self.skip
        self.skip = cmd.skip
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: np.ndarray, out: AnchorsOut) -> None:
        self.dirty = False
        if inp.ndim != 2 or inp.dtype.itemsize not in (1, 4) or inp.dtype.kind not in "ui":
            raise InfurError(_lib.E_SHAPE, f"expected an [H,W] plane of 1- or 4-byte integers, got {inp.shape} {inp.dtype}")
        plane = np.ascontiguousarray(inp)
        h, w = plane.shape
        rows = max(0, int(out.rows))
        dist2 = np.empty((h, w), np.uint32) if out.want_dist2 else None
        anchors = np.empty((rows, _lib.ANCHOR_WORDS), np.uint32) if rows else None
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_anchors(self.ctx.h, ptr(plane), plane.dtype.itemsize, h, w, _lib.ANCHORS_SKIP if self.skip is not None else 0,
                                                self.skip or 0, _ptr(dist2), ptr(anchors), rows))
        out.dist2, out.anchors = dist2, anchors


class AnchorsFrame(NamedTuple):
    """``FramePath.advance_anchors``: ``RegionsFrame``'s fields, then the squared distances [oh, ow] u32 of the label plane (None
    where not wanted) and the anchor rows [min(n, table_rows), 2] u32, row i for region i"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    table: Optional[np.ndarray]
    n: Optional[int]
    scaled: Optional[np.ndarray]
    dist2: Optional[np.ndarray]
    anchors: Optional[np.ndarray]


@dataclass
class CompareCmd:
    """``Compare``'s command: ``Ignore(a, b)`` takes the pixels whose ``a`` (``b``) plane holds that value out of the comparison
    (None: every value is compared); ``pair_slots`` sizes the pair table of the table form (0: the library's 2^20)."""

    ignore_a: Optional[int] = None
    ignore_b: Optional[int] = None
    pair_slots: int = 0

    @staticmethod
    def Ignore(a: Optional[int] = None, b: Optional[int] = None, pair_slots: int = 0) -> "CompareCmd":
        return CompareCmd(ignore_a=a, ignore_b=b, pair_slots=pair_slots)


class CompareOut:
    """``Compare``'s ``&mut Output``: what to produce (``rows_a``, ``rows_b`` values on each side, ``want_matrix``,
    ``want_rows``, ``want_counts``) and, after ``advance``, the results -- ``matrix`` [rows_a, rows_b] u32, ``a`` [rows_a, 4] and
    ``b`` [rows_b, 4] u32 (columns ``_lib.COMPARE_PIXELS`` .. ``_lib.COMPARE_UNION``; a value no compared pixel holds reads
    ``(0, _lib.COMPARE_NONE, 0, 0)``), ``counts`` [8] u32 (``_lib.COMPARE_COMPARED`` .. ``_lib.COMPARE_STATUS``); None for what
    was not wanted."""

    def __init__(self, rows_a: int = 21, rows_b: int = 21, want_matrix: bool = True, want_rows: bool = True, want_counts: bool = True):
        self.rows_a, self.rows_b = rows_a, rows_b
        self.want_matrix, self.want_rows, self.want_counts = want_matrix, want_rows, want_counts
        self.matrix = self.a = self.b = self.counts = None


def _compare_alloc(rows_a: int, rows_b: int, want_matrix: bool, want_rows: bool, want_counts: bool) -> tuple:
    """-> (matrix, rows of a, rows of b, counts): the arrays a compare call fills, None for what is not wanted or has no rows"""
    return (np.empty((rows_a, rows_b), np.uint32) if want_matrix and rows_a * rows_b else None,
            np.empty((rows_a, _lib.COMPARE_WORDS), np.uint32) if want_rows and rows_a else None,
            np.empty((rows_b, _lib.COMPARE_WORDS), np.uint32) if want_rows and rows_b else None,
            np.empty(_lib.COMPARE_COUNT_WORDS, np.uint32) if want_counts else None)


class Compare(Processor):
    """The stage that grades a result: the confusion matrix of two planes -- class planes (u8), label or track planes (u32), in
    any combination -- and per value of either plane its best partner in the other with intersection and union.

    Command = ``CompareCmd``.  Input = a pair of planes (a, b) of one [H, W]; Output = ``CompareOut``.  Integers throughout,
    identical from run to run; ``confusion_summary`` and ``panoptic_summary`` turn them into the usual measures.
    """

    def __init__(self, ctx: Context, ignore_a: Optional[int] = None, ignore_b: Optional[int] = None, pair_slots: int = 0):
        self.ctx = ctx
        self.ignore_a, self.ignore_b, self.pair_slots = ignore_a, ignore_b, pair_slots
        self.dirty = True

    def control(self, cmd: CompareCmd) -> "Compare":
        for v in (cmd.ignore_a, cmd.ignore_b):
            if v is not None and not 0 <= v <= 0xFFFFFFFF:
                raise InfurError(_lib.E_INVALID_ARG, f"ignore value {v}: a u32")
        if not 0 <= cmd.pair_slots <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"pair_slots {cmd.pair_slots}: a u32")
        new = (cmd.ignore_a, cmd.ignore_b, cmd.pair_slots)
        self.dirty = self.dirty or new != (self.ignore_a, self.ignore_b, self.pair_slots)
        self.ignore_a, self.ignore_b, self.pair_slots = new
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def flags(self) -> int:
        return (_lib.COMPARE_IGNORE_A if self.ignore_a is not None else 0) | (_lib.COMPARE_IGNORE_B if self.ignore_b is not None else 0)

    def advance(self, inp, out: CompareOut) -> None:
        self.dirty = False
        a, b = inp
        for p in (a, b):
            if p.ndim != 2 or p.dtype.itemsize not in (1, 4) or p.dtype.kind not in "ui":
                raise InfurError(_lib.E_SHAPE, f"expected an [H,W] plane of 1- or 4-byte integers, got {p.shape} {p.dtype}")
        if a.shape != b.shape:
            raise InfurError(_lib.E_SHAPE, f"two planes of one size, got {a.shape} and {b.shape}")
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        h, w = a.shape
        rows_a, rows_b = max(0, int(out.rows_a)), max(0, int(out.rows_b))
        matrix, ra, rb, counts = _compare_alloc(rows_a, rows_b, out.want_matrix, out.want_rows, out.want_counts)
        ptr = lambda p: p.ctypes.data if p.size else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_compare(self.ctx.h, ptr(a), a.dtype.itemsize, ptr(b), b.dtype.itemsize, h, w, self.flags(), self.ignore_a or 0,
                                                self.ignore_b or 0, _ptr(matrix), rows_a, rows_b, _ptr(ra), _ptr(rb), _ptr(counts), self.pair_slots))
        out.matrix, out.a, out.b, out.counts = matrix, ra, rb, counts


class CompareFrame(NamedTuple):
    """``FramePath.advance_compare``: the class and confidence planes [oh, ow] u8 and the scaled frame (None where not wanted),
    then ``CompareOut``'s four results of the class plane (a) against the caller's truth plane (b)"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    scaled: Optional[np.ndarray]
    matrix: Optional[np.ndarray]
    a: Optional[np.ndarray]
    b: Optional[np.ndarray]
    counts: Optional[np.ndarray]


def confusion_summary(matrix: np.ndarray, names=None) -> dict:
    """The usual measures of a confusion matrix (``matrix[i][j]``: pixels the first plane calls i and the second j; a matrix that
    is not square is read as padded with zeros): ``pixel_accuracy`` (None for an empty matrix), ``classes`` -- one dict per class
    with ``klass``, ``name``, ``intersection``, ``union`` and ``iou`` (None where the union is 0) --, ``miou`` over the classes
    with a non-zero union (None when there is none) and ``fwiou``, the IoUs weighted by the second plane's class frequencies.
    The host adds the matrices of several frames before it asks.  ``names`` as in ``class_summary``."""
    if names is None:
        L = _lib.load()
        names = lambda k: voc_class_name(L, k)  # noqa: E731
    elif not callable(names):
        table = list(names)
        names = lambda k: table[k] if k < len(table) else None  # noqa: E731
    m = np.asarray(matrix, np.uint64)
    k = max(m.shape) if m.size else 0
    sq = np.zeros((k, k), np.uint64)
    if m.size:
        sq[:m.shape[0], :m.shape[1]] = m
    total = int(sq.sum())
    inter = [int(v) for v in np.diag(sq)]
    row, col = [int(v) for v in sq.sum(axis=1)], [int(v) for v in sq.sum(axis=0)]
    classes, ious, fw = [], [], 0.0
    for c in range(k):
        union = row[c] + col[c] - inter[c]
        iou = inter[c] / union if union else None
        classes.append({"klass": c, "name": names(c) or f"class{c}", "intersection": inter[c], "union": union, "iou": iou})
        if union:
            ious.append(iou)
            fw += col[c] * iou
    return {"pixel_accuracy": sum(inter) / total if total else None, "classes": classes, "miou": sum(ious) / len(ious) if ious else None,
            "fwiou": fw / total if total else None}


def panoptic_summary(rows_a: np.ndarray, rows_b: np.ndarray, class_of_a, class_of_b) -> dict:
    """Panoptic quality from ``Compare``'s two row tables of a predicted label plane (a) against a ground-truth one (b).
    ``class_of_a[i]`` and ``class_of_b[j]`` are the classes of the segments (Regions' table column ``_lib.REGION_CLASS``).  A
    segment is one with PIXELS > 0; a pair is a true positive iff it is matched (2 INTER > UNION, which makes it unique and
    mutual) and the classes agree; every other segment of a is a false positive of its class, every other segment of b a false
    negative of its.  -> ``classes``: {class: {tp, fp, fn, sum_iou, pq, sq, rq}} for the classes that occur, and ``pq``, ``sq``,
    ``rq`` averaged over them (None when there is none)."""
    ra = np.asarray(rows_a, np.uint32).reshape(-1, _lib.COMPARE_WORDS)
    rb = np.asarray(rows_b, np.uint32).reshape(-1, _lib.COMPARE_WORDS)
    acc: dict = {}
    slot = lambda c: acc.setdefault(int(c), {"tp": 0, "fp": 0, "fn": 0, "sum_iou": 0.0})  # noqa: E731
    taken = set()
    for i, (pix, partner, inter, union) in enumerate(ra.tolist()):
        if not pix:
            continue
        if 2 * inter > union and int(class_of_a[i]) == int(class_of_b[partner]):
            s = slot(class_of_a[i])
            s["tp"] += 1
            s["sum_iou"] += inter / union
            taken.add(partner)
        else:
            slot(class_of_a[i])["fp"] += 1
    for j, (pix, _, _, _) in enumerate(rb.tolist()):
        if pix and j not in taken:
            slot(class_of_b[j])["fn"] += 1
    for s in acc.values():
        den = s["tp"] + 0.5 * s["fp"] + 0.5 * s["fn"]
        s["pq"] = s["sum_iou"] / den
        s["sq"] = s["sum_iou"] / s["tp"] if s["tp"] else 0.0
        s["rq"] = s["tp"] / den
    mean = lambda f: sum(s[f] for s in acc.values()) / len(acc) if acc else None  # noqa: E731
    return {"classes": dict(sorted(acc.items())), "pq": mean("pq"), "sq": mean("sq"), "rq": mean("rq")}


@dataclass
class AdjacencyCmd:
    """``Adjacency``'s command: ``Skip(value)`` takes the pixels of that value out of every region (None: none are skipped);
    ``pair_slots`` sizes the pair table (0: the library's 2^20)."""

    skip_value: Optional[int] = None
    pair_slots: int = 0

    @staticmethod
    def Skip(value: Optional[int] = None, pair_slots: int = 0) -> "AdjacencyCmd":
        return AdjacencyCmd(skip_value=value, pair_slots=pair_slots)


class AdjacencyOut:
    """``Adjacency``'s ``&mut Output``: what to produce (``rows`` values, ``pair_rows`` records at most, ``want_pairs``,
    ``want_rows``, ``want_counts``) and, after ``advance``, the results -- ``pairs`` [WRITTEN, 4] u32 (columns ``_lib.ADJ_A`` ..
    ``_lib.ADJ_FIRST``, in ascending FIRST), ``table`` [rows, 4] u32 (``_lib.ADJ_DEGREE`` .. ``_lib.ADJ_PERIMETER``), ``counts``
    [8] u32 (``_lib.ADJ_PAIRS`` .. ``_lib.ADJ_STATUS``); None for what was not wanted."""

    def __init__(self, rows: int = 21, pair_rows: int = 4096, want_pairs: bool = True, want_rows: bool = True, want_counts: bool = True):
        self.rows, self.pair_rows = rows, pair_rows
        self.want_pairs, self.want_rows, self.want_counts = want_pairs, want_rows, want_counts
        self.pairs = self.table = self.counts = None


class Adjacency(Processor):
    """The region adjacency graph of a plane -- a class plane (u8), a label or track plane (u32): which values touch along how
    many pixel edges, and per value its degree, longest neighbour and perimeter.

    Command = ``AdjacencyCmd``.  Input = an [H, W] plane; Output = ``AdjacencyOut``.  Integers throughout, identical from run to
    run; ``adjacency_graph`` turns the records into neighbour lists.
    """

    def __init__(self, ctx: Context, skip_value: Optional[int] = None, pair_slots: int = 0):
        self.ctx = ctx
        self.skip_value, self.pair_slots = skip_value, pair_slots
        self.dirty = True

    def control(self, cmd: AdjacencyCmd) -> "Adjacency":
        if cmd.skip_value is not None and not 0 <= cmd.skip_value <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"skip value {cmd.skip_value}: a u32")
        if not 0 <= cmd.pair_slots <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"pair_slots {cmd.pair_slots}: a u32")
        new = (cmd.skip_value, cmd.pair_slots)
        self.dirty = self.dirty or new != (self.skip_value, self.pair_slots)
        self.skip_value, self.pair_slots = new
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: np.ndarray, out: AdjacencyOut) -> None:
        self.dirty = False
        if inp.ndim != 2 or inp.dtype.itemsize not in (1, 4) or inp.dtype.kind not in "ui":
            raise InfurError(_lib.E_SHAPE, f"expected an [H,W] plane of 1- or 4-byte integers, got {inp.shape} {inp.dtype}")
        plane = np.ascontiguousarray(inp)
        h, w = plane.shape
        rows, pair_rows = max(0, int(out.rows)), max(0, int(out.pair_rows))
        pairs = np.empty((pair_rows, _lib.ADJ_PAIR_WORDS), np.uint32) if out.want_pairs else None
        table = np.empty((rows, _lib.ADJ_ROW_WORDS), np.uint32) if out.want_rows and rows else None
        counts = np.zeros(_lib.ADJ_COUNT_WORDS, np.uint32)
        self.ctx.check(self.ctx.L.infur_adjacency(self.ctx.h, plane.ctypes.data if plane.size else None, plane.dtype.itemsize, h, w,
                                                  _lib.ADJ_SKIP if self.skip_value is not None else 0, self.skip_value or 0, rows,
                                                  pairs.ctypes.data if pairs is not None else None, pair_rows, _ptr(table), counts.ctypes.data,
                                                  self.pair_slots))
        out.pairs = pairs[:int(counts[_lib.ADJ_WRITTEN])] if pairs is not None else None
        out.table, out.counts = table, counts if out.want_counts else None


def adjacency_graph(pairs: np.ndarray, rows: int) -> dict:
    """``Adjacency``'s pair records as neighbour lists: {value: [(neighbour, border), ..]} for every value below ``rows``, each list
    in descending border and then ascending neighbour -- its head is the row table's LONGEST.  A value without a neighbour has an
    empty list."""
    graph: dict = {v: [] for v in range(int(rows))}
    for a, b, border, _ in np.asarray(pairs, np.uint32).reshape(-1, _lib.ADJ_PAIR_WORDS).tolist():
        graph.setdefault(a, []).append((b, border))
        graph.setdefault(b, []).append((a, border))
    for v in graph.values():
        v.sort(key=lambda nb: (-nb[1], nb[0]))
    return graph


@dataclass
class SieveCmd:
    """``Sieve``'s command: regions of fewer than ``min_pixels`` pixels are merged; ``max_rounds`` (0: the library's 8, at most
    64); ``pair_slots`` (0: the library's 2^20)."""

    min_pixels: int = 0
    max_rounds: int = 0
    pair_slots: int = 0


class SieveOut:
    """``Sieve``'s ``&mut Output``: what to produce and, after ``advance``, ``klass`` [H, W] u8 (the cleaned plane), ``rows`` [n, 4]
    u32 (``_lib.SIEVE_CLASS`` .. ``_lib.SIEVE_BORDER``), ``counts`` [8] u32 (``_lib.SIEVE_REGIONS`` .. ``_lib.SIEVE_STATUS``); None
    for what was not wanted."""

    def __init__(self, want_klass: bool = True, want_rows: bool = True, want_counts: bool = True):
        self.want_klass, self.want_rows, self.want_counts = want_klass, want_rows, want_counts
        self.klass = self.rows = self.counts = None


class Sieve(Processor):
    """The stage that removes speckle: every region below ``min_pixels`` takes the class of the neighbour it shares the longest
    border with, round by round.

    Command = ``SieveCmd``.  Input = (klass [H, W] u8, labels [H, W] u32, table [rows, 10] u64, n) as ``Regions`` gives them with
    ``min_pixels = 0`` and no background skip; Output = ``SieveOut``.  ``sieve_summary`` names the counts.
    """

    def __init__(self, ctx: Context, min_pixels: int = 0, max_rounds: int = 0, pair_slots: int = 0):
        self.ctx = ctx
        self.min_pixels, self.max_rounds, self.pair_slots = min_pixels, max_rounds, pair_slots
        self.dirty = True

    def control(self, cmd: SieveCmd) -> "Sieve":
        for name in ("min_pixels", "max_rounds", "pair_slots"):
            if not 0 <= getattr(cmd, name) <= 0xFFFFFFFF:
                raise InfurError(_lib.E_INVALID_ARG, f"{name} {getattr(cmd, name)}: a u32")
        new = (cmd.min_pixels, cmd.max_rounds, cmd.pair_slots)
        self.dirty = self.dirty or new != (self.min_pixels, self.max_rounds, self.pair_slots)
        self.min_pixels, self.max_rounds, self.pair_slots = new
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp, out: SieveOut) -> None:
        self.dirty = False
        klass, labels, table, n = inp
        if klass.ndim != 2 or klass.dtype != np.uint8 or labels.shape != klass.shape or labels.dtype != np.uint32:
            raise InfurError(_lib.E_SHAPE, f"expected an [H,W] uint8 class plane and a uint32 label plane of one size, got {klass.shape} "
                                           f"{klass.dtype} and {labels.shape} {labels.dtype}")
        klass, labels = np.ascontiguousarray(klass), np.ascontiguousarray(labels)
        table = np.ascontiguousarray(table, np.uint64).reshape(-1, _lib.REGION_WORDS)
        h, w = klass.shape
        rows = min(int(n), len(table))
        cleaned = np.empty((h, w), np.uint8) if out.want_klass else None
        sieved = np.empty((rows, _lib.SIEVE_ROW_WORDS), np.uint32) if out.want_rows else None
        counts = np.zeros(_lib.SIEVE_COUNT_WORDS, np.uint32) if out.want_counts else None
        ptr = lambda p: p.ctypes.data if p is not None and p.size else None  # noqa: E731
        self.ctx.check(self.ctx.L.infur_sieve(self.ctx.h, ptr(klass), ptr(labels), ptr(table), len(table), int(n), h, w, self.min_pixels,
                                              self.max_rounds, self.pair_slots, ptr(cleaned), ptr(sieved), _ptr(counts)))
        out.klass, out.rows, out.counts = cleaned, sieved, counts


def sieve_summary(counts: np.ndarray) -> dict:
    """``Sieve``'s eight counts by name: ``regions``, ``small``, ``absorbed``, ``stranded``, ``rounds``, ``pixels_changed``,
    ``pairs``, ``status``, and the status bits as ``overflow``, ``rounds_exhausted`` and ``table_short``."""
    c = [int(v) for v in np.asarray(counts).ravel()[:_lib.SIEVE_COUNT_WORDS]]
    status = c[_lib.SIEVE_STATUS]
    return {"regions": c[_lib.SIEVE_REGIONS], "small": c[_lib.SIEVE_SMALL], "absorbed": c[_lib.SIEVE_ABSORBED], "stranded": c[_lib.SIEVE_STRANDED],
            "rounds": c[_lib.SIEVE_ROUNDS], "pixels_changed": c[_lib.SIEVE_PIXELS_CHANGED], "pairs": c[_lib.SIEVE_PAIRS], "status": status,
            "overflow": bool(status & _lib.SIEVE_OVERFLOW), "rounds_exhausted": bool(status & _lib.SIEVE_ROUNDS_EXHAUSTED),
            "table_short": bool(status & _lib.SIEVE_TABLE_SHORT)}


class SieveFrame(NamedTuple):
    """``FramePath.advance_sieve``: the class and confidence planes as decoded and the cleaned class plane [oh, ow] u8 (None where
    not wanted), the label plane, region table and region count of the cleaned plane, Sieve's counts [8] u32, the scaled frame"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    cleaned: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    table: Optional[np.ndarray]
    n: Optional[int]
    counts: Optional[np.ndarray]
    scaled: Optional[np.ndarray]


def runs_decode(runs: np.ndarray, n: int, h: int, w: int, fill: int = 0, dtype=None) -> np.ndarray:
    """The dense [h, w] plane of the first ``min(n, len(runs))`` records; pixels no record covers (skipped or truncated runs) read
    ``fill``.  ``dtype``: uint8 when every value and ``fill`` fit a byte, else uint32."""
    runs = np.asarray(runs, np.uint32).reshape(-1, _lib.RUN_WORDS)[:max(0, int(n))]
    if dtype is None:
        dtype = np.uint8 if fill <= 255 and (len(runs) == 0 or int(runs[:, _lib.RUN_VALUE].max()) <= 255) else np.uint32
    out = np.full(h * w, fill, dtype)
    start, end = runs[:, _lib.RUN_START].astype(np.int64), runs[:, _lib.RUN_END].astype(np.int64)
    if len(runs):  # +v at each start and -v at each end, summed: runs never overlap
        edge = np.zeros(h * w + 1, np.int64)
        cover = np.zeros(h * w + 1, np.int64)
        val = runs[:, _lib.RUN_VALUE].astype(np.int64)
        np.add.at(edge, start, val)
        np.add.at(edge, end, -val)
        np.add.at(cover, start, 1)
        np.add.at(cover, end, -1)
        covered = np.cumsum(cover[:-1]) > 0
        out[covered] = np.cumsum(edge[:-1])[covered].astype(dtype)
    return out.reshape(h, w)


def runs_by_value(runs: np.ndarray, n: int) -> dict:
    """The first ``min(n, len(runs))`` records grouped by value: {value: [k, 2] u32 array of (START, END), in raster order} -- one
    object's (class's, track's) mask as the runs to fill."""
    runs = np.asarray(runs, np.uint32).reshape(-1, _lib.RUN_WORDS)[:max(0, int(n))]
    order = np.argsort(runs[:, _lib.RUN_VALUE], kind="stable")
    vals, first = np.unique(runs[order, _lib.RUN_VALUE], return_index=True)
    parts = np.split(runs[order][:, [_lib.RUN_START, _lib.RUN_END]], first[1:]) if len(vals) else []
    return {int(v): p for v, p in zip(vals, parts)}


@dataclass
class OutlinesCmd:
    """``Outlines``' command: ``Skip(value)`` takes the pixels of that value out of every region (``Skip(None)``: every pixel is
    kept again); ``Connectivity(4 | 8)`` sets the saddle rule -- what Regions was given; ``MaxEdges(n)`` the edge capacity
    (0: the worst case, four per pixel)."""

    skip: Optional[int] = None
    connectivity: Optional[int] = None
    max_edges: Optional[int] = None
    set_skip: bool = False

    @staticmethod
    def Skip(v: Optional[int]) -> "OutlinesCmd":
        return OutlinesCmd(skip=v, set_skip=True)

    @staticmethod
    def Connectivity(k: int) -> "OutlinesCmd":
        return OutlinesCmd(connectivity=k)

    @staticmethod
    def MaxEdges(n: int) -> "OutlinesCmd":
        return OutlinesCmd(max_edges=n)


class OutlinesOut:
    """``Outlines``' ``&mut Output``: what to produce (``loops_rows`` records and ``vertex_rows`` vertices at most) and, after
    ``advance``, the results -- ``loops`` [min(n_loops, loops_rows), 4] u32 (columns ``_lib.LOOP_OFFSET``, ``LOOP_COUNT``,
    ``LOOP_VALUE``, ``LOOP_START``) or None, ``vertices`` [min(n_vertices, vertex_rows)] u32 vertex ids Y*(w+1) + X or None, and
    the full counts ``n_loops``, ``n_vertices``, ``n_edges`` ({0, 0, n_edges} when the edges exceed the capacity)."""

    def __init__(self, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20):
        self.loops_rows, self.vertex_rows = loops_rows, vertex_rows
        self.loops = self.vertices = None
        self.n_loops = self.n_vertices = self.n_edges = 0


def _outlines_flags(skip: Optional[int], connectivity: int) -> int:
    if connectivity not in (4, 8):
        raise InfurError(_lib.E_INVALID_ARG, f"connectivity {connectivity}: 4 or 8")
    return (_lib.OUTLINES_SKIP if skip is not None else 0) | (_lib.OUTLINES_CONN8 if connectivity == 8 else 0)


def _poly_alloc(loops_rows: int, most_loops: int, vertex_rows: int, most_vertices: int) -> tuple:
    """The output arrays of a polygon call, the caller's rows clamped to what there can be -> (loops [lrows, 4] u32, vertices
    [vrows] u32), None where no row is wanted."""
    lrows, vrows = max(0, min(int(loops_rows), most_loops)), max(0, min(int(vertex_rows), most_vertices))
    return np.empty((lrows, _lib.LOOP_WORDS), np.uint32) if lrows else None, np.empty(vrows, np.uint32) if vrows else None


def _poly_rows(a: Optional[np.ndarray]) -> int:
    return len(a) if a is not None else 0


def _poly_slice(loops: Optional[np.ndarray], vertices: Optional[np.ndarray], counts, cut: bool = False) -> tuple:
    """-> (loops[:min(n_loops, rows)], vertices[:min(n_vertices, rows)]); ``cut``: the status says that no record was written"""
    nl, nv = int(counts[0]), int(counts[1])
    return (loops[:0 if cut else min(nl, len(loops))] if loops is not None else None,
            vertices[:min(nv, len(vertices))] if vertices is not None else None)


def _poly_input(loops, vertices, counts) -> tuple:
    """Outlines' results as the input of the stage behind it -> (loops [*, 4] u32, vertices [*] u32, {n_loops, n_vertices} u32)"""
    loops = np.ascontiguousarray(loops if loops is not None else np.zeros((0, _lib.LOOP_WORDS)), np.uint32).reshape(-1, _lib.LOOP_WORDS)
    vertices = np.ascontiguousarray(vertices if vertices is not None else np.zeros(0), np.uint32).reshape(-1)
    return loops, vertices, np.array([int(counts[0]), int(counts[1])], np.uint32)


class Outlines(Processor):
    """The polygon stage: the boundaries of the value-regions of a class plane (u8) or a label / track plane (u32) as closed loops.

    Command = ``OutlinesCmd``.  Input = a plane [H, W] of u8 or u32; Output = ``OutlinesOut``.  Outer loops run clockwise on a
    y-down screen, holes counter-clockwise; integers throughout, identical from run to run.
    """

    def __init__(self, ctx: Context, skip: Optional[int] = None, connectivity: int = 4, max_edges: int = 0):
        self.ctx = ctx
        self.skip, self.connectivity, self.max_edges = skip, connectivity, max_edges
        self.dirty = True

    def control(self, cmd: OutlinesCmd) -> "Outlines":
        skip = cmd.skip if cmd.set_skip else self.skip
        connectivity = cmd.connectivity if cmd.connectivity is not None else self.connectivity
        max_edges = cmd.max_edges if cmd.max_edges is not None else self.max_edges
        if skip is not None and not 0 <= skip <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"skip value {skip}: a u32")
        if connectivity not in (4, 8) or not 0 <= max_edges <= 0xFFFFFFFF:
            raise InfurError(_lib.E_INVALID_ARG, f"connectivity {connectivity}: 4 or 8; max_edges {max_edges}: a u32")
        self.dirty = self.dirty or (skip, connectivity, max_edges) != (self.skip, self.connectivity, self.max_edges)
        self.skip, self.connectivity, self.max_edges = skip, connectivity, max_edges
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: np.ndarray, out: OutlinesOut) -> None:
        self.dirty = False
        if inp.ndim != 2 or inp.dtype.itemsize not in (1, 4) or inp.dtype.kind not in "ui":
            raise InfurError(_lib.E_SHAPE, f"expected an [H,W] plane of 1- or 4-byte integers, got {inp.shape} {inp.dtype}")
        plane = np.ascontiguousarray(inp)
        h, w = plane.shape
        loops, vertices = _poly_alloc(out.loops_rows, h * w, out.vertex_rows, 4 * h * w)
        counts = np.zeros(3, np.uint32)
        self.ctx.check(self.ctx.L.infur_outlines(self.ctx.h, _ptr_some(plane), plane.dtype.itemsize, h, w, _outlines_flags(self.skip, self.connectivity),
                                                 self.skip or 0, self.max_edges, _ptr(loops), _poly_rows(loops), _ptr(vertices), _poly_rows(vertices),
                                                 counts.ctypes.data))
        out.n_loops, out.n_vertices, out.n_edges = (int(v) for v in counts)
        out.loops, out.vertices = _poly_slice(loops, vertices, counts)


class OutlinesFrame(NamedTuple):
    """``FramePath.advance_outlines``: the loop records [min(n_loops, loops_rows), 4] u32 of the class plane, the vertex ids
    [min(n_vertices, vertex_rows)] u32, the counts (n_loops, n_vertices, n_edges), the per-class statistics [k, 8] uint64 or None,
    the scaled BGR frame or None, and the plane's (height, width) -- a vertex id is Y*(width + 1) + X"""

    loops: Optional[np.ndarray]
    vertices: Optional[np.ndarray]
    counts: Optional[tuple]
    stats: Optional[np.ndarray]
    scaled: Optional[np.ndarray]
    shape: tuple


def outlines_polygons(loops: np.ndarray, vertices: np.ndarray, w: int) -> list:
    """The loops whose vertices are all there (a truncated ``vertices`` ends the list) as [(value, is_hole, xy int32 [k, 2])]:
    ``xy`` are the lattice points (x, y) of the closed polygon in order, ``is_hole`` the boundary of a hole (counter-clockwise on a
    y-down screen).  ``w`` is the plane's width."""
    loops = np.asarray(loops, np.uint32).reshape(-1, _lib.LOOP_WORDS)
    vertices = np.asarray(vertices, np.uint32).reshape(-1)
    out = []
    for off, cnt, val, start in loops.tolist():
        if off + cnt > len(vertices):
            break
        ids = vertices[off:off + cnt].astype(np.int64)
        out.append((val, (start & 3) == 2, np.stack([ids % (w + 1), ids // (w + 1)], axis=1).astype(np.int32)))
    return out


def outlines_by_value(loops: np.ndarray, vertices: np.ndarray, w: int) -> dict:
    """``outlines_polygons`` grouped: {value: [(outer xy, [hole xy, ...]), ...]} -- each outer loop with the holes of its value
    that follow it before the value's next outer loop.  On a label or track plane a value is one region, so that a group is one
    object's polygon with its holes (what GeoJSON calls a Polygon); on a class plane, where one value has many regions, a hole is
    listed with the nearest outer loop of its class before it in loop order, which need not be the region it is a hole of."""
    out = {}
    for val, hole, xy in outlines_polygons(loops, vertices, w):
        groups = out.setdefault(int(val), [])
        if hole and groups:
            groups[-1][1].append(xy)
        elif not hole:
            groups.append((xy, []))
    return out


@dataclass
class SimplifyCmd:
    """``Simplify``' command: ``Tolerance(px)`` sets the tolerance in pixels, rounded to sixteenths (``tol16``); ``Tol16(n)`` sets
    the sixteenths themselves."""

    tol16: int = 0

    @staticmethod
    def Tolerance(px: float) -> "SimplifyCmd":
        return SimplifyCmd(tol16=tolerance_to_tol16(px))

    @staticmethod
    def Tol16(n: int) -> "SimplifyCmd":
        return SimplifyCmd(tol16=int(n))


def tolerance_to_tol16(px: float) -> int:
    """a tolerance in pixels -> sixteenths of a pixel, rounded to nearest (half up); what ``segments_cli --outlines-tolerance`` does"""
    t = int(np.floor(float(px) * 16.0 + 0.5))
    if not 0 <= t <= 65535:
        raise InfurError(_lib.E_INVALID_ARG, f"tolerance {px} px: 0 to 4095.9")
    return t


class SimplifyOut:
    """``Simplify``' ``&mut Output``: what to produce (``loops_rows`` records and ``vertex_rows`` vertices at most) and, after
    ``advance``, the results in Outlines' layout -- ``loops`` [min(n_loops, loops_rows), 4] u32 with OFFSET' and COUNT', ``vertices``
    [min(n_vertices, vertex_rows)] u32 -- and the counts ``n_loops``, ``n_vertices``, ``n_degenerate`` (loops with COUNT' < 3: skip
    them) and ``status`` (``_lib.SIMPLIFY_TRUNCATED``: the input was cut off and nothing was produced; ``SIMPLIFY_MALFORMED``)."""

    def __init__(self, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20):
        self.loops_rows, self.vertex_rows = loops_rows, vertex_rows
        self.loops = self.vertices = None
        self.n_loops = self.n_vertices = self.n_degenerate = self.status = 0


class Simplify(Processor):
    """The stage behind Outlines: Douglas-Peucker on every loop, within ``tol16`` sixteenths of a pixel.

    Command = ``SimplifyCmd``.  Input = ``(loops, vertices, counts, (h, w))`` as ``Outlines`` left them (an ``OutlinesOut`` plus the
    plane's shape: ``Simplify.input_of(out, shape)``); Output = ``SimplifyOut``.  ``outlines_polygons`` and ``outlines_by_value``
    read the result as they read Outlines'.  Integers throughout, identical from run to run; topology is not preserved.
    """

    def __init__(self, ctx: Context, tol16: int = 16):
        self.ctx = ctx
        self.tol16 = tol16
        self.dirty = True

    @staticmethod
    def input_of(out: "OutlinesOut", shape: tuple) -> tuple:
        return out.loops, out.vertices, (out.n_loops, out.n_vertices), shape

    def control(self, cmd: SimplifyCmd) -> "Simplify":
        if not 0 <= cmd.tol16 <= 65535:
            raise InfurError(_lib.E_INVALID_ARG, f"tol16 {cmd.tol16}: 0 to 65535")
        self.dirty = self.dirty or cmd.tol16 != self.tol16
        self.tol16 = cmd.tol16
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: tuple, out: SimplifyOut) -> None:
        self.dirty = False
        loops, vertices, counts, (h, w) = inp
        loops, vertices, cin = _poly_input(loops, vertices, counts)
        lo, vo = _poly_alloc(out.loops_rows, len(loops), out.vertex_rows, len(vertices))
        cout = np.zeros(_lib.SIMPLIFY_COUNT_WORDS, np.uint32)
        self.ctx.check(self.ctx.L.infur_simplify(self.ctx.h, _ptr_some(loops), len(loops), _ptr_some(vertices), len(vertices), cin.ctypes.data, h, w,
                                                 self.tol16, _ptr(lo), _poly_rows(lo), _ptr(vo), _poly_rows(vo), cout.ctypes.data))
        out.n_loops, out.n_vertices, out.n_degenerate, out.status = (int(v) for v in cout)
        out.loops, out.vertices = _poly_slice(lo, vo, cout, cut=bool(out.status & _lib.SIMPLIFY_TRUNCATED))


class CoverageOut:
    """``Coverage``'s ``&mut Output``: what to produce (``loops_rows`` records and ``vertex_rows`` vertices at most) and, after
    ``advance``, the results in Outlines' layout -- ``loops`` [min(n_loops, loops_rows), 4] u32 with OFFSET' and COUNT', ``vertices``
    [min(n_vertices, vertex_rows)] u32 -- and the counts ``n_loops``, ``n_vertices``, ``n_degenerate`` (loops with COUNT' < 3: skip
    them), ``status`` (``_lib.COVERAGE_TRUNCATED`` and ``COVERAGE_OVERFLOW``: nothing was produced; ``COVERAGE_MALFORMED``),
    ``n_aug`` (the vertices after the junctions were inserted) and ``n_arcs``."""

    def __init__(self, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20):
        self.loops_rows, self.vertex_rows = loops_rows, vertex_rows
        self.loops = self.vertices = None
        self.n_loops = self.n_vertices = self.n_degenerate = self.status = self.n_aug = self.n_arcs = 0


class Coverage(Processor):
    """Simplify's sibling behind Outlines: the loops are cut at the plane's junctions and every arc is simplified once, within
    ``tol16`` sixteenths of a pixel, so that the polygons of neighbouring regions still share their borders.

    Command = ``SimplifyCmd`` (the tolerance).  Input = ``(plane, loops, vertices, counts, skip)``: the plane Outlines was given,
    what it left, and the value it skipped or None (``Coverage.input_of(plane, out, skip)``); Output = ``CoverageOut``.
    ``outlines_polygons`` and ``outlines_by_value`` read the result as they read Outlines'.  Integers throughout, identical from
    run to run.  ``aug_rows``: the capacity in augmented vertices, 0 for the worst case.
    """

    def __init__(self, ctx: Context, tol16: int = 16, aug_rows: int = 0):
        self.ctx = ctx
        self.tol16 = tol16
        self.aug_rows = aug_rows
        self.dirty = True

    @staticmethod
    def input_of(plane: np.ndarray, out: "OutlinesOut", skip: Optional[int] = None) -> tuple:
        return plane, out.loops, out.vertices, (out.n_loops, out.n_vertices), skip

    def control(self, cmd: SimplifyCmd) -> "Coverage":
        if not 0 <= cmd.tol16 <= 65535:
            raise InfurError(_lib.E_INVALID_ARG, f"tol16 {cmd.tol16}: 0 to 65535")
        self.dirty = self.dirty or cmd.tol16 != self.tol16
        self.tol16 = cmd.tol16
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: tuple, out: CoverageOut) -> None:
        self.dirty = False
        plane, loops, vertices, counts, skip = inp
        plane = np.ascontiguousarray(plane)
        if plane.ndim != 2 or plane.dtype not in (np.uint8, np.uint32):
            raise InfurError(_lib.E_INVALID_ARG, "the plane: [h, w] of uint8 or uint32")
        h, w = plane.shape
        loops, vertices, cin = _poly_input(loops, vertices, counts)
        # junctions are inserted: the output may be longer than the input
        lo, vo = _poly_alloc(out.loops_rows, len(loops), out.vertex_rows, len(vertices) + (h + 1) * (w + 1))
        cout = np.zeros(_lib.COVERAGE_COUNT_WORDS, np.uint32)
        self.ctx.check(self.ctx.L.infur_coverage(self.ctx.h, _ptr_some(plane), plane.itemsize, h, w, _lib.COVERAGE_SKIP if skip is not None else 0,
                                                 skip or 0, _ptr_some(loops), len(loops), _ptr_some(vertices), len(vertices), cin.ctypes.data, self.tol16,
                                                 self.aug_rows, _ptr(lo), _poly_rows(lo), _ptr(vo), _poly_rows(vo), cout.ctypes.data))
        out.n_loops, out.n_vertices, out.n_degenerate, out.status, out.n_aug, out.n_arcs = (int(v) for v in cout)
        out.loops, out.vertices = _poly_slice(lo, vo, cout, cut=bool(out.status & (_lib.COVERAGE_TRUNCATED | _lib.COVERAGE_OVERFLOW)))


class RasterCmd(NamedTuple):
    """``Raster``'s command: the plane's element type (``np.uint8`` or ``np.uint32``) and the value of the pixels no loop paints"""

    dtype: type = np.uint8
    fill_value: int = 0


class RasterOut:
    """``Raster``'s ``&mut Output``: what to produce (``want_plane``) and, after ``advance``, the results -- ``plane`` [h, w] of the
    command's dtype (None when not wanted or when the input was truncated) and the counts ``n`` (loops or records read),
    ``painted`` (pixels exactly one loop claims), ``conflict`` (pixels that were refused and read the fill value: overlapping
    loops, a hole alone, crossed arcs, a value a byte plane cannot hold) and ``status`` (``_lib.RASTER_TRUNCATED``,
    ``RASTER_MALFORMED``, ``RASTER_OUTSIDE``)."""

    def __init__(self, want_plane: bool = True):
        self.want_plane = want_plane
        self.plane = None
        self.n = self.painted = self.conflict = self.status = 0


class Raster(Processor):
    """The stage that goes the other way: the loops of Outlines, Simplify, Coverage or Shapes (its hulls), or the records of Runs,
    filled back into a plane.  A pixel of winding 1 reads its loop's value, every other pixel the fill value.

    Command = ``RasterCmd``.  Input = ``(loops, vertices, counts, (h, w))`` (``Simplify.input_of``) or ``(runs, n, (h, w))``;
    Output = ``RasterOut``.  ``Raster(Outlines(plane)) == plane`` and ``Raster(Runs(plane)) == plane`` with the fill value = the
    skipped value.  Integers throughout, identical from run to run.
    """

    def __init__(self, ctx: Context, dtype=np.uint8, fill_value: int = 0):
        self.ctx = ctx
        self.dtype, self.fill_value = np.dtype(np.uint8), 0
        self.dirty = True
        self.control(RasterCmd(dtype, fill_value))

    def control(self, cmd: RasterCmd) -> "Raster":
        dtype = np.dtype(cmd.dtype)
        if dtype not in (np.dtype(np.uint8), np.dtype(np.uint32)):
            raise InfurError(_lib.E_INVALID_ARG, f"dtype {dtype}: uint8 or uint32")
        if not 0 <= cmd.fill_value <= (255 if dtype.itemsize == 1 else 0xFFFFFFFF):
            raise InfurError(_lib.E_INVALID_ARG, f"fill_value {cmd.fill_value}: a {dtype} plane cannot hold it")
        self.dirty = self.dirty or (dtype, cmd.fill_value) != (self.dtype, self.fill_value)
        self.dtype, self.fill_value = dtype, int(cmd.fill_value)
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: tuple, out: RasterOut) -> None:
        self.dirty = False
        (h, w) = inp[-1]
        plane = np.empty((h, w), self.dtype) if out.want_plane else None
        cout = np.zeros(_lib.RASTER_COUNT_WORDS, np.uint32)
        if len(inp) == 4:
            loops, vertices, cin = _poly_input(*inp[:3])
            rc = self.ctx.L.infur_raster(self.ctx.h, _ptr_some(loops), len(loops), _ptr_some(vertices), len(vertices), cin.ctypes.data, h, w,
                                         self.dtype.itemsize, self.fill_value, _ptr(plane), cout.ctypes.data)
        else:
            runs = np.ascontiguousarray(inp[0] if inp[0] is not None else np.zeros((0, _lib.RUN_WORDS)), np.uint32).reshape(-1, _lib.RUN_WORDS)
            rc = self.ctx.L.infur_raster_runs(self.ctx.h, _ptr_some(runs), len(runs), int(inp[1]), h, w, self.dtype.itemsize, self.fill_value,
                                              _ptr(plane), cout.ctypes.data)
        self.ctx.check(rc)
        out.n, out.painted, out.conflict, out.status = (int(v) for v in cout)
        out.plane = None if out.status & _lib.RASTER_TRUNCATED else plane


def polygon_fidelity(ctx: Context, plane: np.ndarray, tol16: int, shared: bool = False, connectivity: int = 4, skip: Optional[int] = None,
                     rows: int = 21) -> dict:
    """What a tolerance costs, in pixels: Outlines -> Simplify (``shared=False``) or Coverage (``shared=True``) at ``tol16`` -> Raster
    -> Compare against ``plane`` itself, all through the ``_dev`` calls on device buffers: the plane goes up once and a few dozen
    words come back.  ``skip``: the value that belongs to no region (Outlines' and Coverage's SKIP); it is Raster's fill value.
    Without one the fill value is the largest the plane's type holds, which the plane should not use.  A diagnostic: every call
    allocates and frees its twelve device buffers (about 48 bytes per pixel, 100 MB at 1080p) and synchronises once.  ``rows``: the values the
    confusion matrix has room for.  ->

    * ``vertices_in``, ``vertices_out``: the vertices Outlines wrote and the stage behind it kept;
    * ``changed``: the pixels of the re-filled plane that differ from ``plane``;
    * ``conflict``: the pixels several polygons claim, or a hole alone, or crossed arcs (Raster's CONFLICT);
    * ``uncovered``: the pixels no polygon claims beyond those ``plane`` skips (Raster's OUTSIDE pixels less the skipped ones: a
      skipped pixel that a simplified polygon paints counts against it);
    * ``pixel_accuracy``, ``miou``: ``confusion_summary`` of the matrix plane (rows) against re-filled plane (columns).  A pixel
      that reads the fill value lies outside the matrix when the fill value is at or above ``rows``: the two measures are then
      over the painted pixels alone, and ``changed`` is the figure that counts every pixel."""
    plane = np.ascontiguousarray(plane)
    if plane.ndim != 2 or plane.dtype not in (np.dtype(np.uint8), np.dtype(np.uint32)) or not plane.size:
        raise InfurError(_lib.E_SHAPE, f"expected a non-empty [H,W] plane of uint8 or uint32, got {plane.shape} {plane.dtype}")
    L, h, w, elem = ctx.L, plane.shape[0], plane.shape[1], plane.dtype.itemsize
    npix = h * w
    flags = _outlines_flags(skip, connectivity)
    fill = int(skip) if skip is not None else (255 if elem == 1 else 0xFFFFFFFF)
    most_v = 4 * npix + (w + 1) * (h + 1)  # Coverage adds the lattice's junctions
    sizes = {"plane": plane.nbytes, "loops": npix * 16, "vertices": 4 * npix * 4, "counts": 16, "loops2": npix * 16, "vertices2": most_v * 4,
             "counts2": 32, "filled": plane.nbytes, "rcounts": 16, "matrix": max(rows * rows, 1) * 4, "ccounts": _lib.COMPARE_COUNT_WORDS * 4,
             "icounts": _lib.COMPARE_COUNT_WORDS * 4}
    d = {}
    try:
        for name, n in sizes.items():
            p = C.c_void_p(None)
            ctx.check(L.infur_dev_alloc(ctx.h, n, C.byref(p)))
            d[name] = p
        ctx.check(L.infur_memcpy_h2d(ctx.h, d["plane"], plane.ctypes.data, plane.nbytes))
        ctx.check(L.infur_outlines_dev(ctx.h, d["plane"], elem, h, w, flags, skip or 0, 0, d["loops"], npix, d["vertices"], 4 * npix, d["counts"]))
        if shared:
            ctx.check(L.infur_coverage_dev(ctx.h, d["plane"], elem, h, w, _lib.COVERAGE_SKIP if skip is not None else 0, skip or 0, d["loops"], npix,
                                           d["vertices"], 4 * npix, d["counts"], tol16, 0, d["loops2"], npix, d["vertices2"], most_v, d["counts2"]))
        else:
            ctx.check(L.infur_simplify_dev(ctx.h, d["loops"], npix, d["vertices"], 4 * npix, d["counts"], h, w, tol16, d["loops2"], npix,
                                           d["vertices2"], most_v, d["counts2"]))
        ctx.check(L.infur_raster_dev(ctx.h, d["loops2"], npix, d["vertices2"], most_v, d["counts2"], h, w, elem, fill, d["filled"], d["rcounts"]))
        ctx.check(L.infur_compare_dev(ctx.h, d["plane"], elem, d["filled"], elem, h, w, 0, 0, 0, d["matrix"] if rows else None, rows, rows, None, None,
                                      d["ccounts"], 0))
        ctx.check(L.infur_compare_dev(ctx.h, d["plane"], elem, d["filled"], elem, h, w, _lib.COMPARE_IGNORE_A if skip is not None else 0, skip or 0, 0,
                                      None, 0, 0, None, None, d["icounts"], 0))
        ctx.synchronize()

        def words(name, n):
            out = np.empty(n, np.uint32)
            ctx.check(L.infur_memcpy_d2h(ctx.h, out.ctypes.data, d[name], out.nbytes))
            return out

        cin, cout, rc = words("counts", 3), words("counts2", 4), words("rcounts", 4)
        cc, ic = words("ccounts", _lib.COMPARE_COUNT_WORDS), words("icounts", _lib.COMPARE_COUNT_WORDS)
        matrix = words("matrix", rows * rows).reshape(rows, rows) if rows else np.zeros((0, 0), np.uint32)
    finally:
        for p in d.values():
            L.infur_dev_free(ctx.h, p)
    summary = confusion_summary(matrix, names=lambda k: None)
    painted, conflict = int(rc[_lib.RASTER_PAINTED]), int(rc[_lib.RASTER_CONFLICT])
    return {"vertices_in": int(cin[1]), "vertices_out": int(cout[1]), "changed": int(cc[_lib.COMPARE_COMPARED]) - int(cc[_lib.COMPARE_EQUAL]),
            "conflict": conflict, "uncovered": npix - painted - conflict - int(ic[_lib.COMPARE_IGNORED]), "status": int(rc[_lib.RASTER_STATUS]),
            "pixel_accuracy": summary["pixel_accuracy"], "miou": summary["miou"]}


class ShapesOut:
    """``Shapes``' ``&mut Output``: what to produce (``loops_rows`` hull records, ``vertex_rows`` hull vertices, ``shape_rows`` per-loop
    records and ``value_rows`` per-value rows at most; 0 = not wanted) and, after ``advance``, the results -- ``loops`` and
    ``vertices``, the hulls in Outlines' layout; ``shapes`` [min(n_loops, shape_rows), ``_lib.SHAPE_WORDS``] int64 (columns
    ``_lib.SHAPE_AREA2`` .. ``SHAPE_RECT_L``); ``values`` [value_rows, ``_lib.SHAPE_WORDS``] int64 (columns 8 .. 10 are
    ``SHAPE_OUTER``, ``SHAPE_HOLES``, ``SHAPE_LOOP``), every row written -- and the counts ``n_loops``, ``n_vertices`` (hull
    vertices), ``status`` (``_lib.SHAPES_TRUNCATED``: the input was cut off; ``SHAPES_MALFORMED``) and ``largest`` (the largest
    COUNT')."""

    def __init__(self, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20, shape_rows: int = 1 << 16, value_rows: int = 0):
        self.loops_rows, self.vertex_rows, self.shape_rows, self.value_rows = loops_rows, vertex_rows, shape_rows, value_rows
        self.loops = self.vertices = self.shapes = self.values = None
        self.n_loops = self.n_vertices = self.status = self.largest = 0


def _shape_rows(rows: int) -> Optional[np.ndarray]:
    return np.empty((rows, _lib.SHAPE_WORDS), np.int64) if rows > 0 else None


class Shapes(Processor):
    """The descriptor stage behind Outlines: per loop the area, perimeter and moments, the convex hull and the minimum rectangle;
    per value the sums.

    No command (``control(None)``).  Input = ``(loops, vertices, counts, (h, w))`` as ``Outlines`` left them
    (``Shapes.input_of(out, shape)``); Output = ``ShapesOut``.  ``outlines_polygons`` reads the hulls as it reads Outlines' loops;
    ``shape_summary`` turns a row into floats.  Integers throughout, identical from run to run.
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.dirty = True

    @staticmethod
    def input_of(out: "OutlinesOut", shape: tuple) -> tuple:
        return out.loops, out.vertices, (out.n_loops, out.n_vertices), shape

    def control(self, cmd=None) -> "Shapes":
        return self

    def is_dirty(self) -> bool:
        return self.dirty

    def advance(self, inp: tuple, out: ShapesOut) -> None:
        self.dirty = False
        loops, vertices, counts, (h, w) = inp
        loops, vertices, cin = _poly_input(loops, vertices, counts)
        lo, vo = _poly_alloc(out.loops_rows, len(loops), out.vertex_rows, len(vertices))
        shapes, values = _shape_rows(min(int(out.shape_rows), len(loops))), _shape_rows(int(out.value_rows))
        cout = np.zeros(_lib.SHAPES_COUNT_WORDS, np.uint32)
        self.ctx.check(self.ctx.L.infur_shapes(self.ctx.h, _ptr_some(loops), len(loops), _ptr_some(vertices), len(vertices), cin.ctypes.data, h, w,
                                               _ptr(lo), _poly_rows(lo), _ptr(vo), _poly_rows(vo), _ptr(shapes), _poly_rows(shapes), _ptr(values),
                                               _poly_rows(values), cout.ctypes.data))
        out.n_loops, out.n_vertices, out.status, out.largest = (int(v) for v in cout)
        cut = bool(out.status & _lib.SHAPES_TRUNCATED)
        out.loops, out.vertices = _poly_slice(lo, vo, cout, cut=cut)
        out.shapes = shapes[:0 if cut else min(out.n_loops, len(shapes))] if shapes is not None else None
        out.values = values


def shape_summary(measures, rect=None, hull=None) -> dict:
    """Floats on the host from the integers of Shapes.  ``measures``: a per-loop record or a per-value row (their first eight words
    agree).  -> ``area`` (pixels), ``perimeter``, ``centroid`` (x, y) in pixel-centre coordinates, ``orientation`` (radians from
    the x axis towards y, 1/2 atan2(2 mu11, mu20 - mu02)), ``major`` and ``minor`` (the axes of the ellipse with the same second
    moments), ``eccentricity``, ``solidity`` (AREA2 / HULL_AREA2) and ``compactness`` (4 pi A / P^2; 1 for a disc in the continuum).
    ``rect``: a per-loop record (for a value: ``shapes[row[SHAPE_LOOP]]``) adds ``rect_sides`` (along the edge, across it) and
    ``rect_angle`` (of the edge); with ``hull`` as well, the xy [k, 2] of that loop's hull, also ``rect_centre`` in pixel-centre
    coordinates.  The central moments are formed in exact integers and divided once.  None for a row without area."""
    m = [int(v) for v in np.asarray(measures).reshape(-1)[:8]]
    a2, per, m10, m01, m20, m02, m11, hull2 = m
    if a2 == 0:
        return None
    mu20 = (3 * m20 * a2 - 2 * m10 * m10) / (36 * a2)
    mu02 = (3 * m02 * a2 - 2 * m01 * m01) / (36 * a2)
    mu11 = (3 * m11 * a2 - 4 * m10 * m01) / (72 * a2)
    area = a2 / 2
    root = float(np.hypot(mu20 - mu02, 2 * mu11))
    big, small = (mu20 + mu02 + root) / (2 * area), max((mu20 + mu02 - root) / (2 * area), 0.0)
    out = {"area": area, "perimeter": float(per), "centroid": (m10 / (3 * a2) - 0.5, m01 / (3 * a2) - 0.5),
           "orientation": 0.5 * float(np.arctan2(2 * mu11, mu20 - mu02)), "major": 4 * float(np.sqrt(big)), "minor": 4 * float(np.sqrt(small)),
           "eccentricity": float(np.sqrt(1 - small / big)) if big > 0 else 0.0, "solidity": a2 / hull2 if hull2 else None,
           "compactness": 4 * float(np.pi) * abs(area) / (per * per) if per else None}
    if rect is not None:
        r = [int(v) for v in np.asarray(rect).reshape(-1)]
        j, rw, rh, rl = (r[k] for k in (_lib.SHAPE_RECT_EDGE, _lib.SHAPE_RECT_W, _lib.SHAPE_RECT_H, _lib.SHAPE_RECT_L))
        if rl:
            out["rect_sides"] = (rw / float(np.sqrt(rl)), rh / float(np.sqrt(rl)))
            if hull is not None:
                xy = np.asarray(hull, np.float64).reshape(-1, 2)
                e = xy[(j + 1) % len(xy)] - xy[j]
                u = e / np.sqrt(rl)
                n = np.array([-u[1], u[0]])
                along, across = xy[:, 0] * u[0] + xy[:, 1] * u[1], xy[:, 0] * n[0] + xy[:, 1] * n[1]  # (elementwise: no layout-dependent summation)
                c = u * (along.min() + along.max()) / 2 + n * (across.min() + across.max()) / 2 - 0.5
                out["rect_angle"] = float(np.arctan2(e[1], e[0]))
                out["rect_centre"] = (float(c[0]), float(c[1]))
    return out


class ShapesFrame(NamedTuple):
    """``FramePath.advance_shapes``: ``RegionsFrame``'s fields, then the hull records and vertex ids in Outlines' layout, the
    per-loop records [min(n_loops, shape_rows), 12] int64, the per-region rows [table_rows, 12] int64 (row i is region i), the
    counts (n_loops, n_hull_vertices, status, largest COUNT') and the plane's (height, width)"""

    klass: Optional[np.ndarray]
    conf: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    table: Optional[np.ndarray]
    n_regions: Optional[int]
    scaled: Optional[np.ndarray]
    loops: Optional[np.ndarray]
    vertices: Optional[np.ndarray]
    shapes: Optional[np.ndarray]
    values: Optional[np.ndarray]
    counts: Optional[tuple]
    shape: tuple


class PolygonsFrame(NamedTuple):
    """``FramePath.advance_polygons``: ``OutlinesFrame`` with simplified loops, and the counts (n_loops, n_vertices, n_degenerate,
    status)"""

    loops: Optional[np.ndarray]
    vertices: Optional[np.ndarray]
    counts: Optional[tuple]
    stats: Optional[np.ndarray]
    scaled: Optional[np.ndarray]
    shape: tuple


def pack_normalize(ctx: Context, img: np.ndarray) -> np.ndarray:
    """The pre-proc stage on its own (predict_onnx.rs:103-137): BGR u8 HWC -> RGB f32 CHW."""
    img = _check_bgr(img)
    h, w = img.shape[:2]
    out = np.empty((3, h, w), np.float32)
    ctx.check(ctx.L.infur_pack_normalize(ctx.h, img.ctypes.data, w, h, out.ctypes.data))
    return out


# --------------------------------------------------------------------------- #
# the fused per-frame path (what ProcessingApp::advance does per frame, app.rs:107-153)
# --------------------------------------------------------------------------- #
class FramePath:
    """scale -> model -> decode(out[0]) in one call, nothing materialised at full resolution."""

    def __init__(self, ctx: Context, scale_mode: int = _lib.SCALE_NEAREST):
        self.ctx = ctx
        self.scale_mode = scale_mode

    # ---- what every fused call shares ----
    def _front(self, img: np.ndarray, factor: float):
        """The checked frame, its width and height, the factor as the float32 the library sees, and the scaled dimensions (two
        ``c_uint32``, which the call then writes) -> (img, w, h, f, ow, oh)."""
        img = _check_bgr(img)
        h, w = img.shape[:2]
        f = float(np.float32(factor))
        rc = self.ctx.L.infur_scale_validate(f)
        if rc:
            raise ValidScaleError(rc)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        rc = self.ctx.L.infur_scale_out_dims(w, h, f, C.byref(ow), C.byref(oh))
        if rc:
            raise ScaleProcError(rc)
        return img, w, h, f, ow, oh

    def _num_classes(self) -> int:
        """the loaded model's class count, 0 without a model"""
        mi = _lib.ModelInfoC()
        return mi.num_classes if self.ctx.L.infur_model_info_get(self.ctx.h, C.byref(mi)) == _lib.OK else 0

    @staticmethod
    def _plane(ow, oh, want: bool, dtype=np.uint8, channels: int = 0) -> Optional[np.ndarray]:
        """an optional output of the scaled frame's size: [oh, ow] or [oh, ow, channels]"""
        return np.empty((oh.value, ow.value) + ((channels,) if channels else ()), dtype) if want else None

    @staticmethod
    def _stats(k: int, want: bool) -> Optional[np.ndarray]:
        return np.zeros((k, _lib.STAT_WORDS), np.uint64) if want else None

    def _loaded(self, rc: int) -> bool:
        """The no-model rule: False when the call found no model -- the Scale stage has run, every result but ``scaled`` is None
        (the mask is cleared, app.rs:127-129); any other failure raises."""
        if rc == _lib.E_MODEL_NOT_LOADED:
            return False
        self.ctx.check(rc)
        return True

    def advance(self, img: np.ndarray, factor: float = 1.0, want_scaled: bool = False):
        """-> (rgba [oh,ow,4] u8 or None when no model is loaded, scaled BGR or None)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        rgba = self._plane(ow, oh, True, channels=4)
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        rc = self.ctx.L.infur_frame_advance(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, rgba.ctypes.data, rgba.nbytes, _ptr(scaled),
                                            C.byref(ow), C.byref(oh))
        return (rgba if self._loaded(rc) else None), scaled

    def advance_segments(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, want_rgba: bool = False,
                         want_scaled: bool = False, want_klass: bool = True, want_conf: bool = True,
                         want_stats: bool = True) -> SegmentsFrame:
        """The same fused path with the Segments decode instead of ColorCode -> ``SegmentsFrame``; every result field is None
        when no model is loaded (``scaled`` is still produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        k = self._num_classes()
        klass, conf = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf)
        stats = self._stats(k, want_stats)
        rgba, scaled = self._plane(ow, oh, want_rgba, channels=4), self._plane(ow, oh, want_scaled, channels=3)
        rc = self.ctx.L.infur_frame_segments(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, _ptr(klass), _ptr(conf),
                                             oh.value * ow.value, _ptr(stats), k, _ptr(rgba), rgba.nbytes if want_rgba else 0, _ptr(scaled),
                                             C.byref(ow), C.byref(oh))
        if not self._loaded(rc):
            return SegmentsFrame(None, None, None, None, scaled)
        return SegmentsFrame(klass, conf, stats, rgba, scaled)

    def advance_regions(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, connectivity: int = _lib.CONNECT_8,
                        min_pixels: int = 0, flags: int = 0, table_rows: int = 1024, want_labels: bool = True, want_klass: bool = True,
                        want_conf: bool = True, want_scaled: bool = False) -> RegionsFrame:
        """The fused path with both decode stages, scale -> model -> Segments decode -> Regions, in one call -> ``RegionsFrame``;
        every result field is None when no model is loaded (``scaled`` is still produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        npix = oh.value * ow.value
        rows = max(0, min(int(table_rows), npix))
        klass, conf = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf)
        labels = self._plane(ow, oh, want_labels, np.uint32)
        table = np.zeros((rows, _lib.REGION_WORDS), np.uint64) if rows else None
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        n = C.c_uint32(0)
        rc = self.ctx.L.infur_frame_regions(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, connectivity, min_pixels, flags,
                                            _ptr(klass), _ptr(conf), npix, _ptr(labels), npix * 4, _ptr(table), rows, C.addressof(n), _ptr(scaled),
                                            C.byref(ow), C.byref(oh))
        if not self._loaded(rc):
            return RegionsFrame(None, None, None, None, None, scaled)
        return RegionsFrame(klass, conf, labels, table[:min(n.value, rows)] if table is not None else None, n.value, scaled)

    def advance_anchors(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, connectivity: int = _lib.CONNECT_8,
                        min_pixels: int = 0, flags: int = 0, table_rows: int = 1024, want_labels: bool = True, want_klass: bool = True,
                        want_conf: bool = True, want_scaled: bool = False, want_dist2: bool = True) -> AnchorsFrame:
        """The fused path with an anchor per object, scale -> model -> Segments decode -> Regions -> Anchors of the label plane, in
        one call -> ``AnchorsFrame``; every result field is None when no model is loaded (``scaled`` is still produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        npix = oh.value * ow.value
        rows = max(0, min(int(table_rows), npix))
        klass, conf = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf)
        labels = self._plane(ow, oh, want_labels, np.uint32)
        table = np.zeros((rows, _lib.REGION_WORDS), np.uint64) if rows else None
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        dist2 = self._plane(ow, oh, want_dist2, np.uint32)
        anchors = np.empty((rows, _lib.ANCHOR_WORDS), np.uint32) if rows else None
        n = C.c_uint32(0)
        rc = self.ctx.L.infur_frame_anchors(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, connectivity, min_pixels, flags,
                                            _ptr(klass), _ptr(conf), npix, _ptr(labels), npix * 4, _ptr(table), rows, C.addressof(n), _ptr(scaled),
                                            C.byref(ow), C.byref(oh), _ptr(dist2), npix * 4, _ptr(anchors))
        if not self._loaded(rc):
            return AnchorsFrame(None, None, None, None, None, scaled, None, None)
        k = min(n.value, rows)
        return AnchorsFrame(klass, conf, labels, table[:k] if table is not None else None, n.value, scaled, dist2,
                            anchors[:k] if anchors is not None else None)

    def advance_shapes(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, connectivity: int = _lib.CONNECT_8,
                       min_pixels: int = 0, flags: int = 0, table_rows: int = 1024, max_edges: int = 0, loops_rows: int = 1 << 16,
                       vertex_rows: int = 1 << 20, shape_rows: int = 1 << 16, want_labels: bool = False, want_klass: bool = False,
                       want_conf: bool = False, want_scaled: bool = False) -> ShapesFrame:
        """The fused path with a descriptor per object, scale -> model -> Segments decode -> Regions -> Outlines of the label plane
        -> Shapes, in one call -> ``ShapesFrame``; every result field is None when no model is loaded (``scaled`` is still
        produced).  No dense plane crosses PCIe unless it is asked for."""
        img, w, h, f, ow, oh = self._front(img, factor)
        npix = oh.value * ow.value
        rows = max(0, min(int(table_rows), npix))
        klass, conf = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf)
        labels = self._plane(ow, oh, want_labels, np.uint32)
        table = np.zeros((rows, _lib.REGION_WORDS), np.uint64) if rows else None
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        lo, vo = _poly_alloc(loops_rows, npix, vertex_rows, 4 * npix)
        shapes, values = _shape_rows(max(0, min(int(shape_rows), npix))), _shape_rows(rows)
        counts = np.zeros(_lib.SHAPES_COUNT_WORDS, np.uint32)
        n = C.c_uint32(0)
        rc = self.ctx.L.infur_frame_shapes(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, connectivity, min_pixels, flags,
                                           _ptr(klass), _ptr(conf), npix, _ptr(labels), npix * 4, _ptr(table), rows, C.addressof(n), _ptr(scaled),
                                           C.byref(ow), C.byref(oh), max_edges, _ptr(lo), _poly_rows(lo), _ptr(vo), _poly_rows(vo), _ptr(shapes),
                                           _poly_rows(shapes), _ptr(values), counts.ctypes.data)
        shape = (oh.value, ow.value)
        if not self._loaded(rc):
            return ShapesFrame(None, None, None, None, None, scaled, None, None, None, None, None, shape)
        k = min(n.value, rows)
        lo, vo = _poly_slice(lo, vo, counts)
        return ShapesFrame(klass, conf, labels, table[:k] if table is not None else None, n.value, scaled, lo, vo,
                           shapes[:min(int(counts[0]), len(shapes))] if shapes is not None else None, values, tuple(int(v) for v in counts), shape)

    def advance_compare(self, img: np.ndarray, truth: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW,
                        ignore: Optional[int] = None, rows_a: Optional[int] = None, rows_b: Optional[int] = None, pair_slots: int = 0,
                        want_matrix: bool = True, want_rows: bool = True, want_counts: bool = True, want_klass: bool = False,
                        want_conf: bool = False, want_scaled: bool = False) -> CompareFrame:
        """The fused path with a grade, scale -> model -> Segments decode -> Compare of the class plane against ``truth`` ([oh, ow]
        u8; pixels of ``ignore`` are not compared), in one call -> ``CompareFrame``; ``rows_a`` and ``rows_b`` default to the
        model's class count.  Every result field is None when no model is loaded (``scaled`` is still produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        npix = oh.value * ow.value
        truth = np.ascontiguousarray(truth)
        if truth.dtype != np.uint8 or truth.shape != (oh.value, ow.value):
            raise InfurError(_lib.E_SHAPE, f"expected a [{oh.value},{ow.value}] uint8 truth plane, got {truth.shape} {truth.dtype}")
        k = self._num_classes()
        rows_a, rows_b = k if rows_a is None else max(0, int(rows_a)), k if rows_b is None else max(0, int(rows_b))
        klass, conf = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf)
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        matrix, ra, rb, counts = _compare_alloc(rows_a, rows_b, want_matrix, want_rows, want_counts)
        rc = self.ctx.L.infur_frame_compare(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, _lib.COMPARE_IGNORE_B if ignore is not None else 0,
                                            ignore or 0, _ptr(truth), truth.size, _ptr(klass), _ptr(conf), npix, _ptr(matrix), rows_a, rows_b, _ptr(ra),
                                            _ptr(rb), _ptr(counts), pair_slots, _ptr(scaled), C.byref(ow), C.byref(oh))
        if not self._loaded(rc):
            return CompareFrame(None, None, scaled, None, None, None, None)
        return CompareFrame(klass, conf, scaled, matrix, ra, rb, counts)

    def advance_sieve(self, img: np.ndarray, min_pixels: int, factor: float = 1.0, decode: int = _lib.DECODE_RAW,
                      connectivity: int = _lib.CONNECT_8, flags: int = 0, table_rows: int = 1024, max_rounds: int = 0, pair_slots: int = 0,
                      want_labels: bool = True, want_klass: bool = False, want_conf: bool = True, want_cleaned: bool = True,
                      want_scaled: bool = False) -> SieveFrame:
        """The fused path with a cleaned class plane, scale -> model -> Segments decode -> Regions -> Sieve (regions below
        ``min_pixels`` merged into their neighbours) -> Regions of the cleaned plane (``flags``; only with ``want_labels`` or
        ``table_rows``, ``n`` is None otherwise), in one call -> ``SieveFrame``; every result field is None when no model is
        loaded (``scaled`` is still produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        npix = oh.value * ow.value
        rows = max(0, min(int(table_rows), npix))
        klass, conf, cleaned = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf), self._plane(ow, oh, want_cleaned)
        labels = self._plane(ow, oh, want_labels, np.uint32)
        table = np.zeros((rows, _lib.REGION_WORDS), np.uint64) if rows else None
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        counts = np.zeros(_lib.SIEVE_COUNT_WORDS, np.uint32)
        n = C.c_uint32(0)
        again = want_labels or rows > 0  # the regions of the cleaned plane: a second Regions pass, only when something of it is wanted
        rc = self.ctx.L.infur_frame_sieve(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, connectivity, min_pixels, flags, _ptr(klass),
                                          _ptr(conf), npix, _ptr(labels), npix * 4, _ptr(table), rows, C.addressof(n) if again else None, _ptr(scaled),
                                          C.byref(ow), C.byref(oh), max_rounds, pair_slots, _ptr(cleaned), counts.ctypes.data)
        if not self._loaded(rc):
            return SieveFrame(None, None, None, None, None, None, None, scaled)
        return SieveFrame(klass, conf, cleaned, labels, table[:min(n.value, rows)] if table is not None else None, n.value if again else None, counts,
                          scaled)

    def advance_tracks(self, tracks: "Tracks", img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW,
                       connectivity: int = _lib.CONNECT_8, min_pixels: int = 0, flags: int = 0, table_rows: int = 1024,
                       want_labels: bool = True, want_klass: bool = True, want_conf: bool = True, want_scaled: bool = False,
                       want_plane: bool = False) -> TracksFrame:
        """The fused path with all three decode stages, scale -> model -> Segments decode -> Regions -> Tracks, in one call ->
        ``TracksFrame``; every result field is None when no model is loaded (``scaled`` is still produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        npix = oh.value * ow.value
        rows = max(0, min(int(table_rows), npix))
        klass, conf = self._plane(ow, oh, want_klass), self._plane(ow, oh, want_conf)
        labels = self._plane(ow, oh, want_labels, np.uint32)
        table = np.zeros((rows, _lib.REGION_WORDS), np.uint64) if rows else None
        scaled = self._plane(ow, oh, want_scaled, channels=3)
        tor = np.empty(rows, np.uint32) if rows else None
        ttab = np.empty((rows, _lib.TRACK_WORDS), np.uint64) if rows else None
        plane = self._plane(ow, oh, want_plane, np.uint32)
        summary = np.zeros(_lib.TRACKS_SUMMARY_WORDS, np.uint32)
        n = C.c_uint32(0)
        rc = self.ctx.L.infur_frame_tracks(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, connectivity, min_pixels, flags,
                                           _ptr(klass), _ptr(conf), npix, _ptr(labels), npix * 4, _ptr(table), rows, C.addressof(n), _ptr(scaled),
                                           C.byref(ow), C.byref(oh), tracks.t, tracks.min_overlap, _ptr(tor), _ptr(plane), _ptr(ttab),
                                           summary.ctypes.data)
        if not self._loaded(rc):
            return TracksFrame(None, None, None, None, None, scaled, None, None, None, None)
        k = min(n.value, rows)
        gap, memory = tracks.memory(k)
        return TracksFrame(klass, conf, labels, table[:k] if table is not None else None, n.value, scaled,
                           tor[:k] if tor is not None else None, ttab[:k] if ttab is not None else None, plane, summary, gap, memory)

    def advance_runs(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, skip: Optional[int] = None,
                     runs_rows: int = 1 << 16, want_row_start: bool = True, want_stats: bool = True,
                     want_scaled: bool = False) -> RunsFrame:
        """The fused path with the class plane run-length encoded, scale -> model -> Segments decode -> Runs, in one call ->
        ``RunsFrame``: no dense plane crosses PCIe.  Every result field is None when no model is loaded (``scaled`` is still
        produced)."""
        img, w, h, f, ow, oh = self._front(img, factor)
        k = self._num_classes()
        rows = max(0, min(int(runs_rows), oh.value * ow.value))
        runs = np.empty((rows, _lib.RUN_WORDS), np.uint32) if rows else None
        row_start = np.empty(oh.value + 1, np.uint32) if want_row_start else None
        stats, scaled = self._stats(k, want_stats), self._plane(ow, oh, want_scaled, channels=3)
        n = C.c_uint32(0)
        rc = self.ctx.L.infur_frame_runs(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, _lib.RUNS_SKIP if skip is not None else 0,
                                         skip or 0, _ptr(runs), rows, _ptr(row_start), oh.value + 1, C.addressof(n), _ptr(stats), k, _ptr(scaled),
                                         C.byref(ow), C.byref(oh))
        if not self._loaded(rc):
            return RunsFrame(None, None, None, None, scaled)
        return RunsFrame(runs[:min(n.value, rows)] if runs is not None else None, row_start, n.value, stats, scaled)

    def advance_outlines(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, skip: Optional[int] = None,
                         connectivity: int = 4, max_edges: int = 0, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20,
                         want_stats: bool = True, want_scaled: bool = False) -> OutlinesFrame:
        """The fused path with the class plane outlined, scale -> model -> Segments decode -> Outlines, in one call ->
        ``OutlinesFrame``: no dense plane crosses PCIe.  Every result field is None when no model is loaded (``scaled`` is still
        produced)."""
        return self._advance_poly("infur_frame_outlines", OutlinesFrame, 3, False, (), img, factor, decode, skip, connectivity, max_edges, loops_rows,
                                  vertex_rows, want_stats, want_scaled)

    def _advance_poly(self, symbol: str, result, count_words: int, lattice: bool, tol: tuple, img, factor, decode, skip, connectivity, max_edges,
                      loops_rows, vertex_rows, want_stats, want_scaled):
        """The body of the three polygon calls: ``symbol`` with ``count_words`` counts -> ``result``.  ``lattice``: the vertices may
        include the lattice's junctions (Coverage); ``tol``: the arguments between ``max_edges`` and the outputs.  The slices
        follow the counts alone, whatever the status word says."""
        img, w, h, f, ow, oh = self._front(img, factor)
        k = self._num_classes()
        npix = oh.value * ow.value
        loops, vertices = _poly_alloc(loops_rows, npix, vertex_rows, 4 * npix + ((oh.value + 1) * (ow.value + 1) if lattice else 0))
        counts = np.zeros(count_words, np.uint32)
        stats, scaled = self._stats(k, want_stats), self._plane(ow, oh, want_scaled, channels=3)
        rc = getattr(self.ctx.L, symbol)(self.ctx.h, img.ctypes.data, w, h, f, self.scale_mode, decode, _outlines_flags(skip, connectivity), skip or 0,
                                         max_edges, *tol, _ptr(loops), _poly_rows(loops), _ptr(vertices), _poly_rows(vertices), counts.ctypes.data,
                                         _ptr(stats), k, _ptr(scaled), C.byref(ow), C.byref(oh))
        if not self._loaded(rc):
            return result(None, None, None, None, scaled, (oh.value, ow.value))
        return result(*_poly_slice(loops, vertices, counts), tuple(int(v) for v in counts), stats, scaled, (oh.value, ow.value))

    def advance_polygons(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, tol16: int = 16, skip: Optional[int] = None,
                         connectivity: int = 4, max_edges: int = 0, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20,
                         want_stats: bool = True, want_scaled: bool = False) -> PolygonsFrame:
        """The fused path with simplified polygons, scale -> model -> Segments decode -> Outlines -> Simplify within ``tol16``
        sixteenths of a pixel, in one call -> ``PolygonsFrame``.  Every result field is None when no model is loaded (``scaled`` is
        still produced)."""
        return self._advance_poly("infur_frame_polygons", PolygonsFrame, _lib.SIMPLIFY_COUNT_WORDS, False, (tol16,), img, factor, decode, skip,
                                  connectivity, max_edges, loops_rows, vertex_rows, want_stats, want_scaled)

    def advance_coverage(self, img: np.ndarray, factor: float = 1.0, decode: int = _lib.DECODE_RAW, tol16: int = 16, skip: Optional[int] = None,
                         connectivity: int = 4, max_edges: int = 0, loops_rows: int = 1 << 16, vertex_rows: int = 1 << 20,
                         want_stats: bool = True, want_scaled: bool = False) -> PolygonsFrame:
        """The fused path with polygons that fit, scale -> model -> Segments decode -> Outlines -> Coverage within ``tol16``
        sixteenths of a pixel, in one call -> ``PolygonsFrame`` whose counts are Coverage's six (n_loops, n_vertices, n_degenerate,
        status, n_aug, n_arcs).  Every result field is None when no model is loaded (``scaled`` is still produced)."""
        return self._advance_poly("infur_frame_coverage", PolygonsFrame, _lib.COVERAGE_COUNT_WORDS, True, (tol16,), img, factor, decode, skip,
                                  connectivity, max_edges, loops_rows, vertex_rows, want_stats, want_scaled)

    def advance_batch(self, imgs, factor: float = 1.0, outs=None):
        """A batch of independent frames (BASELINE configs[3]) -> list of masks, in order.  ``outs``: caller-owned mask arrays to fill
        (e.g. ``app.PinnedArray(...).array``: pinned frames and masks travel by DMA without the staging copies)."""
        L = self.ctx.L
        imgs = [_check_bgr(i) for i in imgs]
        n = len(imgs)
        f = float(np.float32(factor))
        given = outs
        outs = []
        for k, im in enumerate(imgs):
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            rc = L.infur_scale_out_dims(im.shape[1], im.shape[0], f, C.byref(ow), C.byref(oh))
            if rc:
                raise ScaleProcError(rc)
            if given is not None:
                if given[k].shape != (oh.value, ow.value, 4) or given[k].dtype != np.uint8 or not given[k].flags.c_contiguous:
                    raise ValueError(f"outs[{k}] must be a contiguous uint8 array of shape {(oh.value, ow.value, 4)}")
                outs.append(given[k])
            else:
                outs.append(np.empty((oh.value, ow.value, 4), np.uint8))
        fp = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        ws = (C.c_uint32 * n)(*[im.shape[1] for im in imgs])
        hs = (C.c_uint32 * n)(*[im.shape[0] for im in imgs])
        caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
        self.ctx.check(L.infur_batch_advance(self.ctx.h, fp, ws, hs, n, f, self.scale_mode, op, caps, None, None))
        return outs

    def advance_dev(self, d_bgr: int, w: int, h: int, factor: float, d_rgba: int, rgba_capacity: int,
                    d_scaled: int = 0):
        """Device-resident form: pointers are raw device addresses; asynchronous on ctx.stream."""
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        rc = self.ctx.L.infur_frame_advance_dev(self.ctx.h, d_bgr, w, h, float(np.float32(factor)), self.scale_mode,
                                                d_rgba, rgba_capacity, d_scaled or None, C.byref(ow), C.byref(oh))
        self.ctx.check(rc)
        return ow.value, oh.value


# --------------------------------------------------------------------------- #
# several GPUs from one process (include/infur_hip.h: infur_group_*)
# --------------------------------------------------------------------------- #
class Group:
    """``infur_group``: n contexts (one per GPU) driven together from one host process -- one worker thread per
    context, RCCL weight broadcast over xGMI, contiguous frame slices with no data-path collective
    (BASELINE configs[3]).  The reference runs all processors on one thread of one process
    (infur/src/main.rs:38-40); this is how that host reaches 8 GPUs."""

    def __init__(self, ctxs: List[Context]):
        if not ctxs:
            raise ValueError("a group needs at least one context")
        self.ctxs = list(ctxs)
        self.L = ctxs[0].L
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        g = C.c_void_p(None)
        rc = self.L.infur_group_create(arr, len(ctxs), C.byref(g))
        if rc != _lib.OK:
            raise InfurError(rc, ctxs[0].last_error())
        self.g = g

    def check(self, rc: int):
        if rc != _lib.OK:
            raise InfurError(rc, self.L.infur_group_last_error(self.g).decode() or _lib.status_string(rc))

    @property
    def uses_rccl(self) -> bool:
        return bool(self.L.infur_group_uses_rccl(self.g))

    def worker_numa_nodes(self) -> List[int]:
        """NUMA node each worker thread is pinned to (-1: not pinned)"""
        return [int(self.L.infur_group_worker_numa_node(self.g, i)) for i in range(len(self))]

    def __len__(self):
        return self.L.infur_group_size(self.g)

    def weights_broadcast(self, root: int = 0) -> None:
        self.check(self.L.infur_group_weights_broadcast(self.g, root))

    def advance_batch(self, imgs, factor: float = 1.0, scale_mode: int = _lib.SCALE_NEAREST, outs=None):
        imgs = [_check_bgr(i) for i in imgs]
        n = len(imgs)
        f = float(np.float32(factor))
        given = outs
        outs = []
        for k, im in enumerate(imgs):
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            rc = self.L.infur_scale_out_dims(im.shape[1], im.shape[0], f, C.byref(ow), C.byref(oh))
            if rc:
                raise ScaleProcError(rc)
            if given is not None:
                if given[k].shape != (oh.value, ow.value, 4) or given[k].dtype != np.uint8 or not given[k].flags.c_contiguous:
                    raise ValueError(f"outs[{k}] must be a contiguous uint8 array of shape {(oh.value, ow.value, 4)}")
                outs.append(given[k])
            else:
                outs.append(np.empty((oh.value, ow.value, 4), np.uint8))
        fp = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        ws = (C.c_uint32 * n)(*[im.shape[1] for im in imgs])
        hs = (C.c_uint32 * n)(*[im.shape[0] for im in imgs])
        caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
        self.check(self.L.infur_group_batch_advance(self.g, fp, ws, hs, n, f, scale_mode, op, caps, None, None))
        return outs

    def close(self):
        if getattr(self, "g", None):
            self.L.infur_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
