"""Headless segmentation front end: packed bgr24 frames in, class planes and one caption record line per frame out.

    ffmpeg -i in.mp4 -an -f image2pipe -pix_fmt bgr24 -c:v rawvideo pipe:1 \
      | python -m infur_amd.segments_cli --width 1280 --height 720 --scale 0.5 --model fcn.infurw \
            --labels-out labels.u8 --stats-out captions.jsonl --softmax

``--labels-out`` receives the argmax class planes back to back (ow*oh bytes per frame, one byte per pixel);
``--stats-out`` one JSON line per frame: ``{"frame": n, "width": ow, "height": oh, "classes": [class_summary records]}``
(name, pixels, share, centroid, box, mean confidence of every class that occurs -- the "class label captions" of the
reference's todo list).  ``--softmax`` decodes logits with the softmax probability as confidence instead of the
reference's raw ``c_max * 255``.  Frames go through the fused scale -> model -> segments path one at a time.

``--regions`` adds the per-object view: each JSON line gains ``"regions": [region_summary records]`` (id, class, name, pixels,
share, box, centroid, mean confidence and first pixel of every connected region of the class plane, in raster order of their
first pixels) and ``"n_regions"``; ``--connectivity 4|8``, ``--min-pixels N`` (drop speckle) and ``--skip-background`` select
them, ``--max-regions`` bounds the records per frame, ``--regions-out`` receives the u32 label planes back to back
(0xFFFFFFFF: no kept region).  With ``--regions`` the frame stays on the device between the decode stages: the class and
confidence planes are written to device buffers, labelled there, and only what is written out or summarised comes back.
``--conf-out`` receives the confidence planes (one byte per pixel).  Without these options the output is what it was before
they existed.

``--tracks`` (implies ``--regions``) carries the region identities from frame to frame on the device: every region record
gains ``"track"`` (stable while the object overlaps itself from one frame to the next; null beyond ``--max-regions``),
``"age"`` in frames and ``"dx"``, ``"dy"``, the step of its centroid since the previous frame (null for a new track), and every
line ``"tracks": {"status", "continued", "new", "ended"}``.  ``--min-overlap N`` is the least number of common pixels that
continues a track; ``--tracks-out`` receives the u32 track planes back to back (0xFFFFFFFF: not tracked).
``--tracks-memory N`` keeps a lost track for N frames, so that a region absent for a frame or two returns with its id
(``--tracks-reach PX``: how far per frame of absence it may have moved); ``"tracks"`` then gains ``"revived"``, ``"lost"``,
``"expired"``, ``"held"`` and every region record ``"gap"``, the frames a revived track was absent (0 otherwise).

``--runs-out FILE`` receives a plane run-length encoded on the device: per frame a u32 count n followed by n records of three
u32 (START = y*ow + x of the run's first pixel, END one past its last, VALUE), runs never crossing a row, in raster order, and
every line gains ``"n_runs"``.  ``--runs-plane class|labels|tracks`` picks the plane (``labels`` needs ``--regions``, ``tracks``
needs ``--tracks``); ``--runs-skip VALUE`` leaves the runs of that value out (0: the background class; 4294967295: pixels of no
region / no track).  With the class plane and neither ``--labels-out`` nor ``--conf-out`` the frame goes through
``infur_frame_runs``: records, count and the per-class table are all that crosses PCIe.

``--outlines-out FILE`` receives the region boundaries as closed polygon loops, traced on the device: per frame three u32
(n_loops, n_vertices, n_edges), then n_loops records of four u32 (OFFSET of the loop's first vertex, COUNT of its vertices,
VALUE, START edge id; START & 3 == 2 marks the boundary of a hole), then n_vertices u32 vertex ids Y*(ow + 1) + X, and every line
gains ``"n_loops"``.  With ``--regions`` the label plane is outlined where Regions left it on the device (one polygon with its
holes per object), otherwise the class plane; ``--outlines-skip VALUE`` takes the pixels of that value out (0: the background
class; 4294967295: pixels of no region); ``--connectivity`` is the saddle rule.  With the class plane and no other plane or
records asked for the frame goes through ``infur_frame_outlines``.  ``--outlines-tolerance PX`` (with ``--outlines-out``)
simplifies every loop on the device within PX pixels (Douglas-Peucker; PX is rounded to sixteenths of a pixel): the file then holds
the simplified arrays in the same per-frame layout, its three counts being n_loops, the simplified n_vertices and the number of
degenerate loops (COUNT below 3: a thin region collapsed to two points; skip them), and every line gains ``"n_degenerate"``.
``--outlines-shared`` (with ``--outlines-tolerance``) simplifies every border between two regions once (``infur_coverage``), so that
the polygons of neighbours still fit: same file layout, and junction vertices may be added to a loop.

``--anchors`` (needs ``--regions`` or ``--tracks``) places every object: the label plane goes through the distance transform where
Regions left it on the device (``infur_anchors_dev``, pixels of no region skipped), and every region record gains ``"anchor"``
[x, y], its most interior pixel -- on the object, which its centroid need not be -- and ``"radius"``, the distance from there to the
nearest pixel of anything else or to the frame.  ``--dist-out FILE`` (needs ``--anchors``) receives the u32 planes of squared
distances back to back (0: a pixel of no region).

``--truth FILE`` grades every frame: FILE holds one u8 ground-truth class plane of the scaled frame's size per frame, back to back;
the class plane is compared with it (``infur_compare``; ``--truth-ignore V`` leaves the pixels whose truth is V, a "void" label,
out), every line gains ``"pixel_accuracy"`` and ``"miou"``, and one last line holds the totals of the confusion matrices added up
over the frames: ``"frames"``, ``"pixel_accuracy"``, ``"miou"``, ``"fwiou"``, the per-class IoUs and the matrix itself.

``--sieve N`` removes speckle on the device: the frame goes through ``infur_frame_sieve`` (and with it ``infur_frame_sieve_dev``),
every region of fewer than N pixels takes the class of the neighbour it shares the longest border with (``--sieve-rounds R``: at
most R rounds, 1 to 64; the library's 8 by default), and every line gains ``"sieve": {small, absorbed, stranded, rounds,
pixels_changed, status}``.  ``--labels-out``, ``--regions`` and ``--regions-out`` see the cleaned plane (``--connectivity`` and
``--skip-background`` apply; the regions are those of the cleaned plane, none is dropped), ``"classes"`` is summarised from the
cleaned class plane and the confidence plane as decoded.  ``--sieve`` is refused together with ``--min-pixels``, ``--tracks``,
``--runs-out``, ``--outlines-out``, ``--anchors`` and ``--truth``: those paths read planes this one does not leave on the device.

``--shapes`` (needs ``--regions``) describes every object: the frame goes through ``infur_frame_shapes`` (scale -> model -> decode ->
Regions -> Outlines of the label plane -> Shapes, all on the device), and every region record gains ``"shape"``, the
``shape_summary`` of its row (area, perimeter, centroid, orientation, equivalent-ellipse axes, eccentricity, solidity,
compactness, and the minimum rectangle of its largest outer loop: sides, angle, centre); every line gains ``"n_hull_vertices"``.
``--hulls-out FILE`` (needs ``--shapes``) receives the convex hulls in the layout of ``--outlines-out``: per frame 4 u32 counts
(n_loops, n_hull_vertices, status, largest), then n_loops x 4 u32, then n_hull_vertices u32.  ``--shapes`` is refused together
with ``--sieve``, ``--tracks``, ``--runs-out``, ``--outlines-out``, ``--anchors`` and ``--truth``.

``--outlines-fidelity`` (needs ``--outlines-tolerance``; ``--outlines-out`` is then optional) says what the tolerance costs in pixels:
the class plane goes through ``polygon_fidelity`` -- Outlines -> Simplify (or Coverage with ``--outlines-shared``) -> Raster -> Compare
against the plane itself, all on the device -- and every line gains ``"polygon_fidelity": {vertices_in, vertices_out, changed,
conflict, uncovered, status, pixel_accuracy, miou}``; a last line carries the totals over the frames.  It is refused together with
``--regions``, ``--tracks`` and ``--sieve``: it grades the class plane.  It is a diagnostic, not a fast path: it needs no output
file of its own, with ``--outlines-out`` the Outlines and Simplify or Coverage chain runs twice per frame (once for the file, once
inside ``polygon_fidelity``), and ``polygon_fidelity`` allocates and frees its twelve device buffers on every frame, about 100 MB
at 1080p.
"""
from __future__ import annotations

import argparse
import json
import sys
import time


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--width", type=int, required=True)
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--bilinear", action="store_true", help="bilinear Scale instead of the reference's nearest")
    ap.add_argument("--model", default="")
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f32s", "f32x", "f16hl", "f16"])
    ap.add_argument("--softmax", action="store_true", help="INFUR_DECODE_SOFTMAX instead of INFUR_DECODE_RAW")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--input", default="-", help="raw bgr24 file (default stdin)")
    ap.add_argument("--labels-out", default="", help="raw class planes, one byte per pixel")
    ap.add_argument("--stats-out", default="-", help="JSON lines (default stdout)")
    ap.add_argument("--regions", action="store_true", help="add the connected regions of the class plane to every record")
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8])
    ap.add_argument("--min-pixels", type=int, default=0, help="drop regions with fewer pixels")
    ap.add_argument("--skip-background", action="store_true", help="class 0 forms no region")
    ap.add_argument("--max-regions", type=int, default=1024, help="region records per frame (the count is always complete)")
    ap.add_argument("--regions-out", default="", help="raw u32 label planes, four bytes per pixel (needs --regions)")
    ap.add_argument("--conf-out", default="", help="raw confidence planes, one byte per pixel")
    ap.add_argument("--tracks", action="store_true", help="carry region identities from frame to frame (implies --regions)")
    ap.add_argument("--min-overlap", type=int, default=1, help="common pixels a track needs to continue")
    ap.add_argument("--tracks-out", default="", help="raw u32 track planes, four bytes per pixel (needs --tracks)")
    ap.add_argument("--tracks-memory", type=int, default=0, metavar="N",
                    help="keep a lost track for N frames, so that a region that flickers returns with its id (needs --tracks; 0: off)")
    ap.add_argument("--tracks-reach", type=int, default=0, metavar="PX",
                    help="pixels per frame of absence by which a lost track's box grows when a region looks for it (needs --tracks)")
    ap.add_argument("--runs-out", default="", help="run-length records of a plane: per frame a u32 count, then count x 3 u32")
    ap.add_argument("--runs-plane", default="class", choices=["class", "labels", "tracks"], help="the plane --runs-out encodes")
    ap.add_argument("--runs-skip", type=int, default=None, help="leave out the runs of this value")
    ap.add_argument("--outlines-out", default="", help="polygon loops: per frame 3 u32 counts, then n_loops x 4 u32, then n_vertices u32")
    ap.add_argument("--outlines-skip", type=int, default=None, help="pixels of this value belong to no outlined region")
    ap.add_argument("--outlines-tolerance", type=float, default=None, help="simplify the loops within this many pixels (needs --outlines-out)")
    ap.add_argument("--outlines-shared", action="store_true",
                    help="simplify every shared border once, so that neighbouring polygons still fit (needs --outlines-tolerance)")
    ap.add_argument("--anchors", action="store_true", help="add every region's most interior pixel and its radius (needs --regions or --tracks)")
    ap.add_argument("--dist-out", default="", help="raw u32 planes of squared distances, four bytes per pixel (needs --anchors)")
    ap.add_argument("--truth", default="", help="raw u8 ground-truth class planes, one per frame: adds pixel_accuracy and miou, and a line of totals")
    ap.add_argument("--truth-ignore", type=int, default=None, metavar="V", help="truth pixels of this value are not compared (needs --truth)")
    ap.add_argument("--sieve", type=int, default=None, metavar="N", help="merge regions of fewer than N pixels into their neighbours on the device")
    ap.add_argument("--sieve-rounds", type=int, default=None, metavar="R", help="at most R rounds of merging, 1 to 64 (needs --sieve)")
    ap.add_argument("--outlines-fidelity", action="store_true",
                    help="add what the tolerance costs in pixels: the polygons filled back into a plane and compared with the class plane (needs --outlines-tolerance)")
    ap.add_argument("--shapes", action="store_true", help="add every region's shape descriptors (needs --regions)")
    ap.add_argument("--hulls-out", default="", help="convex hulls: per frame 4 u32 counts, then n_loops x 4 u32, then n_hull_vertices u32 (needs --shapes)")
    a = ap.parse_args(argv)
    if a.hulls_out and not a.shapes:
        ap.error("--hulls-out needs --shapes")
    if a.shapes:
        if not a.regions:
            ap.error("--shapes needs --regions")
        for given, name in ((a.sieve is not None, "--sieve"), (a.tracks, "--tracks"), (a.runs_out, "--runs-out"), (a.outlines_out, "--outlines-out"),
                            (a.anchors, "--anchors"), (a.truth, "--truth")):
            if given:
                ap.error(f"--shapes does not combine with {name}: the fused shapes call leaves no plane on the device for it")
    if a.sieve_rounds is not None and a.sieve is None:
        ap.error("--sieve-rounds needs --sieve")
    if a.sieve is not None and not 1 <= a.sieve <= 0xFFFFFFFF:
        ap.error("--sieve: a number of pixels, at least 1")
    if a.sieve_rounds is not None and not 1 <= a.sieve_rounds <= 64:
        ap.error("--sieve-rounds: 1 to 64")
    if a.sieve is not None:
        for given, name in ((a.min_pixels, "--min-pixels"), (a.tracks, "--tracks"), (a.runs_out, "--runs-out"), (a.outlines_out, "--outlines-out"),
                            (a.anchors, "--anchors"), (a.truth, "--truth")):
            if given:
                ap.error(f"--sieve does not combine with {name}: that path reads planes the sieve call does not leave on the device")
    if a.truth_ignore is not None and not a.truth:
        ap.error("--truth-ignore needs --truth")
    if a.truth_ignore is not None and not 0 <= a.truth_ignore <= 255:
        ap.error("--truth-ignore: a value of the truth plane, a byte")
    if a.outlines_shared and a.outlines_tolerance is None:
        ap.error("--outlines-shared needs --outlines-tolerance")
    if a.tracks_out and not a.tracks:
        ap.error("--tracks-out needs --tracks")
    if (a.tracks_memory or a.tracks_reach) and not a.tracks:
        ap.error("--tracks-memory and --tracks-reach need --tracks")
    if a.tracks_memory < 0 or a.tracks_reach < 0:
        ap.error("--tracks-memory and --tracks-reach are not negative")
    a.regions = a.regions or a.tracks
    if a.regions_out and not a.regions:
        ap.error("--regions-out needs --regions")
    if a.anchors and not a.regions:
        ap.error("--anchors needs --regions or --tracks")
    if a.dist_out and not a.anchors:
        ap.error("--dist-out needs --anchors")

    if a.runs_out and a.runs_plane == "labels" and not a.regions:
        ap.error("--runs-plane labels needs --regions")
    if a.runs_out and a.runs_plane == "tracks" and not a.tracks:
        ap.error("--runs-plane tracks needs --tracks")
    if a.runs_skip is not None and not 0 <= a.runs_skip <= (255 if a.runs_plane == "class" else 0xFFFFFFFF):
        ap.error("--runs-skip: a value of the plane (a byte for the class plane, a u32 otherwise)")

    if a.outlines_skip is not None and not 0 <= a.outlines_skip <= (0xFFFFFFFF if a.regions else 255):
        ap.error("--outlines-skip: a value of the plane (a byte for the class plane, a u32 for the label plane)")

    if a.outlines_fidelity and a.outlines_tolerance is None:
        ap.error("--outlines-fidelity needs --outlines-tolerance")
    if a.outlines_fidelity and (a.regions or a.sieve is not None):
        ap.error("--outlines-fidelity does not combine with --regions, --tracks or --sieve: it grades the class plane")
    if a.outlines_tolerance is not None and not a.outlines_out and not a.outlines_fidelity:
        ap.error("--outlines-tolerance needs --outlines-out or --outlines-fidelity")
    if a.outlines_tolerance is not None and not 0 <= a.outlines_tolerance * 16 + 0.5 < 65536:
        ap.error("--outlines-tolerance: 0 to 4095.9 pixels")

    import numpy as np

    from . import _lib
    from .app import RawVideoSource, VideoProcError
    from .processors import (Compare, CompareOut, confusion_summary, sieve_summary, Context, Coverage, CoverageOut, FramePath, Model, ModelCmd, Outlines, OutlinesOut, Runs, RunsOut, SegmentsFrame, Simplify, SimplifyOut,
                             class_summary, outlines_polygons, polygon_fidelity, region_summary, shape_summary, tolerance_to_tol16, track_summary)

    tol16 = tolerance_to_tol16(a.outlines_tolerance) if a.outlines_tolerance is not None else None

    ctx = Context(device=a.device, dtype=a.dtype)
    model = Model(ctx)
    if a.synthetic_weights:
        from .weights import synth_blob

        model.control(ModelCmd.LoadBlob(synth_blob()))
    elif a.model:
        model.control(ModelCmd.Load(a.model))
    else:
        ap.error("give --model PATH or --synthetic-weights")

    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    flab = open(a.labels_out, "wb") if a.labels_out else None
    fst = sys.stdout if a.stats_out == "-" else open(a.stats_out, "w")
    src = RawVideoSource(fin, a.width, a.height, close_stream=a.input != "-")
    fp = FramePath(ctx, scale_mode=_lib.SCALE_BILINEAR if a.bilinear else _lib.SCALE_NEAREST)
    decode = _lib.DECODE_SOFTMAX if a.softmax else _lib.DECODE_RAW
    img = src.empty_image()
    freg = open(a.regions_out, "wb") if a.regions_out else None
    fconf = open(a.conf_out, "wb") if a.conf_out else None
    ftrk = open(a.tracks_out, "wb") if a.tracks_out else None
    fruns = open(a.runs_out, "wb") if a.runs_out else None
    foutl = open(a.outlines_out, "wb") if a.outlines_out else None
    fdist = open(a.dist_out, "wb") if a.dist_out else None
    ftruth = open(a.truth, "rb") if a.truth else None
    if ftruth is not None:
        classes = model.get_info().num_classes
        grader, total = Compare(ctx, ignore_b=a.truth_ignore), np.zeros((classes, classes), np.uint64)
    rpath = None
    fhull = open(a.hulls_out, "wb") if a.hulls_out else None
    if a.regions and (a.sieve is not None or a.shapes):
        flags = _lib.REGIONS_SKIP_BACKGROUND if a.skip_background else 0
    elif a.regions:
        oh, ow = _out_dims(ctx, a.width, a.height, a.scale)
        rpath = _RegionsPath(ctx, a.width, a.height, ow, oh, a.scale, fp.scale_mode, model.get_info().num_classes, max(0, a.max_regions),
                             tracks=a.tracks, memory=(a.tracks_memory, a.tracks_reach),
                             runs=fruns is not None, outlines=foutl is not None, simplify=tol16 is not None, shared=a.outlines_shared,
                             anchors=a.anchors)
        flags = _lib.REGIONS_SKIP_BACKGROUND if a.skip_background else 0
    fid_total = {k: 0 for k in ("vertices_in", "vertices_out", "changed", "conflict", "uncovered")}
    n, t0 = 0, time.perf_counter()
    while True:
        try:
            fid = src.read_frame(img)
        except VideoProcError as e:
            if e.kind == "FinishedNormally":
                break
            raise
        if a.sieve is not None:  # scale -> model -> decode -> Regions -> Sieve -> Regions of the cleaned plane, in one call
            r = fp.advance_sieve(img, a.sieve, a.scale, decode, a.connectivity, flags if a.regions else 0, table_rows=max(0, a.max_regions) if a.regions else 0,
                                 max_rounds=a.sieve_rounds or 0, want_labels=freg is not None)
            s = SegmentsFrame(r.cleaned, r.conf, _class_stats(r.cleaned, r.conf, model.get_info().num_classes), None, None)
            labels, table, nreg = r.labels, r.table, r.n
        elif a.shapes:  # scale -> model -> decode -> Regions -> Outlines of the label plane -> Shapes, in one call
            r = fp.advance_shapes(img, a.scale, decode, a.connectivity, a.min_pixels, flags, table_rows=max(0, a.max_regions), loops_rows=1 << 32,
                                  vertex_rows=1 << 32, shape_rows=1 << 32, want_labels=freg is not None, want_klass=True, want_conf=True)
            s = SegmentsFrame(r.klass, r.conf, _class_stats(r.klass, r.conf, model.get_info().num_classes), None, None)
            labels, table, nreg = r.labels, r.table, r.n_regions
        elif rpath is not None:
            s, labels, table, nreg = rpath.advance(img, decode, a.connectivity, a.min_pixels, flags, flab is not None or ftruth is not None, fconf is not None,
                                                   freg is not None, keep_labels=(fruns is not None and a.runs_plane == "labels") or foutl is not None or a.anchors)
            if a.tracks:
                ttab, tplane, tsum = rpath.track(max(0, a.min_overlap), ftrk is not None, keep_plane=fruns is not None and a.runs_plane == "tracks")
            if fruns is not None:
                runs, nruns = rpath.runs(a.runs_plane, a.runs_skip)
            if foutl is not None:
                outl = rpath.outlines(a.outlines_skip, a.connectivity, tol16, a.outlines_shared)
            if a.anchors:
                anch, dist2 = rpath.anchors(fdist is not None)
        elif foutl is not None and fruns is None and flab is None and fconf is None and ftruth is None and not a.outlines_fidelity:  # polygons, counts and captions: no dense plane
            if tol16 is None:
                r = fp.advance_outlines(img, a.scale, decode, skip=a.outlines_skip, connectivity=a.connectivity, loops_rows=1 << 32, vertex_rows=1 << 32)
            else:
                fused = fp.advance_coverage if a.outlines_shared else fp.advance_polygons
                r = fused(img, a.scale, decode, tol16, skip=a.outlines_skip, connectivity=a.connectivity, loops_rows=1 << 32, vertex_rows=1 << 32)
            s, outl = SegmentsFrame(None, None, r.stats, None, None), (np.array(r.counts[:3], np.uint32), r.loops, r.vertices)
        elif fruns is not None and flab is None and fconf is None and foutl is None and ftruth is None and not a.outlines_fidelity:  # records, count and captions: no dense plane comes back
            r = fp.advance_runs(img, a.scale, decode, skip=a.runs_skip, runs_rows=1 << 32, want_row_start=False)
            s, runs, nruns = SegmentsFrame(None, None, r.stats, None, None), r.runs, r.n
        else:
            s = fp.advance_segments(img, a.scale, decode, want_klass=flab is not None or fruns is not None or foutl is not None or ftruth is not None or a.outlines_fidelity, want_conf=fconf is not None)
            if foutl is not None:  # the class plane is on the host anyway
                oo = OutlinesOut(loops_rows=1 << 32, vertex_rows=1 << 32)
                Outlines(ctx, skip=a.outlines_skip, connectivity=a.connectivity).advance(s.klass, oo)
                outl = (np.array([oo.n_loops, oo.n_vertices, oo.n_edges], np.uint32), oo.loops, oo.vertices)
                if tol16 is not None:
                    so = (CoverageOut if a.outlines_shared else SimplifyOut)(loops_rows=1 << 32, vertex_rows=1 << 32)
                    if a.outlines_shared:
                        Coverage(ctx, tol16).advance(Coverage.input_of(s.klass, oo, a.outlines_skip), so)
                    else:
                        Simplify(ctx, tol16).advance(Simplify.input_of(oo, s.klass.shape), so)
                    outl = (np.array([so.n_loops, so.n_vertices, so.n_degenerate], np.uint32), so.loops, so.vertices)
            if fruns is not None:  # the class plane is on the host anyway
                ro = RunsOut(runs_rows=1 << 32, want_row_start=False)
                Runs(ctx, skip=a.runs_skip).advance(s.klass, ro)
                runs, nruns = ro.runs, ro.n
        oh, ow = (s.klass.shape if s.klass is not None else _out_dims(ctx, a.width, a.height, a.scale))
        if flab is not None:
            flab.write(memoryview(s.klass).cast("B"))
        if fconf is not None:
            fconf.write(memoryview(s.conf).cast("B"))
        rec = {"frame": fid, "width": ow, "height": oh, "classes": class_summary(s.stats, ow, oh)}
        if ftruth is not None:  # the class plane is on the host anyway
            truth = np.frombuffer(ftruth.read(ow * oh), np.uint8)
            if truth.size != ow * oh:
                raise SystemExit(f"--truth: {a.truth} ends inside frame {fid} ({truth.size} of {ow * oh} bytes)")
            graded = CompareOut(rows_a=classes, rows_b=classes, want_rows=False, want_counts=False)
            grader.advance((s.klass, truth.reshape(oh, ow)), graded)
            total += graded.matrix
            grade = confusion_summary(graded.matrix)
            rec["pixel_accuracy"], rec["miou"] = grade["pixel_accuracy"], grade["miou"]
        if a.outlines_fidelity:  # the class plane is on the host anyway
            fid_rec = polygon_fidelity(ctx, s.klass, tol16, shared=a.outlines_shared, connectivity=a.connectivity, skip=a.outlines_skip,
                                       rows=model.get_info().num_classes)
            rec["polygon_fidelity"] = fid_rec
            for k in fid_total:
                fid_total[k] += fid_rec[k]
        if a.sieve is not None:
            sv = sieve_summary(r.counts)
            rec["sieve"] = {k: sv[k] for k in ("small", "absorbed", "stranded", "rounds", "pixels_changed", "status")}
            if a.regions:
                rec["n_regions"] = nreg
                rec["regions"] = region_summary(table, nreg, ow, oh)
                if freg is not None:
                    freg.write(memoryview(labels).cast("B"))
        if a.shapes:
            rec["n_regions"], rec["n_hull_vertices"] = nreg, r.counts[1]
            rec["regions"] = region_summary(table, nreg, ow, oh)
            hulls = outlines_polygons(r.loops, r.vertices, ow)
            for region, row in zip(rec["regions"], r.values):
                at = int(row[_lib.SHAPE_LOOP])
                region["shape"] = shape_summary(row, r.shapes[at], hulls[at][2]) if 0 <= at < len(r.shapes) else None
            if freg is not None:
                freg.write(memoryview(labels).cast("B"))
            if fhull is not None:
                for part in (np.array(r.counts, np.uint32), r.loops, r.vertices):
                    fhull.write(memoryview(np.ascontiguousarray(part)).cast("B"))
        if rpath is not None:
            rec["n_regions"] = nreg
            rec["regions"] = region_summary(table, nreg, ow, oh, anchors=anch) if a.anchors else region_summary(table, nreg, ow, oh)
            if a.tracks:
                for r, t in zip(rec["regions"], track_summary(table, ttab, nreg, ow, oh)):
                    r["track"], r["age"] = t["track"], t["age"]
                    r["dx"], r["dy"] = t["step"] if t["step"] is not None else (None, None)
                rec["tracks"] = {"status": int(tsum[0]), "continued": int(tsum[1]), "new": int(tsum[2]), "ended": int(tsum[3])}
                if a.tracks_memory:
                    gap, msum = rpath.memory()
                    for r, g in zip(rec["regions"], gap):
                        r["gap"] = int(g)
                    rec["tracks"].update(zip(("revived", "lost", "expired", "held"), (int(v) for v in msum)))
                if ftrk is not None:
                    ftrk.write(memoryview(tplane).cast("B"))
            if freg is not None:
                freg.write(memoryview(labels).cast("B"))
            if fdist is not None:
                fdist.write(memoryview(dist2).cast("B"))
        if fruns is not None:
            rec["n_runs"] = nruns
            fruns.write(int(nruns).to_bytes(4, "little"))
            fruns.write(memoryview(runs).cast("B"))
        if foutl is not None:
            rec["n_loops"] = int(outl[0][0])
            if tol16 is not None:
                rec["n_degenerate"] = int(outl[0][2])
            for part in outl:
                foutl.write(memoryview(np.ascontiguousarray(part)).cast("B"))
        fst.write(json.dumps(rec) + "\n")
        n += 1
    if ftruth is not None:
        grade = confusion_summary(total)
        fst.write(json.dumps({"frames": n, "pixel_accuracy": grade["pixel_accuracy"], "miou": grade["miou"], "fwiou": grade["fwiou"],
                              "classes": [{"klass": c["klass"], "name": c["name"], "iou": c["iou"]} for c in grade["classes"] if c["union"]],
                              "matrix": total.tolist()}) + "\n")
        ftruth.close()
    if a.outlines_fidelity:
        fst.write(json.dumps({"frames": n, "polygon_fidelity": fid_total}) + "\n")
    for f in (flab, fconf, freg, ftrk, fruns, foutl, fdist, fhull, fst):
        if f is not None:
            f.flush()
    el = time.perf_counter() - t0
    sys.stderr.write(f"infur segments: {n} frames in {el:.2f} s ({n / max(el, 1e-9):.1f} frames/s)\n")
    if rpath is not None:
        rpath.close()
    ctx.close()
    return 0


class _RegionsPath:
    """--regions: scale -> model -> Segments decode -> Regions with the frame resident on the device.  infur_frame_segments_dev
    writes class plane, confidence plane and per-class table into device buffers, infur_regions_dev labels those planes where
    they are; the tables, the count and the planes that are written out are all that is copied back."""

    def __init__(self, ctx, w, h, ow, oh, factor, scale_mode, classes, rows, tracks=False, memory=(0, 0), runs=False, outlines=False, simplify=False,
                 shared=False, anchors=False):
        import ctypes as C

        self.ctx, self.w, self.h, self.ow, self.oh, self.factor, self.mode = ctx, w, h, ow, oh, float(factor), scale_mode
        self.k, self.rows = classes, min(rows, ow * oh)
        self.d = {}
        for name, n in (("bgr", w * h * 3), ("klass", ow * oh), ("conf", ow * oh), ("stats", classes * _STAT_BYTES), ("labels", ow * oh * 4),
                        ("table", self.rows * _ROW_BYTES), ("n", 4)) + \
                ((("ttab", self.rows * _TRACK_BYTES), ("tplane", ow * oh * 4), ("tsum", 16)) if tracks else ()) + \
                ((("runs", ow * oh * _RUN_BYTES), ("nruns", 4)) if runs else ()) + \
                ((("loops", ow * oh * _LOOP_BYTES), ("vertices", ow * oh * 16), ("ocounts", 12)) if outlines else ()) + \
                ((("sloops", ow * oh * _LOOP_BYTES), ("svertices", ow * oh * 16 + (4 * (ow + 1) * (oh + 1) if shared else 0)), ("scounts", 24))
                 if outlines and simplify else ()) + \
                ((("anch", self.rows * _ANCHOR_BYTES), ("dist2", ow * oh * 4)) if anchors else ()):
            p = C.c_void_p(None)
            ctx.check(ctx.L.infur_dev_alloc(ctx.h, max(n, 4), C.byref(p)))
            self.d[name] = p
        self.tracker = None
        if tracks:  # --tracks: the label plane stays on the device for the tracker whether it is written out or not
            self.tracker = C.c_void_p(None)
            ctx.check(ctx.L.infur_tracker_create(ctx.h, 0, 0, C.byref(self.tracker)))
            if memory[0]:  # --tracks-memory N [--tracks-reach PX]
                ctx.check(ctx.L.infur_tracker_set_memory(self.tracker, min(memory[0], 0xFFFFFFFF), min(memory[1], 0xFFFFFFFF), 0))

    def _read(self, name, shape, dtype):
        import numpy as np

        out = np.empty(shape, dtype)
        if out.nbytes:
            self.ctx.check(self.ctx.L.infur_memcpy_d2h(self.ctx.h, out.ctypes.data, self.d[name], out.nbytes))
        return out

    def advance(self, img, decode, connectivity, min_pixels, flags, want_klass, want_conf, want_labels, keep_labels=False):
        """-> (SegmentsFrame with the planes that were asked for and the per-class table, labels or None, table rows, n).
        want_*: the plane is copied back; keep_labels: the label plane is written on the device (for `runs`) and stays there"""
        import ctypes as C

        import numpy as np

        from .processors import SegmentsFrame

        c, L, d = self.ctx, self.ctx.L, self.d
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        c.check(L.infur_memcpy_h2d(c.h, d["bgr"], img.ctypes.data, img.nbytes))
        c.check(L.infur_frame_segments_dev(c.h, d["bgr"], self.w, self.h, self.factor, self.mode, decode, d["klass"], d["conf"], self.ow * self.oh,
                                           d["stats"], self.k, None, 0, None, C.byref(ow), C.byref(oh)))
        c.check(L.infur_regions_dev(c.h, d["klass"], d["conf"], self.oh, self.ow, connectivity, min_pixels, flags, d["labels"] if want_labels or keep_labels or self.tracker else None,
                                    d["table"] if self.rows else None, self.rows, d["n"]))
        n = int(self._read("n", (1,), np.uint32)[0])
        seg = SegmentsFrame(self._read("klass", (self.oh, self.ow), np.uint8) if want_klass else None,
                            self._read("conf", (self.oh, self.ow), np.uint8) if want_conf else None,
                            self._read("stats", (self.k, _STAT_BYTES // 8), np.uint64), None, None)
        labels = self._read("labels", (self.oh, self.ow), np.uint32) if want_labels else None
        self.n = n
        return seg, labels, self._read("table", (min(n, self.rows), _ROW_BYTES // 8), np.uint64), n

    def track(self, min_overlap, want_plane, keep_plane=False):
        """infur_tracks_dev on the frame `advance` just labelled -> (track table rows, track plane or None, summary).
        want_plane: the track plane is copied back; keep_plane: it is written on the device (for `runs`) and stays there"""
        import numpy as np

        c, d = self.ctx, self.d
        c.check(c.L.infur_tracks_dev(self.tracker, d["labels"], d["table"], self.rows, d["n"], self.oh, self.ow, min_overlap, None,
                                     d["tplane"] if want_plane or keep_plane else None, d["ttab"] if self.rows else None, d["tsum"]))
        return (self._read("ttab", (min(self.n, self.rows), _TRACK_BYTES // 8), np.uint64),
                self._read("tplane", (self.oh, self.ow), np.uint32) if want_plane else None, self._read("tsum", (4,), np.uint32))

    def memory(self):
        """infur_tracker_memory after `track` -> (gap_of_region of the table's rows, memory summary): --tracks-memory"""
        import numpy as np

        k = min(self.n, self.rows)
        gap, msum = np.zeros(k, np.uint32), np.zeros(4, np.uint32)
        self.ctx.check(self.ctx.L.infur_tracker_memory(self.tracker, gap.ctypes.data if k else None, k, msum.ctypes.data, None, 0))
        return gap, msum

    def runs(self, plane, skip):
        """infur_runs_dev on a plane `advance` / `track` left on the device -> (records [n, 3] u32, n): every run, no dense plane"""
        import numpy as np

        c, d = self.ctx, self.d
        src, elem = {"class": ("klass", 1), "labels": ("labels", 4), "tracks": ("tplane", 4)}[plane]
        c.check(c.L.infur_runs_dev(c.h, d[src], elem, self.oh, self.ow, 1 if skip is not None else 0, skip or 0, d["runs"], self.ow * self.oh, None,
                                   d["nruns"]))
        n = int(self._read("nruns", (1,), np.uint32)[0])
        return self._read("runs", (n, _RUN_BYTES // 4), np.uint32), n

    def anchors(self, want_dist2):
        """infur_anchors_dev on the label plane `advance` left on the device, pixels of no region skipped -> (anchor rows of the
        table's rows [min(n, rows), 2] u32, squared distances [oh, ow] u32 or None)"""
        import numpy as np

        c, d = self.ctx, self.d
        if not (self.rows or want_dist2):
            return np.zeros((0, _ANCHOR_BYTES // 4), np.uint32), None
        c.check(c.L.infur_anchors_dev(c.h, d["labels"], 4, self.oh, self.ow, 1, 0xFFFFFFFF, d["dist2"] if want_dist2 else None,
                                      d["anch"] if self.rows else None, self.rows))
        return (self._read("anch", (min(self.n, self.rows), _ANCHOR_BYTES // 4), np.uint32),
                self._read("dist2", (self.oh, self.ow), np.uint32) if want_dist2 else None)

    def outlines(self, skip, connectivity, tol16=None, shared=False):
        """infur_outlines_dev on the label plane `advance` left on the device -> (counts [3], loops [n_loops, 4], vertices
        [n_vertices]) u32: every object's polygon, no dense plane.  tol16: infur_simplify_dev behind it, on the device too; the
        counts are then n_loops, the simplified n_vertices, n_degenerate.  shared: infur_coverage_dev in its place, which reads the
        label plane too and may insert junctions: its vertices have room for the lattice beside the input's"""
        import numpy as np

        c, d = self.ctx, self.d
        c.check(c.L.infur_outlines_dev(c.h, d["labels"], 4, self.oh, self.ow, (1 if skip is not None else 0) | (2 if connectivity == 8 else 0), skip or 0,
                                       0, d["loops"], self.ow * self.oh, d["vertices"], 4 * self.ow * self.oh, d["ocounts"]))
        if tol16 is not None and shared:
            rows = 4 * self.ow * self.oh + (self.ow + 1) * (self.oh + 1)
            c.check(c.L.infur_coverage_dev(c.h, d["labels"], 4, self.oh, self.ow, 1 if skip is not None else 0, skip or 0, d["loops"], self.ow * self.oh,
                                           d["vertices"], 4 * self.ow * self.oh, d["ocounts"], tol16, 0, d["sloops"], self.ow * self.oh, d["svertices"], rows,
                                           d["scounts"]))
            counts = self._read("scounts", (6,), np.uint32)[:3]
            return counts, self._read("sloops", (int(counts[0]), _LOOP_BYTES // 4), np.uint32), self._read("svertices", (int(counts[1]),), np.uint32)
        if tol16 is not None:
            c.check(c.L.infur_simplify_dev(c.h, d["loops"], self.ow * self.oh, d["vertices"], 4 * self.ow * self.oh, d["ocounts"], self.oh, self.ow, tol16,
                                           d["sloops"], self.ow * self.oh, d["svertices"], 4 * self.ow * self.oh, d["scounts"]))
            counts = self._read("scounts", (4,), np.uint32)[:3]
            return counts, self._read("sloops", (int(counts[0]), _LOOP_BYTES // 4), np.uint32), self._read("svertices", (int(counts[1]),), np.uint32)
        counts = self._read("ocounts", (3,), np.uint32)
        return counts, self._read("loops", (int(counts[0]), _LOOP_BYTES // 4), np.uint32), self._read("vertices", (int(counts[1]),), np.uint32)

    def close(self):
        if self.tracker:
            self.ctx.L.infur_tracker_destroy(self.tracker)
            self.tracker = None
        for p in self.d.values():
            self.ctx.L.infur_dev_free(self.ctx.h, p)
        self.d = {}


def _class_stats(klass, conf, classes):
    """--sieve: the per-class table (INFUR_STAT_WORDS u64 per class) of a cleaned class plane and the confidence plane, on the host"""
    import numpy as np

    h, w = klass.shape
    st = np.zeros((classes, _STAT_BYTES // 8), np.uint64)
    k = klass.ravel().astype(np.int64)
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    ok = k < classes
    k, ys, xs, cf = k[ok], ys[ok], xs[ok], conf.ravel()[ok].astype(np.int64)
    for col, wt in ((0, None), (1, xs), (2, ys), (3, cf)):
        st[:, col] = np.bincount(k, weights=wt, minlength=classes).astype(np.uint64)  # < 2^53: exact
    for col, v, fn, init in ((4, xs, np.minimum, h * w), (5, ys, np.minimum, h * w), (6, xs, np.maximum, 0), (7, ys, np.maximum, 0)):
        acc = np.full(classes, init, np.int64)
        fn.at(acc, k, v)
        st[:, col] = acc.astype(np.uint64)
    return st


_STAT_BYTES = 8 * 8    # INFUR_STAT_WORDS u64 per class
_ROW_BYTES = 10 * 8    # INFUR_REGION_WORDS u64 per region
_TRACK_BYTES = 8 * 8   # INFUR_TRACK_WORDS u64 per region
_RUN_BYTES = 3 * 4     # INFUR_RUN_WORDS u32 per run
_LOOP_BYTES = 4 * 4    # INFUR_LOOP_WORDS u32 per loop
_ANCHOR_BYTES = 2 * 4  # INFUR_ANCHOR_WORDS u32 per region


def _out_dims(ctx, w, h, factor):
    import ctypes as C

    ow, oh = C.c_uint32(0), C.c_uint32(0)
    ctx.L.infur_scale_out_dims(w, h, float(factor), C.byref(ow), C.byref(oh))
    return oh.value, ow.value


if __name__ == "__main__":
    raise SystemExit(main())
