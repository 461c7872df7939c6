"""The ONE definition of how a float mode's output is compared with an oracle: four readings and one table of bars (a plain helper
module like tests/hostile.py: no tests, no fixtures).

readings(got, ref) -> (max_rel, elem, rms, bias), computed in float64:
  max_rel   max |got - ref| / max |ref|                                   (what rel_err of every suite has always been)
  elem      worst |got - ref| / |ref| over the elements with |ref| > 1e-2 max |ref|   (hostile.errors' second figure, elem_err)
  rms       ||got - ref||_2 / ||ref||_2
  bias      |mean(got - ref)| / rms(ref)
The first two are maxima: they see the worst element and nothing systematic.  rms and bias move when many elements are a little
wrong -- a truncation where rounding was meant, a dropped debias term, a tail tile that misses a K slice on elements below the
tensor's maximum -- long before the worst element does.

Policy.  The suite is deterministic (fixed seeds and frames, bit-reproducible kernels, forced forms bit-identical to configuration
0), so a bar needs no room for noise, only for legitimate later changes: bar = min(WAS, 1.3 x MEASURED) per reading, rounded UP to
two significant digits.  A change that worsens any reading of any (mode, scope) by more than 30 % has to say so and move the number
in MEASURED -- it cannot pass silently.  Because of the min, no bar is looser than the one the suite had before this table (WAS).

Scopes (the sizes are the existing tests'; MEASURED is the worst over everything the suite grades under the scope, every variant
-- forced Winograd tiles, direct convs, sub-forms that differ by design -- included):
  hostile/layer       320x240 on the historical hostile set, the 57 conv outputs
  hostile/logits1080  the historical hostile set at 1920x1080 (f32x: F(4x4) and F(6x6))
  hostile/seeds       the 13 cases of the seed sweep
  friendly/layer      the per-layer tests of test_gpu_parity, test_gpu_hl, test_gpu_split, test_gpu_f16_r101 and test_gpu_b2b
  friendly/logits     logits on the friendly weights: the golden sizes, the full-size properties tests, the exporter tests and the
                      modes' own logit tests
  edge                forms.SIZES, NATURAL_SIZES, GEOM_SIZES, the history.TARGETS size that meets an oracle and the tiny / ragged
                      lists: layers and logits
  own/<kind>          tests/test_gpu_own_error.py: each conv layer ALONE, against the float64 evaluation of that layer on the inputs the
                      device itself stored (tests/own_error.py) -- the kernel's own arithmetic, the error of the layers upstream taken
                      out.  <kind> is the kernel family that ran the layer, read off the profile: 1x1, direct, wino2 / wino4 / wino6,
                      head (the f32-output classifiers).  No bar existed before (WAS: none): the bar is 1.3 x MEASURED
  own16/<kind>        f16 only: the same, the reference's conv weights rounded to f16 first -- the f32 accumulation and one rounding of
                      the output remain (elem: 2^-11 = 4.88e-4 measured on the f16-output layers)
  cover/<kind>, cover16/<kind>   tests/test_gpu_edge_cover.py: own/<kind> (own16/<kind>) at the derived sizes of
                      tests/edge_cover.py, for the (mode, kind) where a layer there exceeds the own row: maps of 12 to 63 pixels, where
                      the MEAN error of a layer (bias) averages over a hundred times fewer elements than at the own rows' sizes, and
                      elem finds its worst element among F(6x6) tiles that are all cut (21 x 3).  Spread over the map, not on a
                      border row or a tail tile (LAB_NOTES.md, "Edge cover"); the other (mode, kind) stay under their own rows
The quantised model is bit-exact and has no row.

MEASURED, on one MI355X against the float64 / f32 references the tests use (see LAB_NOTES.md for the bars next to the old ones):
mode  scope              | measured: max_rel elem rms bias  | bar                             | bar before (WAS)
f32   hostile/layer      | 7.7e-06 3.5e-04 2.1e-06 2.6e-08 | 1.1e-05 4.6e-04 2.7e-06 3.5e-08 | 3.0e-05 2.0e-03 -       -      
f32s  hostile/layer      | 3.0e-05 1.9e-03 9.0e-06 1.2e-06 | 4.0e-05 2.6e-03 1.2e-05 1.6e-06 | 1.0e-04 5.0e-03 -       -      
f32x  hostile/layer      | 5.8e-04 2.5e-02 1.2e-04 5.0e-06 | 7.6e-04 3.0e-02 1.6e-04 6.6e-06 | 1.0e-03 3.0e-02 -       -      
f16   hostile/layer      | 4.0e-03 2.4e-01 1.4e-03 1.3e-04 | 5.2e-03 3.2e-01 1.9e-03 1.7e-04 | 1.5e-02 6.0e-01 -       -      
f16hl hostile/layer      | 5.2e-04 3.5e-02 1.3e-04 5.4e-06 | 6.8e-04 4.0e-02 1.7e-04 7.0e-06 | 1.5e-03 4.0e-02 -       -      
f32   hostile/logits1080 | 4.3e-06 3.6e-04 1.5e-06 2.8e-08 | 5.6e-06 4.7e-04 2.1e-06 3.6e-08 | 1.0e-03 2.0e-03 -       -      
f32s  hostile/logits1080 | 1.6e-05 1.1e-03 6.7e-06 1.3e-06 | 2.1e-05 1.5e-03 8.7e-06 1.8e-06 | 1.0e-03 5.0e-03 -       -      
f32x  hostile/logits1080 | 1.3e-04 8.9e-03 6.8e-05 5.2e-06 | 1.8e-04 1.2e-02 8.8e-05 6.9e-06 | 3.0e-04 1.5e-02 -       -      
f16   hostile/logits1080 | 1.7e-03 1.3e-01 1.0e-03 2.0e-04 | 2.2e-03 1.8e-01 1.4e-03 2.7e-04 | 5.0e-03 5.0e-01 -       -      
f16hl hostile/logits1080 | 1.5e-04 9.6e-03 7.8e-05 5.8e-06 | 2.1e-04 1.3e-02 1.1e-04 7.6e-06 | 1.0e-03 2.0e-02 -       -      
f32   hostile/seeds      | 5.2e-06 3.4e-04 2.0e-06 5.7e-08 | 6.8e-06 4.5e-04 2.7e-06 7.5e-08 | 1.0e-03 2.0e-03 -       -      
f32s  hostile/seeds      | 2.3e-05 1.2e-03 9.7e-06 2.1e-06 | 3.0e-05 1.6e-03 1.3e-05 2.8e-06 | 1.0e-03 5.0e-03 -       -      
f32x  hostile/seeds      | 1.9e-04 1.7e-02 9.6e-05 8.7e-06 | 2.5e-04 2.2e-02 1.3e-04 1.2e-05 | 3.0e-04 2.2e-02 -       -      
f16hl hostile/seeds      | 2.2e-04 1.5e-02 1.1e-04 7.7e-06 | 2.9e-04 2.0e-02 1.4e-04 1.0e-05 | 3.0e-04 2.0e-02 -       -      
f32   friendly/layer     | 1.4e-05 1.0e-03 4.5e-06 1.1e-07 | 1.8e-05 1.4e-03 5.9e-06 1.5e-07 | 1.0e-03 -       -       -      
f32s  friendly/layer     | 8.4e-06 5.0e-04 3.2e-06 3.5e-07 | 1.1e-05 6.6e-04 4.2e-06 4.6e-07 | 3.0e-05 -       -       -      
f16   friendly/layer     | 2.2e-03 1.4e-01 1.4e-03 1.3e-04 | 3.0e-03 1.9e-01 1.9e-03 1.8e-04 | 5.0e-03 -       -       -      
f16hl friendly/layer     | 4.2e-04 2.2e-02 2.0e-04 8.3e-06 | 5.5e-04 2.9e-02 2.6e-04 1.1e-05 | 1.0e-03 -       -       -      
f32   friendly/logits    | 1.1e-05 5.0e-04 5.2e-06 2.2e-07 | 1.4e-05 6.6e-04 6.9e-06 2.9e-07 | 1.0e-03 1.0e-03 -       -      
f32s  friendly/logits    | 6.6e-06 3.0e-04 3.8e-06 3.3e-07 | 8.6e-06 3.9e-04 5.0e-06 4.3e-07 | 3.0e-05 -       -       -      
f32x  friendly/logits    | 3.2e-04 1.9e-02 1.8e-04 4.7e-06 | 4.2e-04 2.5e-02 2.3e-04 6.1e-06 | 5.0e-04 -       -       -      
f16   friendly/logits    | 1.9e-03 1.5e-01 1.4e-03 1.8e-04 | 2.5e-03 2.0e-01 1.9e-03 2.4e-04 | 5.0e-03 -       -       -      
f16hl friendly/logits    | 3.3e-04 1.9e-02 2.5e-04 9.9e-06 | 4.3e-04 2.5e-02 3.3e-04 1.3e-05 | 6.0e-04 -       -       -      
f32   edge               | 1.6e-05 7.6e-04 4.9e-06 4.4e-07 | 2.1e-05 1.0e-03 6.4e-06 5.8e-07 | 1.0e-03 -       -       -      
f32s  edge               | 1.0e-05 6.0e-04 3.5e-06 7.0e-07 | 1.4e-05 7.8e-04 4.5e-06 9.1e-07 | 3.0e-05 -       -       -      
f32x  edge               | 5.8e-04 2.6e-02 2.4e-04 1.5e-05 | 7.6e-04 3.5e-02 3.2e-04 2.0e-05 | 1.0e-03 -       -       -      
f16   edge               | 2.1e-03 1.4e-01 1.2e-03 2.1e-04 | 2.7e-03 1.9e-01 1.6e-03 2.8e-04 | 5.0e-03 -       -       -      
f16hl edge               | 5.6e-04 2.7e-02 2.6e-04 2.7e-05 | 7.4e-04 3.6e-02 3.4e-04 3.5e-05 | 1.0e-03 -       -       -      
f32   own/1x1            | 2.3e-06 7.2e-05 6.9e-07 6.3e-09 | 3.1e-06 9.4e-05 9.1e-07 8.3e-09 | -       -       -       -      
f32s  own/1x1            | 2.0e-06 3.7e-05 5.3e-07 3.4e-08 | 2.6e-06 4.8e-05 7.0e-07 4.5e-08 | -       -       -       -      
f32x  own/1x1            | 8.4e-05 2.2e-03 3.2e-05 2.0e-06 | 1.1e-04 2.9e-03 4.2e-05 2.6e-06 | -       -       -       -      
f16   own/1x1            | 6.6e-04 2.5e-02 3.8e-04 3.4e-05 | 8.6e-04 3.3e-02 5.0e-04 4.4e-05 | -       -       -       -      
f16hl own/1x1            | 7.9e-05 1.9e-03 2.8e-05 1.9e-06 | 1.1e-04 2.5e-03 3.7e-05 2.5e-06 | -       -       -       -      
f32   own/direct         | 4.0e-06 1.1e-04 2.0e-06 2.6e-08 | 5.2e-06 1.5e-04 2.6e-06 3.5e-08 | -       -       -       -      
f32s  own/direct         | 3.0e-06 8.8e-05 1.5e-06 2.5e-07 | 3.9e-06 1.2e-04 2.0e-06 3.4e-07 | -       -       -       -      
f32x  own/direct         | 4.1e-05 2.3e-03 2.7e-05 2.0e-06 | 5.4e-05 3.0e-03 3.6e-05 2.6e-06 | -       -       -       -      
f16   own/direct         | 6.3e-04 3.2e-02 4.2e-04 5.0e-05 | 8.2e-04 4.2e-02 5.5e-04 6.5e-05 | -       -       -       -      
f16hl own/direct         | 6.2e-05 2.6e-03 3.4e-05 2.6e-06 | 8.1e-05 3.4e-03 4.5e-05 3.4e-06 | -       -       -       -      
f32   own/wino2          | 1.8e-06 7.3e-05 9.4e-07 1.0e-08 | 2.4e-06 9.6e-05 1.3e-06 1.4e-08 | -       -       -       -      
f32   own/wino4          | 7.2e-06 2.4e-04 1.7e-06 4.3e-08 | 9.3e-06 3.1e-04 2.2e-06 5.6e-08 | -       -       -       -      
f32x  own/wino4          | 3.0e-04 1.5e-02 7.9e-05 2.7e-06 | 4.0e-04 1.9e-02 1.1e-04 3.6e-06 | -       -       -       -      
f16hl own/wino4          | 3.7e-04 1.8e-02 8.1e-05 2.0e-06 | 4.8e-04 2.3e-02 1.1e-04 2.6e-06 | -       -       -       -      
f32   own/wino6          | 1.9e-05 4.3e-04 4.7e-06 3.7e-08 | 2.5e-05 5.6e-04 6.2e-06 4.9e-08 | -       -       -       -      
f32s  own/wino6          | 2.1e-05 3.0e-04 4.2e-06 2.0e-07 | 2.7e-05 3.9e-04 5.5e-06 2.6e-07 | -       -       -       -      
f32x  own/wino6          | 6.2e-04 2.6e-02 2.9e-04 4.3e-06 | 8.1e-04 3.5e-02 3.8e-04 5.6e-06 | -       -       -       -      
f16hl own/wino6          | 7.7e-04 4.6e-02 3.0e-04 3.6e-06 | 1.1e-03 6.1e-02 4.0e-04 4.7e-06 | -       -       -       -      
f32   own/head           | 6.2e-07 1.6e-05 2.8e-07 1.2e-08 | 8.1e-07 2.2e-05 3.7e-07 1.7e-08 | -       -       -       -      
f32s  own/head           | 6.6e-07 1.4e-05 2.4e-07 2.5e-08 | 8.6e-07 1.9e-05 3.2e-07 3.2e-08 | -       -       -       -      
f32x  own/head           | 2.9e-05 1.8e-03 2.1e-05 1.7e-06 | 3.8e-05 2.4e-03 2.8e-05 2.3e-06 | -       -       -       -      
f16   own/head           | 2.4e-04 1.6e-02 2.2e-04 4.1e-05 | 3.2e-04 2.1e-02 2.9e-04 5.3e-05 | -       -       -       -      
f16hl own/head           | 2.6e-05 1.8e-03 1.9e-05 3.1e-06 | 3.5e-05 2.3e-03 2.5e-05 4.1e-06 | -       -       -       -      
f16   own16/1x1          | 4.3e-04 4.9e-04 2.2e-04 3.2e-06 | 5.7e-04 6.4e-04 2.9e-04 4.2e-06 | -       -       -       -      
f16   own16/direct       | 4.6e-04 4.9e-04 2.2e-04 3.7e-06 | 6.0e-04 6.4e-04 2.9e-04 4.9e-06 | -       -       -       -      
f16   own16/head         | 3.9e-07 1.1e-05 1.4e-07 4.1e-09 | 5.1e-07 1.4e-05 1.9e-07 5.4e-09 | -       -       -       -      
f32   cover/1x1          | 1.8e-06 5.9e-05 6.7e-07 2.3e-08 | 2.4e-06 7.7e-05 8.8e-07 3.0e-08 | -       -       -       -      
f32x  cover/1x1          | 4.4e-05 2.9e-03 2.5e-05 2.8e-06 | 5.8e-05 3.9e-03 3.4e-05 3.7e-06 | -       -       -       -      
f32x  cover/direct       | 4.4e-05 3.0e-03 2.8e-05 3.8e-06 | 5.7e-05 3.9e-03 3.6e-05 5.0e-06 | -       -       -       -      
f32   cover/wino2        | 1.8e-06 6.6e-05 1.0e-06 2.8e-08 | 2.3e-06 8.6e-05 1.4e-06 3.6e-08 | -       -       -       -      
f32   cover/wino4        | 6.3e-06 2.4e-04 2.0e-06 7.6e-08 | 8.2e-06 3.2e-04 2.6e-06 9.9e-08 | -       -       -       -      
f32x  cover/wino4        | 2.6e-04 1.1e-02 7.4e-05 5.7e-06 | 3.5e-04 1.5e-02 9.7e-05 7.4e-06 | -       -       -       -      
f16hl cover/wino4        | 2.8e-04 1.7e-02 8.6e-05 5.5e-06 | 3.7e-04 2.3e-02 1.2e-04 7.2e-06 | -       -       -       -      
f32   cover/wino6        | 1.1e-05 6.9e-04 4.3e-06 1.7e-07 | 1.5e-05 9.0e-04 5.6e-06 2.3e-07 | -       -       -       -      
f32s  cover/wino6        | 1.0e-05 7.0e-04 3.0e-06 3.4e-07 | 1.4e-05 9.1e-04 4.0e-06 4.5e-07 | -       -       -       -      
f32x  cover/wino6        | 4.5e-04 2.0e-02 1.8e-04 1.0e-05 | 5.9e-04 2.7e-02 2.3e-04 1.4e-05 | -       -       -       -      
f16hl cover/wino6        | 4.4e-04 2.8e-02 1.8e-04 7.3e-06 | 5.8e-04 3.7e-02 2.4e-04 9.6e-06 | -       -       -       -      
f32s  cover/head         | 5.2e-07 1.8e-05 2.3e-07 3.2e-08 | 6.9e-07 2.4e-05 3.0e-07 4.2e-08 | -       -       -       -      
f16   cover16/1x1        | 4.6e-04 4.9e-04 2.2e-04 9.5e-06 | 6.0e-04 6.4e-04 2.9e-04 1.3e-05 | -       -       -       -      
f16   cover16/direct     | 4.7e-04 4.9e-04 2.3e-04 1.5e-05 | 6.2e-04 6.5e-04 3.1e-04 2.0e-05 | -       -       -       -      
"""
import json
import math
import os

import numpy as np

NAMES = ("max_rel", "elem", "rms", "bias")
MODES = ("f32", "f32s", "f32x", "f16", "f16hl")
SCOPES = ("hostile/layer", "hostile/logits1080", "hostile/seeds", "friendly/layer", "friendly/logits", "edge",
          "own/1x1", "own/direct", "own/wino2", "own/wino4", "own/wino6", "own/head", "own16/1x1", "own16/direct", "own16/head",
          "cover/1x1", "cover/direct", "cover/wino2", "cover/wino4", "cover/wino6", "cover/head", "cover16/1x1", "cover16/direct")
HEADROOM = 1.3  # VERDICT round 6, "Next round" item 2 (ii)

# every (mode, scope) a GPU test asks for (tests/test_accuracy_cpu.py holds the table against this and the GPU files against SCOPES)
ASKED = {
    "hostile/layer": MODES,
    "hostile/logits1080": MODES,
    "hostile/seeds": ("f32", "f32s", "f32x", "f16hl"),
    "friendly/layer": ("f32", "f32s", "f16", "f16hl"),  # (f32x has no per-layer test on the friendly weights: its layers are "edge"'s)
    "friendly/logits": MODES,
    "edge": MODES,
    # tests/own_error.py: the scope is the kernel family that ran the layer; the modes are those whose forced variants reach it
    "own/1x1": MODES,
    "own/direct": MODES,
    "own/wino2": ("f32",),
    "own/wino4": ("f32", "f32x", "f16hl"),
    "own/wino6": ("f32", "f32s", "f32x", "f16hl"),
    "own/head": MODES,
    "own16/1x1": ("f16",),
    "own16/direct": ("f16",),
    "own16/head": ("f16",),
    # tests/test_gpu_edge_cover.py: the (mode, kind) whose own / own16 row a layer at edge_cover.COVER_SIZES exceeds for reasons of
    # arithmetic (see the scopes above); every other (mode, kind) is graded under its own/* row there
    "cover/1x1": ('f32', 'f32x'),
    "cover/direct": ('f32x',),
    "cover/wino2": ('f32',),
    "cover/wino4": ('f32', 'f32x', 'f16hl'),
    "cover/wino6": ('f32', 'f32s', 'f32x', 'f16hl'),
    "cover/head": ('f32s',),
    "cover16/1x1": ('f16',),
    "cover16/direct": ('f16',),
}

_ = None  # a reading that had no bar before this table
# the bars of the suite before this table, (max_rel, elem, rms, bias); where several applied to a (mode, scope), the tightest one
# that held for ALL of its comparisons (a tighter one that held for a part of them stays next to the grade() call as `cap`)
WAS = {
    # LAYER_BAR, LAYER_ELEM_BAR of test_gpu_hostile.py
    ("f32", "hostile/layer"): (3e-5, 2e-3, _, _),
    ("f32s", "hostile/layer"): (1e-4, 5e-3, _, _),
    ("f32x", "hostile/layer"): (1e-3, 3e-2, _, _),
    ("f16", "hostile/layer"): (1.5e-2, 0.6, _, _),
    ("f16hl", "hostile/layer"): (1.5e-3, 4e-2, _, _),
    # LOGIT_BAR, ELEM_BAR (f32x: the 3e-4 of test_f32x_tiles_on_hostile_parameters, 1.5e-2 for F(6x6); F(4x4)'s 1e-2 is a cap there)
    ("f32", "hostile/logits1080"): (1e-3, 2e-3, _, _),
    ("f32s", "hostile/logits1080"): (1e-3, 5e-3, _, _),
    ("f32x", "hostile/logits1080"): (3e-4, 1.5e-2, _, _),
    ("f16", "hostile/logits1080"): (5e-3, 0.5, _, _),
    ("f16hl", "hostile/logits1080"): (1e-3, 2e-2, _, _),
    # SEED_LOGIT_BAR, SEED_ELEM_BAR; f32 and f32s were not in the sweep: LOGIT_BAR and ELEM_BAR
    ("f32", "hostile/seeds"): (1e-3, 2e-3, _, _),
    ("f32s", "hostile/seeds"): (1e-3, 5e-3, _, _),
    ("f32x", "hostile/seeds"): (3e-4, 2.2e-2, _, _),
    ("f16hl", "hostile/seeds"): (3e-4, 2e-2, _, _),
    # REL_TOL (test_gpu_parity.py; its ELEM_TOL held for the default configuration only and stays a cap there: F(6x6) forced onto
    # every 3x3 conv measures 1.02e-3 per element on classifier.0), SPLIT_TOL, F16_TOL, HL_LAYER_TOL
    ("f32", "friendly/layer"): (1e-3, _, _, _),
    ("f32s", "friendly/layer"): (3e-5, _, _, _),
    ("f16", "friendly/layer"): (5e-3, _, _, _),
    ("f16hl", "friendly/layer"): (1e-3, _, _, _),
    # REL_TOL / ELEM_TOL, SPLIT_TOL, FP8X_TOL, F16_TOL, HL_TOL (the exporter's own dict was wider for f32s, f32x and f16hl)
    ("f32", "friendly/logits"): (1e-3, 1e-3, _, _),
    ("f32s", "friendly/logits"): (3e-5, _, _, _),
    ("f32x", "friendly/logits"): (5e-4, _, _, _),
    ("f16", "friendly/logits"): (5e-3, _, _, _),
    ("f16hl", "friendly/logits"): (6e-4, _, _, _),
    # mode_bars() of test_gpu_forms.py (f32x: 5e-4 stays a cap at the sizes SIZE_BARS does not name), ORACLE_TOL, the tiny / ragged tests
    ("f32", "edge"): (1e-3, _, _, _),
    ("f32s", "edge"): (3e-5, _, _, _),
    ("f32x", "edge"): (1e-3, _, _, _),
    ("f16", "edge"): (5e-3, _, _, _),
    ("f16hl", "edge"): (1e-3, _, _, _),
}
# the own-error scopes, and their rows for the cover sizes, had no bar before their rows: the bar is 1.3 x MEASURED
WAS.update({(m, s): (_, _, _, _) for s in SCOPES if s.startswith(("own", "cover")) for m in ASKED[s]})
del _

# measured on an MI355X at the commit that introduced this table: the worst value of each reading over everything the suite grades
# under the (mode, scope) -- from the device's output against the test's float64 / f32 reference, never from a bar
MEASURED = {
    ("f32", "hostile/layer"): (7.72e-06, 3.48e-04, 2.06e-06, 2.62e-08),
    ("f32s", "hostile/layer"): (3.02e-05, 1.95e-03, 8.95e-06, 1.20e-06),
    ("f32x", "hostile/layer"): (5.79e-04, 2.51e-02, 1.18e-04, 5.03e-06),
    ("f16", "hostile/layer"): (3.96e-03, 2.41e-01, 1.42e-03, 1.25e-04),
    ("f16hl", "hostile/layer"): (5.22e-04, 3.55e-02, 1.25e-04, 5.38e-06),
    ("f32", "hostile/logits1080"): (4.27e-06, 3.59e-04, 1.55e-06, 2.75e-08),
    ("f32s", "hostile/logits1080"): (1.59e-05, 1.08e-03, 6.67e-06, 1.34e-06),
    ("f32x", "hostile/logits1080"): (1.31e-04, 8.86e-03, 6.76e-05, 5.25e-06),
    ("f16", "hostile/logits1080"): (1.66e-03, 1.34e-01, 1.05e-03, 2.04e-04),
    ("f16hl", "hostile/logits1080"): (1.54e-04, 9.62e-03, 7.83e-05, 5.79e-06),
    ("f32", "hostile/seeds"): (5.22e-06, 3.44e-04, 2.01e-06, 5.75e-08),
    ("f32s", "hostile/seeds"): (2.26e-05, 1.20e-03, 9.67e-06, 2.08e-06),
    ("f32x", "hostile/seeds"): (1.89e-04, 1.66e-02, 9.59e-05, 8.74e-06),
    ("f16hl", "hostile/seeds"): (2.17e-04, 1.53e-02, 1.06e-04, 7.69e-06),
    ("f32", "friendly/layer"): (1.37e-05, 1.02e-03, 4.47e-06, 1.09e-07),
    ("f32s", "friendly/layer"): (8.37e-06, 5.01e-04, 3.17e-06, 3.48e-07),
    ("f16", "friendly/layer"): (2.25e-03, 1.45e-01, 1.42e-03, 1.31e-04),
    ("f16hl", "friendly/layer"): (4.18e-04, 2.17e-02, 1.97e-04, 8.32e-06),
    ("f32", "friendly/logits"): (1.06e-05, 5.04e-04, 5.25e-06, 2.23e-07),
    ("f32s", "friendly/logits"): (6.61e-06, 2.98e-04, 3.84e-06, 3.27e-07),
    ("f32x", "friendly/logits"): (3.22e-04, 1.90e-02, 1.76e-04, 4.65e-06),
    ("f16", "friendly/logits"): (1.92e-03, 1.47e-01, 1.42e-03, 1.81e-04),
    ("f16hl", "friendly/logits"): (3.29e-04, 1.92e-02, 2.47e-04, 9.87e-06),
    ("f32", "edge"): (1.55e-05, 7.65e-04, 4.89e-06, 4.40e-07),
    ("f32s", "edge"): (1.03e-05, 5.95e-04, 3.45e-06, 6.95e-07),
    ("f32x", "edge"): (5.83e-04, 2.62e-02, 2.45e-04, 1.50e-05),
    ("f16", "edge"): (2.05e-03, 1.41e-01, 1.23e-03, 2.08e-04),
    ("f16hl", "edge"): (5.63e-04, 2.73e-02, 2.61e-04, 2.67e-05),
    # tests/test_gpu_own_error.py, at the commit that introduced it: each layer against the float64 evaluation of THAT layer on the
    # inputs the device stored (tests/own_error.py), the worst layer of every variant, both weight sets and the ResNet-101 case
    ("f32", "own/1x1"): (2.31e-06, 7.16e-05, 6.93e-07, 6.34e-09),
    ("f32s", "own/1x1"): (1.96e-06, 3.69e-05, 5.32e-07, 3.44e-08),
    ("f32x", "own/1x1"): (8.42e-05, 2.17e-03, 3.21e-05, 1.96e-06),
    ("f16", "own/1x1"): (6.56e-04, 2.47e-02, 3.78e-04, 3.36e-05),
    ("f16hl", "own/1x1"): (7.88e-05, 1.89e-03, 2.81e-05, 1.91e-06),
    ("f32", "own/direct"): (3.98e-06, 1.14e-04, 1.99e-06, 2.62e-08),
    ("f32s", "own/direct"): (2.99e-06, 8.76e-05, 1.52e-06, 2.55e-07),
    ("f32x", "own/direct"): (4.08e-05, 2.30e-03, 2.72e-05, 2.00e-06),
    ("f16", "own/direct"): (6.27e-04, 3.19e-02, 4.20e-04, 4.97e-05),
    ("f16hl", "own/direct"): (6.17e-05, 2.61e-03, 3.42e-05, 2.57e-06),
    ("f32", "own/wino2"): (1.82e-06, 7.34e-05, 9.37e-07, 1.03e-08),
    ("f32", "own/wino4"): (7.15e-06, 2.36e-04, 1.68e-06, 4.28e-08),
    ("f32x", "own/wino4"): (3.02e-04, 1.45e-02, 7.87e-05, 2.74e-06),
    ("f16hl", "own/wino4"): (3.66e-04, 1.76e-02, 8.06e-05, 1.97e-06),
    ("f32", "own/wino6"): (1.90e-05, 4.26e-04, 4.73e-06, 3.73e-08),
    ("f32s", "own/wino6"): (2.05e-05, 2.99e-04, 4.22e-06, 1.95e-07),
    ("f32x", "own/wino6"): (6.17e-04, 2.63e-02, 2.88e-04, 4.29e-06),
    ("f16hl", "own/wino6"): (7.70e-04, 4.62e-02, 3.04e-04, 3.56e-06),
    ("f32", "own/head"): (6.16e-07, 1.64e-05, 2.78e-07, 1.24e-08),
    ("f32s", "own/head"): (6.59e-07, 1.41e-05, 2.44e-07, 2.46e-08),
    ("f32x", "own/head"): (2.87e-05, 1.82e-03, 2.09e-05, 1.71e-06),
    ("f16", "own/head"): (2.39e-04, 1.58e-02, 2.23e-04, 4.05e-05),
    ("f16hl", "own/head"): (2.64e-05, 1.76e-03, 1.92e-05, 3.14e-06),
    # f16 against the reference whose conv weights are rounded to f16 first: the f32 accumulation and one rounding of the output
    ("f16", "own16/1x1"): (4.34e-04, 4.88e-04, 2.22e-04, 3.21e-06),
    ("f16", "own16/direct"): (4.58e-04, 4.89e-04, 2.23e-04, 3.71e-06),
    ("f16", "own16/head"): (3.92e-07, 1.07e-05, 1.42e-07, 4.14e-09),
    # tests/test_gpu_edge_cover.py, at the commit that introduced it: the worst layer alone over the six sizes of edge_cover.COVER_SIZES,
    # every baseline and graded sub-form of the (mode, kind)
    ("f32", "cover/1x1"): (1.84e-06, 5.86e-05, 6.73e-07, 2.26e-08),
    ("f32x", "cover/1x1"): (4.40e-05, 2.93e-03, 2.54e-05, 2.77e-06),
    ("f32x", "cover/direct"): (4.37e-05, 2.97e-03, 2.75e-05, 3.78e-06),
    ("f32", "cover/wino2"): (1.76e-06, 6.58e-05, 1.04e-06, 2.76e-08),
    ("f32", "cover/wino4"): (6.25e-06, 2.44e-04, 1.98e-06, 7.56e-08),
    ("f32x", "cover/wino4"): (2.64e-04, 1.15e-02, 7.45e-05, 5.67e-06),
    ("f16hl", "cover/wino4"): (2.79e-04, 1.73e-02, 8.62e-05, 5.48e-06),
    ("f32", "cover/wino6"): (1.10e-05, 6.90e-04, 4.29e-06, 1.75e-07),
    ("f32s", "cover/wino6"): (1.02e-05, 6.99e-04, 3.04e-06, 3.42e-07),
    ("f32x", "cover/wino6"): (4.50e-04, 2.03e-02, 1.76e-04, 1.02e-05),
    ("f16hl", "cover/wino6"): (4.43e-04, 2.83e-02, 1.84e-04, 7.34e-06),
    ("f32s", "cover/head"): (5.24e-07, 1.79e-05, 2.26e-07, 3.21e-08),
    ("f16", "cover16/1x1"): (4.55e-04, 4.89e-04, 2.20e-04, 9.50e-06),
    ("f16", "cover16/direct"): (4.70e-04, 4.94e-04, 2.34e-04, 1.53e-05),
}


def readings(got, ref):
    """(max_rel, elem, rms, bias) of `got` against `ref`, in float64.  A NaN or Inf in `got` makes every reading NaN, which no
    `reading < bar` admits."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    m = float(np.abs(ref).max())
    assert m > 0, "the reference is all zero: nothing to compare with"
    if not np.isfinite(got).all():
        return (float("nan"),) * 4
    d = got - ref
    a = np.abs(d)
    big = np.abs(ref) > 1e-2 * m
    ref_rms = math.sqrt(float(np.mean(ref * ref)))
    return (float(a.max() / m), float((a[big] / np.abs(ref[big])).max()), math.sqrt(float(np.mean(d * d))) / ref_rms,
            abs(float(np.mean(d))) / ref_rms)


def rel_err(got, ref):
    return readings(got, ref)[0]


def elem_err(got, ref):
    return readings(got, ref)[1]


def round_up(x, digits=2):
    """x rounded up to `digits` significant digits"""
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x)) - (digits - 1)
    q = math.ceil(round(x / 10.0 ** e, 9))
    return float(f"{q}e{e}")


def bar(mode, scope):
    """the four bars of (mode, scope): min(WAS, 1.3 x MEASURED) per reading, 1.3 x MEASURED where the reading had no bar"""
    was, meas = WAS[(mode, scope)], MEASURED[(mode, scope)]
    out = []
    for w, x in zip(was, meas):
        b = round_up(HEADROOM * x)
        out.append(b if w is None else min(w, b))
    return tuple(out)


def old_bars_pass(r, mode, scope):
    """would the bars of the suite before this table have passed these readings?"""
    return all(w is None or x < w for x, w in zip(r, WAS[(mode, scope)]))


def fmt(t):
    return "(" + ", ".join("-" if x is None else f"{x:.3g}" for x in t) + ")"


# ---- the records: the same numbers in this module's docstring, in LAB_NOTES.md and in DESIGN.md section 3 (test_accuracy_cpu.py) ----
def table_lines():
    """one line per (mode, scope): the four measured readings, the four bars, the four old bars"""
    def cells(t):
        return " ".join("-".ljust(7) if x is None else f"{x:.1e}" for x in t)

    out = [f"{'mode':6s}{'scope':19s}| measured: max_rel elem rms bias  | bar                             | bar before (WAS)"]
    for scope in SCOPES:
        for mode in ASKED[scope]:
            out.append(f"{mode:6s}{scope:19s}| {cells(MEASURED[(mode, scope)])} | {cells(bar(mode, scope))} | {cells(WAS[(mode, scope)])}")
    return out


def own_design_lines():
    """one table row per (mode, own-error scope) -- the four measured readings and the four bars"""
    def cell(t):
        return " ; ".join(f"{x:.1e}" for x in t)

    return [f"| {mode} | `{scope}` | {cell(MEASURED[(mode, scope)])} | {cell(bar(mode, scope))} |"
            for scope in SCOPES if scope.startswith("own") for mode in ASKED[scope]]


DESIGN_ROWS = {"f32": "| `F32` ", "f32s": "| `F32_SPLIT` ", "f32x": "| `F32_SPLIT_FP8` ", "f16": "| `F16` ", "f16hl": "| **`F16_HL`** "}
NORTH_STAR = 1e-3


def design_cells(mode):
    """the two cells of the mode's row in DESIGN.md section 3: the measured readings on the hostile sets against the float64
    reference (the worse of the 1080p frame and the seed sweep), one sub-entry per reading, and which readings of north_star's
    "logits within 1e-3" the mode's BARS meet"""
    scopes = [s for s in ("hostile/logits1080", "hostile/seeds") if mode in ASKED[s]]
    meas = [max(MEASURED[(mode, s)][i] for s in scopes) for i in range(4)]
    bars = [max(bar(mode, s)[i] for s in scopes) for i in range(4)]
    met = [n for n, b in zip(NAMES[:2], bars[:2]) if b <= NORTH_STAR]
    cell = " ; ".join(f"{n} {x:.1e} (bar {b:.1e})" for n, x, b in zip(NAMES, meas, bars))
    return cell, ", ".join(met) if met else "none"


# ---- two planted faults (tests/test_gpu_accuracy.py, tests/test_accuracy_cpu.py): host arithmetic on tensors a normal run reads back ----
PLANT_SIZES = ((135, 241), (97, 61))  # the ragged sizes of tests/forms.py: stride-8 maps 17x31 and 13x8, M = 527 and 104
TAIL_TILE = 128  # rows of a GEMM tile: the last M mod 128 pixels are the tail tile's
MISSED_K = slice(480, 512)  # the K slice the tail tile "misses"


def classifier_of(blob):
    """(weights [21, 512] float64, bias [21] float64) of the 512 -> 21 classifier of a blob"""
    from infur_amd import weights as W

    _, tensors = W.unpack_blob(blob)
    (w, b), = [(np.array(w, np.float64), np.array(b, np.float64)) for name, w, b in tensors if name == "classifier.4"]
    return w.reshape(w.shape[0], w.shape[1]), b


def plant_p1(x, w, b):
    """P1, a half-precision classifier: the logits of the head's input `x` [512, h, w] with inputs and weights rounded to f16,
    products and sums in float64"""
    x16 = np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
    w16 = w.astype(np.float16).astype(np.float64)
    return np.einsum("kc,chw->khw", w16, x16) + b[:, None, None]


def plant_p2(logits, x, w):
    """P2, a missed K slice in the tail tile: the last M mod 128 pixels of `logits` lose the contribution of input channels 480..511"""
    out = np.array(logits, np.float64)
    k, h, ww = out.shape
    tail = (h * ww) % TAIL_TILE
    assert tail > 0
    flat, xs = out.reshape(k, h * ww), np.asarray(x, np.float64).reshape(x.shape[0], h * ww)
    flat[:, -tail:] -= w[:, MISSED_K] @ xs[MISSED_K, -tail:]
    return out


SEEN = {}  # (mode, scope) -> worst readings of this process, and where
_LOG = os.environ.get("INFUR_ACCURACY_LOG", "")  # a file that gets one JSON line per comparison: how MEASURED is made


def failures(r, mode, scope, cap=None):
    """names of the readings that miss their bar (cap: tighter bars of this one comparison, None entries: none)"""
    bars = effective_bars(mode, scope, cap)
    return [n for n, x, b in zip(NAMES, r, bars) if not x < b]


def effective_bars(mode, scope, cap=None):
    assert mode in ASKED[scope], (mode, scope)
    if (mode, scope) in MEASURED:
        bars = bar(mode, scope)
    else:
        assert _LOG, f"no MEASURED entry for {(mode, scope)}"  # (only a measuring run may grade by the old bars alone)
        bars = tuple(math.inf if w is None else w for w in WAS[(mode, scope)])
    if cap is not None:
        bars = tuple(b if c is None else min(b, c) for b, c in zip(bars, cap))
    return bars


def grade(got, ref, mode, scope, where, cap=None, check=True):
    """All four readings of one comparison against the table's bars -> the readings.  `where`: size, layer, variant -- whatever
    names the comparison in a failure message.  check=False: record and return only (the caller collects and asserts later with
    failures())."""
    r = readings(got, ref)
    key = (mode, scope)
    worst = SEEN.setdefault(key, [[0.0, ""] for _ in NAMES])
    for slot, x in zip(worst, r):
        if not x <= slot[0]:
            slot[0], slot[1] = x, str(where)
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(json.dumps({"mode": mode, "scope": scope, "where": str(where), "r": [x if math.isfinite(x) else str(x) for x in r]}) + "\n")
    if check:
        bad = failures(r, mode, scope, cap)
        assert not bad, message(r, mode, scope, where, cap, bad)
    return r


def message(r, mode, scope, where, cap=None, bad=None):
    bars = effective_bars(mode, scope, cap)
    return (f"{mode} {scope} {where}: {', '.join(bad if bad is not None else failures(r, mode, scope, cap))} over the bar -- "
            f"(max_rel, elem, rms, bias) = {fmt(r)}, bars {fmt(bars)}")
