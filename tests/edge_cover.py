"""Helper of tests/test_edge_cover_cpu.py and tests/test_gpu_edge_cover.py (a plain module like tests/forms.py: no tests, no product
code): the EDGE CLASSES a frame size puts a kernel into, the search for every class some frame of a box reaches, and the frame sizes
that reach what forms.SIZES, NATURAL_SIZES and GEOM_SIZES leave out -- COVER_SIZES, derived, not picked.

The frame size fixes every shape a kernel of this project sees.  A class is a string, "<family>/<where>/<case>", a pure function of one
layer of weights.plan (ConvSpec, IH, IW, OH, OW) and of the kernel that runs it (family, BM, Winograd tile mt): which case of a tile,
border or tail rule of that kernel's index arithmetic the layer's map falls into.  Families and the rule each restates:

  A  GEMM row tail, M = OH x OW against the BM of a tiled form (conv_igemm_kernel.h, conv_hl.hip: a workgroup owns rows m0 .. m0 + BM)
     and against the 32-row MFMA block: M < BM; else M mod BM in {0, 1, BM - 1, other}.  Per conv kind: 1x1s1, 1x1s2, 3x3.
  B  3x3 taps against the border, per dilation d and axis: dim <= d (every pixel loses both side taps), d < dim <= 2d (every pixel
     loses one at least), dim > 2d (an interior exists); the stride-2 3x3 conv (layer2.0.conv2): input dimension odd / even.
  C  Winograd (winograd.hip:547 wino_num_tiles: d x d phases of ceil(dim / d) positions, cut into tiles of mt): per d, axis and mt,
     each phase's length L: empty (phase >= dim), L < mt, else L mod mt in {0, 1, mt - 1, other}.
  D  the 3x3 forms with the input patch in LDS (conv3x3_halo.hip), per axis: dim < 16; else dim mod 16 in {0, 1, 8, 9, 15, other};
     and the tiling word of the plan (16x16, 8x32, mixed; "none": the plan rejects the layer) -- halo_tiling restates
     conv3x3_halo.hip:424 halo_plan and :791 halo4_plan.
  E  the 1x1 forms with the activations in registers (conv1x1_areg.hip, conv1x1_q8.hip, conv_hl_areg.hip): M against their 128- and
     256-pixel workgroups, cases as in A.
  F  stem and pool (stem_pool.hip): the parities of (H, W) and of the stem's map (both are stride-2 windows), H or W below 7 (the
     7x7 window wider than the frame).
  G  decode and up-sample (prepost.hip): low-res height or width of 1 (the bilinear pair collapses), W mod 4 (four pixels a thread).
  X  size-dependent branches A-G miss, each with its source:
     X/halo8    conv3x3_halo.hip:433-434, the 8 x 32 candidate and the strip of H mod 16 rows: a dimension below 16 by its 8-row
                tile (1, 2-7, 8, 9-15); at 16 and above whether the strip candidate exists (H mod 16 in 1..8) or not
     X/halo_bn  conv3x3_halo.hip:850 halo_bn / conv_forms.h halo_bn_rule: configuration 19 on a 64-channel conv runs N tiles of 64
     X/q_pair   infur_quant_model.cpp:33 q_pair_layer, :296: the quantised model's layer1 runs on PIXEL PAIRS -- an (H, W / 2) image of
                128-byte rows -- where the pooled width is even, on the channel-padded (H, W) image where it is odd; its kernels see
                the pair image's dimensions (kernel_dims)

BM and BN of a configuration come from what tests/cpp/conv_forms_test.cpp prints (forms_table), as tests/test_conv_forms_cpu.py reads
it: there is no second copy of that table here.
"""
# What greedy_cover() returns today (held by tests/test_edge_cover_cpu.py); the comments: the stride-4 and stride-8 maps and what the
# size was taken for first.  It stands ABOVE the imports because tests/forms.py, which this module imports, reads it for
# SIZE_SETS["cover"] and PRE_FRAME -- also in the forms child, which imports nothing else.
COVER_SIZES = [
    (146, 215),  # 37x54, 19x27: M = 513 = 1 (mod 64, 128, 256, 32) on the stride-8 map -- the one-row tail tile of every BM and both
                 # workgroups of E; Winograd phases of 27 (mt 4: other), 14 (d 2: 1 mod 6), 7 | 6 (d 4: 0 mod 6)
    (241, 258),  # 61x65, 31x33: M = 1023 = BM - 1 for every BM: the tail tile one row short; halo H = 31 = 15 (mod 16)
    (5, 93),     # 2x24, 1x12: a two-row map (d < dim <= 2d at d = 1; the 16x16 patch on 2 rows), widths 8 (mod 16) and 9-15
    (165, 17),   # 42x5, 21x3: width 3 = d < dim <= 2d at d = 2; phases of 21 | 11 | 6 rows
    (17, 97),    # 5x25, 3x13: height 3 at d = 2; halo width 25 = 9 (mod 16)
    (93, 1),     # 24x1, 12x1: halo height 24 = 8 (mod 16) on a one-column map
]


import functools  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import forms as F  # noqa: E402

sys.path.insert(0, F.ROOT)
from infur_amd import weights as W  # noqa: E402

BOX = 272        # the search box: 1 <= h, w <= BOX
MAX_SIZES = 16   # one float64 TorchModel forward per size
BMS = (64, 128, 256)
DILS = (1, 2, 4)
TILES = (2, 4, 6)
AXES = ("h", "w")
FAMILIES = "ABCDEFGX"


# ---- the class functions --------------------------------------------------------------------------------------------------------------
def tail_case(m, bm):
    """family A / E: M rows against tiles of bm rows"""
    if m < bm:
        return "lt"
    r = m % bm
    return "0" if r == 0 else "1" if r == 1 else "bm-1" if r == bm - 1 else "other"


def conv_kind(spec):
    return "3x3" if spec.k == 3 else f"1x1s{spec.stride}"


def gemm_classes(spec, oh, ow, bm):
    """A: one layer on a tiled form of `bm` rows (bm = 32: the MFMA block)"""
    where = "mfma32" if bm == 32 else f"bm{bm}"
    return {f"A/{conv_kind(spec)}/{where}/{tail_case(oh * ow, bm)}"}


def border_case(dim, d):
    return "le_d" if dim <= d else "le_2d" if dim <= 2 * d else "gt_2d"


def border_classes(spec, ih, iw):
    """B: a 3x3 conv's taps against the border"""
    if spec.stride == 2:
        return {f"B/s2/{a}/{'odd' if n % 2 else 'even'}" for a, n in zip(AXES, (ih, iw))} | \
               {f"B/s2/{a}/{border_case(n, spec.dil)}" for a, n in zip(AXES, (ih, iw))}
    return {f"B/d{spec.dil}/{a}/{border_case(n, spec.dil)}" for a, n in zip(AXES, (ih, iw))}


def phase_lengths(dim, d):
    """positions of each of the d phases of a dilated axis"""
    return [(dim - p + d - 1) // d if dim > p else 0 for p in range(d)]


def phase_case(length, mt):
    if length == 0:
        return "empty"
    if length < mt:
        return "lt"
    r = length % mt
    return "0" if r == 0 else "1" if r == 1 else "mt-1" if r == mt - 1 else "other"


def wino_classes(spec, oh, ow, mt):
    """C: a stride-1 3x3 conv in the Winograd domain with tiles of mt x mt"""
    return {f"C/d{spec.dil}/{a}/mt{mt}/{phase_case(n, mt)}" for a, dim in zip(AXES, (oh, ow)) for n in phase_lengths(dim, spec.dil)}


def halo_axis_case(dim):
    if dim < 16:
        return "lt16"
    r = dim % 16
    return str(r) if r in (0, 1, 8, 9, 15) else "other"


def halo8_case(dim):
    if dim < 16:
        return "1" if dim == 1 else "2-7" if dim < 8 else "8" if dim == 8 else "9-15"
    return "strip" if 1 <= dim % 16 <= 8 else "nostrip"


# conv3x3_halo.hip: h_pieces, h_lds (H_ROWB = 272), h4_slots, h4_lds (H4_ROWB = 528, H4_TMAX = 14)
def _h_pieces(th, tw, d):
    return ((th + 2 * d) * (tw + 2 * d) + 7) // 8


def _h_lds(bn, na, th, tw, d):
    return max(na * _h_pieces(th, tw, d) * 1024 + 3 * bn * (128 if bn <= 128 else 64), 8 * 32 * 272)


def _h4_slots(th, tw, d):
    return (_h_pieces(th, tw, d) + 3) // 4


def _h4_lds(th, tw, d):
    return max(2 * _h4_slots(th, tw, d) * 4096 + 3 * 256 * 64, 4 * 32 * 528)


HALO_PLANS = ("f16/64", "f16/128", "f16/256", "h4/256", "i8/128", "i8/256")


def halo_tiling(oh, ow, d, cin, cout, plan):
    """the tiling word of halo_plan (plan "f16/<bn>", "i8/<bn>") or halo4_plan ("h4/256") for one layer: "16x16", "8x32", "mixed", or
    "none" where no candidate fits.  Restates the candidate rule: fewest rounds of workgroups, fewest tiles, smallest patch; the first
    candidate wins a tie."""
    kind, bn = plan.split("/")
    bn = int(bn)
    es = 1 if kind == "i8" else 2
    cdiv = lambda x, y: (x + y - 1) // y  # noqa: E731
    cands = [("16x16", 16, 16, 0, 0, cdiv(oh, 16) * cdiv(ow, 16)), ("8x32", 8, 32, 0, 0, cdiv(oh, 8) * cdiv(ow, 32))]
    if oh >= 16 and oh % 16 != 0 and oh % 16 <= 8:
        cands.append(("mixed", 16, 16, oh % 16, 32, (oh // 16) * cdiv(ow, 16) + cdiv(ow, 32)))
    kchunks, ntiles = cin * es // 128, cout // bn
    best, best_cost = "none", None
    for word, th1, tw1, th2, tw2, mtiles in cands:
        patch = (th1 + 2 * d) * (tw1 + 2 * d)
        if kind == "h4":
            lds, slots = _h4_lds(th1, tw1, d), _h4_slots(th1, tw1, d)
            if th2:
                lds, slots = max(lds, _h4_lds(th2, tw2, d)), max(slots, _h4_slots(th2, tw2, d))
            if lds > 160 * 1024 or slots > 14:
                continue
            costs = [(cdiv(mtiles * ntiles, 256), mtiles, patch)]
        else:
            costs = []
            for na in ((1,) if (kchunks == 1 or bn == 64) else (2, 1)):
                lds, pieces = _h_lds(bn, na, th1, tw1, d), _h_pieces(th1, tw1, d)
                if th2:
                    lds, pieces = max(lds, _h_lds(bn, na, th2, tw2, d)), max(pieces, _h_pieces(th2, tw2, d))
                if lds > 160 * 1024 or pieces > 72:
                    continue
                slots = 256 * (2 if (bn <= 128 and na == 1 and lds <= 80 * 1024) else 1)
                costs.append((cdiv(mtiles * ntiles, slots) * (11 if (na == 1 and kchunks > 1) else 10), mtiles, patch))
        for cost in costs:
            if best_cost is None or cost < best_cost:
                best, best_cost = word, cost
    return best


def halo_plan_applies(spec, plan):
    """the channel rules of conv3x3_halo_valid / conv3x3_halo4_valid for a plan (the quantised model pads 64 channels to 128)"""
    kind, bn = plan.split("/")
    bn = int(bn)
    if spec.k != 3 or spec.stride != 1 or spec.pad != spec.dil:
        return False
    if kind == "h4" and spec.dil == 4:
        return False
    cin, cout = (max(spec.cin, 128), max(spec.cout, 128)) if kind == "i8" else (spec.cin, spec.cout)
    return cin % (128 if kind == "i8" else 64) == 0 and cout % bn == 0


def halo_classes(spec, oh, ow, plan=None):
    """D and X/halo8: a stride-1 3x3 conv on a form with the input patch in LDS; plan: one of HALO_PLANS for the tiling word too"""
    out = {f"D/{a}/{halo_axis_case(n)}" for a, n in zip(AXES, (oh, ow))} | {f"X/halo8/{a}/{halo8_case(n)}" for a, n in zip(AXES, (oh, ow))}
    if plan is not None and halo_plan_applies(spec, plan):
        cin, cout = (max(spec.cin, 128), max(spec.cout, 128)) if plan.startswith("i8") else (spec.cin, spec.cout)
        out.add(f"D/tile/{plan}/d{spec.dil}/{halo_tiling(oh, ow, spec.dil, cin, cout, plan)}")
    return out


def areg_classes(spec, oh, ow, wg):
    """E: a stride-1 1x1 conv with workgroups of wg pixels"""
    return {f"E/wg{wg}/{tail_case(oh * ow, wg)}"}


def stem_classes(h, w, sh, sw):
    """F: the frame, and the stem's map the pool reads"""
    return {f"F/frame/{h % 2}{w % 2}", f"F/stem/{sh % 2}{sw % 2}", f"F/h/{'lt7' if h < 7 else 'ge7'}", f"F/w/{'lt7' if w < 7 else 'ge7'}"}


def decode_classes(w, lh, lw):
    """G: the low-res logits' size and the frame's width"""
    return {f"G/low/h/{'1' if lh == 1 else 'gt1'}", f"G/low/w/{'1' if lw == 1 else 'gt1'}", f"G/w4/{w % 4}"}


def is_q_pair_layer(spec):
    """infur_quant_model.cpp: q_pair_layer"""
    return spec.name.startswith("backbone.layer1.") and spec.stride == 1 and spec.dil == 1 and (spec.k == 1 or (spec.k == 3 and spec.pad == 1))


def kernel_dims(mode, spec, ih, iw, oh, ow):
    """the image a layer's kernel sees on the product path: the plan's, but for the quantised model's layer1 on pixel pairs"""
    if mode == "i8" and is_q_pair_layer(spec) and ow % 2 == 0:
        return ih, iw // 2, oh, ow // 2
    return ih, iw, oh, ow


def q_pair_classes(spec, ow):
    return {f"X/q_pair/{'pair' if ow % 2 == 0 else 'padded'}"} if is_q_pair_layer(spec) else set()


def is_gemm_layer(spec):
    return spec.role != "stem"


def is_areg_layer(spec):
    return spec.k == 1 and spec.stride == 1 and spec.role not in ("cls", "auxcls")  # (never the f32 logits: conv_forms.h)


def is_halo_layer(spec):
    return spec.k == 3 and spec.stride == 1 and spec.pad == spec.dil


def layer_classes(spec, ih, iw, oh, ow):
    """every class of one layer under EVERY kernel that could run it: what the search unites"""
    out = set()
    if not is_gemm_layer(spec):
        return out
    for bm in BMS + (32,):
        out |= gemm_classes(spec, oh, ow, bm)
    if spec.k == 3:
        out |= border_classes(spec, ih, iw)
    if is_halo_layer(spec):
        for mt in TILES:
            out |= wino_classes(spec, oh, ow, mt)
        out |= halo_classes(spec, oh, ow)
        for plan in HALO_PLANS:
            out |= halo_classes(spec, oh, ow, plan)
        if spec.cout == 64:
            out.add("X/halo_bn/cout64")
    if is_areg_layer(spec):
        for wg in (128, 256):
            out |= areg_classes(spec, oh, ow, wg)
    out |= q_pair_classes(spec, ow)
    return out


# ---- the classes of a frame -----------------------------------------------------------------------------------------------------------
_SPECS = W.graph(50)


def _signature(spec):
    return (spec.k, spec.stride, spec.pad, spec.dil, spec.cin, spec.cout, spec.role in ("cls", "auxcls"), spec.role == "stem", is_q_pair_layer(spec))


# layers with one signature have one set of classes at given dimensions: one representative each
_SIG = {}
for _i, _s in enumerate(_SPECS):
    _SIG.setdefault(_signature(_s), []).append(_i)


@functools.lru_cache(maxsize=None)
def _axis_chain(n):
    """the plan separates by axis: (in, out) of every layer along an axis of n pixels (held against weights.plan by the CPU test)"""
    return tuple((ih, oh) for _, ih, _, oh, _ in W.plan(n, n))


@functools.lru_cache(maxsize=None)
def _sig_classes(sig, ih, iw, oh, ow):
    return frozenset(layer_classes(_SPECS[_SIG[sig][0]], ih, iw, oh, ow))


@functools.lru_cache(maxsize=None)
def _body_classes(s2h, s2w, h0, w0):
    """all layers behind the stem: they see the frame only through the stem's map (h0, w0: the smallest frame sides with that map)"""
    ch, cw = _axis_chain(h0), _axis_chain(w0)
    out = set()
    for sig, idx in _SIG.items():
        dims = {(ch[i][0], cw[i][0], ch[i][1], cw[i][1]) for i in idx}
        for d in dims:
            out |= _sig_classes(sig, *d)
    lh, lw = ch[-1][1], cw[-1][1]
    return frozenset(out), (lh, lw)


def frame_classes(h, w):
    """every class an h x w frame reaches, under every kernel"""
    ch, cw = _axis_chain(h), _axis_chain(w)
    sh, sw = ch[0][1], cw[0][1]
    body, (lh, lw) = _body_classes(sh, sw, 2 * sh - 1, 2 * sw - 1)
    return body | stem_classes(h, w, sh, sw) | decode_classes(w, lh, lw)


def family_of(cls):
    return cls[0]


def by_family(classes):
    out = {f: [] for f in FAMILIES}
    for c in sorted(classes):
        out[family_of(c)].append(c)
    return out


# ---- the search -----------------------------------------------------------------------------------------------------------------------
OLD_SIZES = list(F.SIZES) + list(F.NATURAL_SIZES) + list(F.GEOM_SIZES)


@functools.lru_cache(maxsize=None)
def reachable(box=BOX):
    """every class some frame with 1 <= h, w <= box reaches, and frame -> its classes"""
    per_frame = {(h, w): frame_classes(h, w) for h in range(1, box + 1) for w in range(1, box + 1)}
    return frozenset().union(*per_frame.values()), per_frame


def classes_of(sizes):
    return frozenset().union(*(frame_classes(h, w) for h, w in sizes)) if sizes else frozenset()


def missed_by(sizes, box=BOX):
    return reachable(box)[0] - classes_of(sizes)


def greedy_cover(have=None, box=BOX):
    """Deterministic greedy cover of the classes of the box that `have` (default OLD_SIZES) misses: each step takes the frame that adds
    the most missing classes, the smaller area first among equals, then the smaller (h, w)."""
    _, per_frame = reachable(box)
    missing = set(missed_by(OLD_SIZES if have is None else have, box))
    cand = {s: c & missing for s, c in per_frame.items()}
    cand = {s: c for s, c in cand.items() if c}
    cover = []
    while missing:
        best = min(cand, key=lambda s: (-len(cand[s] & missing), s[0] * s[1], s))
        got = cand[best] & missing
        assert got
        cover.append(best)
        missing -= got
        cand = {s: c & missing for s, c in cand.items() if c & missing}
    return cover


# ---- the table of forms, from the library's own header --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forms_table():
    """(mode, cfg) -> dict(name, family, bm, bn) of every form conv_forms.h admits, from the output of tests/cpp/conv_forms_test.cpp
    (plain g++; the family is read off the name's prefix, conv_forms.h: conv_family_prefix)"""
    src = os.path.join(F.ROOT, "tests", "cpp", "conv_forms_test.cpp")
    inc = os.path.join(F.ROOT, "infur_amd", "csrc")
    mode_name = {0: "f32", 1: "f16", 2: "f32s", 3: "f32x", 4: "i8", 5: "f16hl"}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "conv_forms_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", inc, src, "-o", exe])
        text = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    out = {}
    for ln in text.splitlines():
        p = ln.split()
        if p[0] in ("R", "V", "T", "#"):
            continue
        name, bm, bn = p[2], int(p[4]), int(p[5])
        if name.startswith("conv_igemm_"):
            fam = "tiled"
        elif name.startswith("conv1x1_"):
            fam = "areg"
        elif name.startswith("conv3x3_"):
            fam = "halo4" if "halo4" in name else "halo"
        elif name.startswith("conv_hl<"):
            fam = "hl_areg" if "areg" in name else "hl"
        else:
            raise ValueError(name)
        out[(mode_name[int(p[0])], int(p[1]))] = dict(name=name, family=fam, bm=bm, bn=bn)
    return out


# ---- what a forced form's own kernel met ----------------------------------------------------------------------------------------------
def record_layer(name):
    """the conv a profile record is named after ("/in", "/out": the Winograd transforms; "+...": a launch that does more)"""
    base = name.partition("+")[0]
    for suffix in ("/in", "/out"):
        if base.endswith(suffix):
            base = base[: -len(suffix)]
    return base


def form_classes(form, spec, ih, iw, oh, ow, variant="", mode=""):
    """the classes of one layer under ONE kernel: the form `form` (a forms_table entry) with the profile record's variant tag"""
    fam, words = form["family"], set(filter(None, variant.split(",")))
    out = q_pair_classes(spec, ow) if mode == "i8" else set()
    ih, iw, oh, ow = kernel_dims(mode, spec, ih, iw, oh, ow)
    if fam in ("tiled", "hl"):
        out |= gemm_classes(spec, oh, ow, form["bm"]) | gemm_classes(spec, oh, ow, 32)
        if spec.k == 3:
            out |= border_classes(spec, ih, iw)
    elif fam in ("areg", "hl_areg"):
        # conv1x1_areg.hip says which workgroup ran; conv1x1_q8.hip and conv_hl_areg.hip have 128-pixel workgroups only
        wg = 256 if "bm256" in words else 128
        out |= areg_classes(spec, oh, ow, wg)
    else:
        out |= halo_classes(spec, oh, ow) | border_classes(spec, ih, iw)
        tiling = [w_ for w_ in ("16x16", "8x32", "mixed") if w_ in words]
        bn = [w_[2:] for w_ in words if w_.startswith("bn")]
        if len(tiling) == 1 and len(bn) == 1:
            plan = ("h4" if fam == "halo4" else "i8" if mode == "i8" else "f16") + "/" + bn[0]
            out.add(f"D/tile/{plan}/d{spec.dil}/{tiling[0]}")
        if spec.cout == 64 and "bn64" in words:
            out.add("X/halo_bn/cout64")
    return out


def met_classes(mode, cfg, plain, variants_by_size, table=None):
    """From a child's product-path profile {size tag: [(record name, kernel, variant)]}: the classes the forced form's OWN kernel met,
    and the layers that carried it per size"""
    table = table or forms_table()
    form = table[(mode, cfg)]
    want = F.expected_kernel(mode, cfg, plain)
    met, carried = set(), {}
    for tag, recs in variants_by_size.items():
        h, w = (int(x) for x in tag.split("x"))
        dims = {s.name: (s, ih, iw, oh, ow) for s, ih, iw, oh, ow in W.plan(h, w)}
        for name, kernel, variant in recs:
            if kernel != want or record_layer(name) not in dims:
                continue
            carried.setdefault(tag, []).append(record_layer(name))
            met |= form_classes(form, *dims[record_layer(name)], variant=variant, mode=mode)
    return met, carried


def tiling_mismatches(mode, cfg, plain, variants_by_size, table=None):
    """records of a patch-in-LDS form whose tiling word is not the one halo_tiling restates: [(size tag, layer, said, restated)]"""
    table = table or forms_table()
    form, want, bad = table[(mode, cfg)], F.expected_kernel(mode, cfg, plain), []
    if form["family"] not in ("halo", "halo4"):
        return bad
    for tag, recs in variants_by_size.items():
        h, w = (int(x) for x in tag.split("x"))
        dims = {s.name: (s, oh, ow) for s, _, _, oh, ow in W.plan(h, w)}
        for name, kernel, variant in recs:
            if kernel != want:
                continue
            words = variant.split(",")
            spec, oh, ow = dims[record_layer(name)]
            oh, ow = kernel_dims(mode, spec, oh, ow, oh, ow)[2:]
            kind = "h4" if form["family"] == "halo4" else "i8" if mode == "i8" else "f16"
            cin, cout = (max(spec.cin, 128), max(spec.cout, 128)) if kind == "i8" else (spec.cin, spec.cout)
            restated = halo_tiling(oh, ow, spec.dil, cin, cout, f"{kind}/{words[0][2:]}")
            if restated not in words:
                bad.append((tag, name, variant, restated))
    return bad


def frame_wide_classes(variants_by_size, tile):
    """what every run meets whatever its form: F and G of each frame, and C on the layers whose records name the Winograd transforms
    (tile: the context's, 0 = F(6x6))"""
    mt = tile or 6
    met = set()
    for tag, recs in variants_by_size.items():
        h, w = (int(x) for x in tag.split("x"))
        plan = W.plan(h, w)
        dims = {s.name: (s, ih, iw, oh, ow) for s, ih, iw, oh, ow in plan}
        met |= stem_classes(h, w, plan[0][3], plan[0][4]) | decode_classes(w, plan[-1][3], plan[-1][4])
        for name, kernel, _ in recs:
            if kernel.startswith("wino_input"):
                s, _, _, oh, ow = dims[record_layer(name)]
                met |= wino_classes(s, oh, ow, mt)
    return met


@functools.lru_cache(maxsize=None)
def _layer_dims(i, box):
    """every (IH, IW, OH, OW) layer i takes over the frames of the box: the plan separates by axis"""
    per_axis = sorted({_axis_chain(n)[i] for n in range(1, box + 1)})
    return tuple((a[0], b[0], a[1], b[1]) for a in per_axis for b in per_axis)


@functools.lru_cache(maxsize=None)
def _reachable_on_layer(i, family, bm, box, mode=""):
    spec, out = _SPECS[i], set()
    for ih, iw, oh, ow in _layer_dims(i, box):
        if mode == "i8":
            out |= q_pair_classes(spec, ow)
            ih, iw, oh, ow = kernel_dims(mode, spec, ih, iw, oh, ow)
        if family in ("tiled", "hl"):
            out |= form_classes({"family": family, "bm": bm}, spec, ih, iw, oh, ow)
        elif family in ("areg", "hl_areg"):
            out |= areg_classes(spec, oh, ow, 128)
        else:
            out |= halo_classes(spec, oh, ow) | border_classes(spec, ih, iw)
    return frozenset(out)


def reachable_on(layers, form, box=BOX, mode=""):
    """the classes of `form`'s kernel that SOME frame of the box reaches on one of `layers` -- the families whose class does not hang
    on what the profile says: A and B, E with the 128-pixel workgroup, D and X without the tiling word"""
    out = set()
    for i, s in enumerate(_SPECS):
        if s.name in layers:
            out |= _reachable_on_layer(i, form["family"], form["bm"], box, "i8" if mode == "i8" else "")
    return out


# ---- what the MI355X run met: filled from its first run, then held (tests/test_gpu_edge_cover.py) ---------------------------------------
# REQUIRED[case]: the classes the forced form's own kernel met at COVER_SIZES -- case: "<mode>-cfg<k>[-plain]" of forms.cases(),
# "sub:<id>" of a forms.SUBFORM_CASES entry.  REQUIRED_WIDE[(mode, tile)]: what a baseline meets whatever the form.
# OMITTED[case]: reason -> the classes the box reaches on a layer the form ran on that REQUIRED[case] does not hold.
_REQUIRED_SETS = [('A/1x1s1/bm128/1', 'A/1x1s1/bm128/bm-1', 'A/1x1s1/bm128/lt', 'A/1x1s1/bm128/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm128/1', 'A/3x3/bm128/bm-1', 'A/3x3/bm128/lt', 'A/3x3/mfma32/1',
  'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d',
  'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d',
  'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d', 'B/s2/h/le_2d', 'B/s2/h/odd', 'B/s2/w/even', 'B/s2/w/gt_2d',
  'B/s2/w/le_d', 'B/s2/w/odd'),
 ('A/1x1s1/bm64/1', 'A/1x1s1/bm64/bm-1', 'A/1x1s1/bm64/lt', 'A/1x1s1/bm64/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm64/1', 'A/3x3/bm64/bm-1', 'A/3x3/bm64/lt', 'A/3x3/mfma32/1',
  'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d',
  'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d',
  'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d', 'B/s2/h/le_2d', 'B/s2/h/odd', 'B/s2/w/even', 'B/s2/w/gt_2d',
  'B/s2/w/le_d', 'B/s2/w/odd'),
 ('A/1x1s1/bm128/1', 'A/1x1s1/bm128/bm-1', 'A/1x1s1/bm128/lt', 'A/1x1s1/bm128/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm128/1', 'A/3x3/bm128/bm-1', 'A/3x3/bm128/lt', 'A/3x3/bm128/other',
  'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_2d', 'B/d1/h/le_d',
  'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d',
  'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d', 'B/s2/h/le_2d', 'B/s2/h/odd',
  'B/s2/w/even', 'B/s2/w/gt_2d', 'B/s2/w/le_d', 'B/s2/w/odd'),
 ('A/1x1s1/bm64/1', 'A/1x1s1/bm64/bm-1', 'A/1x1s1/bm64/lt', 'A/1x1s1/bm64/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm64/1', 'A/3x3/bm64/bm-1', 'A/3x3/bm64/lt', 'A/3x3/bm64/other',
  'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_2d', 'B/d1/h/le_d',
  'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d',
  'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d', 'B/s2/h/le_2d', 'B/s2/h/odd',
  'B/s2/w/even', 'B/s2/w/gt_2d', 'B/s2/w/le_d', 'B/s2/w/odd'),
 ('A/1x1s1/bm256/1', 'A/1x1s1/bm256/bm-1', 'A/1x1s1/bm256/lt', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1', 'A/1x1s1/mfma32/lt',
  'A/1x1s1/mfma32/other'),
 ('A/1x1s1/bm128/1', 'A/1x1s1/bm128/bm-1', 'A/1x1s1/bm128/lt', 'A/1x1s1/bm128/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm128/1', 'A/3x3/bm128/bm-1', 'A/3x3/bm128/lt', 'A/3x3/mfma32/1',
  'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d',
  'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d',
  'B/d4/w/gt_2d', 'B/d4/w/le_d'),
 ('A/1x1s1/bm256/1', 'A/1x1s1/bm256/bm-1', 'A/1x1s1/bm256/lt', 'A/1x1s1/bm256/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm256/1', 'A/3x3/bm256/bm-1', 'A/3x3/bm256/lt', 'A/3x3/mfma32/1',
  'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d',
  'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d',
  'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d', 'B/s2/h/le_2d', 'B/s2/h/odd', 'B/s2/w/even', 'B/s2/w/gt_2d',
  'B/s2/w/le_d', 'B/s2/w/odd'),
 ('A/1x1s1/bm256/1', 'A/1x1s1/bm256/bm-1', 'A/1x1s1/bm256/lt', 'A/1x1s1/bm256/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm256/1', 'A/3x3/bm256/bm-1', 'A/3x3/bm256/lt', 'A/3x3/mfma32/1',
  'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d',
  'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d',
  'B/d4/w/gt_2d', 'B/d4/w/le_d'),
 ('E/wg128/1', 'E/wg128/bm-1', 'E/wg128/lt', 'E/wg128/other'),
 ('B/d1/h/gt_2d', 'B/d1/h/le_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d',
  'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'D/h/15', 'D/h/8',
  'D/h/lt16', 'D/h/other', 'D/tile/f16/64/d1/16x16', 'D/tile/f16/64/d1/8x32', 'D/tile/f16/64/d1/mixed', 'D/tile/f16/64/d2/16x16',
  'D/tile/f16/64/d2/mixed', 'D/tile/f16/64/d4/16x16', 'D/tile/f16/64/d4/mixed', 'D/w/1', 'D/w/8', 'D/w/9', 'D/w/lt16', 'D/w/other',
  'X/halo8/h/1', 'X/halo8/h/2-7', 'X/halo8/h/9-15', 'X/halo8/h/nostrip', 'X/halo8/h/strip', 'X/halo8/w/1', 'X/halo8/w/2-7',
  'X/halo8/w/9-15', 'X/halo8/w/nostrip', 'X/halo8/w/strip', 'X/halo_bn/cout64'),
 ('B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d',
  'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'D/h/15', 'D/h/lt16', 'D/h/other',
  'D/tile/f16/256/d1/16x16', 'D/tile/f16/256/d1/mixed', 'D/tile/f16/256/d2/16x16', 'D/tile/f16/256/d2/mixed',
  'D/tile/f16/256/d4/16x16', 'D/tile/f16/256/d4/mixed', 'D/w/1', 'D/w/lt16', 'D/w/other', 'X/halo8/h/1', 'X/halo8/h/2-7',
  'X/halo8/h/9-15', 'X/halo8/h/nostrip', 'X/halo8/h/strip', 'X/halo8/w/1', 'X/halo8/w/2-7', 'X/halo8/w/9-15', 'X/halo8/w/nostrip',
  'X/halo8/w/strip'),
 ('B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d',
  'B/d2/w/le_2d', 'B/d2/w/le_d', 'D/h/15', 'D/h/lt16', 'D/h/other', 'D/tile/h4/256/d1/16x16', 'D/tile/h4/256/d1/mixed',
  'D/tile/h4/256/d2/16x16', 'D/tile/h4/256/d2/mixed', 'D/w/1', 'D/w/lt16', 'D/w/other', 'X/halo8/h/1', 'X/halo8/h/2-7',
  'X/halo8/h/9-15', 'X/halo8/h/nostrip', 'X/halo8/h/strip', 'X/halo8/w/1', 'X/halo8/w/2-7', 'X/halo8/w/9-15', 'X/halo8/w/nostrip',
  'X/halo8/w/strip'),
 ('A/1x1s1/bm256/1', 'A/1x1s1/bm256/bm-1', 'A/1x1s1/bm256/lt', 'A/1x1s1/bm256/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/3x3/bm256/1', 'A/3x3/bm256/bm-1', 'A/3x3/bm256/lt', 'A/3x3/bm256/other',
  'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_2d', 'B/d1/h/le_d',
  'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d',
  'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d', 'B/s2/h/le_2d', 'B/s2/h/odd',
  'B/s2/w/even', 'B/s2/w/gt_2d', 'B/s2/w/le_d', 'B/s2/w/odd'),
 ('E/wg256/1', 'E/wg256/bm-1', 'E/wg256/lt', 'E/wg256/other'),
 ('B/d1/h/gt_2d', 'B/d1/h/le_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d',
  'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'D/h/15', 'D/h/8',
  'D/h/lt16', 'D/h/other', 'D/tile/f16/128/d1/16x16', 'D/tile/f16/128/d1/mixed', 'D/tile/f16/128/d2/16x16',
  'D/tile/f16/128/d2/mixed', 'D/tile/f16/128/d4/16x16', 'D/tile/f16/128/d4/mixed', 'D/tile/f16/64/d1/16x16',
  'D/tile/f16/64/d1/8x32', 'D/tile/f16/64/d1/mixed', 'D/w/1', 'D/w/8', 'D/w/9', 'D/w/lt16', 'D/w/other', 'X/halo8/h/1',
  'X/halo8/h/2-7', 'X/halo8/h/9-15', 'X/halo8/h/nostrip', 'X/halo8/h/strip', 'X/halo8/w/1', 'X/halo8/w/2-7', 'X/halo8/w/9-15',
  'X/halo8/w/nostrip', 'X/halo8/w/strip', 'X/halo_bn/cout64'),
 ('A/1x1s1/bm128/1', 'A/1x1s1/bm128/bm-1', 'A/1x1s1/bm128/lt', 'A/1x1s1/bm128/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/1x1s2/bm128/1', 'A/1x1s2/bm128/bm-1', 'A/1x1s2/bm128/lt', 'A/1x1s2/mfma32/1',
  'A/1x1s2/mfma32/bm-1', 'A/1x1s2/mfma32/lt', 'A/1x1s2/mfma32/other', 'A/3x3/bm128/1', 'A/3x3/bm128/bm-1', 'A/3x3/bm128/lt',
  'A/3x3/bm128/other', 'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d',
  'B/d1/h/le_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d',
  'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d',
  'B/s2/h/le_2d', 'B/s2/h/odd', 'B/s2/w/even', 'B/s2/w/gt_2d', 'B/s2/w/le_d', 'B/s2/w/odd', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('A/1x1s1/bm64/1', 'A/1x1s1/bm64/bm-1', 'A/1x1s1/bm64/lt', 'A/1x1s1/bm64/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/1x1s2/bm64/1', 'A/1x1s2/bm64/bm-1', 'A/1x1s2/bm64/lt', 'A/1x1s2/mfma32/1',
  'A/1x1s2/mfma32/bm-1', 'A/1x1s2/mfma32/lt', 'A/1x1s2/mfma32/other', 'A/3x3/bm64/1', 'A/3x3/bm64/bm-1', 'A/3x3/bm64/lt',
  'A/3x3/bm64/other', 'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d',
  'B/d1/h/le_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d',
  'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d',
  'B/s2/h/le_2d', 'B/s2/h/odd', 'B/s2/w/even', 'B/s2/w/gt_2d', 'B/s2/w/le_d', 'B/s2/w/odd', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('A/1x1s1/bm128/1', 'A/1x1s1/bm128/bm-1', 'A/1x1s1/bm128/lt', 'A/1x1s1/bm128/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/1x1s2/bm128/1', 'A/1x1s2/bm128/bm-1', 'A/1x1s2/bm128/lt', 'A/1x1s2/mfma32/1',
  'A/1x1s2/mfma32/bm-1', 'A/1x1s2/mfma32/lt', 'A/1x1s2/mfma32/other', 'A/3x3/bm128/1', 'A/3x3/bm128/bm-1', 'A/3x3/bm128/lt',
  'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d',
  'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d',
  'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('A/1x1s1/bm256/1', 'A/1x1s1/bm256/bm-1', 'A/1x1s1/bm256/lt', 'A/1x1s1/bm256/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/1x1s2/bm256/1', 'A/1x1s2/bm256/bm-1', 'A/1x1s2/bm256/lt', 'A/1x1s2/mfma32/1',
  'A/1x1s2/mfma32/bm-1', 'A/1x1s2/mfma32/lt', 'A/1x1s2/mfma32/other', 'A/3x3/bm256/1', 'A/3x3/bm256/bm-1', 'A/3x3/bm256/lt',
  'A/3x3/bm256/other', 'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d',
  'B/d1/h/le_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d',
  'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'B/s2/h/even', 'B/s2/h/gt_2d',
  'B/s2/h/le_2d', 'B/s2/h/odd', 'B/s2/w/even', 'B/s2/w/gt_2d', 'B/s2/w/le_d', 'B/s2/w/odd', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('A/1x1s1/bm256/1', 'A/1x1s1/bm256/bm-1', 'A/1x1s1/bm256/lt', 'A/1x1s1/bm256/other', 'A/1x1s1/mfma32/1', 'A/1x1s1/mfma32/bm-1',
  'A/1x1s1/mfma32/lt', 'A/1x1s1/mfma32/other', 'A/1x1s2/bm256/1', 'A/1x1s2/bm256/bm-1', 'A/1x1s2/bm256/lt', 'A/1x1s2/mfma32/1',
  'A/1x1s2/mfma32/bm-1', 'A/1x1s2/mfma32/lt', 'A/1x1s2/mfma32/other', 'A/3x3/bm256/1', 'A/3x3/bm256/bm-1', 'A/3x3/bm256/lt',
  'A/3x3/mfma32/1', 'A/3x3/mfma32/bm-1', 'A/3x3/mfma32/lt', 'A/3x3/mfma32/other', 'B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d',
  'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d',
  'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('E/wg128/1', 'E/wg128/bm-1', 'E/wg128/lt', 'E/wg128/other', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('B/d1/h/gt_2d', 'B/d1/h/le_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d',
  'B/d2/w/gt_2d', 'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'D/h/15', 'D/h/8',
  'D/h/lt16', 'D/h/other', 'D/tile/i8/128/d1/16x16', 'D/tile/i8/128/d1/8x32', 'D/tile/i8/128/d1/mixed', 'D/tile/i8/128/d2/16x16',
  'D/tile/i8/128/d2/mixed', 'D/tile/i8/128/d4/16x16', 'D/tile/i8/128/d4/mixed', 'D/w/1', 'D/w/9', 'D/w/lt16', 'D/w/other',
  'X/halo8/h/1', 'X/halo8/h/2-7', 'X/halo8/h/9-15', 'X/halo8/h/nostrip', 'X/halo8/h/strip', 'X/halo8/w/1', 'X/halo8/w/2-7',
  'X/halo8/w/9-15', 'X/halo8/w/nostrip', 'X/halo8/w/strip', 'X/q_pair/padded', 'X/q_pair/pair'),
 ('B/d1/h/gt_2d', 'B/d1/h/le_d', 'B/d1/w/gt_2d', 'B/d1/w/le_d', 'B/d2/h/gt_2d', 'B/d2/h/le_2d', 'B/d2/h/le_d', 'B/d2/w/gt_2d',
  'B/d2/w/le_2d', 'B/d2/w/le_d', 'B/d4/h/gt_2d', 'B/d4/h/le_d', 'B/d4/w/gt_2d', 'B/d4/w/le_d', 'D/h/15', 'D/h/lt16', 'D/h/other',
  'D/tile/i8/256/d1/16x16', 'D/tile/i8/256/d1/mixed', 'D/tile/i8/256/d2/16x16', 'D/tile/i8/256/d2/mixed', 'D/tile/i8/256/d4/16x16',
  'D/tile/i8/256/d4/mixed', 'D/w/1', 'D/w/lt16', 'D/w/other', 'X/halo8/h/1', 'X/halo8/h/2-7', 'X/halo8/h/9-15', 'X/halo8/h/nostrip',
  'X/halo8/h/strip', 'X/halo8/w/1', 'X/halo8/w/2-7', 'X/halo8/w/9-15', 'X/halo8/w/nostrip', 'X/halo8/w/strip')]
REQUIRED = {'f32-cfg0': _REQUIRED_SETS[0], 'f32-cfg1': _REQUIRED_SETS[1], 'f32-cfg2': _REQUIRED_SETS[2], 'f32-cfg3': _REQUIRED_SETS[3], 'f32-cfg4': _REQUIRED_SETS[4], 'f32-cfg5': _REQUIRED_SETS[5], 'f32-cfg6': _REQUIRED_SETS[6], 'f32-cfg7': _REQUIRED_SETS[0], 'f32-cfg8': _REQUIRED_SETS[2], 'f32-cfg9': _REQUIRED_SETS[1], 'f32-cfg10': _REQUIRED_SETS[3], 'f32-cfg11': _REQUIRED_SETS[7], 'f32-cfg12': _REQUIRED_SETS[6], 'f32s-cfg0': _REQUIRED_SETS[0], 'f32s-cfg1': _REQUIRED_SETS[1], 'f32s-cfg2': _REQUIRED_SETS[2], 'f32s-cfg3': _REQUIRED_SETS[3], 'f32s-cfg4': _REQUIRED_SETS[4], 'f32s-cfg5': _REQUIRED_SETS[5], 'f32s-cfg6': _REQUIRED_SETS[6], 'f32s-cfg7': _REQUIRED_SETS[0], 'f32s-cfg8': _REQUIRED_SETS[2], 'f32s-cfg9': _REQUIRED_SETS[1], 'f32s-cfg10': _REQUIRED_SETS[3], 'f32s-cfg11': _REQUIRED_SETS[7], 'f32s-cfg12': _REQUIRED_SETS[6], 'f32x-cfg0': _REQUIRED_SETS[0], 'f32x-cfg1': _REQUIRED_SETS[1], 'f32x-cfg2': _REQUIRED_SETS[2], 'f32x-cfg3': _REQUIRED_SETS[3], 'f32x-cfg4': _REQUIRED_SETS[4], 'f32x-cfg5': _REQUIRED_SETS[5], 'f32x-cfg6': _REQUIRED_SETS[6], 'f32x-cfg7': _REQUIRED_SETS[0], 'f32x-cfg8': _REQUIRED_SETS[2], 'f32x-cfg9': _REQUIRED_SETS[1], 'f32x-cfg10': _REQUIRED_SETS[3], 'f32x-cfg11': _REQUIRED_SETS[7], 'f32x-cfg12': _REQUIRED_SETS[6], 'f16-cfg0': _REQUIRED_SETS[0], 'f16-cfg1': _REQUIRED_SETS[1], 'f16-cfg2': _REQUIRED_SETS[2], 'f16-cfg3': _REQUIRED_SETS[3], 'f16-cfg4': _REQUIRED_SETS[4], 'f16-cfg5': _REQUIRED_SETS[5], 'f16-cfg6': _REQUIRED_SETS[6], 'f16-cfg7': _REQUIRED_SETS[0], 'f16-cfg8': _REQUIRED_SETS[2], 'f16-cfg9': _REQUIRED_SETS[1], 'f16-cfg10': _REQUIRED_SETS[3], 'f16-cfg11': _REQUIRED_SETS[7], 'f16-cfg12': _REQUIRED_SETS[6], 'f16-cfg13': _REQUIRED_SETS[7], 'f16-cfg14': _REQUIRED_SETS[6], 'f16-cfg15': _REQUIRED_SETS[8], 'f16-cfg16': _REQUIRED_SETS[7], 'f16-cfg17': _REQUIRED_SETS[6], 'f16-cfg19': _REQUIRED_SETS[9], 'f16-cfg20': _REQUIRED_SETS[10], 'f16-cfg21': _REQUIRED_SETS[11], 'f16hl-cfg0': _REQUIRED_SETS[2], 'f16hl-cfg0-plain': _REQUIRED_SETS[2], 'f16hl-cfg5': _REQUIRED_SETS[5], 'f16hl-cfg5-plain': _REQUIRED_SETS[5], 'f16hl-cfg6': _REQUIRED_SETS[12], 'f16hl-cfg6-plain': _REQUIRED_SETS[12], 'f16hl-cfg11': _REQUIRED_SETS[7], 'f16hl-cfg11-plain': _REQUIRED_SETS[7], 'f16hl-cfg12': _REQUIRED_SETS[12], 'f16hl-cfg12-plain': _REQUIRED_SETS[12], 'f16hl-cfg13': _REQUIRED_SETS[7], 'f16hl-cfg13-plain': _REQUIRED_SETS[7], 'f16hl-cfg14': _REQUIRED_SETS[5], 'f16hl-cfg14-plain': _REQUIRED_SETS[5], 'f16hl-cfg15': _REQUIRED_SETS[8], 'f16hl-cfg15-plain': _REQUIRED_SETS[8], 'f16hl-cfg16': _REQUIRED_SETS[5], 'f16hl-cfg16-plain': _REQUIRED_SETS[5], 'f16hl-cfg17': _REQUIRED_SETS[12], 'f16hl-cfg17-plain': _REQUIRED_SETS[12], 'sub:f32-cfg0-WINO_LDS=0': _REQUIRED_SETS[0], 'sub:f32-cfg0-WINO_VEC=1': _REQUIRED_SETS[0], 'sub:f32-cfg0-WINO_VEC=2': _REQUIRED_SETS[0], 'sub:f32-cfg0-WINO_VEC=2-F2': _REQUIRED_SETS[0], 'sub:f32-cfg0-WINO_VEC=2-F4': _REQUIRED_SETS[0], 'sub:f16-cfg15-AREG_BM=256': _REQUIRED_SETS[13], 'sub:f16-cfg19': _REQUIRED_SETS[9], 'sub:f16-cfg19-HALO_BN=128': _REQUIRED_SETS[14], 'sub:f16-cfg20': _REQUIRED_SETS[10], 'sub:f16-cfg0-B2B=1-B2B_DMA=0': _REQUIRED_SETS[0], 'sub:f16-cfg0-B2B=1-B2B_DMA=1': _REQUIRED_SETS[0], 'sub:f16-cfg0-B2B=1-B2B_FORM=1': _REQUIRED_SETS[0], 'sub:f16-cfg0-B2B=1-B2B_FORM=2': _REQUIRED_SETS[0], 'sub:f16-cfg0-STEM_F32=1': _REQUIRED_SETS[0], 'sub:f32s-cfg0-STEM_F32=1': _REQUIRED_SETS[0], 'i8-cfg0': _REQUIRED_SETS[15], 'i8-cfg1': _REQUIRED_SETS[16], 'i8-cfg2': _REQUIRED_SETS[15], 'i8-cfg3': _REQUIRED_SETS[16], 'i8-cfg4': _REQUIRED_SETS[4], 'i8-cfg5': _REQUIRED_SETS[17], 'i8-cfg6': _REQUIRED_SETS[18], 'i8-cfg7': _REQUIRED_SETS[15], 'i8-cfg8': _REQUIRED_SETS[15], 'i8-cfg9': _REQUIRED_SETS[16], 'i8-cfg10': _REQUIRED_SETS[16], 'i8-cfg11': _REQUIRED_SETS[19], 'i8-cfg12': _REQUIRED_SETS[18], 'i8-cfg13': _REQUIRED_SETS[19], 'i8-cfg14': _REQUIRED_SETS[18], 'i8-cfg15': _REQUIRED_SETS[20], 'i8-cfg16': _REQUIRED_SETS[19], 'i8-cfg17': _REQUIRED_SETS[18], 'i8-cfg18': _REQUIRED_SETS[20], 'i8-cfg19': _REQUIRED_SETS[21], 'i8-cfg20': _REQUIRED_SETS[22], 'sub:i8-cfg18': _REQUIRED_SETS[20], 'sub:i8-cfg18-Q8_NSPLIT=2': _REQUIRED_SETS[20], 'sub:i8-cfg18-Q8_NSPLIT=4': _REQUIRED_SETS[20], 'sub:i8-cfg18-Q8_NSPLIT=8': _REQUIRED_SETS[20]}
REQUIRED_WIDE = {('f16', 0): ('F/frame/01', 'F/frame/10', 'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11', 'F/w/ge7', 'F/w/lt7',
              'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f16hl', 0): ('C/d1/h/mt6/0', 'C/d1/h/mt6/1', 'C/d1/h/mt6/lt', 'C/d1/h/mt6/other', 'C/d1/w/mt6/0', 'C/d1/w/mt6/1',
                'C/d1/w/mt6/lt', 'C/d1/w/mt6/other', 'C/d2/h/mt6/0', 'C/d2/h/mt6/empty', 'C/d2/h/mt6/lt', 'C/d2/h/mt6/mt-1',
                'C/d2/h/mt6/other', 'C/d2/w/mt6/0', 'C/d2/w/mt6/1', 'C/d2/w/mt6/empty', 'C/d2/w/mt6/lt', 'C/d2/w/mt6/mt-1',
                'C/d2/w/mt6/other', 'C/d4/h/mt6/0', 'C/d4/h/mt6/1', 'C/d4/h/mt6/empty', 'C/d4/h/mt6/lt', 'C/d4/h/mt6/other',
                'C/d4/w/mt6/0', 'C/d4/w/mt6/1', 'C/d4/w/mt6/empty', 'C/d4/w/mt6/lt', 'C/d4/w/mt6/other', 'F/frame/01', 'F/frame/10',
                'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11', 'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1',
                'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f16hl', 4): ('C/d1/h/mt4/0', 'C/d1/h/mt4/1', 'C/d1/h/mt4/lt', 'C/d1/h/mt4/mt-1', 'C/d1/w/mt4/0', 'C/d1/w/mt4/1', 'C/d1/w/mt4/lt',
                'C/d1/w/mt4/mt-1', 'C/d2/h/mt4/0', 'C/d2/h/mt4/1', 'C/d2/h/mt4/empty', 'C/d2/h/mt4/lt', 'C/d2/h/mt4/mt-1',
                'C/d2/h/mt4/other', 'C/d2/w/mt4/0', 'C/d2/w/mt4/1', 'C/d2/w/mt4/empty', 'C/d2/w/mt4/lt', 'C/d2/w/mt4/mt-1',
                'C/d2/w/mt4/other', 'C/d4/h/mt4/0', 'C/d4/h/mt4/1', 'C/d4/h/mt4/empty', 'C/d4/h/mt4/lt', 'C/d4/h/mt4/mt-1',
                'C/d4/h/mt4/other', 'C/d4/w/mt4/0', 'C/d4/w/mt4/1', 'C/d4/w/mt4/empty', 'C/d4/w/mt4/lt', 'C/d4/w/mt4/mt-1',
                'C/d4/w/mt4/other', 'F/frame/01', 'F/frame/10', 'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11',
                'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f32', 0): ('C/d1/h/mt6/0', 'C/d1/h/mt6/1', 'C/d1/h/mt6/lt', 'C/d1/h/mt6/other', 'C/d1/w/mt6/0', 'C/d1/w/mt6/1', 'C/d1/w/mt6/lt',
              'C/d1/w/mt6/other', 'C/d2/h/mt6/0', 'C/d2/h/mt6/empty', 'C/d2/h/mt6/lt', 'C/d2/h/mt6/mt-1', 'C/d2/h/mt6/other',
              'C/d2/w/mt6/0', 'C/d2/w/mt6/1', 'C/d2/w/mt6/empty', 'C/d2/w/mt6/lt', 'C/d2/w/mt6/mt-1', 'C/d2/w/mt6/other',
              'C/d4/h/mt6/0', 'C/d4/h/mt6/1', 'C/d4/h/mt6/empty', 'C/d4/h/mt6/lt', 'C/d4/h/mt6/other', 'C/d4/w/mt6/0',
              'C/d4/w/mt6/1', 'C/d4/w/mt6/empty', 'C/d4/w/mt6/lt', 'C/d4/w/mt6/other', 'F/frame/01', 'F/frame/10', 'F/frame/11',
              'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11', 'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1',
              'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f32', 2): ('C/d1/h/mt2/0', 'C/d1/h/mt2/1', 'C/d1/h/mt2/lt', 'C/d1/w/mt2/0', 'C/d1/w/mt2/1', 'C/d1/w/mt2/lt', 'C/d2/h/mt2/0',
              'C/d2/h/mt2/1', 'C/d2/h/mt2/empty', 'C/d2/h/mt2/lt', 'C/d2/w/mt2/0', 'C/d2/w/mt2/1', 'C/d2/w/mt2/empty',
              'C/d2/w/mt2/lt', 'C/d4/h/mt2/0', 'C/d4/h/mt2/1', 'C/d4/h/mt2/empty', 'C/d4/h/mt2/lt', 'C/d4/w/mt2/0', 'C/d4/w/mt2/1',
              'C/d4/w/mt2/empty', 'C/d4/w/mt2/lt', 'F/frame/01', 'F/frame/10', 'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10',
              'F/stem/11', 'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2',
              'G/w4/3'),
 ('f32', 4): ('C/d1/h/mt4/0', 'C/d1/h/mt4/1', 'C/d1/h/mt4/lt', 'C/d1/h/mt4/mt-1', 'C/d1/w/mt4/0', 'C/d1/w/mt4/1', 'C/d1/w/mt4/lt',
              'C/d1/w/mt4/mt-1', 'C/d2/h/mt4/0', 'C/d2/h/mt4/1', 'C/d2/h/mt4/empty', 'C/d2/h/mt4/lt', 'C/d2/h/mt4/mt-1',
              'C/d2/h/mt4/other', 'C/d2/w/mt4/0', 'C/d2/w/mt4/1', 'C/d2/w/mt4/empty', 'C/d2/w/mt4/lt', 'C/d2/w/mt4/mt-1',
              'C/d2/w/mt4/other', 'C/d4/h/mt4/0', 'C/d4/h/mt4/1', 'C/d4/h/mt4/empty', 'C/d4/h/mt4/lt', 'C/d4/h/mt4/mt-1',
              'C/d4/h/mt4/other', 'C/d4/w/mt4/0', 'C/d4/w/mt4/1', 'C/d4/w/mt4/empty', 'C/d4/w/mt4/lt', 'C/d4/w/mt4/mt-1',
              'C/d4/w/mt4/other', 'F/frame/01', 'F/frame/10', 'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11',
              'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f32s', 0): ('C/d1/h/mt6/0', 'C/d1/h/mt6/1', 'C/d1/h/mt6/lt', 'C/d1/h/mt6/other', 'C/d1/w/mt6/0', 'C/d1/w/mt6/1', 'C/d1/w/mt6/lt',
               'C/d1/w/mt6/other', 'C/d2/h/mt6/0', 'C/d2/h/mt6/empty', 'C/d2/h/mt6/lt', 'C/d2/h/mt6/mt-1', 'C/d2/h/mt6/other',
               'C/d2/w/mt6/0', 'C/d2/w/mt6/1', 'C/d2/w/mt6/empty', 'C/d2/w/mt6/lt', 'C/d2/w/mt6/mt-1', 'C/d2/w/mt6/other',
               'C/d4/h/mt6/0', 'C/d4/h/mt6/1', 'C/d4/h/mt6/empty', 'C/d4/h/mt6/lt', 'C/d4/h/mt6/other', 'C/d4/w/mt6/0',
               'C/d4/w/mt6/1', 'C/d4/w/mt6/empty', 'C/d4/w/mt6/lt', 'C/d4/w/mt6/other', 'F/frame/01', 'F/frame/10', 'F/frame/11',
               'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11', 'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1',
               'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f32x', 0): ('C/d1/h/mt6/0', 'C/d1/h/mt6/1', 'C/d1/h/mt6/lt', 'C/d1/h/mt6/other', 'C/d1/w/mt6/0', 'C/d1/w/mt6/1', 'C/d1/w/mt6/lt',
               'C/d1/w/mt6/other', 'C/d2/h/mt6/0', 'C/d2/h/mt6/empty', 'C/d2/h/mt6/lt', 'C/d2/h/mt6/mt-1', 'C/d2/h/mt6/other',
               'C/d2/w/mt6/0', 'C/d2/w/mt6/1', 'C/d2/w/mt6/empty', 'C/d2/w/mt6/lt', 'C/d2/w/mt6/mt-1', 'C/d2/w/mt6/other',
               'C/d4/h/mt6/0', 'C/d4/h/mt6/1', 'C/d4/h/mt6/empty', 'C/d4/h/mt6/lt', 'C/d4/h/mt6/other', 'C/d4/w/mt6/0',
               'C/d4/w/mt6/1', 'C/d4/w/mt6/empty', 'C/d4/w/mt6/lt', 'C/d4/w/mt6/other', 'F/frame/01', 'F/frame/10', 'F/frame/11',
               'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11', 'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1',
               'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('f32x', 4): ('C/d1/h/mt4/0', 'C/d1/h/mt4/1', 'C/d1/h/mt4/lt', 'C/d1/h/mt4/mt-1', 'C/d1/w/mt4/0', 'C/d1/w/mt4/1', 'C/d1/w/mt4/lt',
               'C/d1/w/mt4/mt-1', 'C/d2/h/mt4/0', 'C/d2/h/mt4/1', 'C/d2/h/mt4/empty', 'C/d2/h/mt4/lt', 'C/d2/h/mt4/mt-1',
               'C/d2/h/mt4/other', 'C/d2/w/mt4/0', 'C/d2/w/mt4/1', 'C/d2/w/mt4/empty', 'C/d2/w/mt4/lt', 'C/d2/w/mt4/mt-1',
               'C/d2/w/mt4/other', 'C/d4/h/mt4/0', 'C/d4/h/mt4/1', 'C/d4/h/mt4/empty', 'C/d4/h/mt4/lt', 'C/d4/h/mt4/mt-1',
               'C/d4/h/mt4/other', 'C/d4/w/mt4/0', 'C/d4/w/mt4/1', 'C/d4/w/mt4/empty', 'C/d4/w/mt4/lt', 'C/d4/w/mt4/mt-1',
               'C/d4/w/mt4/other', 'F/frame/01', 'F/frame/10', 'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11',
               'F/w/ge7', 'F/w/lt7', 'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3'),
 ('i8', 0): ('F/frame/01', 'F/frame/10', 'F/frame/11', 'F/h/ge7', 'F/h/lt7', 'F/stem/10', 'F/stem/11', 'F/w/ge7', 'F/w/lt7',
             'G/low/h/1', 'G/low/h/gt1', 'G/low/w/1', 'G/low/w/gt1', 'G/w4/1', 'G/w4/2', 'G/w4/3')}
_OMITTED_SETS = [{'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm128/0', 'A/1x1s1/mfma32/0',
                                                                               'A/3x3/bm128/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/3x3/bm128/other',),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm64/0', 'A/1x1s1/mfma32/0', 'A/3x3/bm64/0',
                                                                               'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/3x3/bm64/other',),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm128/0', 'A/1x1s1/mfma32/0',
                                                                               'A/3x3/bm128/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/d1/w/le_2d', 'B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm64/0', 'A/1x1s1/mfma32/0', 'A/3x3/bm64/0',
                                                                               'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/d1/w/le_2d', 'B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm256/0', 'A/1x1s1/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/1x1s1/bm256/other',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm128/0', 'A/1x1s1/mfma32/0',
                                                                               'A/3x3/bm128/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/3x3/bm128/other',),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm256/0', 'A/1x1s1/mfma32/0',
                                                                               'A/3x3/bm256/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/3x3/bm256/other',),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm256/0', 'A/1x1s1/mfma32/0',
                                                                               'A/3x3/bm256/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/3x3/bm256/other',),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('E/wg128/0',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('D/h/0',),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('D/h/1', 'D/w/15'),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/d1/w/le_2d',),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d', 'X/halo8/h/8'),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d', 'D/h/9', 'D/w/0', 'X/halo8/w/8')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('D/h/0', 'D/w/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('D/h/1', 'D/w/15'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d', 'X/halo8/h/8'),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d', 'X/halo8/w/8'),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d',
                                                                                                                                    'D/h/8',
                                                                                                                                    'D/h/9',
                                                                                                                                    'D/w/8',
                                                                                                                                    'D/w/9')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('D/h/0', 'D/w/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('D/h/1', 'D/w/15'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('X/halo8/h/8',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('X/halo8/w/8',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d',
                                                                                                                                    'D/h/8',
                                                                                                                                    'D/h/9',
                                                                                                                                    'D/w/8',
                                                                                                                                    'D/w/9')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm256/0', 'A/1x1s1/mfma32/0',
                                                                               'A/3x3/bm256/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/d1/w/le_2d', 'B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',)},
 {"at 146x215 the form ran there under another variant than the class's (the hook or size rule of the case picks it)": ('E/wg128/1',
                                                                                                                        'E/wg128/other'),
  "at 241x258 the form ran there under another variant than the class's (the hook or size rule of the case picks it)": ('E/wg128/bm-1',),
  "at 5x93 the form ran there under another variant than the class's (the hook or size rule of the case picks it)": ('E/wg128/lt',),
  'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('E/wg128/0',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm128/0', 'A/1x1s1/mfma32/0',
                                                                               'A/1x1s2/bm128/0', 'A/1x1s2/mfma32/0',
                                                                               'A/3x3/bm128/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/1x1s2/bm128/other',),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/w/le_2d',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm64/0', 'A/1x1s1/mfma32/0',
                                                                               'A/1x1s2/bm64/0', 'A/1x1s2/mfma32/0', 'A/3x3/bm64/0',
                                                                               'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/1x1s2/bm64/other',),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/w/le_2d',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm128/0', 'A/1x1s1/mfma32/0',
                                                                               'A/1x1s2/bm128/0', 'A/1x1s2/mfma32/0',
                                                                               'A/3x3/bm128/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/1x1s2/bm128/other', 'A/3x3/bm128/other'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm256/0', 'A/1x1s1/mfma32/0',
                                                                               'A/1x1s2/bm256/0', 'A/1x1s2/mfma32/0',
                                                                               'A/3x3/bm256/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/1x1s2/bm256/other',),
  'no cover size puts a layer of the form into it; 3x5 of forms.py does': ('B/s2/h/le_d', 'B/s2/w/le_2d'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/w/le_2d',)},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('A/1x1s1/bm256/0', 'A/1x1s1/mfma32/0',
                                                                               'A/1x1s2/bm256/0', 'A/1x1s2/mfma32/0',
                                                                               'A/3x3/bm256/0', 'A/3x3/mfma32/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('A/1x1s2/bm256/other', 'A/3x3/bm256/other'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d',),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d',),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/h/le_2d',
                                                                                                                                    'B/d1/w/le_2d')},
 {'no cover size puts a layer of the form into it; 128x128 of forms.py does': ('D/h/0', 'D/w/0'),
  'no cover size puts a layer of the form into it; 135x241 of forms.py does': ('D/h/1', 'D/w/15'),
  'no cover size puts a layer of the form into it; 64x256 of forms.py does': ('B/d4/h/le_2d', 'X/halo8/h/8'),
  'no cover size puts a layer of the form into it; 97x61 of forms.py does': ('B/d4/w/le_2d', 'D/h/9', 'X/halo8/w/8'),
  'only frames outside the committed sizes put a layer of THIS form into it; the committed sizes reach the class on other layers': ('B/d1/w/le_2d',
                                                                                                                                    'D/w/8')}]
OMITTED = {'f32-cfg0': _OMITTED_SETS[0], 'f32-cfg1': _OMITTED_SETS[1], 'f32-cfg2': _OMITTED_SETS[2], 'f32-cfg3': _OMITTED_SETS[3], 'f32-cfg4': _OMITTED_SETS[4], 'f32-cfg5': _OMITTED_SETS[5], 'f32-cfg6': _OMITTED_SETS[6], 'f32-cfg7': _OMITTED_SETS[0], 'f32-cfg8': _OMITTED_SETS[2], 'f32-cfg9': _OMITTED_SETS[1], 'f32-cfg10': _OMITTED_SETS[3], 'f32-cfg11': _OMITTED_SETS[7], 'f32-cfg12': _OMITTED_SETS[6], 'f32s-cfg0': _OMITTED_SETS[0], 'f32s-cfg1': _OMITTED_SETS[1], 'f32s-cfg2': _OMITTED_SETS[2], 'f32s-cfg3': _OMITTED_SETS[3], 'f32s-cfg4': _OMITTED_SETS[4], 'f32s-cfg5': _OMITTED_SETS[5], 'f32s-cfg6': _OMITTED_SETS[6], 'f32s-cfg7': _OMITTED_SETS[0], 'f32s-cfg8': _OMITTED_SETS[2], 'f32s-cfg9': _OMITTED_SETS[1], 'f32s-cfg10': _OMITTED_SETS[3], 'f32s-cfg11': _OMITTED_SETS[7], 'f32s-cfg12': _OMITTED_SETS[6], 'f32x-cfg0': _OMITTED_SETS[0], 'f32x-cfg1': _OMITTED_SETS[1], 'f32x-cfg2': _OMITTED_SETS[2], 'f32x-cfg3': _OMITTED_SETS[3], 'f32x-cfg4': _OMITTED_SETS[4], 'f32x-cfg5': _OMITTED_SETS[5], 'f32x-cfg6': _OMITTED_SETS[6], 'f32x-cfg7': _OMITTED_SETS[0], 'f32x-cfg8': _OMITTED_SETS[2], 'f32x-cfg9': _OMITTED_SETS[1], 'f32x-cfg10': _OMITTED_SETS[3], 'f32x-cfg11': _OMITTED_SETS[7], 'f32x-cfg12': _OMITTED_SETS[6], 'f16-cfg0': _OMITTED_SETS[0], 'f16-cfg1': _OMITTED_SETS[1], 'f16-cfg2': _OMITTED_SETS[2], 'f16-cfg3': _OMITTED_SETS[3], 'f16-cfg4': _OMITTED_SETS[4], 'f16-cfg5': _OMITTED_SETS[5], 'f16-cfg6': _OMITTED_SETS[6], 'f16-cfg7': _OMITTED_SETS[0], 'f16-cfg8': _OMITTED_SETS[2], 'f16-cfg9': _OMITTED_SETS[1], 'f16-cfg10': _OMITTED_SETS[3], 'f16-cfg11': _OMITTED_SETS[7], 'f16-cfg12': _OMITTED_SETS[6], 'f16-cfg13': _OMITTED_SETS[7], 'f16-cfg14': _OMITTED_SETS[6], 'f16-cfg15': _OMITTED_SETS[8], 'f16-cfg16': _OMITTED_SETS[7], 'f16-cfg17': _OMITTED_SETS[6], 'f16-cfg19': _OMITTED_SETS[9], 'f16-cfg20': _OMITTED_SETS[10], 'f16-cfg21': _OMITTED_SETS[11], 'f16hl-cfg0': _OMITTED_SETS[2], 'f16hl-cfg0-plain': _OMITTED_SETS[2], 'f16hl-cfg5': _OMITTED_SETS[5], 'f16hl-cfg5-plain': _OMITTED_SETS[5], 'f16hl-cfg6': _OMITTED_SETS[12], 'f16hl-cfg6-plain': _OMITTED_SETS[12], 'f16hl-cfg11': _OMITTED_SETS[7], 'f16hl-cfg11-plain': _OMITTED_SETS[7], 'f16hl-cfg12': _OMITTED_SETS[12], 'f16hl-cfg12-plain': _OMITTED_SETS[12], 'f16hl-cfg13': _OMITTED_SETS[7], 'f16hl-cfg13-plain': _OMITTED_SETS[7], 'f16hl-cfg14': _OMITTED_SETS[5], 'f16hl-cfg14-plain': _OMITTED_SETS[5], 'f16hl-cfg15': _OMITTED_SETS[8], 'f16hl-cfg15-plain': _OMITTED_SETS[8], 'f16hl-cfg16': _OMITTED_SETS[5], 'f16hl-cfg16-plain': _OMITTED_SETS[5], 'f16hl-cfg17': _OMITTED_SETS[12], 'f16hl-cfg17-plain': _OMITTED_SETS[12], 'sub:f32-cfg0-WINO_LDS=0': _OMITTED_SETS[0], 'sub:f32-cfg0-WINO_VEC=1': _OMITTED_SETS[0], 'sub:f32-cfg0-WINO_VEC=2': _OMITTED_SETS[0], 'sub:f32-cfg0-WINO_VEC=2-F2': _OMITTED_SETS[0], 'sub:f32-cfg0-WINO_VEC=2-F4': _OMITTED_SETS[0], 'sub:f16-cfg15-AREG_BM=256': _OMITTED_SETS[13], 'sub:f16-cfg19': _OMITTED_SETS[9], 'sub:f16-cfg19-HALO_BN=128': _OMITTED_SETS[9], 'sub:f16-cfg20': _OMITTED_SETS[10], 'sub:f16-cfg0-B2B=1-B2B_DMA=0': _OMITTED_SETS[0], 'sub:f16-cfg0-B2B=1-B2B_DMA=1': _OMITTED_SETS[0], 'sub:f16-cfg0-B2B=1-B2B_FORM=1': _OMITTED_SETS[0], 'sub:f16-cfg0-B2B=1-B2B_FORM=2': _OMITTED_SETS[0], 'sub:f16-cfg0-STEM_F32=1': _OMITTED_SETS[0], 'sub:f32s-cfg0-STEM_F32=1': _OMITTED_SETS[0], 'i8-cfg0': _OMITTED_SETS[14], 'i8-cfg1': _OMITTED_SETS[15], 'i8-cfg2': _OMITTED_SETS[14], 'i8-cfg3': _OMITTED_SETS[15], 'i8-cfg4': _OMITTED_SETS[4], 'i8-cfg5': _OMITTED_SETS[16], 'i8-cfg6': _OMITTED_SETS[17], 'i8-cfg7': _OMITTED_SETS[14], 'i8-cfg8': _OMITTED_SETS[14], 'i8-cfg9': _OMITTED_SETS[15], 'i8-cfg10': _OMITTED_SETS[15], 'i8-cfg11': _OMITTED_SETS[18], 'i8-cfg12': _OMITTED_SETS[17], 'i8-cfg13': _OMITTED_SETS[18], 'i8-cfg14': _OMITTED_SETS[17], 'i8-cfg15': _OMITTED_SETS[8], 'i8-cfg16': _OMITTED_SETS[18], 'i8-cfg17': _OMITTED_SETS[17], 'i8-cfg18': _OMITTED_SETS[8], 'i8-cfg19': _OMITTED_SETS[19], 'i8-cfg20': _OMITTED_SETS[10], 'sub:i8-cfg18': _OMITTED_SETS[8], 'sub:i8-cfg18-Q8_NSPLIT=2': _OMITTED_SETS[8], 'sub:i8-cfg18-Q8_NSPLIT=4': _OMITTED_SETS[8], 'sub:i8-cfg18-Q8_NSPLIT=8': _OMITTED_SETS[8]}


def omitted(case):
    """class -> reason"""
    return {c: reason for reason, classes in OMITTED.get(case, {}).items() for c in classes}
