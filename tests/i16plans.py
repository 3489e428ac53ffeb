"""The int16 launch planner's space, restated on plain numbers (no GPU, no library).

csrc/yolo2_int16.hip decides per conv launch and batch which kernel and shape run: `autotune` enumerates candidates, `plan_conv`
re-validates every field, and a plan line  B L S path P pad splitk pp w16 fuse hiacc ks  (config/plan_gfx950.txt, option plan_file)
is applied only if plan_conv reproduces it exactly.  This module restates

  parse_line   y2_plan_line_parse (csrc/yolo2_plan.hip): the ranges a line must be in
  candidates   the shapes autotune hands to plan_conv for one launch (its 34 `cfgx` values) + the conv + pool fusion it times
  refusal      the rule of plan_conv (or of the fusion set-up) that refuses a shape, None if the shape is legal; RULES cites the
               source line of each (tests/test_i16_plans_host.py checks that the cited text is still on that line)
  pack         plan files in which file k pins every launch of every conv layer to its k-th shape

so that tests/test_gpu_i16_plans.py can pin the whole network to one exact shape per launch, prove that it took, and compare bits.
Nothing here depends on the batch except the K-split's `kKsMaxBatch`: tile_items_bound does not read the frame count, and both
sides of y2_ks_fits scale with it.
"""
import os
import re
from collections import namedtuple

import numpy as np

from yolo2_amd import net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
TABLE = os.path.join(PKG, "config", "plan_gfx950.txt")
SRC = os.path.join(PKG, "csrc", "yolo2_int16.hip")

Line = namedtuple("Line", "B L S path P pad splitk pp w16 fuse hiacc ks")
Shape = namedtuple("Shape", "P pad splitk pp w16 fuse hiacc ks")        # a line without its key and arithmetic form
Launch = namedtuple("Launch", "L S path n_launches splitk_ok fusable")  # what the loader proved for one launch of conv layer L

PADS = (0, 160 * 1024 // 6, 160 * 1024 // 4)
RANGES = dict(path=(0, 1, 2, 3, 4), P=(1, 2, 4, 8), pad=PADS, splitk=(0, 4, 8), pp=(1, 2, 4), w16=(0, 1), fuse=(0, 1), hiacc=(0, 1),
              ks=(0, 2, 4, 8, 16))
K_MAX_TILE_ITEMS = 2048     # y2_internal.hpp kMaxTileItems
K_KS_MAX_BATCH = 4          # yolo2_int16.hip kKsMaxBatch
FUSE_LAYERS = (0, 2, 6, 10, 16)
CONV_IDX = [l.idx for l in net.CONVS]


def shape_of(line):
    return Shape(*line[4:])


def parse_line(text):
    """y2_plan_line_parse: a Line, or None for a comment, fewer than 10 leading integers (hiacc and ks default to 0) or a field
    outside the planner's ranges."""
    if text.startswith("#"):
        return None
    v = []
    for tok in text.split()[:12]:
        if not re.fullmatch(r"[+-]?\d+", tok):
            break
        v.append(int(tok))
    if len(v) < 10:
        return None
    ln = Line(*(v + [0, 0])[:12])
    if not (0 < ln.B <= 4096 and 0 <= ln.L < 32 and 0 <= ln.S <= 8):
        return None
    if any(getattr(ln, f) not in ok for f, ok in RANGES.items()):
        return None
    return ln


def read_table(path=TABLE):
    """The lines of a plan file as the loader keeps them: {(B, L, S): Line}, a later line for the same key wins."""
    out = {}
    for text in open(path):
        ln = parse_line(text)
        if ln is not None:
            out[(ln.B, ln.L, ln.S)] = ln
    return out


# ---------------------------------------------------------------------------- geometry (csrc/layout.hpp)

def tile_items_bound(l, T, halo):
    rows, frames = (T - 1) // l.w + 1, (T - 1) // (l.h * l.w) + 1
    return T + rows + frames * (l.w + 1) + 2 * halo + 1


def pool_tile_items_bound(l):
    ow, ohw = l.w // 2, (l.h // 2) * (l.w // 2)
    wraps, frames = min(63, (63 + ow - 1) // ow), min(63, (63 + ohw - 1) // ohw)
    return 126 + wraps * (l.w + 2) + frames * (l.w + 1) + 3 * (l.w + 1) + 4


def ks_fits(ks, l, batch):
    """y2_ks_fits against ks_potential_bytes: 24 bytes per split, output item and pixel; room for 16 splits of 64 items x 2704 pixels
    per frame, none for batches past kKsMaxBatch."""
    cap = 0 if batch > K_KS_MAX_BATCH else 16 * 24 * 64 * 2704 * batch
    return cap != 0 and ks * ((l.n + 3) // 4) * (batch * l.h * l.w) * 24 <= cap


# ---------------------------------------------------------------------------- the rules

# name: (line of csrc/yolo2_int16.hip, text on that line)
RULES = {
    "maxP": (82, "const int maxP = (p.path == 1 || p.path == 3 || p.path == 4) ? 8 : 4;"),
    "tile_items": (91, "while (p.P > 1 && tile_items_bound(gin, 64 * p.P, halo) > kMaxTileItems) p.P >>= 1;"),
    "splitk_pp": (93, "if (p.splitk_pp > 1 && !(p.splitk == 4 && p.K == 3 && p.path == 4 && !opt.splitk_no_pack)) p.splitk_pp = 1;"),
    "splitk": (99, "if (!p.splitk_ok || (S != 4 && !(S == 8 && p.K == 1)) || gin.CG % S != 0 || gin.CG < 4 * S || S * (lt + p.K * p.K * 32) > kMaxTileItems) p.splitk = 0;"),
    "ks": (104, "if (p.splitk || p.mb_count || p.path != 4 || p.K != 3 || gin.CG % p.ks != 0 || gin.CG / p.ks < 2 || tile_items_bound(gin, 64, halo) > kMaxTileItems ||"),
    "ks_fits": (105, "!y2_ks_fits(p.ks, CGout, npix, p.ks_cap))"),
    "ks_shape": (107, "else { p.P = 1; p.w16 = 0; p.hiacc = 0; }"),
    "splitk_shape": (109, "if (p.splitk) p.P = 1;"),
    "w16": (112, "if (p.w16 && (p.splitk || p.K != 3 || (p.path != 3 && p.path != 4) || p.P > 2 || tile_items_bound(gin, 64 * p.P, halo) > 1024)) p.w16 = 0;"),
    "w16_pad": (131, "if (p.w16) p.lds_pad = 0;"),
    "hiacc": (132, "if (p.hiacc && (p.path != 4 || p.splitk || p.w16 || p.P > 4)) p.hiacc = 0;"),
    "ks_pad": (140, "if (p.ks) { p.grid.y *= p.ks; p.lds_pad = 0; }"),
    # conv + pool fusion: plan_conv_pool and setup_pool_fusion.  The only rule whose breach is not refused: apply_plan_lines keeps the
    # table and runs the separate kernels (line 888), so the launch a line with fuse=1 names there is never the one that runs.
    "fuse": (188, "if (p.K != 3 || (p.path != 3 && p.path != 4) || (gin.H & 1) || (gin.W & 1)) return false;"),
    "fuse_tile": (190, "if (lt > 12 * 256) return false;"),
    "fuse_layer": (925, "if (kNet[i + 1].type != L_MAX) continue;"),
}
# where the restated enumeration and the comparison live
CITES = {
    "candidates": (692, "for (int cfgx = 0; cfgx < 18 + 12 + 4; ++cfgx) {"),
    "no_cap_on_wide_tiles": (701, "if (pad && P > 2) continue;"),
    "splitk_offered": (711, "if (!sp->splitk_ok || !c->extra[i].empty() || fs == 0) continue;"),
    "ks_cap": (838, "cand.ks_cap = s == 0 ? ks_potential_bytes(c, c->batch) : 0;"),
    "exact": (842, "if (cand.P != pl.P || cand.lds_pad != pl.pad || cand.splitk != pl.splitk || cand.splitk_pp != pl.pp || cand.w16 != pl.w16 ||"),
    "fuse_chosen": (860, "for (int i = 0; i < 32; ++i) c->fuse_pool[i] = c->fuse_pool[i] && fuse[i];"),
}


def refusal(la, batch, sh):
    """The name (a key of RULES) of the first rule that keeps plan_conv from reproducing shape `sh` for launch `la` at `batch` -
    such a line sends the whole batch to the stopwatch - or None if the line is applied as it stands.  Follows plan_conv's order,
    because later rules read what earlier ones left (a refused split-K no longer stands in the way of ks, w16, hiacc)."""
    l = net.LAYERS[la.L]
    K, CG, path = l.size, (l.c + 3) // 4, la.path
    halo = l.w + 2 if K == 3 else 0
    P, splitk, pp, w16, hiacc, ks, pad = sh.P, sh.splitk, sh.pp, sh.w16, sh.hiacc, sh.ks, sh.pad
    if P > (8 if path in (1, 3, 4) else 4):
        return "maxP"
    if P > 1 and tile_items_bound(l, 64 * P, halo) > K_MAX_TILE_ITEMS:
        return "tile_items"
    if splitk:      # (pp is only looked at here: "splitk=0 pp=2" is reproduced as it stands, and means nothing)
        if pp > 1 and not (splitk == 4 and K == 3 and path == 4):
            return "splitk_pp"
        lt = tile_items_bound(l, 64 // splitk * pp, halo)
        if (not la.splitk_ok or (splitk != 4 and not (splitk == 8 and K == 1)) or CG % splitk or CG < 4 * splitk
                or splitk * (lt + K * K * 32) > K_MAX_TILE_ITEMS):
            return "splitk"
    if ks:
        if splitk or la.n_launches > 1 or path != 4 or K != 3 or CG % ks or CG // ks < 2 or tile_items_bound(l, 64, halo) > K_MAX_TILE_ITEMS:
            return "ks"
        if la.S != 0 or not ks_fits(ks, l, batch):
            return "ks_fits"
        if P != 1 or w16 or hiacc:
            return "ks_shape"
        if pad:
            return "ks_pad"
    if splitk and P != 1:
        return "splitk_shape"
    if w16:
        if splitk or K != 3 or path not in (3, 4) or P > 2 or tile_items_bound(l, 64 * P, halo) > 1024:
            return "w16"
        if pad:
            return "w16_pad"
    if hiacc and (path != 4 or splitk or w16 or P > 4):
        return "hiacc"
    if sh.fuse:     # (stated on launch 0; on another launch the field is not read)
        if la.S == 0 and la.L not in FUSE_LAYERS:
            return "fuse_layer"
        if la.S == 0 and not la.fusable:
            return "fuse"
        if la.S == 0 and pool_tile_items_bound(l) > 12 * 256:
            return "fuse_tile"
    return None


def legal(la, batch, sh):
    return refusal(la, batch, sh) is None


def candidates(la, batch):
    """What autotune enumerates for one launch, in its order, as (cfgx, Shape): 0..11 pixels per lane x occupancy cap, 12..15 the four
    lane-split forms, 16 / 17 sixteen channels per wavefront, 18..29 the first twelve again with one accumulator per channel (form D),
    30..33 the K-split over 2 / 4 / 8 / 16 workgroups - before plan_conv has its say (`refusal`).  cfgx 34 is not autotune's: the
    conv + pool fusion that setup_pool_fusion times afterwards, stated on a one-pixel tile (the fused kernel has one shape)."""
    out = []
    for cfgx in range(18 + 12 + 4):
        ks = 2 << (cfgx - 30) if cfgx >= 30 else 0
        cfg = 3 if ks else (cfgx - 18 if cfgx >= 18 else cfgx)
        hiacc = cfgx >= 18 and not ks
        if hiacc and la.path != 4:
            continue
        if ks and batch > K_KS_MAX_BATCH:
            continue
        w16 = cfg >= 16
        P = cfg - 15 if w16 else (1 if cfg >= 12 else 8 >> (cfg & 3))
        pad = 0 if cfg >= 12 else PADS[cfg >> 2]
        if pad and P > 2:
            continue
        splitk = pp = 0
        if 12 <= cfg < 16:
            if not la.splitk_ok or la.n_launches > 1:
                continue
            splitk, pp = (8 if cfg == 13 else 4), (2 if cfg == 14 else 4 if cfg == 15 else 1)
        out.append((cfgx, Shape(P, pad, splitk, pp or 1, int(w16), 0, int(hiacc), ks)))
    if la.S == 0 and la.L in FUSE_LAYERS:
        out.append((34, Shape(1, 0, 0, 1, 0, 1, 0, 0)))
    return out


def kernel_of(la, sh):
    """The kernel a legal shape runs (launch_conv's order)."""
    if sh.fuse and la.S == 0:
        return "k_conv_i16_pool"
    return "k_conv_i16_ks" if sh.ks else "k_conv_i16_w16" if sh.w16 else "k_conv_i16_splitk" if sh.splitk else "k_conv_i16"


def expected_plan(la, sh):
    """What yolo2_hip_conv_plan_string must state for launch 0 of a layer planned from a legal line.  The fused kernel has one shape."""
    if sh.fuse:
        return dict(P=4, pad=0, w16=0, hiacc=0, ks=0, splitk=0, pp=1, fused=2 if la.L == 16 else 1)
    return dict(P=sh.P, pad=sh.pad, w16=sh.w16, hiacc=sh.hiacc, ks=sh.ks, splitk=sh.splitk, pp=sh.pp, fused=0)


def plan_fields(text):
    """"P=1 pad=0 ... edge=0" -> {"P": 1, ...}"""
    return {k: int(v) for k, v in (kv.split("=") for kv in text.split())}


# ---------------------------------------------------------------------------- what the loader proves (resolve_q), from the model

def _launches(forms_by_ord, splitk_ok):
    out = {}
    for l in net.CONVS:
        forms = forms_by_ord[l.ord]
        fusable = l.idx in FUSE_LAYERS and all(f in (3, 4) for f in forms)
        for s, f in enumerate(forms):
            out[(l.idx, s)] = Launch(l.idx, s, f, len(forms), True if splitk_ok is None else bool(splitk_ok[l.ord]), fusable)
    return out


def launches_from_counts(path_counts, splitk_ok=None):
    """The launches of every conv layer from the per-form block counts of yolo2_hip_layer_path_counts: the form with most blocks
    (the first of equals) is launch 0, the others follow in ascending order of form.  splitk_ok: per ordinal (splitk_proved);
    None takes the proof for granted."""
    forms = []
    for l in net.CONVS:
        counts = list(path_counts[l.ord])
        dom = max(range(5), key=lambda k: (counts[k], -k))
        forms.append([dom] + [k for k in range(5) if k != dom and counts[k]])
    return _launches(forms, splitk_ok)


def launches_from_table(table, batch, splitk_ok=None):
    """The same from the `path` column of a complete plan table (it states the forms of the model it was measured on)."""
    forms = []
    for l in net.CONVS:
        f = []
        while (batch, l.idx, len(f)) in table:
            f.append(table[(batch, l.idx, len(f))].path)
        assert f, f"batch {batch} has no line for layer {l.idx}"
        forms.append(f)
    return _launches(forms, splitk_ok)


def splitk_proved(model):
    """resolve_q's bound for the lane-split kernel, per conv ordinal: the layer runs a 32-bit form, every increment stays below 2^29
    and the unclamped sum of one split below 2^30 (maxsum = the largest sum of |w| over the 4 input channels of one tap)."""
    aq = [int(x) for x in model.act_q]
    out, route24_q, pending = [], 0, None
    for l in net.LAYERS:
        if l.type == net.REORG:
            if route24_q > 0:
                pending = min(route24_q, cur)
            continue
        if l.type != net.CONV:
            continue
        o = l.ord
        qa_in = aq[o] if pending is None else pending
        qa_out = aq[o + 1]
        pending, cur = None, qa_out
        if l.idx == 24:
            route24_q = cur
        so, sb = qa_in + int(model.weight_q[o]) - qa_out, int(model.bias_q[o]) - qa_out
        w = np.abs(model.w_nat[o].astype(np.int64)).reshape(l.n, l.c, l.size * l.size)
        if l.c % 4:
            w = np.concatenate([w, np.zeros((l.n, 4 - l.c % 4, w.shape[2]), np.int64)], axis=1)
        maxsum = int(w.reshape(l.n, -1, 4, w.shape[2]).sum(axis=2).max())
        bias0 = int(np.abs(model.bias[o].astype(np.int64)).max())
        if so < 0:
            out.append(False)
            continue
        mag, bmag = min(so, 30), min(abs(sb), 30)
        rnd = (1 << (mag - 1)) if mag > 0 else 0
        if sb > 0:
            bias0 = ((bias0 + ((1 << (bmag - 1)) if bmag > 0 else 0)) >> bmag) + 1
        elif sb < 0:
            bias0 <<= bmag
        accmax, pmax = max(32768, bias0), maxsum * 32768
        ok32 = bias0 <= 2147483647 and (pmax + rnd + accmax <= 2147483647 or (accmax << mag) + rnd + pmax <= 2147483647)
        tmax = (pmax + rnd) >> mag
        steps = ((l.c + 3) // 4 // 4 + 1) * l.size * l.size
        out.append(bool(ok32 and tmax < (1 << 29) and tmax * steps < (1 << 30)))
    return out


# ---------------------------------------------------------------------------- plan files

def distinct_table_shapes(table):
    """{(L, S): [Line ...]} - the distinct (path, shape) of every launch over all batches of the table, in order of first appearance."""
    out = {}
    for (B, L, S) in sorted(table):
        ln = table[(B, L, S)]
        got = out.setdefault((L, S), [])
        if not any(g[3:] == ln[3:] for g in got):
            got.append(ln)
    return out


def pack(per_launch, launches, batch, outdir, tag, count=None):
    """Plan files for `batch`: file k gives every launch its k-th shape of per_launch[(L, S)] (a list of Shape), a launch with fewer
    shapes its last.  Returns [(file name, {(L, S): Shape})].  Every file has a name of its own: the library keeps a table per name.
    count: write that many files (not fewer than the longest list needs; the surplus repeats the last file under other names)."""
    assert set(per_launch) == set(launches) and all(per_launch.values())
    need = max(len(v) for v in per_launch.values())
    assert count is None or count >= need, (count, need)
    files = []
    for k in range(need if count is None else count):
        chosen = {key: v[min(k, len(v) - 1)] for key, v in per_launch.items()}
        name = os.path.join(str(outdir), f"{tag}_b{batch}_{k:02d}.txt")
        with open(name, "w") as f:
            f.write("# B L S path P pad splitk pp w16 fuse hiacc ks\n")
            for (L, S) in sorted(chosen):
                sh = chosen[(L, S)]
                f.write(" ".join(str(x) for x in (batch, L, S, launches[(L, S)].path) + tuple(sh)) + "\n")
        files.append((name, chosen))
    return files


def replay_lists(table, launches, batch):
    """Item 3's lists: for every launch the table's distinct shapes whose form is the one proved for this model and which are legal at
    `batch` for that form (for the model the table was measured on: all of them)."""
    per, distinct = {}, distinct_table_shapes(table)
    for key, la in launches.items():
        lines = distinct.get(key) or distinct[(key[0], 0)]      # (a launch the table's model does not have: the layer's shapes)
        shapes = []
        for ln in lines:
            sh = shape_of(ln)
            if legal(la, batch, sh) and sh not in shapes:
                shapes.append(sh)
        per[key] = shapes or [Shape(1, 0, 0, 1, 0, 0, 0, 0)]
    return per


def sweep_lists(launches, batch):
    """Item 4's lists: every candidate of the tuner that plan_conv accepts."""
    return {key: [sh for _, sh in candidates(la, batch) if legal(la, batch, sh)] for key, la in launches.items()}
