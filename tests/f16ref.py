"""fp64 reference of every launch of the fp16 and split-fp16 passes, and the per-launch checker (CPU only).

The GPU's tensors are read back raw (yolo2_hip_debug_f16_tensor: items of Cp halves per pixel, plain fp16 or split [hi | lo | hi]
parts).  Each launch of the launch table is judged ALONE: its reference input is the GPU's own decoded input tensor, its reference
output is computed in float64 with exactly the rounding the design applies (table KERNELS), and the GPU output is compared with it

  (1) element by element against a hard bound that cannot flake: the deterministic fp32 summation bound gamma_n * S
      (S = sum |a w| + |bias|, carried through leaky / pool, and through a fused 1x1 by convolving it with |w2|) plus half an
      output ulp;
  (2) statistically, in output units, separately on each partition (four border lines, interior, every 32-channel block, the
      last partial 256-pixel tile of a ragged batch), so that a dropped tap, a wrong 32-channel block or a shifted tile cannot be
      averaged away by the rest of the tensor.

Unit of (2):
  * fp16 outputs: e = (gpu - fl16(ref)) / ulp16(fl16(ref)).  A legal kernel differs from fl16(ref) only where its fp32 sum lies on
    the other side of a rounding midpoint: e in {-1, 0, 1}, mostly 0.
  * split (hi + lo) and fp32 outputs (the region layer): e = (gpu - ref) / u with u = 2^-22 sqrt(n sum (a w)^2) + 2^-22 |ref| + 2^-24.
    The representation itself is good to ~2^-22 |v|, so what a legal kernel shows is fp32 summation noise: a sequential fp32 sum of n
    terms has an rms error of about 2^-24 sqrt(n sum (a w)^2 / 6) = u / 10; blocked (MFMA) sums less.

Thresholds (STAT_LIMITS) and their derivation: see the comment there and tests/test_f16_layer_ref.py, which measures them on
simulated legal kernels and on mutated ones.
"""
import numpy as np
import torch
import torch.nn.functional as F

from yolo2_amd import net

torch.set_num_threads(16)

LEAKY = float(np.float32(0.1))       # the kernels multiply by 0.1f
U32 = 2.0 ** -24                     # fp32 unit roundoff

# ------------------------------------------------------------------ rounding model per kernel name
#
# op: conv0 (layers 0 + 1 from the float frames), conv (input = the items as they are: fp16, or split hi + lo), pool, reorg.
# x / w for conv0: what the kernel multiplies: "f16" = fp16 RNE of the fp32 value, "f32" = the fp32 value, "split" = (hi, lo) with
# products hi.hi + lo.hi + hi.lo.  conv layers >= 2 take the weights as the path packs them (fp16 RNE, or [w_hi | w_hi | w_lo]) and
# store fp16 RNE or the (hi, lo) split; bias and leaky in fp32 always.  inter: the fused 3x3 -> 1x1 launches round the 3x3's leaky'd
# result to fp16 (it passes through LDS as halves).  paths: which pass may run the kernel.
_F, _S, _B = ("fp16",), ("split",), ("fp16", "split")
KERNELS = {
    "k_conv0_pool_mfma": dict(op="conv0", x="f16", w="f16", paths=_F),
    "k_conv0_pool_f16": dict(op="conv0", x="f32", w="f32", paths=_F),
    "k_conv0_pool_mfma<split>": dict(op="conv0", x="split", w="split", paths=_S),
    "k_conv0_pool_f16<split>": dict(op="conv0", x="f32", w="f32", paths=_S),
    "k_maxpool2_f16": dict(op="pool", paths=_F),
    "k_maxpool2_split": dict(op="pool", paths=_S),
    "k_reorg_f16": dict(op="reorg", paths=_F),
    "k_reorg_split": dict(op="reorg", paths=_S),
    "k_conv_f16_rw<+1x1>": dict(op="conv", inter="f16", paths=_F),
    "k_conv_f16_rwb<+1x1>": dict(op="conv", inter="f16", paths=_F),
    "k_conv_f16_halo<256,2,16>+1x1": dict(op="conv", inter="f16", paths=_F),
    "k_gemm1_f16_p<256,64,3>": dict(op="conv", paths=_B),     # (layer 30 of both passes)
    "k_gemm1_f16_p<256,128,3>": dict(op="conv", paths=_B),
}
for _k in ("k_conv_f16_rwc", "k_conv_f16_rw<pool>", "k_conv_f16_rwb<pool>", "k_conv_f16_rw", "k_gemm1_f16_p<256,256,2>",
           "k_gemm1_f16_p<128,256,3>", "k_conv_f16_c32_pool", "k_conv_f16_glds<64>", "k_conv_f16<128,64,64>", "k_conv_f16<128,64,32>",
           "k_conv_f16_halo_p<256,16,32>", "k_conv_f16_halo_p<256,16,16>", "k_conv_f16_halo_p<128,8,32>", "k_conv_f16_halo_p<128,8,16>",
           "k_conv_f16_halo<256,2,16,16>", "k_conv_f16_halo<256,2,16>", "k_conv_f16_halo<256,2>", "k_conv_f16_halo<128,3>",
           "k_conv_f16_glds<128>", "k_conv_f16<128,128,64>", "k_conv_f16<128,128,32>"):
    KERNELS[_k] = dict(op="conv", paths=_F)
for _k in ("k_conv_f16_glds<64,split>", "k_conv_f16_halo_p<256,16,32,split>", "k_conv_f16_halo_p<128,8,32,split>",
           "k_conv_f16_halo<256,2,16,32,split>", "k_conv_f16_halo<128,3,8,32,split>", "k_conv_f16_glds<128,split>"):
    KERNELS[_k] = dict(op="conv", paths=_S)


def rounding_of(kernel, path):
    """The table entry of `kernel`; a kernel the table does not know fails (a new kernel cannot ship unchecked)."""
    if kernel not in KERNELS:
        raise KeyError(f"kernel {kernel!r} has no rounding model in tests/f16ref.py KERNELS: add it before it ships")
    r = KERNELS[kernel]
    if path not in r["paths"]:
        raise KeyError(f"kernel {kernel!r} is not expected on the {path} pass")
    return r


# ------------------------------------------------------------------ fp16 helpers

def fl16(x):
    """fp16 round-to-nearest-even of float64 values, back as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def ulp16(x):
    """Spacing of fp16 numbers at |x| (2^-24 in the subnormal range)."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10)


def split_pair(v):
    """(hi, lo) of the design: hi = fp16(fp32 v), lo = fp16(fp32 v - hi) (the difference is exact in fp32)."""
    v32 = np.asarray(v, dtype=np.float32).astype(np.float64)
    hi = fl16(v32)
    return hi, fl16(v32 - hi)


def gamma(n):
    k = n * U32
    return k / (1.0 - k)


# ------------------------------------------------------------------ item layout

def decode(raw, geom, split):
    """Raw items [PL][Cp] (uint16) of one frame -> dense float64 [C][H][W] (split: hi + lo, both returned as well).
    Returns dict(v, hi, lo) and checks that a split item's second hi copy equals the first."""
    C, Cp, H, W, Wp, ps, off = (geom[k] for k in ("C", "Cp", "H", "W", "Wp", "part_stride", "ch_off"))
    h = raw.view(np.float16).reshape(H + 1, Wp, Cp)[1:, :W, :]
    if not split:
        hi = h[:, :, off:off + C].astype(np.float64).transpose(2, 0, 1)
        return dict(v=hi, hi=hi, lo=np.zeros_like(hi))
    p0 = h[:, :, off:off + C]
    p1 = h[:, :, ps + off:ps + off + C]
    p2 = h[:, :, 2 * ps + off:2 * ps + off + C]
    if not np.array_equal(p0.view(np.uint16), p2.view(np.uint16)):
        bad = np.argwhere(p0.view(np.uint16) != p2.view(np.uint16))
        raise AssertionError(f"split items: the second hi copy differs from the first at {len(bad)} places, first (y, x, c) {bad[0]}")
    hi = p0.astype(np.float64).transpose(2, 0, 1)
    lo = p1.astype(np.float64).transpose(2, 0, 1)
    return dict(v=hi + lo, hi=hi, lo=lo)


def encode(v, geom, split):
    """Inverse of decode for tests: dense [C][H][W] values -> raw items [PL][Cp] uint16 with zero padding (split: (hi, lo) of v)."""
    C, Cp, H, W, Wp, ps, off = (geom[k] for k in ("C", "Cp", "H", "W", "Wp", "part_stride", "ch_off"))
    items = np.zeros((H + 1, Wp, Cp), dtype=np.float16)
    t = np.asarray(v, dtype=np.float64).transpose(1, 2, 0)
    if split:
        hi, lo = split_pair(t)
        items[1:, :W, off:off + C] = hi
        items[1:, :W, ps + off:ps + off + C] = lo
        items[1:, :W, 2 * ps + off:2 * ps + off + C] = hi
    else:
        items[1:, :W, off:off + C] = fl16(t)
    return items.reshape(-1, Cp).view(np.uint16)


def make_geom(C, H, W, split, ch_off=0, C_items=None):
    """Geometry of the tensor a layer of C channels lives in (C_items: the channel count the items are sized for, 1280 for h_cat)."""
    Ci = C_items or C
    ps = (Ci + 31) // 32 * 32
    Cp = (3 * ps + 63) // 64 * 64 if split else ps
    return dict(C=C, Cp=Cp, H=H, W=W, Wp=W + 1, items=(H + 1) * (W + 1), part_stride=ps if split else Cp, ch_off=ch_off)


def padding_violations(raw, geom, split):
    """Places of a frame's items that must hold exact zeros and do not: the pad row and column, channels beyond C (split: each part's
    tail up to the part stride and the [3 part_stride, Cp) tail).  Returns a list of strings (empty = clean)."""
    C, Cp, H, W, Wp, ps, off = (geom[k] for k in ("C", "Cp", "H", "W", "Wp", "part_stride", "ch_off"))
    it = raw.reshape(H + 1, Wp, Cp)
    bad = []
    if np.any(it[0]):
        bad.append("pad row")
    if np.any(it[:, W]):
        bad.append("pad column")
    live = np.zeros(Cp, dtype=bool)
    cat = ps == 1280                                       # (the concat tensor: the other layer's channels live there too)
    lo_c, hi_c = (0, 1280) if cat else (off, off + C)
    for p in range(3 if split else 1):
        live[p * ps + lo_c:p * ps + hi_c] = True
    if np.any(it[1:, :W][:, :, ~live]):
        bad.append("channels beyond C")
    return bad


# ------------------------------------------------------------------ the network's steps

def step_layers(table, first):
    """Layers a launch covers: from its own layer up to the next launch's, minus routes and the region layer."""
    later = sorted(l for l in table if l > first)
    end = later[0] if later else 32
    return [l for l in range(first, end) if net.LAYERS[l].type in (net.CONV, net.MAXPOOL, net.REORG)]


def input_layer(layer):
    """The layer whose output tensor a layer reads (28 = the concat of 27 and 24)."""
    return {26: 16, 29: 28}.get(layer, layer - 1)


class Weights:
    """Per-conv-layer weights [N][C][K][K] (float64 of the fp32 values) and biases, from SynthModel.weights_nat_f32()."""

    def __init__(self, model):
        wn, b = model.weights_nat_f32(), model.bias_f32()
        self.w, self.b = {}, {}
        wo = bo = 0
        for l in net.CONVS:
            n = l.n * l.c * l.size * l.size
            self.w[l.idx] = wn[wo:wo + n].astype(np.float64).reshape(l.n, l.c, l.size, l.size)
            self.b[l.idx] = b[bo:bo + l.n].astype(np.float64)
            wo += n
            bo += l.n


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))[None]


def _conv(x, w, K):
    return F.conv2d(_t(x), torch.from_numpy(np.ascontiguousarray(w)), padding=K // 2)[0].numpy()


def conv_ref(l, x_parts, w_parts, bias, out_kind, leaky_slope=LEAKY, mutate=None):
    """One conv layer in float64: sum over the (x, w) pairs of products the design takes, + bias, leaky.
    Returns dict(v = exact value of the design's arithmetic, e = deterministic fp32 bound, q = sum (a w)^2, n = products)."""
    K = l.size
    n = l.c * K * K * len(x_parts)
    v = sum(_conv(x, w, K) for x, w in zip(x_parts, w_parts))
    S = sum(_conv(np.abs(x), np.abs(w), K) for x, w in zip(x_parts, w_parts))
    q = sum(_conv(x * x, w * w, K) for x, w in zip(x_parts, w_parts))
    bias = bias.copy()
    if mutate and mutate[0] == "no_bias_block":
        blk = min(mutate[1], (len(bias) - 1) // 32)
        bias[32 * blk:32 * blk + 32] = 0.0
    v = v + bias[:, None, None]
    e = gamma(n + 2) * (S + np.abs(bias)[:, None, None])
    slope = np.ones_like(v)
    if l.leaky:
        slope = np.where(v < 0, leaky_slope, 1.0)
        v = v * slope
    return dict(v=v, e=e, q=q * slope * slope, n=n)


def _round_out(r, kind):
    """Output rounding of a conv stage (kind f16 / split / f32): the hard bound grows by half an output ulp."""
    v, e = r["v"], r["e"]
    if kind == "f16":
        r["e"] = e + 0.5 * ulp16(np.abs(v) + e)
    elif kind == "split":
        r["e"] = e + 2.0 ** -22 * (np.abs(v) + e) + 2.0 ** -25
    else:
        r["e"] = e + U32 * (np.abs(v) + e)
    return r


def pool2(a):
    C, H, W = a.shape
    return a.reshape(C, H // 2, 2, W // 2, 2).max(axis=(2, 4))


def reorg(a):
    """Darknet legacy reorg (stride 2) of [64][26][26] -> [256][13][13], as the reference indexes it."""
    flat = a.reshape(-1)
    out = np.empty(256 * 169, dtype=a.dtype)
    o = np.arange(256 * 169)
    k = o // (26 * 416)
    rem = o - k * (26 * 416)
    j = rem // 26
    i = rem - j * 26
    out[:] = flat[(2 * i + (k & 1)) + 52 * (2 * j + (k >> 1))]
    return out.reshape(256, 13, 13)


def step_ref(path, kernel, layers, x, W, mutate=None):
    """Reference of one launch.  path: "fp16" / "split" / "exact" (no rounding anywhere: the wiring test); x: dict(v, hi, lo) of the
    input (layer 0: the float frame [3][416][416] as v); W: Weights.  Returns dict(ref, bound, unit, kind) with kind f16 / split /
    f32 (the unit's meaning: see the module doc) or exact (pool / reorg: bit-exact steps).
    mutate: a deliberate error (tests only), e.g. ("drop_channel", c), ("drop_border_tap", tap), ("shift_tile", t0), ("no_bias_block",
    blk), ("leaky", slope), ("pool_offset",), ("no_lo",), ("no_wlo",), ("rtz",)."""
    exact = path == "exact"
    rm = dict(op="conv", x="f32", w="f32") if exact and layers[0] == 0 else \
        (dict(op=net.LAYERS[layers[0]].type) if exact else rounding_of(kernel, path))
    if exact and rm["op"] == net.CONV:
        rm = dict(op="conv")
    if rm["op"] in ("pool", net.MAXPOOL):
        return dict(ref=pool2(x["v"]), kind="exact")
    if rm["op"] in ("reorg", net.REORG):
        return dict(ref=reorg(x["v"]), kind="exact")
    split = path == "split"
    out_kind = "exact" if exact else ("split" if split else "f16")
    slope = mutate[1] if mutate and mutate[0] == "leaky" else LEAKY
    cur = None
    e_in = None
    for i, L in enumerate(layers):
        l = net.LAYERS[L]
        if l.type == net.MAXPOOL:
            if mutate and mutate[0] == "pool_offset":     # window one row down (the last row repeats)
                cur = {k: (np.concatenate([a[:, 1:], a[:, -1:]], axis=1) if isinstance(a, np.ndarray) else a) for k, a in cur.items()}
            cur = {k: (pool2(a) if isinstance(a, np.ndarray) else a) for k, a in cur.items()}   # (e, q: max over the window)
            continue
        w = W.w[L]
        if mutate and mutate[0] == "drop_channel" and i == 0:
            w = w.copy()
            w[:, mutate[1]] = 0.0
        if i == 0:
            if L == 0 and not exact:
                xm, wm = rm["x"], rm["w"]
                xv = x["v"]
                xp = {"f16": [fl16(xv)], "f32": [xv], "split": None}[xm]
                if xm == "split":
                    xh, xl = split_pair(xv)
                    wh, wl = split_pair(w)
                    xp, wp = [xh, xl, xh], [wh, wh, wl]
                    if mutate and mutate[0] == "no_wlo":
                        xp, wp = [xh, xl], [wh, wh]
                else:
                    wp = [fl16(w)] if wm == "f16" else [w]
            elif exact:
                xp, wp = [x["v"]], [w]
            elif split:
                wh, wl = split_pair(w)
                if mutate and mutate[0] == "no_lo":
                    xp, wp = [x["hi"], x["hi"]], [wh, wl]
                elif mutate and mutate[0] == "no_wlo":             # only a_hi w_lo dropped: the tail part of the packed weights
                    xp, wp = [x["hi"], x["lo"]], [wh, wh]
                else:
                    xp, wp = [x["hi"], x["lo"], x["hi"]], [wh, wh, wl]
            else:
                xp, wp = [x["v"]], [fl16(w)]
            if mutate and mutate[0] == "drop_border_tap":
                r = conv_ref(l, xp, wp, W.b[L], out_kind, slope)
                t = mutate[1]                                       # tap index 0..8: its contribution removed on row 0 only
                wt = [np.zeros_like(a) for a in wp]
                for a, b_ in zip(wt, wp):
                    a[:, :, t // 3, t % 3] = b_[:, :, t // 3, t % 3]
                part = sum(_conv(xx, ww, l.size) for xx, ww in zip(xp, wt))
                dv = np.zeros_like(r["v"])
                dv[:, 0, :] = part[:, 0, :]
                pre = r["v"] / np.where(r["v"] < 0, slope, 1.0) if l.leaky else r["v"]
                pre = pre - dv
                r["v"] = pre * (np.where(pre < 0, slope, 1.0) if l.leaky else 1.0)
            else:
                r = conv_ref(l, xp, wp, W.b[L], out_kind, slope, mutate if L == layers[0] else None)
        else:   # a 1x1 fused behind the 3x3: input = the 3x3's result rounded to fp16 (KERNELS inter), its bound convolved with |w2|
            tin = cur["v"]
            e_t = cur["e"]
            if not exact:
                e_t = e_t + ulp16(np.abs(tin) + e_t)
                tin = fl16(tin)
            w2 = w if exact else fl16(w)
            r = conv_ref(l, [tin], [w2], W.b[L], out_kind, slope)
            r["e"] = r["e"] + _conv(e_t, np.abs(w2), l.size)
            # statistics: where the output is small against its terms, the intermediate's rounding dominates the output ulp.  A kernel's
            # fp32 sum lands on the other side of a midpoint in ~1 % of the intermediate's elements, each such flip moves the output by
            # ulp16(T_c) w2_c whatever the output's size: the unit of (2) is at least sqrt(sum_c (ulp16(T_c) w2_c)^2), the size of
            # one flip per channel.  (Measured on the GPU with the rms of uniform rounding, sqrt(1/12) of this, as the floor: 1.4e-3 of
            # the left column of layer 4 / 5 of the letterbox frame lay beyond one unit, at most 3, hard-bound ratio 0.11.)
            r["floor"] = np.sqrt(_conv(ulp16(tin) ** 2, w2 * w2, l.size))
            if l.leaky:
                r["floor"] = r["floor"] * np.where(r["v"] < 0, slope, 1.0)
        cur = r
    if not exact:
        cur = _round_out(cur, out_kind if not (layers[-1] == 30) else "f32")
    kind = "f32" if layers[-1] == 30 else out_kind
    # unit of the statistics (module doc)
    unit = None
    if kind in ("split", "f32"):
        unit = 2.0 ** -22 * np.sqrt(cur["n"] * cur["q"]) + 2.0 ** -22 * np.abs(cur["v"]) + 2.0 ** -24
    res = dict(ref=cur["v"], bound=cur["e"], unit=unit, kind=kind, floor=cur.get("floor"))
    if mutate and mutate[0] == "shift_tile":
        ref = res["ref"].copy()
        C, H, Wd = ref.shape
        flat = ref.reshape(C, -1)
        t0 = mutate[1]
        flat[:, t0:t0 + 256] = np.roll(flat[:, t0:t0 + 256], 1, axis=1)
        res["ref"] = flat.reshape(C, H, Wd)
    if mutate and mutate[0] == "rtz" and kind == "f16":
        v = res["ref"]
        r = v.astype(np.float16)
        tz = np.nextafter(r, np.float16(0))
        res["ref"] = np.where(np.abs(r.astype(np.float64)) > np.abs(v), tz, r).astype(np.float64)
    return res


# ------------------------------------------------------------------ the checker
#
# Statistical limits per output kind, measured on simulated legal kernels (tests/test_f16_layer_ref.py:
# test_checker_accepts_legal_kernels prints the worst partition of each layer) and on the GPU (profiles/r05_f16_layer_parity.txt):
#   f16:   e in {-1, 0, +1}; a legal kernel flips where its fp32 sum crosses a rounding midpoint, i.e. with probability about
#          2 |fp32 error| / ulp16 = 2 * 2^-24 sqrt(n) / 2^-11 ~ 1e-2 at n = 11520 (layer 29) and less below: rms = sqrt(flips) <= 0.1-0.15,
#          |mean| ~ rms / sqrt(N) (N >= 5000 per partition) ~ 0.002, |e| > 1 essentially never (only where |v| << S 2^-13).
#          Limits: fraction(|e| > 1) <= 1e-3, |mean| <= 0.05, rms <= 0.5.  Round-toward-zero output: e = -1 on half the elements,
#          rms 0.71; a dropped tap / channel / bias block moves values by many ulps: fraction >> 1e-3.
#   split, f32: e in units of u = 2^-22 sqrt(n sum (a w)^2) + ...: sequential fp32 summation noise has rms <= u / 10 (module doc), so
#          |e| > 1 is a > 10 sigma event.  Limits: fraction(|e| > 1) <= 1e-3, |mean| <= 0.05, rms <= 0.5.  A dropped lo term moves
#          the sum by ~2^-12 sqrt(sum (a w)^2) = 2^10 / sqrt(n) u >= 5 u at every layer (n <= 34560).
STAT_LIMITS = {k: dict(frac=1e-3, mean=0.05, rms=0.5) for k in ("f16", "split", "f32")}


def partitions(C, H, W, tail=None):
    """Boolean masks [C][H][W] of the partitions every statistic is computed on separately.  tail: flat pixel indices (y * W + x) of
    the last partial 256-pixel tile of a ragged batch inside this frame."""
    m = {}
    z = np.zeros((C, H, W), dtype=bool)
    for name, sl in (("top", (slice(None), 0, slice(None))), ("bottom", (slice(None), H - 1, slice(None))),
                     ("left", (slice(None), slice(None), 0)), ("right", (slice(None), slice(None), W - 1)),
                     ("interior", (slice(None), slice(1, H - 1), slice(1, W - 1)))):
        a = z.copy()
        a[sl] = True
        m[name] = a
    for b in range((C + 31) // 32):
        a = z.copy()
        a[32 * b:32 * b + 32] = True
        m[f"ch{32 * b}"] = a
    if tail is not None and len(tail):
        a = z.copy().reshape(C, -1)
        a[:, tail] = True
        m["tail"] = a.reshape(C, H, W)
    return m


def errors_in_units(gpu, res):
    ref = res["ref"]
    if res["kind"] == "f16":
        r = fl16(ref)
        u = ulp16(r) if res.get("floor") is None else np.maximum(ulp16(r), res["floor"])
        return (gpu - r) / u
    return (gpu - ref) / res["unit"]


def check_step(gpu, res, tail=None, limits=None, hard_only=False):
    """Judges one launch.  gpu: decoded output [C][H][W] (float64); res: step_ref's result.  Returns (failures, report): failures is
    a list of strings (empty = accepted), report the figures printed per step."""
    ref = res["ref"]
    assert gpu.shape == ref.shape, (gpu.shape, ref.shape)
    fails = []
    if res["kind"] == "exact":
        n_bad = int((gpu != ref).sum())
        if n_bad:
            fails.append(f"bit-exact step differs at {n_bad} elements (max |d| {np.abs(gpu - ref).max():.3g})")
        return fails, dict(kind="exact", mismatches=n_bad)
    d = np.abs(gpu - ref)
    ratio = d / res["bound"]
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        fails.append(f"hard bound exceeded: {int((ratio > 1).sum())} elements, worst {worst:.3g} x at (c, y, x) {tuple(int(v) for v in i)}"
                     f" gpu {gpu[i]!r} ref {ref[i]!r} bound {res['bound'][i]:.3g}")
    e = errors_in_units(gpu, res)
    rep = dict(kind=res["kind"], max_units=float(np.abs(e).max()), worst_bound_ratio=worst, parts={})
    if hard_only:
        return fails, rep
    lim = limits or STAT_LIMITS[res["kind"]]
    for name, m in partitions(*ref.shape, tail=tail).items():
        x = e[m]
        st = dict(frac=float((np.abs(x) > 1.0).mean()), mean=float(x.mean()), rms=float(np.sqrt((x * x).mean())), n=int(x.size))
        rep["parts"][name] = st
        if st["frac"] > lim["frac"] or abs(st["mean"]) > lim["mean"] or st["rms"] > lim["rms"]:
            fails.append(f"{name}: frac(|e|>1) {st['frac']:.2e} mean {st['mean']:+.3f} rms {st['rms']:.3f} (limits {lim['frac']:.0e} / "
                         f"{lim['mean']} / {lim['rms']}, {st['n']} elements)")
    return fails, rep


def report_line(tag, kernel, rep):
    """One printed line per step: kernel, max |err| in units, worst ratio to the hard bound, statistics border vs interior."""
    if rep["kind"] == "exact":
        return f"{tag:<26} {kernel:<36} exact      mismatches {rep['mismatches']}"
    p = rep["parts"]
    border = [p[k] for k in ("top", "bottom", "left", "right")]
    bf = max(s["frac"] for s in border)
    bm = max(abs(s["mean"]) for s in border)
    br = max(s["rms"] for s in border)
    it = p["interior"]
    blk = max(s["rms"] for k, s in p.items() if k.startswith("ch"))
    tail = f" tail rms {p['tail']['rms']:.3f}" if "tail" in p else ""
    return (f"{tag:<26} {kernel:<36} {rep['kind']:<5} max|e| {rep['max_units']:6.2f} u  bound ratio {rep['worst_bound_ratio']:.3f}  "
            f"border frac {bf:.1e} |mean| {bm:.3f} rms {br:.3f}  interior frac {it['frac']:.1e} mean {it['mean']:+.3f} rms {it['rms']:.3f}"
            f"  worst 32-ch block rms {blk:.3f}{tail}")
