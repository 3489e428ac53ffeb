"""Worst-case inputs for the int16 conv, on plain numbers (numpy only: no GPU, no library).

The int16 path runs every block of output channels in the narrowest arithmetic form the loader can prove exact from the weights
(choose_path / splitk_ok in csrc/yolo2_int16.hip, the PACK recovery argument in csrc/kernels_int16.hpp).  Each proof is a statement
about the worst input: every operand of a 4-channel quad at -32768 or 32767 with the weights' signs aligned, step after step in
the same direction.  Random data never comes near it, so this module builds it:

  quad_weights    weights whose every (output, group, tap) quad has sum |w| == M exactly
  extreme_inputs  activations at the two extremes only
  chain_at        one output's chain restated on Python integers (the oracle is held against it in the host test)
  chain_model     a whole network in which four "watched" convs see per-channel constants and carry weights +-a whose sign
                  depends only on the input-channel group, with `a` chosen per output channel so that the unclamped sum of one
                  quarter of the chain lands on every regime of the split-K triples (a below, at, and beyond 2^15 and 2^16)

tests/test_i16_adversarial_host.py pins all of it against the oracle; tests/test_gpu_i16_adversarial.py runs it on the kernels.
"""
from collections import namedtuple

import numpy as np

from yolo2_amd import net, synth

LO, HI = -32768, 32767
SIGNS = ("pos", "neg", "alt_group", "alt_out")
KINDS = ("min", "max", "quad_random", "checker")


def w8(w):
    return (w + 7) // 8 * 8


def quad_weights(N, C, K, M, sign):
    """Natural [N][C][K][K] int16 weights in which the channels of every group of 4 input channels (a last group of C % 4 channels
    included) have magnitudes that sum to M exactly, split as evenly as integers allow, the same for every tap and output.
    sign: "pos", "neg", "alt_group" (+ on even groups, - on odd) or "alt_out" (+ on even output channels, - on odd)."""
    assert sign in SIGNS, sign
    CG = (C + 3) // 4
    mag = np.zeros(CG * 4, dtype=np.int64)
    for g in range(CG):
        real = min(4, C - 4 * g)
        q, r = divmod(M, real)
        mag[4 * g:4 * g + real] = q
        mag[4 * g:4 * g + r] += 1
    sgn = np.ones((N, CG), dtype=np.int64)
    if sign == "neg":
        sgn[:] = -1
    elif sign == "alt_group":
        sgn[:, 1::2] = -1
    elif sign == "alt_out":
        sgn[1::2, :] = -1
    w = (np.repeat(sgn, 4, axis=1) * mag[None, :])[:, :C]
    assert w.min() >= LO and w.max() <= HI, f"M = {M} does not fit int16 weights"
    return np.ascontiguousarray(np.broadcast_to(w[:, :, None, None], (N, C, K, K)).astype(np.int16))


def extreme_inputs(C, H, W, kind, seed=0):
    """int16 [C][H][w8(W)] holding only -32768 and 32767: "min", "max", "quad_random" (per pixel and group of 4 channels one random
    extreme, shared by the group's channels) or "checker" (per pixel, a checkerboard).  Columns W..w8(W)-1 stay zero."""
    assert kind in KINDS, kind
    x = np.zeros((C, H, w8(W)), dtype=np.int16)
    if kind == "min":
        x[:, :, :W] = LO
    elif kind == "max":
        x[:, :, :W] = HI
    elif kind == "quad_random":
        CG = (C + 3) // 4
        pick = np.random.default_rng(seed).integers(0, 2, (CG, H, W))
        x[:, :, :W] = np.repeat(np.where(pick == 1, HI, LO), 4, axis=0)[:C]
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        x[:, :, :W] = np.where((yy + xx) % 2 == 0, LO, HI)[None]
    return x


# ---------------------------------------------------------------------------- the form-limit cases of the per-layer driver tier

SHIFTS = (5, 9, 14, 16)              # s = Qa_in + Qw - Qa_out
BIAS_SHIFTS = (3, 0, -1)             # Qb - Qa_out
PROBE = dict(C=4, N=32, HW={3: 5, 1: 5})       # the layer the limits are bisected on
LAYER = dict(C=8, N=40, HW={3: 9, 1: 8})       # ... and the one they are run on: two groups, a ragged channel block, borders
BIAS_SETS = ("zero", "max", "min", "one_lo")


def bias_set(N, name):
    """int16 [N]: all 0, all +32767, all -32767, or zeros with a single -32768 (which no packed int16 accumulator can start from)."""
    b = np.zeros(N, dtype=np.int16)
    if name == "max":
        b[:] = 32767
    elif name == "min":
        b[:] = -32767
    elif name == "one_lo":
        b[N // 2] = -32768
    else:
        assert name == "zero", name
    return b


def layer_q(s, bias_shift):
    """(Qw, Qa_in, Qa_out, Qb) of a layer call with output shift s and bias shift `bias_shift`."""
    return s, 9, 9, 9 + bias_shift


# ---------------------------------------------------------------------------- the chain on Python integers

def shift(v, s):
    """The conv's requantisation of an integer by s bits (magnitude capped at 30): round-half-up right shift, or a left shift."""
    mag = min(abs(s), 30)
    if s > 0:
        return (v + (1 << (mag - 1))) >> mag
    return v << mag if s < 0 else v


def sat16(v):
    return max(LO, min(HI, v))


def leaky16(v):
    return -((-v) // 10) if v < 0 else v      # truncating /10


def chain_at(x, w_nat, bias, m, oy, ox, W, pad, so, sb, leaky):
    """Output channel m at pixel (oy, ox) of a stride-1 conv, on Python integers: the accumulator starts from the shifted bias, then
    one saturating step per (group of 4 input channels, tap) - groups outer, taps inner; a tap outside the image contributes p = 0."""
    _, C, K, _ = w_nat.shape
    H = x.shape[1]
    acc = shift(int(bias[m]), sb)
    for g in range((C + 3) // 4):
        for i in range(K):
            for j in range(K):
                yy, xx = oy + i - pad, ox + j - pad
                p = 0
                if 0 <= yy < H and 0 <= xx < W:
                    for c in range(4 * g, min(4 * g + 4, C)):
                        p += int(w_nat[m, c, i, j]) * int(x[c, yy, xx])
                acc = sat16(acc + shift(p, so))
    return leaky16(acc) if leaky else acc


def worst_quad_products(w_nat, x):
    """(min, max) over every (output, group, tap, pixel) of the quad's dot product p, taps outside the image left out (numpy int64)."""
    N, C, K, _ = w_nat.shape
    pad = K // 2
    H, W8 = x.shape[1:]
    Cp = (C + 3) // 4 * 4
    w = np.zeros((N, Cp, K, K), dtype=np.int64)
    w[:, :C] = w_nat
    xs = np.zeros((Cp, H, W8), dtype=np.int64)
    xs[:C] = x
    lo, hi = 0, 0
    for i in range(K):
        for j in range(K):
            y0, y1 = max(0, pad - i), min(H, H + pad - i)        # output rows whose tap (i, j) is inside the image
            x0, x1 = max(0, pad - j), W8 - max(0, j - pad)
            src = xs[:, y0 + i - pad:y1 + i - pad, x0 + j - pad:x1 + j - pad]
            p = np.einsum("ngc,gcyx->ngyx", w[:, :, i, j].reshape(N, Cp // 4, 4), src.reshape(Cp // 4, 4, *src.shape[1:]))
            lo, hi = min(lo, int(p.min())), max(hi, int(p.max()))
    return lo, hi


# ---------------------------------------------------------------------------- designed chains in a whole network

# driver -> watched, by conv ordinal.  M: every quad of the watched conv gets sum |w| == M (split evenly) in place of the target
# ladder; driver_bias: the driver's per-channel bias cycle (its output, hence the watched conv's input, is leaky(bias)).
Case = namedtuple("Case", "driver watched M driver_bias", defaults=(None, None))
CASES = (Case(9, 10), Case(11, 12), Case(13, 14), Case(17, 18))
DRIVER_BIAS = (32767, 16384, -32768, 5)
INPUT_CONSTS = tuple(leaky16(b) for b in DRIVER_BIAS)      # (32767, 16384, -3276, 5)
WATCHED_BIAS = (0, 30000, -30000)
PARTS = 4       # the quarter chains of the lane-split kernel's S = 4 (its S = 8 on 1x1 layers halves them again)


def _period(tpl):
    return lambda CG: np.array(tpl, dtype=np.int64)[np.arange(CG) % len(tpl)]


def _runs(R, first=1):
    return lambda CG: first * (1 - 2 * ((np.arange(CG) // (CG // R)) % 2)).astype(np.int64)


# the sign of an input-channel group's weights: constant, period 2 and 4, and 2 .. 32 equal runs over the chain
PATTERNS = (("all+", _period((1,))), ("all-", _period((-1,))), ("alt", _period((1, -1))), ("++--", _period((1, 1, -1, -1))),
            ("--++", _period((-1, -1, 1, 1))), ("+--+", _period((1, -1, -1, 1))), ("halves+-", _runs(2)), ("halves-+", _runs(2, -1)),
            ("runs4", _runs(4)), ("runs8", _runs(8)), ("runs16", _runs(16)), ("runs32", _runs(32)))
# what |unclamped sum of a quarter chain| is aimed at, as (name, predicate on (v, G)); G: the most one unit of `a` moves that sum
TARGETS = (
    ("about 6000", lambda v, G: 4000 <= v <= 8000),
    ("just under 32768", lambda v, G: 32768 - G <= v < 32768),
    ("32768 or the nearest above", lambda v, G: 32768 <= v < 32768 + G),
    ("inside (32768, 65535)", lambda v, G: 32768 + G <= v <= 65535 - G),
    ("65535 or the nearest below", lambda v, G: 65535 - G < v <= 65535),
    ("65536 or the nearest above", lambda v, G: 65536 <= v < 65536 + G),
    ("inside (65536, 131072)", lambda v, G: 65536 + G <= v < 131072),
    ("above 131072", lambda v, G: v > 131072),
)
ChainInfo = namedtuple("ChainInfo", "layer consts so sums target pattern a granule")


def _pick_magnitudes(steps, csum, so, side):
    """For weights side * a on every channel of a quarter chain of `steps` steps whose quads see inputs summing to csum: the `a` per
    TARGETS entry, and G.  |sum| = steps * |shift(side * a * csum, so)| does not decrease with a."""
    a = np.arange(1, 8192, dtype=np.int64)
    rnd = (1 << (so - 1)) if so > 0 else 0
    v = np.abs(steps * ((side * a * csum + rnd) >> so))
    assert np.all(np.diff(v) >= 0)
    G = int(np.diff(v).max())
    first_ge = lambda t: int(np.searchsorted(v, t, side="left"))      # index of the smallest a with v >= t
    nearest = lambda t: int(np.abs(v - t).argmin())
    idx = (nearest(6000), first_ge(32768) - 1, first_ge(32768), nearest(49152), first_ge(65536) - 1, first_ge(65536), nearest(98304),
           first_ge(131073))
    return [int(a[i]) for i in idx], G


def chain_model(seed, cases=CASES, weight_q=None, bias_q=None, act_q=None):
    """A SynthModel whose `driver` convs have zero weights, bias_q == act_q of their output and a per-channel bias cycle, so that the
    `watched` conv behind each sees an input that is constant per channel (zero padding at the border), and whose watched convs have
    weights +-a with the sign a function of the input-channel group (PATTERNS), `a` per output channel from the TARGETS ladder (or
    the case's M), biases cycling through WATCHED_BIAS.  All other layers keep their synthetic weights.
    Returns (model, {watched ordinal: ChainInfo}); ChainInfo.sums [N][PARTS] are the unclamped quarter-chain sums at an interior pixel."""
    nconv = len(net.CONVS)
    wq = list(weight_q) if weight_q is not None else [synth.STD_Q["weight_q"]] * nconv
    bq = list(bias_q) if bias_q is not None else [synth.STD_Q["bias_q"]] * nconv
    aq = list(act_q) if act_q is not None else [synth.STD_Q["act_q_in"]] + [synth.STD_Q["act_q"]] * nconv
    assert not {c.driver for c in cases} & {c.watched for c in cases}, "a driver must not itself be watched"
    for c in cases:
        assert c.watched == c.driver + 1 and net.CONVS[c.watched].idx == net.CONVS[c.driver].idx + 1
        bq[c.driver] = aq[c.driver + 1]      # out = bias
    model = synth.SynthModel(seed=seed, weight_q=wq, bias_q=bq, act_q=aq)
    info = {}
    for c in cases:
        d, l = net.CONVS[c.driver], net.CONVS[c.watched]
        cyc = np.array(c.driver_bias or DRIVER_BIAS, dtype=np.int16)
        _set_conv(model, c.driver, np.zeros((d.n, d.c, d.size, d.size), np.int16), cyc[np.arange(d.n) % len(cyc)])
        consts = np.array([leaky16(int(b)) for b in model.bias[c.driver]], dtype=np.int64)
        N, C, KK, CG = l.n, l.c, l.size * l.size, l.c // 4
        assert C % 4 == 0 and CG % 32 == 0 and C == d.n
        so = aq[c.watched] + wq[c.watched] - aq[c.watched + 1]
        steps = CG // PARTS * KK
        m = np.arange(N)
        if c.M is None:
            assert len(cyc) == 4, "the target ladder assumes every quad sees the same four constants"
            csum = int(consts[:4].sum())
            mags = {side: _pick_magnitudes(steps, csum, so, side) for side in (1, -1)}
            G = max(mags[1][1], mags[-1][1])
            combo = m % (len(PATTERNS) * len(TARGETS))
            pattern, target = combo % len(PATTERNS), combo // len(PATTERNS)
            bias_i = (m + m // (len(PATTERNS) * len(TARGETS))) % len(WATCHED_BIAS)
            sgn = np.stack([PATTERNS[p][1](CG) for p in pattern])                                     # [N][CG]
            a = np.array([mags[int(sgn[k, 0])][0][t] for k, t in enumerate(target)], dtype=np.int64)
            w2 = np.repeat(sgn * a[:, None], 4, axis=1)                                               # [N][C]
        else:
            pattern, target, bias_i, G = m % len(PATTERNS), np.full(N, -1), m % len(WATCHED_BIAS), 0
            sgn = np.stack([PATTERNS[p][1](CG) for p in pattern])
            w2 = np.repeat(sgn, 4, axis=1) * quad_weights(1, C, 1, c.M, "pos").reshape(1, C).astype(np.int64)
            a = np.full(N, c.M, dtype=np.int64)
        assert np.abs(w2).max() <= HI
        w_nat = np.ascontiguousarray(np.broadcast_to(w2[:, :, None, None], (N, C, l.size, l.size)).astype(np.int16))
        _set_conv(model, c.watched, w_nat, np.array(WATCHED_BIAS, dtype=np.int16)[bias_i])
        rnd = (1 << (so - 1)) if so > 0 else 0
        p = (w2 * consts[None, :]).reshape(N, CG, 4).sum(axis=2)
        t = (p + rnd) >> so
        sums = KK * t.reshape(N, PARTS, CG // PARTS).sum(axis=2)
        info[c.watched] = ChainInfo(l.idx, consts.astype(np.int16), so, sums, target, pattern, a, G)
    return model, info


def _set_conv(model, o, w_nat, bias):
    l = net.CONVS[o]
    model.w_nat[o] = w_nat
    model.w_reorg[o] = synth.reorg_weights(w_nat.reshape(-1), l.c, l.n, l.size)
    model.bias[o] = np.ascontiguousarray(bias, dtype=np.int16)


def designed_input(info, l):
    """The tensor a watched conv must see: ChainInfo.consts per channel over the image, columns out_w.. zero (layer l = its driver)."""
    x = np.zeros((l.out_c, l.out_h, w8(l.out_w)), dtype=np.int16)
    x[:, :, :l.out_w] = info.consts[:, None, None]
    return x
