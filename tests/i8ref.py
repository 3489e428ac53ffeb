"""The int8 pass's arithmetic (include/yolo2_hip.h "int8 pass") restated in numpy / torch on float64.

Every value stays an integer below 2^53, so float64 products and sums are exact: this file is the definition the GPU is held to
bit for bit.  It shares no code with the library.  Tensors are dense [B][C][H][W]; weights natural [N][C][K][K].
"""
import numpy as np
import torch
import torch.nn.functional as F

from yolo2_amd import net

Q_MIN, Q_MAX = -8, 24


def rha(v):
    """round half away from zero"""
    v = np.asarray(v, dtype=np.float64)
    return np.trunc(v + np.copysign(0.5, v))


def q8(m, h=1.0, what="tensor"):
    """the largest q in -8..24 with h * m * 2^q < 127.5 (double); 24 for m = 0"""
    m = float(m)
    if not (m >= 0.0) or not np.isfinite(m):
        raise ValueError(f"{what}: max {m} is not a finite non-negative number")
    if m == 0.0:
        return Q_MAX
    for q in range(Q_MAX, Q_MIN - 1, -1):
        if float(h) * m * 2.0 ** q < 127.5:
            return q
    raise ValueError(f"{what}: no Q in {Q_MIN}..{Q_MAX} holds max {m}")


def act_q_from_stats(act_absmax, headroom=1.0):
    a = [q8(act_absmax[0], 1.0, "input")] + [q8(act_absmax[o + 1], headroom, f"output of conv {o}") for o in range(len(net.CONVS))]
    a[20] = a[21] = min(a[20], a[21])
    return np.array(a, dtype=np.int32)


def qin(ord_, act_q):
    return int(act_q[13] if ord_ == 20 else (act_q[20] if ord_ == 21 else act_q[ord_]))


def quantize_layer(w_f32, b_f32, q_in):
    """fp32 [N][C][K][K], [N] -> (w8 int8, bias32 int32, Qw int32 [N])"""
    w = np.asarray(w_f32, dtype=np.float32)
    N = w.shape[0]
    mx = np.abs(w.reshape(N, -1)).max(axis=1)
    qw = np.array([q8(m, 1.0, f"channel {i}") for i, m in enumerate(mx)], dtype=np.int32)
    w8 = np.clip(rha(w.astype(np.float64) * (2.0 ** qw.astype(np.float64)).reshape(N, 1, 1, 1)), -127, 127).astype(np.int8)
    b32 = rha(np.asarray(b_f32, dtype=np.float32).astype(np.float64) * 2.0 ** (q_in + qw.astype(np.float64))).astype(np.int64)
    assert np.abs(b32).max() < 2 ** 31
    return w8, b32.astype(np.int32), qw


class ModelI8:
    """per conv ordinal: w8 [N][C][K][K], bias32 [N], qw [N]; act_q [24]"""

    def __init__(self, w_nat_f32, bias_f32, act_q):
        self.act_q = np.array(act_q, dtype=np.int32)
        self.w8, self.bias32, self.qw = [], [], []
        for l, w, b in zip(net.CONVS, w_nat_f32, bias_f32):
            a, c, d = quantize_layer(np.asarray(w).reshape(l.n, l.c, l.size, l.size), b, qin(l.ord, self.act_q))
            self.w8.append(a); self.bias32.append(c); self.qw.append(d)

    def flat(self):
        return (np.concatenate([w.reshape(-1) for w in self.w8]), np.concatenate(self.bias32), np.concatenate(self.qw))


def quantize_input(frames, q):
    return np.clip(rha(np.asarray(frames, dtype=np.float32).astype(np.float64) * 2.0 ** int(q)), -128, 127)


def _acc(x, w8, bias32):
    K = w8.shape[2]
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)), torch.from_numpy(w8.astype(np.float64)),
                 torch.from_numpy(np.asarray(bias32).astype(np.float64)), padding=K // 2)
    return y.numpy()


def _finish(acc, qw, q_in, q_out, leaky, out_float):
    """acc: float64 integers [B][N][H][W] -> int8 values (float64) or the float32 region rule"""
    if leaky:
        acc = np.where(acc < 0, np.trunc(acc / 10.0), acc)      # |acc| < 2^31: the float64 quotient truncates to the integer quotient
    qw = np.asarray(qw, dtype=np.int64).reshape(1, -1, 1, 1)
    if out_float:
        return acc.astype(np.float32) * (2.0 ** -(q_in + qw).astype(np.float64)).astype(np.float32)
    s = q_in + qw - q_out
    assert s.min() >= -7 and s.max() <= 31
    a = acc.astype(np.int64)
    sp = np.maximum(s, 1)
    y = np.where(s > 0, (a + (1 << (sp - 1))) >> sp, a << np.maximum(-s, 0))
    return np.clip(y, -128, 127).astype(np.float64)


def conv(x, w8, bias32, qw, q_in, q_out, leaky, out_float=False):
    """x: integer-valued [B][C][H][W] -> int8 [B][N][H][W] (or float32 with out_float)"""
    acc = _acc(x, w8, bias32)
    assert np.abs(acc).max() < 2 ** 31
    y = _finish(acc, qw, q_in, q_out, leaky, out_float)
    return y if out_float else y.astype(np.int8)


def conv_loop(x, w8, bias32, qw, q_in, q_out, leaky, out_float=False):
    """the same as plain Python integer loops (tiny shapes only): the check of conv()"""
    x = np.asarray(x).astype(np.int64)
    B, C, H, W = x.shape
    N, _, K, _ = w8.shape
    p = K // 2
    out = np.zeros((B, N, H, W), dtype=np.float32 if out_float else np.int8)
    for b in range(B):
        for m in range(N):
            for yy in range(H):
                for xx in range(W):
                    acc = int(bias32[m])
                    for c in range(C):
                        for i in range(K):
                            for j in range(K):
                                sy, sx = yy + i - p, xx + j - p
                                if 0 <= sy < H and 0 <= sx < W:
                                    acc += int(w8[m, c, i, j]) * int(x[b, c, sy, sx])
                    if leaky and acc < 0:
                        acc = -((-acc) // 10)
                    if out_float:
                        out[b, m, yy, xx] = np.float32(acc) * np.float32(2.0 ** -(q_in + int(qw[m])))
                        continue
                    s = q_in + int(qw[m]) - q_out
                    v = (acc + (1 << (s - 1))) >> s if s > 0 else acc << -s
                    out[b, m, yy, xx] = max(-128, min(127, v))
    return out


def pool(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def reorg(x):
    """the legacy Darknet reorg of [B][64][26][26] -> [B][256][13][13] (flat index permutation)"""
    o = np.arange(256 * 169)
    k, rem = o // (26 * 416), o % (26 * 416)
    j, i = rem // 26, rem % 26
    sidx = (2 * i + (k & 1)) + 52 * (2 * j + (k >> 1))
    B = x.shape[0]
    return x.reshape(B, -1)[:, sidx].reshape(B, 256, 13, 13)


def forward(frames, m: ModelI8, keep=False):
    """float frames [B][3][416][416] -> float32 region [B][425][13][13] (and, with keep, every layer's int8 tensor by layer index;
    -1 is the quantised input)"""
    x = quantize_input(frames, m.act_q[0])
    outs = {-1: x.astype(np.int8)} if keep else {}
    saved = {}
    for l in net.LAYERS:
        if l.type == net.CONV:
            o = l.ord
            x = conv(x, m.w8[o], m.bias32[o], m.qw[o], qin(o, m.act_q), int(m.act_q[o + 1]), l.leaky, out_float=(l.idx == 30))
            if l.idx != 30:
                x = x.astype(np.float64)
        elif l.type == net.MAXPOOL:
            x = pool(x)
        elif l.type == net.REORG:
            x = reorg(x)
        elif l.type == net.ROUTE:
            x = saved[16] if l.idx == 25 else np.concatenate([saved[27], saved[24]], axis=1)
        elif l.type == net.REGION:
            break
        saved[l.idx] = x
        if keep and l.idx != 30:
            outs[l.idx] = x.astype(np.int8)
    return (x, outs) if keep else x


def float_forward(frames, w_nat_f32, bias_f32):
    """the float pass in float64 on the same weights -> (region float64 [B][425][13][13], act_absmax [24])"""
    x = torch.from_numpy(np.asarray(frames, dtype=np.float32).astype(np.float64))
    mx = [float(x.abs().max())]
    saved = {}
    for l in net.LAYERS:
        if l.type == net.CONV:
            w = torch.from_numpy(np.asarray(w_nat_f32[l.ord], dtype=np.float32).astype(np.float64).reshape(l.n, l.c, l.size, l.size))
            b = torch.from_numpy(np.asarray(bias_f32[l.ord], dtype=np.float32).astype(np.float64))
            x = F.conv2d(x, w, b, padding=l.size // 2)
            if l.leaky:
                x = torch.where(x < 0, 0.1 * x, x)
            mx.append(float(x.abs().max()))
        elif l.type == net.MAXPOOL:
            x = F.max_pool2d(x, 2)
        elif l.type == net.REORG:
            x = torch.from_numpy(reorg(x.numpy()))
        elif l.type == net.ROUTE:
            x = saved[16] if l.idx == 25 else torch.cat([saved[27], saved[24]], dim=1)
        elif l.type == net.REGION:
            break
        saved[l.idx] = x
    return x.numpy(), np.array(mx, dtype=np.float64)


def boxes(region):
    """region [B][425][13][13] -> boxes [B][845][4] (x, y, w, h relative to the image), all 5 x 169 slots"""
    r = np.asarray(region, dtype=np.float64).reshape(-1, 5, 85, 13, 13)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    col, row = np.arange(13).reshape(1, 1, 1, 13), np.arange(13).reshape(1, 1, 13, 1)
    an = np.array(net.ANCHORS).reshape(5, 2)
    bx = (col + sig(r[:, :, 0])) / 13.0
    by = (row + sig(r[:, :, 1])) / 13.0
    bw = np.exp(r[:, :, 2]) * an[:, 0].reshape(1, 5, 1, 1) / 13.0
    bh = np.exp(r[:, :, 3]) * an[:, 1].reshape(1, 5, 1, 1) / 13.0
    return np.stack([bx, by, bw, bh], axis=-1).reshape(r.shape[0], 845, 4)


def mean_iou(region_a, region_b):
    a, b = boxes(region_a), boxes(region_b)
    def lohi(v):
        return v[..., 0] - v[..., 2] / 2, v[..., 0] + v[..., 2] / 2, v[..., 1] - v[..., 3] / 2, v[..., 1] + v[..., 3] / 2
    al, ar, at, ab = lohi(a)
    bl, br, bt, bb = lohi(b)
    iw = np.clip(np.minimum(ar, br) - np.maximum(al, bl), 0, None)
    ih = np.clip(np.minimum(ab, bb) - np.maximum(at, bt), 0, None)
    inter = iw * ih
    union = a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter
    return float((inter / union).mean())


def model_f32(model):
    """(natural fp32 weights per conv, fp32 biases per conv) of a synth.SynthModel: its exact fp32 twin"""
    w = [wn.astype(np.float32) * np.float32(2.0 ** -int(model.weight_q[i])) for i, wn in enumerate(model.w_nat)]
    b = [bb.astype(np.float32) * np.float32(2.0 ** -int(model.bias_q[i])) for i, bb in enumerate(model.bias)]
    return w, b
