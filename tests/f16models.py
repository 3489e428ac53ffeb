"""Test-side weight sets for the fp16 and split-fp16 passes (CPU only).

synth.SynthModel's fp32 weights are int16 values times 2^-14: every such value below 0.125 in magnitude is exactly an fp16 number, so
the fp16 pass's weight rounding does nothing on it and the w_lo part of the split pass's packed weights [w_hi | w_hi | w_lo] is all
zero on the nine 3x3 layers from 12 on.  DenseModel scales every output channel of that model by its own factor, which fills the
fp32 mantissa: more than 97 % of its weights have w_lo != 0, and most of those w_lo are fp16 subnormals (|w| < 0.125 puts lo below
2^-14), as on any trained network with folded batch-norm.
"""
import numpy as np

from yolo2_amd import net, synth


def channel_factors(l, spread):
    """Per-output-channel factors of conv layer l: 2^((2 u - 1) spread) with u uniform in [0, 1), normalised to unit mean square."""
    u = (synth.splitmix64(synth._counter(77000 + l.ord, l.n)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    f = np.exp2((2.0 * u - 1.0) * spread)
    return f / np.sqrt(np.mean(f * f))


class DenseModel:
    """SynthModel(seed) with every output channel n of every conv layer scaled by f_n: w = fp32(w_nat 2^-Qw f_n), bias =
    fp32(b 2^-Qb f_n).  spread 0.5: factors in about 0.68..1.39; spread 3.0: about 0.045..3.1 (a 64x range of channel magnitudes
    inside one tensor).  Exposes what fr.Weights, load_weights_fp32 and orclib.forward_f32 read."""

    def __init__(self, seed=1, spread=0.5, base=None):
        base = base or synth.SynthModel(seed=seed)      # (base: an already built SynthModel(seed), to share between spreads)
        self.seed, self.spread = seed, spread
        self.w_nat, self.w_reorg, self.bias = [], [], []
        for l in net.CONVS:
            f = channel_factors(l, spread)
            qw, qb = int(base.weight_q[l.ord]), int(base.bias_q[l.ord])
            w = (base.w_nat[l.ord].astype(np.float64) * 2.0 ** -qw * f[:, None, None, None]).astype(np.float32)
            self.w_nat.append(w)
            self.w_reorg.append(synth.reorg_weights(w.reshape(-1), l.c, l.n, l.size))
            self.bias.append((base.bias[l.ord].astype(np.float64) * 2.0 ** -qb * f).astype(np.float32))

    def weights_f32(self):
        return np.concatenate(self.w_reorg)

    def weights_nat_f32(self):
        return np.concatenate([w.reshape(-1) for w in self.w_nat])

    def bias_f32(self):
        return np.concatenate(self.bias)
