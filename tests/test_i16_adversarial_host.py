"""The worst-case int16 inputs of tests/i16adv.py, pinned against the oracle on the CPU, so that the GPU tests built on them
(tests/test_gpu_i16_adversarial.py) cannot silently go soft:

  * the chain of one output restated on Python integers equals orclib.conv_i16 on the builders' data (interior, edge, corner; K 1, 3),
  * chain_model through the whole-network oracle: every watched conv sees exactly the designed constants, every target interval of
    the quarter-chain sums is hit with both signs, and the outputs are neither mostly saturated nor few in kind,
  * the driver-tier cases really hold the worst quad: p = -M * 32768 and +M * 32768.
"""
import numpy as np
import pytest

import i16adv
import orclib
from yolo2_amd import net, synth


def _pixels(H, W):
    return [(H // 2, W // 2), (0, W // 2), (H // 2, W - 1), (0, 0), (H - 1, W - 1), (H - 1, 0)]      # interior, edges, corners


@pytest.mark.parametrize("K", [1, 3])
def test_chain_restatement_equals_oracle_on_builder_data(K):
    """quad_weights x extreme_inputs on the layer of the GPU file's part A, over shifts, bias shifts and bias sets."""
    C, N, HW = i16adv.LAYER["C"], i16adv.LAYER["N"], i16adv.LAYER["HW"][K]
    pad = K // 2
    checked = 0
    for s, bs, M in ((14, 3, 16383), (14, 0, 16384), (14, -1, 49152), (5, 0, 31), (9, 3, 65534), (16, 0, 65535), (14, 0, 300)):
        Qw, Qai, Qao, Qb = i16adv.layer_q(s, bs)
        for sign in i16adv.SIGNS:
            w = i16adv.quad_weights(N, C, K, M, sign)
            assert np.array_equal(np.abs(w.astype(np.int64)).reshape(N, C // 4, 4, K, K).sum(axis=2), np.full((N, C // 4, K, K), M))
            wr = synth.reorg_weights(w, C, N, K)
            for kind, bname in zip(i16adv.KINDS, i16adv.BIAS_SETS):
                x = i16adv.extreme_inputs(C, HW, HW, kind, seed=M)
                b = i16adv.bias_set(N, bname)
                want = orclib.conv_i16(x, wr, b, C, N, K, 1, HW, HW, pad, 1, Qw, Qai, Qao, Qb)
                for m in (0, 1, N // 2, N - 1):
                    for oy, ox in _pixels(HW, HW):
                        assert i16adv.chain_at(x, w, b, m, oy, ox, HW, pad, s, bs, True) == want[m, oy, ox], (s, bs, M, sign, kind, bname, m, oy, ox)
                        checked += 1
    assert checked == 7 * 4 * 4 * 4 * 6


def test_extreme_inputs_hold_only_extremes():
    for kind in i16adv.KINDS:
        x = i16adv.extreme_inputs(8, 9, 9, kind, seed=1)
        assert x.shape == (8, 9, 16) and not x[:, :, 9:].any()
        assert set(np.unique(x[:, :, :9])) <= {-32768, 32767}
        assert np.array_equal(x[0:4], np.broadcast_to(x[0], (4, 9, 16))) and np.array_equal(x[4:8], np.broadcast_to(x[4], (4, 9, 16)))
    assert len(np.unique(i16adv.extreme_inputs(8, 9, 9, "quad_random", seed=1)[:, :, :9])) == 2
    c = i16adv.extreme_inputs(4, 4, 4, "checker")
    assert c[0, 0, 0] == -32768 and c[0, 0, 1] == 32767 and c[0, 1, 0] == 32767


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("M", [1, 31, 16383, 49151, 65534, 65536])
def test_driver_tier_cases_attain_the_worst_quad(K, M):
    """Over the cases of part A no quad exceeds M * 32768 in magnitude, and both ends are attained: weights negative on inputs
    -32768 give +M * 32768, weights positive on the same inputs -M * 32768."""
    C, N, HW = i16adv.LAYER["C"], i16adv.LAYER["N"], i16adv.LAYER["HW"][K]
    for sign in i16adv.SIGNS:
        w = i16adv.quad_weights(N, C, K, M, sign)
        for kind in i16adv.KINDS:
            lo, hi = i16adv.worst_quad_products(w, i16adv.extreme_inputs(C, HW, HW, kind, seed=M))
            assert -M * 32768 <= lo and hi <= M * 32768
            if kind == "min" and sign in ("neg", "pos"):
                assert (lo, hi) == ((0, M * 32768) if sign == "neg" else (-M * 32768, 0))
            if kind in ("min", "quad_random", "checker") and sign in ("alt_group", "alt_out"):
                assert (lo, hi) == (-M * 32768, M * 32768), (sign, kind)


# ---------------------------------------------------------------------------- chain_model

@pytest.fixture(scope="module")
def chain():
    model, info = i16adv.chain_model(3)
    orclib.oracle().orc_set_threads(16)
    _, _, _, layers = orclib.forward_i16(model, synth.frames(11, 1)[0], dump=True)
    return model, info, layers


def test_chain_model_watched_inputs_are_the_designed_constants(chain):
    model, info, layers = chain
    assert sorted(info) == [c.watched for c in i16adv.CASES] == [10, 12, 14, 18]
    for o, inf in info.items():
        l = net.CONVS[o]
        assert (l.idx, l.size, l.c, l.n, l.h) == {10: (14, 3, 256, 512, 26), 12: (16, 3, 256, 512, 26), 14: (19, 1, 1024, 512, 13),
                                                  18: (23, 3, 1024, 1024, 13)}[o]
        assert net.LAYERS[l.idx + 1].type == (net.MAXPOOL if o == 12 else net.CONV)
        x = layers[l.idx - 1]
        assert np.array_equal(x[:, :, :l.w], i16adv.designed_input(inf, net.LAYERS[l.idx - 1])[:, :, :l.w])
        assert sorted(np.unique(x[:, :, :l.w])) == sorted(i16adv.INPUT_CONSTS) == [-3276, 5, 16384, 32767]
        for g in range(l.c // 4):
            assert sorted(x[4 * g:4 * g + 4, 0, 0]) == sorted(i16adv.INPUT_CONSTS)      # every quad sees all four
        w = model.w_nat[o].astype(np.int64)
        assert np.array_equal(w, np.broadcast_to(w[:, :, :1, :1], w.shape))                       # the same on every tap
        assert np.array_equal(np.abs(w[:, :, 0, 0]), np.broadcast_to(inf.a[:, None], (l.n, l.c)))   # +-a ...
        sg = np.sign(w[:, :, 0, 0]).reshape(l.n, l.c // 4, 4)
        assert np.array_equal(sg, np.broadcast_to(sg[:, :, :1], sg.shape))                        # ... signed per group
        assert sorted(set(model.bias[o].tolist())) == sorted(i16adv.WATCHED_BIAS)
    # every other layer keeps its synthetic weights (SynthModel's own draw, restated for conv 1)
    l1 = net.CONVS[1]
    fan_in = l1.c * l1.size * l1.size
    draw = synth.scaled_gauss_i16(3 * 1000 + 1 * 2 + 1, l1.n * fan_in, (2.0 / fan_in) ** 0.5 * (1 << int(model.weight_q[1])))
    assert np.array_equal(model.w_nat[1].reshape(-1), draw)
    touched = set(info) | {c.driver for c in i16adv.CASES}
    assert all(len(np.unique(model.w_nat[o])) > 100 for o in range(len(net.CONVS)) if o not in touched)


def test_chain_model_hits_every_target_with_both_signs(chain):
    """Per watched conv and target: a channel designed for it has a quarter chain of one sign whose unclamped sum (as the builder
    states it) satisfies the target, on the positive and on the negative side; and the stated sums are the chain's own."""
    model, info, layers = chain
    for o, inf in info.items():
        l = net.CONVS[o]
        CG, KK = l.c // 4, l.size * l.size
        for ti, (name, pred) in enumerate(i16adv.TARGETS):
            for side in (1, -1):
                hit = False
                for m in np.nonzero(inf.target == ti)[0]:
                    sgn = i16adv.PATTERNS[inf.pattern[m]][1](CG).reshape(i16adv.PARTS, -1)
                    for q in range(i16adv.PARTS):
                        if np.all(sgn[q] == side) and pred(abs(int(inf.sums[m, q])), inf.granule) and np.sign(inf.sums[m, q]) == side:
                            hit = True
                assert hit, (o, name, side)
        # the stated sums against a step-by-step restatement, for one channel per (pattern, target)
        consts = [int(v) for v in inf.consts]
        for m in range(len(i16adv.PATTERNS) * len(i16adv.TARGETS)):
            w = model.w_nat[o][m, :, 0, 0]
            t = [i16adv.shift(sum(int(w[4 * g + k]) * consts[4 * g + k] for k in range(4)), inf.so) for g in range(CG)]
            assert [KK * sum(t[q * CG // 4:(q + 1) * CG // 4]) for q in range(4)] == [int(v) for v in inf.sums[m]], (o, m)
        assert {i16adv.PATTERNS[p][0] for p in inf.pattern} == {n for n, _ in i16adv.PATTERNS}
        runs = {int((np.diff(fn(CG)) != 0).sum()) + 1 for _, fn in i16adv.PATTERNS}
        assert {1, 2, 4, 8, 16, 32, CG} <= runs, runs


def test_chain_model_outputs_cannot_hide_a_failure(chain):
    """At most half of a watched conv's outputs sit at 32767 / -32768 / -3276 and at least 16 distinct values occur; the oracle's
    tensor equals the restated chain at interior, edge and corner pixels of channels of every target."""
    model, info, layers = chain
    for o, inf in info.items():
        l = net.CONVS[o]
        y = layers[l.idx][:, :, :l.w]
        sat = float(np.isin(y, (32767, -32768, -3276)).mean())
        distinct = len(np.unique(y))
        print(f"[i16 adversarial] conv {o} (layer {l.idx}): {100 * sat:.1f} % saturated, {100 * float((y == -3276).mean()):.1f} % at -3276, "
              f"{distinct} distinct values")
        assert sat <= 0.5 and distinct >= 16, (o, sat, distinct)
        x = i16adv.designed_input(inf, net.LAYERS[l.idx - 1])
        sb = int(model.bias_q[o]) - int(model.act_q[o + 1])
        step = len(i16adv.PATTERNS) * len(i16adv.TARGETS) // 8 + 1
        for m in list(range(0, l.n, step))[:12]:
            for oy, ox in _pixels(l.h, l.w)[:4]:
                assert i16adv.chain_at(x, model.w_nat[o], model.bias[o], m, oy, ox, l.w, l.pad, inf.so, sb, True) == layers[l.idx][m, oy, ox], (o, m, oy, ox)
