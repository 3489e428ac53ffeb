"""CPU tests of the full-mantissa weight set (tests/f16models.py) and of the ("no_wlo",) mutation of tests/f16ref.py.

synth.SynthModel's weights are int16 values times 2^-14, so the w_lo part of the split pass's packed weights is all zero on the nine
3x3 layers from 12 on and nothing that reads, packs or multiplies it is checked by a test that loads those weights.  These tests pin
what DenseModel puts there instead (census, determinism, value range), show on one launch why the grid model cannot see a dropped
a_hi * w_lo term while the dense one can, and repeat the checker's soundness and teeth tests on dense weights."""
import os

import numpy as np
import pytest

import f16models as fm
import f16ref as fr
import orclib
import test_f16_layer_ref as lr
from yolo2_amd import net, synth

SPREADS = {0.5: dict(lo_nonzero=0.95, vmax=8.0), 3.0: dict(lo_nonzero=0.85, vmax=32.0)}


@pytest.fixture(scope="module")
def grid():
    return synth.SynthModel(seed=1)


@pytest.fixture(scope="module")
def dense(grid):
    return {s: fm.DenseModel(1, s, base=grid) for s in SPREADS}


@pytest.fixture(scope="module")
def dense_weights(dense):
    return fr.Weights(dense[0.5])


@pytest.fixture(scope="module")
def dense_exact(dense_weights):
    return lr.forward_exact(synth.frames(40, 1)[0].astype(np.float64), dense_weights)


# ------------------------------------------------------------------ the model

@pytest.fixture(scope="module")
def grid_weights(grid):
    return fr.Weights(grid)


def split_pair_f32(w):
    """fr.split_pair of fp32 values in their own formats (the difference is exact in fp32): as float16 arrays, a tenth of the time."""
    hi = w.astype(np.float16)
    return hi, (w - hi.astype(np.float32)).astype(np.float16)


@pytest.mark.parametrize("spread", list(SPREADS))
def test_census_w_lo_is_populated_and_mostly_subnormal(spread, dense):
    """In every conv layer: >= 95 % (spread 3.0: >= 85 %) of the non-zero weights have w_lo != 0, >= 99.9 % are not fp16 numbers, and at
    least half of the non-zero w_lo are fp16 subnormals.  Measured minima: 96.9 % / 89.8 % (layer 29), 99.969 %, 79 % (layer 0; 100 %
    on every 3x3 layer from 12 on)."""
    for l in net.CONVS:
        w = dense[spread].w_nat[l.ord].reshape(-1)
        hi, lo = split_pair_f32(w)
        if l.ord < 3:   # the same pair as the checker's
            h64, l64 = fr.split_pair(w)
            assert np.array_equal(hi.astype(np.float64), h64) and np.array_equal(lo.astype(np.float64), l64)
        n, nz = np.count_nonzero(w), lo != 0                  # (a zero weight has hi = lo = 0: it counts in neither numerator)
        share, not_f16 = np.count_nonzero(nz) / n, np.count_nonzero(hi.astype(np.float32) != w) / n
        sub = np.count_nonzero(nz & ((lo.view(np.uint16) & 0x7C00) == 0)) / np.count_nonzero(nz)      # exponent field 0 = subnormal
        print(f"spread {spread} L{l.idx}: w_lo != 0 {share:.4f}  not fp16 {not_f16:.5f}  subnormal w_lo {sub:.4f}  max |w| {np.abs(w).max():.3f}")
        assert share >= SPREADS[spread]["lo_nonzero"], (l.idx, share)
        assert not_f16 >= 0.999, (l.idx, not_f16)
        assert sub >= 0.5, (l.idx, sub)


def test_grid_model_has_no_w_lo_on_the_deep_3x3_layers(grid_weights):
    """What the dense model is for: on SynthModel(1) not one weight of the 3x3 layers from 12 on has a lo part."""
    for L in (12, 14, 16, 18, 20, 22, 23, 24, 29):
        assert not split_pair_f32(grid_weights.w[L].astype(np.float32))[1].any(), L


def test_two_constructions_give_the_same_bytes(dense, grid):
    a, b = dense[0.5], fm.DenseModel(1, 0.5)     # (b from scratch: its own SynthModel)
    for name in ("weights_f32", "weights_nat_f32", "bias_f32"):
        x, y = getattr(a, name)(), getattr(b, name)()
        assert x.dtype == np.float32 and x.tobytes() == y.tobytes(), name
    assert dense[3.0].weights_f32().tobytes() != a.weights_f32().tobytes()
    base = grid
    assert dense[0.5].weights_f32().shape == base.weights_f32().shape and dense[0.5].bias_f32().shape == base.bias_f32().shape
    # the reorg stream is the natural tensor in the accelerator's tile order, layer by layer
    l = net.CONVS[3]
    assert np.array_equal(dense[0.5].w_reorg[3], synth.reorg_weights(dense[0.5].w_nat[3].reshape(-1), l.c, l.n, l.size))


@pytest.mark.parametrize("spread", list(SPREADS))
def test_region_tensor_range(spread, dense):
    """The fp32 oracle's region tensor of synth.frames(40, 1)[0] is finite, max |v| < 8 (spread 0.5, measured 5.58) / < 32 (spread
    3.0, measured 15.4): the model stays far from fp16 overflow, so the GPU tests never judge an overflow artefact."""
    orclib.oracle().orc_set_threads(min(16, os.cpu_count() or 1))
    r = orclib.forward_f32(dense[spread], synth.frames(40, 1)[0])
    print(f"spread {spread}: max |region| = {np.abs(r).max():.3f}")
    assert np.isfinite(r).all()
    assert np.abs(r).max() < SPREADS[spread]["vmax"], np.abs(r).max()


# ------------------------------------------------------------------ why the grid cannot see it

def _layer22_input():
    """An input of layer 22's shape with full (hi, lo) pairs: seeded, leaky'd normal values."""
    v = np.random.default_rng(22).standard_normal((512, 13, 13))
    v = np.where(v < 0, fr.LEAKY * v, v)
    hi, lo = fr.split_pair(v)
    return dict(v=hi + lo, hi=hi, lo=lo)


def test_no_wlo_is_invisible_on_the_grid_model_and_visible_on_the_dense_one(grid_weights, dense_weights):
    kernel = "k_conv_f16_halo<256,2,16,32,split>"
    x = _layer22_input()
    assert x["lo"].any()
    grid = grid_weights
    a = fr.step_ref("split", kernel, [22], x, grid)
    b = fr.step_ref("split", kernel, [22], x, grid, mutate=("no_wlo",))
    assert np.array_equal(a["ref"], b["ref"])
    a = fr.step_ref("split", kernel, [22], x, dense_weights)
    b = fr.step_ref("split", kernel, [22], x, dense_weights, mutate=("no_wlo",))
    d = np.abs(a["ref"] - b["ref"]) / a["unit"]
    print(f"dense L22: dropping a_hi w_lo moves the reference by up to {d.max():.1f} u, rms {np.sqrt((d * d).mean()):.1f} u")
    assert not np.array_equal(a["ref"], b["ref"])
    assert np.sqrt((d * d).mean()) > fr.STAT_LIMITS["split"]["rms"]
    # the other mutation of the split products drops a_lo w_hi as well: it is visible on both models
    c = fr.step_ref("split", kernel, [22], x, grid, mutate=("no_lo",))
    assert not np.array_equal(a["ref"], c["ref"])


# ------------------------------------------------------------------ soundness and teeth on dense weights

DENSE_STEPS = [s for s in lr.SIM_STEPS if (s[0] == "split" and s[2] in ([8], [9], [20], [29], [30])) or (s[0] == "fp16" and s[2] in ([20], [29]))]
DENSE_SPLIT = [s for s in DENSE_STEPS if s[0] == "split"]
assert len(DENSE_STEPS) == 7 and len(DENSE_SPLIT) == 5


@pytest.mark.slow
@pytest.mark.parametrize("path,kernel,layers", DENSE_STEPS, ids=[f"{p}-L{ls[0]}" for p, _, ls in DENSE_STEPS])
def test_checker_accepts_legal_kernels_on_dense_weights(path, kernel, layers, dense_exact, dense_weights):
    """Soundness with subnormal w_lo: the simulated legal kernel passes the hard bound and STAT_LIMITS for two chunk orders."""
    x = lr.step_input(path, layers[0], dense_exact)
    res = fr.step_ref(path, kernel, layers, x, dense_weights)
    for seed in (1, 2):
        gpu = lr.simulate(path, layers, x, dense_weights, seed)
        fails, rep = fr.check_step(gpu, res)
        print(fr.report_line(f"dense sim {path} L{layers[0]} s{seed}", kernel, rep))
        assert not fails, fails


@pytest.mark.slow
@pytest.mark.parametrize("path,kernel,layers", DENSE_SPLIT, ids=[f"{p}-L{ls[0]}" for p, _, ls in DENSE_SPLIT])
def test_checker_rejects_dropped_w_lo_on_dense_weights(path, kernel, layers, dense_exact, dense_weights):
    """Teeth: the legal kernel's output against a reference without a_hi * w_lo is rejected at every split launch."""
    x = lr.step_input(path, layers[0], dense_exact)
    gpu = lr.simulate(path, layers, x, dense_weights, 1)
    res = fr.step_ref(path, kernel, layers, x, dense_weights, mutate=("no_wlo",))
    fails, rep = fr.check_step(gpu, res)
    print(fr.report_line(f"no_wlo dense {path} L{layers[0]}", kernel, rep), "->", fails[:1])
    assert fails, "a dropped a_hi * w_lo term was accepted"
