"""CPU tests of the per-launch fp16 / split-fp16 reference and checker (tests/f16ref.py): item layout, wiring of the step references
against the fp32 oracle, soundness on simulated legal kernels, and teeth (each deliberate kernel error is rejected)."""
import os
import re

import numpy as np
import pytest

import f16ref as fr
import orclib
from yolo2_amd import net, synth

ROOT = orclib.ROOT


@pytest.fixture(scope="module")
def model():
    return synth.SynthModel(seed=1)


@pytest.fixture(scope="module")
def weights(model):
    return fr.Weights(model)


def forward_exact(frame, W):
    """Every layer's output of the fp64 network, chaining the step references without any rounding (layer 28 = the concat)."""
    out = {}
    for l in net.LAYERS[:31]:
        i = l.idx
        if l.type == net.ROUTE:
            out[i] = out[16] if i == 25 else np.concatenate([out[27], out[24]])
            continue
        x = frame if i == 0 else out[fr.input_layer(i)]
        out[i] = fr.step_ref("exact", None, [i], dict(v=x), W)["ref"]
    return out


@pytest.fixture(scope="module")
def exact(weights):
    return forward_exact(synth.frames(40, 1)[0].astype(np.float64), weights)


# ------------------------------------------------------------------ layout

@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("C,H,W,off,Ci", [(64, 5, 7, 0, None), (425 - 1, 3, 4, 0, None), (256, 13, 13, 0, 1280), (1024, 13, 13, 256, 1280)])
def test_item_layout_round_trip(C, H, W, off, Ci, split):
    rng = np.random.default_rng(C + H)
    v = rng.standard_normal((C, H, W)) * 3
    g = fr.make_geom(C, H, W, split, off, Ci)
    raw = fr.encode(v, g, split)
    assert raw.shape == ((H + 1) * (W + 1), g["Cp"]) and g["Cp"] % 32 == 0
    if split:
        assert g["Cp"] % 64 == 0 and g["Cp"] >= 3 * g["part_stride"]
    d = fr.decode(raw, g, split)
    if split:   # hi + lo carries 22 bits: within 2^-22 relative of the fp32 value
        assert np.all(np.abs(d["v"] - v.astype(np.float32)) <= 2.0 ** -22 * np.abs(v) + 2.0 ** -25)
        assert np.array_equal(d["hi"], fr.fl16(v.astype(np.float32)))
    else:
        assert np.array_equal(d["v"], fr.fl16(v))
    assert fr.padding_violations(raw, g, split) == []
    # the zero padding the next layer relies on: a stray value in any pad place is reported
    it = raw.reshape(H + 1, W + 1, g["Cp"]).copy()
    for where, idx in (("pad row", (0, 1, off)), ("pad column", (2, W, off)), ("channels beyond C", (1, 0, g["Cp"] - 1))):
        if where == "channels beyond C" and (Ci == 1280 or g["Cp"] - 1 < off + C + (2 * g["part_stride"] if split else 0)):   # (none)
            continue
        bad = it.copy()
        bad[idx] = 0x3C00
        assert where in fr.padding_violations(bad.reshape(raw.shape), g, split)
    if split:   # the second hi copy must equal the first
        bad = it.copy()
        bad[1, 0, 2 * g["part_stride"] + off] ^= 1
        with pytest.raises(AssertionError, match="second hi copy"):
            fr.decode(bad.reshape(raw.shape), g, split)


def test_rounding_helpers():
    x = np.array([1.0, 1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 65504.0, 2.0 ** -20, -3.0e-5])
    assert np.array_equal(fr.fl16(x), x.astype(np.float16).astype(np.float64))
    assert fr.fl16(1.0 + 2 ** -11) == 1.0 and fr.fl16(1.0 + 3 * 2 ** -11) == 1.0 + 2 ** -9      # ties to even
    assert fr.ulp16(1.0) == 2 ** -10 and fr.ulp16(0.75) == 2 ** -11 and fr.ulp16(1e-7) == 2 ** -24
    hi, lo = fr.split_pair(np.float32(0.1))
    assert hi == fr.fl16(np.float32(0.1)) and lo == fr.fl16(np.float64(np.float32(0.1)) - hi) and lo != 0
    with pytest.raises(KeyError, match="no rounding model"):
        fr.rounding_of("k_conv_f16_new_kernel", "fp16")


# ------------------------------------------------------------------ wiring

def test_wiring_chained_references_reproduce_the_fp32_oracle(model, exact):
    """The fp64 step references chained without any rounding give the fp32 oracle's region tensor (pinned to the reference's fixtures)
    to ~1e-5: the route / reorg / concat order, the padding semantics and the weight layout are those of the network."""
    orclib.oracle().orc_set_threads(min(16, os.cpu_count() or 1))
    want = orclib.forward_f32(model, synth.frames(40, 1)[0]).reshape(425, 13, 13)
    got = exact[30]
    err = np.abs(got - want).max()
    print(f"wiring: max |fp64 chain - fp32 oracle| = {err:.3g} on values up to {np.abs(want).max():.3g}")
    assert err <= 2e-5, err


# ------------------------------------------------------------------ simulated kernels

def sim_conv(l, xp, wp, bias, rng, leaky_slope=fr.LEAKY):
    """A legal kernel's arithmetic: products of 16-channel chunks (exact, as in an MFMA), accumulated in fp32 in a permuted chunk
    order, + bias and leaky in fp32.  Returns float64 of the fp32 result."""
    K = l.size
    C = xp[0].shape[0]
    chunks = [(p, c0) for p in range(len(xp)) for c0 in range(0, C, 16)]
    order = rng.permutation(len(chunks))
    acc = None
    for k in order:
        p, c0 = chunks[k]
        part = fr._conv(xp[p][c0:c0 + 16], wp[p][:, c0:c0 + 16], K).astype(np.float32)
        acc = part if acc is None else (acc + part).astype(np.float32)
    v = (acc + bias.astype(np.float32)[:, None, None]).astype(np.float32)
    if l.leaky:
        v = np.where(v < 0, (v * np.float32(leaky_slope)).astype(np.float32), v)
    return v.astype(np.float64)


def simulate(path, layers, x, W, seed=0):
    """Output of a legal kernel for the launch covering `layers` (decoded value, as the checker sees the GPU's)."""
    rng = np.random.default_rng(seed)
    split = path == "split"
    cur = None
    for i, L in enumerate(layers):
        l = net.LAYERS[L]
        if l.type == net.MAXPOOL:
            cur = fr.pool2(cur)
            continue
        w = W.w[L]
        if i == 0:
            if L == 0:
                xp, wp = ([x["v"].astype(np.float32).astype(np.float64)], [w]) if not split else None, None
                if split:
                    xh, xl = fr.split_pair(x["v"])
                    wh, wl = fr.split_pair(w)
                    xp, wp = [xh, xl, xh], [wh, wh, wl]
                else:
                    xp, wp = [fr.fl16(x["v"])], [fr.fl16(w)]
            elif split:
                wh, wl = fr.split_pair(w)
                xp, wp = [x["hi"], x["lo"], x["hi"]], [wh, wh, wl]
            else:
                xp, wp = [x["v"]], [fr.fl16(w)]
            cur = sim_conv(l, xp, wp, W.b[L], rng)
        else:
            cur = sim_conv(l, [fr.fl16(cur)], [fr.fl16(w)], W.b[L], rng)
    if layers[-1] == 30:
        return cur
    if split:
        hi, lo = fr.split_pair(cur)
        return hi + lo
    return fr.fl16(cur)


def step_input(path, L, exact):
    """The decoded input a launch at layer L would read on `path` (from the fp64 network, rounded to the path's items)."""
    v = exact[fr.input_layer(L)] if L else None
    if L == 0:
        return dict(v=synth.frames(40, 1)[0].astype(np.float64))
    if path == "split":
        hi, lo = fr.split_pair(v)
        return dict(v=hi + lo, hi=hi, lo=lo)
    r = fr.fl16(v)
    return dict(v=r, hi=r, lo=np.zeros_like(r))


# (kernel, covered layers) of the launches the soundness and teeth tests simulate: the default plans' steps at layers 0, 2, 8, 20, 29
# (+ the region layer and a split 1x1)
SIM_STEPS = [
    ("fp16", "k_conv0_pool_mfma", [0, 1]), ("fp16", "k_conv_f16_rwc", [2, 3]), ("fp16", "k_conv_f16_halo<256,2,16>+1x1", [8, 9]),
    ("fp16", "k_conv_f16_halo<256,2,16>", [20]), ("fp16", "k_conv_f16_halo<256,2,16>", [29]), ("fp16", "k_gemm1_f16_p<256,128,3>", [30]),
    ("split", "k_conv0_pool_mfma<split>", [0, 1]), ("split", "k_conv_f16_glds<64,split>", [2, 3]),
    ("split", "k_conv_f16_halo<256,2,16,32,split>", [8]), ("split", "k_conv_f16_glds<128,split>", [9]),
    ("split", "k_conv_f16_halo<256,2,16,32,split>", [20]), ("split", "k_conv_f16_halo<256,2,16,32,split>", [29]),
    ("split", "k_gemm1_f16_p<256,128,3>", [30]),
]


@pytest.mark.slow
@pytest.mark.parametrize("path,kernel,layers", SIM_STEPS, ids=[f"{p}-L{ls[0]}" for p, _, ls in SIM_STEPS])
def test_checker_accepts_legal_kernels(path, kernel, layers, exact, weights):
    """Soundness: a legal kernel (fp32 accumulation of 16-channel chunks in a permuted order, fp16 RNE or split output) passes the hard
    bound and every statistical limit at real layer shapes, for two different chunk orders.  Prints the figures STAT_LIMITS is set from."""
    x = step_input(path, layers[0], exact)
    res = fr.step_ref(path, kernel, layers, x, weights)
    for seed in (1, 2):
        gpu = simulate(path, layers, x, weights, seed)
        fails, rep = fr.check_step(gpu, res)
        print(fr.report_line(f"sim {path} L{layers[0]} s{seed}", kernel, rep))
        assert not fails, fails


MUTATIONS = [
    ("drop_channel", 5), ("drop_border_tap", 7), ("shift_tile", 2560), ("no_bias_block", 1), ("leaky", 0.125), ("pool_offset",),
    ("no_lo",), ("rtz",),
]
# the launches each mutation is tried on: (path, kernel, layers); pools only where the launch pools, no_lo only on the split pass,
# round-toward-zero on the fp16 pass (the split representation's rounding is below its fp32 noise)
TEETH = []
for _m in MUTATIONS:
    for _p, _k, _ls in SIM_STEPS:
        if _m[0] == "pool_offset" and len(_ls) == 1 or _m[0] == "pool_offset" and net.LAYERS[_ls[-1]].type != net.MAXPOOL:
            continue
        if _m[0] == "no_lo" and (_p != "split" or _ls[0] == 0):
            continue
        if _m[0] == "rtz" and (_p != "fp16" or _ls[-1] == 30):
            continue
        if _m[0] in ("leaky",) and _ls[-1] == 30:
            continue
        if _m[0] == "drop_border_tap" and net.LAYERS[_ls[0]].size != 3:
            continue
        if _m[0] == "shift_tile" and _ls[-1] in (20, 29, 30):      # (13 x 13 planes: a 256-pixel tile spans frames; shift 0..255)
            _m2 = ("shift_tile", 0)
            TEETH.append((_m2, _p, _k, _ls))
            continue
        if _m[0] == "drop_channel" and _ls[0] == 0:
            _m2 = ("drop_channel", 1)
            TEETH.append((_m2, _p, _k, _ls))
            continue
        TEETH.append((_m, _p, _k, _ls))


@pytest.mark.slow
@pytest.mark.parametrize("mut,path,kernel,layers", TEETH, ids=[f"{m[0]}-{p}-L{ls[0]}" for m, p, _, ls in TEETH])
def test_checker_rejects_mutated_kernels(mut, path, kernel, layers, exact, weights):
    """Teeth: the legal kernel's output against a reference with one deliberate error (the error a subtly wrong kernel would make) is
    rejected - and, for the errors well inside the hard bound, ONLY by the statistical checks (hard_only=True accepts them)."""
    x = step_input(path, layers[0], exact)
    gpu = simulate(path, layers, x, weights, 1)
    res = fr.step_ref(path, kernel, layers, x, weights, mutate=mut)
    fails, rep = fr.check_step(gpu, res)
    print(fr.report_line(f"{mut[0]} {path} L{layers[0]}", kernel, rep), "->", fails[:1])
    assert fails, f"mutation {mut} was accepted"


def test_hard_bound_alone_misses_the_subtle_mutations(exact, weights):
    """The statistical checks are what gives the checker teeth: with the hard bound alone (gamma_n S is loose by orders of magnitude
    on the deep layers), round-toward-zero output and a dropped lo term pass."""
    missed = []
    for mut, path, kernel, layers in ((("rtz",), "fp16", "k_conv_f16_halo<256,2,16>", [20]),
                                      (("no_lo",), "split", "k_conv_f16_halo<256,2,16,32,split>", [29])):
        x = step_input(path, layers[0], exact)
        gpu = simulate(path, layers, x, weights, 1)
        res = fr.step_ref(path, kernel, layers, x, weights, mutate=mut)
        if not fr.check_step(gpu, res, hard_only=True)[0]:
            missed.append(mut[0])
        assert fr.check_step(gpu, res)[0], mut
    assert missed == ["rtz", "no_lo"], missed


# ------------------------------------------------------------------ variant coverage

DIAGNOSTIC_OPTIONS = {"f16_skip", "f16_lanes", "f16_no_lanes"}    # (+ stamp_layer, which has no f16_ name): not kernel variants


def test_every_f16_option_has_a_gpu_variant():
    """Every f16_* option of the options table (csrc/yolo2_plan.hip) is exercised by tests/test_gpu_f16_layers.py's variant list,
    except the declared diagnostic ones."""
    src = open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "csrc", "yolo2_plan.hip")).read()
    opts = set(re.findall(r'\{"(f16_[a-z0-9_]+)"', src))
    assert len(opts) >= 19, opts
    import test_gpu_f16_layers as g
    covered = {v[len("YOLO2_"):].lower() for v in g.F16_VARIANTS}
    assert opts - DIAGNOSTIC_OPTIONS <= covered, sorted(opts - DIAGNOSTIC_OPTIONS - covered)
    assert covered <= opts, sorted(covered - opts)
