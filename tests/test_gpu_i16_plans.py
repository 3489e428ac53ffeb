"""The int16 planner's launch shapes, each run bit-exact from a plan file (run with -m gpu on the MI355X box).

Which kernel and shape a conv launch runs is decided by plan_conv / autotune (csrc/yolo2_int16.hip); the force_* hooks and the
stopwatch reach only part of that space, and not a fixed part.  Option plan_file pins it: a line is applied only if plan_conv
reproduces it exactly, so a file that names one shape per launch either runs exactly those kernels ("plan table", and conv_plan says
which) or sends the batch to timing ("autotuned in this process").  tests/i16plans.py restates the space; here

  * the committed table's distinct shapes (test_table_shape_replayed) and every table batch up to 32 (test_table_batch),
  * every candidate of the tuner that plan_conv accepts (test_tuner_candidate), and one per refusing rule (test_illegal_line_is_refused),
  * the A/B options no other test sets (OPTION_CASES, LANE_CASES)

run on batch 3 as [fixture frame, another frame, fixture frame] - tiles straddle frames - and must give the bits of
tests/golden/fullnet.npz (the compiled reference's region tensor) and of the oracle.  No tolerances: everything is array_equal.

Nothing depends on the batch except the K-split over workgroups (`ks`), which exists for batches <= 4: batch 3 is legal for all of it.
One context per Q set serves the whole module and is re-planned per case (yolo2_hip_set_batch re-plans an unlaned context).
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import i16plans
import orclib
from i16plans import Shape
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
FULL = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))
TABLE = i16plans.read_table()
BATCH = 3
QSETS = ("std", "varq")

# How many files the two sweeps need, known without a GPU so that the cases can be listed: the longest list of any launch.  The
# table's own model (std) has 3x3 form D layers with every split-K proof, which is the launch with most legal candidates; a Q set
# whose launches have fewer repeats its last file (pack(count=...)), and _state asserts that none needs more.
_STD = i16plans.launches_from_table(TABLE, BATCH)
N_REPLAY = max(len(v) for v in i16plans.replay_lists(TABLE, _STD, BATCH).values())
N_SWEEP = max(len(v) for v in i16plans.sweep_lists(_STD, BATCH).values())

# ---- item 5: the int16 A/B options no other test sets (tests/test_i16_plans_host.py holds the option list against these)
# name: (options, what must show in conv_plan).  no_grp and no_xcd_remap act inside plan_conv and are planned without timing through force_p;
# the other three act inside autotune and cost one timed batch each.
OPTION_CASES = {
    "no_grp": ({"no_grp": 1, "force_p": 2}, "every 1x1 layer runs one channel group per barrier"),
    "no_xcd_remap": ({"no_xcd_remap": 1, "force_p": 1}, "no launch remaps its grid over the XCDs"),
    "splitk_no_pack": ({"splitk_no_pack": 1, "splitk": 1}, "the lane-split kernel keeps unpacked triples on form D layers"),
    "no_hiacc": ({"no_hiacc": 1}, "no launch runs one accumulator register per channel"),
    "no_w16": ({"no_w16": 1}, "no launch runs sixteen channels per wavefront"),
}
# name: (options, batch, lanes expected)
LANE_CASES = {
    "lanes+lane_split": ({"lanes": 3, "lane_split": "12,4,8"}, 24, 3),      # (the default would be 8 + 8 + 8; all are table batches)
    "no_lanes": ({"no_lanes": 1}, 16, 1),
}
CHILD_CASES = {"lane_priority": ({"YOLO2_LANE_PRIORITY": "0"}, 16, 2)}      # latched process-wide: a process of its own
OPTIONS_EXERCISED = sorted({o for opts, _ in OPTION_CASES.values() for o in opts} | {o for opts, _, _ in LANE_CASES.values() for o in opts}
                           | {"plan_file"} | {k[len("YOLO2_"):].lower() for env, _, _ in CHILD_CASES.values() for k in env})


def _qsets():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.Q_SETS


def _diagnose(ctx, model, frame, frame_idx):
    """Layer-by-layer diff against the oracle to localise a mismatch."""
    _, _, _, layers = orclib.forward_i16(model, frame, dump=True)
    fused = ctx.pool_fused_layers()
    for i in sorted(layers):
        if i in fused and i != 16:
            continue          # conv + pool ran as one kernel: that conv's own tensor was never written
        got = ctx.debug_layer_output(i, frame_idx)
        l = net.LAYERS[i]
        if not np.array_equal(got[:, :, :l.out_w], layers[i][:, :, :l.out_w]):
            bad = np.argwhere(got[:, :, :l.out_w] != layers[i][:, :, :l.out_w])
            return f"first differing layer {i} ({l.type}) [{ctx.conv_plan(l.ord) if l.type == net.CONV else ''}]: {len(bad)} elems, first at {bad[0]}"
    return "all layer tensors equal"


class _State:
    pass


@pytest.fixture(scope="module")
def states(tmp_path_factory):
    """Per Q set, made on first use and kept for the module: the model, the three frames, the fixture's and the oracle's region
    tensors (computed once), one context, what its loader proved, and the plan files of both sweeps."""
    assert hipdrv.lib().yolo2_hip_device_count() >= 1, "no GPU visible: these tests must run on the GPU box"
    made = {}
    fseed = int(FULL["meta/frame_seed"])
    base = np.concatenate([synth.frames(fseed + k, 1) for k in range(4)])     # frame 0: the fixture's
    outdir = tmp_path_factory.mktemp("i16plans")

    def get(qset):
        if qset in made:
            return made[qset]
        st = _State()
        st.qset, st.base = qset, base
        st.model = synth.SynthModel(seed=int(FULL["meta/model_seed"]), **_qsets()[qset])
        st.frames = np.concatenate([base[0:1], base[1:2], base[0:1]])
        st.want0 = FULL[f"i16/{qset}/region_raw_i16"].reshape(425, 13, 13)
        orclib.oracle().orc_set_threads(16)
        st.want1 = orclib.forward_i16(st.model, base[1])[0].reshape(425, 13, 13)
        st.ctx = hipdrv.Yolo2Hip(0)
        st.ctx.load_model(st.model)
        st.launches = i16plans.launches_from_counts(st.ctx.layer_path_counts(), i16plans.splitk_proved(st.model))
        assert [st.launches[(l.idx, 0)].path for l in net.CONVS] == st.ctx.layer_paths()
        if qset == "std":   # the committed table states this model's forms
            assert {k: la.path for k, la in st.launches.items()} == {k: la.path for k, la in _STD.items()}
        st.replay_lists = i16plans.replay_lists(TABLE, st.launches, BATCH)
        if qset == "std":   # ... and every one of its lines is legal with what the loader really proved (the host tests assume the proofs)
            assert st.replay_lists == i16plans.replay_lists(TABLE, _STD, BATCH)
        st.sweep_lists = i16plans.sweep_lists(st.launches, BATCH)
        st.replay = i16plans.pack(st.replay_lists, st.launches, BATCH, outdir, f"replay_{qset}", count=N_REPLAY)
        st.sweep = i16plans.pack(st.sweep_lists, st.launches, BATCH, outdir, f"sweep_{qset}", count=N_SWEEP)
        st.outdir = outdir
        st.alone = None
        for name, lists in (("replay", st.replay_lists), ("sweep", st.sweep_lists)):
            print(f"[i16 plans] {qset} {name}: {sum(len(v) for v in lists.values())} (layer, launch, shape) pairs over {len(lists)} launches")
        made[qset] = st
        return st

    yield get
    for st in made.values():
        st.ctx.close()


def _plan_from(st, fname, batch=BATCH):
    st.ctx.set_option("plan_file", fname)
    st.ctx.set_batch(batch)
    return st.ctx.plan_source()


def _check_bits(st, ctx, region, what):
    for f, want in ((0, st.want0), (1, st.want1), (2, st.want0)):
        if not np.array_equal(region[f], want):
            pytest.fail(f"{what}: frame {f}: " + _diagnose(ctx, st.model, st.frames[f], f))


def _run_file(st, fname, chosen):
    """One plan file: it must be taken as it stands, every layer must state the requested shape, and the bits must be right."""
    src = _plan_from(st, fname)
    if src != "plan table":      # name the refused line (the library says which on stderr when verbose)
        st.ctx.set_option("verbose", 1)
        try:
            _plan_from(st, fname)
        finally:
            st.ctx.set_option("verbose", None)
        pytest.fail(f"{os.path.basename(fname)}: plan source is '{src}': the planner refused a line that i16plans.legal accepts\n" + open(fname).read())
    for l in net.CONVS:
        la = st.launches[(l.idx, 0)]
        want = i16plans.expected_plan(la, chosen[(l.idx, 0)])
        got = i16plans.plan_fields(st.ctx.conv_plan(l.ord))
        assert {k: got[k] for k in want} == want and got["form"] == la.path and got["extra"] == la.n_launches - 1, (l.idx, chosen[(l.idx, 0)], got)
    region, q = st.ctx.run_batch_host(st.frames)
    assert q == int(FULL[f"i16/{st.qset}/final_q"])
    _check_bits(st, st.ctx, region, os.path.basename(fname))


# ------------------------------------------------------------------ item 3: the committed table, replayed

@pytest.mark.parametrize("k", range(N_REPLAY))
@pytest.mark.parametrize("qset", QSETS)
def test_table_shape_replayed(qset, k, states):
    """File k gives every launch the k-th distinct shape the committed table holds for it over all its batches (for varq: with the form
    this model's loader proved, shapes illegal for that form dropped).  The `ks` shapes come from the table's batches 1 - 3; their rule
    does not depend on the batch up to 4, so they run here at batch 3 like everything else."""
    st = states(qset)
    assert max(len(v) for v in st.replay_lists.values()) <= N_REPLAY
    _run_file(st, *st.replay[k])


def _base_frames_alone(st):
    """The four base frames, each run alone (batch 1, committed table); frames 0 and 1 are held to the fixture and the oracle."""
    if st.alone is None:
        st.ctx.set_option("plan_file", None)
        out = []
        for f in range(4):
            r, _ = st.ctx.run_batch_host(st.base[f:f + 1])
            assert st.ctx.plan_source() == "plan table"
            out.append(r[0])
        assert np.array_equal(out[0], st.want0) and np.array_equal(out[1], st.want1)
        st.alone = out
    return st.alone


def _period4(st, ctx, batch, what):
    frames = np.concatenate([st.base] * ((batch + 3) // 4))[:batch]
    region, _ = ctx.run_batch_host(frames)
    alone = _base_frames_alone(st)
    bad = [f for f in range(batch) if not np.array_equal(region[f], alone[f % 4])]
    assert not bad, f"{what}: frames {bad} differ from the same frame run alone"


@pytest.mark.parametrize("batch", sorted(b for b in {k[0] for k in TABLE} if b <= 32))
def test_table_batch(batch, states):
    """Every batch of the committed table up to 32, once, under the committed table: 1 - 12 unlaned; 16 and 32 as two lanes (of 8 and
    16 frames: table batches too); 21 and 22 - the lane sizes of the bench's batch 64 - unlaned (option no_lanes), since a context of
    21 frames would split into lanes of sizes the table does not hold.  Frames of period 4, each equal to the same frame run alone."""
    st = states("std")
    alone = _base_frames_alone(st)
    assert len(alone) == 4
    unlaned = batch in (21, 22)
    st.ctx.set_option("plan_file", None)
    try:
        if unlaned:
            st.ctx.set_option("no_lanes", 1)
        st.ctx.set_batch(batch)
        assert st.ctx.plan_source() == "plan table"
        assert st.ctx.num_lanes() == (2 if batch in (16, 32) else 1)
        want = {l.idx: TABLE[(batch // 2 if batch in (16, 32) else batch, l.idx, 0)] for l in net.CONVS}      # (conv_plan: lane 0's)
        for l in net.CONVS:
            exp = i16plans.expected_plan(st.launches[(l.idx, 0)], i16plans.shape_of(want[l.idx]))
            got = i16plans.plan_fields(st.ctx.conv_plan(l.ord))
            assert {k: got[k] for k in exp} == exp, (l.idx, want[l.idx], got)
        _period4(st, st.ctx, batch, f"batch {batch}")
    finally:
        st.ctx.set_option("no_lanes", None)
        st.ctx.set_batch(BATCH)      # (leaves lane mode: the other cases re-plan an unlaned context)


# ------------------------------------------------------------------ item 4: the tuner's whole space

@pytest.mark.parametrize("k", range(N_SWEEP))
@pytest.mark.parametrize("qset", QSETS)
def test_tuner_candidate(qset, k, states):
    """File k gives every launch the k-th of the candidates autotune enumerates for it and plan_conv accepts (i16plans.candidates /
    legal).  A file that ends in "autotuned in this process" is a failure: legal() said the planner would take every line."""
    st = states(qset)
    assert max(len(v) for v in st.sweep_lists.values()) <= N_SWEEP
    _run_file(st, *st.sweep[k])


# one line per refusing rule, put into a file of one-pixel tiles (legal everywhere): (rule, batch, layer, shape, force_path)
# force_path=2 makes every launch the 64-bit form, for which nothing is proved: maxP is 4 and the lane-split bounds do not hold.
ILLEGAL = [
    ("maxP", 3, 8, Shape(8, 0, 0, 1, 0, 0, 0, 0), 2),
    ("splitk", 3, 13, Shape(1, 0, 4, 1, 0, 0, 0, 0), 2),            # not proved (splitk_ok)
    ("splitk", 3, 22, Shape(1, 0, 8, 1, 0, 0, 0, 0), None),         # 8 splits on a 3x3 layer
    ("splitk_pp", 3, 21, Shape(1, 0, 4, 2, 0, 0, 0, 0), None),      # 2 pixels per lane on a 1x1 layer
    ("ks", 3, 4, Shape(1, 0, 0, 1, 0, 0, 0, 16), None),             # 16 splits of 16 channel groups: fewer than two each
    ("ks_fits", 5, 8, Shape(1, 0, 0, 1, 0, 0, 0, 2), None),         # no triple scratch past batch 4
    ("ks_shape", 3, 8, Shape(2, 0, 0, 1, 0, 0, 0, 2), None),        # the K-split kernel has one pixel per lane
    ("w16", 3, 8, Shape(4, 0, 0, 1, 1, 0, 0, 0), None),             # sixteen channels per wavefront: at most 2 pixels per lane
    ("hiacc", 3, 8, Shape(8, 0, 0, 1, 0, 0, 1, 0), None),           # one register per channel: at most 4 pixels per lane
    # fields that an accepted kernel choice resets, so that the line is not reproduced
    ("splitk_shape", 3, 13, Shape(2, 0, 4, 1, 0, 0, 0, 0), None),   # the lane-split kernel has its own tile: P is 1
    ("w16_pad", 3, 8, Shape(1, 27306, 0, 1, 1, 0, 0, 0), None),     # no occupancy cap on the two-wave workgroups
    ("ks_pad", 3, 8, Shape(1, 27306, 0, 1, 0, 0, 0, 2), None),      # ... nor on the K-split kernel
]
# RULES not among them: tile_items and fuse_tile refuse nothing in this network (tests/test_i16_plans_host.py computes that);
# fuse and fuse_layer are not refused (next test).


@pytest.mark.parametrize("rule,batch,layer,shape,force", ILLEGAL, ids=[f"{r}-L{l}-{'x'.join(map(str, s))}" for r, _, l, s, _ in ILLEGAL])
def test_illegal_line_is_refused(rule, batch, layer, shape, force, states, tmp_path):
    """legal() from the other side: one line that the named rule refuses sends the whole batch to timing, and the bits stay right."""
    st = states("std")
    ctx = st.ctx
    launches = st.launches
    if force is not None:
        ctx = hipdrv.Yolo2Hip(0)
        ctx.set_option("force_path", force)
        ctx.load_model(st.model)
        assert set(ctx.layer_paths()) == {force}
        launches = i16plans.launches_from_counts(ctx.layer_path_counts(), [False] * len(net.CONVS))
    try:
        la = launches[(layer, 0)]
        assert i16plans.refusal(la, batch, shape) == rule
        good = {key: Shape(1, 0, 0, 1, 0, 0, 0, 0) for key in launches}
        assert all(i16plans.legal(launches[key], batch, sh) for key, sh in good.items())
        (ok_file, _), = i16plans.pack({k: [v] for k, v in good.items()}, launches, batch, tmp_path, f"legal_{rule}_{layer}")
        good[(layer, 0)] = shape
        (bad_file, _), = i16plans.pack({k: [v] for k, v in good.items()}, launches, batch, tmp_path, f"illegal_{rule}_{layer}")
        frames = np.concatenate([st.frames, st.frames])[:batch]
        for fname, source in ((ok_file, "plan table"), (bad_file, "autotuned in this process")):    # the file is taken without the line
            ctx.set_option("plan_file", fname)
            ctx.set_batch(batch)
            assert ctx.plan_source() == source, (fname, ctx.plan_source())
            region, _ = ctx.run_batch_host(frames)
            want = [st.want0, st.want1, st.want0, st.want0, st.want1][:batch]
            for f in range(batch):
                assert np.array_equal(region[f], want[f]), (source, f, _diagnose(ctx, st.model, frames[f], f))
    finally:
        if ctx is not st.ctx:
            ctx.close()


def test_fuse_on_a_layer_that_cannot_fuse_runs_separate_kernels(states, tmp_path):
    """The one rule whose breach is not refused: fuse=1 on a conv without a pool behind it (layer 4) or whose blocks do not all run a
    packed form keeps the table and runs the conv and the pool apart."""
    st = states("std")
    shapes = {key: [Shape(1, 0, 0, 1, 0, 1, 0, 0)] for key in st.launches}
    (fname, chosen), = i16plans.pack(shapes, st.launches, BATCH, tmp_path, "fuse_everywhere")
    assert i16plans.refusal(st.launches[(4, 0)], BATCH, chosen[(4, 0)]) == "fuse_layer"
    assert _plan_from(st, fname) == "plan table"
    fusable = [L for (L, S), la in st.launches.items() if S == 0 and i16plans.legal(la, BATCH, chosen[(L, S)])]
    assert st.ctx.pool_fused_layers() == sorted(fusable) == list(i16plans.FUSE_LAYERS)
    assert all((i16plans.plan_fields(st.ctx.conv_plan(l.ord))["fused"] != 0) == (l.idx in fusable) for l in net.CONVS)
    region, _ = st.ctx.run_batch_host(st.frames)
    _check_bits(st, st.ctx, region, "fuse=1 on every line")


# ------------------------------------------------------------------ item 5: the options no other test sets

def _with_options(st, opts):
    ctx = hipdrv.Yolo2Hip(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.load_model(st.model)
    return ctx


@pytest.mark.parametrize("name", list(OPTION_CASES))
def test_ab_option(name, states):
    """Each int16 A/B option that nothing else sets: the launches change where the option says, the bits do not."""
    opts, _ = OPTION_CASES[name]
    st = states("std")
    ctx = _with_options(st, opts)
    try:
        ctx.set_batch(BATCH)
        assert ctx.plan_source() == ("forced by a test hook" if "force_p" in opts else "autotuned in this process")
        plans = {l.idx: i16plans.plan_fields(ctx.conv_plan(l.ord)) for l in net.CONVS}
        one_by_one = [l.idx for l in net.CONVS if l.size == 1]
        if name == "no_grp":
            assert all(plans[L]["grp"] == 1 and plans[L]["P"] == 2 for L in one_by_one), plans
        elif name == "no_xcd_remap":
            assert all(p["xcd"] == 0 for p in plans.values()), plans
        elif name == "splitk_no_pack":
            split = [L for L, p in plans.items() if p["splitk"]]
            assert len(split) >= 10 and any(net.LAYERS[L].size == 3 for L in split) and any(net.LAYERS[L].size == 1 for L in split), plans
            assert all(p["pack"] == 0 and p["pp"] == 1 for p in plans.values()) and all(plans[L]["form"] == 4 for L in split), plans
        elif name == "no_hiacc":
            assert all(p["hiacc"] == 0 for p in plans.values()), plans
        elif name == "no_w16":
            assert all(p["w16"] == 0 for p in plans.values()), plans
        region, _ = ctx.run_batch_host(st.frames)
        _check_bits(st, ctx, region, name)
        if "force_p" in opts:        # the same forced plan without the option does the opposite
            ctx.set_option(name, None)
            ctx.set_batch(BATCH)
            dflt = {l.idx: i16plans.plan_fields(ctx.conv_plan(l.ord)) for l in net.CONVS}
            if name == "no_grp":
                assert all(dflt[L]["grp"] == 8 for L in one_by_one), dflt
            else:
                assert all(p["xcd"] >= 1 for p in dflt.values()), dflt
    finally:
        ctx.close()
    if name == "splitk_no_pack":     # the default packs (committed table: form D layers on the lane-split kernel)
        st.ctx.set_option("plan_file", None)
        st.ctx.set_batch(BATCH)
        dflt = [i16plans.plan_fields(st.ctx.conv_plan(l.ord)) for l in net.CONVS]
        assert any(p["pack"] == 1 for p in dflt) and all(p["pack"] == (1 if p["splitk"] and p["form"] == 4 else 0) for p in dflt), dflt


@pytest.mark.parametrize("name", list(LANE_CASES))
def test_lane_option(name, states):
    """Lane count and split by option: every frame of the batch equals the same frame run alone, whichever lane ran it."""
    opts, batch, lanes = LANE_CASES[name]
    st = states("std")
    ctx = _with_options(st, opts)
    try:
        ctx.set_batch(batch)
        assert ctx.num_lanes() == lanes and ctx.plan_source() == "plan table"      # lanes of 8 / a context of 16: table batches
        _period4(st, ctx, batch, name)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(CHILD_CASES))
def test_lane_option_latched_per_process(name):
    """lane_priority is read once per process (the lanes' stream priority): a fresh process runs a laned batch with it; every frame
    must equal the same frame run alone in that process, and frame 0 the fixture."""
    env_extra, batch, lanes = CHILD_CASES[name]
    code = (
        "import sys, json, numpy as np\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'yolo-fpga-accelerator_amd')!r})\n"
        "from yolo2_amd import hipdrv, synth\n"
        "m = synth.SynthModel(seed=1); ctx = hipdrv.Yolo2Hip(0); ctx.load_model(m)\n"
        "base = np.concatenate([synth.frames(7 + k, 1) for k in range(4)])\n"
        f"r, _ = ctx.run_batch_host(np.concatenate([base] * {(batch + 3) // 4})[:{batch}])\n"
        "lanes, src, opts = ctx.num_lanes(), ctx.plan_source(), ctx.options()\n"
        "alone = [ctx.run_batch_host(base[f:f + 1])[0][0] for f in range(4)]\n"
        f"want = np.load({os.path.join(ROOT, 'tests', 'golden', 'fullnet.npz')!r})['i16/std/region_raw_i16'].reshape(425, 13, 13)\n"
        "print('PROBE ' + json.dumps({'lanes': lanes, 'source': src, 'options': opts, 'fixture': bool(np.array_equal(alone[0], want)),\n"
        f"    'bad': [f for f in range({batch}) if not np.array_equal(r[f], alone[f % 4])]}}))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("YOLO2_")}
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
    assert r["lanes"] == lanes and r["source"] == "plan table" and "lane_priority=0" in r["options"], r
    assert r["fixture"] and r["bad"] == [], r
