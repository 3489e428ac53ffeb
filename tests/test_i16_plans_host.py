"""The int16 planner's space as tests/i16plans.py restates it, held against the committed plan table, the source lines it cites and the
sweeps of tests/test_gpu_i16_plans.py.  No GPU: the arithmetic forms are the ones the committed table states for the model it was
measured on, and the loader's split-K proofs are taken for granted (the GPU module computes them and asserts they change nothing)."""
import os
import re

import i16plans
from i16plans import Shape
from yolo2_amd import hipdrv, net

import test_gpu_i16_plans as g

TABLE = i16plans.read_table()
BATCHES = sorted({k[0] for k in TABLE})


def _launches(batch):
    return i16plans.launches_from_table(TABLE, batch)


def test_every_table_line_parses_and_every_batch_is_complete():
    text = [ln for ln in open(i16plans.TABLE) if ln.strip() and not ln.startswith("#")]
    assert len(text) == 360 and all(i16plans.parse_line(ln) is not None for ln in text)
    assert len(TABLE) == len(text)                                    # no key twice
    assert BATCHES == [1, 2, 3, 4, 5, 7, 8, 12, 16, 21, 22, 32, 64, 128, 256]
    for B in BATCHES:      # 23 conv layers + the second launch of layer 5, whose blocks run two forms
        assert sorted(k[1:] for k in TABLE if k[0] == B) == sorted([(L, 0) for L in i16plans.CONV_IDX] + [(5, 1)]), B


PARSER_PROBES = [
    "3 4 0 4 1 0 0 1 0 0 0 0", "3 4 0 4 1 0 0 1 0 0", "3 4 0 4 1 0 0 1 0", "# 3 4 0 4 1 0 0 1 0 0 0 0", "3 4 0 4 1 0 0 1 0 0 x 2",
    "3 4 0 4 3 0 0 1 0 0 0 0", "3 4 0 4 1 12345 0 1 0 0 0 0", "3 4 0 4 1 27306 8 4 1 1 1 16", "3 4 0 5 1 0 0 1 0 0 0 0",
    "3 4 0 4 1 0 2 1 0 0 0 0", "3 4 0 4 1 0 0 3 0 0 0 0", "3 4 0 4 1 0 0 1 2 0 0 0", "3 4 0 4 1 0 0 1 0 0 0 3", "0 4 0 4 1 0 0 1 0 0 0 0",
    "4097 4 0 4 1 0 0 1 0 0 0 0", "3 32 0 4 1 0 0 1 0 0 0 0", "3 4 9 4 1 0 0 1 0 0 0 0", "3 4 0 4 8 40960 4 2 0 0 1 0 trailing words",
]


def test_parser_agrees_with_the_library(tmp_path):
    """parse_line against y2_plan_line_parse, reached through the weight-side cache check (a cache with one plan line is accepted iff
    the line parses; tests/test_host_logic.py builds such files the same way)."""
    from test_host_logic import _cache_text
    L = hipdrv.lib()
    n = hipdrv.C.c_int(0)
    for i, probe in enumerate(PARSER_PROBES):
        f = tmp_path / f"p{i}.y2plan"
        f.write_text(_cache_text(0x1234, [probe]))
        ok = L.yolo2_hip_plan_cache_check(str(f).encode(), 0x1234, hipdrv.C.byref(n)) == hipdrv.YOLO2_SUCCESS
        assert ok == (i16plans.parse_line(probe) is not None), probe


def test_cited_source_lines_say_what_the_rules_restate():
    src = open(i16plans.SRC).read().splitlines()
    for name, (line, text) in {**i16plans.RULES, **i16plans.CITES}.items():
        assert text in src[line - 1], f"{name}: csrc/yolo2_int16.hip:{line} reads {src[line - 1].strip()!r}"
    hdr = open(os.path.join(i16plans.PKG, "csrc", "y2_internal.hpp")).read()
    assert f"constexpr int kMaxTileItems = {i16plans.K_MAX_TILE_ITEMS};" in hdr
    assert f"constexpr int kKsMaxBatch = {i16plans.K_KS_MAX_BATCH};" in "\n".join(src)


def test_legal_accepts_every_table_line():
    for (B, L, S), ln in TABLE.items():
        la = _launches(B)[(L, S)]
        assert la.path == ln.path
        assert i16plans.refusal(la, B, i16plans.shape_of(ln)) is None, ln


def _missing_from_replay(table):
    """The distinct (layer, launch, form, shape) of `table` that test_table_shape_replayed would not run."""
    launches = i16plans.launches_from_table(table, g.BATCH)
    per = i16plans.replay_lists(table, launches, g.BATCH)
    ran = {(L, S, launches[(L, S)].path, sh) for (L, S), shapes in per.items() for sh in shapes}
    return {(ln.L, ln.S, ln.path, i16plans.shape_of(ln)) for ln in table.values()} - ran, per


def test_replay_runs_every_distinct_table_shape():
    """A table line that the replay (tests/test_gpu_i16_plans.py::test_table_shape_replayed) does not run fails here: all 103 distinct
    (layer, shape) of the table are in its lists, at most 8 per launch, and the GPU module lists a case for each file."""
    missing, per = _missing_from_replay(TABLE)
    assert not missing, missing
    # 103 distinct (layer, shape) pairs; 106 as (layer, launch, shape), since three shapes of layer 5 occur on both of its launches
    assert len({(L, sh) for (L, S), shapes in per.items() for sh in shapes}) == 103
    assert sum(len(v) for v in per.values()) == 106 and max(len(v) for v in per.values()) == 8 == g.N_REPLAY
    # from the other side, on copies of the table with one made-up line: a legal new shape joins the lists by itself, and the census
    # above (106) no longer holds - whoever adds a line sees this test and the new GPU case; a line plan_conv would refuse is missed
    made_up = dict(TABLE)
    made_up[(64, 8, 0)] = i16plans.Line(64, 8, 0, 4, 2, 27306, 0, 1, 0, 0, 1, 0)
    assert Shape(2, 27306, 0, 1, 0, 0, 1, 0) not in per[(8, 0)]
    missing, per2 = _missing_from_replay(made_up)
    assert not missing and sum(len(v) for v in per2.values()) == 107
    made_up[(64, 8, 0)] = i16plans.Line(64, 8, 0, 4, 4, 0, 0, 1, 1, 0, 0, 0)                 # w16 at 4 pixels per lane
    assert _missing_from_replay(made_up)[0] == {(8, 0, 4, Shape(4, 0, 0, 1, 1, 0, 0, 0))}
    # and one shape taken out of the lists is missed
    launches = _launches(g.BATCH)
    short = i16plans.replay_lists(TABLE, launches, g.BATCH)
    gone = short[(29, 0)].pop()
    ran = {(L, S, launches[(L, S)].path, sh) for (L, S), shapes in short.items() for sh in shapes}
    assert {(ln.L, ln.S, ln.path, i16plans.shape_of(ln)) for ln in TABLE.values()} - ran == {(29, 0, 4, gone)}


def test_pack_gives_every_launch_its_kth_shape(tmp_path):
    launches = _launches(g.BATCH)
    per = i16plans.sweep_lists(launches, g.BATCH)
    files = i16plans.pack(per, launches, g.BATCH, tmp_path, "t", count=g.N_SWEEP + 1)
    assert len(files) == g.N_SWEEP + 1 and len({f for f, _ in files}) == len(files)
    seen = {key: [] for key in per}
    for k, (fname, chosen) in enumerate(files):
        got = i16plans.read_table(fname)
        assert set(got) == {(g.BATCH,) + key for key in launches}
        for key, sh in chosen.items():
            assert i16plans.shape_of(got[(g.BATCH,) + key]) == sh == per[key][min(k, len(per[key]) - 1)] and got[(g.BATCH,) + key].path == launches[key].path
            if sh not in seen[key]:
                seen[key].append(sh)
    assert seen == per


def test_ledger_of_the_sweep():
    """What test_tuner_candidate runs, counted: the union of the legal candidates over the launches holds every value the parser
    accepts for P, pad, splitk, pp and ks, w16 at 1 and 2 pixels per lane, hiacc at 1, 2 and 4, the fusion on all five layers in front
    of a pool, and each kernel on a 3x3 and (where it has one) a 1x1 layer."""
    launches = _launches(g.BATCH)
    per = i16plans.sweep_lists(launches, g.BATCH)
    assert all(per.values()) and max(len(v) for v in per.values()) == g.N_SWEEP <= 34
    union = [(launches[key], sh) for key, shapes in per.items() for sh in shapes]
    for field in ("P", "pad", "splitk", "pp", "ks"):
        assert {getattr(sh, field) for _, sh in union} == set(i16plans.RANGES[field]), field
    assert {sh.P for _, sh in union if sh.w16} == {1, 2}
    assert {sh.P for _, sh in union if sh.hiacc} == {1, 2, 4}
    assert {la.L for la, sh in union if sh.fuse} == set(i16plans.FUSE_LAYERS)
    kernels = {(i16plans.kernel_of(la, sh), net.LAYERS[la.L].size) for la, sh in union}
    assert kernels == {("k_conv_i16", 3), ("k_conv_i16", 1), ("k_conv_i16_splitk", 3), ("k_conv_i16_splitk", 1), ("k_conv_i16_w16", 3),
                       ("k_conv_i16_ks", 3), ("k_conv_i16_pool", 3)}       # (w16, ks and the fused kernel are 3x3 kernels)
    # every candidate is either run or refused by a named rule; no legal one is left out of the files
    for key, la in launches.items():
        for cfgx, sh in i16plans.candidates(la, g.BATCH):
            why = i16plans.refusal(la, g.BATCH, sh)
            assert (sh in per[key]) == (why is None) and (why is None or why in i16plans.RULES), (key, cfgx, sh, why)
    # the hiacc twins of the split-K and w16 forms (cfgx 30 - 18 .. 35 - 18) are always refused: 34 loop values, 26 + fusion that can run
    assert g.N_SWEEP == 8 + 3 + 2 + 7 + 4 + 1
    # rules that refuse nothing in this network, whatever the form (why test_illegal_line_is_refused has no case for them)
    for l in net.CONVS:
        halo = l.w + 2 if l.size == 3 else 0
        assert i16plans.tile_items_bound(l, 512, halo) <= i16plans.K_MAX_TILE_ITEMS
        assert l.idx not in i16plans.FUSE_LAYERS or i16plans.pool_tile_items_bound(l) <= 12 * 256
    assert {r for r, *_ in g.ILLEGAL} == set(i16plans.RULES) - {"tile_items", "fuse_tile", "fuse", "fuse_layer"}
    for rule, batch, layer, shape, force in g.ILLEGAL:
        la = _launches(batch)[(layer, 0)]
        if force is not None:
            la = la._replace(path=force, splitk_ok=False)
        assert i16plans.refusal(la, batch, shape) == rule, (rule, layer, shape)


# int16 options that are no A/B switch of the int16 planner or are exercised elsewhere, each with its reason
OPTIONS_ELSEWHERE = {
    "verbose": "prints only (set by tests/test_gpu_ref_app.py)",
    "no_plan_cache": "selects no kernel: ignores a bound weight-side cache, planning then goes on to the table like any context here",
    "no_poolfuse": "tests/test_gpu_parity.py::test_conv_pool_fusion_default_and_disabled",
    "poolfuse": "tests/test_gpu_parity.py::test_fullnet_conv_pool_fused",
    "no_ks": "tests/test_gpu_parity.py::test_ks_scratch_is_sized_from_the_accepted_plans",
    "grp16": "tests/test_gpu_parity.py::test_fullnet_sixteen_groups_per_barrier_on_1x1_layers",
    "no_edge_tiles": "tests/test_gpu_edge_tiles.py",
    "force_w16": "tests/test_gpu_parity.py::test_fullnet_sixteen_channels_per_wavefront",
    "force_hiacc": "tests/test_gpu_parity.py::test_fullnet_form_d_one_register_per_channel",
    "force_path": "tests/test_gpu_parity.py::test_fullnet_paths_and_64bit_fallback (and the refusal cases here)",
    "force_ks": "tests/test_gpu_parity.py::test_fullnet_ksplit_across_workgroups",
    "autotune": "tests/test_gpu_parity.py::test_recorded_plan_round_trips",
    "plan_write": "tests/test_gpu_parity.py::test_recorded_plan_round_trips",
    "stamp_layer": "diagnostic: time stamps of one layer's workgroups (tools/stamps.py)",
    "f32_p": "the fp32 tiled path: tests/test_gpu_parity.py::test_fp32_tiled_batch_bit_exact",
}


def test_every_int16_option_is_exercised_or_excused():
    """The option table of csrc/yolo2_plan.hip: every name that is not an f16_* option (tests/test_f16_layer_ref.py holds those) is set
    by a case of tests/test_gpu_i16_plans.py or stands in OPTIONS_ELSEWHERE with the test that sets it."""
    src = open(os.path.join(i16plans.PKG, "csrc", "yolo2_plan.hip")).read()
    table = src[src.index("const FlagOpt kFlags[]"):src.index("int Y2Options::set")]
    opts = {o for o in re.findall(r'\{"([a-z0-9_]+)", &Y2Options::', table) if not o.startswith("f16_")}
    assert len(opts) >= 27, sorted(opts)
    exercised = set(g.OPTIONS_EXERCISED)
    assert {"no_grp", "no_xcd_remap", "splitk_no_pack", "splitk", "no_hiacc", "no_w16", "lanes", "lane_split", "no_lanes", "lane_priority",
            "plan_file", "force_p"} <= exercised
    assert exercised <= opts and set(OPTIONS_ELSEWHERE) <= opts, sorted((exercised | set(OPTIONS_ELSEWHERE)) - opts)
    assert not exercised & set(OPTIONS_ELSEWHERE)
    assert opts == exercised | set(OPTIONS_ELSEWHERE), sorted(opts - exercised - set(OPTIONS_ELSEWHERE))
    root = os.path.dirname(i16plans.PKG)
    for name, where in OPTIONS_ELSEWHERE.items():      # the excuse names a test file that does set the option
        m = re.search(r"tests/[a-z0-9_]+\.py", where)
        if m:
            text = open(os.path.join(root, m.group(0))).read()
            assert name in text.lower(), (name, where)
