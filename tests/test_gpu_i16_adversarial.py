"""The int16 conv on worst-case chains at the limits of each arithmetic form (run with -m gpu on the MI355X box).

The loader runs every block of output channels in the narrowest form it can prove exact from the weights; each proof is a statement
about the worst input - every operand of a quad at -32768 or 32767, weights' signs aligned, step after step the same way - which
random data never comes near.  tests/i16adv.py builds that input (tests/test_i16_adversarial_host.py holds it to the oracle on the CPU):

  part A  the per-layer driver call at every transition of the selected form in M = sum |w| of a quad, found by bisection on
          yolo2_hip_last_layer_path - whatever form the loader picks must be exact on the worst input, at M* - 1 .. M* + 2,
  part B  designed chains (quarter-chain sums below, at and beyond 2^15 and 2^16, both signs) in four watched convs of a whole
          network, through every launch shape a context can be given: the lane-split kernels (packed, unpacked, int32 triples),
          the K-split over workgroups, sixteen channels per wavefront, one register per channel, conv + pool, grp16, edge tiles,
          and every tuner candidate from plan files.

Every comparison is array_equal against the oracle.  The limits found and the plan lines that ran are printed.
"""
import numpy as np
import pytest

import i16adv
import i16plans
import orclib
from i16plans import Shape
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu
FORMS = {0: "A", 1: "B", 2: "64-bit", 3: "C", 4: "D"}
M_MAX = 4 * 32767      # the largest quad sum positive int16 weights can hold


@pytest.fixture(scope="module", autouse=True)
def driver():
    L = hipdrv.lib()
    assert L.yolo2_hip_device_count() >= 1, "no GPU visible: these tests must run on the GPU box"
    hipdrv.check(L.yolo2_accel_init(), "yolo2_accel_init")
    yield L
    L.yolo2_accel_cleanup()


def _process_option(name, value):
    hipdrv.check(hipdrv.lib().yolo2_hip_set_option(None, name.encode(), None if value is None else str(value).encode()),
                 "yolo2_hip_set_option")


# ------------------------------------------------------------------ part A: form limits through the per-layer driver call

class _LayerCall:
    """yolo2_execute_conv_layer on one layer shape (stride 1, "same"), device buffers kept between calls."""

    def __init__(self, C, N, K, HW):
        self.C, self.N, self.K, self.HW, self.pad = C, N, K, HW, K // 2
        self.shape = (N, HW, orclib.w8(HW))
        self.bx = hipdrv.DevBuf(nbytes=C * HW * orclib.w8(HW) * 2)
        self.bw = hipdrv.DevBuf(nbytes=N * C * K * K * 2)
        self.bb = hipdrv.DevBuf(nbytes=N * 2)
        self.by = hipdrv.DevBuf(nbytes=int(np.prod(self.shape)) * 2)
        self.calls = 0

    def _put(self, buf, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == buf.nbytes
        hipdrv.check(hipdrv.lib().yolo2_hip_memcpy_h2d(buf.addr, arr.ctypes.data, arr.nbytes), "h2d")

    def run(self, x, wr, b, q):
        """-> (output, form that ran, 1 if the edge-class kernel ran)"""
        L, C, N, K, HW = hipdrv.lib(), self.C, self.N, self.K, self.HW
        self._put(self.bx, x); self._put(self.bw, wr); self._put(self.bb, b)
        hipdrv.check(L.yolo2_hip_memset(self.by.addr, 0, self.by.nbytes), "memset")
        T = min(min(27 - K + 1, 13), HW)
        TM, TN, mL = min(N, 32), min(C, 4), -(-N // min(N, 32))
        Qw, Qai, Qao, Qb = q
        hipdrv.check(L.yolo2_execute_conv_layer(self.bx.addr, self.by.addr, self.bw.addr, self.bb.addr, C, N, K, 1, HW, HW, HW, HW, self.pad, 1, 0,
                                                TM, TN, T, T, (mL + 1) * TM, mL * TM, (mL + 1) * TM, 0, Qw, Qai, Qao, Qb, 60000),
                     "yolo2_execute_conv_layer")
        self.calls += 1
        return self.by.get(np.int16, self.shape), L.yolo2_hip_last_layer_path(), L.yolo2_hip_last_layer_edge()

    def oracle(self, x, wr, b, q):
        return orclib.conv_i16(x, wr, b, self.C, self.N, self.K, 1, self.HW, self.HW, self.pad, 1, *q)

    def free(self):
        for d in (self.bx, self.bw, self.bb, self.by):
            d.free()


_weights = {}


def _quad(N, C, K, M, sign):
    key = (N, C, K, M, sign)
    if key not in _weights:
        _weights[key] = synth.reorg_weights(i16adv.quad_weights(N, C, K, M, sign), C, N, K)
    return _weights[key]


def _transitions(form_at, lo=1, hi=M_MAX):
    """[(M*, form up to M*, form from M* + 1)] over lo..hi, by bisection.  Assumes only that a form, once left as M grows, does not
    come back (each form is legal up to a bound of its own) - the runs at M* - 1 .. M* + 2 check the forms found."""
    out, f = [], form_at(lo)
    while f != form_at(hi):
        a, b = lo, hi
        while b - a > 1:
            mid = (a + b) // 2
            if form_at(mid) == f:
                a = mid
            else:
                b = mid
        out.append((a, f, form_at(b)))
        lo, f = b, form_at(b)
    return out


def _limits(K, q, bname):
    """The transitions of the form the loader selects for quads of sum M, on the tiny probe layer."""
    C, N, HW = i16adv.PROBE["C"], i16adv.PROBE["N"], i16adv.PROBE["HW"][K]
    probe = _LayerCall(C, N, K, HW)
    x, b, seen = i16adv.extreme_inputs(C, HW, HW, "min"), i16adv.bias_set(N, bname), {}

    def form_at(M):
        if M not in seen:
            seen[M] = probe.run(x, synth.reorg_weights(i16adv.quad_weights(N, C, K, M, "pos"), C, N, K), b, q)[1]
        return seen[M]
    try:
        return _transitions(form_at)
    finally:
        probe.free()


def _form_at(trans, M):
    for m_star, f_lo, _ in trans:
        if M <= m_star:
            return f_lo
    return trans[-1][2]


def _first_diff(got, want, W):
    bad = np.argwhere(got[:, :, :W] != want[:, :, :W])
    return f"{len(bad)} differ, first at (channel, y, x) = {tuple(int(v) for v in bad[0])}: got {int(got[tuple(bad[0])])}, want {int(want[tuple(bad[0])])}"


@pytest.mark.parametrize("bias_shift", i16adv.BIAS_SHIFTS)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("s", i16adv.SHIFTS)
def test_form_limits_exact_on_worst_input(s, K, bias_shift, driver):
    """Per bias set: bisect the limits; at each limit M* run M* - 1 .. M* + 2 on every extreme input x every sign pattern - the form
    that ran is the one the bisection found on that side of the limit, and the bits are the oracle's; at M* the forced forms
    A, B, C, D and 64-bit (an illegal one falls back to the loader's choice) and, where edge-class tiles apply, raster tiles agree."""
    q = i16adv.layer_q(s, bias_shift)
    C, N, HW = i16adv.LAYER["C"], i16adv.LAYER["N"], i16adv.LAYER["HW"][K]
    orclib.oracle().orc_set_threads(1)
    call = _LayerCall(C, N, K, HW)
    try:
        for bname in i16adv.BIAS_SETS:
            trans = _limits(K, q, bname)
            print(f"[i16 limits] s={s} K={K} bias shift={bias_shift} bias={bname}: " +
                  (", ".join(f"{FORMS[a]} up to M={m}, then {FORMS[b]}" for m, a, b in trans) or f"one form over 1..{M_MAX}"))
            assert trans, "the 64-bit form must take over before the largest quad sum"
            assert trans[-1][2] == 2 and len({f for _, f, _ in trans}) == len(trans), trans
            if bname == "one_lo" and i16adv.shift(-32768, bias_shift) < -32767:
                # a shifted bias of -32768 or below does not fit a packed int16 accumulator: forms C and D must not be chosen
                # (with bias shift 3 the accumulator starts from -4096, which does fit)
                assert not {3, 4} & {f for _, f, _ in trans}, trans
            b = i16adv.bias_set(N, bname)
            for m_star, _, _ in trans:
                for M in (m_star - 1, m_star, m_star + 1, m_star + 2):
                    if not 1 <= M <= M_MAX:
                        continue
                    for sign in i16adv.SIGNS:
                        wr = _quad(N, C, K, M, sign)
                        for kind in i16adv.KINDS:
                            what = (bname, M, m_star, sign, kind)
                            x = i16adv.extreme_inputs(C, HW, HW, kind, seed=M)
                            want = call.oracle(x, wr, b, q)
                            got, form, edge = call.run(x, wr, b, q)
                            assert form == _form_at(trans, M), (what, form, trans)
                            assert np.array_equal(got, want), (what, FORMS[form], _first_diff(got, want, HW))
                            if M != m_star:
                                continue
                            try:
                                for force in (0, 1, 3, 4, 2):
                                    _process_option("force_path", force)
                                    forced, fform, _ = call.run(x, wr, b, q)
                                    assert fform in (force, form), (what, force, fform)
                                    assert np.array_equal(forced, want), (what, "forced", FORMS[fform], _first_diff(forced, want, HW))
                                _process_option("force_path", None)
                                if K == 3 and form in (3, 4):
                                    assert edge == 1, what      # (one pixel per lane on a layer this small)
                                    _process_option("no_edge_tiles", 1)
                                    raster, rform, redge = call.run(x, wr, b, q)
                                    assert (rform, redge) == (form, 0), what
                                    assert np.array_equal(raster, want), (what, "raster tiles", _first_diff(raster, want, HW))
                            finally:
                                _process_option("force_path", None)
                                _process_option("no_edge_tiles", None)
        print(f"[i16 limits] s={s} K={K} bias shift={bias_shift}: {call.calls} layer calls")
    finally:
        call.free()
        _weights.clear()


# ------------------------------------------------------------------ part B: designed chains through the launch shapes of a context

WATCHED = {c.watched: net.CONVS[c.watched].idx for c in i16adv.CASES}       # conv ordinal -> layer
ONE_PIXEL = Shape(1, 0, 0, 1, 0, 0, 0, 0)
SWEEP_BATCH = 3
# the longest candidate list a watched launch can have: form D with every proof (pack(count=...) repeats the last file for shorter ones)
N_SWEEP = max(len([sh for _, sh in i16plans.candidates(la, SWEEP_BATCH) if i16plans.legal(la, SWEEP_BATCH, sh)])
              for la in (i16plans.Launch(L, 0, 4, 1, True, L in i16plans.FUSE_LAYERS) for L in WATCHED.values()))


class _State:
    pass


def _oracle_watched(model, info):
    """Per watched conv: the designed input and the oracle's conv of it (and the pool behind conv 12), computed once."""
    designed, want = {}, {}
    for o, inf in info.items():
        l = net.CONVS[o]
        designed[o] = i16adv.designed_input(inf, net.LAYERS[l.idx - 1])
        want[l.idx] = orclib.conv_i16(designed[o], model.w_reorg[o], model.bias[o], l.c, l.n, l.size, 1, l.w, l.h, l.pad, 1,
                                      int(model.weight_q[o]), int(model.act_q[o]), int(model.act_q[o + 1]), int(model.bias_q[o]))
        if net.LAYERS[l.idx + 1].type == net.MAXPOOL:
            want[l.idx + 1] = orclib.maxpool(want[l.idx], l.n, l.w, l.h)
    return designed, want


def _load(model, opts=None):
    ctx = hipdrv.Yolo2Hip(0)
    for k, v in (opts or {}).items():
        ctx.set_option(k, v)
    ctx.load_model(model)
    return ctx


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """The chain model, two frames and their oracle results (computed once), and two contexts for the module: one only ever planned
    by the force_* hooks, one planned by the table, the stopwatch and plan files (a forced plan keeps the fields a tuned one left)."""
    st = _State()
    st.model, st.info = i16adv.chain_model(3)
    orclib.oracle().orc_set_threads(16)
    st.designed, st.want = _oracle_watched(st.model, st.info)
    f, g = synth.frames(11, 1), synth.frames(12, 1)
    st.frames = {1: f, 3: np.concatenate([f, g, f])}          # batch 3: tiles straddle frames
    st.region = [orclib.forward_i16(st.model, fr[0])[0].reshape(425, 13, 13) for fr in (f, g)]
    st.forced, st.tuned = _load(st.model), _load(st.model)
    st.launches = i16plans.launches_from_counts(st.tuned.layer_path_counts(), i16plans.splitk_proved(st.model))
    for o, L in WATCHED.items():      # what the model is designed for: every block of a watched conv form D, the split proved
        la = st.launches[(L, 0)]
        assert (la.path, la.n_launches, la.splitk_ok) == (4, 1, True), (o, la)
    lists = {key: ([sh for _, sh in i16plans.candidates(la, SWEEP_BATCH) if i16plans.legal(la, SWEEP_BATCH, sh)] if key[0] in WATCHED.values()
                   else [ONE_PIXEL]) for key, la in st.launches.items()}
    assert max(len(v) for v in lists.values()) <= N_SWEEP
    print(f"[i16 adversarial] tuner candidates: {sum(len(lists[(L, 0)]) for L in WATCHED.values())} (layer, shape) pairs over the watched layers")
    st.sweep = i16plans.pack(lists, st.launches, SWEEP_BATCH, tmp_path_factory.mktemp("i16adv"), "adv", count=N_SWEEP)
    yield st
    st.forced.close()
    st.tuned.close()


def _check_chains(st, ctx, batch, what, model=None, info=None, designed=None, want=None, region=None):
    """Every watched conv of every frame: the observed input is the designed one, the output the oracle's conv of it (the pool's
    tensor too behind conv 12), and the region tensor the whole-network oracle's."""
    info, designed, want = info or st.info, designed or st.designed, want or st.want
    got_region, _ = ctx.run_batch_host(st.frames[batch])
    fused = ctx.pool_fused_layers()
    for o in info:
        l = net.CONVS[o]
        print(f"[i16 adversarial] {what} batch {batch}: conv {o} (layer {l.idx}) ran [{ctx.conv_plan(o)}]")
        for f in range(batch):
            x = ctx.debug_layer_output(l.idx - 1, f)
            assert np.array_equal(x[:, :, :l.w], designed[o][:, :, :l.w]), (what, o, f, "the watched conv did not see the designed constants")
            check = [l.idx + 1] if l.idx + 1 in want else []
            if l.idx not in fused or l.idx == 16:      # (conv + pool as one kernel writes only the pool's tensor, except layer 16's, which is routed)
                check.insert(0, l.idx)
            for i in check:
                y, ow = ctx.debug_layer_output(i, f), net.LAYERS[i].out_w
                assert np.array_equal(y[:, :, :ow], want[i][:, :, :ow]), \
                    f"{what}: batch {batch} frame {f} layer {i} [{ctx.conv_plan(o)}]: {_first_diff(y, want[i], ow)}"
    region = region or st.region
    for f in range(batch):
        assert np.array_equal(got_region[f], region[f % 2]), (what, batch, f, "region tensor")


def _legal(st, o, batch, sh):
    return i16plans.legal(st.launches[(WATCHED[o], 0)], batch, sh)


# name: (options, expectation per watched conv: (state, conv ordinal, batch) -> {plan field: value}, the field that must be set on some conv)
def _expect_ks(ks):
    return lambda st, o, B: {"ks": ks if _legal(st, o, B, Shape(1, 0, 0, 1, 0, 0, 0, ks)) else 0, "P": 1, "splitk": 0}


def _expect_w16(P):
    return lambda st, o, B: {"w16": 1, "P": P, "form": 4} if _legal(st, o, B, Shape(P, 0, 0, 1, 1, 0, 0, 0)) else {"w16": 0}


def _expect_hiacc(P):
    return lambda st, o, B: {"hiacc": 1, "P": P, "form": 4, "w16": 0, "splitk": 0, "ks": 0} if _legal(st, o, B, Shape(P, 0, 0, 1, 0, 0, 1, 0)) else {"hiacc": 0}


FORCED_CASES = {
    **{f"ks{k}": ({"force_p": 1, "force_ks": k}, _expect_ks(k), "ks") for k in (2, 4, 8, 16)},
    **{f"w16_p{P}": ({"force_p": P, "force_w16": 1}, _expect_w16(P), "w16") for P in (1, 2)},
    **{f"hiacc_p{P}": ({"force_p": P, "force_hiacc": 1}, _expect_hiacc(P), "hiacc") for P in (1, 2, 4)},
    # (the expectations of these three are exact: no "took" field)
    "poolfuse": ({"force_p": 1, "poolfuse": 1}, lambda st, o, B: {"fused": 2} if o == 12 else {"fused": 0}, None),
    "grp16": ({"force_p": 1, "grp16": 1}, lambda st, o, B: {"grp": 16 if net.CONVS[o].size == 1 else 1}, None),
    "edge_tiles": ({"force_p": 1}, lambda st, o, B: {"edge": int(net.CONVS[o].size == 3), "P": 1, "hiacc": 0, "w16": 0, "ks": 0}, None),
    "raster_tiles": ({"force_p": 1, "no_edge_tiles": 1}, lambda st, o, B: {"edge": 0, "P": 1, "hiacc": 0, "w16": 0, "ks": 0}, None),
}


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", list(FORCED_CASES))
def test_chains_forced_shape(name, batch, chain):
    """The launch shapes the force_* hooks reach: each asserted from conv_plan, so that a case that did not take fails."""
    opts, expect, took = FORCED_CASES[name]
    st, ctx = chain, chain.forced
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_batch(batch)
        assert ctx.plan_source() == "forced by a test hook"
        plans = {o: i16plans.plan_fields(ctx.conv_plan(o)) for o in WATCHED}
        for o, got in plans.items():
            want = expect(st, o, batch)
            assert {k: got[k] for k in want} == want, (name, o, got)
        assert took is None or any(p[took] for p in plans.values()), (name, plans)
        _check_chains(st, ctx, batch, name)
    finally:
        for k in opts:
            ctx.set_option(k, None)


TUNED_CASES = {
    "default": {},
    "splitk": {"splitk": 1, "no_poolfuse": 1},
    "splitk_no_pack": {"splitk": 1, "splitk_no_pack": 1, "no_poolfuse": 1},
}


def _assert_lane_split(plans, pack):
    for o, p in plans.items():
        K = net.CONVS[o].size
        assert p["splitk"] in ((4,) if K == 3 else (4, 8)) and p["P"] == 1 and p["fused"] == 0 and p["pack"] == pack(p), (o, p)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", list(TUNED_CASES))
def test_chains_tuned_shape(name, batch, chain):
    """The default plan, and the lane-split kernel wherever it is legal: packed int16 triples on these form D layers (`a` wraps and is
    recovered from l and h), and the unpacked int32 triples with splitk_no_pack."""
    st, ctx, opts = chain, chain.tuned, TUNED_CASES[name]
    try:
        ctx.set_option("plan_file", None)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_batch(batch)
        plans = {o: i16plans.plan_fields(ctx.conv_plan(o)) for o in WATCHED}
        assert all(p["form"] == 4 and p["extra"] == 0 for p in plans.values()), plans
        if name != "default":
            assert ctx.plan_source() == "autotuned in this process"
            _assert_lane_split(plans, (lambda p: 1) if name == "splitk" else (lambda p: 0))
        _check_chains(st, ctx, batch, f"{name} ({ctx.plan_source()})")
    finally:
        for k in opts:
            ctx.set_option(k, None)


def test_chains_lane_split_int32_triples(chain):
    """force_path=0: every launch form A, so the lane-split kernel carries int32 triples (a, l, h) through the same chains."""
    st = chain
    ctx = _load(st.model, {"force_path": 0, "splitk": 1, "no_poolfuse": 1})
    try:
        for batch in (1, 3):
            ctx.set_batch(batch)
            plans = {o: i16plans.plan_fields(ctx.conv_plan(o)) for o in WATCHED}
            assert all(p["form"] == 0 and p["extra"] == 0 for p in plans.values()), plans
            _assert_lane_split(plans, lambda p: 0)
            _check_chains(st, ctx, batch, "splitk, force_path=0")
    finally:
        ctx.close()


@pytest.mark.parametrize("k", range(N_SWEEP))
def test_chains_tuner_candidate(k, chain):
    """File k gives every launch of the four watched layers the k-th of the candidates autotune enumerates for it and plan_conv
    accepts (S = 4 and 8, 2 and 4 pixels per lane, every tile shape and occupancy cap, w16, hiacc, the K-split, conv + pool), all
    other layers a one-pixel tile; the file must be taken as it stands."""
    st, ctx = chain, chain.tuned
    fname, chosen = st.sweep[k]
    ctx.set_option("plan_file", fname)
    try:
        ctx.set_batch(SWEEP_BATCH)
        assert ctx.plan_source() == "plan table", (ctx.plan_source(), open(fname).read())
        for o, L in WATCHED.items():
            want = i16plans.expected_plan(st.launches[(L, 0)], chosen[(L, 0)])
            got = i16plans.plan_fields(ctx.conv_plan(o))
            assert {f: got[f] for f in want} == want and got["form"] == 4, (L, chosen[(L, 0)], got)
        _check_chains(st, ctx, SWEEP_BATCH, f"candidate file {k}")
    finally:
        ctx.set_option("plan_file", None)


# ---- the unpacked lane split at its own limit

def _split_rule(M, so, steps):
    """The rule written above splitk_ok (csrc/yolo2_int16.hip): every increment below 2^29, the unclamped sum of one split below 2^30."""
    tmax = (M * 32768 + ((1 << (so - 1)) if so > 0 else 0)) >> so
    return tmax < (1 << 29) and tmax * steps < (1 << 30)


def _chain_case(case, weight_q=None):
    st = _State()
    st.model, st.info = i16adv.chain_model(3, cases=(case,), weight_q=weight_q)
    st.designed, st.want = _oracle_watched(st.model, st.info)
    f = synth.frames(11, 1)
    st.frames = {1: f}
    st.region = [orclib.forward_i16(st.model, f[0])[0].reshape(425, 13, 13)]
    return st


@pytest.mark.parametrize("over", [0, 1])
def test_unpacked_lane_split_at_its_limit(over):
    """Conv 14 (1x1, 1024 channels, S = 8) with output shift 2 and inputs all 32767: every increment of a sub-chain has one sign and
    is (M * 32768 + 2) >> 2.  M* is the largest quad sum for which the split's rule holds; bits equal the oracle at M* (the split
    kernel must run) and at M* + 1 (whatever runs)."""
    l = net.CONVS[14]
    so, steps = 2, (l.c // 4 // 4 + 1) * l.size * l.size
    m_star = max(M for M in range(1, 4096) if _split_rule(M, so, steps))
    assert _split_rule(m_star, so, steps) and not _split_rule(m_star + 1, so, steps) and m_star == 2016
    wq = [synth.STD_Q["weight_q"]] * len(net.CONVS)
    wq[14] = so
    orclib.oracle().orc_set_threads(16)
    st = _chain_case(i16adv.Case(13, 14, M=m_star + over, driver_bias=(32767,)), weight_q=wq)
    assert st.info[14].so == so and set(st.info[14].consts.tolist()) == {32767}
    assert i16plans.splitk_proved(st.model)[14] == (not over)
    ctx = _load(st.model, {"splitk": 1, "no_poolfuse": 1})
    try:
        ctx.set_batch(1)
        p = i16plans.plan_fields(ctx.conv_plan(14))
        print(f"[i16 adversarial] unpacked split, M = {m_star + over} (M* = {m_star}): form {FORMS[p['form']]}, split kernel {'ran' if p['splitk'] else 'did not run'} [{ctx.conv_plan(14)}]")
        assert p["pack"] == 0 and p["form"] in (0, 1)
        if not over:
            assert p["splitk"] in (4, 8), p
        _check_chains(st, ctx, 1, f"unpacked split at M* + {over}")
    finally:
        ctx.close()


@pytest.mark.parametrize("over", [0, 1])
def test_form_d_limit_one_register_per_channel(over):
    """force_hiacc acts only on contexts planned with force_p: conv 10 of a chain model whose every quad holds sum |w| = M*, form D's
    limit as the driver tier states it for these Q values, run with one accumulator register per channel; at M* + 1 the loader
    must have left form D."""
    q = i16adv.layer_q(14, 3)
    limits = _limits(3, q, "zero")
    m_star = [m for m, f, _ in limits if f == 4]
    assert len(m_star) == 1, limits
    orclib.oracle().orc_set_threads(16)
    st = _chain_case(i16adv.Case(9, 10, M=m_star[0] + over))
    ctx = _load(st.model, {"force_p": 1, "force_hiacc": 1})
    try:
        if over:
            assert ctx.layer_paths()[10] != 4, "the crafted model's form D limit is not the driver tier's"
            return
        ctx.set_batch(1)
        p = i16plans.plan_fields(ctx.conv_plan(10))
        assert (p["form"], p["hiacc"], p["extra"]) == (4, 1, 0), p
        _check_chains(st, ctx, 1, f"form D limit M = {m_star[0]}, hiacc")
    finally:
        ctx.close()
