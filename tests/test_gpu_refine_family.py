"""The refinement engine (``mftx_raft_refine``: motion encoder, both SepConvGRU passes, flow head, mask head, OU heads and the launch
schedule that strings them together) stage by stage against fp64, at small and odd sizes, on every schedule.

a. Free-running: 1, 2, 3 and 12 iterations of every case of tests/refine_reference.py; every workspace region that is valid after the
   call (REGION_MAP, the table in RaftEngine.region's docstring) and every output against the fp64 oracle's trace.
b. Teacher-forced single iterations from the fp64 state after iteration k - 1: the one-step error.
c. Every schedule (option set) at 3 iterations, each against fp64 -- after asserting on ``RaftEngine.plan`` that the schedule meant is
   the schedule run.
d. Graph replay, e. untouched memory, f. batch independence, g. non-finite input.

Bounds: error against fp64 <= K_MAX x the fp32 oracle's maximum error and <= K_MEAN x its mean error on the same case, per region
(8 and 4, the constants of tests/test_gpu_offgrid.py, set before the first run; 16 and 8 for ouh, the engine's longest sum, with the
fp32 MFMA arithmetic only, for the reason written at refine_reference.BOUNDS_FP32_ARITH); regions stored in split form may add the representation error SPLIT_REP |ref| + SPLIT_FLOOR.  tests/test_refine_reference.py shows on the CPU that another fp32 realisation of
the same mathematics stays within 8 and 4 on every case and iteration count (largest ratios 2.63 / 1.15) and that eleven seeded faults do not.  Observed ratios:
profiles/refine_noise.txt.

Needs an MI355X."""

import numpy as np
import pytest
import torch

import corr_reference as cr
import refine_reference as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT, F32 = "split", "fp32"


@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


# =====================================================================================================================
# schedules
# =====================================================================================================================
TILES = {"tile_conv": 2}
TILES_PLAN = dict(presplit=True, tiles_on=True, gru_fused=True, two_pass=True, flow="fused", head_fused=True, defer_update=True,
                  ou_fused=True, ou_materialised=False)
APART = {"fuse_lookup": 0, "fuse_flow": 0, "tile_conv": 0, "fuse_head": 0}


def _t(extra, **expect):
    return dict(TILES, **extra), dict(TILES_PLAN, **expect)


# name -> (arithmetic, options, ondemand_corr, the PLAN_FIELDS the schedule is known by).  (tile_cells and tile_volume are no plan
# fields: those schedules are known by their option and must otherwise be the schedule they vary.)
SCHEDULES = {
    "default": (SPLIT, {}, False, dict(presplit=True, fuse_lookup=True, flow="fused", use_graph=True)),
    "tile_conv 2": (SPLIT, TILES, False, dict(TILES_PLAN, fuse_lookup=True, use_graph=True)),
}


def _add(name, arith, options, expect, ondemand=False):
    SCHEDULES[name] = (arith, options, ondemand, expect)


_add("fuse_gru 0", SPLIT, *_t({"fuse_gru": 0}, gru_fused=False))
_add("fuse_head 0", SPLIT, *_t({"fuse_head": 0}, head_fused=False, defer_update=False))
_add("fuse_head 2", SPLIT, *_t({"fuse_head": 2}, head_fused=True, defer_update=False))
_add("fuse_ou 0", SPLIT, *_t({"fuse_ou": 0}, ou_fused=False, ou_materialised=True))
_add("fuse_ou 2", SPLIT, *_t({"fuse_ou": 2}, ou_fused=True, ou_materialised=True))
_add("tile_conv2p 0", SPLIT, *_t({"tile_conv2p": 0}, two_pass=False))
_add("tile_cells 64", SPLIT, *_t({"tile_cells": 64}))
_add("tile_cells 32", SPLIT, *_t({"tile_cells": 32}))
_add("fuse_flow 0 fork -1", SPLIT, *_t({"fuse_flow": 0, "fork": -1}, flow="side", defer_update=False, side_stream=True))
_add("fuse_flow 0 fork 0", SPLIT, *_t({"fuse_flow": 0, "fork": 0}, flow="after_lookup", defer_update=False, side_stream=False))
_add("fuse_flow 0 fork 2", SPLIT, *_t({"fuse_flow": 0, "fork": 2}, flow="first", defer_update=False))
_add("tile_conv 0", SPLIT, {"tile_conv": 0}, dict(presplit=True, tiles_on=False, gru_fused=False, two_pass=False, head_fused=False, ou_fused=False,
                                                  ou_materialised=True, flow="fused"))
_add("all apart", SPLIT, APART, dict(presplit=True, fuse_lookup=False, tiles_on=False, flow="side", head_fused=False, ou_fused=False))
_add("all apart presplit 0", SPLIT, dict(APART, presplit=0), dict(presplit=False, fuse_lookup=False, tiles_on=False, flow="side", head_fused=False))
_add("tile_volume 0", SPLIT, {"tile_volume": 0}, dict(presplit=True, fuse_lookup=True, flow="fused"))
_add("ondemand_corr", SPLIT, {}, dict(fuse_lookup=False, use_graph=False), ondemand=True)
_add("fp32 group 1", F32, {"group": 1}, dict(presplit=False, flow="with_lookup", pair_second=True, tiles_on=False, side_stream=False))
_add("fp32 group 0", F32, {"group": 0}, dict(presplit=False, flow="after_lookup", pair_second=False, tiles_on=False))
# per-pair map lists (mftx_raft_refine_gather), and lists with the left frames' prepared parts (mftx_raft_frame_prepare)
_add("lists", SPLIT, {}, dict(presplit=True, fuse_lookup=True, flow="fused", ctx_supplied=False))
_add("lists prepared", SPLIT, TILES, dict(TILES_PLAN, ctx_supplied=True))

# (schedule, shape) pairs a schedule cannot run at, with the reason.  Every kernel of every schedule is applicable at every shape of
# refine_reference.SHAPES (lookup_convc1_applicable only refuses batches whose byte offsets pass 2^31), so the table is empty; a
# plan that differs from the schedule meant fails the test instead of dropping the shape.
EXCLUDED = {}

_ENGINES = {}


def engine(ops, name):
    """One engine per schedule for the module (an engine owns its workspace and its captured graphs)."""
    if name not in _ENGINES:
        arith, options, ondemand, _ = SCHEDULES[name]
        sd = {k: v.to(DEV) for k, v in rr.weights().items()}
        _ENGINES[name] = ops.RaftEngine(sd, DEV, ondemand_corr=ondemand, arith=ops.ARITH_SPLIT if arith == SPLIT else ops.ARITH_F32,
                                        options=options)
    return _ENGINES[name]


def plan_of(eng, name, P, h, w):
    """The plan of the call, checked against the fields the schedule is known by."""
    plan = eng.plan(P, h, w, ctx_supplied=(name == "lists prepared"))
    assert set(plan) == set(eng.PLAN_FIELDS)
    want = SCHEDULES[name][3]
    assert {k: plan[k] for k in want} == want, (name, (P, h, w), plan)
    return plan


# =====================================================================================================================
# running the engine and reading it back
# =====================================================================================================================
def to_dev(data):
    return {k: (v.to(DEV) if v is not None else None) for k, v in data.items()}


def run(eng, name, d, case, iters, want_flow_lr=True):
    """One refine of a case's device tensors on a schedule's engine -> (flow, occl, sigma, flow_lr)."""
    P, h, w = case.P, case.h, case.w
    if not name.startswith("lists"):
        return eng.refine(d["f1"], d["f2"], d["net"], d["inp"], h, w, iters, want_flow_lr=want_flow_lr, flow_init=d["flow_init"])
    assert eng.can_gather(P)
    lists = [[d[k][p] for p in range(P)] for k in ("f1", "f2", "net", "inp")]
    prepared = None
    if name == "lists prepared":
        parts = [eng.prepare_frame(d["f1"][p], d["inp"][p], h, w, context=True, split=True) for p in range(P)]
        prepared = {"ctx": [c for c, _ in parts], "f1s": [s for _, s in parts], "f2s": None}
    return eng.refine(*lists, h, w, iters, want_flow_lr=want_flow_lr, flow_init=d["flow_init"], prepared=prepared)


def read_back(eng, plan, P, h, w, outs):
    """Every region of REGION_MAP that is valid on `plan`, and the outputs -> {name: CPU tensor}."""
    got, rows = {}, {}
    sp = plan["presplit"]
    for name in rr.valid_regions(plan):
        r = rr.REGION_MAP[name]
        if r.region is None:
            got[name] = (outs[3] if len(outs) > 3 else eng.region("flow_lr", P, h, w, 2)).reshape(-1, 2).cpu()
            continue
        if r.region not in rows:
            width = rr.ROW_WIDTH.get(r.region, r.hi)
            rows[r.region] = eng.region(r.region, P, h, w, width, split=sp if r.region == "fh" else None).cpu()
        got[name] = rows[r.region][:, r.lo:r.hi]
    got.update({k: outs[i].cpu() for i, k in enumerate(rr.OUTPUTS)})
    return got


def hold(tag, got, r32, r64, plan, inp, fails, eng):
    """Every tensor of `got` against the fp64 run with the fp32 run's noise; one line per region; failures appended.  eng: the engine
    the tensors come from (its arithmetic decides the one raised bound, refine_reference.BOUNDS_FP32_ARITH)."""
    from mft_amd.ops import ARITH_F32
    a, b = rr.region_tensors(r32), rr.region_tensors(r64)
    sp = plan["presplit"]
    fp32 = eng.arith == ARITH_F32
    for name, t in got.items():
        if name == "inp":
            if not rr.inp_bits_ok(t, inp.cpu(), sp):
                fails.append((tag, "inp", "not the caller's bits"))
            continue
        split = name in rr.REGION_MAP and rr.REGION_MAP[name].split and sp
        stats = rr.compare(t, a[name], b[name], split_region=split)
        print(rr.line(tag, name, stats, *rr.bound(name, fp32)))
        if not rr.within(stats, *rr.bound(name, fp32)):
            fails.append((tag, name) + stats)


def same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)) for k in a)


# =====================================================================================================================
# a. free-running, stage by stage
# =====================================================================================================================
FREE = ("default", "tile_conv 2", "fp32 group 1")          # both arithmetics; the split one with ring-buffered and with tile-resident GEMMs


@pytest.mark.parametrize("iters", rr.ITERS)
@pytest.mark.parametrize("case", rr.CASES, ids=str)
def test_free_running_stage_by_stage(ops, case, iters):
    """Iterations 2 and 3 matter: the pending update and the ping-pong buffers exist from the second iteration on."""
    r32, r64 = rr.reference(case, iters)
    d = to_dev(rr.inputs(case))
    fails = []
    for name in FREE:
        eng = engine(ops, name)
        plan = plan_of(eng, name, case.P, case.h, case.w)
        outs = run(eng, name, d, case, iters)
        got = read_back(eng, plan, case.P, case.h, case.w, outs)
        assert set(rr.ALWAYS_VALID) <= set(got) and set(rr.OUTPUTS) <= set(got)
        hold(f"free {case} iters {iters:2d} [{name}]", got, r32, r64, plan, d["inp"], fails, eng)
    assert not fails, fails


def test_free_running_other_weights(ops, weights_np):
    """The same on the suite's other seeded weights (the weights_np fixture)."""
    case, iters = rr.Case(2, 17, 23, "rand", "quarter"), 3
    sd = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    r32, r64 = (rr.run_oracle(sd, rr.inputs(case), case.P, case.h, case.w, iters, dt) for dt in (torch.float32, torch.float64))
    d = to_dev(rr.inputs(case))
    fails = []
    for arith, options in ((ops.ARITH_SPLIT, {}), (ops.ARITH_SPLIT, TILES), (ops.ARITH_F32, {})):
        eng = ops.RaftEngine({k: v.to(DEV) for k, v in sd.items()}, DEV, arith=arith, options=options)
        plan = eng.plan(case.P, case.h, case.w)
        outs = eng.refine(d["f1"], d["f2"], d["net"], d["inp"], case.h, case.w, iters, want_flow_lr=True, flow_init=d["flow_init"])
        hold(f"weights_np {case} iters {iters} [arith {arith} {options}]", read_back(eng, plan, case.P, case.h, case.w, outs), r32, r64, plan,
             d["inp"], fails, eng)
    assert not fails, fails


# =====================================================================================================================
# b. teacher-forced single iterations
# =====================================================================================================================
FORCED_CASES = [rr.Case(*s, "rand", None) for s in rr.VARIED]


@pytest.mark.parametrize("k", rr.FORCED_K)
@pytest.mark.parametrize("case", FORCED_CASES, ids=str)
def test_teacher_forced_single_iteration(ops, case, k):
    """net (rounded to fp32) and flow_init = coords1 - grid from the fp64 run after iteration k - 1, one iteration: every region against
    fp64's iteration k, with the noise of the fp32 oracle started from the same state -- one update, no accumulated drift."""
    r32, r64 = rr.reference_forced(case, k)
    d = to_dev(rr.forced_state(case, k))
    fails = []
    for name in FREE:
        eng = engine(ops, name)
        plan = plan_of(eng, name, case.P, case.h, case.w)
        outs = run(eng, name, d, case, 1)
        hold(f"forced {case} k {k:2d} [{name}]", read_back(eng, plan, case.P, case.h, case.w, outs), r32, r64, plan, d["inp"], fails, eng)
    assert not fails, fails


# =====================================================================================================================
# c. every schedule
# =====================================================================================================================
@pytest.mark.parametrize("case", rr.CASES, ids=str)
def test_every_schedule_against_fp64(ops, case):
    """Each option set at 3 iterations against fp64 (not against another schedule: the bitwise cross-schedule tests of
    tests/test_gpu_kernels.py stay where they are), with the regions its plan materialises."""
    r32, r64 = rr.reference(case, 3)
    d = to_dev(rr.inputs(case))
    fails, checked = [], set()
    for name in SCHEDULES:
        if (name, (case.P, case.h, case.w)) in EXCLUDED:
            continue
        eng = engine(ops, name)
        plan = plan_of(eng, name, case.P, case.h, case.w)
        outs = run(eng, name, d, case, 3)
        got = read_back(eng, plan, case.P, case.h, case.w, outs)
        assert set(rr.ALWAYS_VALID) <= set(got) and set(rr.OUTPUTS) <= set(got)
        checked |= set(got)
        hold(f"schedule {case} [{name}]", got, r32, r64, plan, d["inp"], fails, eng)
    assert checked == set(rr.REGION_MAP) | set(rr.OUTPUTS), "a region of REGION_MAP no schedule materialises"
    assert not fails, fails


def test_schedule_table_is_complete():
    """Every schedule runs at every shape but the excluded ones, whose reasons are written down; each is left at least two shapes, one
    of them odd in both dimensions."""
    for name in SCHEDULES:
        left = [s for s in rr.SHAPES if (name, s) not in EXCLUDED]
        assert len(left) >= 2 and any(s[1] % 2 and s[2] % 2 for s in left), name
    for key, reason in EXCLUDED.items():
        assert key[0] in SCHEDULES and key[1] in rr.SHAPES and reason


def test_options_without_a_plan_field_reach_the_library(ops):
    """tile_cells and tile_volume are no plan fields, so plan_of cannot tell those schedules from the ones they vary.  That the library
    holds what was set shows in what it refuses on the host, before any kernel of the layer is launched: a tile size it has no
    kernel for (the tile-resident launchers check the option's value), and per-pair map lists without the tile-resident volume."""
    case = rr.Case(1, 16, 16, "rand", None)
    d = to_dev(rr.inputs(case))
    for name in ("tile_cells 64", "tile_cells 32"):
        base = engine(ops, name)
        assert base.plan(case.P, case.h, case.w) == engine(ops, "tile_conv 2").plan(case.P, case.h, case.w)
    eng = ops.RaftEngine({k: v.to(DEV) for k, v in rr.weights().items()}, DEV, options=dict(TILES, tile_cells=48))
    with pytest.raises(ops.MftxError, match="cells per tile"):
        run(eng, "tile_cells 48", d, case, 1)
    for cells in (64, 32):                                 # the same handle with a size it has: runs
        eng.set_option("tile_cells", cells)
        assert all(bool(torch.isfinite(t).all()) for t in run(eng, "tile_cells", d, case, 1))
    vol = engine(ops, "tile_volume 0")
    assert vol.plan(case.P, case.h, case.w) == engine(ops, "default").plan(case.P, case.h, case.w)
    assert engine(ops, "default").can_gather(case.P) and not vol.can_gather(case.P)
    lists = [[d[k][0]] for k in ("f1", "f2", "net", "inp")]
    vol._gather, vol._tile_volume = True, 1               # (past the Python-side guard: the refusal asserted is the library's)
    try:
        with pytest.raises(ops.MftxError, match="tile-resident correlation volume"):
            vol.refine(*lists, case.h, case.w, 1)
    finally:
        vol._tile_volume = 0


# =====================================================================================================================
# d. graph replay
# =====================================================================================================================
@pytest.mark.parametrize("name", ["default", "tile_conv 2"])
def test_graph_replay_same_bits(ops, name):
    """Four consecutive calls of one shape (plain launches, the capture, replays): outputs and all valid regions are the same bits;
    one capture and at least one launch of the graph.  Then another shape, then the first again on the same engine: the first bits."""
    assert SCHEDULES[name][0] == SPLIT and not SCHEDULES[name][2]
    eng = ops.RaftEngine({k: v.to(DEV) for k, v in rr.weights().items()}, DEV, options=SCHEDULES[name][1])      # (its own: no graph yet)
    case, other = rr.Case(2, 17, 23, "rand", "quarter"), rr.Case(1, 16, 16, "rand", None)
    d, do = to_dev(rr.inputs(case)), to_dev(rr.inputs(other))
    plan = plan_of(eng, name, case.P, case.h, case.w)
    assert plan["use_graph"] and eng.graph_stats() == (0, 0)

    def call():       # (no flow_lr output: its address is part of the graph's key, and every call would allocate another)
        outs = run(eng, name, d, case, 3, want_flow_lr=False)
        return read_back(eng, plan, case.P, case.h, case.w, outs)

    first = call()
    assert all(bool(torch.isfinite(v).all()) for v in first.values())
    for n in range(3):
        assert same_bits(call(), first), f"call {n + 2}"
    captures, launches = eng.graph_stats()
    assert captures == 1 and launches >= 1, (captures, launches)
    run(eng, name, do, other, 3, want_flow_lr=False)
    assert same_bits(call(), first), "after another shape"
    r32, r64 = rr.reference(case, 3)
    fails = []
    hold(f"graph {case} [{name}]", first, r32, r64, plan, d["inp"], fails, eng)
    assert not fails, fails


# =====================================================================================================================
# e. untouched memory
# =====================================================================================================================
GUARD = 64


@pytest.mark.parametrize("name", ["default", "tile_conv 2", "fp32 group 1"])
def test_untouched_memory(ops, name):
    """The workspace filled with NaN before the call, the five outputs in the middle of one buffer between canaries (the raw entry
    point: ops.refine allocates its own): every valid region and output finite and the bits of an ordinary call, canaries intact,
    hx[:, 128:256] still inp, the caller's maps unchanged."""
    from mft_amd import _lib
    case, iters = rr.Case(2, 17, 23, "rand", "quarter"), 3
    P, h, w = case.P, case.h, case.w
    eng = engine(ops, name)
    plan = plan_of(eng, name, P, h, w)
    d = to_dev(rr.inputs(case))
    keep = {k: v.clone() for k, v in d.items()}
    want = read_back(eng, plan, P, h, w, run(eng, name, d, case, iters))
    ws = eng.workspace(P, h, w)
    ws.fill_(0xFF)                                            # every word 0xFFFFFFFF: a NaN
    assert bool(torch.isnan(ws[: ws.numel() // 4 * 4].view(torch.float32)).all())
    sizes = [P * 2 * 64 * h * w, P * 64 * h * w, P * 64 * h * w, P * 64 * h * w * 4, P * h * w * 2]       # flow, occl, sigma, packed, flow_lr
    offs = np.cumsum([GUARD] + [s + GUARD for s in sizes])
    buf = torch.full((int(offs[-1]),), 7.5, device=DEV)
    views = [buf[int(o): int(o) + s] for o, s in zip(offs[:-1], sizes)]
    assert all(v.data_ptr() % 16 == 0 for v in views)
    _lib.check(_lib.load().mftx_raft_refine(eng._h, P, h, w, iters, d["f1"].data_ptr(), d["f2"].data_ptr(), d["net"].data_ptr(),
                                           d["inp"].data_ptr(), d["flow_init"].data_ptr(), 0, 0, 0, 0, *[v.data_ptr() for v in views],
                                           ws.data_ptr(), ws.numel(), ops._stream()), "mftx_raft_refine")
    torch.cuda.synchronize()
    outs = (views[0].view(P, 2, 8 * h, 8 * w), views[1].view(P, 1, 8 * h, 8 * w), views[2].view(P, 1, 8 * h, 8 * w), views[4].view(P, h * w, 2))
    got = read_back(eng, plan, P, h, w, outs)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    assert same_bits(got, want)
    packed = views[3].view(P, 8 * h, 8 * w, 4).cpu()
    assert torch.equal(packed[..., :2].permute(0, 3, 1, 2), got["flow"]) and torch.equal(packed[..., 2], got["occl"][:, 0]) \
        and torch.equal(packed[..., 3], got["sigma"][:, 0])
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for o, s in zip(offs[:-1], sizes):
        mask[int(o): int(o) + s] = False
    assert int(mask.sum()) == GUARD * 6 and bool((buf.cpu()[mask] == 7.5).all()), "canaries"
    assert rr.inp_bits_ok(got["inp"], d["inp"].cpu(), plan["presplit"])
    for k, v in d.items():
        assert torch.equal(v.view(torch.int32), keep[k].view(torch.int32)), k


# =====================================================================================================================
# f. batch independence
# =====================================================================================================================
@pytest.mark.parametrize("name", ["default", "tile_conv 2"])
def test_pair_bits_independent_of_batch_at_small_sizes(ops, name):
    """Pair p of a P = 3 call equals the P = 1 call on its maps, bit for bit, outputs and regions."""
    case = rr.Case(3, 24, 40, "rand", None)
    eng = engine(ops, name)
    d = to_dev(rr.inputs(case))
    N = case.h * case.w
    plan3, plan1 = plan_of(eng, name, 3, case.h, case.w), plan_of(eng, name, 1, case.h, case.w)
    assert plan3 == plan1
    all3 = read_back(eng, plan3, 3, case.h, case.w, run(eng, name, d, case, 3))
    for p in range(3):
        one = {k: (v[p:p + 1].contiguous() if v is not None else None) for k, v in d.items()}
        got = read_back(eng, plan1, 1, case.h, case.w, run(eng, name, one, case._replace(P=1), 3))
        part = {k: (v[p:p + 1] if k in rr.OUTPUTS else v[p * N:(p + 1) * N]) for k, v in all3.items()}
        for k in got:
            assert torch.equal(got[k].contiguous().view(torch.int32), part[k].contiguous().view(torch.int32)), (p, k)


# =====================================================================================================================
# g. non-finite input
# =====================================================================================================================
@pytest.mark.parametrize("name", ["default", "tile_conv 2", "fp32 group 1"])
def test_nonfinite_input_stays_in_its_pair(ops, name):
    """One NaN in net at one cell of pair 0: every output pixel of pair 1 keeps the bits of the clean run, the counter is above 0 and
    the NaN reaches pair 0's outputs (nothing masks it).  One +inf in flow_init: the lookups of that cell are NaN, the rule
    tests/corr_reference.py pins for non-finite coordinates (hostile_coords), and the call returns without error."""
    case = rr.Case(2, 17, 23, "rand", "quarter")
    P, h, w = case.P, case.h, case.w
    N = h * w
    eng = engine(ops, name)
    plan = plan_of(eng, name, P, h, w)
    d = to_dev(rr.inputs(case))
    eng.nonfinite_count(reset=True)
    clean = [t.cpu() for t in run(eng, name, d, case, 3)]
    assert eng.nonfinite_count() == 0 and all(bool(torch.isfinite(t).all()) for t in clean)
    cell = (h // 2) * w + w // 2
    bad = dict(d, net=d["net"].clone())
    bad["net"][0, cell, 5] = float("nan")
    outs = [t.cpu() for t in run(eng, name, bad, case, 3)]
    assert eng.nonfinite_count(reset=True) > 0
    for a, b in zip(outs, clean):
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "pair 1 changed"
    assert all(bool(torch.isnan(t[0]).any()) for t in outs[:3])
    # +inf in flow_init, pair 0: one iteration, so that `corr` holds the lookup at the coordinates given
    assert float("inf") in cr.HOSTILE_NONFINITE
    hot = dict(d, flow_init=d["flow_init"].clone())
    hot["flow_init"][0, cell, 0] = float("inf")
    outs = [t.cpu() for t in run(eng, name, hot, case, 1)]
    corr = eng.region("corr", P, h, w, 324).cpu()
    assert bool(torch.isnan(corr[cell]).all()), "a non-finite coordinate gives NaN lookups"
    others = torch.ones(P * N, dtype=torch.bool)
    others[cell] = False
    assert bool(torch.isfinite(corr[others]).all())
    clean1 = [t.cpu() for t in run(eng, name, d, case, 1)]
    for a, b in zip(outs, clean1):
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "pair 1 changed"
    assert eng.nonfinite_count(reset=True) > 0
