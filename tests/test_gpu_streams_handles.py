"""Stream ordering of the handles: ``RaftEngine.refine`` (every way its launches reach a stream: plain, under capture, as a replayed
graph; on the caller's stream, on the private stream that stands in for the null stream, on the engine's forked side stream),
``RaftEngine.prepare_frame``, ``EncoderEngine.forward`` and ``RaftEngine.nonfinite_snapshot``.

The technique is tests/stream_harness.py's: the calling stream is kept busy by a bounded spin, the call's input tensors are rewritten
in place behind the spin (so addresses, and with them graph keys, repeat), the call is made, a copy of its outputs is enqueued behind
it on the same stream and an event recorded; after that event alone both the outputs and the copy are the bits a SECOND handle with
the same options gives for the same inputs where no race is possible.  The reference runs after the stalled calls, and every stalled
call's input set differs from the one before it, so bytes left over from an earlier call are never the expected answer.

On the null stream the spin, the rewrite and the copy are all on the null stream: exactly what ``StreamProxy::enter`` and ``leave``
(mft_amd/csrc/graph_cache.h) have to order the private stream against.
"""
import numpy as np
import pytest
import torch

import refine_reference as rr
import stream_harness as sh
import test_gpu_refine_family as rf

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = 2
SCHEDULES = ("default", "tile_conv 2", "fuse_flow 0 fork -1", "all apart", "ondemand_corr", "fp32 group 1", "lists prepared")
SHAPES = ((1, 16, 16), (2, 17, 23))
KINDS = ("rand", "hot", "same")          # input set i of the stalled calls; the warm-up runs on "zero"
STREAMS = ("null", "side", "alternating")


@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


@pytest.fixture(scope="module")
def cycles_per_ms():
    return sh.calibrate()


_ENGINES = {}


def engines(ops, name):
    """(the engine that is stalled, the reference engine) of a schedule: two instances with the same options, a workspace each."""
    if name not in _ENGINES:
        arith, options, ondemand, _ = rf.SCHEDULES[name]
        sd = {k: v.to(DEV) for k, v in rr.weights().items()}
        make = lambda: ops.RaftEngine(sd, DEV, ondemand_corr=ondemand, arith=ops.ARITH_SPLIT if arith == rf.SPLIT else ops.ARITH_F32,      # noqa: E731
                                      options=dict(options))
        _ENGINES[name] = (make(), make())     # (split_weights(check_range=True) inside construction waits for the host: not stalled)
    return _ENGINES[name]


def streams_of(mode, n, cycles_per_ms):
    """The calling stream of each of n calls.  Side streams are probed first (stream_harness.visible_stream): work that the product
    wrongly put on the null stream, or on the other side stream, would not be serialised with them by a shared hardware queue."""
    if mode == "null":
        return [torch.cuda.default_stream()] * n
    a = sh.visible_stream(cycles_per_ms)
    if mode == "side":
        return [a] * n
    b = sh.visible_stream(cycles_per_ms, against=(a,))
    return [(a, b)[i % 2] for i in range(n)]


def device_sets(case_shape, kinds):
    return [{k: v.to(DEV) for k, v in rr.inputs(rr.Case(*case_shape, kind, None)).items() if v is not None} for kind in kinds]


def rewrite(buf, new):
    for k in buf:
        buf[k].copy_(new[k], non_blocking=True)


def stalled_calls(call, buf, sets, streams, cycles_per_ms, warm, what):
    """The warm-up sequence (unstalled, on `warm`, one call per stream of the stalled sequence, each timed), then `reset()` by the
    caller, then this: per input set, a stall on the call's stream, the rewrite, the call, the same-stream copy, an event; the outputs
    are read after the event alone.  -> [(outputs, copies)] as CPU bit views."""
    got = []
    for i, (new, s, host) in enumerate(zip(sets, streams, warm)):
        ms = sh.stall_ms(host)
        end = sh.stall(s, ms, cycles_per_ms)
        with torch.cuda.stream(s):
            rewrite(buf, new)
            outs = call(buf)
            behind = sh.enqueued_behind(end)             # immediately after the product call returned
            snap = [o.clone() for o in outs]
            done = torch.cuda.Event()
            done.record(s)
        done.synchronize()                               # the event only
        got.append((sh.host_copies(outs), sh.host_copies(snap)))
        print(f"{what} call {i}: warm-up took {1e3 * host:.2f} ms on the host, stalled for {ms:.0f} ms, enqueued behind the stall: {behind}")
        assert behind, f"{what} call {i}: the stall of {ms:.0f} ms had ended when the call returned: nothing is proven"
    return got


def warm_up(call, buf, zero, streams):
    """One unstalled call per stream of the sequence on the "zero" inputs -> the host seconds each took (plain launch, capture and
    replay differ).  Leaves every stream idle."""
    torch.cuda.synchronize()
    host = []
    for s in streams:
        with torch.cuda.stream(s):
            rewrite(buf, zero)
            _, t = sh.timed(lambda: call(buf))
        s.synchronize()
        host.append(t)
    torch.cuda.synchronize()
    return host


def assert_same(got, want, what):
    for i, ((outs, snap), ref) in enumerate(zip(got, want)):
        for j, (o, c, r) in enumerate(zip(outs, snap, ref)):
            assert o.shape == r.shape and o.dtype == r.dtype, (what, i, j)
            assert torch.equal(o, r), (f"{what} call {i} output {j}: {int((o != r).sum())} of {r.numel()} elements differ from the reference "
                                       "engine: the call, or part of it, ran elsewhere or too early")
            assert torch.equal(c, r), (f"{what} call {i} output {j}: the same-stream copy differs in {int((c != r).sum())} elements: the result "
                                       "was not ordered in front of the stream's next work")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", STREAMS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", SCHEDULES)
def test_refine_is_ordered(ops, cycles_per_ms, name, shape, mode):
    P, h, w = shape
    case = rr.Case(P, h, w, "rand", None)
    eng, ref = engines(ops, name)
    plan = rf.plan_of(eng, name, P, h, w)
    # a graph is keyed by its stream (mft_amd/csrc/raft_engine.hip: GraphKey), so each of two alternating streams needs its own plain launch,
    # capture and replay: six calls there, three otherwise
    sets = device_sets(shape, KINDS) * (2 if mode == "alternating" else 1)
    zero = device_sets(shape, ("zero",))[0]
    buf = {k: v.clone() for k, v in zero.items()}
    streams = streams_of(mode, len(sets), cycles_per_ms)
    # (without flow_lr: its address is part of the graph key, and the outputs of every stalled call are kept until they are compared;
    # "lists prepared": prepare_frame, then refine)
    call = lambda d: list(rf.run(eng, name, dict(d, flow_init=None), case, ITERS, want_flow_lr=False))      # noqa: E731
    warm = warm_up(call, buf, zero, streams)
    ops.check(ops._lib.load().mftx_raft_clear_graphs(eng._h), "mftx_raft_clear_graphs")    # the stalled calls start over: plain, capture, replay
    torch.cuda.synchronize()
    c0, r0 = eng.graph_stats()
    got = stalled_calls(call, buf, sets, streams, cycles_per_ms, warm, f"{name} {shape} {mode}")
    torch.cuda.synchronize()
    c1, r1 = eng.graph_stats()
    print(f"{name} {shape} {mode}: {c1 - c0} graphs captured and {r1 - r0} replayed in the stalled calls")
    if plan["use_graph"]:
        assert c1 - c0 >= 1 and r1 - r0 >= 1, f"{name}: {c1 - c0} captures and {r1 - r0} replays in the stalled calls, expected one of each at least"
    else:
        assert (c1, r1) == (c0, r0)
    want = []
    for d in sets:
        want.append(sh.host_copies(rf.run(ref, name, dict(d, flow_init=None), case, ITERS, want_flow_lr=False)))
        torch.cuda.synchronize()
    assert not all(torch.equal(a, b) for a, b in zip(want[0], want[1])) and not all(torch.equal(a, b) for a, b in zip(want[1], want[2]))
    assert_same(got, want, f"{name} {shape} {mode}")
    torch.cuda.synchronize()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", STREAMS)
@pytest.mark.parametrize("planar", [True, False])
def test_refine_packed_output_is_ordered(ops, cycles_per_ms, mode, planar):
    """The packed [P, H0, W0, 4] output beside the planar ones, and alone (planar=False): behind a stall it holds the reference engine's
    planes, interleaved (as tests/test_gpu_kernels.py::test_convex_upsample_packed_equals_planar states it)."""
    shape = (2, 17, 23)
    P, h, w = shape
    eng, ref = engines(ops, "default")
    sets = device_sets(shape, KINDS)
    zero = device_sets(shape, ("zero",))[0]
    buf = {k: v.clone() for k, v in zero.items()}
    streams = streams_of(mode, len(sets), cycles_per_ms)
    packed = torch.zeros(P, 8 * h, 8 * w, 4, device=DEV)

    def call(d):
        outs = eng.refine(d["f1"], d["f2"], d["net"], d["inp"], h, w, ITERS, packed=packed, planar=planar)
        return [packed] + ([o for o in outs] if planar else [])

    warm = warm_up(call, buf, zero, streams)
    ops.check(ops._lib.load().mftx_raft_clear_graphs(eng._h), "mftx_raft_clear_graphs")
    torch.cuda.synchronize()
    got = stalled_calls(call, buf, sets, streams, cycles_per_ms, warm, f"packed planar={planar} {mode}")
    torch.cuda.synchronize()
    want = []
    for d in sets:
        flow, occl, sigma = ref.refine(d["f1"], d["f2"], d["net"], d["inp"], h, w, ITERS)
        pk = torch.cat([flow, occl, sigma], 1).permute(0, 2, 3, 1).contiguous()
        want.append(sh.host_copies([pk] + ([flow, occl, sigma] if planar else [])))
        torch.cuda.synchronize()
    assert_same(got, want, f"packed planar={planar} {mode}")
    torch.cuda.synchronize()


# ---- negative control -----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_harness_sees_a_planted_ordering_bug(ops, cycles_per_ms):
    """The negative control of this file: ``ops.copy_bytes`` called under another stream than the current one is reported, with a
    probed side stream stalled and the null stream or a side stream as the other one -- and with the NULL stream stalled and a side
    stream as the other one, the direction in which a missing ``StreamProxy::leave`` wait shows.  If not, the tests here prove nothing."""
    side = sh.visible_stream(cycles_per_ms)
    pairs = [(side, torch.cuda.default_stream()), (side, torch.cuda.Stream()), (torch.cuda.default_stream(), side)]
    for stalled, other in pairs:
        assert sh.planted_bug_is_seen(stalled, other, cycles_per_ms, copy=ops.copy_bytes, n=125 * 187 + 3), \
            "the harness is blind in this process: a copy made on another stream, in front of the rewrite of its source, was not seen"
    torch.cuda.synchronize()


# ---- encoders ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ("null", "side"))
@pytest.mark.parametrize("size", [(128, 136), (125, 187)], ids=str)
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("prefix", ["fnet", "cnet"])
def test_encoder_forward_is_ordered(ops, cycles_per_ms, prefix, graph, size, mode):
    H, W = size
    sd = {k: v.to(DEV) for k, v in rr.weights().items()}
    # three instances: one is warmed (unstalled: its host times size the stalls), one is stalled from its first call on -- so the plain
    # launch, the capture and the first replay of its graph are all enqueued behind a stall -- and one is the reference
    warm_enc, enc, ref = (ops.EncoderEngine(sd, prefix, prefix == "fnet", DEV, graph=graph) for _ in range(3))
    rng = np.random.default_rng([H, W, int(graph), int(prefix == "fnet"), STREAMS.index(mode)])
    imgs = [{"img": torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)} for _ in range(4)]
    zero, sets = imgs[0], imgs[1:]
    buf = {"img": zero["img"].clone()}
    streams = streams_of(mode, len(sets), cycles_per_ms)
    call = lambda d: [o for o in enc.forward(d["img"]) if o is not None]      # noqa: E731
    warm = warm_up(lambda d: [o for o in warm_enc.forward(d["img"]) if o is not None], buf, zero, streams)
    enc._ws = torch.empty_like(warm_enc._ws)                  # (the workspace, allocated before anything is stalled)
    torch.cuda.synchronize()
    got = stalled_calls(call, buf, sets, streams, cycles_per_ms, warm, f"{prefix} graph={graph} {size} {mode}")
    torch.cuda.synchronize()
    want = []
    for d in sets:
        want.append(sh.host_copies([o for o in ref.forward(d["img"]) if o is not None]))
        torch.cuda.synchronize()
    assert not torch.equal(want[0][0], want[1][0])
    assert_same(got, want, f"{prefix} graph={graph} {size} {mode}")
    torch.cuda.synchronize()


# ---- the non-finite snapshot --------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ("null", "side"))
def test_nonfinite_snapshot_carries_its_own_call(ops, cycles_per_ms, mode):
    """Behind a stalled refinement on inputs that produce NaN (one NaN in net, the recipe of
    tests/test_gpu_refine_family.py::test_nonfinite_input_stays_in_its_pair), the pinned word read after the event carries the count of
    THAT call; behind a stalled clean call it carries 0, and the first word still holds what it held."""
    shape = (2, 17, 23)
    P, h, w = shape
    eng, ref = engines(ops, "default")
    clean, other = device_sets(shape, ("rand", "hot"))
    bad = dict(other, net=other["net"].clone())
    bad["net"][0, (h // 2) * w + w // 2, 5] = float("nan")
    zero = device_sets(shape, ("zero",))[0]
    buf = {k: v.clone() for k, v in zero.items()}
    words = [torch.full((4,), -1, dtype=torch.int32).pin_memory() for _ in range(2)]
    s = streams_of(mode, 1, cycles_per_ms)[0]
    state = {"words": words[0]}

    def call(d):
        outs = list(eng.refine(d["f1"], d["f2"], d["net"], d["inp"], h, w, ITERS))
        eng.nonfinite_snapshot(state["words"])
        return outs

    eng.nonfinite_count(reset=True)                      # (reads the counter back: waits for the host by contract, before any stall)
    scratch = torch.full((4,), -1, dtype=torch.int32).pin_memory()
    state["words"] = scratch
    warm = warm_up(call, buf, zero, [s])
    assert int(scratch[0]) == 0
    state["words"] = words[0]
    got_bad = stalled_calls(call, buf, [bad], [s], cycles_per_ms, warm, f"nonfinite {mode}")
    n_bad = int(words[0][0])                             # after the event behind the snapshot: no other wait
    torch.cuda.synchronize()
    assert eng.nonfinite_count(reset=True) == n_bad      # (host wait by contract; the counter is zero again)
    state["words"] = words[1]
    got_clean = stalled_calls(call, buf, [clean], [s], cycles_per_ms, warm, f"nonfinite, clean {mode}")
    n_clean = int(words[1][0])
    torch.cuda.synchronize()
    ref.nonfinite_count(reset=True)
    want_bad = sh.host_copies(ref.refine(bad["f1"], bad["f2"], bad["net"], bad["inp"], h, w, ITERS))
    want_n = ref.nonfinite_count(reset=True)             # (host wait by contract)
    want_clean = sh.host_copies(ref.refine(clean["f1"], clean["f2"], clean["net"], clean["inp"], h, w, ITERS))
    assert ref.nonfinite_count() == 0
    assert want_n > 0 and n_bad == want_n, (n_bad, want_n)
    assert n_clean == 0 and int(words[0][0]) == want_n, (n_clean, int(words[0][0]))
    assert_same(got_bad, [want_bad], f"nonfinite {mode}")
    assert_same(got_clean, [want_clean], f"nonfinite, clean {mode}")
    torch.cuda.synchronize()
