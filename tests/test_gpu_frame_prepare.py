"""A frame's share of its refinements computed once per frame (``mftx_raft_frame_prepare``): the context features' part of the GRU
gate sums and the split form of the feature map, handed to ``mftx_raft_refine_gather_ex`` instead of being recomputed in every pair.

A. The split map: ``mftx_split_weights`` (what the prepare call runs) equals the register split of the tile-resident volume kernel's
   query loads (``mftx_volume_query_split``: split8 itself) value for value -- also at the edges of the fp16 range.
B. The engine: ``refine`` with and without the prepared parts, bit for bit, before and after graph capture, with the pointers changing
   from call to call.
C. The tracker: 40 frames with ``frame_prepare`` on and off, bit for bit, ramp-up frames included, one and two frames in flight.

Needs an MI355X."""
import numpy as np
import pytest
import torch

from mft_amd.synth import SyntheticVideo

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# =====================================================================================================================
# A. the split map
# =====================================================================================================================

def test_prepared_split_map_equals_volume_register_split():
    """Every 8 floats -> [hi x 8 | lo x 8]: the standalone split kernel and split8 give the same 32 bytes for feature-like values,
    for values whose low half is subnormal or zero, for the largest operands of the split arithmetic, and for zeros of both signs."""
    from mft_amd import ops, _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    parts = [torch.randn(64 * 64 * 256, generator=g),                                   # a feature map's worth
             torch.randn(1 << 16, generator=g) * 1e-3, torch.randn(1 << 16, generator=g) * 1e-6, torch.randn(1 << 16, generator=g) * 1e-9,
             torch.randn(1 << 16, generator=g) * 3e4,
             torch.randn(1 << 16, generator=g).clamp(-1, 1) * 65503.0,
             torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12,
                           1.0 - 2.0 ** -12, 2049.0 / 2048.0, 6.1e-5, 5.9e-8, 3.0e-8] * 4)]
    # every fp16 value, and each with a small fp32 residual on either side
    halves = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.float16).float()
    halves = halves[torch.isfinite(halves)]
    halves = halves[: halves.numel() // 8 * 8]
    parts += [halves, halves * (1 + 2.0 ** -13), halves * (1 - 2.0 ** -13)]
    x = torch.cat(parts).cuda()
    assert x.numel() % 8 == 0 and bool(torch.isfinite(x).all())
    a, b = torch.empty_like(x), torch.empty_like(x)
    ops.check(lib.mftx_split_weights(x.data_ptr(), a.data_ptr(), x.numel(), None), "mftx_split_weights")
    ops.check(lib.mftx_volume_query_split(x.data_ptr(), b.data_ptr(), x.numel(), None), "mftx_volume_query_split")
    torch.cuda.synchronize()
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), (int(diff.sum()), x[(diff.nonzero()[:8, 0] // 8) * 8].tolist())
    # ... and the halves are what they are specified to be: hi = fp16(x), lo = fp16((x - hi) * 2048)
    h16 = a.view(torch.float16).reshape(-1, 2, 8)
    xr = x.reshape(-1, 8)
    hi = xr.to(torch.float16)
    lo = ((xr - hi.float()) * 2048.0).to(torch.float16)
    assert torch.equal(h16[:, 0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(h16[:, 1].view(torch.int16), lo.view(torch.int16))


def test_frame_prepare_split_map_is_the_split_weights_form():
    from mft_amd import ops
    eng, _ = _engine()
    g = torch.Generator().manual_seed(4)
    h, w = 33, 47
    fmap = torch.randn(h * w, 256, generator=g).cuda()
    ctx, fsplit = eng.prepare_frame(fmap, None, h, w, context=False)
    assert ctx is None
    want = torch.empty_like(fmap)
    from mft_amd import _lib
    ops.check(_lib.load().mftx_split_weights(fmap.data_ptr(), want.data_ptr(), fmap.numel(), None), "mftx_split_weights")
    assert torch.equal(_bits(fsplit), _bits(want))


# =====================================================================================================================
# B. the engine
# =====================================================================================================================

def _engine(options=None):
    from mft_amd import ops
    from mft_amd.weights import make_weights
    sd = {k: torch.from_numpy(v).cuda() for k, v in make_weights(7).items()}
    opts = {"tile_conv": 2}
    opts.update(options or {})
    return ops.RaftEngine(sd, "cuda", options=opts), sd


def _frame(g, h, w, like=None):
    f = torch.randn(h * w, 256, generator=g) if like is None else like.cpu() + 0.3 * torch.randn(h * w, 256, generator=g)
    return {"fmap": f.cuda(), "net": torch.tanh(torch.randn(h * w, 128, generator=g)).cuda(),
            "inp": torch.relu(torch.randn(h * w, 128, generator=g)).cuda()}


def _equal_outputs(a, b, what):
    for name, x, y in zip(("flow", "occl", "sigma", "packed"), a, b):
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(_bits(x), _bits(y)), (what, name, int((x != y).sum()))


# P = 1, 3, 7 at 64 x 64 cells, a ragged size, and a size with more gate tiles than CUs (as test_engine_fused_gru_bitwise)
@pytest.mark.parametrize("P,h,w", [(1, 64, 64), (3, 64, 64), (7, 64, 64), (2, 33, 47), (1, 135, 240)])
def test_engine_refine_with_prepared_parts_bitwise(P, h, w):
    """refine on per-pair map lists, with the left frames' context parts, their split maps and the right frame's split map supplied
    -- all of them, and each kind alone -- against the same call without: flow, occl, sigma and packed bit for bit.  Six rounds on one
    engine and one workspace: the first call of a key runs plain launches, the second captures the graph, later ones replay it; every
    round takes ANOTHER set of frames (other tensors at other addresses, other values), so a pointer frozen into the captured graph
    would read the previous round's parts and show."""
    eng, _ = _engine()
    ref, _ = _engine()
    g = torch.Generator().manual_seed(100 * P + h)
    H0, W0 = 8 * h, 8 * w
    iters = 3
    kinds = [("ctx", "f1s", "f2s"), ("ctx",), ("f1s",), ("f2s",), ("ctx", "f1s", "f2s"), ("ctx", "f1s", "f2s")]
    keep = []                                              # earlier rounds' tensors stay allocated: new rounds get new addresses
    for rnd, kind in enumerate(kinds):
        lefts = [_frame(g, h, w) for _ in range(P)]
        right = _frame(g, h, w, like=lefts[0]["fmap"])
        for f in lefts + [right]:
            f["ctx"], f["fsplit"] = eng.prepare_frame(f["fmap"], f["inp"], h, w)
        keep.append((lefts, right))
        maps = ([f["fmap"] for f in lefts], [right["fmap"]] * P, [f["net"] for f in lefts], [f["inp"] for f in lefts])
        prepared = {"ctx": [f["ctx"] for f in lefts] if "ctx" in kind else None,
                    "f1s": [f["fsplit"] for f in lefts] if "f1s" in kind else None,
                    "f2s": right["fsplit"] if "f2s" in kind else None}
        pk_a = torch.empty(P, H0, W0, 4, device="cuda")
        pk_b = torch.empty(P, H0, W0, 4, device="cuda")
        want = ref.refine(*maps, h, w, iters, packed=pk_b)
        got = eng.refine(*maps, h, w, iters, packed=pk_a, prepared=prepared)
        _equal_outputs(tuple(got) + (pk_a,), tuple(want) + (pk_b,), (rnd, kind))
    captures, replays = eng.graph_stats()
    assert captures >= 1 and replays >= 1, (captures, replays)          # the later rounds did run from captured graphs


def test_engine_prepared_parts_fall_back_where_the_fused_pass_does_not_run():
    """Context parts supplied to an engine whose GRU passes run as two kernels (fuse_gru = 0), or on the ring-buffered family
    (tile_conv = 0), are ignored -- computed in the engine as ever --: same bits as without; the split maps are used either way."""
    g = torch.Generator().manual_seed(5)
    P, h, w = 2, 24, 40
    for opts in ({"fuse_gru": 0}, {"tile_conv": 0}):
        eng, _ = _engine(opts)
        lefts = [_frame(g, h, w) for _ in range(P)]
        right = _frame(g, h, w, like=lefts[0]["fmap"])
        for f in lefts + [right]:
            f["ctx"], f["fsplit"] = eng.prepare_frame(f["fmap"], f["inp"], h, w)
        maps = ([f["fmap"] for f in lefts], [right["fmap"]] * P, [f["net"] for f in lefts], [f["inp"] for f in lefts])
        # (wrong on purpose: parts the engine must not read)
        bogus = [tuple(torch.full_like(t, 3.0) for t in f["ctx"]) for f in lefts]
        for _ in range(3):
            want = eng.refine(*maps, h, w, 3)
            got = eng.refine(*maps, h, w, 3, prepared={"ctx": bogus, "f1s": [f["fsplit"] for f in lefts], "f2s": right["fsplit"]})
            _equal_outputs(got, want, opts)


def test_frame_prepare_refusals():
    from mft_amd import ops
    g = torch.Generator().manual_seed(6)
    h, w = 24, 40
    f = _frame(g, h, w)
    eng, sd = _engine({"tile_conv": 1})
    with pytest.raises(ops.MftxError, match="pinned"):              # the batch would choose the kernel family
        eng.prepare_frame(f["fmap"], f["inp"], h, w)
    eng.prepare_frame(f["fmap"], None, h, w, context=False)          # the split map alone needs no pinned family
    e32 = ops.RaftEngine(sd, "cuda", arith=ops.ARITH_F32)
    with pytest.raises(ops.MftxError, match="split arithmetic"):
        e32.prepare_frame(f["fmap"], f["inp"], h, w)
    eng2, _ = _engine()
    ctx, fs = eng2.prepare_frame(f["fmap"], f["inp"], h, w)
    other = _frame(g, h, w)
    with pytest.raises(ops.MftxError, match="ONE second map"):      # a split second map with distinct second maps
        eng2.refine([f["fmap"]] * 2, [f["fmap"], other["fmap"]], [f["net"]] * 2, [f["inp"]] * 2, h, w, 2, prepared={"f2s": fs})
    with pytest.raises(ops.MftxError, match="per-pair"):
        eng2.refine(f["fmap"][None], f["fmap"][None], f["net"][None], f["inp"][None], h, w, 2, prepared={"f2s": fs})


# =====================================================================================================================
# C. the tracker
# =====================================================================================================================

N_FRAMES = 41          # init + 40 tracked: the delta-32 pair joins at frame 32, everything before is ramp-up


def _flower(weights_np, frames_in_flight, prepare):
    from mft_amd.config import Config
    from mft_amd.raft import RAFTWrapper
    c = Config()
    c.flow_iters = 12
    c.frames_in_flight = frames_in_flight
    c.frame_prepare = prepare
    return RAFTWrapper(c, state_dict=weights_np)


def _track(flower, frames):
    from mft_amd.config import Config
    from mft_amd.MFT import MFT
    c = Config()
    c.deltas = [np.inf, 1, 2, 4, 8, 16, 32]
    c.occlusion_threshold = 0.02
    c.keep_result_on_device = True
    c.flow_config = Config()
    c.flow_config.of_class = lambda cfg: flower
    tr = MFT(c)
    tr.init(frames[0])
    out = []
    for f in frames[1:]:
        r = tr.track(f).result
        out.append(tuple(t.detach().cpu().clone() for t in (r.flow, r.occlusion, r.sigma)))
    torch.cuda.synchronize()
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("frames_in_flight", [1, 2])
@pytest.mark.parametrize("H,W", [(512, 512), (125, 187)])
def test_tracker_same_bits_with_and_without_frame_prepare(weights_np, monkeypatch, H, W, frames_in_flight):
    """40 tracked frames with the seven deltas of the flagship configuration: ``frame_prepare`` on against off, every frame's flow,
    occlusion and sigma bit for bit -- the ramp-up frames (batches of 1 .. 6 pairs) and the full batches, at 512 x 512 and at a size off
    every grid, with one and with two frames in flight.  The run with the switch on must actually have used prepared parts."""
    monkeypatch.delenv("MFTX_FRAME_PREPARE", raising=False)
    vid = SyntheticVideo(H, W, n_frames=N_FRAMES, seed=0)
    frames = [np.array(vid[i]) for i in range(N_FRAMES)]
    off = _flower(weights_np, frames_in_flight, False)
    want = _track(off, frames)
    assert all(f.ctx is None and f.fsplit is None for f in off._frames.values())
    del off
    on = _flower(weights_np, frames_in_flight, True)
    got = _track(on, frames)
    assert on._frames and all(f.fsplit is not None for f in on._frames.values())
    if H == 512:                                   # (7 pairs of 64 x 64 cells fill the chip: the tile-resident family, context parts prepared)
        assert all(f.ctx is not None for f in on._frames.values())
    assert len(got) == len(want) == N_FRAMES - 1
    for i, (a, b) in enumerate(zip(got, want), 1):
        for name, x, y in zip(("flow", "occlusion", "sigma"), a, b):
            assert torch.isfinite(x).all(), (i, name)
            assert torch.equal(_bits(x), _bits(y)), (H, W, frames_in_flight, i, name, int((x != y).sum()))
    assert on.nonfinite_count() == 0
