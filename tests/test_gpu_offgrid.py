"""The tracker at frame sizes off every grid, the copy kernel that moves its frames and results, and re-initialisation.

A. ``mftx_copy_bytes`` against the source bytes: the byte tail, the grid-stride loop above 8 MiB, pinned host memory on either
   side, the alignment guard and the stream it runs on.
B. ``MFT.track()`` through the real flow plugin at sizes where H * W % 4 takes all four values, against the oracle tracker, with
   tolerances tied to the oracle's own rounding noise (fp32 oracle vs fp64 oracle) instead of the north-star bar alone; the same
   bits on every way a frame can come in and a result can go out; one plugin fed changing sizes.
C. ``MFT.init()`` on a tracker (or a plugin) that has seen a non-finite frame starts clean, and the guard still works afterwards.

Needs an MI355X."""
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import mft_oracle as O
from mft_amd.synth import SyntheticVideo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def epe(a, b):
    return (a.double() - b.double()).pow(2).sum(0).sqrt()


def make_flower(weights_np, iters=12, frames_in_flight=None):
    from mft_amd.config import Config
    from mft_amd.raft import RAFTWrapper
    c = Config()
    c.flow_iters = iters
    if frames_in_flight is not None:
        c.frames_in_flight = frames_in_flight
    return RAFTWrapper(c, state_dict=weights_np)


def make_tracker(flower, deltas):
    """As tests/test_gpu_e2e.py::make_tracker: no host-path knob set, so meta.result is a PendingHostResult."""
    from mft_amd.config import Config
    from mft_amd.MFT import MFT
    c = Config()
    c.deltas = list(deltas)
    c.occlusion_threshold = 0.02
    c.flow_config = Config()
    c.flow_config.of_class = lambda cfg: flower
    return MFT(c)


@pytest.fixture(scope="module")
def flower(weights_np):
    return make_flower(weights_np)


@pytest.fixture(scope="module")
def flower2(weights_np):
    return make_flower(weights_np, frames_in_flight=2)


# =====================================================================================================================
# A. mftx_copy_bytes
# =====================================================================================================================

MIB = 1 << 20
# byte tails of every kind around one 16-byte unit, an odd frame (uint8 H x W x 3), an odd plane (fp32 H x W), and two lengths above
# 2048 blocks x 256 threads x 16 bytes = 8 MiB, where the grid-stride loop takes a second (and a fourth) round -- with a tail
COPY_LENGTHS = [0, 1, 15, 16, 17, 255, 4099, 125 * 187 * 3, 127 * 129 * 4, 8 * MIB + 16 + 5, 24 * MIB + 3]
GUARD = 64


def _canary(n):
    return torch.from_numpy(((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8))


def _place(x, where):
    """A uint8 CPU tensor -> device memory or pinned host memory (the front of a larger pinned buffer: a tensor without
    elements has no storage to pin)."""
    if where == "device":
        return x.to(DEV)
    out = torch.empty(x.numel() + 16, dtype=torch.uint8).pin_memory()[:x.numel()]
    assert out.is_pinned()
    return out.copy_(x)


def _host_bytes(t):
    torch.cuda.synchronize()
    return t.cpu().numpy() if t.is_cuda else t.numpy().copy()


@pytest.mark.parametrize("direction", ["device_to_device", "pinned_to_device", "device_to_pinned"])
@pytest.mark.parametrize("n", COPY_LENGTHS)
def test_copy_bytes_equals_source_bytes(n, direction):
    """dst == src bit for bit, and not one byte before or behind dst is written: dst is the middle of a buffer with 64 canary bytes
    on either side, starts on a 16-byte boundary and ends wherever n says -- the canary behind it starts at the first byte the
    kernel's tail loop must not touch."""
    from mft_amd import ops
    src_where, dst_where = {"device_to_device": ("device", "device"), "pinned_to_device": ("pinned", "device"),
                            "device_to_pinned": ("device", "pinned")}[direction]
    want = np.random.default_rng(1000 + n % 9973).integers(0, 256, size=n, dtype=np.uint8)
    src = _place(torch.from_numpy(want.copy()), src_where)
    canary = _canary(GUARD + n + GUARD)
    big = _place(canary, dst_where)
    dst = big[GUARD:GUARD + n]
    assert big.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    assert ops.copy_bytes(src, dst) is dst
    got = _host_bytes(big)
    assert np.array_equal(got[GUARD:GUARD + n], want), (n, direction, int((got[GUARD:GUARD + n] != want).sum()))
    assert np.array_equal(got[:GUARD], canary.numpy()[:GUARD]), "bytes before dst were written"
    assert np.array_equal(got[GUARD + n:], canary.numpy()[GUARD + n:]), "bytes behind dst were written"
    assert np.array_equal(_host_bytes(src), want), "the source changed"


def test_copy_bytes_rejects_what_it_cannot_move():
    """A pointer off the 16-byte grid is refused by the library (MFTX_E_ALIGN) before any launch; non-contiguous tensors, sizes
    that differ and pageable host memory are refused by the wrapper.  The destination keeps its bytes every time."""
    from mft_amd import ops
    from mft_amd._lib import MftxError
    n = 4096
    canary = _canary(n + 32)
    data = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=n + 32, dtype=np.uint8))
    for src_where, dst_where in (("device", "device"), ("pinned", "device"), ("device", "pinned")):
        src_big, dst_big = _place(data, src_where), _place(canary, dst_where)
        cases = {
            "source +4 bytes": (src_big[4:4 + n], dst_big[:n]),
            "destination +4 bytes": (src_big[:n], dst_big[4:4 + n]),
            "both +4 bytes": (src_big[4:4 + n], dst_big[4:4 + n]),
            "non-contiguous source": (src_big[:2 * 1024:2], dst_big[:1024]),
            "non-contiguous destination": (src_big[:1024], dst_big[:2 * 1024:2]),
            "sizes differ": (src_big[:n], dst_big[:n - 16]),
            "pageable source": (data[:n], dst_big[:n]),
        }
        for name, (s, d) in cases.items():
            with pytest.raises(MftxError, match="copy_bytes"):
                ops.copy_bytes(s, d)
            assert np.array_equal(_host_bytes(dst_big), canary.numpy()), (name, src_where, dst_where)
    pageable = canary.clone()
    with pytest.raises(MftxError, match="copy_bytes"):
        ops.copy_bytes(_place(data, "device")[:n], pageable[:n])
    assert torch.equal(pageable, canary)
    # the unsigned views of one fp32 tensor: element size does not matter, bytes do
    f = torch.arange(1024, dtype=torch.float32, device=DEV)
    g = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ops.copy_bytes(f, g)
    assert torch.equal(g.view(torch.float32), f)


@pytest.mark.parametrize("direction", ["device_to_device", "device_to_pinned"])
def test_copy_bytes_runs_on_the_current_stream(direction):
    """On a side stream the copy is ordered behind what that stream produced before it -- here the source is rewritten on the
    side stream behind a delay, so a copy on any other stream would move the old bytes -- and its result is there once an event
    recorded behind it has completed.  (Nothing is required of dst before that.)"""
    from mft_amd import ops
    n = 125 * 187 * 4 * 4 + 7
    old = torch.full((n,), 3, dtype=torch.uint8, device=DEV)
    new = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=n, dtype=np.uint8)).to(DEV)
    src = old.clone()
    big = _place(_canary(GUARD + n + GUARD), "device" if direction == "device_to_device" else "pinned")
    dst = big[GUARD:GUARD + n]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)             # (a bounded spin of some milliseconds: the side stream is busy, the others are not)
        src.copy_(new)
        ops.copy_bytes(src, dst)
        done = side.record_event()
    done.synchronize()
    got = big.cpu().numpy() if big.is_cuda else big.numpy().copy()       # (after the event only: no device-wide synchronisation first)
    torch.cuda.synchronize()
    assert np.array_equal(got[GUARD:GUARD + n], new.cpu().numpy())
    assert np.array_equal(got[:GUARD], _canary(GUARD).numpy()) and np.array_equal(got[GUARD + n:], _canary(GUARD + n + GUARD).numpy()[GUARD + n:])


# =====================================================================================================================
# B. the tracker at off-grid sizes
# =====================================================================================================================

# (H, W): H * W % 4 takes all four values, the pad amounts of both axes are odd and even, the 1/8 grid is at least 16 x 16 (below
# that the reference's own coordinate normalisation divides by zero at the coarsest correlation level); (128, 136) is the control
SIZES = [(125, 187), (127, 129), (130, 131), (129, 133), (121, 122), (128, 136)]
DELTAS = (np.inf, 1, 2, 4)
ITERS = 12
N_TRACKED = 6

# HIP-vs-fp64 error as a multiple of the oracle's own fp32-vs-fp64 error.  The products of the default (split fp16 x 3) arithmetic
# are specified at <= 2^-23 each, i.e. fp32 grade, but the summation order differs from the oracle's (MFMA tiles, 12 iterations, four
# chained candidates), so a factor above 1 is expected: 4 for means, 8 for the one-pixel maxima -- set before the first run, never above
# 16.  Observed on an MI355X: profiles/offgrid_tracker_noise.txt (ratio per size, frame and quantity).
K_MEAN = 4.0
K_MAX = 8.0


def _frames(H, W, n=N_TRACKED + 1):
    vid = SyntheticVideo(H, W, n_frames=8, seed=0)
    return [np.array(vid[i]) for i in range(n)]


def _oracle_tracker(sd):
    return O.Tracker(lambda l, r, li, ri: O.compute_flow(sd, li, ri, ITERS), deltas=DELTAS)


def _cpu(r):
    return tuple(t.detach().cpu().clone() for t in (r.flow, r.occlusion, r.sigma))


def _assert_same_bits(got, want, what):
    for name, a, b in zip(("flow", "occlusion", "sigma"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        assert torch.equal(a, b), (what, name, int((a != b).sum()))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("H,W", SIZES)
def test_tracker_offgrid_vs_oracle(flower, weights_cpu, H, W):
    """Six tracked frames from init with deltas {inf, 1, 2, 4} and 12 iterations on the HIP tracker -- the default configuration,
    meta.result a PendingHostResult -- on the oracle tracker in fp32 and on the oracle tracker in fp64 (MFT/MFT.py:104-143,
    MFT/results.py:87-136, 250-265).  Per frame: requested pairs and memory keys equal, the result on the host with the right
    shapes, chosen-delta agreement >= 99.9 % (pixels that chose differently are left out of the plane comparisons; the cap is
    meaningful here, tools/offgrid_tie_margin.py: noise of 1e-5 on every flow input flips <= 0.014 % of the pixels), occlusion
    exactly 1 where the oracle's chained position leaves the image, and

        error(HIP, oracle fp64)  <=  K * error(oracle fp32, oracle fp64)

    for the mean EPE, mean |occlusion| and mean relative sigma difference (K_MEAN) and for the maxima of the three (K_MAX), over
    the pixels where all three trackers chose the same delta.  The absolute bars of the other tracker tests (mean EPE <= 1e-3 px,
    occlusion < 2e-3, sigma < 2e-3 relative, against the fp32 oracle) stay asserted as the outer fence."""
    from mft_amd.results import FlowOUTrackingResult, PendingHostResult
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    frames = _frames(H, W)
    tr = make_tracker(flower, DELTAS)
    meta = tr.init(frames[0])
    assert meta.result.flow.shape == (2, H, W) and not meta.result.flow.is_cuda
    ref32 = _oracle_tracker(weights_cpu)
    ref32.init(frames[0])
    with O.precision(torch.float64):
        ref64 = _oracle_tracker(O.cast_weights(weights_cpu, torch.float64))
        ref64.init(frames[0])
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    n_fractional = n_outside = 0
    failures = []
    for i in range(1, N_TRACKED + 1):
        got = tr.track(frames[i]).result
        assert isinstance(got, PendingHostResult) and isinstance(got, FlowOUTrackingResult), type(got)
        chosen = tr.last_chosen.cpu().long()
        with torch.no_grad():
            w32 = ref32.track(frames[i])
            with O.precision(torch.float64):
                w64 = ref64.track(frames[i])
        assert w64.result[0].dtype == torch.float64 and w32.result[0].dtype == torch.float32
        assert sorted(tr.last_pairs) == sorted(w32.pairs) == sorted(w64.pairs), (i, tr.last_pairs, w32.pairs)
        assert sorted(tr.memory.keys()) == w32.memory_keys == w64.memory_keys, i
        assert (got.H, got.W) == (H, W)
        assert got.flow.shape == (2, H, W) and got.occlusion.shape == (1, H, W) and got.sigma.shape == (1, H, W)
        assert not got.flow.is_cuda and got.flow.dtype == torch.float32 and got.ready()
        assert tr.memory[i]['result'].flow.shape == (2, H, W) and chosen.shape == (H, W)
        rf, ro, rs = w32.result
        df, do, ds = w64.result
        same = chosen == w32.chosen.long()
        same3 = same & (chosen == w64.chosen.long())
        assert same.float().mean() >= 0.999, (i, float(same.float().mean()))
        assert same3.float().mean() >= 0.999, (i, float(same3.float().mean()))
        # ---- the outer fence: the absolute bars of test_c2_tracker_real_state_vs_oracle, against the fp32 oracle
        e = epe(got.flow, rf)
        assert float(e[same].mean()) <= 1e-3, (i, float(e[same].mean()))
        assert float(e.mean()) <= 1e-3, (i, float(e.mean()))
        assert (got.occlusion - ro).abs()[0][same].max() < 2e-3, i
        assert ((got.sigma - rs).abs() / rs.clamp_min(1e-6))[0][same].max() < 2e-3, i
        # ---- the invalid mask (results.py:250-265): where the oracle's chained position leaves the image, occlusion is exactly 1
        px, py = xx + rf[0], yy + rf[1]
        outside = (px < 0) | (py < 0) | (px >= W) | (py >= H)
        n_outside += int(outside.sum())
        assert bool((got.occlusion[0][outside & same] == 1).all()), i
        if i >= 2:
            n_fractional += int(((rf[0] != rf[0].round()) | (rf[1] != rf[1].round())).sum())
        # ---- against the oracle's own rounding noise
        def errors(flow, occl, sigma):
            ee = epe(flow, df)[same3]
            eo = (occl.double() - do).abs()[0][same3]
            es = ((sigma.double() - ds).abs() / ds.clamp_min(1e-6))[0][same3]
            return {"epe_mean": float(ee.mean()), "epe_max": float(ee.max()), "occl_mean": float(eo.mean()), "occl_max": float(eo.max()),
                    "sigma_mean": float(es.mean()), "sigma_max": float(es.max())}
        noise, hip = errors(rf, ro, rs), errors(got.flow, got.occlusion, got.sigma)
        for q in noise:
            k = K_MAX if q.endswith("_max") else K_MEAN
            ratio = hip[q] / noise[q] if noise[q] > 0 else (0.0 if hip[q] == 0 else float("inf"))
            print(f"offgrid-noise {H}x{W} frame {i} {q:10s} hip/fp64 {hip[q]:.3e}  fp32/fp64 {noise[q]:.3e}  ratio {ratio:6.2f}  (bound {k:g})"
                  f"  agree {float(same3.float().mean()):.5f}")
            if not hip[q] <= k * noise[q]:
                failures.append((i, q, hip[q], noise[q], ratio))
    assert not failures, failures
    assert n_fractional > 0.5 * (N_TRACKED - 1) * H * W, n_fractional
    assert n_outside > 0, "the sequence should push some pixels out of the image"


def _run_default(flower, frames):
    """The default API loop: pageable numpy frames in, PendingHostResults out, read after the loop."""
    tr = make_tracker(flower, DELTAS)
    tr.init(frames[0])
    res = [tr.track(f).result for f in frames[1:]]
    return res, [_cpu(r) for r in res]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("H,W", [(125, 187), (130, 131)])
def test_offgrid_same_bits_on_every_way_in_and_out(flower, flower2, H, W):
    """However a frame reaches the tracker (pageable numpy, FrameRing's pinned tensors, a pinned view off the 16-byte grid, device
    tensors) and however a result leaves it (PendingHostResult, the blocking copy, kept on the device, ResultDrain from the
    tracker's planes and from plane views of one [4, H, W] tensor -- submit's fallback for planes off the 16-byte grid), with one and
    with two frames in flight: the same bits as the default loop."""
    from mft_amd.results import FlowOUTrackingResult, PendingHostResult
    from mft_amd.video import FrameRing, ResultDrain
    frames = _frames(H, W)
    pending, base = _run_default(flower, frames)
    assert all(isinstance(r, PendingHostResult) for r in pending)
    for b in base:
        assert b[0].shape == (2, H, W) and b[1].shape == (1, H, W) and b[2].shape == (1, H, W)
        assert all(torch.isfinite(t).all() for t in b)
    # a PendingHostResult at an off-grid size behaves like the CPU result it stands for
    r = pending[-1]
    torch.cuda.synchronize()
    assert r.ready() and r.wait() is r and r.ready()
    assert all(t.data_ptr() % 16 == 0 for t in (r.flow, r.occlusion, r.sigma)) and r.flow.is_contiguous()
    c = r.clone()
    assert type(c) is FlowOUTrackingResult
    _assert_same_bits(_cpu(c), base[-1], "clone")
    p = pickle.loads(pickle.dumps(r))
    assert type(p) is FlowOUTrackingResult and (p.H, p.W) == (H, W)
    _assert_same_bits(_cpu(p), base[-1], "pickle")
    assert r.cpu() is r

    def pinned_off_grid(f):
        buf = torch.empty(f.size + 32, dtype=torch.uint8).pin_memory()
        v = buf[4:4 + f.size].view(f.shape)
        assert v.is_pinned() and v.data_ptr() % 16 == 4
        v.copy_(torch.from_numpy(f))
        return v

    ways_in = {
        "FrameRing": lambda: iter(FrameRing(iter(frames))),
        "pinned view off the 16-byte grid": lambda: iter([pinned_off_grid(f) for f in frames]),
        "device tensors": lambda: iter([torch.from_numpy(f).to(DEV) for f in frames]),
    }
    for fif, fl in ((1, flower), (2, flower2)):
        if fif == 2:
            _assert_frames_equal(_run_default(fl, frames)[1], base, "numpy frames, 2 frames in flight")
            assert len(fl._lanes) == 2
        for name, source in ways_in.items():
            tr = make_tracker(fl, DELTAS)
            it = source()
            tr.init(next(it))
            got = [tr.track(f).result for f in it]
            _assert_frames_equal([_cpu(g) for g in got], base, f"in: {name}, {fif} in flight")
        # ---- ways out
        tr = make_tracker(fl, DELTAS)
        tr.C.lazy_host_result = False
        tr.init(frames[0])
        got = [tr.track(f).result for f in frames[1:]]
        assert all(type(g) is FlowOUTrackingResult and not g.flow.is_cuda for g in got)
        _assert_frames_equal([_cpu(g) for g in got], base, f"out: blocking copy, {fif} in flight")
        tr = make_tracker(fl, DELTAS)
        tr.C.keep_result_on_device = True
        tr.init(frames[0])
        got = [tr.track(f).result for f in frames[1:]]
        assert all(g.flow.is_cuda for g in got)
        _assert_frames_equal([_cpu(g) for g in got], base, f"out: kept on the device, {fif} in flight")
        for views in (False, True):
            tr = make_tracker(fl, DELTAS)
            tr.C.keep_result_on_device = True
            tr.init(frames[0])
            drain = ResultDrain(depth=3, nonfinite_from=tr)
            got, took_fallback = [], False
            for f in frames[1:]:
                res = tr.track(f).result
                if views:
                    packed = torch.cat(res.planes(), 0)
                    assert packed.shape == (4, H, W)
                    planes = (packed[0:2], packed[2:3], packed[3:4])
                    took_fallback |= any(t.data_ptr() % 16 != 0 for t in planes)
                    drain.submit(planes)
                else:
                    drain.submit(res)
                if len(drain) == 3:
                    got.append(tuple(t.clone() for t in drain.collect(copy=True)))
            while len(drain):
                got.append(tuple(t.clone() for t in drain.collect(copy=True)))
            assert took_fallback == views, "a plane view of [4, H, W] must be off the 16-byte grid at this size"
            _assert_frames_equal(got, base, f"out: ResultDrain ({'plane views' if views else 'tracker planes'}), {fif} in flight")
        assert fl.nonfinite_count() == 0


def _assert_frames_equal(got, base, what):
    assert len(got) == len(base), (what, len(got), len(base))
    for i, (a, b) in enumerate(zip(got, base), 1):
        _assert_same_bits(a, b, f"{what}, frame {i}")


def test_one_plugin_changing_sizes(weights_np):
    """One RAFTWrapper fed (127, 129), then (125, 187), then (127, 129) again -- init() in between: the first and the third run
    are equal bit for bit, and equal to a fresh plugin's.  Both sizes pad to the same 1/8 grid height and to different widths:
    cached graphs, workspaces, staging buffers and tile choices keyed by shape must not leak from one size into the next."""
    n = 3
    small, wide = _frames(127, 129, n + 1), _frames(125, 187, n + 1)

    def run(fl, frames):
        tr = make_tracker(fl, DELTAS)
        tr.init(frames[0])
        return [_cpu(tr.track(f).result) for f in frames[1:]]

    fl = make_flower(weights_np)
    first, middle, third = run(fl, small), run(fl, wide), run(fl, small)
    _assert_frames_equal(third, first, "(127, 129) again on a used plugin")
    _assert_frames_equal(first, run(make_flower(weights_np), small), "(127, 129) on a fresh plugin")
    _assert_frames_equal(middle, run(make_flower(weights_np), wide), "(125, 187) on a fresh plugin")
    # ... and on ONE tracker object re-initialised at another size
    tr = make_tracker(fl, DELTAS)
    for frames, want in ((wide, middle), (small, first), (wide, middle)):
        tr.init(frames[0])
        _assert_frames_equal([_cpu(tr.track(f).result) for f in frames[1:]], want, f"one tracker, {frames[0].shape}")
    assert fl.nonfinite_count() == 0


# =====================================================================================================================
# C. re-initialising a tracker after a non-finite frame
# =====================================================================================================================

EVERY = 3
N_CLEAN = 2 * EVERY + 2
RE_DELTAS = (np.inf, 1)
PATHS = ["lazy", "blocking", "device"]


def _re_tracker(fl, path):
    tr = make_tracker(fl, RE_DELTAS)
    tr.C.nonfinite_check_every = EVERY
    if path == "blocking":
        tr.C.lazy_host_result = False
    elif path == "device":
        tr.C.keep_result_on_device = True
    return tr


def _poison(fl, frame_id):
    """As test_nonfinite_results_are_counted_and_raise: features whose correlation leaves the fp16 range of the split arithmetic
    -- NaN flows out of the refinement, counted by the plugin; no fault."""
    from mft_amd.raft import FrameFeatures
    N = 16 * 24
    f = torch.full((N, 256), 7.0e4, device=DEV)
    z = torch.zeros(N, 128, device=DEV)
    assert frame_id in fl._frames
    fl._frames[frame_id] = FrameFeatures(f, z, z, 16, 24, (0, 0, 0, 0), (128, 192))


def _track_and_read(tr, frames):
    """track() every frame and read every result the way its path delivers it."""
    out = []
    for f in frames:
        r = tr.track(f).result
        out.append(_cpu(r))
    return out


def _poisoned(weights_np, path, vid):
    """A plugin and a tracker that have met a poisoned frame and raised the FloatingPointError it causes."""
    fl = make_flower(weights_np, iters=2)
    tr = _re_tracker(fl, path)
    tr.init(vid[0])
    _track_and_read(tr, [vid[1]])
    _poison(fl, 1)
    with pytest.raises(FloatingPointError, match="non-finite"):
        _track_and_read(tr, [vid[i] for i in range(2, 2 + 2 * EVERY)])      # (at once on the host paths, within 2 x EVERY frames on the device path)
    return fl, tr


@pytest.mark.parametrize("who", ["same tracker", "second tracker on the plugin"])
@pytest.mark.parametrize("path", PATHS)
def test_reinit_after_nonfinite_frame_starts_clean(weights_np, path, who):
    """After a poisoned frame and its FloatingPointError, init() on clean frames -- on the same tracker, or on a second tracker
    created afterwards on the same plugin, and without any nonfinite_count(reset=True) by hand -- tracks 2 x nonfinite_check_every + 2
    frames without an error on every host path, with the bits of a fresh tracker on a fresh plugin; and the guard still works
    afterwards: another poisoned frame raises within the documented 2 x nonfinite_check_every frames."""
    bad_vid = SyntheticVideo(128, 192, n_frames=2 + 2 * EVERY, seed=1)
    vid = SyntheticVideo(128, 192, n_frames=1 + N_CLEAN + 2 * EVERY, seed=4)
    clean = [vid[i] for i in range(1 + N_CLEAN)]
    fresh = _re_tracker(make_flower(weights_np, iters=2), path)
    fresh.init(clean[0])
    want = _track_and_read(fresh, clean[1:])
    assert all(torch.isfinite(t).all() for w in want for t in w)

    fl, tr = _poisoned(weights_np, path, bad_vid)
    if who != "same tracker":
        tr = _re_tracker(fl, path)
    tr.init(clean[0])
    got = _track_and_read(tr, clean[1:])                      # must not raise
    _assert_frames_equal(got, want, f"{path}, {who}")
    assert tr.current_frame_i == N_CLEAN and fl.nonfinite_count() == 0
    # the guard after re-init
    _poison(fl, N_CLEAN)
    with pytest.raises(FloatingPointError, match="non-finite"):
        _track_and_read(tr, [vid[i] for i in range(1 + N_CLEAN, 1 + N_CLEAN + 2 * EVERY)])
    assert tr.current_frame_i <= N_CLEAN + 2 * EVERY
