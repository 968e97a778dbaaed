"""Stream ordering of the flow plugin and the tracker (mft_amd/raft.py, MFT.py, multi.py, video.py): the shared encode stream, the
lanes of ``frames_in_flight``, the side streams of ``_refine_split``, the staging ring, ``FrameRing``, ``ResultDrain``, lazy host
results and the track store -- with one of the streams the configuration uses kept busy by a bounded spin (tests/stream_harness.py).

A stalled stream turns a missing dependency into a deterministic read of old bytes: a lane that does not wait for a frame's
``ready`` event refines recycled memory while the encode stream is still spinning, a selection that does not wait for its lane chains
the previous frame's flows, a staging slot rewritten before its upload ran uploads the next frame.  The plugin is first warmed on
another video, so lanes, workspaces, graphs and pinned buffers exist and hold OTHER frames' data; the stalled run comes next, and the
reference last: the same video on a fresh tracker with one frame in flight, synchronous encoding and a device-wide synchronise after
every call.  Every frame's flow, occlusion and sigma, the chosen candidates, the track store's words and the host copies must be the
reference's, bit for bit.

``enqueued_behind`` is asserted after the first ``track`` that follows a stall.  ``init`` is not asked: it returns the CPU identity
and reads the non-finite counters back, so by contract it waits for the caller's stream -- and with it for any stream that shares
the caller's hardware queue (a process has four; measured here: a stall on lane 1 or on the split side stream, enqueued in front of
``init``, had ended when ``init`` returned, whichever stream the caller was on).  The long stall of pattern (a) is therefore enqueued
right behind ``init``, in front of the first ``track``.
"""
import contextlib
import itertools
import time

import numpy as np
import pytest
import torch

import stream_harness as sh
import tracker_helpers as th
from mft_amd.synth import SyntheticVideo

DEV = "cuda"
INF = np.inf
DELTAS = (INF, 1, 2)                     # cached features leave the window inside the sequence: the allocator recycles their blocks
ITERS = 4
_SEEDS = itertools.count(7100)            # a video seed per test that nothing else in the process has tracked

CONFIGS = {
    "1 lane": dict(lanes=1), "1 lane async": dict(lanes=1, ae=True), "1 lane sync": dict(lanes=1, ae=False),
    "2 lanes": dict(lanes=2), "2 lanes async": dict(lanes=2, ae=True), "2 lanes sync": dict(lanes=2, ae=False),
    "3 lanes": dict(lanes=3), "3 lanes async": dict(lanes=3, ae=True), "3 lanes sync": dict(lanes=3, ae=False),
    "fp32 split": dict(lanes=1, arith="fp32", split_streams=2, deltas=(INF, 1, 2, 3, 4, 5), n=12),      # six pairs from frame 6 on
    "numpy frames": dict(lanes=2, frames="numpy", n=10),                                                  # more frames than STAGING_SLOTS
    "frame ring": dict(lanes=2, ae=True, frames="ring"),
    "lazy host results": dict(lanes=2, frames="numpy", results="lazy"),
    "result drain": dict(lanes=2, results="drain"),
    "track store": dict(lanes=2, store=True),
    "two templates": dict(lanes=2, multi=True, store=True),
    "guard every frame": dict(lanes=2, nf_every=1),           # the non-finite snapshot words (two pinned slots) turn over every frame
}


def has_enc(cfg):
    ae = cfg.get("ae")
    return bool(ae) or (ae is None and cfg["lanes"] > 1 and cfg.get("arith") != "fp32") or cfg.get("frames") == "ring"


def targets_of(name):
    """Every stream the configuration uses: the caller's (the default stream, and a user stream), the encode stream, each lane, the
    split side stream."""
    cfg = CONFIGS[name]
    lanes = cfg["lanes"] if cfg.get("arith") != "fp32" and cfg["lanes"] > 1 else 0
    return (["default", "user"] + (["enc"] if has_enc(cfg) else []) + [f"lane{k}" for k in range(lanes)]
            + (["side1"] if cfg.get("split_streams", 1) > 1 else []))


OFF_GRID = ("2 lanes", "numpy frames", "track store")       # ... and these once more at 125 x 187 (pads on both axes, H * W odd)
CASES = [(name, target, pattern, (128, 136)) for name in CONFIGS for target in targets_of(name) for pattern in "ab"]
CASES += [(name, target, pattern, (125, 187)) for name in OFF_GRID for target in targets_of(name) for pattern in "ab"]


@pytest.fixture(scope="module")
def cycles_per_ms():
    return sh.calibrate()


def make_tracker(weights_np, cfg, reference=False):
    """The configuration's tracker (tests/tracker_helpers.py).  reference: one frame in flight, synchronous encoding, one stream for
    every batch."""
    ae = False if reference else (cfg["ae"] if cfg.get("ae") is not None else th.UNSET)
    return th.make_tracker(weights_np, 1 if reference else cfg["lanes"], ITERS, cfg.get("deltas", DELTAS), async_encode=ae,
                           arith=cfg.get("arith"), split_streams=1 if reference else cfg.get("split_streams", 1),
                           keep_on_device=cfg.get("results") != "lazy", track_store=bool(cfg.get("store")), multi=bool(cfg.get("multi")),
                           nonfinite_check_every=cfg.get("nf_every"))


def video(H, W, n, seed):
    vid = SyntheticVideo(H, W, n_frames=n, seed=seed)
    return [np.array(vid[i]) for i in range(n)]


class Hooks:
    """Where the stalls go.  before(i) / after(i) are called around call i of the sequence; first_track: the index of the first
    ``track`` call."""

    def __init__(self, stream, pattern, warm_times, first_track, cycles_per_ms):
        self.stream, self.pattern, self.warm, self.first, self.cpm = stream, pattern, warm_times, first_track, cycles_per_ms
        self.end = self.behind = None
        self.lengths = []

    def _stall(self, ms):
        self.lengths.append(ms)
        return sh.stall(self.stream, ms, self.cpm)

    def before(self, i):
        if self.pattern == "a":
            if i == self.first:                              # (behind init(), which waits for the host by contract: the module's docstring)
                self.end = self._stall(sh.stall_ms(sum(self.warm)))
        elif i >= self.first:
            end = self._stall(sh.stall_ms(self.warm[i]))
            if i == self.first:
                self.end = end

    def after(self, i):
        if i == self.first:
            self.behind = sh.enqueued_behind(self.end)      # immediately after the first track() behind a stall returned


def run_sequence(tr, fl, cfg, frames_np, hooks=None, sync_each=False):
    """One pass of the video -> (what was computed, as [(label, CPU bit view)]; host seconds per call)."""
    from mft_amd.video import FrameRing, ResultDrain
    n = len(frames_np)
    kind = cfg.get("frames", "device")
    if kind == "device":
        frames = [torch.from_numpy(f).to(DEV) for f in frames_np]
        torch.cuda.current_stream().synchronize()            # device frames are complete when they are passed in
    elif kind == "numpy":
        frames = [f.copy() for f in frames_np]
    else:
        ring = FrameRing(frames_np, keep=2, streams=[fl.ensure_encode_stream()]).prepare(frames_np[0].shape)
        frames = iter(ring)
    drain = ResultDrain(depth=2, nonfinite_from=tr) if cfg.get("results") == "drain" else None
    multi = bool(cfg.get("multi"))
    device_results, lazy_results, host_results, chosen, times = [], [], [], [], []
    if multi:
        tr.init([0, 3])
    for i in range(n):
        frame = next(frames) if kind == "ring" else frames[i]
        if hooks:
            hooks.before(i)
        t0 = time.perf_counter()
        if multi:
            metas = tr.track(i, frame)
        elif i == 0:
            metas = tr.init(frame)
        else:
            metas = tr.track(frame)
        times.append(time.perf_counter() - t0)
        if hooks:
            hooks.after(i)
        if kind == "numpy":
            frame[:] = 0                                     # the caller may recycle its array at once: the plugin staged it
        if multi:
            for s in sorted(metas):
                device_results.append((f"frame {i} template {s}", metas[s].result))
                if getattr(tr.templates[s], "last_chosen", None) is not None and s != i:
                    chosen.append((f"chosen {i} template {s}", tr.templates[s].last_chosen))
        elif i > 0:
            r = metas.result
            (lazy_results if cfg.get("results") == "lazy" else device_results).append((f"frame {i}", r))
            chosen.append((f"chosen {i}", tr.last_chosen))
            if drain is not None:
                if len(drain) >= drain.depth:                # collected as late as the depth allows
                    host_results.append(drain.collect(copy=True))
                drain.submit(r)
        if sync_each:
            torch.cuda.synchronize()
    while drain is not None and len(drain):
        host_results.append(drain.collect(copy=True))
    out = []
    for label, r in lazy_results:                            # read only after the last frame: each waits for its own event
        out += [(f"{label} {k} (lazy host)", sh.as_bits(t).clone()) for k, t in zip(("flow", "occlusion", "sigma"), (r.flow, r.occlusion, r.sigma))]
    torch.cuda.synchronize()
    for label, r in device_results:
        out += [(f"{label} {k}", sh.as_bits(t).cpu()) for k, t in zip(("flow", "occlusion", "sigma"), (r.flow, r.occlusion, r.sigma))]
    out += [(label, c.cpu()) for label, c in chosen]
    for j, planes in enumerate(host_results):
        out += [(f"drained {j} plane {k}", sh.as_bits(t)) for k, t in enumerate(planes)]
    stores = {}
    if cfg.get("store"):
        stores = dict(tr.track_stores) if multi else {0: tr.track_store}
        assert stores and all(len(st) > 1 for st in stores.values())
    for s, st in sorted(stores.items()):
        for slot in range(len(st)):
            out.append((f"store {s} slot {slot} packed", sh.as_bits(st.packed(slot)).cpu()))
            out.append((f"store {s} slot {slot} lohi", sh.as_bits(st.lohi(slot)).cpu()))
    return out, times


def resolve(fl, target, user):
    if target == "default":
        return torch.cuda.default_stream()
    if target == "user":
        return user
    if target == "enc":
        assert fl._enc_stream is not None
        return fl._enc_stream
    if target.startswith("lane"):
        k = int(target[4:])
        assert len(fl._lanes) > k, (target, len(fl._lanes))
        return fl._lanes[k][1]
    k = int(target[4:])
    assert len(fl._side) > k and fl._side[k] is not None, (target, fl._side)
    return fl._side[k]


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,target,pattern,size", CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_tracker_is_ordered(weights_np, cycles_per_ms, name, target, pattern, size):
    cfg = CONFIGS[name]
    H, W = size
    n = cfg.get("n", 9)
    seed = next(_SEEDS)
    frames_np, warm_np = video(H, W, n, seed), video(H, W, n, seed + 50_000)
    tr, fl = make_tracker(weights_np, cfg)
    user = sh.visible_stream(cycles_per_ms) if target == "user" else None     # (work wrongly put on the default stream is seen there)
    with (torch.cuda.stream(user) if user is not None else contextlib.nullcontext()):
        _, warm_times = run_sequence(tr, fl, cfg, warm_np)                   # lanes, workspaces, graphs and pinned buffers exist now
        torch.cuda.synchronize()
        hooks = Hooks(resolve(fl, target, user), pattern, warm_times, 0 if cfg.get("multi") else 1, cycles_per_ms)
        got, _ = run_sequence(tr, fl, cfg, frames_np, hooks=hooks)
    torch.cuda.synchronize()
    print(f"{name} / {target} / {pattern} / {size}: warm calls took {1e3 * min(warm_times[1:]):.2f} .. {1e3 * max(warm_times[1:]):.2f} ms on the host, "
          f"stalls of {min(hooks.lengths):.0f} .. {max(hooks.lengths):.0f} ms, enqueued behind the stall: {hooks.behind}")
    assert hooks.behind, f"{name} / {target} / {pattern}: the stall had ended when the first track() behind it returned: nothing is proven"
    ref_tr, ref_fl = make_tracker(weights_np, cfg, reference=True)
    want, _ = run_sequence(ref_tr, ref_fl, cfg, frames_np, sync_each=True)
    assert [label for label, _ in got] == [label for label, _ in want]
    bad = [(label, int((a != b).sum())) for (label, a), (_, b) in zip(got, want) if a.shape != b.shape or not torch.equal(a, b)]
    assert not bad, f"{name} with {target} stalled ({pattern}): {len(bad)} of {len(got)} tensors differ from the race-free run, first {bad[:4]}"
    torch.cuda.synchronize()


# ---- negative control ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_harness_sees_a_planted_ordering_bug(cycles_per_ms):
    """A toy producer that calls ``ops.copy_bytes`` under ``torch.cuda.stream(other)`` instead of on the current stream (only valid
    bytes move): steps 1-4 of tests/test_gpu_streams_ops.py must report the mismatch (``stream_harness.planted_bug_is_seen``), with
    the null stream and with a side stream as the other one.  If they do not, the harness is blind in this process -- two streams
    sharing a hardware queue, which serialises them, would be one cause -- and every other test of this file proves nothing."""
    from mft_amd import ops
    side = sh.visible_stream(cycles_per_ms)
    for other in (torch.cuda.default_stream(), torch.cuda.Stream()):
        assert sh.planted_bug_is_seen(side, other, cycles_per_ms, copy=ops.copy_bytes, n=125 * 187 + 3), \
            "the harness is blind in this process: a copy made on another stream, in front of the rewrite of its source, was not seen"
    torch.cuda.synchronize()


# ---- the staging ring of a shape the plugin drops -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_dropped_staging_ring_is_not_recycled_under_its_upload(weights_np, cycles_per_ms):
    """``_stage_host_frame`` keeps pinned rings for four frame shapes; a fifth shape drops the oldest ring.  Its buffers go back to the
    pinned pool, which knows nothing of the copy KERNEL that still has to read them (only torch's own copies are recorded there): the
    next user of the pool gets the block and writes into it.  With the encode stream stalled the upload of the dropped shape's frame
    is still pending at that moment, so it must arrive intact all the same: the plugin has to wait for a dropped ring's uploads.
    (That wait is a host wait by contract, like a staging slot's ``synchronize()``: ``enqueued_behind`` is asserted before it.)"""
    import gc
    rng = np.random.default_rng(next(_SEEDS))
    shapes = [(64, 60 + k, 3) for k in range(5)]              # five shapes, one size class of the pinned pool (11.5 .. 12.3 kB)
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]

    def stage(fl, enc, k):
        with torch.cuda.stream(enc):
            return fl._device_image(frames[k].copy())

    def grab(first):
        """The next user of the pinned pool: whoever gets the dropped ring's block writes into it."""
        held = []
        for _ in range(32):
            t = torch.empty(64 * 64 * 3, dtype=torch.uint8).pin_memory()
            held.append(t)
            if t.data_ptr() == first:
                t.numpy()[:] = 0xEE
                return True
        return False

    def sequence(fl, enc, stall_end=None):
        dev = [stage(fl, enc, k) for k in range(4)]
        behind = stall_end is not None and sh.enqueued_behind(stall_end)      # immediately after the fourth upload was enqueued
        first = fl._staging[shapes[0]]["slots"][0][0].data_ptr()
        dev.append(stage(fl, enc, 4))                          # the fifth shape: the first shape's ring is dropped
        assert shapes[0] not in fl._staging and shapes[4] in fl._staging
        gc.collect()                                           # (a slot and its buffer refer to each other: freed by the collector)
        reused = grab(first)
        still = stall_end is not None and sh.enqueued_behind(stall_end)
        return dev, behind, reused, still

    # the same sequence on another plugin, unstalled: its host time (the collector's included) sizes the stall, and its rings warm the
    # pinned pool
    fl0 = make_tracker(weights_np, CONFIGS["2 lanes async"])[1]
    enc = fl0.ensure_encode_stream()
    gc.collect()
    _, host = sh.timed(lambda: sequence(fl0, enc))
    torch.cuda.synchronize()
    del fl0
    gc.collect()
    fl = make_tracker(weights_np, CONFIGS["2 lanes async"])[1]
    assert fl.ensure_encode_stream() is enc
    ms = sh.stall_ms(host)
    end = sh.stall(enc, ms, cycles_per_ms)
    dev, behind, reused, still = sequence(fl, enc, end)
    with torch.cuda.stream(enc):
        done = torch.cuda.Event()
        done.record(enc)
    done.synchronize()
    got = [d.cpu().numpy() for d in dev]
    torch.cuda.synchronize()
    print(f"dropped staging ring: the sequence took {1e3 * host:.2f} ms on the host, stalled for {ms:.0f} ms, enqueued behind the stall: "
          f"{behind}; the pinned pool handed the dropped block out again: {reused}; the stall was still running then: {still} (False where "
          "the plugin waited for the dropped ring's uploads)")
    assert behind, "the stall had ended when the fourth upload was enqueued: nothing is proven"
    assert reused, "the pinned pool did not hand the dropped ring's block out again: nothing is proven"
    for k, (g, f) in enumerate(zip(got, frames)):
        assert np.array_equal(g, f), f"frame {k}: {int((g != f).sum())} bytes differ from what was handed in"
