"""``DenseTrackStore.appearance`` on the device (csrc/trackstore.hip: ts_appearance_kernel through
``atlas_ops.trackstore_appearance``) against the composition it fuses -- ``DenseTrackStore._compose_appearance`` on a device store:
``ops.trackstore_unpack``, ``ops.warp_backward`` and torch elementwise per column, float32 sums in column order -- bit for bit;
against the host store within a measured tolerance; through a tracker pass; its argument checks; and behind a stalled stream."""
import ctypes

import numpy as np
import pytest
import torch

import stream_catalog as cat
import stream_harness as sh
from test_gpu_streams_ops import run_behind_stall
from test_track_appearance import CASE_SIGMA_MAX, COLUMNS, SIZES, case_store, images_for, set_lohi, visible_share_ok
from test_track_locate import const_planes, field, make_store

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered")]
DEV = "cuda"
CHANNELS = [1, 3, 4]
# reference, stack, fill, sigma_max: each of them both ways
OPTIONS = [(True, True, 200, None), (False, False, 0, None), (True, False, 0, CASE_SIGMA_MAX), (False, True, 0, CASE_SIGMA_MAX)]


def bits(t):
    return t.contiguous().view(torch.int32)


def dev_images(images):
    return [torch.from_numpy(i).to(DEV) for i in images]


def composition(st, frames, images, reference=None, thr=0.5, sigma_max=None, stack=False, fill=0):
    """The definition on a device store -> (sum, sumsq, count, warped, visible)."""
    assert st.native
    return st._compose_appearance(st._slots(frames), images, reference, thr, sigma_max, stack, fill)


def same(got, want, stack):
    """``got``: a TrackAppearance; ``want``: the composition's tuple.  Bits of the sums, count, the stack's bytes."""
    total, totalsq, count, warped, visible = want
    assert got.sum.is_cuda and got.sum.dtype == torch.float32 and got.sum.shape == total.shape and got.sum.is_contiguous()
    assert got.count.dtype == torch.int32 and torch.equal(got.count, count), int((got.count != count).sum())
    assert torch.equal(bits(got.sum), bits(total)), int((bits(got.sum) != bits(total)).sum())
    assert torch.equal(bits(got.sumsq), bits(totalsq)), int((bits(got.sumsq) != bits(totalsq)).sum())
    if stack:
        assert got.warped.dtype == torch.uint8 and got.visible.dtype == torch.bool
        assert torch.equal(got.visible, visible), int((got.visible != visible).sum())
        assert torch.equal(got.visible.view(torch.uint8), visible.view(torch.uint8))            # 0 / 1, no other byte
        assert torch.equal(got.warped, warped), int((got.warped != warped).sum())
    else:
        assert got.warped is None and got.visible is None


# ---- 1. bitwise against the composition on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("n", COLUMNS)
@pytest.mark.parametrize("H,W", SIZES)
def test_appearance_is_the_composition_bitwise(H, W, n):
    st = case_store(H, W, n, device=DEV)
    for C in CHANNELS:
        images, ref = dev_images(images_for(n, n, H, W, C)), dev_images(images_for(100 + n, 1, H, W, C))[0]
        for with_ref, stack, fill, smax in OPTIONS:
            reference = ref if with_ref else None
            got = st.appearance(images, reference=reference, sigma_max=smax, stack=stack, fill=fill)
            want = composition(st, None, images, reference, sigma_max=smax, stack=stack, fill=fill)
            same(got, want, stack)
            if stack:
                ok, share = visible_share_ok(got.visible.cpu().numpy(), H)
                assert ok, (H, W, n, smax, share)
    stacked = st.appearance(torch.stack(images), reference=ref, stack=True, fill=200)           # one [T, H, W, C] tensor: the same
    same(stacked, composition(st, None, images, ref, stack=True, fill=200), True)


# ---- 2. a store of three chunks, a column subset in another order, a column twice ----------------------------------------------------
def test_three_chunk_store_column_subset():
    H, W, C = 37, 53, 3
    st = case_store(H, W, 5, device=DEV, frames_per_chunk=2)
    assert len(st._chunks) == 3
    images = dev_images(images_for(9, 5, H, W, C))
    ref = dev_images(images_for(10, 1, H, W, C))[0]
    frames = [4, 1, 3, 1]
    got = st.appearance([images[f] for f in frames], frames, reference=ref, stack=True, fill=3)
    same(got, composition(st, frames, [images[f] for f in frames], ref, stack=True, fill=3), True)
    assert got.frames == frames and torch.equal(got.visible[1], got.visible[3]) and torch.equal(got.warped[1], got.warped[3])
    cpu = case_store(H, W, 5, frames_per_chunk=2).appearance([images[f].cpu() for f in frames], frames, reference=ref.cpu(), stack=True, fill=3)
    assert torch.equal(got.count.cpu(), cpu.count) and torch.equal(got.visible.cpu(), cpu.visible)


# ---- 3. NaN, inf and flat channels ----------------------------------------------------------------------------------------------------
def test_nan_inf_and_flat_channels_come_out_as_the_composition_has_them():
    H, W, C = 37, 53, 3
    images = dev_images(images_for(11, 3, H, W, C))
    ref = dev_images(images_for(12, 1, H, W, C))[0]
    for ch in (0, 1):                       # a stored frame whose flow plane is NaN: the whole column is invisible
        st = set_lohi(case_store(H, W, 3, device=DEV), 1, ch, float("nan"), float("nan"))
        assert torch.isnan(st.result(1).flow[ch]).all()
        got = st.appearance(images, reference=ref, stack=True, fill=200)
        same(got, composition(st, None, images, ref, stack=True, fill=200), True)
        assert not got.visible[1].any() and (got.warped[1] == 200).all()
        two = st.appearance([images[0], images[2]], [0, 2], reference=ref)
        assert torch.equal(got.count, two.count) and torch.equal(bits(got.sum), bits(two.sum)) and torch.equal(bits(got.sumsq), bits(two.sumsq))
    for ch in (2, 3):                       # NaN occlusion, NaN sigma
        st = set_lohi(case_store(H, W, 3, device=DEV), 1, ch, float("nan"), float("nan"))
        got = st.appearance(images, reference=ref, stack=True)
        same(got, composition(st, None, images, ref, stack=True), True)
        assert not got.visible[1].any()
    st = set_lohi(case_store(H, W, 3, device=DEV), 2, 3, 0.5, float("inf"))                  # sigma +inf where its word is not 0, NaN where it is
    sigma = st.result(2).sigma[0]
    assert torch.isposinf(sigma).any() and torch.isnan(sigma).any()
    got = st.appearance(images, reference=ref, stack=True)
    same(got, composition(st, None, images, ref, stack=True), True)
    assert got.visible[2][torch.isposinf(sigma)].any() and not got.visible[2][torch.isnan(sigma)].any()
    bounded = st.appearance(images, reference=ref, stack=True, sigma_max=1e30)
    same(bounded, composition(st, None, images, ref, sigma_max=1e30, stack=True), True)
    assert not bounded.visible[2].any()
    flat = make_store(H, W, {0: const_planes(H, W), 1: const_planes(H, W, fx=2.5, fy=-1.25, occl=0.5, sigma=0.3), 2: field(3, H, W, 5.0)}, device=DEV)
    got = flat.appearance(images, reference=ref, stack=True, fill=1)
    same(got, composition(flat, None, images, ref, stack=True, fill=1), True)
    assert got.visible[0].all() and torch.equal(got.warped[0], images[0])                    # the identity sees the frame itself


# ---- 4. sentinels, repeatability -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,n,C", [(37, 53, 5, 3), (9, 17, 17, 4), (65, 130, 3, 1), (37, 53, 6, 2)])
def test_outputs_inside_sentinel_buffers(H, W, n, C):
    from mft_amd import atlas_ops, ops
    st = case_store(H, W, n, device=DEV)
    images, ref = dev_images(images_for(n, n, H, W, C)), dev_images(images_for(100 + n, 1, H, W, C))[0]
    want = composition(st, None, images, ref, stack=True, fill=200)
    fp, lp = ops.trackstore_slot_addresses(st._chunks, st._lohi, list(range(n)))
    px = H * W
    runs = []
    for _ in range(2):
        fbuf = torch.full((2 * C * px + 7,), -7.0, device=DEV)
        ibuf = torch.full((px + 5,), -7, dtype=torch.int32, device=DEV)
        bbuf = torch.full((n * px * C + n * px + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        total, totalsq = fbuf[3:3 + C * px].view(C, H, W), fbuf[4 + C * px:4 + 2 * C * px].view(C, H, W)
        count = ibuf[2:2 + px].view(H, W)
        warped = bbuf[3:3 + n * px * C].view(n, H, W, C)                                     # (an odd address: bytes need no alignment)
        visible = bbuf[8 + n * px * C:8 + n * px * C + n * px].view(n, H, W).view(torch.bool)
        atlas_ops.trackstore_appearance(fp, lp, images, ref, total, totalsq, count, warped, visible, fill=200)
        got = host_like(total, totalsq, count, warped, visible)
        same(got, want, True)
        for buf, spans, fillv in ((fbuf, [(0, 3), (3 + C * px, 4 + C * px), (4 + 2 * C * px, None)], -7.0), (ibuf, [(0, 2), (2 + px, None)], -7),
                                  (bbuf, [(0, 3), (3 + n * px * C, 8 + n * px * C), (8 + n * px * C + n * px, None)], 0xA5)):
            for a, b in spans:
                assert (buf[a:b] == fillv).all(), (a, b)
        runs.append([t.clone() for t in (total, totalsq, count, warped, visible.view(torch.uint8))])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else bits(a), b.view(torch.uint8) if b.dtype == torch.uint8 else bits(b))


class host_like:
    """The wrapper's outputs under the result object's names."""
    def __init__(self, total, totalsq, count, warped, visible):
        self.sum, self.sumsq, self.count, self.warped, self.visible = total, totalsq, count, warped, visible


def test_without_a_stack_nothing_else_is_written_and_no_columns_give_zeros():
    from mft_amd import atlas_ops, ops
    H, W, C = 9, 17, 3
    st = case_store(H, W, 4, device=DEV)
    images = dev_images(images_for(4, 4, H, W, C))
    got = st.appearance(images)
    same(got, composition(st, None, images), False)
    none = st.appearance([], [], stack=True)
    assert none.sum.is_cuda and not none.sum.any() and not none.count.any() and tuple(none.warped.shape) == (0, H, W, 1)
    total, totalsq, count = torch.full((C, H, W), -7.0, device=DEV), torch.full((C, H, W), -7.0, device=DEV), torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    atlas_ops.trackstore_appearance([], [], [], None, total, totalsq, count)
    assert not total.any() and not totalsq.any() and not count.any()
    fp, lp = ops.trackstore_slot_addresses(st._chunks, st._lohi, [0, 1, 2, 3])
    # the stack's two parts do not need each other
    want = composition(st, None, images, stack=True, fill=5)
    warped, visible = torch.full((4, H, W, C), 0xA5, dtype=torch.uint8, device=DEV), torch.zeros((4, H, W), dtype=torch.bool, device=DEV)
    atlas_ops.trackstore_appearance(fp, lp, images, None, total, totalsq, count, warped=warped, fill=5)
    assert torch.equal(warped, want[3]) and torch.equal(count, want[2]) and torch.equal(bits(total), bits(want[0]))
    atlas_ops.trackstore_appearance(fp, lp, images, None, total, totalsq, count, visible=visible, fill=5)
    assert torch.equal(visible, want[4]) and torch.equal(count, want[2]) and torch.equal(bits(totalsq), bits(want[1]))
    with pytest.raises(atlas_ops.MftxError):
        atlas_ops.trackstore_appearance(fp, lp, images[:3], None, total, totalsq, count)
    with pytest.raises(atlas_ops.MftxError):
        atlas_ops.trackstore_appearance(fp, lp, [i.cpu() for i in images], None, total, totalsq, count)


# ---- 5. against the host store -------------------------------------------------------------------------------------------------------
# What the device's sampler and torch's CPU grid_sample differ by, measured on the MI355X over the cases below (the largest
# |difference| of sum / max(count, 1) and of sumsq / max(count, 1), printed by the test), and what is accepted: 4 x that, the margin
# for another torch build's CPU grid_sample -- the cases are deterministic.
# Measured: 4.58e-5 levels (3 * 2^-16, from 37 x 53 up) and 0.0156 levels^2 (2^-6, from 37 x 53 up, in the cases without a reference:
# sums of squares of samples up to 255, i.e. 2.4e-7 of 65025; 0.0117 with one).  Accepted: 1.83e-4 and 0.0625.
MEASURED_MEAN, MEASURED_MEANSQ = 3 * 2.0 ** -16, 2.0 ** -6
ACCEPT_MEAN, ACCEPT_MEANSQ = 4 * MEASURED_MEAN, 4 * MEASURED_MEANSQ
WARPED_SHARE = 1e-3              # of the visible bytes may differ, by one level


@pytest.mark.parametrize("H,W", SIZES)
def test_device_against_host_store(H, W):
    """count and visible are EQUAL; warped differs by at most one level on at most 0.1 % of the visible bytes (measured: 0, 0, 0, 2,
    4 and 12 bytes of 272 .. 5.4 M, at most 0.0003 %); the per-pixel means of d and d * d are within ACCEPT_MEAN / ACCEPT_MEANSQ = 4 x
    the largest difference measured on the MI355X over the cases of the bitwise test, with and without a reference, fill and
    sigma_max, the stack on: 4.58e-5 -> 1.83e-4 levels and 0.0156 -> 0.0625 levels^2."""
    worst = [0.0, 0.0]
    differing = seen = 0
    for n in COLUMNS:
        dev, cpu = case_store(H, W, n, device=DEV), case_store(H, W, n)
        for k in range(n):
            assert torch.equal(dev.packed(k).view(torch.int16).cpu(), cpu.packed(k).view(torch.int16)) and torch.equal(bits(dev.lohi(k)).cpu(), bits(cpu.lohi(k)))
        for C in CHANNELS:
            images, ref = images_for(n, n, H, W, C), images_for(100 + n, 1, H, W, C)[0]
            for with_ref, _, fill, smax in OPTIONS:                       # (the stack on in all four: warped and visible are compared)
                reference = ref if with_ref else None
                got = dev.appearance(images, reference=reference, sigma_max=smax, stack=True, fill=fill)
                want = cpu.appearance(images, reference=reference, sigma_max=smax, stack=True, fill=fill)
                assert torch.equal(got.count.cpu(), want.count) and torch.equal(got.visible.cpu(), want.visible)
                per = want.count.clamp(min=1).to(torch.float32)
                worst[0] = max(worst[0], float((got.sum.cpu() / per - want.sum / per).abs().max()))
                worst[1] = max(worst[1], float((got.sumsq.cpu() / per - want.sumsq / per).abs().max()))
                diff = (got.warped.cpu().to(torch.int32) - want.warped.to(torch.int32)).abs()
                assert int(diff.max()) <= 1
                differing += int(diff.sum())
                seen += int(want.visible.sum()) * C
    print(f"{H}x{W}: device and host differ by at most {worst[0]:.3g} in sum / count and {worst[1]:.3g} in sumsq / count "
          f"(accepted: {ACCEPT_MEAN}, {ACCEPT_MEANSQ}); warped differs on {differing} of {seen} visible bytes ({differing / max(seen, 1):.3%})")
    assert differing <= WARPED_SHARE * seen
    assert worst[0] <= ACCEPT_MEAN and worst[1] <= ACCEPT_MEANSQ


# ---- 6. through the engine -----------------------------------------------------------------------------------------------------------
def test_appearance_of_a_tracker_pass():
    from mft_amd.synth import SyntheticVideo
    from test_gpu_trackstore import _config
    H, W = 128, 160
    video = SyntheticVideo(H, W, n_frames=6, seed=21)
    conf = _config(1, track_store=True)
    tracker = conf.tracker_class(conf)
    for k in range(len(video)):
        tracker.init(video[0]) if k == 0 else tracker.track(video[k])
    st = tracker.track_store
    assert len(st) == 6 and st.frame_ids == list(range(6))
    frames = [video[k] for k in range(6)]
    got = st.appearance(frames, reference=frames[0], stack=True)
    images = dev_images(frames)
    same(got, composition(st, None, images, images[0], stack=True), True)
    assert int(got.count.min()) >= 1                       # the template frame's identity result sees itself
    assert got.visible[0].all() and torch.equal(got.warped[0], images[0])
    rms = float(got.var.sqrt()[got.count > 1].mean())
    print(f"tracker pass: count {int(got.count.min())} .. {int(got.count.max())}, mean photometric deviation {rms:.3g} levels")


# ---- 7. argument errors ---------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_writes_nothing():
    from mft_amd import _lib, ops
    lib = _lib.load()
    H, W, C, n = 9, 17, 3, 3
    st = case_store(H, W, n, device=DEV)
    images = torch.stack(dev_images(images_for(1, n, H, W, C)))
    fp, lp = ops.trackstore_slot_addresses(st._chunks, st._lohi, [0, 1, 2])
    ip = images.data_ptr() + np.arange(n, dtype=np.int64) * (H * W * C)
    up, (frames, lohis, imgs) = ops._upload_tables(torch.device(DEV), (fp, lp, ip), ())
    outs = {"sum": torch.full((C, H, W), -7.0, device=DEV), "sumsq": torch.full((C, H, W), -7.0, device=DEV),
            "count": torch.full((H, W), -7, dtype=torch.int32, device=DEV), "warped": torch.full((n, H, W, C), 0xA5, dtype=torch.uint8, device=DEV),
            "visible": torch.full((n, H, W), 0xA5, dtype=torch.uint8, device=DEV)}
    before = {k: v.clone() for k, v in outs.items()}
    valid = dict(frames=frames, lohis=lohis, images=imgs, T=n, C=C, H=H, W=W, reference=None, thr=0.5, smax=float("inf"), fill=0,
                 **{k: v.data_ptr() for k, v in outs.items()})
    order = ("frames", "lohis", "images", "T", "C", "H", "W", "reference", "thr", "smax", "fill", "sum", "sumsq", "count", "warped", "visible")

    def call(**kw):
        a = dict(valid, **kw)
        return lib.mftx_trackstore_appearance(*[a[k] for k in order], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    err = lib.mftx_last_error_string
    E_ARG, E_ALIGN = -1, -2
    refused = [dict(frames=None), dict(lohis=None), dict(images=None), dict(sum=None), dict(sumsq=None), dict(count=None), dict(C=0), dict(C=5), dict(H=1), dict(W=1), dict(H=65536, W=32768), dict(fill=-1), dict(fill=256), dict(T=-1)]
    for kw in refused:
        assert call(**kw) == E_ARG and b"trackstore_appearance" in err(), kw
    assert call(H=65536, W=32768) == E_ARG and b"2^31" in err()
    assert call(C=5) == E_ARG and b"channels" in err() and call(fill=256) == E_ARG and b"fill" in err()
    for kw in (dict(frames=frames + 4), dict(lohis=lohis + 4), dict(images=imgs + 4), dict(sum=valid["sum"] + 2), dict(count=valid["count"] + 1)):
        assert call(**kw) == E_ALIGN and b"aligned" in err(), kw
    assert call(T=0) == 0 and call(T=0, frames=None, sum=None) == 0                             # no columns: a no-op
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, before[k]), k
    assert call() == 0                                                                         # ... and the valid call does write
    torch.cuda.synchronize()
    assert not any(torch.equal(v, before[k]) for k, v in outs.items())


# ---- 8. stream ordering ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


@pytest.fixture(scope="module")
def cycles_per_ms():
    return sh.calibrate()


APPEARANCE_C = 3


def _appearance_fixed(ops):
    return {"reference": torch.from_numpy(images_for(40, 1, cat.HF, cat.WF, APPEARANCE_C)[0]).to(DEV)}


def _appearance_inputs(ops, seed):
    """The store's chunks and the video as payload."""
    out = cat._store(ops, seed)
    out["images"] = torch.from_numpy(np.stack(images_for(50 + seed, 3, cat.HF, cat.WF, APPEARANCE_C))).to(DEV)
    return out


def _appearance_call(ops, fx, inp, v=0):
    from mft_amd import atlas_ops
    slots = np.asarray(cat.SLOTS[v])                       # the columns of the first and of the second call behind one stall
    frame_ptrs, lohi_ptrs = ops.trackstore_slot_addresses(*cat._chunks(inp), slots)
    n = int(slots.shape[0])
    images = inp["images"] if v == 0 else [inp["images"][k] for k in (2, 0, 1)]
    outs = atlas_ops.trackstore_appearance(frame_ptrs, lohi_ptrs, images, fx["reference"], torch.full((APPEARANCE_C, cat.HF, cat.WF), -7.0, device=DEV),
                                           torch.full((APPEARANCE_C, cat.HF, cat.WF), -7.0, device=DEV),
                                           torch.full((cat.HF, cat.WF), -7, dtype=torch.int32, device=DEV),
                                           torch.full((n, cat.HF, cat.WF, APPEARANCE_C), 7, dtype=torch.uint8, device=DEV),
                                           torch.zeros((n, cat.HF, cat.WF), dtype=torch.bool, device=DEV), fill=200)
    return list(outs)


APPEARANCE_ENTRY = cat.Entry("trackstore_appearance", ("trackstore_appearance",), _appearance_fixed, _appearance_inputs, _appearance_call, True, None)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("variants", [(0,), (0, 1)], ids=["one call", "table uploads back to back"])
def test_appearance_runs_on_its_stream(ops, cycles_per_ms, variants):
    run_behind_stall(ops, APPEARANCE_ENTRY, cycles_per_ms, variants=variants)
