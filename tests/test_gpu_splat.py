"""csrc/splat.hip on the GPU: the integer forward splat (``FlowOUTrackingResult.warp_forward_device``), the edit and point
overlays and ``vis.DeviceOverlay``, bit for bit against the numpy restatements of tests/test_splat.py (and through them
against the reference's own ``warp_forward`` outputs and the host overlay path)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import golden_inputs as gi
import test_splat as ts
from mft_amd import ops, vis
from mft_amd import video as vio
from mft_amd.results import FlowOUTrackingResult

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def result_of(flow, occl=None):
    _, H, W = flow.shape
    occl = np.zeros((1, H, W), F32) if occl is None else occl.reshape(1, H, W)
    return FlowOUTrackingResult(T(flow), T(occl), torch.zeros(1, H, W, device=DEV), validate=False)


def check_splat(flow, img, mask=None, border=None, bound=None):
    """device == restatement, bit for bit; returns the device output as numpy"""
    want, _, _ = ts.splat_forward(flow, img, mask=mask, border=border, bound=bound)
    got = result_of(flow).warp_forward_device(T(img), mask=None if mask is None else T(mask), border=border, value_bound=bound)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == img.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want)), float((got.cpu() - torch.from_numpy(want)).abs().max())
    return got.cpu().numpy()


def smooth_case(H, W, seed, C=3):
    r = gi._rng(83, seed)
    flow = gi.smooth_field(r, 2, H, W, cells=3, amp=4.0).astype(F32)
    flow[:, :, : max(1, W // 8)] -= 6.0
    return flow, r.random((H, W, C)).astype(F32), r.random((H, W)) < 0.7


def grid(H, W):
    gy, gx = np.mgrid[0:H, 0:W]
    return np.stack([gx, gy]).astype(F32)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("border", [None, -1.0])
def test_warp_forward_device_golden_inputs(golden_dir, masked, border):
    d = gi.results_api_inputs()
    out = check_splat(d["flow"], d["img"], mask=d["mask"] if masked else None, border=border)
    g = np.load(golden_dir / "results_api.npz")
    if not masked and border is None:
        assert np.allclose(out, g["warp_forward"], atol=1e-5)
    if masked and border == -1.0:
        assert np.allclose(out, g["warp_forward_masked"], atol=1e-5)
    if not masked and border is None:          # a value bound given: the same fixed point here (k = 0 or 1 leave V = 23), no read-back
        check_splat(d["flow"], d["img"], bound=1.0)


@pytest.mark.parametrize("H,W", [(61, 67), (3, 5), (1, 1)])
def test_warp_forward_device_sizes(H, W):
    """61 x 67: W no multiple of 64, H * W odd, more than one block; 3 x 5; 1 x 1: every weight is 0, nothing is hit"""
    flow, img, mask = smooth_case(H, W, H)
    if (H, W) == (3, 5):
        flow = (flow * 0.2).astype(F32)
    out = check_splat(flow, img)
    check_splat(flow, img, mask=mask, border=2.5)
    check_splat(flow, img[..., :1])
    check_splat(flow, (img * 255).astype(np.uint8), mask=mask)               # integer values: V = 0
    if (H, W) == (1, 1):
        assert not out.any()


def contracting(H=40, W=56):
    g = grid(H, W)
    centre = np.array([(W - 1) / 2, (H - 1) / 2], F32).reshape(2, 1, 1)
    return (F32(-0.5) * (g - centre)).astype(F32)


def test_warp_forward_device_many_sources_per_destination():
    H, W = 40, 56
    r = gi._rng(84)
    img = (r.random((H, W, 3)) * 8 - 4).astype(F32)                           # signed values: two's complement sums
    out = check_splat(contracting(H, W), img)
    assert (out == 0).all(-1).mean() > 0.5                                   # the frame shrank to its middle quarter
    # all 2240 pixels to ONE integer location: one address, 2240 adds of weight 1; the output is the integer mean
    tx, ty = 20, 17
    flow = (np.array([tx, ty], F32).reshape(2, 1, 1) - grid(H, W)).astype(F32)
    vals = r.integers(0, 256, size=(H, W, 2))
    for img in (vals.astype(F32), vals.astype(np.uint8)):
        out = check_splat(flow, img)
        want = np.zeros((H, W, 2), F32)
        want[ty, tx] = (vals.reshape(-1, 2).sum(0).astype(np.float64) / (H * W)).astype(F32)
        assert np.array_equal(out, want)


def test_warp_forward_device_nonfinite_flow():
    H, W = 61, 67
    flow, img, _ = smooth_case(H, W, 5)
    bad = flow.copy()
    spots = [(0, 3, 4, np.nan), (1, 10, 11, np.inf), (0, 20, 30, -np.inf), (1, 60, 66, np.nan), (0, 33, 0, np.inf), (1, 33, 0, -np.inf)]
    finite = np.ones((H, W), bool)
    for c, y, x, v in spots:
        bad[c, y, x] = v
        finite[y, x] = False
    out = check_splat(bad, img)
    # those pixels contribute nothing and the rest is unchanged: the same as masking them out of the clean flow
    assert np.array_equal(out, check_splat(flow, img, mask=finite))
    assert np.isfinite(out).all()


def test_splat_is_bitwise_reproducible():
    H, W = 40, 56
    img = T((gi._rng(85).random((H, W, 3)) * 3).astype(F32))
    res = result_of(contracting(H, W))
    first = res.warp_forward_device(img, value_bound=3.0)
    for _ in range(19):
        assert torch.equal(res.warp_forward_device(img, value_bound=3.0), first)


def test_native_path_refuses_without_enough_bits():
    from mft_amd._lib import MftxError
    flow, img, _ = smooth_case(3, 5, 1)
    with pytest.raises(MftxError, match="warp_forward"):
        result_of(flow).warp_forward_device(T(img), value_bound=2.0 ** 40)      # k = 41: V < 12
    with pytest.raises(MftxError):
        ops.splat_forward(T(flow), T(img)[:2], 1.0)


# ---------------------------------------------------------------------------
# overlays
# ---------------------------------------------------------------------------

def device_edit(c):
    H, W = c["frame"].shape[:2]
    acc = ops.splat_accumulator(4, H, W, DEV)
    out = ops.overlay_edit(T(c["flow"]), T(c["occl"].reshape(1, H, W)), T(c["edit"]), T(c["frame"]), acc,
                           ops.edit_alpha_divisor(c["edit"]))
    assert not acc.any()                                           # cleared behind the composite
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W,seed", ts.OVERLAY_CASES)
def test_overlay_edit_seeded_cases(H, W, seed):
    c = ts.overlay_case(H, W, seed)
    got = device_edit(c)
    assert np.array_equal(got, ts.overlay_edit(c["flow"], c["occl"], c["edit"], c["frame"]))
    nan = dict(c, occl=c["occl"].copy())
    nan["occl"][0, 5:9, 5:30] = np.nan                             # a NaN occlusion is masked out
    assert np.array_equal(device_edit(nan), ts.overlay_edit(nan["flow"], nan["occl"], nan["edit"], nan["frame"]))


def test_overlay_edit_zero_flow_and_alpha_quirk():
    H, W = 40, 56
    frame = np.random.default_rng(2).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    edit = np.zeros((H, W, 4), np.uint8)
    edit[5:15, 8:20] = (40, 80, 120, 255)
    occl = np.zeros((1, H, W), F32)
    occl[0, 5:8, 8:12] = 1.0
    c = dict(flow=np.zeros((2, H, W), F32), occl=occl, edit=edit, frame=frame)
    out = device_edit(c)
    gray = vis.to_gray_3ch(frame)
    assert np.array_equal(out, ts.overlay_edit(c["flow"], occl, edit, frame))
    assert tuple(out[10, 10]) == (40, 80, 120)
    assert np.array_equal(out[6, 9], gray[6, 9]) and np.array_equal(out[30, 30], gray[30, 30])
    inside = np.zeros((H, W), bool)
    inside[5:15, 8:20] = True
    inside[5:8, 8:12] = False
    assert np.array_equal(out[~inside], gray[~inside])
    # every non-zero alpha equal to 1: the blend does not rescale alpha (divisor 1), the edit is opaque
    c2 = ts.overlay_case(H, W, 3)
    c2["edit"][..., 3] = np.minimum(c2["edit"][..., 3], 1)
    assert ops.edit_alpha_divisor(c2["edit"]) == 1.0 and ops.edit_alpha_divisor(c["edit"]) == 255.0
    got = device_edit(c2)
    assert np.array_equal(got, ts.overlay_edit(c2["flow"], c2["occl"], c2["edit"], c2["frame"]))
    res = FlowOUTrackingResult(torch.from_numpy(c2["flow"]), torch.from_numpy(c2["occl"]), torch.zeros(1, H, W))
    assert ts.within_one_level(got, vis.draw_edit(c2["frame"], res, c2["edit"]))[2]


@pytest.mark.parametrize("radius", [3, 2.5])
def test_overlay_dots_matches_draw_dots(radius):
    H, W = 40, 56
    frame = np.random.default_rng(4).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rows = [(10.0, 12.0, 0.0), (30.4, 20.6, 0.9), (-50.0, 3.0, 0.0), (55.0, 39.0, 0.2),      # visible, occluded, far outside, corner
            (np.nan, 5.0, 0.0), (20.0, np.inf, 0.0),                                        # not finite
            (10.5, 30.5, 0.0), (11.5, 20.5, 0.1), (42.5, 0.5, 0.5),                         # half-integers: round half even
            (40.0, 25.0, 0.0), (42.3, 26.8, 0.0),                                           # two overlapping dots
            (0.2, 38.9, 0.0), (3.0e9, 1.0, 0.0), (17.49999, 9.50001, np.nan)]
    table = np.array([r + (0.3,) for r in rows], F32)
    want = vis.draw_dots(frame, table[:, :2], table[:, 2], radius=radius)
    got = ops.overlay_dots(T(frame), T(table), radius=radius)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != frame).any(-1).sum() > 100
    fr = T(frame)
    assert ops.overlay_dots(fr, T(table), radius=radius, out=fr) is fr and np.array_equal(fr.cpu().numpy(), want)     # in place
    assert np.array_equal(ops.overlay_dots(T(frame), torch.zeros(0, 4, device=DEV)).cpu().numpy(), frame)          # no points


def test_device_overlay_clears_behind_itself():
    H, W = 61, 67
    a, b = ts.overlay_case(H, W, 1), ts.overlay_case(H, W, 2)
    q = vis.get_queries((H, W), 9)
    ov = vis.DeviceOverlay(a["edit"], q, H, W)
    outs = []
    for c in (a, b):
        pts, ed = ov.render(c["frame"], result_of(c["flow"], c["occl"]))
        outs.append((pts.clone(), ed.clone()))
    for c, (pts, ed) in zip((a, b), outs):
        fresh = vis.DeviceOverlay(a["edit"], q, H, W).render(c["frame"], result_of(c["flow"], c["occl"]))
        assert torch.equal(pts, fresh[0]) and torch.equal(ed, fresh[1])
        assert np.array_equal(ed.cpu().numpy(), ts.overlay_edit(c["flow"], c["occl"], a["edit"], c["frame"]))
    done = ov.download(wait=True)
    assert len(done) == 2 and ov.pending() == 0
    for (pts, ed), (hp, he) in zip(outs, done):
        assert np.array_equal(hp, pts.cpu().numpy()) and np.array_equal(he, ed.cpu().numpy())


def test_device_overlay_end_to_end():
    """Four 128 x 160 synthetic frames, stand-in weights: the point frames are draw_dots on the downloaded tracks, the edit
    frames draw_edit on the downloaded results up to its uint8 truncation (1 level, at most 0.5 % of the values)."""
    from mft_amd.config import load_config
    from mft_amd.synth import SyntheticVideo
    repo = Path(__file__).resolve().parents[1]
    conf = load_config(repo / "configs" / "MFT_cfg.py")
    conf.flow_config.model = None
    conf.flow_config.synthetic_weights_seed = 7
    conf.flow_config.flow_iters = 4
    conf.deltas = [np.inf, 1, 2]
    conf.keep_result_on_device = True
    tracker = conf.tracker_class(conf)
    H, W = 128, 160
    vid = SyntheticVideo(H, W, n_frames=4, seed=1)
    r = gi._rng(98)
    edit = np.zeros((H, W, 4), np.uint8)
    edit[30:90, 40:120] = r.integers(0, 256, size=(60, 80, 4), dtype=np.uint8)
    edit[..., 3][r.random((H, W)) < 0.25] = 0
    ov = vis.DeviceOverlay(edit, vis.get_queries((H, W), 16), H, W)
    kept = []
    for i in range(4):
        meta = tracker.init(vid[i]) if i == 0 else tracker.track(vid[i])
        res = meta.result.cuda() if i == 0 else meta.result
        assert res.flow.is_cuda
        ov.render(vid[i], res)
        kept.append(res.clone())
    done = ov.download(wait=True, tracks=True)
    assert len(done) == 4
    for i, (pts, ed, tracks) in enumerate(done):
        assert pts.dtype == np.uint8 and pts.shape == (H, W, 3) and tracks.shape == (80, 4)
        assert np.array_equal(pts, vis.draw_dots(vid[i], tracks[:, :2], tracks[:, 2]))
        worst, frac, ok = ts.within_one_level(ed, vis.draw_edit(vid[i], kept[i].cpu(), edit))
        print(f"frame {i}: max {worst} level(s), {100 * frac:.4f} % of the values differ")
        assert ok, (i, worst, frac)
    assert (done[0][0] == np.array(vis.RED, np.uint8)).all(-1).sum() > 100
    assert (done[0][1] != vis.to_gray_3ch(vid[0])).any(-1).sum() > 1000         # frame 0: the edit where it was painted


def test_demo_gpu_overlays_on_png_directory(tmp_path):
    from mft_amd.synth import SyntheticVideo
    repo = Path(__file__).resolve().parents[1]
    vid = SyntheticVideo(128, 160, n_frames=4, seed=1)
    for i in range(4):
        vio.imwrite_bgr(tmp_path / "in" / f"{i:03d}.png", vid[i])
    edit = np.zeros((128, 160, 4), np.uint8)
    edit[30:50, 40:70] = (0, 255, 255, 200)
    vio.imwrite_bgr(tmp_path / "edit.png", edit)
    res = subprocess.run([sys.executable, str(repo / "demo.py"), "--video", str(tmp_path / "in"), "--edit", str(tmp_path / "edit.png"),
                          "--out", str(tmp_path / "out"), "--synthetic_weights_seed", "7", "--grid_spacing", "16", "--gpu-overlays"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    pts = sorted((tmp_path / "out" / "in_points").glob("*.png"))
    eds = sorted((tmp_path / "out" / "in_edit").glob("*.png"))
    assert len(pts) == 4 and len(eds) == 4
    first = vio.imread_bgr(pts[0])
    assert first.shape == (128, 160, 3) and (first == np.array(vis.RED, np.uint8)).all(-1).sum() > 100
    assert (vio.imread_bgr(eds[0])[30:50, 40:70] != vis.to_gray_3ch(vid[0])[30:50, 40:70]).any()
