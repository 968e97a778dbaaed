"""``DenseTrackStore.inverse`` / ``results_from`` on the device (csrc/trackstore.hip: ts_atlas_scatter_kernel,
ts_atlas_resolve_kernel in their identity mode through ``ops.trackstore_invert``) against the host restatement (mft_amd/trackstore.py, device="cpu":
``locate`` at every pixel centre), bit for bit; the fields are those of tests/test_track_locate.py and tests/test_track_inverse.py."""
import functools

import numpy as np
import pytest
import torch

import test_track_inverse as inv
import test_track_locate as host
from mft_amd.synth import SyntheticVideo
from test_gpu_track_locate import _config, assert_same, bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAME_IDS = host.FRAME_IDS
TOL = host.TOL


def both(H, W, frames, **kw):
    return host.make_store(H, W, frames, device=DEV, **kw), host.make_store(H, W, frames, **kw)


@functools.lru_cache(maxsize=None)
def smooth(H, W, amp):
    """(device store, host store, the host's inverse of the three frames in one call)."""
    dev, cpu = both(H, W, host.smooth_frames(H, W, amp))
    return dev, cpu, cpu.inverse(list(FRAME_IDS))


def check_frames(dev, cpu, ids, thr=0.5):
    """Each frame alone and all of them in one call; -> the host's (table, cell) of the joint call."""
    want = cpu.inverse(list(ids), occlusion_threshold=thr)
    got = dev.inverse(list(ids), occlusion_threshold=thr)
    assert got[0].is_cuda and got[0].shape == (len(ids), dev.H, dev.W, 4) and got[1].dtype == torch.int32
    assert_same((got[0].reshape(-1, 4), got[1].reshape(-1)), (want[0].reshape(-1, 4), want[1].reshape(-1)))
    for k, f in enumerate(ids):
        one = dev.inverse(f, occlusion_threshold=thr)
        assert one[0].shape == (dev.H, dev.W, 4) and one[1].shape == (dev.H, dev.W)
        assert_same((one[0].reshape(-1, 4), one[1].reshape(-1)), (want[0][k].reshape(-1, 4), want[1][k].reshape(-1)))
    return want


# ---- 1. smooth fields: ragged tiles in both directions -----------------------------------------------------------------------
@pytest.mark.parametrize("amp", [1.5, 5.0])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_inverse_is_the_host_restatement_bitwise(H, W, amp):
    dev, cpu, want = smooth(H, W, amp)
    got = dev.inverse(list(FRAME_IDS))
    assert got[0].is_cuda and got[0].shape == (3, H, W, 4) and got[1].shape == (3, H, W) and got[1].dtype == torch.int32
    assert_same((got[0].reshape(-1, 4), got[1].reshape(-1)), (want[0].reshape(-1, 4), want[1].reshape(-1)))
    for k, f in enumerate(FRAME_IDS):
        one = dev.inverse(f)
        assert one[0].shape == (H, W, 4) and one[1].shape == (H, W)
        assert_same((one[0].reshape(-1, 4), one[1].reshape(-1)), (want[0][k].reshape(-1, 4), want[1][k].reshape(-1)))
    found = (want[1] >= 0).float().mean().item()
    assert found > 0.8 and (amp == 1.5 or int((want[1] < 0).sum()) > 300)           # both kinds of answer are exercised


# ---- 2. cells that the wave walks together, on a smooth field ----------------------------------------------------------------
def test_large_boxes_of_a_smooth_field():
    H, W = 24, 40
    dev, cpu = both(H, W, {0: host.field(0, H, W, 12.0)})
    walked, inside = inv.box_counts(cpu, 0)
    assert (inside > inv.INLINE).sum() > 50 and (walked > inv.INLINE).sum() >= (inside > inv.INLINE).sum()
    want = check_frames(dev, cpu, [0])
    assert 100 < int((want[1] >= 0).sum()) < H * W


# ---- 3. torn cells -----------------------------------------------------------------------------------------------------------
def test_torn_cells_cover_much_of_the_frame():
    H, W = 37, 53
    dev, cpu = both(H, W, {0: inv.torn_planes(), 6: host.field(437, H, W, 1.5)})
    walked, inside = inv.box_counts(cpu, 0)
    assert (inside > 64).sum() == 12 and inside.max() == 770
    want = check_frames(dev, cpu, [0, 6])
    assert int((want[1][0] >= 0).sum()) == 1921


# ---- 4. choice frames, nothing mapped, degenerate shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.5, 1.0])
def test_choice_rule_on_the_device(thr):
    H, W = host.CHOICE_HW
    dev, cpu = both(H, W, host.choice_frames())
    walked, _ = inv.box_counts(cpu, 1)
    assert walked.max() > inv.INLINE                                                # the seam cells: phase two decides a choice too
    want = check_frames(dev, cpu, [0, 1, 2], thr)
    assert int((want[1][1] >= 0).sum()) == 1120 and int((want[1][2] >= 0).sum()) == 1120


def test_shifted_out_frame_on_the_device():
    H, W = 40, 56
    dev, cpu = both(H, W, {7: host.shifted_out_planes(H, W), 2: host.field(1, H, W, 1.5)})
    got = dev.inverse(7)
    assert (got[1] == -1).all() and (bits(got[0]) == 0x7fc00000).all()
    check_frames(dev, cpu, [7, 2])


@pytest.mark.parametrize("H,W", [(2, 2), (2, 70), (70, 2)])
def test_degenerate_shapes(H, W):
    """One cell, one row of cells (three ragged tiles), one column of cells (nine tiles of one cell column)."""
    dev, cpu = both(H, W, {1: host.field(5, H, W, 1.5), 0: host.const_planes(H, W)})
    want = check_frames(dev, cpu, [1, 0])
    assert (want[1][1] >= 0).all()


# ---- 5. chunks ---------------------------------------------------------------------------------------------------------------
def test_frames_of_three_chunks_in_one_call():
    H, W = 37, 53
    frames = {f: host.field(k, H, W, 5.0 if k % 2 else 1.5) for k, f in enumerate((20, 21, 22, 23, 24))}
    dev, cpu = both(H, W, frames, frames_per_chunk=2)
    assert len(dev._chunks) == 3
    check_frames(dev, cpu, [24, 21, 22, 20])                                        # chunks 2, 0, 1 and 0 again


# ---- 6. reproducibility, untouched memory ------------------------------------------------------------------------------------
def test_same_bits_every_time_and_nothing_else_written():
    H, W = 37, 53
    dev, cpu, want = smooth(H, W, 5.0)
    want = (want[0].reshape(-1, 4), want[1].reshape(-1))
    ids = list(FRAME_IDS)
    big_t = torch.full((5, H, W, 4), -7.0, device=DEV)
    big_c = torch.full((5, H, W), -77, dtype=torch.int32, device=DEV)
    out = (big_t[1:4], big_c[1:4])
    for _ in range(5):
        again = dev.inverse(ids, out=out)
        assert again[0] is out[0] and again[1] is out[1]
        assert_same((out[0].reshape(-1, 4), out[1].reshape(-1)), want)
    assert (big_t[0] == -7).all() and (big_t[4] == -7).all() and (big_c[0] == -77).all() and (big_c[4] == -77).all()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = dev.inverse(ids)
    s.synchronize()
    assert_same((other[0].reshape(-1, 4), other[1].reshape(-1)), want)
    with pytest.raises(ValueError):
        dev.inverse(ids, out=(big_t[1:4], big_c[1:4].cpu()))
    with pytest.raises(ValueError):
        dev.inverse(ids, out=(torch.empty((3, H, W, 8), device=DEV)[..., :4], big_c[1:4]))       # not contiguous
    with pytest.raises(KeyError):
        dev.inverse([3, 99])


# ---- 7. results_from on the device -------------------------------------------------------------------------------------------
def test_results_from_on_the_device():
    H, W = 37, 53
    dev, cpu, _ = smooth(H, W, 5.0)
    src = 8
    flow, occl, sigma, found = dev.results_from(src)
    assert flow.is_cuda and flow.shape == (3, 2, H, W) and occl.shape == (3, 1, H, W) and sigma.shape == (3, 1, H, W)
    assert found.shape == (H, W) and found.dtype == torch.bool
    hf, ho, hs, hfound = cpu.results_from(src)
    table, cell = dev.inverse(src)
    assert_same((table.reshape(-1, 4), cell.reshape(-1)), tuple(t.reshape(-1, *t.shape[2:]) for t in cpu.inverse(src)))
    assert torch.equal(found.cpu(), hfound) and 100 < int((~hfound).sum())
    # against the host store's: what the device's sampler and torch's differ by (tests/test_gpu_trackstore.py, device vs host query)
    for name, got, want, tol in (("flow", flow, hf, 1e-5), ("occlusion", occl, ho, 1e-6), ("sigma", sigma, hs, 1e-6)):
        err = float((got.cpu()[:, :, hfound] - want[:, :, hfound]).abs().max())
        print(f"{name}: device and host differ by at most {err:.3g}")
        assert err <= tol
        assert torch.equal(bits(got)[:, :, ~hfound], bits(want)[:, :, ~hfound])      # NaN, 1 and +inf where nothing is found
    # bitwise the composition rule on the device's own inverse and query
    template = torch.where(cell.reshape(-1, 1) >= 0, table.reshape(-1, 4)[:, 0:2], torch.zeros((), device=DEV))
    want = inv.composed(table.cpu().numpy(), cell.cpu().numpy(), dev.query(template).cpu().numpy())
    for got, w in zip((flow, occl, sigma), want[:3]):
        assert np.array_equal(bits(got).numpy(), w.view(np.int32))
    assert np.array_equal(found.cpu().numpy(), want[3])
    r, f2 = dev.result_from(src, 5)
    assert torch.equal(bits(r.flow), bits(flow[2])) and torch.equal(bits(r.sigma), bits(sigma[2])) and torch.equal(f2, found)


# ---- 8. through the tracker --------------------------------------------------------------------------------------------------
def test_a_mid_video_frame_inverted_through_the_tracker():
    H, W, t = 128, 160, 3
    video = SyntheticVideo(H, W, n_frames=6, seed=21)
    tracker = _config(1).tracker_class(_config(1))
    for k in range(len(video)):
        tracker.init(video[0]) if k == 0 else tracker.track(video[k])
    st = tracker.track_store
    assert len(st) == 6 and st.frame_ids == list(range(6))
    cpu = host.make_store(H, W, {})
    cpu._chunks, cpu._lohi = [c.cpu() for c in st._chunks], [l.cpu() for l in st._lohi]
    cpu.frame_ids, cpu._slot_of = list(st.frame_ids), dict(st._slot_of)
    got, want = st.inverse(t), cpu.inverse(t)
    assert_same((got[0].reshape(-1, 4), got[1].reshape(-1)), (want[0].reshape(-1, 4), want[1].reshape(-1)))
    r, found = st.result_from(t, t)
    visible = found & (r.occlusion[0] < 0.5)
    print(f"{int(found.sum())} of {H * W} pixels found, {int(visible.sum())} of them stored as visible")
    assert int(visible.sum()) > 0
    err = float(r.flow[:, visible].abs().max())
    print(f"    the flow from frame {t} to itself is within {err:.3g} px of zero")
    assert err <= TOL


# ---- 9. the demo with the edit painted on a later frame ----------------------------------------------------------------------
def test_demo_with_the_edit_given_on_a_later_frame(tmp_path):
    """demo.py --track-store --edit-frame 2: on frame 2 itself the edit sits where it was painted, elsewhere the frame stays gray."""
    import subprocess
    import sys
    from pathlib import Path
    from mft_amd import video as vio
    repo = Path(__file__).resolve().parents[1]
    vid = SyntheticVideo(128, 160, n_frames=4, seed=1)
    for i in range(4):
        vio.imwrite_bgr(tmp_path / "in" / f"{i:03d}.png", vid[i])
    edit = np.zeros((128, 160, 4), np.uint8)
    edit[30:50, 40:70] = (0, 255, 255, 200)                                          # B, G, R, A
    vio.imwrite_bgr(tmp_path / "edit.png", edit)
    res = subprocess.run([sys.executable, str(repo / "demo.py"), "--video", str(tmp_path / "in"), "--edit", str(tmp_path / "edit.png"),
                          "--out", str(tmp_path / "out"), "--synthetic_weights_seed", "7", "--track-store", "--edit-frame", "2"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    eds = sorted((tmp_path / "out" / "in_edit").glob("*.png"))
    assert len(eds) == 4
    at = vio.imread_bgr(eds[2]).astype(np.int32)
    tinted = at[:, :, 2] - at[:, :, 0] > 50                                          # red well above blue: the edit's colour over gray
    print(f"frame 2: {int(tinted[32:48, 42:68].sum())} of {16 * 26} pixels inside the painted box carry the edit, "
          f"{int(tinted.sum() - tinted[28:52, 38:72].sum())} outside it")
    assert tinted[32:48, 42:68].mean() > 0.5 and not tinted[:24].any() and not tinted[56:].any()
    res = subprocess.run([sys.executable, str(repo / "demo.py"), "--video", str(tmp_path / "in"), "--edit-frame", "2"],
                         capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "--track-store" in res.stderr                       # the flag reads the store
