"""``DenseTrackStore.locate`` / ``tracks_from`` on the device (csrc/trackstore.hip: ts_locate_search_kernel,
ts_locate_resolve_kernel through ``ops.trackstore_locate``) against the host restatement of the same definition
(mft_amd/trackstore.py, device="cpu"), bit for bit; the fields and points are those of tests/test_track_locate.py."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import golden_inputs as gi
import test_track_locate as host
from mft_amd.config import load_config
from mft_amd.synth import SyntheticVideo

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
DEV = "cuda"
FRAME_IDS = host.FRAME_IDS
TOL = host.TOL


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same(got, want):
    """(table, cell) of the device store against the host store's: cells equal, tables equal as int32 bits."""
    assert torch.equal(got[1].cpu(), want[1]), np.flatnonzero((got[1].cpu() != want[1]).numpy())
    assert torch.equal(bits(got[0]), bits(want[0])), np.flatnonzero((bits(got[0]) != bits(want[0])).any(dim=1).numpy())


@functools.lru_cache(maxsize=None)
def stores(H, W, amp):
    frames = host.smooth_frames(H, W, amp)
    return host.make_store(H, W, frames, device=DEV), host.make_store(H, W, frames)


def special_points(H, W):
    """Corners and edges of the frame, points on grid lines, and a few outside the frame or far from it."""
    return np.array([[3.25, 7.5], [0.0, 0.0], [W - 1.0, H - 1.0], [5.0, 9.0], [-2.0, 4.0], [W + 4.5, 10.0], [W - 0.5, H - 0.5],
                     [-0.5, -0.5], [W - 1.0, 0.0], [0.0, H - 1.0], [-1.0, -1.0], [float(W), float(H)], [1.0e5, -1.0e5],
                     [20.0, -0.25], [31.0, 8.0], [32.0, 8.5], [12.5, 16.0]], np.float32)


@functools.lru_cache(maxsize=None)
def queries(N, H, W, amp):
    """N points given on the stored frames: the special points, images of template points on each frame (so that they have
    preimages, several where the field folds), and uniform points over the frame and a margin around it."""
    _, cpu = stores(H, W, amp)
    sp = special_points(H, W)
    if N <= 7:
        return np.ascontiguousarray(sp[:N])
    n_img = (N - len(sp)) // 2
    P = host.template_points(n_img, H, W, seed=N)
    img = cpu.query(P).numpy()
    img = np.stack([img[n, n % 3, 0:2] for n in range(n_img)])
    r = np.random.default_rng(N)
    rest = r.uniform(-3, max(H, W) + 3, size=(N - len(sp) - n_img, 2)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([sp, img, rest]).astype(np.float32))


# ---- 7. device = host restatement, bitwise -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 7, 301])
@pytest.mark.parametrize("amp", [1.5, 5.0])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_locate_is_the_host_restatement_bitwise(H, W, amp, N):
    dev, cpu = stores(H, W, amp)
    q = queries(N, H, W, amp)
    xy = torch.from_numpy(q).to(DEV)
    found = 0
    for f in FRAME_IDS:                                           # one frame
        want = cpu.locate(q, f)
        got = dev.locate(xy, f)
        assert got[0].is_cuda and got[0].shape == (N, 4) and got[1].dtype == torch.int32
        assert_same(got, want)
        found += int((want[1] >= 0).sum())
    ids = [FRAME_IDS[(n * 7 + n // 5) % 3] for n in range(N)]      # per-point frames over the three stored frames, unsorted
    want = cpu.locate(q, ids)
    got = dev.locate(xy, ids)
    assert_same(got, want)
    assert_same(dev.locate(q, np.array(ids)), want)               # host points, an array of ids
    if N == 301:
        assert found > 3 * 150 and int((want[1] < 0).sum()) > 10  # both kinds of answer are exercised
    # the same call again gives the same bits, on another stream too
    out = (torch.empty((N, 4), device=DEV), torch.empty((N,), dtype=torch.int32, device=DEV))
    for _ in range(5):
        again = dev.locate(xy, ids, out=out)
        assert again[0] is out[0] and again[1] is out[1]
        assert_same(again, want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = dev.locate(xy, ids)
    s.synchronize()
    assert_same(other, want)


# ---- 8. choice and not-found cases -------------------------------------------------------------------------------------------
def test_choice_rule_on_the_device():
    """Several lanes (the left cell and the seam cell sit in one wave's tile) and several workgroups (the right half's cell is
    in another tile) hold candidates for one query."""
    H, W = host.CHOICE_HW
    frames = host.choice_frames()
    dev, cpu = host.make_store(H, W, frames, device=DEV), host.make_store(H, W, frames)
    q = host.choice_queries()
    rows = np.floor(q[:, 1]).astype(np.int64)
    for f, thr in ((0, 0.5), (1, 0.5), (2, 0.5), (2, 1.0)):
        want = cpu.locate(q, f, occlusion_threshold=thr)
        got = dev.locate(q, f, occlusion_threshold=thr)
        assert_same(got, want)
        assert (want[1] >= 0).all()
    # what the host test pins, on the device's own answer: frame 1 -> the right half, frame 2 -> left (x <= 13) or the seam
    c1, c2 = dev.locate(q, 1)[1].cpu().numpy(), dev.locate(q, 2)[1].cpu().numpy()
    assert (c1 % (W - 1) >= W // 2).all() and np.array_equal(c1 // (W - 1), rows)
    assert (c2[:6] % (W - 1) <= 13).all() and (c2[6:] % (W - 1) == W // 2 - 1).all()
    ids = [2, 0, 1, 2, 0, 1, 1, 2, 0, 2]
    assert_same(dev.locate(q, ids), cpu.locate(q, ids))


def test_no_preimage_on_the_device():
    H, W = 40, 56
    frames, q, ids, want_found = host.no_preimage_case(H, W)
    dev, cpu = host.make_store(H, W, frames, device=DEV), host.make_store(H, W, frames)
    q = q.copy()
    q[18:] = cpu.query(q[18:], frames=[2]).numpy()[:, 0, 0:2]
    got = dev.locate(q[:9], 7)
    assert (got[1] == -1).all() and (bits(got[0]) == 0x7fc00000).all()
    assert_same(got, cpu.locate(q[:9], 7))
    assert_same(dev.locate(q, ids), cpu.locate(q, ids))
    far = np.array([[1.0e5, -1.0e5], [np.nan, 3.0], [-50.0, 4.0], [np.inf, 2.0]], np.float32)
    assert_same(dev.locate(far, 2), cpu.locate(far, 2))
    assert (dev.locate(far, 2)[1] == -1).all()
    coords, occl, found = dev.tracks_from(q, ids)
    assert np.array_equal(found, want_found) and np.isnan(coords[:9]).all() and (occl[:9] == 1).all()
    hc, ho, hf = cpu.tracks_from(q, ids)
    ok = np.flatnonzero(want_found)
    # (the located template points are the host's bit for bit; the read-out that follows agrees with the host's sampler within
    # its fp32 operation-order tolerance, as tests/test_gpu_trackstore.py has it)
    assert np.array_equal(found, hf) and np.abs(coords[ok] - hc[ok]).max() <= 1e-5 and np.abs(occl[ok] - ho[ok]).max() <= 1e-6
    table, _ = dev.locate(q, ids)
    want = dev.query(table[torch.from_numpy(ok).to(DEV), 0:2]).cpu().numpy()
    assert np.array_equal(coords[ok], want[:, :, 0:2]) and np.array_equal(occl[ok], want[:, :, 2])


# ---- 9. chunks ---------------------------------------------------------------------------------------------------------------
def test_frames_of_three_chunks_in_one_call():
    H, W = 37, 53
    frames = {f: host.field(k, H, W, 5.0 if k % 2 else 1.5) for k, f in enumerate((20, 21, 22, 23, 24))}
    dev, cpu = host.make_store(H, W, frames, device=DEV, frames_per_chunk=2), host.make_store(H, W, frames, frames_per_chunk=2)
    assert len(dev._chunks) == 3
    P = host.template_points(60, H, W, seed=9)
    ids = [(20, 23, 24, 21)[(n * 3 + n // 7) % 4] for n in range(60)]               # chunks 0, 1, 2 and 0 again
    img = cpu.query(P).numpy()
    q = np.stack([img[n, ids[n] - 20, 0:2] for n in range(60)])
    want = cpu.locate(q, ids)
    assert (want[1] >= 0).all()
    assert_same(dev.locate(q, ids), want)


# ---- 10. untouched memory ----------------------------------------------------------------------------------------------------
def test_only_the_n_rows_are_written():
    H, W, N = 37, 53, 77
    dev, cpu = stores(H, W, 5.0)
    q = queries(301, H, W, 5.0)[:N]
    ids = [FRAME_IDS[n % 3] for n in range(N)]
    big_t = torch.full((N + 5, 4), -7.0, device=DEV)
    big_c = torch.full((N + 5,), -77, dtype=torch.int32, device=DEV)
    out = (big_t[2:N + 2], big_c[3:N + 3])
    got = dev.locate(q, ids, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[1] is out[1]
    assert_same(out, cpu.locate(q, ids))
    assert (big_t[:2] == -7).all() and (big_t[N + 2:] == -7).all() and (big_c[:3] == -77).all() and (big_c[N + 3:] == -77).all()
    with pytest.raises(ValueError):
        dev.locate(q, ids, out=(big_t[:N], big_c[:N].cpu()))
    with pytest.raises(ValueError):
        dev.locate(q, ids, out=(torch.empty((N, 8), device=DEV)[:, :4], big_c[:N]))     # not contiguous
    with pytest.raises(KeyError):
        dev.locate(q, [99] * N)


# ---- 11. through the tracker -------------------------------------------------------------------------------------------------
def _config(fif):
    conf = load_config(REPO / "configs" / "MFT_cfg.py")
    conf.flow_config.model = None
    conf.flow_config.synthetic_weights_seed = gi.WEIGHT_SEED          # make_weights(seed): stand-in weights
    conf.flow_config.flow_iters = 4
    conf.flow_config.frames_in_flight = fif
    conf.deltas = [np.inf, 1, 2]
    conf.keep_result_on_device = True
    conf.track_store = True
    return conf


@pytest.mark.parametrize("fif", [1, 2])
def test_points_given_mid_video_through_the_tracker(fif):
    H, W, t = 128, 160, 3
    video = SyntheticVideo(H, W, n_frames=6, seed=21)
    tracker = _config(fif).tracker_class(_config(fif))
    for k in range(len(video)):
        tracker.init(video[0]) if k == 0 else tracker.track(video[k])
    st = tracker.track_store
    assert len(st) == 6 and st.frame_ids == list(range(6))
    P = host.template_points(100, H, W, seed=4)
    at_t = st.query(P, frames=[t])[:, 0]                           # device [100, 4]
    coords, occl, found = st.tracks_from(at_t[:, 0:2], t)
    Q = at_t[:, 0:2].cpu().numpy()
    visible = at_t[:, 2].cpu().numpy() < 0.5
    print(f"fif {fif}: {int(found.sum())} of 100 found, {int(visible.sum())} stored as visible at frame {t}")
    assert coords.shape == (100, 6, 2) and occl.shape == (100, 6) and found[visible].all()
    err = np.abs(coords[found, t] - Q[found]).max()
    print(f"    the track at frame {t} is within {err:.3g} px of the query")
    assert err <= TOL
    # ... and it is the host restatement's answer on the same stored frames
    cpu = host.make_store(H, W, {})
    cpu._chunks, cpu._lohi = [c.cpu() for c in st._chunks], [l.cpu() for l in st._lohi]
    cpu.frame_ids, cpu._slot_of = list(st.frame_ids), dict(st._slot_of)
    assert_same(st.locate(at_t[:, 0:2], t), cpu.locate(Q, t))
