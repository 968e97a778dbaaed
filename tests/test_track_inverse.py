"""``DenseTrackStore.inverse`` / ``results_from`` / ``result_from`` on the host (device="cpu"): the dense inverse is ``locate`` at
every pixel centre of a stored frame, and the results FROM that frame are the inverse followed by ``query``.  No GPU needed.

The fields and stores are those of tests/test_track_locate.py; what is built here (``grid``, ``box_counts``, ``torn_planes``,
``composed``) is shared with tests/test_gpu_track_inverse.py, which holds the device path to this restatement bit for bit."""
import functools

import numpy as np
import pytest
import torch

from test_track_locate import (CHOICE_HW, FRAME_IDS, choice_frames, const_planes, field, lipschitz, make_store, shifted_out_planes,
                               smooth_frames)
from mft_amd.results import FlowOUTrackingResult
from mft_amd.trackstore import LOCATE_EPS

INLINE = 16                      # centres a cell's own lane walks on the device (csrc/trackstore.hip: TI_INLINE)


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def grid(H, W):
    """The pixel centres (x, y), row-major: float32 [H * W, 2]."""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x.ravel(), y.ravel()], axis=1).astype(np.float32)


def located_on_grid(st, f, thr=0.5):
    """``locate`` with the pixel grid as its points, shaped like ``inverse``'s answer."""
    t, c = st.locate(grid(st.H, st.W), f, occlusion_threshold=thr)
    return t.reshape(st.H, st.W, 4), c.reshape(st.H, st.W)


def assert_inverse_is_locate(st, f, thr=0.5):
    t, c = st.inverse(f, occlusion_threshold=thr)
    wt, wc = located_on_grid(st, f, thr)
    assert t.shape == (st.H, st.W, 4) and t.dtype == torch.float32 and c.shape == (st.H, st.W) and c.dtype == torch.int32
    assert torch.equal(c, wc) and np.array_equal(bits(t), bits(wt))
    return t.numpy(), c.numpy()


def box_counts(st, f):
    """Per template cell of stored frame ``f``: how many pixel centres the integer range of its widened box holds (floor of
    the lower and ceil of the upper bounds, clipped to the frame -- what the device kernel walks), and how many of them pass
    the box test itself."""
    r = st.result(f)
    fx, fy = r.flow[0].cpu().numpy(), r.flow[1].cpu().numpy()
    H, W = fx.shape
    mx, my = np.arange(W, dtype=np.float32)[None, :] + fx, np.arange(H, dtype=np.float32)[:, None] + fy

    def span(m, n):
        a, b, c, d = m[:-1, :-1].ravel(), m[:-1, 1:].ravel(), m[1:, :-1].ravel(), m[1:, 1:].ravel()
        lo = np.fmin(np.fmin(a, b), np.fmin(c, d)) - LOCATE_EPS
        hi = np.fmax(np.fmax(a, b), np.fmax(c, d)) + LOCATE_EPS
        walked = np.clip(np.ceil(hi), -1, n - 1) - np.clip(np.floor(lo), 0, n) + 1
        inside = np.clip(np.floor(hi), -1, n - 1) - np.clip(np.ceil(lo), 0, n) + 1
        return np.maximum(walked, 0).astype(np.int64), np.maximum(inside, 0).astype(np.int64)

    (wx, ix), (wy, iy) = span(mx, W), span(my, H)
    return wx * wy, ix * iy


def torn_planes():
    """field(437, 37, 53, 1.5) with three pixels' flow overwritten: the cells around them are torn over much of the frame."""
    flow, occl, sigma = field(437, 37, 53, 1.5)
    flow = flow.copy()
    flow[:, 10, 20] = (40, 20)
    flow[:, 30, 5] = (-10, -35)
    flow[:, 18, 40] = (-45, 15)
    return flow, occl, sigma


def composed(table, cell, q):
    """The rule of ``results_from`` in numpy float32: table [H, W, 4] and cell [H, W] of ``inverse``, q [H * W, T, 4] of ``query``
    at the located template points -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W], found [H, W])."""
    H, W = cell.shape
    T = q.shape[1]
    found = (cell >= 0).ravel()
    tb = table.reshape(H * W, 4)
    with np.errstate(all="ignore"):
        flow = q[:, :, 0:2] - grid(H, W)[:, None, :]
        occl = np.maximum(tb[:, None, 2], q[:, :, 2])
        sigma = np.sqrt(tb[:, None, 3] * tb[:, None, 3] + q[:, :, 3] * q[:, :, 3])
    flow[~found], occl[~found], sigma[~found] = np.nan, 1.0, np.inf
    assert flow.dtype == np.float32 and occl.dtype == np.float32 and sigma.dtype == np.float32
    return (np.ascontiguousarray(flow.transpose(1, 2, 0)).reshape(T, 2, H, W), np.ascontiguousarray(occl.T).reshape(T, 1, H, W),
            np.ascontiguousarray(sigma.T).reshape(T, 1, H, W), found.reshape(H, W))


@functools.lru_cache(maxsize=None)
def smooth_store(H, W, amp):
    return make_store(H, W, smooth_frames(H, W, amp))


# ---- 1. inverse is locate on the grid ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [1.5, 5.0])
def test_inverse_is_locate_on_the_pixel_grid(amp):
    H, W = 37, 53
    st = smooth_store(H, W, amp)
    for f in FRAME_IDS:
        assert_inverse_is_locate(st, f)
    ids = [FRAME_IDS[2], FRAME_IDS[0], FRAME_IDS[2]]                                # a list of ids, one of them twice
    t, c = st.inverse(ids)
    assert t.shape == (3, H, W, 4) and c.shape == (3, H, W)
    for k, f in enumerate(ids):
        wt, wc = located_on_grid(st, f)
        assert torch.equal(c[k], wc) and np.array_equal(bits(t[k]), bits(wt))
    out = (torch.full((3, H, W, 4), -7.0), torch.full((3, H, W), -7, dtype=torch.int32))
    got = st.inverse(np.array(ids), out=out)
    assert got[0] is out[0] and got[1] is out[1] and np.array_equal(bits(out[0]), bits(t)) and torch.equal(out[1], c)
    t0, c0 = st.inverse([])
    assert t0.shape == (0, H, W, 4) and c0.shape == (0, H, W)


# ---- 2. identity -------------------------------------------------------------------------------------------------------------
def test_identity_frame_inverts_to_the_pixel_grid():
    H, W = 37, 53
    st = make_store(H, W, {4: const_planes(H, W)})
    t, c = assert_inverse_is_locate(st, 4)
    assert (c >= 0).all()
    assert np.array_equal(t[..., 0:2].reshape(-1, 2), grid(H, W)) and not t[..., 2:4].any()


# ---- 3. both kinds of answer -------------------------------------------------------------------------------------------------
def test_a_folding_field_leaves_pixels_without_a_preimage():
    st = smooth_store(37, 53, 5.0)
    t, c = st.inverse(3)
    found = c.numpy() >= 0
    print(f"found share {found.mean():.3f}, {int((~found).sum())} pixels not found")
    assert found.mean() > 0.8 and (~found).sum() > 100
    assert np.isnan(t.numpy()[~found]).all() and np.isfinite(t.numpy()[found]).all()


# ---- 4. nothing maps into the frame ------------------------------------------------------------------------------------------
def test_shifted_out_frame_has_no_preimage_anywhere():
    H, W = 40, 56
    st = make_store(H, W, {7: shifted_out_planes(H, W)})
    t, c = assert_inverse_is_locate(st, 7)
    assert (c == -1).all() and np.isnan(t).all()


# ---- 5. choice rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,thr", [(1, 0.5), (1, 1.0), (2, 0.5), (2, 1.0)])
def test_choice_rule_carries_over(f, thr):
    H, W = CHOICE_HW
    st = make_store(H, W, choice_frames())
    t, c = assert_inverse_is_locate(st, f, thr)                                      # the winner per pixel is locate's
    found = c >= 0
    assert found.sum() == 1120 and H * W == 2240
    assert found[:, :W // 2].all() and not found[:, W // 2:].any()                   # both halves and the seam land on the left half


# ---- 6. results_from the identity frame --------------------------------------------------------------------------------------
def test_results_from_the_identity_frame_are_the_stored_results():
    H, W = 37, 53
    frames = {0: const_planes(H, W)}
    frames.update(smooth_frames(H, W, 1.5))
    st = make_store(H, W, frames)
    flow, occl, sigma, found = st.results_from(0)
    ids = [0] + list(FRAME_IDS)
    assert st.frame_ids == ids and flow.shape == (4, 2, H, W) and occl.shape == (4, 1, H, W) and sigma.shape == (4, 1, H, W)
    assert found.shape == (H, W) and found.dtype == torch.bool and found.all()
    for k, f in enumerate(ids):
        r = st.result(f)
        for name, got, want, bound in (("flow", flow[k], r.flow, 2.0 ** -15 * lipschitz(r.flow.numpy()) + 2.0 ** -16),
                                       ("occlusion", occl[k], r.occlusion, 2.0 ** -15 * lipschitz(r.occlusion.numpy()) + 2.0 ** -22),
                                       ("sigma", sigma[k], r.sigma, 2.0 ** -15 * lipschitz(r.sigma.numpy()) + 2.0 ** -22)):
            err = float((got - want).abs().max())
            print(f"frame {f}: {name} differs by at most {err:.3g} (bound {bound:.3g})")
            assert err <= bound


# ---- 7. composition and not-found values -------------------------------------------------------------------------------------
def test_results_from_is_the_composition_of_inverse_and_query():
    H, W = 37, 53
    st = smooth_store(H, W, 5.0)
    src = 8
    table, cell = st.inverse(src)
    found = cell >= 0
    assert 100 < int((~found).sum()) < H * W // 2
    template = torch.where(found.reshape(-1, 1), table.reshape(-1, 4)[:, 0:2], torch.zeros(()))
    for frames in (None, [5, 3]):
        q = st.query(template, frames).numpy()
        want = composed(table.numpy(), cell.numpy(), q)
        got = st.results_from(src, frames)
        assert got[0].shape == (q.shape[1], 2, H, W) and got[3].dtype == torch.bool
        for g, w in zip(got[:3], want[:3]):
            assert g.dtype == torch.float32 and np.array_equal(bits(g), w.view(np.int32))
        assert np.array_equal(got[3].numpy(), want[3]) and torch.equal(got[3], found)
    flow, occl, sigma, _ = st.results_from(src, [5])
    lost = ~found
    assert np.isnan(flow[0][:, lost].numpy()).all() and (occl[0, 0][lost] == 1).all() and torch.isposinf(sigma[0, 0][lost]).all()
    assert torch.isfinite(flow[0][:, found]).all() and torch.isfinite(sigma[0, 0][found]).all()
    # from a frame to itself: a found pixel stays where it is, up to the acceptance residual and the sampler's rounding
    back = st.results_from(src, [src])[0][0]
    assert float(back[:, found].abs().max()) <= 2.0 ** -9


# ---- 8. interface and errors -------------------------------------------------------------------------------------------------
def test_result_from_interface_and_documented_errors():
    H, W = 37, 53
    st = smooth_store(H, W, 5.0)
    r, found = st.result_from(8, 5)
    assert isinstance(r, FlowOUTrackingResult) and (r.H, r.W) == (H, W)
    assert r.flow.shape == (2, H, W) and r.occlusion.shape == (1, H, W) and r.sigma.shape == (1, H, W)
    assert found.shape == (H, W) and found.dtype == torch.bool
    flow, occl, sigma, f2 = st.results_from(8, [5])
    assert np.array_equal(bits(r.flow), bits(flow[0])) and np.array_equal(bits(r.occlusion), bits(occl[0]))
    assert np.array_equal(bits(r.sigma), bits(sigma[0])) and torch.equal(found, f2)
    assert st.results_from(8, [])[0].shape == (0, 2, H, W)
    for call in (lambda: st.inverse(99), lambda: st.inverse([3, 99]), lambda: st.results_from(99), lambda: st.results_from(3, [8, 99]),
                 lambda: st.result_from(99, 3), lambda: st.result_from(3, 99)):
        with pytest.raises(KeyError):
            call()
    with pytest.raises(ValueError):
        st.inverse([[3, 8], [5, 3]])
    for out in ((torch.zeros(H, W, 4), torch.zeros(H, W)),                                       # cell is not int32
                (torch.zeros(H, W, 4, dtype=torch.float64), torch.zeros(H, W, dtype=torch.int32)),
                (torch.zeros(H * W, 4), torch.zeros(H * W, dtype=torch.int32)),                   # locate's shapes, not inverse's
                (torch.zeros(1, H, W, 4), torch.zeros(1, H, W, dtype=torch.int32)),               # one id: no leading axis
                (torch.zeros(H, W, 8)[:, :, :4], torch.zeros(H, W, dtype=torch.int32))):          # not contiguous
        with pytest.raises(ValueError):
            st.inverse(3, out=out)
    with pytest.raises(ValueError):
        st.inverse([3, 8], out=(torch.zeros(H, W, 4), torch.zeros(H, W, dtype=torch.int32)))


def test_phase_two_inputs_are_what_they_are_meant_to_be():
    """The fields that tests/test_gpu_track_inverse.py uses to reach the kernel's second phase do hold cells whose ranges exceed
    what a lane walks itself."""
    st = make_store(24, 40, {0: field(0, 24, 40, 12.0)})
    walked, inside = box_counts(st, 0)
    print(f"amp 12: {int((walked > INLINE).sum())} of {walked.size} cells walk more than {INLINE} centres (largest {walked.max()}); "
          f"{int((inside > INLINE).sum())} hold more than {INLINE} (largest {inside.max()})")
    assert walked.size == 23 * 39 and (inside > INLINE).sum() > 50 and (walked >= inside).all()
    st = make_store(37, 53, {0: torn_planes()})
    walked, inside = box_counts(st, 0)
    print(f"torn: {int((inside > 64).sum())} cells hold more than 64 centres (largest {inside.max()}; walked: {walked.max()})")
    assert (inside > 64).sum() == 12 and inside.max() == 770 and (walked >= inside).all()
    c = st.inverse(0)[1].numpy()
    print(f"torn: {int((c >= 0).sum())} of {c.size} pixels found")
    assert (c >= 0).sum() == 1921 and c.size == 1961


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    import re
    from pathlib import Path
    from mft_amd import _lib, ops
    repo = Path(__file__).resolve().parents[1]
    name = "mftx_trackstore_invert"
    assert re.search(r"\b%s\s*\(" % name, (repo / "include" / "mftx.h").read_text()) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, name) and callable(ops.trackstore_invert)

    def call(G=1, H=8, W=8):                                                         # checks that come before anything is launched
        return lib.mftx_trackstore_invert(None, None, G, H, W, 0.5, None, None, None, None)

    assert call() == -1 and b"trackstore_invert" in lib.mftx_last_error_string()
    assert call(H=1) == -1 and call(W=1) == -1 and call(G=-1) == -1
    assert call(G=0) == 0                                                            # no frames: a no-op
