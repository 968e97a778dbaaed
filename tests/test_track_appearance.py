"""``DenseTrackStore.appearance`` on the host (device="cpu": the definition as a torch composition -- ``result(frame)``, the
reference's ``warp_backward`` formulation, the visibility mask, float32 sums in column order): the video read along every track.  No
GPU needed.

The builders of this file (images, cases, the per-pixel restatement) are shared with tests/test_gpu_track_appearance.py, which holds
the fused device kernel to the device composition bit for bit and to this host path within a measured tolerance."""
import numpy as np
import pytest
import torch

from test_track_locate import T, const_planes, field, make_store, shifted_out_planes

# (a (min, max) table that holds inf or NaN dequantises through inf - inf and 0 * inf: numpy says so)
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered")


def images_for(seed, n, H, W, C):
    """n seeded uint8 frames (H, W, C)."""
    r = np.random.default_rng([17, seed, H, W, C])
    return [r.integers(0, 256, size=(H, W, C), dtype=np.uint8) for _ in range(n)]


def amplitude(H, W):
    """The flow amplitude of a size's fields: 5.0 (folding, a good share shifted out) from 9 x 17 up, 1.5 below."""
    return 5.0 if H >= 9 else 1.5


def field_store(H, W, seeds, device="cpu", **kw):
    """A store of len(seeds) smooth frames, frame ids 0, 1, ..."""
    return make_store(H, W, {k: field(s, H, W, amplitude(H, W)) for k, s in enumerate(seeds)}, device=device, **kw)


def case_planes(seed, H, W):
    """One stored frame of the shared cases: ``field`` at the size's amplitude; at 2 x 2 (where a smooth field is nearly constant)
    seeded uniform flows in [-0.6, 0.6], occlusion in [0, 1) and sigma in [0.05, 0.75)."""
    if (H, W) != (2, 2):
        return field(seed, H, W, amplitude(H, W))
    r = np.random.default_rng([23, seed])
    return (r.uniform(-0.6, 0.6, (2, H, W)).astype(np.float32), r.uniform(0, 1, (1, H, W)).astype(np.float32),
            r.uniform(0.05, 0.75, (1, H, W)).astype(np.float32))


SIZES = [(2, 2), (3, 5), (9, 17), (37, 53), (64, 64), (65, 130)]
COLUMNS = [1, 3, 4, 5, 17]
CASE_SIGMA_MAX = 0.4             # the finite sigma_max of the shared cases


def case_store(H, W, n, device="cpu", **kw):
    """Frame k is case_planes(k): with these seeds every case has both visible and invisible pixel-frames, with and without
    CASE_SIGMA_MAX, from 9 x 17 up at least 10 % of each (test_shared_cases_have_both_kinds holds it)."""
    return make_store(H, W, {k: case_planes(k, H, W) for k in range(n)}, device=device, **kw)


def visible_share_ok(visible, H):
    share = float(np.asarray(visible).mean())
    low = 0.1 if H >= 9 else 0.0
    return (0.0 < share < 1.0) and (low <= share <= 1.0 - low), share


def set_lohi(st, frame, channel, lo, hi):
    """A channel's (min, max) table overwritten: a way to hold values no quantisation would keep -- (nan, nan) makes the whole
    channel NaN, (lo, +inf) makes it +inf wherever its word is not 0 (and NaN where it is)."""
    st.lohi(st.slot_of(frame))[channel] = torch.tensor([lo, hi], dtype=torch.float32).to(st.device)
    return st


def per_pixel(st, frames, images, reference, thr=0.5, smax=None):
    """The definition pixel by pixel, column by column, channel by channel, over explicit taps: float64 arithmetic on the float32
    positions -> (sum, sumsq [C, H, W] float64, count [H, W], c [T, H, W, C] float64, visible [T, H, W])."""
    H, W, n = st.H, st.W, len(frames)
    C = images[0].shape[2]
    total, totalsq, count = np.zeros((C, H, W)), np.zeros((C, H, W)), np.zeros((H, W), np.int32)
    cs, visible = np.zeros((n, H, W, C)), np.zeros((n, H, W), bool)
    smax = np.inf if smax is None else smax
    for k, f in enumerate(frames):
        r = st.result(f)
        flow, occl, sigma = r.flow.numpy(), r.occlusion.numpy()[0], r.sigma.numpy()[0]
        for y in range(H):
            for x in range(W):
                px, py = np.float32(x) + flow[0, y, x], np.float32(y) + flow[1, y, x]
                vis = bool(occl[y, x] <= thr and sigma[y, x] <= smax and 0 <= px <= W - 1 and 0 <= py <= H - 1)
                visible[k, y, x] = vis
                if not (np.isfinite(px) and np.isfinite(py)):
                    continue
                x0, y0 = int(np.floor(px)), int(np.floor(py))
                wx, wy = float(px) - x0, float(py) - y0
                for ch in range(C):
                    def tap(yy, xx):
                        return float(images[k][yy, xx, ch]) if 0 <= yy < H and 0 <= xx < W else 0.0
                    c = tap(y0, x0) * (1 - wx) * (1 - wy) + tap(y0, x0 + 1) * wx * (1 - wy) + tap(y0 + 1, x0) * (1 - wx) * wy \
                        + tap(y0 + 1, x0 + 1) * wx * wy
                    cs[k, y, x, ch] = c
                    if vis:
                        d = c - (0.0 if reference is None else float(reference[y, x, ch]))
                        total[ch, y, x] += d
                        totalsq[ch, y, x] += d * d
                if vis:
                    count[y, x] += 1
    return total, totalsq, count, cs, visible


# What a float32 bilinear sample of 8-bit values may be off by, whatever the order of its operations: the position is the same
# float32 number on both sides and W - 1, H - 1 are powers of two at the sizes below (the samplers' coordinate round trip is exact),
# so what is left are the weights' and the blend's roundings -- four products of two factors and three sums of values up to 255,
# each rounded to 2^-24 relative: under 16 half-ulps of 255.
SAMPLE_EPS = 16 * 255 * 2.0 ** -24


# ---- 1. the per-pixel loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("H,W", [(3, 5), (9, 17)])
def test_composition_is_the_per_pixel_loop(H, W, C):
    st = field_store(H, W, (1, 2, 3))
    images, reference = images_for(0, 3, H, W, C), images_for(1, 1, H, W, C)[0]
    got = st.appearance(images, reference=reference, stack=True, fill=9)
    total, totalsq, count, cs, visible = per_pixel(st, [0, 1, 2], images, reference)
    assert got.count.dtype == torch.int32 and got.sum.dtype == torch.float32 and got.warped.dtype == torch.uint8 and got.visible.dtype == torch.bool
    assert tuple(got.sum.shape) == (C, H, W) and tuple(got.warped.shape) == (3, H, W, C) and tuple(got.visible.shape) == (3, H, W)
    assert np.array_equal(got.count.numpy(), count) and np.array_equal(got.visible.numpy(), visible)
    assert visible.any() and not visible.all()
    # per column the sample is off by SAMPLE_EPS at most and d by as much; d * d by 2 |d| SAMPLE_EPS, |d| <= 255; the float32
    # running sums add half an ulp of their size per column
    n = 3
    assert np.abs(got.sum.numpy() - total).max() <= n * (SAMPLE_EPS + 255 * n * 2.0 ** -24)
    assert np.abs(got.sumsq.numpy() - totalsq).max() <= n * (2 * 255 * SAMPLE_EPS + 255 * 255 * n * 2.0 ** -24)
    w = got.warped.numpy()
    assert (w[~visible] == 9).all()
    level = np.rint(np.clip(cs, 0, 255))
    clear = visible[..., None] & (np.abs(cs - np.floor(cs) - 0.5) > SAMPLE_EPS)            # not within reach of a tie
    assert np.array_equal(w[clear], level[clear].astype(np.uint8))
    assert (np.abs(w.astype(np.int32) - level)[np.broadcast_to(visible[..., None], w.shape)] <= 1).all()


@pytest.mark.parametrize("H,W", SIZES)
def test_shared_cases_have_both_kinds(H, W):
    """Visibility depends only on the dequantised planes, which host and device stores share bit for bit: the condition of the
    device test's cases is checked here."""
    for n in COLUMNS:
        st = case_store(H, W, n)
        for smax in (None, CASE_SIGMA_MAX):
            vis = st.appearance([np.zeros((H, W, 1), np.uint8)] * n, stack=True, sigma_max=smax).visible.numpy()
            ok, share = visible_share_ok(vis, H)
            assert ok, (H, W, n, smax, share)


# ---- 2. integer shifts: the residual against the template is exactly zero -------------------------------------------------------------
SHIFTS = ((0, 0), (3, 1), (-2, 2), (5, -4))


def shifted_video(H, W, C, seed=5):
    """-> (template, frames): frame k shows the template shifted by SHIFTS[k], seeded noise where the template does not reach."""
    template = images_for(seed, 1, H, W, C)[0]
    frames = images_for(seed + 1, len(SHIFTS), H, W, C)
    inside = []
    for k, (fx, fy) in enumerate(SHIFTS):
        ys, xs = np.mgrid[0:H, 0:W]
        ok = (xs + fx >= 0) & (xs + fx <= W - 1) & (ys + fy >= 0) & (ys + fy <= H - 1)
        frames[k][(ys + fy)[ok], (xs + fx)[ok]] = template[ys[ok], xs[ok]]
        inside.append(ok)
    return template, frames, np.stack(inside)


def shift_store(H, W, device="cpu"):
    return make_store(H, W, {k: const_planes(H, W, fx=fx, fy=fy) for k, (fx, fy) in enumerate(SHIFTS)}, device=device)


@pytest.mark.parametrize("H,W,exact", [(9, 17, True), (37, 53, False)])
def test_integer_shifts_leave_no_residual(H, W, exact):
    """At 9 x 17 W - 1 and H - 1 are powers of two and the sampler's coordinate round trip is exact: the sums are exactly 0.  At
    37 x 53 it is not (residuals of the order of 1e-3 times a level), and only ``warped`` is held to the template."""
    template, frames, inside = shifted_video(H, W, 3)
    got = shift_store(H, W).appearance(frames, reference=template, stack=True, fill=0)
    assert np.array_equal(got.count.numpy(), inside.sum(axis=0)) and np.array_equal(got.visible.numpy(), inside)
    assert inside[0].all() and not inside[1:].all(axis=(1, 2)).any()
    if exact:
        assert not got.sum.numpy().any() and not got.sumsq.numpy().any()
        assert np.array_equal(got.mean.numpy(), template.astype(np.float32)) and not got.var.numpy().any()
    else:
        # the round trip's four operations round a coordinate below 64 by half an ulp (2^-19) each; a tap pair differs by 255 at most,
        # per axis; and the blend adds SAMPLE_EPS -- per column, four columns
        bound = len(SHIFTS) * (2 * 255 * 4 * 2.0 ** -19 + SAMPLE_EPS)
        print(f"{H}x{W}: largest |sum| {np.abs(got.sum.numpy()).max():.3g} (bound {bound:.3g})")
        assert np.abs(got.sum.numpy()).max() <= bound
    w = got.warped.numpy()
    for k in range(len(SHIFTS)):
        assert np.array_equal(w[k][inside[k]], template[inside[k]]) and not w[k][~inside[k]].any()


# ---- 3. visibility ---------------------------------------------------------------------------------------------------------------
VH, VW = 9, 17


def visibility_cases(device="cpu"):
    """-> {name: (store, frames, kwargs, expected count [H, W])}: each rule of the definition on constant planes (flat channels: kept
    exactly)."""
    above_half, ones = float(np.nextafter(np.float32(0.5), np.float32(1))), np.ones((VH, VW), np.int32)
    cases = {}
    st = make_store(VH, VW, {0: const_planes(VH, VW, occl=0.5), 1: const_planes(VH, VW, occl=above_half)}, device=device)
    cases["occlusion == threshold is visible, the next float is not"] = (st, None, {}, ones)
    edge = ones.copy()
    edge[:, VW - 1] = 0                                      # flow x = 1: pixel W - 2 lands on W - 1 exactly, pixel W - 1 on W
    st = make_store(VH, VW, {0: const_planes(VH, VW, fx=1.0)}, device=device)
    cases["px == W - 1 is visible"] = (st, None, {}, edge)
    edge2 = edge.copy()
    edge2[:, VW - 2] = 0                                     # 15 + (1 + 2^-18) = 16 + 2^-18 in float32: just above W - 1
    st = make_store(VH, VW, {0: const_planes(VH, VW, fx=1.0 + 2.0 ** -18)}, device=device)
    cases["px just above W - 1 is not"] = (st, None, {}, edge2)
    low = ones.copy()
    low[VH - 1, :] = 0
    st = make_store(VH, VW, {0: const_planes(VH, VW, fy=1.0)}, device=device)
    cases["py == H - 1 is visible"] = (st, None, {}, low)
    st = make_store(VH, VW, {0: const_planes(VH, VW, sigma=0.25), 1: const_planes(VH, VW, sigma=0.75), 2: const_planes(VH, VW, sigma=0.5)},
                    device=device)
    cases["sigma_max excludes"] = (st, None, {"sigma_max": 0.5}, 2 * ones)
    cases["no sigma_max: every sigma"] = (st, None, {}, 3 * ones)
    f = field(4, VH, VW, 0.0)                                # zero flow, a sigma channel with a range
    st = set_lohi(make_store(VH, VW, {0: f}, device=device), 0, 3, 0.5, float("inf"))
    words = st.packed(0).cpu().numpy().astype(np.int64)[:, :, 3]
    occluded = st.result(0).occlusion[0].cpu().numpy() > 0.5
    cases["+inf sigma is visible without sigma_max (its NaN is not)"] = (st, None, {}, ((words != 0) & ~occluded).astype(np.int32))
    cases["+inf sigma is excluded by a sigma_max"] = (st, None, {"sigma_max": 1e30}, 0 * ones)
    for ch, what in ((0, "flow x"), (1, "flow y"), (2, "occlusion"), (3, "sigma")):
        st = set_lohi(make_store(VH, VW, {0: const_planes(VH, VW), 1: const_planes(VH, VW)}, device=device), 1, ch, float("nan"), float("nan"))
        cases[f"NaN {what} is invisible"] = (st, None, {}, ones)
    st = make_store(VH, VW, {0: const_planes(VH, VW), 1: shifted_out_planes(VH, VW)}, device=device)
    cases["a frame shifted wholly out adds nothing"] = (st, None, {}, ones)
    return cases


with np.errstate(invalid="ignore"):
    VISIBILITY_NAMES = list(visibility_cases())


@pytest.mark.parametrize("name", VISIBILITY_NAMES)
def test_visibility_rules(name):
    st, frames, kw, count = visibility_cases()[name]
    images = images_for(3, len(st), VH, VW, 2)
    got = st.appearance(images, frames, stack=True, fill=77, **kw)
    assert np.array_equal(got.count.numpy(), count), name
    vis = got.visible.numpy()
    assert np.array_equal(vis.sum(axis=0), count)
    assert (got.warped.numpy()[~vis] == 77).all()
    assert np.isfinite(got.sum.numpy()).all() and np.isfinite(got.sumsq.numpy()).all()         # nothing invisible leaks into the sums
    assert not got.sum.numpy()[:, count == 0].any()


# ---- 4. call forms and errors ----------------------------------------------------------------------------------------------------
def test_call_forms():
    H, W, C = 9, 17, 3
    st = make_store(H, W, {f: field(s, H, W, 5.0) for s, f in enumerate((3, 8, 5))})
    images = images_for(7, 3, H, W, C)
    by_id = dict(zip((3, 8, 5), images))
    reference = images_for(8, 1, H, W, C)[0]
    base = st.appearance(images, reference=reference, stack=True)
    assert base.frames == [3, 8, 5] and base.reference is not None
    # one [T, H, W, C] tensor, tensors, numpy arrays: the same
    for form in (torch.from_numpy(np.stack(images)), [T(i) for i in images]):
        other = st.appearance(form, reference=T(reference), stack=True)
        for a in ("count", "sum", "sumsq", "warped", "visible"):
            assert torch.equal(getattr(other, a), getattr(base, a)), a
    # another order of the columns: count and the stack's rows permute; a frame given twice counts twice
    order = [5, 3, 8, 3]
    other = st.appearance([by_id[f] for f in order], order, reference=reference, stack=True)
    assert other.frames == order
    vis = base.visible.numpy()
    assert np.array_equal(other.visible.numpy(), vis[[2, 0, 1, 0]]) and np.array_equal(other.warped.numpy(), base.warped.numpy()[[2, 0, 1, 0]])
    assert np.array_equal(other.count.numpy(), base.count.numpy() + vis[0])
    seq = st.appearance([by_id[3], by_id[3]], [3, 3], reference=reference)
    one = st.appearance([by_id[3]], [3], reference=reference)
    assert np.array_equal(seq.sum.numpy(), one.sum.numpy() + one.sum.numpy()) and np.array_equal(seq.count.numpy(), 2 * one.count.numpy())
    # no stack unless asked for
    plain = st.appearance(images, reference=reference)
    assert plain.warped is None and plain.visible is None and torch.equal(plain.sum, base.sum) and torch.equal(plain.count, base.count)
    # without a reference the sums are those of the samples themselves
    raw = st.appearance(images)
    assert raw.reference is None and (raw.sum.numpy() >= 0).all()
    seen = base.count.numpy() > 0
    assert seen.any() and not seen.all()
    np.testing.assert_allclose(raw.mean.numpy()[seen], base.mean.numpy()[seen], atol=1e-3)
    # mean and var: NaN where the pixel was never visible
    assert np.isnan(base.mean.numpy()[~seen]).all() and np.isnan(base.var.numpy()[~seen]).all()
    assert tuple(base.mean.shape) == (H, W, C) and (base.var.numpy()[seen] >= 0).all()
    n = base.count.numpy()[seen].astype(np.float32)
    np.testing.assert_array_equal(base.mean.numpy()[seen], reference[seen].astype(np.float32) + base.sum.numpy().transpose(1, 2, 0)[seen] / n[:, None])
    # no columns: zeros
    none = st.appearance([], [], reference=reference, stack=True)
    assert not none.count.numpy().any() and not none.sum.numpy().any() and tuple(none.sum.shape) == (C, H, W)
    assert tuple(none.warped.shape) == (0, H, W, C) and tuple(none.visible.shape) == (0, H, W)
    assert np.isnan(none.mean.numpy()).all()


def test_errors_come_before_any_work(monkeypatch):
    from mft_amd.trackstore import DenseTrackStore
    H, W, C = 9, 17, 3
    st = make_store(H, W, {f: field(s, H, W, 5.0) for s, f in enumerate((3, 8, 5))})
    images = images_for(7, 3, H, W, C)
    calls = []
    monkeypatch.setattr(DenseTrackStore, "_result_of_slot", lambda self, slot: calls.append(slot))       # any work would pass here
    monkeypatch.setattr(DenseTrackStore, "_compose_appearance", lambda self, *a: calls.append(a))
    allocated = []
    for fn in ("zeros", "empty", "from_numpy"):
        monkeypatch.setattr(torch, fn, lambda *a, _fn=fn, **k: allocated.append(_fn))
    with pytest.raises(KeyError):
        st.appearance(images, [3, 4, 5])
    assert not allocated and not calls
    monkeypatch.undo()
    monkeypatch.setattr(DenseTrackStore, "_result_of_slot", lambda self, slot: calls.append(slot))
    monkeypatch.setattr(DenseTrackStore, "_compose_appearance", lambda self, *a: calls.append(a))
    bad = {
        "too few images": dict(images=images[:2]),
        "float images": dict(images=[i.astype(np.float32) for i in images]),
        "a float tensor": dict(images=torch.zeros((3, H, W, C))),
        "planar images": dict(images=[i.transpose(2, 0, 1) for i in images]),
        "another size": dict(images=[i[:, :-1] for i in images]),
        "five channels": dict(images=[np.zeros((H, W, 5), np.uint8)] * 3),
        "no channel axis": dict(images=[i[:, :, 0] for i in images]),
        "mixed channel counts": dict(images=[images[0], images[1], images[2][:, :, :1]]),
        "a [T, H, W] tensor": dict(images=torch.zeros((3, H, W), dtype=torch.uint8)),
        "a stack of another length": dict(images=torch.zeros((2, H, W, C), dtype=torch.uint8)),
        "reference of another C": dict(images=images, reference=np.zeros((H, W, 1), np.uint8)),
        "float reference": dict(images=images, reference=np.zeros((H, W, C), np.float32)),
        "reference of another size": dict(images=images, reference=np.zeros((W, H, C), np.uint8)),
        "fill beyond a byte": dict(images=images, fill=256),
        "negative fill": dict(images=images, fill=-1),
    }
    for name, kw in bad.items():
        with pytest.raises(ValueError):
            st.appearance(**kw)
        assert not calls, name


def test_entry_point_is_declared_and_bound():
    import re
    from pathlib import Path
    from mft_amd import _lib, atlas_ops
    header = (Path(__file__).resolve().parents[1] / "include" / "mftx.h").read_text()
    name = "mftx_trackstore_appearance"
    assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 17
    assert callable(atlas_ops.trackstore_appearance)
