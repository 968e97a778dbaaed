"""``TrackAtlas.results_from`` on the device (csrc/trackstore.hip: ts_flow_from_kernel through ``ops.trackstore_flow_from``) against
the composition it fuses -- ``atlas.inverse``, per-template ``atlas.query`` and the torch rule of ``DenseTrackStore.results_from``,
all on device tensors -- bit for bit wherever the expected value is no NaN and NaN exactly where it is one; against the host
atlas within what the project accepts between the device sampler and torch's; and through a ``MultiTemplateMFT`` pass."""
import functools

import numpy as np
import pytest
import torch

import test_track_atlas as host
import test_gpu_track_atlas as ga
from test_track_atlas_flow import INF_BITS, NAN_BITS, ONE_BITS
from test_track_locate import const_planes, field, make_store, shifted_out_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def device_composition(atlas, src, cols, thr=0.5):
    """The definition on device tensors -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W], found, template)."""
    H, W, T = atlas.H, atlas.W, len(cols)
    N = H * W
    table, _, entry = atlas.inverse(src, thr)
    tb, e = table.reshape(N, 4), entry.reshape(N)
    found = e >= 0
    tmpl_of = torch.tensor([f for f, _ in atlas.entries], dtype=torch.int32, device=DEV)
    template = torch.where(found, tmpl_of[e.clamp(min=0).long()], torch.full_like(e, -1))
    at = torch.where(found[:, None], tb[:, 0:2], torch.zeros((), device=DEV))
    idx = torch.arange(N, device=DEV)
    g = torch.stack([idx % W, idx // W], dim=1).to(torch.float32)
    flow = torch.full((N, T, 2), float("nan"), device=DEV)
    occl = torch.ones((N, T), device=DEV)
    sigma = torch.full((N, T), float("inf"), device=DEV)
    for s in sorted({f for f, _ in atlas.entries}):
        cov = atlas.covered(s, cols)
        if not any(cov):
            continue
        q = atlas.query(s, at, cols)                                                 # [N, T, 4]; a row of NaN where not covered
        s_src, s_dst = tb[:, None, 3], q[:, :, 3]
        m = (template == s)[:, None] & torch.tensor(cov, device=DEV)[None, :]
        flow = torch.where(m[:, :, None], q[:, :, 0:2] - g[:, None, :], flow)
        occl = torch.where(m, torch.maximum(tb[:, None, 2], q[:, :, 2]), occl)
        sigma = torch.where(m, torch.sqrt((s_src * s_src + s_dst * s_dst).to(torch.float64)).to(torch.float32), sigma)
    return (flow.permute(1, 2, 0).reshape(T, 2, H, W).contiguous(), occl.t().reshape(T, 1, H, W).contiguous(),
            sigma.t().reshape(T, 1, H, W).contiguous(), found.view(H, W), template.view(H, W))


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same(got, want):
    """Bits where the expected value is no NaN, NaN-ness elsewhere; found and template equal."""
    for name, g, w in zip(("flow", "occlusion", "sigma"), got[:3], want[:3]):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w.shape, name
        nan = torch.isnan(w)
        assert torch.equal(torch.isnan(g), nan), name
        assert torch.equal(bits(g)[~nan], bits(w)[~nan]), (name, int((bits(g)[~nan] != bits(w)[~nan]).sum()))
    assert got[3].dtype == torch.bool and torch.equal(got[3], want[3])
    assert got[4].dtype == torch.int32 and torch.equal(got[4], want[4])


def assert_all_fill(flow, occl, sigma):
    assert (bits(flow) == NAN_BITS).all() and (bits(occl) == ONE_BITS).all() and (bits(sigma) == INF_BITS).all()


@functools.lru_cache(maxsize=None)
def distinct_stores(H, W, n, device):
    """``case_stores``'s entries, each under a template of its own: entry k is template 10 + k (its identity frame) over the video
    frames 1 and 2, so that the lanes of a wave read different rows of the pointer tables and no template covers another's frame."""
    return tuple(make_store(H, W, {10 + k: const_planes(H, W), 1: ga.entry_planes(k, 1, H, W), 2: ga.entry_planes(k, 2, H, W)}, device=device)
                 for k in range(n))


def case_atlas(H, W, n, kind, device=DEV):
    from mft_amd import TrackAtlas
    if kind == "one template":
        return TrackAtlas([(0, st) for st in ga.case_stores(H, W, n, device)])
    return TrackAtlas([(10 + k, st) for k, st in enumerate(distinct_stores(H, W, n, device))])


# ---- 1. bitwise against the composition on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one template", "a template each"])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("H,W", [(2, 2), (2, 70), (9, 34), (24, 40), (37, 53)])
def test_results_from_is_the_composition_bitwise(H, W, T, n, kind):
    from mft_amd import ops
    assert T <= 5 or T == ops.TRACKSTORE_FLOW_COLUMNS + 1                             # one more than a workgroup walks
    atlas = case_atlas(H, W, n, kind)
    cols = [atlas.frames[(3 * i + i // 4) % len(atlas.frames)] for i in range(T)]    # repeats, no order
    for src in (1, 2):
        got = atlas.results_from(src, cols)
        assert got[0].shape == (T, 2, H, W) and got[1].shape == (T, 1, H, W) and got[2].shape == (T, 1, H, W)
        assert_same(got, device_composition(atlas, src, cols))
    if n == 5 and (H, W) in ((9, 34), (24, 40), (37, 53)):
        e = atlas.inverse(1)[2]
        won = [int((e == k).sum()) for k in range(5)]
        print(f"{H}x{W} {kind}: entries win {won} pixels on frame 1, {int((e < 0).sum())} not found")
        assert sum(w > 0 for w in won) >= 3                                           # the winners do interleave
        row = e.reshape(-1)[:64 * ((H * W) // 64)].reshape(-1, 64)
        assert ((row.max(dim=1).values != row.min(dim=1).values).sum() > 0)          # ... within a wave's 64 pixels


# ---- 2. against the host atlas -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(13, 21), (24, 40)])
def test_device_and_host_atlas_agree(H, W):
    """Within what tests/test_gpu_track_inverse.py::test_results_from_on_the_device accepts between the device sampler and torch's:
    1e-5 px, 1e-6, 1e-6.  Measured: 1.9e-06 / 6.0e-08 / 2.4e-07 at 13 x 21, 3.8e-06 / 3.0e-08 / 1.2e-07 at 24 x 40."""
    from mft_amd import TrackAtlas
    dev = TrackAtlas(list(enumerate(host.two_template_stores(H, W, device=DEV, amp=5.0))))
    cpu = TrackAtlas(list(enumerate(host.two_template_stores(H, W, amp=5.0))))
    got, want = dev.results_from(2), cpu.results_from(2)
    assert torch.equal(got[3].cpu(), want[3]) and torch.equal(got[4].cpu(), want[4])
    t = want[4].numpy()
    assert (t == 0).any() and (t == 1).any()
    for name, g, w, tol in (("flow", got[0], want[0], 1e-5), ("occlusion", got[1], want[1], 1e-6), ("sigma", got[2], want[2], 1e-6)):
        g = g.cpu()
        fill = torch.isnan(want[0][:, 0:1]).expand_as(w)                               # not found, or not covered: per pixel and column
        assert torch.equal(bits(g)[fill], bits(w)[fill]) and fill.any() and not fill.all()
        err = float((g[~fill] - w[~fill]).abs().max())
        print(f"{H}x{W} {name}: device and host differ by at most {err:.3g} (accepted: {tol:g})")
        assert err <= tol


# ---- 3. stores of three chunks, a joined template with uncovered columns inside a column block -----------------------------------
def test_three_chunks_and_a_joined_template():
    from mft_amd import TrackAtlas
    H, W = 24, 40
    fwd = make_store(H, W, {f: (const_planes(H, W) if f == 5 else field(f, H, W, 1.5)) for f in (5, 6, 7, 8, 9)}, device=DEV, frames_per_chunk=2)
    bwd = make_store(H, W, {f: (const_planes(H, W) if f == 5 else field(f, H, W, 1.5)) for f in (5, 4, 3, 2, 1)}, device=DEV, frames_per_chunk=2)
    other = make_store(H, W, {11: const_planes(H, W), 10: field(10, H, W, 1.5), 7: field(17, H, W, 5.0)}, device=DEV, frames_per_chunk=2)
    assert len(fwd._chunks) == 3 and len(bwd._chunks) == 3 and len(other._chunks) == 2
    atlas = TrackAtlas([(5, fwd), (5, bwd), (11, other)])
    cols = [1, 9, 10, 2, 8, 11, 3, 7, 10, 4, 6, 11, 5, 12, 7, 1, 9, 11, 10, 2]        # 10, 11 (and 12): not covered by template 5
    assert atlas.covered(5, cols)[:6] == [True, True, False, True, True, False] and atlas.covered(11, cols)[:6] == [False, False, True, False, False, True]
    for src in (7, 3):
        got = atlas.results_from(src, cols)
        assert_same(got, device_composition(atlas, src, cols))
        if src == 7:
            t = got[4]
            print(f"frame 7: template 5 wins {int((t == 5).sum())} pixels, template 11 {int((t == 11).sum())}, {int((t < 0).sum())} not found")
            assert (t == 5).any() and (t == 11).any()
            five = (t == 5)
            assert (bits(got[0][2])[:, five] == NAN_BITS).all() and torch.isfinite(got[0][1][:, five]).all()
            assert (bits(got[0][13]) == NAN_BITS).all()                                # frame 12: nobody's


# ---- 4. nothing is found -----------------------------------------------------------------------------------------------------
def test_a_source_that_nothing_maps_into():
    from mft_amd import TrackAtlas
    H, W = 24, 40
    st = make_store(H, W, {0: const_planes(H, W), 7: shifted_out_planes(H, W), 2: field(1, H, W, 1.5)}, device=DEV)
    atlas = TrackAtlas([(0, st)])
    flow, occl, sigma, found, template = atlas.results_from(7)
    assert not found.any() and (template == -1).all() and flow.shape == (3, 2, H, W)
    assert_all_fill(flow, occl, sigma)


# ---- 5. special values -------------------------------------------------------------------------------------------------------
def test_nan_and_inf_come_out_as_the_composition_has_them():
    from mft_amd import TrackAtlas
    s0, s1 = host.two_template_stores(host.AH, host.AW, device=DEV, amp=1.5)
    host.with_sigma_range(s0, 0.5, float("inf"))          # template 0's frame 1: sigma +inf wherever its word is not 0 (NaN where it is)
    host.with_sigma_range(s1, float("nan"))               # template 1's own frame: sigma NaN, which counts as +0 in the key
    atlas = TrackAtlas([(0, s0), (1, s1)])
    seen_inf = seen_nan = 0
    for src in (1, 2):
        got = atlas.results_from(src)
        want = device_composition(atlas, src, atlas.frames)
        assert_same(got, want)
        found = want[3]
        read = found[None] & ~torch.isnan(want[0][:, 0])                             # found, and the column covered: no fill
        seen_inf += int(torch.isposinf(want[2][:, 0][read]).sum())
        seen_nan += int(torch.isnan(want[2][:, 0][read]).sum())
    print(f"sigma of found pixels: {seen_inf} +inf, {seen_nan} NaN")
    assert seen_inf > 0 and seen_nan > 0


# ---- 6. reproducibility, bounds, the columns a workgroup walks ------------------------------------------------------------------
def test_same_bits_every_time_nothing_else_written_whatever_the_column_blocks():
    from mft_amd import ops
    H, W, T = 37, 53, 21
    atlas = case_atlas(H, W, 5, "a template each")
    cols = [atlas.frames[(3 * i + i // 4) % len(atlas.frames)] for i in range(T)]
    want = device_composition(atlas, 2, cols)
    runs = []
    for _ in range(2):
        big = [torch.full((T + 2, c, H, W), -7.0, device=DEV) for c in (2, 1, 1)]
        out = tuple(b[1:T + 1] for b in big)
        got = atlas.results_from(2, cols, out=out)
        assert all(g is o for g, o in zip(got[:3], out))
        assert_same(got, want)
        assert all((b[0] == -7).all() and (b[T + 1] == -7).all() for b in big)
        runs.append(big)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*runs))
    table, _, entry = atlas.inverse(2)
    for cpb in (1, 3, 64):                                                            # a tuning choice, not a result
        out = tuple(torch.full((T, c, H, W), -7.0, device=DEV) for c in (2, 1, 1))
        ops.trackstore_flow_from(table, entry, *atlas._flow_tables(cols), *out, columns_per_block=cpb)
        assert all(torch.equal(bits(o), bits(b[1:T + 1])) for o, b in zip(out, runs[0])), cpb
    with pytest.raises(ValueError):
        atlas.results_from(2, cols, out=(out[0], out[1], out[2].cpu()))
    with pytest.raises(ValueError):
        atlas.results_from(2, cols, out=(out[0], out[1][:-1], out[2]))
    with pytest.raises(KeyError):
        atlas.results_from(99, cols)


# ---- 7. through the engine ---------------------------------------------------------------------------------------------------
def test_results_from_a_mid_video_frame_through_the_engine():
    from mft_amd import TrackAtlas
    from mft_amd.results import FlowOUTrackingResult
    fwd, bwd = (p[0] for p in ga.passes_with_stores(1))
    atlas = TrackAtlas.from_passes(fwd, bwd)
    mid, last = 6, ga.N_FRAMES - 1
    assert [t for t, _ in atlas.entries] == [0, 3, 5, 7, 11] and atlas.frames == list(range(ga.N_FRAMES))
    got = atlas.results_from(mid)
    assert_same(got, device_composition(atlas, mid, atlas.frames))
    flow, occl, sigma, found, template = got
    alone = {s: int((st.inverse(mid)[1] >= 0).sum()) for s, st in atlas.entries if mid in st._slot_of}
    print(f"frame {mid}: the atlas finds {int(found.sum())} of {found.numel()} pixels; single stores {alone}; "
          f"winners {dict(zip(*(a.tolist() for a in np.unique(template.cpu().numpy(), return_counts=True))))}")
    assert int(found.sum()) >= max(alone.values())
    r, f2, t2 = atlas.result_from(mid, last)
    assert isinstance(r, FlowOUTrackingResult) and torch.equal(f2, found) and torch.equal(t2, template)
    assert torch.equal(bits(r.flow), bits(flow[last])) and torch.equal(bits(r.sigma), bits(sigma[last]))
    img = torch.from_numpy(ga._video()[mid].astype(np.float32)).to(DEV)
    warped = r.warp_forward_device(img, mask=found)
    assert warped.shape == img.shape and torch.isfinite(warped).all()
    followed = found & torch.isfinite(r.flow).all(dim=0)                              # found AND its template covers the last frame
    assert followed.any() and torch.isfinite(r.sigma[0][followed]).all()
