"""``TrackAtlas.best_query_from`` on the device (csrc/trackstore.hip: ts_tracks_best_kernel through
``atlas_ops.trackstore_tracks_from_best``) against the composition it fuses -- ``TrackAtlas._compose_best_points`` on device tensors:
per-candidate ``atlas.query``, ``chain_behind_inverse`` and the key minimum in torch, from the same located rows -- bit for bit
wherever the expected value is no NaN and NaN exactly where it is one; against the host atlas wherever the choice is unambiguous;
through a ``MultiTemplateMFT`` pass; and behind a stalled stream."""
import numpy as np
import pytest
import torch

import stream_catalog as cat
import stream_harness as sh
import test_track_atlas as host
import test_gpu_track_atlas as ga
import test_track_atlas_best as hb
import test_track_atlas_points as hp
from test_gpu_streams_ops import run_behind_stall
from test_gpu_track_atlas_best import columns
from test_gpu_track_atlas_flow import bits, case_atlas
from test_track_atlas_flow import INF_BITS, NAN_BITS, ONE_BITS
from test_track_locate import const_planes, field, make_store

pytestmark = pytest.mark.gpu
DEV = "cuda"


def composition(atlas, pts, frame, cols, thr=0.5):
    """The definition on device tensors -> (table, entry, template)."""
    xy = torch.as_tensor(pts, dtype=torch.float32).to(DEV)
    N = int(xy.shape[0])
    groups, holders = atlas._point_groups(frame, N, "composition")
    tq, cq = atlas._locate_candidates(xy, groups, holders, thr)
    table, entry = atlas._compose_best_points(tq, cq, groups, holders, cols, thr, N)
    tmpl_of = torch.tensor([f for f, _ in atlas.entries], dtype=torch.int32, device=DEV)
    return table, entry, torch.where(entry >= 0, tmpl_of[entry.clamp(min=0).long()], torch.full_like(entry, -1))


def same(got, want):
    """Bits where the expected value is no NaN, NaN-ness elsewhere; entry and template equal."""
    assert got[0].is_cuda and got[0].dtype == torch.float32 and got[0].shape == want[0].shape and got[0].is_contiguous()
    nan = torch.isnan(want[0])
    assert torch.equal(torch.isnan(got[0]), nan)
    assert torch.equal(bits(got[0])[~nan], bits(want[0])[~nan]), int((bits(got[0])[~nan] != bits(want[0])[~nan]).sum())
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == torch.int32 and g.is_cuda and torch.equal(g, w), int((g != w).sum())


def assert_all_fill(table, entry):
    assert (bits(table[..., 0:2]) == NAN_BITS).all() and (bits(table[..., 2]) == ONE_BITS).all() and (bits(table[..., 3]) == INF_BITS).all()
    assert (entry == -1).all()


def frame_ids(N):
    """One source frame, and the N points spread over frames 1 and 2: 1 + the rest, 64 + 65 (of 129 or more), alternating."""
    ids = [("one frame", 1)]
    if N >= 2:
        ids += [("1 + the rest", [2] + [1] * (N - 1)), ("alternating", [1 + i % 2 for i in range(N)])]
    if N >= 129:
        ids.append(("64 + 65", [2] * 64 + [1] * 65 + [2] * (N - 129)))
    return ids


# ---- 1. bitwise against the composition on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one template", "a template each"])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("H,W", [(2, 2), (2, 70), (9, 34), (24, 40), (37, 53)])
def test_best_query_from_is_the_composition_bitwise(H, W, T, n, kind):
    from mft_amd import atlas_ops
    assert T <= 5 or T == atlas_ops.TRACKSTORE_POINTS_COLUMNS + 1                     # one more than a workgroup walks
    atlas = case_atlas(H, W, n, kind)
    cols = columns(atlas, T)
    assert len(atlas._holders(1)) == n and len(atlas._holders(2)) == n
    for N in (1, 63, 64, 65, 130):                                                    # a tile, one point less, one more, two and a bit
        pts = hp.mixed_points(H, W, N)
        for what, ids in frame_ids(N):
            got = atlas.best_query_from(torch.from_numpy(pts).to(DEV), ids, cols)
            assert got[0].shape == (N, T, 4) and got[1].shape == (N, T) and got[2].shape == (N, T)
            same(got, composition(atlas, pts, ids, cols))
    if n == 5 and T == 17 and kind == "a template each" and (H, W) in ((9, 34), (24, 40), (37, 53)):
        e = atlas.best_query_from(hp.off_grid_points(H, W, 128), 1, cols)[1]           # [128, T]: two whole tiles
        won = [int((e == k).sum()) for k in range(5)]
        print(f"{H}x{W}: candidates win {won} point-columns from frame 1, {int((e < 0).sum())} are fill")
        assert sum(w > 0 for w in won) >= 3                                           # the winners do interleave
        tile = e.reshape(2, 64, T)
        assert (tile.max(dim=1).values != tile.min(dim=1).values).any()               # ... within a tile's 64 points
        assert (e.max(dim=1).values != e.min(dim=1).values).any()                     # ... and across the columns of one point


def test_the_three_template_atlas_and_host_points():
    for H, W in ((13, 21), (24, 40)):
        atlas = hb.three_templates(H, W, 1.5, device=DEV)
        pts = hp.case_points(H, W)
        for src in hp.SOURCES:
            for cols in (atlas.frames, [3, 0, 0, 2, 1]):
                same(atlas.best_query_from(pts[src], src, cols), composition(atlas, pts[src], src, cols))     # (host points: uploaded)
        every = np.concatenate([pts[s] for s in hp.SOURCES])
        ids = np.repeat(hp.SOURCES, hp.N_POINTS)
        mix = np.random.default_rng(5).permutation(len(ids))
        got = atlas.best_query_from(every[mix], ids[mix])
        same(got, composition(atlas, every[mix], ids[mix], atlas.frames))
        for src in hp.SOURCES:                                                         # row by row one call per frame
            at = torch.from_numpy(ids[mix] == src).to(DEV)
            one = atlas.best_query_from(every[mix][ids[mix] == src], src)
            assert all(torch.equal(bits(g[at]), bits(w)) for g, w in zip(got, one))
        c, o, found, template = atlas.best_tracks_from(pts[2], 2)
        old = atlas.tracks_from(pts[2], 2)
        assert np.isnan(old[0][:, 0:2]).all() and found[:, 0:2].mean() > 0.9 and (~found).mean() <= 0.05
        assert np.array_equal(found, got[1].cpu().numpy()[np.argsort(mix)][hp.N_POINTS:2 * hp.N_POINTS] >= 0)


# ---- 2. stores of three chunks, a joined template with uncovered columns inside a column block -----------------------------------
def test_three_chunks_and_a_joined_template():
    from mft_amd import TrackAtlas
    H, W = 24, 40
    fwd = make_store(H, W, {f: (const_planes(H, W) if f == 5 else field(f, H, W, 1.5)) for f in (5, 6, 7, 8, 9)}, device=DEV, frames_per_chunk=2)
    bwd = make_store(H, W, {f: (const_planes(H, W) if f == 5 else field(f, H, W, 1.5)) for f in (5, 4, 3, 2, 1)}, device=DEV, frames_per_chunk=2)
    other = make_store(H, W, {11: const_planes(H, W), 10: field(10, H, W, 1.5), 7: field(17, H, W, 5.0)}, device=DEV, frames_per_chunk=2)
    assert len(fwd._chunks) == 3 and len(bwd._chunks) == 3 and len(other._chunks) == 2
    atlas = TrackAtlas([(5, fwd), (5, bwd), (11, other)])
    cols = [1, 9, 10, 2, 8, 11, 3, 7, 10, 4, 6, 11, 5, 12, 7, 1, 9, 11, 10, 2]        # 10, 11 (and 12): not covered by template 5
    pts = hp.mixed_points(H, W, 100)
    for ids in (7, 3, 5, [(7, 3, 5, 10)[i % 4] for i in range(100)]):
        got = atlas.best_query_from(pts, ids, cols)
        same(got, composition(atlas, pts, ids, cols))
        if ids == 7:
            t = got[2]
            print(f"from frame 7: template 5 wins {int((t == 5).sum())} point-columns, template 11 {int((t == 11).sum())}, {int((t < 0).sum())} fill")
            assert (t[:, 1] == 5).any() and (t[:, 1] != 11).all()                      # frame 9: template 5 alone covers it
            assert (t[:, 2] == 11).any() and (t[:, 2] != 5).all()                      # frame 10: template 11 alone
            assert (t[:, 7] == 5).any() and (t[:, 7] == 11).any()                      # frame 7: both, interleaved
            assert_all_fill(got[0][:, 13], got[1][:, 13])                              # frame 12: nobody's


# ---- 3. special values -------------------------------------------------------------------------------------------------------
def test_nan_and_inf_come_out_as_the_composition_has_them():
    from mft_amd import TrackAtlas
    s0, s1 = host.two_template_stores(host.AH, host.AW, device=DEV, amp=1.5)
    host.with_sigma_range(s0, 0.5, float("inf"))          # template 0's frame 1: sigma +inf wherever its word is not 0 (NaN where it is)
    host.with_sigma_range(s1, float("nan"))               # template 1's own frame: sigma NaN
    atlas = TrackAtlas([(0, s0), (1, s1)])
    pts = np.concatenate([hp.mixed_points(host.AH, host.AW, 70), hp.grid(host.AH, host.AW)])
    seen_inf = seen_nan = 0
    for src in (1, 2):
        got = atlas.best_query_from(pts, src)
        want = composition(atlas, pts, src, atlas.frames)
        same(got, want)
        read = want[1] >= 0
        seen_inf += int(torch.isposinf(want[0][..., 3][read]).sum())
        seen_nan += int(torch.isnan(want[0][..., 3][read]).sum())
    print(f"sigma of answered point-columns: {seen_inf} +inf, {seen_nan} NaN")
    assert seen_inf > 0 and seen_nan > 0


# ---- 4. reproducibility, bounds, the columns a workgroup walks ------------------------------------------------------------------
def test_same_bits_every_time_nothing_else_written_whatever_the_column_blocks():
    from mft_amd import atlas_ops
    H, W, T, N = 37, 53, 21, 130
    atlas = case_atlas(H, W, 5, "a template each")
    cols = columns(atlas, T)
    pts = torch.from_numpy(hp.mixed_points(H, W, N)).to(DEV)
    ids = [1 + (i // 3) % 2 for i in range(N)]
    want = composition(atlas, pts, ids, cols)
    first = atlas.best_query_from(pts, ids, cols)
    same(first, want)
    for _ in range(4):
        again = atlas.best_query_from(pts, ids, cols)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, first))
    groups, holders = atlas._point_groups(ids, N, "test")
    tq, cq = atlas._locate_candidates(pts, groups, holders, 0.5)
    host_tables = atlas._points_tables(groups, holders, cols, N)
    for cpb in (1, 4, 16, 0, T):                                                      # a tuning choice, not a result
        big = [torch.full((N + 2, T, 4), -7.0, device=DEV), torch.full((N + 2, T), -7, dtype=torch.int32, device=DEV)]
        atlas_ops.trackstore_tracks_from_best(tq, cq, *host_tables, (H, W), big[0][1:N + 1], big[1][1:N + 1], columns_per_block=cpb)
        assert all(torch.equal(bits(b[1:N + 1]), bits(f)) for b, f in zip(big, first)), cpb
        assert all((b[0] == -7).all() and (b[N + 1] == -7).all() for b in big), cpb
    big = [torch.full((N + 2, T, 4), -7.0, device=DEV), torch.full((N + 2, T), -7, dtype=torch.int32, device=DEV)]
    got = atlas.best_query_from(pts, ids, cols, out=(big[0][1:N + 1], big[1][1:N + 1]))
    assert got[0].data_ptr() == big[0][1].data_ptr() and all(torch.equal(bits(g), bits(f)) for g, f in zip(got, first))
    assert all((b[0] == -7).all() and (b[N + 1] == -7).all() for b in big)
    with pytest.raises(ValueError):
        atlas.best_query_from(pts, ids, cols, out=(first[0], first[1].cpu()))
    with pytest.raises(KeyError):
        atlas.best_query_from(pts, 99, cols)
    # no candidates at all: everything is fill
    out = (torch.full((N, 2, 4), -7.0, device=DEV), torch.full((N, 2), -7, dtype=torch.int32, device=DEV))
    atlas_ops.trackstore_tracks_from_best(tq[:0], cq[:0], [1, N - 1], [0, 0], [], [], np.arange(N)[::-1], np.zeros((0, 2), np.int64),
                                          np.zeros((0, 2), np.int64), (H, W), *out)
    assert_all_fill(*out)
    # empty calls launch nothing
    e = atlas.best_query_from(pts[:0], 1, cols)
    assert e[0].shape == (0, T, 4) and e[0].is_cuda and e[1].shape == (0, T)
    e = atlas.best_query_from(pts, ids, [])
    assert e[0].shape == (N, 0, 4) and e[2].shape == (N, 0) and e[2].is_cuda


# ---- 5. against the host atlas -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,amp", hb.HOST_CASES)
def test_device_and_host_atlas_agree_where_the_choice_is_unambiguous(H, W, amp):
    """``entry`` equal wherever the host's own candidates leave no doubt (tests/test_track_atlas_points.py: ``ambiguous_points``), and
    there x and y, occlusion and sigma within what tests/test_gpu_track_atlas_best.py accepts between the device sampler and torch's:
    1e-5 px, 1e-6, 1e-6."""
    cpu, pts, per_src = hp.points_case(H, W, amp)
    dev = hb.three_templates(H, W, amp, device=DEV)
    worst = {"xy": 0.0, "occlusion": 0.0, "sigma": 0.0}
    for src in hp.SOURCES:
        want, amb, answered = per_src[src]
        got = [t.cpu().numpy() for t in dev.best_query_from(pts[src], src)]
        assert amb.sum() / answered.sum() <= hb.AMBIGUOUS_CAP
        clear = answered & ~amb
        assert np.array_equal(got[1] < 0, want[1] < 0) and np.array_equal(got[1] < 0, ~answered)
        assert np.array_equal(got[1][clear], want[1][clear]) and np.array_equal(got[2][clear], want[2][clear])
        hp.assert_fill_rows(got[0], got[1], got[2], ~answered)
        for name, sl, tol in (("xy", slice(0, 2), 1e-5), ("occlusion", slice(2, 3), 1e-6), ("sigma", slice(3, 4), 1e-6)):
            err = float(np.abs(got[0][..., sl][clear] - want[0][..., sl][clear]).max())
            worst[name] = max(worst[name], err)
            assert err <= tol, (name, src, err)
        print(f"{H}x{W} amp {amp} from {src}: {int(amb.sum())} of {int(answered.sum())} answered point-columns ambiguous; another winner than "
              f"the host's on {int((got[1] != want[1]).sum())}")
    print(f"{H}x{W} amp {amp}: device and host differ by at most " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + " (accepted: 1e-05, 1e-06, 1e-06)")


# ---- 6. through the engine ---------------------------------------------------------------------------------------------------
def test_backward_columns_from_a_mid_video_template_frame_through_the_engine():
    from mft_amd import TrackAtlas
    fwd, bwd = (p[0] for p in ga.passes_with_stores(1))
    atlas = TrackAtlas.from_passes(fwd, bwd)
    mid = 5                                                # a template of the forward pass: its store holds frames 5 .. 11 only
    assert atlas._holders(mid) == [0, 1, 2, 3, 4] and atlas.covered(mid)[:mid] == [False] * mid
    ys, xs = np.mgrid[8:atlas.H:30, 8:atlas.W:30]
    pts = np.stack([xs.ravel() + 0.25, ys.ravel() + 0.5], axis=1).astype(np.float32)
    coords, occl, found, template = atlas.tracks_from(pts, mid)
    assert (template == mid).all() and np.isnan(coords[:, :mid]).all()                 # template 5 wins every point: the columns before it are fill
    got = atlas.best_query_from(pts, mid)
    same(got, composition(atlas, pts, mid, atlas.frames))
    c, o, f, t = atlas.best_tracks_from(pts, mid)
    shares = f.mean(axis=0)
    print(f"from frame {mid}: answered share per column {[round(float(s), 3) for s in shares]}; winners "
          f"{dict(zip(*(a.tolist() for a in np.unique(t, return_counts=True))))}")
    assert (shares[:mid] > 0).all() and (t[:, :mid] != mid).all() and (t[:, mid] == mid).all()
    assert np.isfinite(c[f]).all() and np.array_equal(f, got[1].cpu().numpy() >= 0)
    both = ~np.isnan(coords[:, :, 0])
    assert f[both].all() and np.array_equal(hp.bits(c[:, mid:][t[:, mid:] == mid]), hp.bits(coords[:, mid:][t[:, mid:] == mid]))
    spread = np.repeat(pts, 2, axis=0)                                                 # ... and points given on two frames of the video
    ids = [mid, 8] * len(pts)
    same(atlas.best_query_from(spread, ids), composition(atlas, spread, ids, atlas.frames))


# ---- 7. stream ordering ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


@pytest.fixture(scope="module")
def cycles_per_ms():
    return sh.calibrate()


POINT_GROUPS = ([3, 64], [64, 3])            # the groups of the first and of the second call behind one stall: two tiles either way


def _points_fixed(ops):
    """The located rows of two candidates per group: template points about the frame, occlusion and sigma, cells with holes.  Address
    material: the same for every input set."""
    rows, cells = [], []
    for k in range(4):
        xy = cat._points(cat.NQ, 20 + k)
        r = np.random.default_rng(300 + k)
        rows.append(torch.cat([xy, torch.from_numpy(r.uniform(0, 0.6, (cat.NQ, 1)).astype(np.float32)),
                               torch.from_numpy(r.uniform(0.05, 1.0, (cat.NQ, 1)).astype(np.float32))], dim=1))
        cells.append(torch.from_numpy(((np.arange(cat.NQ) + k) % 5 - 1).astype(np.int32)))
    # rows run group after group, candidate after candidate: 2 x 3 + 2 x 64 (or 2 x 64 + 2 x 3) -- 134 either way
    return {"located": torch.cat([t[:cat.NQ] for t in rows])[:2 * cat.NQ].contiguous().to(DEV),
            "cells": torch.cat(cells)[:2 * cat.NQ].contiguous().to(DEV)}


def _points_call(ops, fx, inp, v=0):
    from mft_amd import atlas_ops
    slots = np.asarray(cat.FLOW_COLUMNS[v])
    frame_ptrs, lohi_ptrs = ops.trackstore_slot_addresses(*cat._chunks(inp), slots)
    T = slots.shape[1]
    order = np.arange(cat.NQ) if v == 0 else np.arange(cat.NQ)[::-1]
    return list(atlas_ops.trackstore_tracks_from_best(fx["located"], fx["cells"], POINT_GROUPS[v], [2, 2], [0, 1, 0, 1] if v == 0 else [3, 2, 1, 0],
                                                      [0, 1, 1, 0] if v == 0 else [1, 0, 0, 1], order, frame_ptrs, lohi_ptrs, (cat.HF, cat.WF),
                                                      torch.full((cat.NQ, T, 4), -7.0, device=DEV),
                                                      torch.full((cat.NQ, T), -7, dtype=torch.int32, device=DEV), columns_per_block=2))


POINTS_ENTRY = cat.Entry("trackstore_tracks_from_best", ("trackstore_tracks_from_best",), _points_fixed, cat._store, _points_call, True, None)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("variants", [(0,), (0, 1)], ids=["one call", "table uploads back to back"])
def test_tracks_from_best_runs_on_its_stream(ops, cycles_per_ms, variants):
    run_behind_stall(ops, POINTS_ENTRY, cycles_per_ms, variants=variants)
