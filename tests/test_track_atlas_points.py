"""``TrackAtlas.best_query_from`` / ``best_tracks_from`` on the host (device="cpu"): points given on any video frame(s) followed with
the template chosen per point AND destination frame -- every entry that holds a point's frame locates it by itself, follows its own
template point through its template's stores, chains, and the smallest (occluded, chained sigma, rank) wins.  No GPU needed; the stores
are those of tests/test_track_atlas_best.py.

``off_grid_points``, ``mixed_points``, ``case_points``, ``candidate_rows``, ``ambiguous_points`` and ``points_case`` are shared with
tests/test_gpu_track_atlas_points.py."""
import functools

import numpy as np
import pytest
import torch

from mft_amd.trackstore import chain_behind_inverse
from test_track_atlas import CH, CW, joined_atlas, two_template_stores
from test_track_atlas_best import AMBIGUITY, AMBIGUOUS_CAP, HOST_CASES, THR, corner_store, key_of, set_range, three_templates
from test_track_atlas_flow import INF_BITS, NAN_BITS, ONE_BITS
from test_track_inverse import grid
from test_track_locate import bits, const_planes, field, make_store, shifted_out_planes

N_POINTS = 130                   # per source frame: three tiles of the device kernel, the last one of two points
SOURCES = (1, 2, 3)


def off_grid_points(H, W, n=N_POINTS, seed=7):
    """n seeded points inside the frame, off the pixel grid: float32 (n, 2) xy."""
    r = np.random.default_rng(seed)
    return (r.random((n, 2)) * np.array([W - 1, H - 1])).astype(np.float32)


def mixed_points(H, W, n, seed=3):
    """n points: off-grid ones, pixel centres, duplicates, points outside the frame and NaN."""
    pts = off_grid_points(H, W, n, seed)
    g = grid(H, W)
    for i in range(n):
        kind = i % 9
        if kind == 2:
            pts[i] = g[(7 * i) % len(g)]
        elif kind == 4 and i >= 4:
            pts[i] = pts[i - 4]
        elif kind == 6:
            pts[i] = (W + 3.5, -2.25) if i % 2 else (-1.5, H + 0.75)
        elif kind == 8:
            pts[i] = (np.nan, 1.0) if i % 2 else (np.nan, np.nan)
    return pts


def candidate_rows(atlas, pts, src, cols, thr=THR):
    """Per candidate of ``src`` its own chained answer to the points, on the atlas's device -> (ranks, ok [E, T, N] bool, rows
    [E, N, T, 4]): ``store.locate``, ``atlas.query`` on the candidate's template, ``chain_behind_inverse`` with a grid of zeros."""
    ranks = atlas._holders(src)
    xy = torch.as_tensor(pts, dtype=torch.float32).to(atlas.device)
    oks, rows = [], []
    for r in ranks:
        s, st = atlas.entries[r]
        tb, cell = st.locate(xy, src, thr)
        found = cell >= 0
        at = torch.where(found[:, None], tb[:, 0:2], torch.zeros((), device=tb.device))
        ok = found[:, None] & torch.tensor(atlas.covered(s, cols), dtype=torch.bool, device=tb.device)[None, :]
        p, o, sg = chain_behind_inverse(tb, atlas.query(s, at, cols), torch.zeros_like(at), ok)
        oks.append(ok.t())
        rows.append(torch.cat([p, o[:, None], sg[:, None]], dim=1).permute(2, 0, 1))
    return ranks, torch.stack(oks), torch.stack(rows)


def ambiguous_points(atlas, pts, src, cols, thr=THR):
    """tests/test_track_atlas_best.py's ``ambiguous`` for points, from the atlas's own candidates alone -> (ambiguous [N, T] bool,
    answered [N, T] bool) as numpy: the best and the second-best candidate agree in ``occluded`` and differ in sigma by less than
    AMBIGUITY, or some candidate's chained occlusion is within AMBIGUITY of the threshold."""
    ranks, ok, rows = candidate_rows(atlas, pts, src, cols, thr)
    ok, rows = ok.cpu().numpy(), rows.cpu().numpy()
    o, s = rows[:, :, :, 2].transpose(0, 2, 1), rows[:, :, :, 3].transpose(0, 2, 1)                # [E, T, N]
    none = np.iinfo(np.int64).max
    key = np.where(ok, key_of(o, s, np.asarray(ranks)[:, None, None], thr), none)
    answered = ok.any(axis=0)
    with np.errstate(invalid="ignore"):
        near_thr = (ok & (np.abs(o - np.float32(thr)) < AMBIGUITY)).any(axis=0)
        close = np.zeros_like(answered)
        if len(ranks) >= 2:
            order = np.argsort(key, axis=0)
            a, b = order[0][None], order[1][None]
            both = np.take_along_axis(ok, b, 0)[0]
            oa, ob = (~(np.take_along_axis(o, i, 0)[0] <= np.float32(thr)) for i in (a, b))
            sa, sb = (np.take_along_axis(s, i, 0)[0] for i in (a, b))
            close = answered & both & (oa == ob) & ~(np.abs(sa - sb) >= AMBIGUITY)
    return ((near_thr | close) & answered).T, answered.T


def case_points(H, W, n=N_POINTS, seed=7):
    """{source frame: n off-grid points}: one generator, frames 1, 2, 3 drawn one after the other."""
    r = np.random.default_rng(seed)
    return {src: (r.random((n, 2)) * np.array([W - 1, H - 1])).astype(np.float32) for src in SOURCES}


@functools.lru_cache(maxsize=None)
def points_case(H, W, amp):
    """-> (the host atlas, {src: its points}, {src: (best_query_from(points, src) as numpy, ambiguous, answered)}): computed once."""
    atlas = three_templates(H, W, amp)
    pts = case_points(H, W)
    per_src = {}
    for src in SOURCES:
        got = tuple(t.numpy() for t in atlas.best_query_from(pts[src], src))
        per_src[src] = (got,) + ambiguous_points(atlas, pts[src], src, atlas.frames)
    return atlas, pts, per_src


def same_rows(got, want):
    """Bits where the expected value is no NaN, NaN-ness elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def assert_fill_rows(table, entry, template, where):
    t, e, m = np.asarray(table), np.asarray(entry), np.asarray(template)
    assert (bits(t[..., 0])[where] == NAN_BITS).all() and (bits(t[..., 1])[where] == NAN_BITS).all()
    assert (bits(t[..., 2])[where] == ONE_BITS).all() and (bits(t[..., 3])[where] == INF_BITS).all()
    assert (e[where] == -1).all() and (m[where] == -1).all()


# ---- 1. the brute force ------------------------------------------------------------------------------------------------------
def brute_force(atlas, pts, srcs, cols, thr=THR):
    """The definition with a loop per point, column and candidate; selection in plain Python.  srcs: a frame id per point."""
    N, T = len(pts), len(cols)
    table = np.empty((N, T, 4), np.float32)
    table[...] = (np.nan, np.nan, 1.0, np.inf)
    entry = np.full((N, T), -1, np.int32)
    thr32 = np.float32(thr)
    with np.errstate(all="ignore"):
        for n in range(N):
            src = int(srcs[n])
            cands = []
            for r, (s, st) in enumerate(atlas.entries):
                if src not in st._slot_of:
                    continue
                tb, cl = st.locate(pts[n:n + 1], src, thr)
                cands.append((r, s, tb.numpy()[0], int(cl[0])))
            for t, f in enumerate(cols):
                best = None
                for r, s, tb, cl in cands:
                    owner = next((o for tf, o in atlas.entries if tf == s and f in o._slot_of), None)
                    if cl < 0 or owner is None:
                        continue
                    qx, qy, o_dst, s_dst = owner.query(tb[None, 0:2], [f]).numpy()[0, 0]
                    o_src, s_src = tb[2], tb[3]
                    o = o_src if np.isnan(o_src) else (o_dst if np.isnan(o_dst) else max(o_src, o_dst))
                    sg = np.float32(np.sqrt(np.float64(np.float32(np.float32(s_src * s_src) + np.float32(s_dst * s_dst)))))
                    key = int(key_of(o, sg, r, thr).item())
                    assert key >> 39 == (0 if o <= thr32 else 1)
                    if best is None or key < best[0]:
                        best = (key, qx, qy, o, sg, r)
                if best is not None:
                    table[n, t] = best[1:5]
                    entry[n, t] = best[5]
    tmpl_of = np.asarray([f for f, _ in atlas.entries], np.int32)
    return table, entry, np.where(entry >= 0, tmpl_of[entry.clip(0)], -1).astype(np.int32)


def assert_same_points(got, want):
    same_rows(got[0].detach().cpu().numpy(), want[0])
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("H,W", [(13, 21), (24, 40)])
def test_equals_the_brute_force_bit_for_bit(H, W):
    atlas = three_templates(H, W, 5.0 if (H, W) == (13, 21) else 1.5)
    pts = mixed_points(H, W, 40)
    for src in SOURCES:
        for cols in (None, [0, 3, 1], [2, 2, 0], [3]):
            cols = atlas.frames if cols is None else cols
            got = atlas.best_query_from(pts, src, cols)
            assert got[0].shape == (40, len(cols), 4) and got[1].shape == (40, len(cols)) and got[2].shape == (40, len(cols))
            assert_same_points(got, brute_force(atlas, pts, [src] * 40, cols))
    joined = joined_atlas()[0]                               # a joined template (forward and backward store of template 5)
    pts = mixed_points(joined.H, joined.W, 20)
    for src in (6, 4):
        assert_same_points(joined.best_query_from(pts, src), brute_force(joined, pts, [src] * 20, joined.frames))


# ---- 2. the dense call on pixel centres --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,amp", [(13, 21, 5.0), (24, 40, 1.5)])
def test_pixel_centres_agree_with_best_results_from(H, W, amp):
    atlas = three_templates(H, W, amp)
    g = grid(H, W)
    T = len(atlas.frames)
    for src in SOURCES:
        table, entry, template = (t.numpy() for t in atlas.best_query_from(g, src))
        flow, occl, sigma, dentry, dtemplate = (t.numpy() for t in atlas.best_results_from(src))
        assert np.array_equal(entry.T.reshape(T, H, W), dentry) and np.array_equal(template.T.reshape(T, H, W), dtemplate)
        per_col = table.transpose(1, 0, 2).reshape(T, H, W, 4)
        assert np.array_equal(bits(per_col[..., 2]), bits(occl[:, 0])) and np.array_equal(bits(per_col[..., 3]), bits(sigma[:, 0]))
        gx, gy = g[:, 0].reshape(H, W), g[:, 1].reshape(H, W)
        for c, pixel in ((0, gx), (1, gy)):
            with np.errstate(invalid="ignore"):
                d = (per_col[..., c] - pixel[None]).astype(np.float32)
            known = ~np.isnan(flow[:, c])
            assert known.any() and np.array_equal(bits(d)[known], bits(flow[:, c])[known])
            assert np.isnan(per_col[..., c][~known]).all()


# ---- 3. several source frames in one call ------------------------------------------------------------------------------------
def test_frame_ids_per_point_in_any_order_are_one_call_per_frame():
    H, W = 13, 21
    atlas = three_templates(H, W, 5.0)
    pts = mixed_points(H, W, 70)
    pts[10:20] = pts[0:10]                                   # repeated points, given on other frames
    ids = np.random.default_rng(11).integers(1, 4, 70)
    ids[0:10], ids[10:20] = 2, 3
    for cols in (None, [3, 0, 3, 1, 0]):                     # ... and repeated columns
        got = [t.numpy() for t in atlas.best_query_from(pts, ids, cols)]
        for f in SOURCES:
            at = ids == f
            assert at.any()
            want = [t.numpy() for t in atlas.best_query_from(pts[at], f, cols)]
            same_rows(got[0][at], want[0])
            assert np.array_equal(got[1][at], want[1]) and np.array_equal(got[2][at], want[2])
        one = [t.numpy() for t in atlas.best_query_from(pts, [2] * 70, cols)]           # N ids of one frame: the single id
        want = [t.numpy() for t in atlas.best_query_from(pts, 2, cols)]
        same_rows(one[0], want[0])
        assert np.array_equal(one[1], want[1])
    c, o, found, template = atlas.best_tracks_from(pts, list(ids))
    t, e, m = (x.numpy() for x in atlas.best_query_from(pts, ids))
    assert c.shape == (70, 4, 2) and o.shape == (70, 4) and found.dtype == np.bool_ and template.dtype == np.int64
    same_rows(c, t[:, :, 0:2])
    assert np.array_equal(bits(o), bits(t[:, :, 2])) and np.array_equal(found, e >= 0) and np.array_equal(template, m)
    assert np.isnan(c[~found]).all() and (o[~found] == 1).all() and (template[~found] == -1).all() and found.any() and not found.all()


# ---- 4. the properties -------------------------------------------------------------------------------------------------------
def test_a_single_holder_equals_tracks_from():
    """Coordinates bit for bit; the occlusion is the chained maximum max(o_src, o_dst) where ``tracks_from`` returns o_dst alone."""
    from mft_amd import TrackAtlas
    s0, s1 = two_template_stores(amp=5.0)
    atlas = TrackAtlas([(0, s0), (1, s1)])
    assert atlas._holders(0) == [0]
    pts = mixed_points(atlas.H, atlas.W, 60)
    for cols in (None, [2, 0, 7]):                           # (7: nobody's)
        c, o, found, template = atlas.best_tracks_from(pts, 0, cols)
        wc, wo, wfound, wtemplate = atlas.tracks_from(pts, 0, cols)
        same_rows(c, wc)
        assert np.array_equal(found, ~np.isnan(wc[:, :, 0])) and np.array_equal(found.any(axis=1), wfound) and wfound.any()
        assert np.array_equal(template, np.where(found, wtemplate[:, None], -1))
        o_src = atlas.locate(pts, 0)[0][:, 2].numpy()
        assert np.array_equal(bits(o[found]), bits(np.maximum(o_src[:, None], wo)[found])) and (o[~found] == 1).all()
    # frame 1 of template 0 is no identity: the located occlusion is not 0, and the two occlusions do differ
    st = make_store(13, 21, {0: const_planes(13, 21), 1: field(3, 13, 21, 1.5), 2: field(4, 13, 21, 1.5)})
    one = TrackAtlas([(0, st)])
    c, o, found, _ = one.best_tracks_from(pts, 1)
    wc, wo, wfound, _ = one.tracks_from(pts, 1)
    same_rows(c, wc)
    o_src = one.locate(pts, 1)[0][:, 2].numpy()
    assert np.array_equal(bits(o[found]), bits(np.maximum(o_src[:, None], wo)[found])) and (o[found] > wo[found]).any()


@pytest.mark.parametrize("H,W,amp", HOST_CASES)
def test_never_worse_than_tracks_from(H, W, amp):
    atlas, all_pts, per_src = points_case(H, W, amp)
    for src in SOURCES:
        pts = all_pts[src]
        (table, entry, template), _, answered = per_src[src]
        wc, wo, wfound, wtemplate = atlas.tracks_from(pts, src)
        old = ~np.isnan(wc[:, :, 0])
        assert old.any() and (entry[old] >= 0).all()                                     # what tracks_from answers is answered
        assert np.array_equal(entry >= 0, answered)
        rank = atlas.locate(pts, src)[2].numpy()
        took_same = old & (entry == rank[:, None])                                       # the same entry: the same coordinates
        assert took_same.any() and np.array_equal(bits(table[:, :, 0:2][took_same]), bits(wc[took_same]))
        changes = int(((entry.max(axis=1) != entry.min(axis=1)) & (entry >= 0).all(axis=1)).sum())
        print(f"{H}x{W} amp {amp} from {src}: tracks_from leaves {1 - old.mean():.1%} of the point-columns unanswered, best_tracks_from "
              f"{(entry < 0).mean():.1%}; winners {[int((entry == r).sum()) for r in range(3)]}; the winner changes between the columns "
              f"of {changes} of {len(pts)} points")
        if src == 2:
            assert old.mean() == 0.5                                                     # template 2 holds neither frame 0 nor 1
            assert (entry < 0).mean() <= 0.05
            assert all((entry == r).any() for r in range(3))


# ---- 5. the key's corners, on exact inputs -----------------------------------------------------------------------------------
def corner_winner(stores, thr=THR):
    from mft_amd import TrackAtlas
    atlas = TrackAtlas([(10 + k, st) for k, st in enumerate(stores)])
    pts = np.array([[2.5, 3.25], [0.0, 0.0], [6.75, 4.5]], np.float32)
    table, entry, template = (t.numpy() for t in atlas.best_query_from(pts, 1, [2], thr))
    e = np.unique(entry)
    assert e.size == 1 and e[0] >= 0 and (template == 10 + e[0]).all() and float(np.abs(table[:, 0, 0:2] - pts).max()) <= 2.0 ** -9
    return int(e[0]), table[:, 0, 2], table[:, 0, 3]


def test_key_corners():
    w, o, s = corner_winner([corner_store(0, occl=0.9, sigma=0.125), corner_store(1, occl=0.0, sigma=4.0)])
    assert w == 1 and (o == 0).all() and (s == 4).all()                                  # visible beats occluded whatever the sigma
    w, o, s = corner_winner([corner_store(0, occl=0.9, sigma=0.125), corner_store(1, occl=0.0, sigma=4.0)], thr=1.0)
    assert w == 0 and (o == np.float32(0.9)).all() and (s == 0.125).all()                # neither occluded: the lower sigma
    assert corner_winner([corner_store(0, sigma=0.5), corner_store(1, sigma=0.25), corner_store(2, sigma=0.375)])[0] == 1
    assert corner_winner([corner_store(0, sigma=0.25), corner_store(1, sigma=0.25)])[0] == 0      # equal sigma: the rank breaks the tie
    nan = lambda k: set_range(corner_store(k), 3, float("nan"))  # noqa: E731
    huge = lambda k: set_range(corner_store(k), 3, 3.0e38)  # noqa: E731  (its square is +inf in float32)
    w, o, s = corner_winner([nan(0), huge(1)])
    assert w == 1 and (bits(s) == INF_BITS).all()                                        # a NaN sigma sorts behind +inf ...
    w, o, s = corner_winner([huge(0), corner_store(1, sigma=1000.0)])
    assert w == 1 and (s == 1000).all()                                                  # ... which loses to a number
    assert corner_winner([nan(0), corner_store(1, sigma=1000.0)])[0] == 1
    w, o, s = corner_winner([nan(0)])
    assert w == 0 and np.isnan(s).all()                                                  # alone it is the answer
    nan_occl = lambda k, sigma: set_range(corner_store(k, sigma=sigma), 2, float("nan"))  # noqa: E731
    assert corner_winner([nan_occl(0, 0.125), corner_store(1, occl=0.0, sigma=4.0)])[0] == 1       # a NaN occlusion is occluded
    w, o, s = corner_winner([corner_store(0, occl=0.9, sigma=4.0), nan_occl(1, 0.125)])
    assert w == 1 and np.isnan(o).all() and (s == 0.125).all()
    assert corner_winner([corner_store(0, occl=0.9, sigma=0.125), nan_occl(1, 4.0)])[0] == 0
    # the only candidate that covers the column is occluded: an answer, not the fill
    from mft_amd import TrackAtlas
    lone = make_store(CH, CW, {20: const_planes(CH, CW), 1: const_planes(CH, CW, sigma=0.125)})
    atlas = TrackAtlas([(10, corner_store(0, occl=0.9, sigma=4.0)), (20, lone)])
    table, entry, template = atlas.best_query_from([[2.5, 3.25]], 1, [2, 20])
    assert entry.tolist() == [[0, 1]] and template.tolist() == [[10, 20]] and table[0, :, 3].tolist() == [4.0, 0.125]
    old = atlas.tracks_from([[2.5, 3.25]], 1, [2])
    assert old[3].tolist() == [20] and np.isnan(old[0]).all()                            # (the per-point rule follows `lone` into the fill)


# ---- 6. what is not found, empty calls, errors ---------------------------------------------------------------------------------
def test_points_that_are_not_found_empty_calls_and_documented_errors():
    from mft_amd import TrackAtlas
    H, W = 13, 21
    atlas = three_templates(H, W)
    lost = np.array([[W + 4.0, 3.0], [-3.0, -3.0], [5.0, H + 9.0], [np.nan, 2.0], [3.0, np.nan], [np.nan, np.nan]], np.float32)
    for src in SOURCES:
        assert_fill_rows(*(t.numpy() for t in atlas.best_query_from(lost, src)), np.ones((6, 4), bool))
    c, o, found, template = atlas.best_tracks_from(lost, [1, 2, 3, 3, 2, 1])
    assert np.isnan(c).all() and (o == 1).all() and not found.any() and (template == -1).all()
    st = make_store(H, W, {0: const_planes(H, W), 7: shifted_out_planes(H, W), 2: field(1, H, W, 1.5)})
    table, entry, template = TrackAtlas([(0, st)]).best_query_from(off_grid_points(H, W, 9), 7)      # nothing maps into frame 7
    assert table.shape == (9, 3, 4)
    assert_fill_rows(table.numpy(), entry.numpy(), template.numpy(), np.ones((9, 3), bool))
    # a column nobody covers, next to one that is answered
    u = [t.numpy() for t in atlas.best_query_from(off_grid_points(H, W, 9), 2, [7, 1])]
    assert_fill_rows(u[0][:, 0:1], u[1][:, 0:1], u[2][:, 0:1], np.ones((9, 1), bool))
    assert (u[1][:, 1] >= 0).any()
    # empty calls
    for pts, cols, shape in ((np.zeros((0, 2), np.float32), None, (0, 4)), (off_grid_points(H, W, 5), [], (5, 0)),
                             (np.zeros((0, 2), np.float32), [], (0, 0))):
        table, entry, template = atlas.best_query_from(pts, 2, cols)
        assert table.shape == shape + (4,) and entry.shape == shape and template.shape == shape
        assert table.dtype == torch.float32 and entry.dtype == torch.int32 and template.dtype == torch.int32
        c, o, found, template = atlas.best_tracks_from(pts, 2, cols)
        assert c.shape == shape + (2,) and o.shape == shape and found.shape == shape and template.shape == shape
    assert atlas.best_query_from(np.zeros((0, 2), np.float32), [])[0].shape == (0, 4, 4)
    # out
    pts = off_grid_points(H, W, 7)
    want = atlas.best_query_from(pts, 2, [1, 0])
    big = (torch.full((9, 2, 4), -7.0), torch.full((9, 2), -7, dtype=torch.int32))
    out = tuple(b[1:8] for b in big)
    got = atlas.best_query_from(pts, 2, [1, 0], out=out)
    assert got[0] is out[0] and got[1] is out[1]
    same_rows(got[0].numpy(), want[0].numpy())
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert all((b[0] == -7).all() and (b[8] == -7).all() for b in big)
    # the threshold is the locates' and the key's
    low = atlas.best_query_from(pts, 2, [1, 0], occlusion_threshold=0.05)
    assert_same_points(low, brute_force(atlas, pts, [2] * 7, [1, 0], 0.05))
    # errors, all before any work
    for call in (lambda: atlas.best_query_from(pts, 7), lambda: atlas.best_tracks_from(pts, 7, [1]),
                 lambda: atlas.best_query_from(pts, [1, 2, 3, 7, 1, 2, 3])):
        with pytest.raises(KeyError):
            call()
    ok = lambda: [torch.zeros(7, 2, 4), torch.zeros(7, 2, dtype=torch.int32)]  # noqa: E731
    bad = []
    for i, t in ((0, torch.zeros(7, 2, 3)), (0, torch.zeros(7, 2, 4, dtype=torch.float64)), (1, torch.zeros(7, 2)),
                 (1, torch.zeros(7, 3, dtype=torch.int32)), (0, torch.zeros(7, 2, 8)[..., ::2]), (1, np.zeros((7, 2), np.int32)),
                 (0, torch.zeros(6, 2, 4))):
        o = ok()
        o[i] = t
        bad.append(o)
    bad.append(ok()[:1])
    for o in bad:
        with pytest.raises(ValueError):
            atlas.best_query_from(pts, 2, [1, 0], out=o)
    with pytest.raises(KeyError):
        atlas.best_query_from(pts, 7, [1, 0], out=bad[0])                                # the KeyError comes first
    for call in (lambda: atlas.best_query_from(np.zeros((7, 3), np.float32), 2), lambda: atlas.best_query_from(np.zeros(7, np.float32), 2),
                 lambda: atlas.best_query_from(pts, [1, 2]), lambda: atlas.best_query_from(pts, [[2] * 7])):
        with pytest.raises(ValueError):
            call()
    # tracks_from is what it was
    old = atlas.tracks_from(pts, 2)
    assert np.isnan(old[0][:, 0:2]).all() and (old[1][:, 0:2] == 1).all() and old[2].shape == (7,)


# ---- 7. the inputs of the device comparison ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,amp", HOST_CASES)
def test_inputs_of_the_device_comparison_are_rarely_ambiguous(H, W, amp):
    _, pts, per_src = points_case(H, W, amp)
    amb = sum(int(per_src[s][1].sum()) for s in SOURCES)
    answered = sum(int(per_src[s][2].sum()) for s in SOURCES)
    total = sum(per_src[s][2].size for s in SOURCES)
    print(f"{H}x{W} amp {amp}: {amb} of {answered} answered point-columns are ambiguous ({amb / answered:.3%}); {answered / total:.1%} answered")
    assert answered > 0.9 * total and amb / answered <= AMBIGUOUS_CAP


# ---- 8. plumbing -------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_exported_and_checks_its_arguments():
    import ctypes
    import re
    from pathlib import Path
    from mft_amd import _lib, atlas_ops
    repo = Path(__file__).resolve().parents[1]
    name = "mftx_trackstore_tracks_from_best"
    assert re.search(r"\b%s\s*\(" % name, (repo / "include" / "mftx.h").read_text()) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, name) and lib.mftx_version() == 400
    variant = repo / "mft_amd" / "libmftx_lfwide.so"
    if variant.exists():
        assert hasattr(ctypes.CDLL(str(variant)), name)
    assert callable(atlas_ops.trackstore_tracks_from_best) and atlas_ops.TRACKSTORE_POINTS_COLUMNS == 16 and atlas_ops.TRACKSTORE_POINTS_TILE == 64
    fb = lib.mftx_trackstore_tracks_from_best
    buf = (ctypes.c_double * 8)()                                                     # host memory: only its address is looked at
    a = ctypes.addressof(buf)
    a16 = a if a % 16 == 0 else a + 8

    def call(located=a16, cells=a, tiles=a, groups=a, rank_of=a, row_of=a, order=a, frames=a, lohis=a, n_tiles=1, G=1, C=1, most=1, Q=1,
             N=1, R=1, T=1, H=8, W=8, cpb=0, table=a16, entry=a):
        return fb(located, cells, tiles, groups, rank_of, row_of, order, frames, lohis, n_tiles, G, C, most, Q, N, R, T, H, W, 0.5, cpb,
                  table, entry, None)

    err = lib.mftx_last_error_string
    assert call(T=0) == 0 and call(N=0) == 0 and call(T=0, located=None, table=None) == 0       # no points, no columns: a no-op
    assert call(T=-1) == -1 and b"trackstore_tracks_from_best" in err()
    for arg in ("N", "n_tiles", "G", "C", "Q", "most"):
        assert call(**{arg: -1}) == -1, arg
    assert call(most=257, C=300) == -1 and b"256" in err()
    assert call(H=1) == -1 and call(W=1) == -1 and call(cpb=-1) == -1 and call(R=0) == -1 and call(Q=0) == -1
    assert call(n_tiles=0) == -1 and call(G=0) == -1 and call(G=2) == -1 and call(n_tiles=2) == -1 and call(most=2) == -1
    for arg in ("located", "cells", "tiles", "groups", "rank_of", "row_of", "order", "frames", "lohis", "table", "entry"):
        assert call(**{arg: None}) == -1 and err().endswith(b"null pointer: " + arg.encode()), arg
    for arg in ("tiles", "groups", "order", "table", "entry"):                        # without candidates only these are needed
        assert call(C=0, most=0, Q=0, located=None, cells=None, rank_of=None, row_of=None, frames=None, lohis=None, **{arg: None}) == -1, arg
    assert call(H=65536, W=32768) == -1 and b"2^31" in err()
    assert call(T=65536 * 2, cpb=1) == -1 and b"column blocks" in err()
    assert call(located=a16 + 8) == -2 and b"located must be 16-byte aligned" in err()
    assert call(table=a16 + 8) == -2 and b"table must be 16-byte aligned" in err()
    assert call(frames=a + 4) == -2 and b"frames" in err() and call(lohis=a + 4) == -2
    for arg in ("cells", "tiles", "groups", "rank_of", "row_of", "order", "entry"):
        assert call(**{arg: a + 2}) == -2 and (arg.encode() + b" must be 4-byte aligned") in err(), arg


def test_the_host_tables_of_the_launch():
    from mft_amd import atlas_ops
    tiles, groups, Q, C = atlas_ops.points_tables([1, 129, 64], [2, 0, 3])
    assert tiles.tolist() == [[0, 0], [1, 0], [1, 64], [1, 128], [2, 0]]
    assert groups.tolist() == [[0, 1, 0, 0, 2], [2, 129, 1, 2, 2], [2, 64, 130, 2, 5]] and (Q, C) == (2 + 192, 5)
    with pytest.raises(atlas_ops.MftxError):
        atlas_ops.points_tables([0], [1])
