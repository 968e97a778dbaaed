"""``MultiTemplateMFT`` with ``C.multi_template_stores`` and ``TrackAtlas`` (mft_amd/trackatlas.py) on the host: the pass keeps, per
template, the store a single ``MFT`` with ``C.track_store`` keeps; the atlas answers from whichever store sees a query best.
No GPU needed: the host doubles of tests/test_trackstore.py restated, the CPU stores of tests/test_track_locate.py.

The builders of this file (``atlas_case``, ``two_template_stores``) are shared with tests/test_gpu_track_atlas.py, which holds
the device paths to this restatement bit for bit."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import mft_oracle as O
from test_track_inverse import bits, grid
from test_track_locate import const_planes, field, make_store

DELTAS = (np.inf, 1, 2, 4)
PH, PW = 24, 40                  # the pass's frames
N_FRAMES = 9


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ---- the host doubles --------------------------------------------------------------------------------------------------------
class OracleBackend:
    """No chain_select_multi: the pass chains per template and appends per template through the store's CPU path."""

    @staticmethod
    def chain_select(Ls, Rs, thr):
        from mft_amd.MFT import is_packed, unpack_planes
        Rs = [unpack_planes(r) if is_packed(r) else r for r in Rs]
        f, o, s, idx = O.select([O.chain(l, r) for l, r in zip(Ls, Rs)], thr)
        return f, o, s, idx.to(torch.int8)


class StubFlower:
    def compute_flow(self, src_img, dst_img, mode="flow", init_flow=None, **kw):
        flow, occl, sigma = gi.stub_flowou(gi.decode_id(src_img), gi.decode_id(dst_img), PH, PW)
        return T(flow), {"occlusion": T(occl), "sigma": T(sigma), "debug": None}


def make_config(**extra):
    from mft_amd.config import Config
    c = Config()
    c.deltas = list(DELTAS)
    c.occlusion_threshold = 0.02
    c.flow_config = Config()
    flower = StubFlower()
    c.flow_config.of_class = lambda cfg: flower
    c.keep_result_on_device = True
    for k, v in extra.items():
        setattr(c, k, v)
    return c


def frames_of(first, direction):
    return range(first, N_FRAMES) if direction > 0 else range(first, -1, -1)


def single_store(start, direction, **extra):
    from mft_amd.MFT import MFT
    tr = MFT(make_config(track_store=True, **extra), backend=OracleBackend(), device="cpu")
    for k, f in enumerate(frames_of(start, direction)):
        tr.init(gi.id_image(f, PH, PW), start_frame_i=start, time_direction=direction) if k == 0 else tr.track(gi.id_image(f, PH, PW))
    return tr.track_store


def run_pass(starts, direction, **extra):
    """-> (the pass, {frame: {start: (planes, last_pairs, last_chosen)}})."""
    from mft_amd.multi import MultiTemplateMFT
    mt = MultiTemplateMFT(make_config(**extra), backend=OracleBackend(), device="cpu")
    mt.init(starts, time_direction=direction)
    first = min(starts) if direction > 0 else max(starts)
    out = {}
    for f in frames_of(first, direction):
        metas = mt.track(f, gi.id_image(f, PH, PW))
        out[f] = {s: (tuple(p.clone() for p in m.result.planes()), list(mt.templates[s].last_pairs),
                      None if mt.templates[s].last_chosen is None else mt.templates[s].last_chosen.clone()) for s, m in metas.items()}
    return mt, out


def same_store(a, b):
    assert a.frame_ids == b.frame_ids and (a.H, a.W, a.frames_per_chunk) == (b.H, b.W, b.frames_per_chunk)
    for slot in range(len(a)):
        assert torch.equal(a.packed(slot).cpu().view(torch.int16), b.packed(slot).cpu().view(torch.int16)), (a.frame_ids[0], slot)
        assert torch.equal(a.lohi(slot).cpu().view(torch.int32), b.lohi(slot).cpu().view(torch.int32)), (a.frame_ids[0], slot)


# ---- 1. the pass keeps the single trackers' stores ---------------------------------------------------------------------------
@pytest.mark.parametrize("starts,direction", [((0, 3, 5), +1), ((8, 4), -1)])
def test_pass_with_stores_keeps_each_templates_single_tracker_store(starts, direction):
    from mft_amd.trackstore import DenseTrackStore
    plain, want = run_pass(starts, direction)
    assert plain.track_stores == {} and plain.stats["store_append_calls"] == 0
    mt, got = run_pass(starts, direction, multi_template_stores=True, track_store_frames_per_chunk=4)
    assert sorted(mt.track_stores) == sorted(starts)
    for s in starts:
        st = mt.track_stores[s]
        assert isinstance(st, DenseTrackStore) and st.frame_ids == list(frames_of(s, direction)) and st.frames_per_chunk == 4
        same_store(st, single_store(s, direction, track_store_frames_per_chunk=4))
    assert sorted(got) == sorted(want)
    for f in want:                                                                   # nothing else changes
        assert sorted(got[f]) == sorted(want[f])
        for s in want[f]:
            assert all(torch.equal(a, b) for a, b in zip(got[f][s][0], want[f][s][0])), (s, f)
            assert got[f][s][1] == want[f][s][1]
            assert (got[f][s][2] is None and want[f][s][2] is None) or torch.equal(got[f][s][2], want[f][s][2])
    # the host doubles append per template: one store call per (template, frame)
    assert mt.stats["store_append_calls"] == sum(len(mt.track_stores[s]) for s in starts)


def test_track_store_stays_refused_and_the_cap_bounds_the_sum():
    from mft_amd.multi import MultiTemplateMFT
    multi = MultiTemplateMFT(make_config(track_store=True, multi_template_stores=True), backend=OracleBackend(), device="cpu")
    with pytest.raises(ValueError, match="track_store"):
        multi.init([0])
    chunk = 2 * (PH * PW * 8 + 32)
    mt = MultiTemplateMFT(make_config(multi_template_stores=True, track_store_frames_per_chunk=2, track_store_max_bytes=2 * chunk),
                          backend=OracleBackend(), device="cpu")
    mt.init([0, 1])
    mt.track(0, gi.id_image(0, PH, PW))                  # store 0 opens a chunk
    mt.track(1, gi.id_image(1, PH, PW))                  # store 1 opens one: the sum is at the cap
    assert sum(st.nbytes for st in mt.track_stores.values()) == 2 * chunk
    before = {s: (list(st.frame_ids), st.nbytes, st.packed(0).clone()) for s, st in mt.track_stores.items()}
    with pytest.raises(MemoryError):
        mt.track(2, gi.id_image(2, PH, PW))              # store 0 would open its second chunk, store 1 has room: nothing is appended
    assert sorted(mt.track_stores) == [0, 1] and mt.current_frame_i == 1
    for s, st in mt.track_stores.items():
        assert st.frame_ids == before[s][0] and st.nbytes == before[s][1] and torch.equal(st.packed(0), before[s][2])
    assert mt.templates[0].current_frame_i == 1 and sorted(mt.templates[1].memory) == [1]
    # a cap that a NEW template's first chunk would exceed: that template gets no store either
    mt = MultiTemplateMFT(make_config(multi_template_stores=True, track_store_frames_per_chunk=2, track_store_max_bytes=chunk),
                          backend=OracleBackend(), device="cpu")
    mt.init([0, 1])
    mt.track(0, gi.id_image(0, PH, PW))
    with pytest.raises(MemoryError):
        mt.track(1, gi.id_image(1, PH, PW))
    assert sorted(mt.track_stores) == [0] and len(mt.track_stores[0]) == 1


def test_a_failed_append_leaves_nothing_of_the_frame_behind():
    from mft_amd.multi import MultiTemplateMFT
    mt = MultiTemplateMFT(make_config(multi_template_stores=True), backend=OracleBackend(), device="cpu")
    mt.init([0, 1])
    mt.track(0, gi.id_image(0, PH, PW))
    mt.track(1, gi.id_image(1, PH, PW))

    def broken(planes, frame_i=None):
        raise RuntimeError("no")

    mt.track_stores[1].append = broken                   # the second store fails after the first has taken frame 2
    with pytest.raises(RuntimeError):
        mt.track(2, gi.id_image(2, PH, PW))
    assert mt.track_stores[0].frame_ids == [0, 1] and mt.track_stores[1].frame_ids == [1] and mt.current_frame_i == 1
    del mt.track_stores[1].append
    mt.track(2, gi.id_image(2, PH, PW))                  # ... and the frame can be taken again
    assert mt.track_stores[0].frame_ids == [0, 1, 2] and mt.track_stores[1].frame_ids == [1, 2]
    same_store(mt.track_stores[0], _first_frames(single_store(0, +1), 3))
    st = mt.track_stores[0]
    with pytest.raises(ValueError):
        st.unreserve(1)                                  # only the last slot can be given back
    st.unreserve(2)
    assert st.frame_ids == [0, 1] and 2 not in st._slot_of


def _first_frames(st, n):
    """The store cut back to its first n frames (a view for comparisons)."""
    for f in list(st.frame_ids[n:])[::-1]:
        st.unreserve(f)
    return st


def test_reserve_hands_out_the_next_slots_views():
    st = make_store(6, 8, {4: const_planes(6, 8)}, frames_per_chunk=2)
    slot, packed, lohi = st.reserve(9)
    assert slot == 1 and st.frame_ids == [4, 9] and st.slot_of(9) == 1 and st.next_needs_chunk
    assert packed.shape == (6, 8, 4) and packed.dtype == torch.uint16 and lohi.shape == (4, 2)
    assert packed.data_ptr() == st.packed(1).data_ptr() and lohi.data_ptr() == st.lohi(1).data_ptr()
    with pytest.raises(ValueError):
        st.reserve(9)
    assert st.reserve()[0] == 2 and len(st._chunks) == 2                              # (default id: the number stored so far was 2)
    capped = make_store(6, 8, {0: const_planes(6, 8)}, frames_per_chunk=1, max_bytes=6 * 8 * 8 + 32)
    with pytest.raises(MemoryError):
        capped.reserve(1)
    assert capped.frame_ids == [0]


# ---- 2. coverage on exact inputs ---------------------------------------------------------------------------------------------
CH, CW = 6, 8


def coverage_stores(device="cpu"):
    """a: template 0, frame 1 shifted by (+3, 0) at sigma 0.5; b: template 1 (identity on frame 1); c: template 0, frame 1
    shifted by (+1, 0) at sigma 0.25.  Every value is kept exactly by the quantisation (flat channels)."""
    a = make_store(CH, CW, {0: const_planes(CH, CW), 1: const_planes(CH, CW, fx=3.0, sigma=0.5)}, device=device)
    b = make_store(CH, CW, {1: const_planes(CH, CW)}, device=device)
    c = make_store(CH, CW, {0: const_planes(CH, CW), 1: const_planes(CH, CW, fx=1.0, sigma=0.25)}, device=device)
    return a, b, c


def test_coverage_on_exact_inputs():
    from mft_amd import TrackAtlas
    a, b, c = coverage_stores()
    g = grid(CH, CW)
    x = g[:, 0]
    ta, ca = a.locate(g, 1)
    assert np.array_equal(ca.numpy() >= 0, x >= 3)                                    # a alone: exactly the pixels x >= 3
    f = x >= 3
    assert np.array_equal(ta.numpy()[f, 0], x[f] - 3) and np.array_equal(ta.numpy()[f, 1], g[f, 1]) and (ta.numpy()[f, 3] == 0.5).all()
    atlas = TrackAtlas([(0, a), (1, b)])
    assert atlas.frames == [0, 1] and [t for t, _ in atlas.entries] == [0, 1] and atlas.entries[1][1] is b
    t, cl, e = atlas.locate(g, 1)
    assert t.shape == (48, 4) and cl.dtype == torch.int32 and e.dtype == torch.int32
    assert (cl.numpy() >= 0).all() and (e.numpy() == 1).all()                        # all 48, every one won by b: sigma 0 on its own frame
    assert np.array_equal(t.numpy()[:, 0:2], g) and not t.numpy()[:, 2:4].any()
    tb, cb = b.locate(g, 1)
    assert np.array_equal(bits(t), bits(tb)) and torch.equal(cl, cb)
    # c in place of b: x = 1, 2 go to it, and x >= 3 too because 0.25 < 0.5; x = 0 is not found
    atlas = TrackAtlas([(0, a), (0, c)])
    t, cl, e = atlas.locate(g, 1)
    assert np.array_equal(e.numpy(), np.where(x >= 1, 1, -1)) and np.array_equal(cl.numpy() >= 0, x >= 1)
    assert np.array_equal(t.numpy()[x >= 1, 0], x[x >= 1] - 1) and (t.numpy()[x >= 1, 3] == 0.25).all()
    assert np.isnan(t.numpy()[x == 0]).all() and (cl.numpy()[x == 0] == -1).all()
    # on frame 0 both are the identity at sigma 0: the lower rank
    assert (atlas.locate(g, 0)[2].numpy() == 0).all()


# ---- 3. the order ------------------------------------------------------------------------------------------------------------
def flat_store(occl=0.0, sigma=0.0, device="cpu"):
    """Template 0; frame 1 has zero flow and constant occlusion and sigma (kept exactly: flat channels)."""
    return make_store(CH, CW, {0: const_planes(CH, CW), 1: const_planes(CH, CW, occl=occl, sigma=sigma)}, device=device)


def with_sigma_range(st, lo, hi=None):
    """The stored frame 1's sigma channel set to the constant ``lo`` through its (min, max) table (the words are 0): a way to
    hold values no quantisation would keep, NaN among them."""
    st.lohi(st.slot_of(1))[3] = torch.tensor([lo, lo if hi is None else hi])
    return st


def winners(stores, thr=0.5, f=1):
    from mft_amd import TrackAtlas
    t, c, e = TrackAtlas([(0, st) for st in stores]).locate(grid(CH, CW), f, occlusion_threshold=thr)
    assert (c.numpy() >= 0).all()
    e = np.unique(e.numpy())
    assert e.size == 1
    return int(e[0]), t


def test_order_visible_then_sigma_then_rank():
    occluded, visible = flat_store(occl=0.9, sigma=0.1), flat_store(occl=0.0, sigma=5.0)
    assert winners([occluded, visible])[0] == 1                                       # visible beats occluded whatever the sigma
    w, t = winners([occluded, visible], thr=1.0)                                      # ... and with neither occluded the lower sigma
    assert w == 0 and (t.numpy()[:, 2] == np.float32(0.9)).all() and (t.numpy()[:, 3] == np.float32(0.1)).all()
    assert winners([flat_store(sigma=0.5), flat_store(sigma=0.25), flat_store(sigma=0.375)])[0] == 1
    assert winners([flat_store(sigma=0.25), flat_store(sigma=0.25)])[0] == 0          # equal sigma bits: the lower rank
    nan, zero, small = with_sigma_range(flat_store(), float("nan")), flat_store(sigma=0.0), flat_store(sigma=2.0 ** -20)
    negative = with_sigma_range(flat_store(), -1.0)
    w, t = winners([small, nan])
    assert w == 1 and np.isnan(t.numpy()[:, 3]).all()                                 # a NaN sigma counts as +0: below any positive one
    assert winners([zero, nan])[0] == 0 and winners([nan, zero])[0] == 0              # ... and ties with a zero: the lower rank
    assert winners([small, negative])[0] == 1 and winners([zero, negative])[0] == 0
    from mft_amd import TrackAtlas
    twins = [make_store(CH, CW, {0: const_planes(CH, CW), 1: field(3, CH, CW, 0.5)}) for _ in range(2)]
    t, c, e = TrackAtlas([(0, st) for st in twins]).locate(grid(CH, CW), 1)            # identical stores: rank 0 wherever anything is found
    wt, wc = twins[0].locate(grid(CH, CW), 1)
    assert np.array_equal(e.numpy(), np.where(wc.numpy() >= 0, 0, -1)) and (wc.numpy() >= 0).sum() > 24
    assert np.array_equal(bits(t), bits(wt)) and torch.equal(c, wc)


# ---- 4. the calls ------------------------------------------------------------------------------------------------------------
AH, AW = 13, 21


def two_template_stores(H=AH, W=AW, device="cpu", amp=1.5):
    """Template 0 over frames 0, 1, 2 and template 1 over frames 1, 2: smooth seeded fields (amp 1.5: few pixels lost; 5: folds)."""
    s0 = make_store(H, W, {0: const_planes(H, W), 1: field(11, H, W, amp), 2: field(12, H, W, amp)}, device=device)
    s1 = make_store(H, W, {1: const_planes(H, W), 2: field(13, H, W, amp)}, device=device)
    return s0, s1


def test_inverse_is_locate_on_the_pixel_grid():
    from mft_amd import TrackAtlas
    atlas = TrackAtlas(list(enumerate(two_template_stores(amp=5.0))))
    g = grid(AH, AW)
    for f in (0, 1, 2):
        t, c, e = atlas.inverse(f)
        assert t.shape == (AH, AW, 4) and c.shape == (AH, AW) and e.shape == (AH, AW) and e.dtype == torch.int32
        wt, wc, we = atlas.locate(g, f)
        assert np.array_equal(bits(t).reshape(-1, 4), bits(wt)) and torch.equal(c.reshape(-1), wc) and torch.equal(e.reshape(-1), we)
    t, c, e = atlas.inverse([2, 0, 2])
    assert t.shape == (3, AH, AW, 4) and c.shape == (3, AH, AW) and e.shape == (3, AH, AW)
    for k, f in enumerate((2, 0, 2)):
        wt, wc, we = atlas.inverse(f)
        assert np.array_equal(bits(t[k]), bits(wt)) and torch.equal(c[k], wc) and torch.equal(e[k], we)
    e2 = atlas.inverse(2)[2].numpy()
    print(f"frame 2: template 0 wins {int((e2 == 0).sum())}, template 1 {int((e2 == 1).sum())}, {int((e2 < 0).sum())} not found")
    assert (e2 == 0).any() and (e2 == 1).any()                                        # both templates win somewhere
    assert (atlas.inverse(0)[2] == 0).all()                                           # only template 0 holds frame 0
    # per-point frames in one call
    ids = [(n * 7 + n // 5) % 3 for n in range(len(g))]
    t, c, e = atlas.locate(g, ids)
    for f in (0, 1, 2):
        sel = np.flatnonzero(np.asarray(ids) == f)
        wt, wc, we = atlas.locate(g[sel], f)
        assert np.array_equal(bits(t)[sel], bits(wt)) and torch.equal(c[sel], wc) and torch.equal(e[sel], we)
    assert atlas.inverse([])[0].shape == (0, AH, AW, 4)


def joined_atlas():
    """Template 5 forward (5, 6, 7) and backward (5, 4, 3), and template 9 on its own frame."""
    from mft_amd import TrackAtlas
    H, W = AH, AW
    fwd = make_store(H, W, {5: const_planes(H, W), 6: field(21, H, W, 1.5), 7: field(22, H, W, 1.5)})
    bwd = make_store(H, W, {5: const_planes(H, W), 4: field(23, H, W, 1.5), 3: field(24, H, W, 1.5)})
    nine = make_store(H, W, {9: const_planes(H, W)})
    return TrackAtlas([(9, nine), (5, fwd), (5, bwd)]), fwd, bwd, nine


def test_query_joins_the_forward_and_backward_store_of_a_template():
    atlas, fwd, bwd, nine = joined_atlas()
    assert [t for t, _ in atlas.entries] == [5, 5, 9] and atlas.entries[0][1] is fwd and atlas.entries[1][1] is bwd
    assert atlas.frames == [3, 4, 5, 6, 7, 9]
    P = np.array([[2.5, 3.25], [10.0, 6.0], [19.75, 11.5]], np.float32)
    q = atlas.query(5, P)
    assert q.shape == (3, 6, 4) and q.dtype == torch.float32
    for k, (f, st) in enumerate([(3, bwd), (4, bwd), (5, fwd), (6, fwd), (7, fwd)]):
        assert np.array_equal(bits(q[:, k]), bits(st.query(P, [f])[:, 0])), f
    assert np.isnan(q[:, 5].numpy()).all()                                            # frame 9: neither store of template 5 holds it
    assert np.array_equal(bits(atlas.query(5, P, [7, 3])), bits(torch.stack([fwd.query(P, [7])[:, 0], bwd.query(P, [3])[:, 0]], dim=1)))
    assert np.array_equal(bits(atlas.query(5, P, [6, 5])), bits(fwd.query(P, [6, 5])))
    assert np.isnan(atlas.query(9, P, [5]).numpy()).all() and np.array_equal(atlas.query(9, P, [9])[:, 0, 0:2].numpy(), P)
    with pytest.raises(KeyError):
        atlas.query(6, P)


def test_tracks_from_returns_the_winners_template():
    from mft_amd import TrackAtlas
    s0, s1 = two_template_stores()
    atlas = TrackAtlas([(0, s0), (1, s1)])
    g = grid(AH, AW)
    pts = np.concatenate([g[::7], [[-5.0, -5.0]]]).astype(np.float32)
    coords, occl, found, template = atlas.tracks_from(pts, 1)
    T_ = len(atlas.frames)
    assert coords.shape == (len(pts), T_, 2) and occl.shape == (len(pts), T_) and found.dtype == bool and template.shape == (len(pts),)
    table, cell, entry = atlas.locate(pts, 1)
    assert np.array_equal(found, entry.numpy() >= 0) and not found[-1] and found[:-1].all()
    assert np.array_equal(template, np.where(found, np.asarray([0, 1])[entry.numpy().clip(0)], -1))
    assert (template[:-1] == 1).all()                                                 # on its own frame template 1 is the identity at sigma 0
    assert np.isnan(coords[-1]).all() and (occl[-1] == 1).all()
    want = s1.query(table[found][:, 0:2]).numpy()                                     # template 1 holds frames 1, 2; frame 0 is not covered
    assert np.isnan(coords[found, 0]).all() and (occl[found, 0] == 1).all()
    assert np.array_equal(coords[found, 1:], want[:, :, 0:2]) and np.array_equal(occl[found, 1:], want[:, :, 2])
    assert np.abs(coords[found, 1] - pts[found]).max() <= 2.0 ** -9                  # a point stays where it was given
    # on frame 2 both templates win somewhere, and each point follows its own
    coords, occl, found, template = atlas.tracks_from(g, 2, frames=[2, 0])
    assert set(np.unique(template)) >= {0, 1}
    assert np.isnan(coords[template == 1, 1]).all() and np.isfinite(coords[template == 0, 1]).all()
    assert np.abs(coords[found, 0] - g[found]).max() <= 2.0 ** -9


def test_documented_errors():
    from mft_amd import TrackAtlas
    from mft_amd.trackatlas import MAX_ENTRIES
    s0, s1 = two_template_stores()
    atlas = TrackAtlas([(0, s0), (1, s1)])
    small = make_store(6, 8, {0: const_planes(6, 8)})
    with pytest.raises(ValueError):
        TrackAtlas([(0, s0), (0, small)])                                             # mixed sizes
    with pytest.raises(ValueError):
        TrackAtlas([(1, s0)])                                                         # the first frame is not the template
    with pytest.raises(ValueError):
        TrackAtlas([(0, make_store(6, 8, {}))])
    with pytest.raises(ValueError):
        TrackAtlas([])
    with pytest.raises(ValueError):
        TrackAtlas([(0, small)] * (MAX_ENTRIES + 1))
    assert len(TrackAtlas([(0, small)] * MAX_ENTRIES).entries) == MAX_ENTRIES
    P = np.zeros((2, 2), np.float32)
    for call in (lambda: atlas.locate(P, 7), lambda: atlas.locate(P, [0, 7]), lambda: atlas.inverse(7), lambda: atlas.inverse([1, 7]),
                 lambda: atlas.tracks_from(P, 7), lambda: atlas.query(7, P)):
        with pytest.raises(KeyError):
            call()
    with pytest.raises(ValueError):
        atlas.locate(P, [0, 1, 2])
    with pytest.raises(ValueError):
        atlas.locate(np.zeros((2, 3), np.float32), 0)
    with pytest.raises(ValueError):
        atlas.inverse([[0, 1]])
    t, c, e = atlas.locate(np.zeros((0, 2), np.float32), 1)
    assert t.shape == (0, 4) and c.shape == (0,) and e.shape == (0,)


def test_from_passes_ranks_forward_before_backward():
    from mft_amd import TrackAtlas
    fwd, _ = run_pass((3, 5), +1, multi_template_stores=True)
    bwd, _ = run_pass((5, 8), -1, multi_template_stores=True)
    atlas = TrackAtlas.from_passes(fwd, bwd)
    assert [t for t, _ in atlas.entries] == [3, 5, 5, 8] and atlas.frames == list(range(N_FRAMES))
    assert atlas.entries[1][1] is fwd.track_stores[5] and atlas.entries[2][1] is bwd.track_stores[5]
    P = np.array([[4.0, 5.0], [30.5, 17.25]], np.float32)
    q = atlas.query(5, P)
    assert q.shape == (2, N_FRAMES, 4) and np.isfinite(q.numpy()).all()               # template 5 covers the whole video
    assert np.array_equal(bits(q[:, 2]), bits(bwd.track_stores[5].query(P, [2])[:, 0]))
    assert np.array_equal(bits(q[:, 7]), bits(fwd.track_stores[5].query(P, [7])[:, 0]))
    t, c, e = atlas.locate(P, 8)
    assert (e.numpy() == 3).all()                                                     # template 8 on its own frame


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------------
NEW = ("mftx_trackstore_append_multi_workspace_bytes", "mftx_trackstore_append_multi", "mftx_trackstore_invert_atlas")


def test_entry_points_are_declared_bound_exported_and_check_their_arguments():
    import ctypes
    import re
    from pathlib import Path
    import mft_amd
    from mft_amd import _lib, ops
    repo = Path(__file__).resolve().parents[1]
    header = (repo / "include" / "mftx.h").read_text()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        variant = repo / "mft_amd" / "libmftx_lfwide.so"
        if variant.exists():
            assert hasattr(ctypes.CDLL(str(variant)), name), name
    assert lib.mftx_version() == 400
    assert callable(ops.trackstore_append_multi) and callable(ops.trackstore_invert_atlas) and callable(ops.trackstore_locate_frames)
    assert mft_amd.TrackAtlas.__name__ == "TrackAtlas"
    one = lib.mftx_trackstore_workspace_bytes()
    assert lib.mftx_trackstore_append_multi_workspace_bytes(0) == 0 and lib.mftx_trackstore_append_multi_workspace_bytes(5) == 5 * one
    # argument checks that come before anything is launched
    am = lib.mftx_trackstore_append_multi
    assert am(0, None, None, None, 8, 8, None, None, None, 0, None) == 0                # T == 0: a no-op
    assert am(2, None, None, None, 8, 8, None, None, None, 0, None) == -1 and b"trackstore_append_multi" in lib.mftx_last_error_string()
    assert am(-1, None, None, None, 8, 8, None, None, None, 0, None) == -1 and am(0, None, None, None, 1, 8, None, None, None, 0, None) == -1
    ia = lib.mftx_trackstore_invert_atlas
    assert ia(None, None, None, None, 0, 0, 8, 8, 0.5, None, None, None, None, None) == 0      # no planes: a no-op
    assert ia(None, None, None, None, 1, 1, 8, 8, 0.5, None, None, None, None, None) == -1 and b"trackstore_invert_atlas" in lib.mftx_last_error_string()
    assert ia(None, None, None, None, 1, 257, 8, 8, 0.5, None, None, None, None, None) == -1 and b"256" in lib.mftx_last_error_string()
    assert ia(None, None, None, None, 0, 0, 4098, 4098, 0.5, None, None, None, None, None) == -1 and b"2^24" in lib.mftx_last_error_string()
    assert ia(None, None, None, None, 0, 0, 4097, 4097, 0.5, None, None, None, None, None) == 0  # exactly 2^24 cells
    assert ia(None, None, None, None, -1, 0, 8, 8, 0.5, None, None, None, None, None) == -1
    assert ia(None, None, None, None, 0, 0, 1, 8, 0.5, None, None, None, None, None) == -1
