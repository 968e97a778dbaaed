"""``TrackAtlas.results_from`` / ``result_from`` / ``covered`` on the host (device="cpu"): the dense results from any video frame,
every pixel followed on the template that sees it best -- ``inverse``, then ``query`` on the winner's template, chained by the rule
of ``DenseTrackStore.results_from``.  No GPU needed; the stores are those of tests/test_track_locate.py, tests/test_track_inverse.py
and tests/test_track_atlas.py.

``composed_by_hand`` is shared with tests/test_gpu_track_atlas_flow.py."""
import numpy as np
import pytest
import torch

from mft_amd.results import FlowOUTrackingResult
from test_track_atlas import AH, AW, CH, CW, coverage_stores, joined_atlas, two_template_stores
from test_track_inverse import bits, grid
from test_track_locate import const_planes, make_store, smooth_frames

NAN_BITS = 0x7fc00000
INF_BITS = 0x7f800000
ONE_BITS = 0x3f800000


def assert_fill(flow, occl, sigma, where):
    """``where``: a bool mask [H, W] (or [T, H, W] with the planes' leading axis) of the pixels that carry the fill."""
    assert (bits(flow)[..., 0, :, :][where] == NAN_BITS).all() and (bits(flow)[..., 1, :, :][where] == NAN_BITS).all()
    assert (bits(occl)[..., 0, :, :][where] == ONE_BITS).all() and (bits(sigma)[..., 0, :, :][where] == INF_BITS).all()


def composed_by_hand(atlas, src, cols, stores_of, thr=0.5):
    """The definition, pixel group by pixel group, in numpy float32: ``atlas.inverse(src)``, then for the pixels of each winning
    template the columns of ``stores_of[template]`` -- a list of (frames held, store) in the order ``query`` prefers them -- read
    out by that store's own ``query`` -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W], found, template)."""
    H, W, T = atlas.H, atlas.W, len(cols)
    table, cell, entry = (t.cpu() for t in atlas.inverse(src, thr))
    tb, e = table.numpy().reshape(-1, 4), entry.numpy().reshape(-1)
    flow = np.full((H * W, T, 2), np.nan, np.float32)
    occl = np.ones((H * W, T), np.float32)
    sigma = np.full((H * W, T), np.inf, np.float32)
    template = np.where(e >= 0, np.asarray([f for f, _ in atlas.entries])[e.clip(0)], -1).astype(np.int32)
    g = grid(H, W)
    for s in np.unique(template[template >= 0]):
        rows = np.flatnonzero(template == s)
        for k, f in enumerate(cols):
            st = next((st for held, st in stores_of[int(s)] if f in held), None)
            if st is None:
                continue
            q = st.query(torch.from_numpy(tb[rows, 0:2]).to(st.device), [f]).cpu().numpy()[:, 0]
            with np.errstate(all="ignore"):
                flow[rows, k] = q[:, 0:2] - g[rows]
                occl[rows, k] = np.maximum(tb[rows, 2], q[:, 2])
                sigma[rows, k] = np.sqrt(tb[rows, 3] * tb[rows, 3] + q[:, 3] * q[:, 3])
    return (np.ascontiguousarray(flow.transpose(1, 2, 0)).reshape(T, 2, H, W), np.ascontiguousarray(occl.T).reshape(T, 1, H, W),
            np.ascontiguousarray(sigma.T).reshape(T, 1, H, W), (e >= 0).reshape(H, W), template.reshape(H, W))


def assert_same_results(got, want):
    """got: the five tensors of ``results_from``; want: five numpy arrays.  Bits where the expected value is no NaN, NaN-ness elsewhere."""
    for g, w in zip(got[:3], want[:3]):
        g = g.detach().cpu().numpy()
        assert g.shape == w.shape and g.dtype == np.float32
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan])
    assert got[3].dtype == torch.bool and np.array_equal(got[3].cpu().numpy(), want[3])
    assert got[4].dtype == torch.int32 and np.array_equal(got[4].cpu().numpy(), want[4])


# ---- 1. one entry ------------------------------------------------------------------------------------------------------------
def test_one_entry_is_the_stores_own_results_from():
    from mft_amd import TrackAtlas
    H, W = 37, 53
    frames = {0: const_planes(H, W)}
    frames.update(smooth_frames(H, W, 5.0))
    st = make_store(H, W, frames)
    atlas = TrackAtlas([(0, st)])
    assert atlas.frames == [0, 3, 5, 8] and st.frame_ids == [0, 3, 8, 5]
    for src, cols in ((3, None), (8, [5, 3]), (0, [8])):
        got = atlas.results_from(src, cols)
        want = st.results_from(src, atlas.frames if cols is None else cols)
        T = len(atlas.frames if cols is None else cols)
        assert got[0].shape == (T, 2, H, W) and got[1].shape == (T, 1, H, W) and got[2].shape == (T, 1, H, W)
        for g, w in zip(got[:3], want[:3]):
            assert g.dtype == torch.float32 and np.array_equal(bits(g), bits(w))
        assert got[3].dtype == torch.bool and torch.equal(got[3], want[3])
        assert got[4].shape == (H, W) and got[4].dtype == torch.int32
        assert torch.equal(got[4], torch.where(want[3], 0, -1).to(torch.int32))
        lost = ~want[3].numpy()
        assert_fill(got[0], got[1], got[2], np.broadcast_to(lost, (T, H, W)))
        if src == 3:
            assert lost.sum() > 100                                                  # both kinds of answer
        if src == 0:
            assert not lost.any()


# ---- 2. exact inputs ---------------------------------------------------------------------------------------------------------
def test_exact_inputs_written_out_by_hand():
    from mft_amd import TrackAtlas
    a, b, c = coverage_stores()
    x = np.broadcast_to(np.arange(CW), (CH, CW))
    # (0, a), (1, b): on frame 1 template 1 is the identity at sigma 0 and wins every pixel.  It does not cover frame 0.
    flow, occl, sigma, found, template = TrackAtlas([(0, a), (1, b)]).results_from(1, [0, 1])
    assert found.all() and (template == 1).all() and template.dtype == torch.int32
    assert_fill(flow[0], occl[0], sigma[0], np.ones((CH, CW), bool))
    assert not flow[1].numpy().any() and not occl[1].numpy().any() and not sigma[1].numpy().any()
    # (0, a), (0, c): c (shift +1, sigma 0.25) wins x >= 1, its template point being (x - 1, y); x = 0 is not found.  Template
    # 0's columns are read from its lowest-ranked entry that holds the frame, a: the identity on frame 0 -- flow (x - 1) - x = -1,
    # sigma sqrt(0.25^2 + 0) -- and a shift of +3 at sigma 0.5 on frame 1 -- flow (x - 1 + 3) - x = 2, sigma sqrt(0.0625 + 0.25).
    flow, occl, sigma, found, template = TrackAtlas([(0, a), (0, c)]).results_from(1, [0, 1])
    hit = x >= 1
    assert np.array_equal(found.numpy(), hit) and np.array_equal(template.numpy(), np.where(hit, 0, -1))
    assert_fill(flow, occl, sigma, np.broadcast_to(~hit, (2, CH, CW)))
    assert (flow[0, 0].numpy()[hit] == -1).all() and (flow[1, 0].numpy()[hit] == 2).all() and not flow[:, 1].numpy()[:, hit].any()
    assert not occl[:, 0].numpy()[:, hit].any()
    assert (sigma[0, 0].numpy()[hit] == np.float32(0.25)).all()
    assert (sigma[1, 0].numpy()[hit] == np.float32(np.sqrt(np.float64(0.3125)))).all()


# ---- 3. a joined template, uncovered columns ---------------------------------------------------------------------------------
def test_joined_template_and_uncovered_columns():
    atlas, fwd, bwd, nine = joined_atlas()
    assert atlas.frames == [3, 4, 5, 6, 7, 9]
    assert atlas.covered(5) == [True, True, True, True, True, False] and atlas.covered(9) == [False] * 5 + [True]
    assert atlas.covered(5, [9, 3, 9]) == [False, True, False] and atlas.covered(9, []) == []
    with pytest.raises(KeyError):
        atlas.covered(6)
    stores_of = {5: [((5, 6, 7), fwd), ((5, 4, 3), bwd)], 9: [((9,), nine)]}
    got = atlas.results_from(6)
    want = composed_by_hand(atlas, 6, atlas.frames, stores_of)
    assert_same_results(got, want)
    found = got[3].numpy()
    assert found.sum() > AH * AW // 2 and (got[4].numpy()[found] == 5).all()
    # frames 3 and 4 come from the backward store, 5, 6 and 7 from the forward one; 9 is not covered
    table = atlas.inverse(6)[0].reshape(-1, 4)
    at = torch.where(got[3].reshape(-1, 1), table[:, 0:2], torch.zeros(()))
    for k, (f, st) in enumerate([(3, bwd), (4, bwd), (5, fwd), (6, fwd), (7, fwd)]):
        q = st.query(at, [f])[:, 0].numpy().reshape(AH, AW, 4)
        assert np.array_equal(got[0][k, 0].numpy()[found], (q[..., 0] - grid(AH, AW)[:, 0].reshape(AH, AW))[found]), f
        assert np.isfinite(got[0][k].numpy()[:, found]).all() and np.isfinite(got[2][k].numpy()[:, found]).all()
    assert_fill(got[0][5], got[1][5], got[2][5], np.ones((AH, AW), bool))
    assert float(np.abs(got[0][3].numpy()[:, found]).max()) <= 2.0 ** -9                # from frame 6 to itself: nothing moves
    # frame 9: template 9 alone holds it, and covers nothing else
    flow, occl, sigma, found, template = atlas.results_from(9)
    assert found.all() and (template == 9).all()
    assert_fill(flow[:5], occl[:5], sigma[:5], np.ones((5, AH, AW), bool))
    assert not flow[5].numpy().any() and not occl[5].numpy().any() and not sigma[5].numpy().any()


# ---- 4. two templates winning different pixels -------------------------------------------------------------------------------
def test_each_pixel_follows_its_own_winner():
    from mft_amd import TrackAtlas
    s0, s1 = two_template_stores(amp=5.0)
    atlas = TrackAtlas([(0, s0), (1, s1)])
    stores_of = {0: [((0, 1, 2), s0)], 1: [((1, 2), s1)]}
    for cols in (None, [2, 0], [1]):
        got = atlas.results_from(2, cols)
        want = composed_by_hand(atlas, 2, atlas.frames if cols is None else cols, stores_of)
        assert_same_results(got, want)
    template = got[4].numpy()
    assert (template == 0).any() and (template == 1).any()                             # both templates win somewhere on frame 2
    flow, occl, sigma, found, template = atlas.results_from(2)
    one, zero = template.numpy() == 1, template.numpy() == 0
    assert_fill(flow[0], occl[0], sigma[0], one | ~found.numpy())                      # template 1 does not cover frame 0
    assert np.isfinite(flow[0].numpy()[:, zero]).all() and np.isfinite(flow[1:].numpy()[:, :, found.numpy()]).all()


# ---- 5. interface ------------------------------------------------------------------------------------------------------------
def test_interface_out_and_documented_errors():
    from mft_amd import TrackAtlas
    s0, s1 = two_template_stores(amp=5.0)
    atlas = TrackAtlas([(0, s0), (1, s1)])
    H, W = AH, AW
    flow, occl, sigma, found, template = atlas.results_from(2, [1])
    r, f2, t2 = atlas.result_from(2, 1)
    assert isinstance(r, FlowOUTrackingResult) and (r.H, r.W) == (H, W)
    assert r.flow.shape == (2, H, W) and r.occlusion.shape == (1, H, W) and r.sigma.shape == (1, H, W)
    assert np.array_equal(bits(r.flow), bits(flow[0])) and np.array_equal(bits(r.occlusion), bits(occl[0]))
    assert np.array_equal(bits(r.sigma), bits(sigma[0])) and torch.equal(f2, found) and torch.equal(t2, template)
    # out: written in place, inside a larger buffer that is left alone
    big = [torch.full((4, c, H, W), -7.0) for c in (2, 1, 1)]
    out = tuple(b[1:3] for b in big)
    got = atlas.results_from(2, [1, 0], out=out)
    assert all(g is o for g, o in zip(got[:3], out))
    want = atlas.results_from(2, [1, 0])
    for g, w, b in zip(got[:3], want[:3], big):
        assert np.array_equal(bits(g), bits(w)) and (b[0] == -7).all() and (b[3] == -7).all()
    # an empty list of frames, and a repeated id
    e = atlas.results_from(2, [])
    assert e[0].shape == (0, 2, H, W) and e[1].shape == (0, 1, H, W) and e[2].shape == (0, 1, H, W) and torch.equal(e[3], found)
    rep = atlas.results_from(2, [1, 0, 1])
    for g, w in zip(rep[:3], want[:3]):
        assert np.array_equal(bits(g[0]), bits(w[0])) and np.array_equal(bits(g[1]), bits(w[1])) and np.array_equal(bits(g[2]), bits(w[0]))
    # the threshold is the inverse's
    assert torch.equal(atlas.results_from(2, [1], occlusion_threshold=0.1)[4], torch.where(
        atlas.inverse(2, 0.1)[2] >= 0, atlas.inverse(2, 0.1)[2], torch.full((), -1, dtype=torch.int32)))
    # a frame that no entry holds is no error as a column: nothing covers it
    u = atlas.results_from(2, [7])
    assert_fill(u[0], u[1], u[2], np.ones((1, H, W), bool))
    for call in (lambda: atlas.results_from(7), lambda: atlas.results_from(7, [1]), lambda: atlas.result_from(7, 1),
                 lambda: atlas.result_from(1, 7), lambda: atlas.covered(7)):
        with pytest.raises(KeyError):
            call()
    ok = lambda: [torch.zeros(2, 2, H, W), torch.zeros(2, 1, H, W), torch.zeros(2, 1, H, W)]
    bad = []
    for i, t in ((0, torch.zeros(2, 1, H, W)), (1, torch.zeros(2, H, W)), (2, torch.zeros(2, 1, H, W, dtype=torch.float64)),
                 (1, torch.zeros(3, 1, H, W)), (0, torch.zeros(2, 2, H, 2 * W)[..., ::2]), (2, np.zeros((2, 1, H, W), np.float32))):
        o = ok()
        o[i] = t
        bad.append(o)
    bad.append(ok()[:2])
    for o in bad:
        with pytest.raises(ValueError):
            atlas.results_from(2, [1, 0], out=o)
    with pytest.raises(KeyError):
        atlas.results_from(7, [1, 0], out=bad[0])                                      # the KeyError comes first


# ---- 6. plumbing -------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_exported_and_checks_its_arguments():
    import ctypes
    import re
    from pathlib import Path
    from mft_amd import _lib, ops
    repo = Path(__file__).resolve().parents[1]
    name = "mftx_trackstore_flow_from"
    assert re.search(r"\b%s\s*\(" % name, (repo / "include" / "mftx.h").read_text()) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, name)
    variant = repo / "mft_amd" / "libmftx_lfwide.so"
    if variant.exists():
        assert hasattr(ctypes.CDLL(str(variant)), name)
    assert callable(ops.trackstore_flow_from) and callable(ops.trackstore_slot_addresses) and ops.TRACKSTORE_FLOW_COLUMNS == 16
    ff = lib.mftx_trackstore_flow_from
    buf = (ctypes.c_double * 8)()                                                     # host memory: only its address is looked at
    a = ctypes.addressof(buf)
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a16 = a if a % 16 == 0 else a + 8

    def call(table=a16, entry=a, row_of=a, frames=a, lohis=a, n_ranks=1, R=1, T=1, H=8, W=8, cpb=0, flow=a, occl=a, sigma=a):
        return ff(table, entry, row_of, frames, lohis, n_ranks, R, T, H, W, cpb, flow, occl, sigma, None)

    err = lib.mftx_last_error_string
    assert call(T=0) == 0 and call(T=0, table=None, flow=None) == 0                   # no columns: a no-op
    assert call(T=-1) == -1 and b"trackstore_flow_from" in err()
    assert call(H=1) == -1 and call(W=1) == -1 and call(cpb=-1) == -1 and call(n_ranks=0) == -1 and call(R=0) == -1
    for arg in ("table", "entry", "row_of", "frames", "lohis", "flow", "occl", "sigma"):
        assert call(**{arg: None}) == -1 and err().endswith(b"null pointer: " + arg.encode()), arg
    assert call(H=65536, W=32768) == -1 and b"2^31" in err()
    assert call(T=65536 * 2, cpb=1) == -1 and b"column blocks" in err()
    assert call(table=a16 + 8) == -2 and b"table must be 16-byte aligned" in err()
    assert call(frames=a + 4) == -2 and b"frames" in err() and call(lohis=a + 4) == -2
    for arg in ("entry", "row_of", "flow", "occl", "sigma"):
        assert call(**{arg: a + 2}) == -2 and (arg.encode() + b" must be 4-byte aligned") in err(), arg
