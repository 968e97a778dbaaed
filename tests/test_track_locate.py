"""``DenseTrackStore.locate`` / ``tracks_from`` on the host (device="cpu": the numpy float32 restatement of the definition in
DESIGN.md, "locate"): points given ON a stored frame are taken back to the template points they are the images of.  No GPU needed.

The builders of this file (fields, stores, points) are shared with tests/test_gpu_track_locate.py, which holds the device path to
this restatement bit for bit."""
import numpy as np
import pytest
import torch

import golden_inputs as gi

EPS = 2.0 ** -10                 # the definition's acceptance residual
TOL = 2.0 ** -9                  # ... and what a round trip may be off by: see test_injective_round_trip


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def field(seed, H, W, amp):
    """Seeded smooth planes as tests/test_gpu_trackstore.py::field makes them, the flow's amplitude given: 1.5 is injective
    (checked where it matters), 5.0 folds."""
    r = gi._rng(91, seed, H, W)
    flow = gi.smooth_field(r, 2, H, W, cells=4, amp=amp)
    occl = np.clip(gi.smooth_field(r, 1, H, W, cells=5, amp=0.6), 0, 1).astype(np.float32)
    sigma = (0.05 + np.abs(gi.smooth_field(r, 1, H, W, cells=5, amp=0.7))).astype(np.float32)
    return flow.astype(np.float32), occl, sigma


def const_planes(H, W, fx=0.0, fy=0.0, occl=0.0, sigma=0.0):
    flow = np.stack([np.broadcast_to(np.float32(fx), (H, W)), np.broadcast_to(np.float32(fy), (H, W))]).astype(np.float32)
    o = np.broadcast_to(np.float32(occl), (H, W)).astype(np.float32)[None]
    s = np.broadcast_to(np.float32(sigma), (H, W)).astype(np.float32)[None]
    return flow, o.copy(), s.copy()


def make_store(H, W, frames, device="cpu", **kw):
    """frames: {frame id: (flow, occl, sigma) numpy planes}, appended in the dict's order."""
    from mft_amd.trackstore import DenseTrackStore
    st = DenseTrackStore(H, W, device=device, **kw)
    for f, planes in frames.items():
        st.append(tuple(T(p).to(device) for p in planes), f)
    return st


FRAME_IDS = (3, 8, 5)            # three stored frames, appended in this order
# Seeds whose amplitude-1.5 flow has the gradient the round trip's tolerance presumes (at most 0.34 per pixel: at 37 x 53, where
# the coarse grid's cells are 9 pixels wide, few seeds do; test_injective_round_trip asserts it)
GENTLE_SEEDS = {(37, 53): (437, 2224, 2877), (64, 64): (14, 64, 115)}


def smooth_frames(H, W, amp):
    seeds = GENTLE_SEEDS[(H, W)] if amp == 1.5 else (0, 1, 2)
    return {f: field(seed, H, W, amp) for seed, f in zip(seeds, FRAME_IDS)}


def template_points(n, H, W, seed=0):
    """n seeded template points inside the template's grid [0, W - 1] x [0, H - 1]."""
    r = np.random.default_rng([seed, H, W])
    return (r.uniform(0, 1, size=(n, 2)) * np.array([W - 1, H - 1])).astype(np.float32)


def lipschitz(p):
    """max |difference of horizontal neighbours| + max |difference of vertical neighbours| of a plane: what its bilinear
    interpolant moves by, at most, per pixel of max-norm distance."""
    return float(np.abs(np.diff(p, axis=-1)).max() + np.abs(np.diff(p, axis=-2)).max())


def choice_planes(H, W, sigma_left, sigma_right, occl_right):
    """Left half: zero flow.  Right half: shifted by exactly -W/2 in x, so that both halves land on x in [0, W/2).  Sigma
    ``sigma_left`` / ``sigma_right``; occlusion 0 on the left, ``occl_right`` on the right.  Every value is an end of its
    channel's range (or the channel is flat), so the quantisation keeps it exactly."""
    flow, occl, sigma = const_planes(H, W, sigma=sigma_left)
    flow[0, :, W // 2:] = -(W // 2)
    sigma[0, :, W // 2:] = sigma_right
    occl[0, :, W // 2:] = occl_right
    return flow, occl, sigma


def shifted_out_planes(H, W):
    """Flow +(W + 8) in x everywhere: nothing maps into the frame."""
    return const_planes(H, W, fx=W + 8.0, sigma=0.25)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. identity -------------------------------------------------------------------------------------------------------------
def test_identity_returns_the_points_and_their_cells():
    H, W = 37, 53
    st = make_store(H, W, {4: const_planes(H, W)})
    # Points on a lattice of eighths (exact in float32), the frame's corners and edges included.  A point ON a shared edge is a
    # candidate of both cells with equal keys but for the cell, and goes to the lower one.  (A point closer than eps to an edge
    # without being on it is, by the definition's clamp, a candidate of the neighbouring cell too -- at its edge, up to eps
    # away: the 4-ulp claim is for points on an edge or at least eps from it, which a lattice of eighths guarantees.)
    r = np.random.default_rng(5)
    P = np.stack([r.integers(0, 8 * (W - 1) + 1, size=150), r.integers(0, 8 * (H - 1) + 1, size=150)], axis=1).astype(np.float32) / 8
    P = np.concatenate([P, [[0, 0], [W - 1, H - 1], [W - 1, 0], [0, H - 1], [7, 9], [7, 9.5], [7.5, 9], [W - 1, 11.25], [20.125, H - 1]]]).astype(np.float32)
    table, cell = st.locate(P, 4)
    assert table.shape == (len(P), 4) and table.dtype == torch.float32 and cell.shape == (len(P),) and cell.dtype == torch.int32
    table, cell = table.numpy(), cell.numpy()
    assert np.abs(table[:, 0:2] - P).max() <= 4 * 2.0 ** -23 * max(H, W)
    assert not table[:, 2:4].any()
    j = np.minimum(np.where(P[:, 0] == np.floor(P[:, 0]), P[:, 0] - 1, np.floor(P[:, 0])).clip(0), W - 2)
    i = np.minimum(np.where(P[:, 1] == np.floor(P[:, 1]), P[:, 1] - 1, np.floor(P[:, 1])).clip(0), H - 2)
    assert np.array_equal(cell, (i * (W - 1) + j).astype(np.int32))
    # closer than eps to an edge: still within eps of the point
    near = np.array([[7 + 2.0 ** -12, 9.5], [30.25, 12 - 2.0 ** -11]], np.float32)
    t, c = st.locate(near, 4)
    assert (c.numpy() >= 0).all() and np.abs(t.numpy()[:, 0:2] - near).max() <= EPS


# ---- 2. injective round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_injective_round_trip(H, W):
    frames = smooth_frames(H, W, 1.5)
    st = make_store(H, W, frames)
    P = template_points(120, H, W)
    Q = st.query(P).numpy()                                       # [120, 3, 4], columns in append order
    for k, f in enumerate(FRAME_IDS):
        r = st.result(f)
        # The premise of the tolerance: the stored flow's gradient is at most 0.34 per pixel, so P -> P + flow(P) moves two
        # points apart by at least (1 - 0.34) of their distance, and a template point whose image is within eps of Q is within
        # eps / (1 - 0.34) < 2 eps = 2^-9 px of the one whose image is Q.  (In the max norm the flow's Lipschitz constant is
        # the larger row sum of these gradients; below 1 the map is injective, which is asserted too.)
        fl = r.flow.numpy()
        gx, gy = np.abs(np.diff(fl, axis=2)).max(axis=(1, 2)), np.abs(np.diff(fl, axis=1)).max(axis=(1, 2))
        grad = max(gx.max(), gy.max())
        print(f"{H}x{W} frame {f}: max flow gradient {grad:.3f}, max-norm Lipschitz constant {(gx + gy).max():.3f}")
        assert grad <= 0.34 and (gx + gy).max() < 1
        table, cell = st.locate(Q[:, k, 0:2], f)
        table, cell = table.numpy(), cell.numpy()
        assert (cell >= 0).all()
        err = np.abs(table[:, 0:2] - P).max()
        print(f"    template point recovered within {err:.3g} px")
        assert err <= TOL
        ci, cj = cell // (W - 1), cell % (W - 1)
        assert (np.abs(table[:, 0] - (cj + 0.5)) <= 0.5).all() and (np.abs(table[:, 1] - (ci + 0.5)) <= 0.5).all()
        # occlusion and sigma: query's values at P, up to what the two interpolants differ by over TOL in each coordinate
        for ch, plane in ((2, r.occlusion.numpy()[0]), (3, r.sigma.numpy()[0])):
            assert np.abs(table[:, ch] - Q[:, k, ch]).max() <= lipschitz(plane) * TOL + 1e-6


# ---- 3. folding field --------------------------------------------------------------------------------------------------------
def test_folding_field_every_located_point_maps_back_onto_the_query():
    H, W = 37, 53
    st = make_store(H, W, smooth_frames(H, W, 5.0))
    fl = st.result(FRAME_IDS[0]).flow.numpy()
    assert np.abs(np.diff(fl, axis=2)).max() > 1.0                # it does fold
    P = template_points(120, H, W)
    Q = st.query(P).numpy()
    moved = 0
    for k, f in enumerate(FRAME_IDS):
        table, cell = st.locate(Q[:, k, 0:2], f)
        assert (cell.numpy() >= 0).all()                          # each query is the image of a template point
        back = st.query(table[:, 0:2], frames=[f]).numpy()[:, 0, 0:2]
        err = np.abs(back - Q[:, k, 0:2]).max()
        moved += int((np.abs(table.numpy()[:, 0:2] - P).max(axis=1) > TOL).sum())
        print(f"frame {f}: located points map back within {err:.3g} px")
        assert err <= TOL                                         # eps plus the sampler's rounding
    print(f"{moved} of {3 * len(P)} queries came back as another preimage")


# ---- 4. choice rule ----------------------------------------------------------------------------------------------------------
CHOICE_HW = (40, 56)


def choice_frames():
    H, W = CHOICE_HW
    # (frame 0: the constant sigma is 0, the one constant that every interpolation weight keeps exactly -- the four weights of a
    # cell sum to 1 only up to rounding, so a constant 0.5 comes out an ulp apart in different cells and the tie is no tie)
    return {0: choice_planes(H, W, 0.0, 0.0, 0.0), 1: choice_planes(H, W, 0.5, 0.125, 0.0), 2: choice_planes(H, W, 0.5, 0.125, 1.0)}


def choice_queries():
    """x <= W/2 - 2, off the grid lines; the first six have x <= 13 (see test_choice_rule)."""
    return np.array([[1.25, 3.5], [5.5, 0.25], [12.75, 20.5], [9.5, 38.25], [3.25, 17.75], [13.0, 30.5],
                     [14.5, 2.25], [20.25, 11.5], [25.5, 33.75], [26.0, 8.5]], np.float32)


def test_choice_rule():
    H, W = CHOICE_HW
    half = W // 2
    st = make_store(H, W, choice_frames())
    Q = choice_queries()
    assert Q[:, 0].max() <= half - 2
    row = np.floor(Q[:, 1]).astype(np.int64)
    col = np.where(Q[:, 0] == np.floor(Q[:, 0]), Q[:, 0] - 1, np.floor(Q[:, 0])).astype(np.int64)
    left, right, seam = row * (W - 1) + col, row * (W - 1) + half + col, row * (W - 1) + half - 1
    ulp4 = 4 * 2.0 ** -23 * max(H, W)

    def located(frame, **kw):
        table, cell = st.locate(Q, frame, **kw)
        return table.numpy(), cell.numpy()

    # equal sigma: the left cell, the lowest index
    t, c = located(0)
    assert np.array_equal(c, left) and np.abs(t[:, 0:2] - Q).max() <= ulp4 and not t[:, 2:4].any()
    # lower sigma on the right half: the right half's cell
    t, c = located(1)
    assert np.array_equal(c, right) and np.abs(t[:, 0] - (Q[:, 0] + half)).max() <= ulp4 and np.abs(t[:, 1] - Q[:, 1]).max() <= ulp4
    assert np.abs(t[:, 3] - 0.125).max() <= 1e-7 and (t[:, 2] == 0).all()
    # ... but occluded there: the left cell again.  The cell ACROSS the seam (columns W/2 - 1 .. W/2) is a fold whose image runs
    # from x = W/2 - 1 back to 0: a real preimage of every query, at u = 1 - x / (W/2 - 1), where occlusion is u and sigma lies
    # between the halves'.  For x <= 13 that is u > 0.5: occluded, and it loses to the left cell as the right half's does.
    # For x > 13.5 it is not occluded and of lower sigma than the left cell, so by the definition the seam cell is the answer.
    t, c = located(2)
    low = Q[:, 0] <= 13
    assert low.sum() == 6 and np.array_equal(c[low], left[low]) and np.abs(t[low, 0:2] - Q[low]).max() <= ulp4
    assert np.array_equal(c[~low], seam[~low])
    u = 1 - Q[~low, 0] / (half - 1)
    assert np.abs(t[~low, 0] - (half - 1 + u)).max() <= TOL and np.abs(t[~low, 2] - u).max() <= TOL and (t[~low, 2] <= 0.5).all()
    # with the threshold at 1.0 nothing counts as occluded and the right half wins once more
    t, c = located(2, occlusion_threshold=1.0)
    assert np.array_equal(c, right) and np.abs(t[:, 2] - 1).max() <= 1e-6 and np.abs(t[:, 3] - 0.125).max() <= 1e-7


# ---- 5. no preimage ----------------------------------------------------------------------------------------------------------
def no_preimage_case(H=40, W=56):
    """(frames, queries, per-point frame ids, found): a frame nothing of which lands inside the frame next to an ordinary one."""
    frames = {7: shifted_out_planes(H, W), 2: field(1, H, W, 1.5)}
    inside = template_points(9, H, W, seed=3)
    q = np.concatenate([inside, inside + np.array([W + 8.0, 0], np.float32), inside[:4]]).astype(np.float32)
    ids = [7] * 9 + [7] * 9 + [2] * 4
    found = np.array([False] * 9 + [True] * 9 + [True] * 4)
    return frames, q, ids, found


def test_no_preimage():
    H, W = 40, 56
    frames, q, ids, want_found = no_preimage_case(H, W)
    st = make_store(H, W, frames)
    table, cell = st.locate(q[:9], 7)
    assert (cell.numpy() == -1).all() and np.isnan(table.numpy()).all()
    far = np.array([[1.0e5, -1.0e5], [np.nan, 3.0], [-50.0, 4.0]], np.float32)                # far outside every image; a NaN
    table, cell = st.locate(far, 2)
    assert (cell.numpy() == -1).all() and np.isnan(table.numpy()).all()
    # frame 2 has an ordinary flow: its queries are made images of template points first
    q = q.copy()
    q[18:] = st.query(q[18:], frames=[2]).numpy()[:, 0, 0:2]
    coords, occl, found = st.tracks_from(q, ids)
    assert coords.shape == (22, 2, 2) and occl.shape == (22, 2) and found.dtype == bool and np.array_equal(found, want_found)
    assert np.isnan(coords[:9]).all() and (occl[:9] == 1).all()
    table, cell = st.locate(q, ids)
    ok = np.flatnonzero(want_found)
    want = st.query(table[ok, 0:2]).numpy()
    assert np.array_equal(coords[ok], want[:, :, 0:2]) and np.array_equal(occl[ok], want[:, :, 2])
    assert np.abs(coords[9:18, 0] - q[9:18]).max() <= TOL and np.abs(coords[18:, 1] - q[18:]).max() <= TOL
    c1, o1, f1 = st.tracks_from(q[9:18], 7, frames=[2])
    assert c1.shape == (9, 1, 2) and f1.all() and np.array_equal(c1[:, 0], coords[9:18, 1]) and np.array_equal(o1[:, 0], occl[9:18, 1])


# ---- 6. mixed frames in one call; errors -------------------------------------------------------------------------------------
def mixed_ids(n):
    """Per-point frame ids: unsorted, frames repeated, frame 5 given for ONE point."""
    ids = [FRAME_IDS[(3 * k + k // 4) % 2] for k in range(n)]          # frames 3 and 8, interleaved
    if n > 2:
        ids[n // 2] = 5
    return ids


def test_mixed_frames_in_one_call_equal_the_per_frame_calls():
    H, W = 37, 53
    st = make_store(H, W, smooth_frames(H, W, 5.0))
    P = template_points(41, H, W, seed=2)
    ids = mixed_ids(41)
    assert ids.count(5) == 1 and ids != sorted(ids) and ids.count(3) > 5 and ids.count(8) > 5
    Q = st.query(P).numpy()
    q = np.stack([Q[n, FRAME_IDS.index(f), 0:2] for n, f in enumerate(ids)])
    table, cell = st.locate(q, ids)
    assert (cell.numpy() >= 0).all()
    for f in FRAME_IDS:
        sel = np.flatnonzero(np.array(ids) == f)
        t, c = st.locate(q[sel], f)
        assert np.array_equal(bits(table.numpy()[sel]), bits(t.numpy())) and np.array_equal(cell.numpy()[sel], c.numpy())
    t2, c2 = st.locate(T(q), np.array(ids))                                          # a tensor of points, an array of ids
    assert np.array_equal(bits(t2.numpy()), bits(table.numpy())) and torch.equal(c2, cell)
    out = (torch.full((41, 4), -7.0), torch.full((41,), -7, dtype=torch.int32))
    got = st.locate(q, ids, out=out)
    assert got[0] is out[0] and got[1] is out[1] and np.array_equal(bits(out[0].numpy()), bits(table.numpy())) and torch.equal(out[1], cell)
    t0, c0 = st.locate(np.zeros((0, 2), np.float32), 3)
    assert t0.shape == (0, 4) and c0.shape == (0,)


def test_documented_errors():
    H, W = 37, 53
    st = make_store(H, W, smooth_frames(H, W, 1.5))
    q = template_points(4, H, W)
    with pytest.raises(KeyError):
        st.locate(q, 99)
    with pytest.raises(KeyError):
        st.locate(q, [3, 8, 99, 5])
    with pytest.raises(KeyError):
        st.tracks_from(q, 3, frames=[3, 99])
    for bad in (np.zeros((4, 3), np.float32), np.zeros(8, np.float32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            st.locate(bad, 3)
    with pytest.raises(ValueError):
        st.locate(q, [3, 8, 5])                                                      # three ids for four points
    with pytest.raises(ValueError):
        st.locate(q, [[3, 8], [5, 3]])
    for out in ((torch.zeros(5, 4), torch.zeros(4, dtype=torch.int32)), (torch.zeros(4, 4), torch.zeros(4)),
                (torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError):
            st.locate(q, 3, out=out)


def test_group_tables():
    """ops.locate_tables: queries grouped by slot, stable; every address from its chunk's."""
    from mft_amd import ops
    slots = [5, 2, 5, 0, 2, 5, 7]
    buf, G, off = ops.locate_tables(slots, [1000, 2000], [100, 200], 4, 64)
    assert G == 4 and off == (0, 32, 64, 84, 112) and buf.dtype == np.int64 and buf.nbytes >= 112 + 28
    assert buf[:4].tolist() == [1000, 1000 + 2 * 64, 2000 + 64, 2000 + 3 * 64]                 # slots 0, 2, 5, 7
    assert buf[4:8].tolist() == [100, 100 + 2 * 32, 200 + 32, 200 + 3 * 32]
    tail = buf[8:].view(np.int32)
    assert tail[:5].tolist() == [0, 1, 3, 6, 7]
    assert tail[5:12].tolist() == [3, 1, 4, 0, 2, 5, 6] and tail[12:19].tolist() == [2, 1, 2, 0, 1, 2, 3]
    buf, G, off = ops.locate_tables([9], [0, 0, 4096], [0, 0, 512], 4, 8)
    assert G == 1 and buf[:2].tolist() == [4096 + 8, 512 + 32] and buf[2:].view(np.int32)[:4].tolist() == [0, 1, 0, 0]


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    import re
    from pathlib import Path
    from mft_amd import _lib, ops
    repo = Path(__file__).resolve().parents[1]
    name = "mftx_trackstore_locate"
    assert re.search(r"\b%s\s*\(" % name, (repo / "include" / "mftx.h").read_text()) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, name) and callable(ops.trackstore_locate) and lib.mftx_version() == 400
    # argument checks that need no device: they come before anything is launched
    null = (None, None, None, 1, None, None, 8, 8, 3, None, 0.5, None, None, None, None)
    assert lib.mftx_trackstore_locate(*null) == -1
    assert b"trackstore_locate" in lib.mftx_last_error_string()

    def call(G=1, H=8, W=8, N=3):
        return lib.mftx_trackstore_locate(None, None, None, G, None, None, H, W, N, None, 0.5, None, None, None, None)

    assert call(H=1) == -1 and call(W=1) == -1 and call(N=-1) == -1 and call(G=-1) == -1
    assert b"trackstore_locate" in lib.mftx_last_error_string()
    assert call(N=0) == 0 and call(N=0, G=0) == 0                                   # N == 0: a no-op
