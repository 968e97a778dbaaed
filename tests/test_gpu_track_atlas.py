"""The device paths of the track atlas: ``mftx_trackstore_append_multi`` (T results quantised in one call) against
``trackstore_append`` per frame, ``mftx_trackstore_invert_atlas`` (all entries of a video frame scattered onto one key plane) against
per-entry ``trackstore_invert`` plus the key minimum and against the sparse ``TrackAtlas.locate`` -- all bit for bit -- and a
``MultiTemplateMFT`` pass that keeps a store per template, through the real engine."""
import functools

import numpy as np
import pytest
import torch

import test_track_atlas as host
from mft_amd.synth import SyntheticVideo
from test_gpu_multi_template import _config, _frames_of
from test_track_locate import TOL, const_planes, make_store

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def words(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ---- 1. append_multi ---------------------------------------------------------------------------------------------------------
def append_frames(T, H, W):
    """T frames' planes, every plane a slice of ONE buffer that begins 4 bytes into an allocation: 4-byte aligned only (and with
    H W % 4 != 0 the planes are no multiple of 16 bytes apart).  Kinds in turn: a flat channel next to ordinary ones, sigma
    with +inf, the identity, a NaN, ordinary."""
    n = H * W
    r = np.random.default_rng([T, H, W])
    buf = torch.zeros(T * 4 * n + 1, dtype=torch.float32)
    frames = []
    for j in range(T):
        v = r.normal(size=(4, n)).astype(np.float32) * np.float32(1 + j)
        v[2], v[3] = np.abs(v[2]) % 1, np.abs(v[3]) + np.float32(0.05)
        kind = j % 5
        if kind == 0:
            v[2] = np.float32(0.25)                          # a flat occlusion
        elif kind == 1:
            v[3, r.integers(n)] = np.inf
        elif kind == 2:
            v[:] = 0                                          # the identity result
        elif kind == 3:
            v[0, r.integers(n)] = np.nan
        buf[1 + j * 4 * n: 1 + (j + 1) * 4 * n] = torch.from_numpy(v.reshape(-1))
    dev = buf.to(DEV)
    for j in range(T):
        p = dev[1 + j * 4 * n: 1 + (j + 1) * 4 * n]
        frames.append((p[:2 * n].view(2, H, W), p[2 * n:3 * n].view(1, H, W), p[3 * n:].view(1, H, W)))
    return frames


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (33, 47), (64, 96)])
@pytest.mark.parametrize("T", [1, 2, 5, 65])
def test_append_multi_is_append_per_frame_bitwise(T, H, W):
    from mft_amd import ops
    assert T <= 5 or T == ops.TRACKSTORE_APPEND_MULTI_FRAMES + 1                     # one more than an argument block carries
    frames = append_frames(T, H, W)
    assert frames[0][0].data_ptr() % 16 == 4
    want_p = torch.full((T, H, W, 4), 0x5555, dtype=torch.uint16, device=DEV)
    want_l = torch.full((T, 4, 2), -7.0, device=DEV)
    for j, planes in enumerate(frames):
        ops.trackstore_append(planes, want_p[j], want_l[j])
    got_p, got_l = torch.full_like(want_p, 0x3333), torch.full_like(want_l, -9.0)
    ops.trackstore_append_multi([(planes, got_p[j], got_l[j]) for j, planes in enumerate(frames)])
    assert torch.equal(words(got_p), words(want_p))
    assert torch.equal(bits(got_l), bits(want_l))
    if T >= 5:                                                                       # the kinds are what they are meant to be
        l = want_l.cpu().numpy()
        assert l[0, 2, 0] == l[0, 2, 1] == np.float32(0.25) and not words(want_p)[0, :, :, 2].any()
        assert np.isposinf(l[1, 3, 1]) and not l[2].any() and not words(want_p)[2].any()
    if H * W > 4:
        assert (H * W + 1023) // 1024 == {35: 1, 33 * 47: 2, 64 * 96: 6}[H * W]          # blocks of partials per frame


def test_append_multi_checks_its_arguments():
    from mft_amd import _lib, ops
    lib = _lib.load()
    H, W, T = 5, 7, 2
    frames = append_frames(T, H, W)
    packed = torch.zeros((T, H, W, 4), dtype=torch.uint16, device=DEV)
    lohi = torch.zeros((T, 4, 2), device=DEV)
    ws = torch.empty(lib.mftx_trackstore_append_multi_workspace_bytes(T), dtype=torch.uint8, device=DEV)

    def call(flow=None, packed_ptrs=None, ws_bytes=None, ws_ptr=ws.data_ptr()):
        arr = lambda ptrs: _lib.ptr_array(ptrs)
        a = [arr(flow or [f[0].data_ptr() for f in frames]), arr([f[1].data_ptr() for f in frames]), arr([f[2].data_ptr() for f in frames]),
             arr(packed_ptrs or [packed[j].data_ptr() for j in range(T)]), arr([lohi[j].data_ptr() for j in range(T)])]
        return lib.mftx_trackstore_append_multi(T, a[0][0], a[1][0], a[2][0], H, W, a[3][0], a[4][0], ws_ptr,
                                                ws.numel() if ws_bytes is None else ws_bytes, None)

    assert call(flow=[frames[0][0].data_ptr(), None]) == -1 and b"frame 1" in lib.mftx_last_error_string()       # a null plane
    assert call(ws_ptr=None) == -1
    rc = call(packed_ptrs=[packed[0].data_ptr(), packed[1].data_ptr() + 4])
    assert rc == -2 and b"8-byte aligned" in lib.mftx_last_error_string()                               # misaligned packed
    rc = call(ws_bytes=ws.numel() - 1)
    assert rc == -3 and b"workspace too small" in lib.mftx_last_error_string()
    torch.cuda.synchronize()
    assert not words(packed).any() and not lohi.any()                                                                   # nothing was launched
    assert call() == 0
    ops.trackstore_append_multi([])                                                                              # no frames: a no-op
    torch.cuda.synchronize()
    assert lohi.any()


# ---- 2. invert_atlas ---------------------------------------------------------------------------------------------------------
def affine(seed, H, W, shift):
    """A smooth random affine flow: gradients of at most 0.08 per pixel around a shift of up to ``shift`` px."""
    r = np.random.default_rng([77, seed])
    a = r.uniform(-0.08, 0.08, size=(2, 2)).astype(np.float32)
    b = r.uniform(-shift, shift, size=2).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    x, y = x - np.float32((W - 1) / 2), y - np.float32((H - 1) / 2)
    return np.stack([a[0, 0] * x + a[0, 1] * y + b[0], a[1, 0] * x + a[1, 1] * y + b[1]]).astype(np.float32)


def entry_planes(k, f, H, W):
    """Frame ``f`` of entry ``k``: 0 = affine with one torn cell whose box spans the frame; 1 and 2 = identical words; 3 = occluded
    on the left half at the LOWEST sigma (the others are visible there at higher sigma); 4 = an infinite corner.  (A stored
    channel holds an infinity only with an infinite range, which makes every value of it infinite or NaN: frame 2 of entry 4 is
    that.  At 24 x 40, where device is compared with device, its frame 1 has a corner near the largest value a channel can hold
    next to finite ones, 3e38: the boxes around it are limited in float, the cell arithmetic overflows, and the other pixels'
    flow x collapses onto the channel's minimum.)"""
    seed = 10 * f + (1 if k == 2 else k)
    flow = affine(seed, H, W, 2.0)
    r = np.random.default_rng([78, seed])
    occl = np.full((1, H, W), 0.125, np.float32)
    sigma = (0.25 + 0.5 * r.random((1, H, W))).astype(np.float32)
    if k == 0:
        flow[:, min(1, H - 1), min(1, W - 1)] = (W, H)                                # torn: the cells around it reach across the whole frame
    elif k == 3:
        occl[0, :, :(W + 1) // 2] = 0.875
        sigma[:] = 0.03125 + 0.03125 * r.random((1, H, W)).astype(np.float32)
    elif k == 4:
        if f == 2 or (H, W) == (24, 40):
            flow[0, min(1, H - 1), min(2, W - 1)] = np.inf if f == 2 else np.float32(3.0e38)
    return flow, occl, sigma


@functools.lru_cache(maxsize=None)
def case_stores(H, W, n, device):
    """n entries of template 0 over the video frames 0 (identity), 1 and 2."""
    return tuple(make_store(H, W, {0: const_planes(H, W), 1: entry_planes(k, 1, H, W), 2: entry_planes(k, 2, H, W)}, device=device)
                 for k in range(n))


def key_minimum(tables, cells, ranks, thr=0.5):
    """Per-entry inverse tables [E, H, W, 4] and cells [E, H, W] -> the winner by the smallest (occlusion > thr, bits of
    (sigma > 0 ? sigma : +0), rank), in torch: (table, cell, entry)."""
    s = tables[..., 3]
    sig = torch.where(s > 0, s, torch.zeros_like(s)).contiguous().view(torch.int32).to(torch.int64)
    occ = (tables[..., 2] > thr).to(torch.int64)
    rk = torch.tensor(ranks, dtype=torch.int64, device=tables.device).view(-1, 1, 1)
    key = occ * 2 ** 40 + sig * 2 ** 8 + rk
    key = torch.where(cells >= 0, key, torch.full_like(key, 2 ** 62))
    best, arg = key.min(dim=0)
    found = best < 2 ** 62
    t = torch.gather(tables, 0, arg[None, ..., None].expand(1, *arg.shape, 4))[0]
    c = torch.gather(cells, 0, arg[None])[0]
    e = rk.view(-1)[arg].to(torch.int32)
    nan = torch.full((), float("nan"), device=tables.device)
    return torch.where(found[..., None], t, nan), torch.where(found, c, torch.full_like(c, -1)), torch.where(found, e, torch.full_like(e, -1))


def assert_same3(got, want):
    assert torch.equal(got[1].cpu(), want[1].cpu()), np.flatnonzero((got[1].cpu() != want[1].cpu()).numpy().ravel())[:10]
    assert torch.equal(got[2].cpu(), want[2].cpu()), np.flatnonzero((got[2].cpu() != want[2].cpu()).numpy().ravel())[:10]
    assert torch.equal(bits(got[0]), bits(want[0]))


@pytest.mark.parametrize("layout", [(1,), (2,), (5,), (5, 0, 2), (0, 2, 0)])
@pytest.mark.parametrize("H,W", [(2, 2), (9, 34), (24, 40)])
def test_invert_atlas_is_per_entry_invert_plus_the_key_minimum(H, W, layout):
    """Plane g holds video frame 1 + g % 2 of the first layout[g] entries; the ranks reported are 3 * k + 1."""
    from mft_amd import ops
    stores = case_stores(H, W, 5, DEV)
    G = len(layout)
    views, ranks, first_of = [], [], [0]
    for g, n in enumerate(layout):
        f = 1 + g % 2
        views += [(st.packed(st.slot_of(f)), st.lohi(st.slot_of(f))) for st in stores[:n]]
        ranks += [3 * k + 1 for k in range(n)]
        first_of.append(len(views))
    table = torch.full((G, H, W, 4), -7.0, device=DEV)
    cell = torch.full((G, H, W), -77, dtype=torch.int32, device=DEV)
    entry = torch.full((G, H, W), -77, dtype=torch.int32, device=DEV)
    got = ops.trackstore_invert_atlas(views, first_of, ranks, table, cell, entry)
    assert got[0] is table and got[2] is entry
    for g, n in enumerate(layout):
        f = 1 + g % 2
        if n == 0:
            assert (cell[g] == -1).all() and (entry[g] == -1).all() and (bits(table[g]) == 0x7fc00000).all()
            continue
        per = [st.inverse(f) for st in stores[:n]]                                   # mftx_trackstore_invert, entry by entry
        want = key_minimum(torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]), [3 * k + 1 for k in range(n)])
        assert_same3((table[g], cell[g], entry[g]), want)
        if n == 1:                                                                   # one entry: invert plus entry
            assert torch.equal(bits(table[g]), bits(per[0][0])) and torch.equal(cell[g], per[0][1])
            assert torch.equal(entry[g] >= 0, cell[g] >= 0) and ((entry[g] == 1) | (entry[g] == -1)).all()
    if layout == (5,) and (H, W) != (2, 2):
        e = entry[0].cpu().numpy()
        print(f"{H}x{W}: entries win {[int((e == 3 * k + 1).sum()) for k in range(5)]} pixels, {int((e < 0).sum())} not found")
        assert (e != 7).all()                                                        # identical words: the lower rank, everywhere
        assert (e == 4).sum() > 0                                                    # its twin does win pixels
        # entry 3 (rank 10) has the lowest sigma everywhere: it wins where it is visible, and where it is occluded it loses to
        # every visible entry
        o3, c3 = per[3][0][..., 2].cpu().numpy(), per[3][1].cpu().numpy()
        others = np.zeros_like(c3, dtype=bool)
        for k in (0, 1, 4):
            others |= (per[k][1].cpu().numpy() >= 0) & (per[k][0][..., 2].cpu().numpy() <= 0.5)
        lost = (c3 >= 0) & (o3 > 0.5) & others
        print(f"    entry 3 is occluded and another entry visible at {int(lost.sum())} pixels; it is visible at {int(((c3 >= 0) & (o3 <= 0.5)).sum())}")
        assert lost.sum() > 0 and (e[lost] != 10).all() and (e[(c3 >= 0) & (o3 <= 0.5)] == 10).all() and (e == 10).sum() > 0


@pytest.mark.parametrize("H,W", [(9, 34), (24, 40)])
def test_invert_is_invert_atlas_with_one_entry_per_plane_bytewise(H, W):
    """``mftx_trackstore_invert`` and ``mftx_trackstore_invert_atlas`` launch the same two kernels, the first in their identity
    mode (no first_of: plane g is frame g, the key's low word all cell), the second with first_of = [0, 1, 2, 3]: one mode
    pinned against the other on G = 3 frames.  At 9 x 34 the 33 cell columns make two ragged tile columns; entry 0 has the torn
    cell that the whole wave walks."""
    from mft_amd import ops
    st = case_stores(H, W, 1, DEV)[0]
    slots = [st.slot_of(f) for f in (1, 2, 0)]
    table = torch.full((3, H, W, 4), -7.0, device=DEV)
    cell = torch.full((3, H, W), -77, dtype=torch.int32, device=DEV)
    ops.trackstore_invert(st._chunks, st._lohi, slots, table, cell)
    a_table, a_cell, a_entry = torch.full_like(table, -9.0), torch.full_like(cell, -99), torch.full_like(cell, -99)
    ops.trackstore_invert_atlas([(st.packed(s), st.lohi(s)) for s in slots], [0, 1, 2, 3], [0, 0, 0], a_table, a_cell, a_entry)
    assert torch.equal(bits(table), bits(a_table))
    assert torch.equal(cell.cpu(), a_cell.cpu())
    assert torch.equal(a_entry.cpu(), torch.where(cell >= 0, 0, -1).to(torch.int32).cpu())
    assert (cell >= 0).any()


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(2, 2), (9, 34), (24, 40)])
def test_atlas_inverse_locate_and_the_host_atlas_agree_bitwise(H, W, n):
    from mft_amd import TrackAtlas
    dev = TrackAtlas([(0, st) for st in case_stores(H, W, n, DEV)])
    g = torch.from_numpy(host.grid(H, W)).to(DEV)
    dense = dev.inverse([1, 2, 0])
    assert dense[0].shape == (3, H, W, 4) and dense[0].is_cuda and dense[2].dtype == torch.int32
    for k, f in enumerate((1, 2, 0)):
        sparse = dev.locate(g, f)                                                    # one mftx_trackstore_locate call + the reduction
        assert_same3((dense[0][k].reshape(-1, 4), dense[1][k].reshape(-1), dense[2][k].reshape(-1)), sparse)
        one = dev.inverse(f)
        assert_same3(one, (dense[0][k], dense[1][k], dense[2][k]))
    ids = [(i * 7 + i // 5) % 3 for i in range(H * W)]                               # per-point frames, unsorted, in one call
    mixed = dev.locate(g, ids)
    for k, f in enumerate((1, 2, 0)):
        sel = torch.tensor([i for i, x in enumerate(ids) if x == f], dtype=torch.int64, device=DEV)
        assert_same3(tuple(m[sel] for m in mixed), (dense[0][k].reshape(-1, 4)[sel], dense[1][k].reshape(-1)[sel], dense[2][k].reshape(-1)[sel]))
    if (H, W) != (24, 40):                                                           # the host atlas: numpy per cell
        cpu = TrackAtlas([(0, st) for st in case_stores(H, W, n, "cpu")])
        assert_same3(dense, cpu.inverse([1, 2, 0]))
    with pytest.raises(KeyError):
        dev.inverse([1, 9])


def test_invert_atlas_refuses_what_its_key_cannot_hold():
    from mft_amd import _lib, ops
    st = case_stores(2, 2, 1, DEV)[0]
    view = (st.packed(0), st.lohi(0))                                                 # the identity frame: every pixel found, cell 0
    out = (torch.empty((1, 2, 2, 4), device=DEV), torch.empty((1, 2, 2), dtype=torch.int32, device=DEV),
           torch.empty((1, 2, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.MftxError, match="256"):
        ops.trackstore_invert_atlas([view] * 257, [0, 257], list(range(257)), *out)
    ops.trackstore_invert_atlas([view] * 256, [0, 256], list(range(256)), *out)       # 256 entries of identical words: rank 0
    assert (out[2] == 0).all() and (out[1] == 0).all()
    with pytest.raises(_lib.MftxError):
        ops.trackstore_invert_atlas([view], [0, 2], [0], *out)
    lib = _lib.load()
    assert lib.mftx_trackstore_invert_atlas(None, None, None, None, 1, 257, 2, 2, 0.5, None, None, None, None, None) == -1


# ---- 3. the pass -------------------------------------------------------------------------------------------------------------
N_FRAMES = 12
PASSES = (((0, 3, 5), +1), ((11, 7), -1))


def _video():
    return SyntheticVideo(128, 160, n_frames=N_FRAMES, seed=21)


def _conf(fif, **extra):
    conf = _config([np.inf, 1, 2, 4], 4, fif)
    for k, v in extra.items():
        setattr(conf, k, v)
    return conf


def _run_pass(conf, video, starts, direction):
    from mft_amd.multi import MultiTemplateMFT
    mt = MultiTemplateMFT(conf)
    mt.init(starts, time_direction=direction)
    out = {}
    for f in _frames_of(min(starts) if direction > 0 else max(starts), len(video), direction):
        metas = mt.track(f, video[f])
        out[f] = {s: (tuple(p.clone() for p in m.result.planes()), list(mt.templates[s].last_pairs),
                      None if mt.templates[s].last_chosen is None else mt.templates[s].last_chosen.clone()) for s, m in metas.items()}
    return mt, out


@functools.lru_cache(maxsize=None)
def passes_with_stores(fif):
    video = _video()
    return tuple(_run_pass(_conf(fif, multi_template_stores=True, track_store_frames_per_chunk=5), video, starts, d) for starts, d in PASSES)


@pytest.mark.parametrize("fif", [1, 2])
def test_pass_keeps_the_single_trackers_stores_bitwise(fif):
    video = _video()
    tracker = _conf(fif, track_store=True, track_store_frames_per_chunk=5)
    tracker = tracker.tracker_class(tracker)
    for (starts, direction), (mt, got) in zip(PASSES, passes_with_stores(fif)):
        plain, want = _run_pass(_conf(fif), video, starts, direction)
        assert plain.track_stores == {} and sorted(mt.track_stores) == sorted(starts)
        for f in want:                                                               # the results do not change
            for s in want[f]:
                assert all(torch.equal(a, b) for a, b in zip(got[f][s][0], want[f][s][0])), (s, f)
                assert got[f][s][1] == want[f][s][1]
                assert (got[f][s][2] is None and want[f][s][2] is None) or torch.equal(got[f][s][2], want[f][s][2])
        for s in starts:
            for k, f in enumerate(_frames_of(s, len(video), direction)):
                tracker.init(video[f], start_frame_i=s, time_direction=direction) if k == 0 else tracker.track(video[f])
            host.same_store(mt.track_stores[s], tracker.track_store)
            assert mt.track_stores[s].frames_per_chunk == 5 and len(mt.track_stores[s]._chunks) == -(-len(mt.track_stores[s]) // 5)
        assert mt.stats["store_append_calls"] == mt.stats["frames"] == len(want)         # ONE append call per frame


def test_tracks_from_any_frame_through_the_atlas():
    """Points given on frame 6, at the images of a grid of template-3 points P, followed through the atlas of both passes, come
    back within the store's documented quantisation bound (README: 0.51 (max - min) / 65535 + 2^-21 max(|min|, |max|) per channel
    and frame; for coordinates plus the rounding of x + flow x, as tests/test_trackstore.py has it) of ``stores[3].tracks(P)``.
    Measured: 79 of the 80 points are located within 7.63e-06 px of their grid point and their tracks differ by at most 2.3e-05 px
    (three fp32 spacings of the coordinate) against bounds of 1.5e-05 (the identity frame, where they differ by 7.6e-06) to 1.1e-04; the channel bound alone (0 on the identity frame, 7e-06
    .. 1e-04 on the stand-in weights' sub-pixel flows) is below the coordinates' own rounding.  That comparison is defined where the atlas follows the template point P itself: the
    stand-in weights' flows fold, so an image point can have several preimages, and of those ``locate`` returns the one with
    the smallest key, not necessarily P (where it returns another, the tracks are those of another template point, up to 3.67 px
    away); and a point that another template wins is followed on that template, whose stand-in flows describe another motion.
    So the bound is asserted (a) through template 3's store alone, on the points whose located template point is within the
    round trip's tolerance of P -- at least a quarter of the grid, P being a preimage of its own image everywhere -- and (b)
    through the whole atlas on those of them that template 3 wins.  Also: every found point is back on its query at frame 6,
    each track is its winner's ``query`` of the located point, a one-entry atlas is the store's own ``tracks_from``, and on
    every frame the atlas finds at least the pixels the template-0 store finds alone."""
    from mft_amd import TrackAtlas
    fwd, bwd = (p[0] for p in passes_with_stores(1))
    atlas = TrackAtlas.from_passes(fwd, bwd)
    assert [t for t, _ in atlas.entries] == [0, 3, 5, 7, 11] and atlas.frames == list(range(N_FRAMES))
    st3 = fwd.track_stores[3]
    y, x = np.mgrid[8:128:16, 8:160:16]
    P = np.stack([x.ravel(), y.ravel()], axis=1).astype(np.float32)
    on6 = st3.query(P, [6])[:, 0, 0:2].contiguous()
    alone = TrackAtlas([(3, st3)])
    c1, o1, f1, t1 = alone.tracks_from(on6, 6)
    c2, o2, f2 = st3.tracks_from(on6, 6)
    assert np.array_equal(f1, f2) and np.array_equal(t1, np.where(f2, 3, -1)) and f2.any()
    assert np.array_equal(c1.view(np.int32), c2.view(np.int32)) and np.array_equal(o1.view(np.int32), o2.view(np.int32))
    # (a) the issue's bound, where the atlas follows P itself
    from test_trackstore import quant_bound
    ref = st3.tracks(P, frames=list(range(3, N_FRAMES)))[0]                          # [80, 9, 2]: frames 3 .. 11
    # per frame and coordinate, as tests/test_trackstore.py applies the documented bound to coordinates: the channel's bound plus the
    # fp32 rounding of the sums x + flow x themselves -- 1e-5 there, for coordinates below 128 (spacing 2^-17); these frames are 160
    # wide, so the spacing of coordinates below 256, 2^-16
    bound = 2.0 ** -16 + np.array([[quant_bound(st3.lohi(st3.slot_of(f))[c].cpu().numpy()) for c in (0, 1)] for f in range(3, N_FRAMES)])
    back = alone.locate(on6, 6)[0][:, 0:2].cpu().numpy()
    with np.errstate(invalid="ignore"):
        itself = f2 & (np.abs(back - P).max(axis=1) <= TOL)
    err = np.abs(c1[itself] - ref[itself])                                           # [n, 9, 2]
    print(f"template 3 alone: {int(f2.sum())} of {len(P)} found, {int(itself.sum())} located within {TOL:.3g} px of their grid point "
          f"(at most {np.abs(back - P).max(axis=1)[itself].max(initial=0.0):.3g} px); elsewhere up to {np.nanmax(np.abs(c1[f2] - ref[f2])):.3g} px from the grid's tracks")
    print("    max |tracks_from - stores[3].tracks| per frame 3..11 (x, y) / bound: " +
          ", ".join(f"{e[0]:.2g} {e[1]:.2g} / {b[0]:.2g} {b[1]:.2g}" for e, b in zip(err.max(axis=0), bound)))
    assert itself.sum() >= len(P) // 4
    assert (err <= bound[None]).all()
    coords, occl, found, template = atlas.tracks_from(on6, 6)
    # (b) ... and through the whole atlas, where template 3 wins such a point
    won = itself & (template == 3)
    with np.errstate(invalid="ignore"):
        won &= np.abs(atlas.locate(on6, 6)[0][:, 0:2].cpu().numpy() - P).max(axis=1) <= TOL
    print(f"    template 3 wins {int((template == 3).sum())} points in the whole atlas, {int(won.sum())} of them at their grid point")
    assert won.any() and (np.abs(coords[won][:, 3:] - ref[won]) <= bound[None]).all() and np.isnan(coords[template == 3][:, :3]).all()
    assert coords.shape == (len(P), N_FRAMES, 2) and found[f2].all()
    print(f"atlas: {int(found.sum())} of {len(P)} found, winners {dict(zip(*np.unique(template, return_counts=True)))}")
    Q = on6.cpu().numpy()
    err = np.abs(coords[found, 6] - Q[found]).max()
    print(f"    the track at frame 6 is within {err:.3g} px of the query")
    assert err <= TOL
    table, cell, entry = atlas.locate(on6, 6)
    for s in np.unique(template[found]):
        rows = np.flatnonzero(template == s)
        want = atlas.query(int(s), table[torch.from_numpy(rows).to(DEV)][:, 0:2]).cpu().numpy()
        covered = ~np.isnan(want[0, :, 0])
        assert np.array_equal(np.ascontiguousarray(coords[rows][:, covered]).view(np.int32),
                              np.ascontiguousarray(want[:, covered, 0:2]).view(np.int32))
        assert np.isnan(coords[rows][:, ~covered]).all() and (occl[rows][:, ~covered] == 1).all()
    dense = atlas.inverse(list(range(N_FRAMES)))[1] >= 0
    st0 = fwd.track_stores[0].inverse(list(range(N_FRAMES)))[1] >= 0
    share = [(float(a.float().mean()), float(b.float().mean())) for a, b in zip(st0, dense)]
    print("    found share per frame, template 0 alone / atlas: " + ", ".join(f"{a:.3f}/{b:.3f}" for a, b in share))
    assert (dense | ~st0).all() and all(b >= a for a, b in share)
    assert dense[0].all() and dense[11].all()                                        # a template's own frame is covered entirely
