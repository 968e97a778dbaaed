"""``TrackAtlas.best_results_from`` / ``best_result_from`` on the host (device="cpu"): the dense results from any video frame with the
template chosen per pixel AND destination frame -- every entry that holds the source frame inverts it by itself, follows its own
template point through its template's stores, chains, and the smallest (occluded, chained sigma, rank) wins.  No GPU needed; the
stores are those of tests/test_track_locate.py and tests/test_track_atlas.py.

``three_templates``, ``candidate_planes``, ``ambiguous`` and ``HOST_CASES`` are shared with tests/test_gpu_track_atlas_best.py."""
import functools

import numpy as np
import pytest
import torch

from mft_amd.results import FlowOUTrackingResult
from mft_amd.trackstore import chain_behind_inverse
from test_track_atlas import CH, CW, joined_atlas, two_template_stores
from test_track_atlas_flow import INF_BITS, NAN_BITS, ONE_BITS, assert_fill
from test_track_inverse import grid
from test_track_locate import bits, const_planes, field, make_store

THR = 0.5
HOST_CASES = [(13, 21, 1.5), (13, 21, 5.0), (24, 40, 1.5), (24, 40, 5.0), (37, 53, 5.0)]         # H, W, amp: device against host
AMBIGUITY = 1e-4                 # sigma of the two best, or an occlusion and the threshold, closer than this: either answer is right
AMBIGUOUS_CAP = 0.01             # ... which may be so for at most this share of the answered pixel-columns


def three_templates(H, W, amp=1.5, device="cpu"):
    """Forward-only templates plus one frame behind: template 0 over frames 0 .. 3, template 1 over 1, 2, 3 and 0, template 2 over
    2 and 3.  From frame 2 template 2 wins every pixel it sees (sigma 0 on its own frame) and covers neither frame 0 nor frame 1."""
    from mft_amd import TrackAtlas
    f = lambda seed: field(seed, H, W, amp)  # noqa: E731
    s0 = make_store(H, W, {0: const_planes(H, W), 1: f(11), 2: f(12), 3: f(14)}, device=device)
    s1 = make_store(H, W, {1: const_planes(H, W), 2: f(13), 3: f(15), 0: f(17)}, device=device)
    s2 = make_store(H, W, {2: const_planes(H, W), 3: f(16)}, device=device)
    return TrackAtlas([(0, s0), (1, s1), (2, s2)])


def key_of(o, s, rank, thr=THR):
    """The definition's key on numpy arrays (int64)."""
    o, s = np.asarray(o, np.float32), np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        occluded = ~(o <= np.float32(thr))
        fld = np.where(np.isnan(s), 0x7fffffff, np.where(s > 0, np.ascontiguousarray(s).view(np.int32), 0)).astype(np.int64)
    return (occluded.astype(np.int64) << 39) | (fld << 8) | np.asarray(rank, np.int64)


def candidate_planes(atlas, src, cols, thr=THR):
    """Per candidate of ``src`` its own chained answer, on the atlas's device -> (ranks, ok [E, T, N] bool, occlusion [E, T, N],
    sigma [E, T, N]): ``store.inverse``, ``atlas.query`` on the candidate's template, ``chain_behind_inverse``."""
    ranks = atlas._holders(src)
    N = atlas.H * atlas.W
    g = atlas.entries[0][1]._pixel_grid()
    oks, os_, ss = [], [], []
    for r in ranks:
        s, st = atlas.entries[r]
        table, cell = st.inverse(src, thr)
        tb, found = table.reshape(N, 4), cell.reshape(N) >= 0
        at = torch.where(found[:, None], tb[:, 0:2], torch.zeros((), device=tb.device))
        ok = found[:, None] & torch.tensor(atlas.covered(s, cols), dtype=torch.bool, device=tb.device)[None, :]
        _, o, sg = chain_behind_inverse(tb, atlas.query(s, at, cols), g, ok)
        oks.append(ok.t())
        os_.append(o)
        ss.append(sg)
    return ranks, torch.stack(oks), torch.stack(os_), torch.stack(ss)


def ambiguous(atlas, src, cols, thr=THR):
    """From the atlas's own (host) candidates alone -> (ambiguous [T, N] bool, answered [T, N] bool) as numpy: a pixel-column is
    ambiguous where the best and the second-best candidate agree in ``occluded`` and differ in sigma by less than AMBIGUITY, or
    where some candidate's chained occlusion is within AMBIGUITY of the threshold."""
    ranks, ok, o, s = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in candidate_planes(atlas, src, cols, thr))
    E = len(ranks)
    none = np.iinfo(np.int64).max
    key = np.where(ok, key_of(o, s, np.asarray(ranks)[:, None, None], thr), none)
    answered = ok.any(axis=0)
    with np.errstate(invalid="ignore"):
        near_thr = (ok & (np.abs(o - np.float32(thr)) < AMBIGUITY)).any(axis=0)
        close = np.zeros_like(answered)
        if E >= 2:
            order = np.argsort(key, axis=0)
            a, b = order[0][None], order[1][None]
            both = np.take_along_axis(ok, b, 0)[0]                                          # (the best is ok wherever anything is)
            oa, ob = (~(np.take_along_axis(o, i, 0)[0] <= np.float32(thr)) for i in (a, b))
            sa, sb = (np.take_along_axis(s, i, 0)[0] for i in (a, b))
            close = answered & both & (oa == ob) & ~(np.abs(sa - sb) >= AMBIGUITY)         # (a NaN or inf - inf difference: ambiguous)
    return (near_thr | close) & answered, answered


@functools.lru_cache(maxsize=None)
def host_case(H, W, amp):
    """-> (the host atlas, its best_results_from(2), ambiguous, answered): computed once, read by every test that needs it."""
    atlas = three_templates(H, W, amp)
    got = atlas.best_results_from(2)
    amb, answered = ambiguous(atlas, 2, atlas.frames)
    return atlas, got, amb, answered


# ---- 1. the brute force ------------------------------------------------------------------------------------------------------
def brute_force(atlas, src, cols, thr=THR):
    """The definition with a loop per pixel, column and candidate; selection in plain Python."""
    H, W, T = atlas.H, atlas.W, len(cols)
    N = H * W
    g = grid(H, W)
    ranks = [r for r, (_, st) in enumerate(atlas.entries) if src in st._slot_of]
    inv, reads = [], []
    for r in ranks:
        s, st = atlas.entries[r]
        table, cell = st.inverse(src, thr)
        tb, cl = table.numpy().reshape(N, 4), cell.numpy().reshape(N)
        at = np.where((cl >= 0)[:, None], tb[:, 0:2], np.float32(0)).astype(np.float32)
        per_col = []
        for f in cols:                                   # the template's stores joined: its lowest-ranked entry that holds the frame
            owner = next((o for t, o in atlas.entries if t == s and f in o._slot_of), None)
            per_col.append(None if owner is None else owner.query(torch.from_numpy(at), [f]).numpy()[:, 0])
        inv.append((tb, cl))
        reads.append(per_col)
    flow = np.full((T, 2, N), np.nan, np.float32)
    occl = np.ones((T, N), np.float32)
    sigma = np.full((T, N), np.inf, np.float32)
    entry = np.full((T, N), -1, np.int32)
    thr32 = np.float32(thr)
    with np.errstate(all="ignore"):
        for p in range(N):
            for t in range(T):
                best = None
                for k, r in enumerate(ranks):
                    tb, cl = inv[k]
                    q = reads[k][t]
                    if cl[p] < 0 or q is None:
                        continue
                    o_src, s_src, (qx, qy, o_dst, s_dst) = tb[p, 2], tb[p, 3], q[p]
                    fx, fy = np.float32(qx - g[p, 0]), np.float32(qy - g[p, 1])
                    o = o_src if np.isnan(o_src) else (o_dst if np.isnan(o_dst) else max(o_src, o_dst))
                    sg = np.float32(np.sqrt(np.float64(np.float32(np.float32(s_src * s_src) + np.float32(s_dst * s_dst)))))
                    fld = 0x7fffffff if np.isnan(sg) else (int(np.float32(sg).view(np.int32)) if sg > 0 else 0)
                    key = (0 if o <= thr32 else 1, fld, r)
                    if best is None or key < best[0]:
                        best = (key, fx, fy, o, sg, r)
                if best is not None:
                    flow[t, 0, p], flow[t, 1, p], occl[t, p], sigma[t, p], entry[t, p] = best[1:]
    tmpl_of = np.asarray([f for f, _ in atlas.entries], np.int32)
    template = np.where(entry >= 0, tmpl_of[entry.clip(0)], -1).astype(np.int32)
    return flow.reshape(T, 2, H, W), occl.reshape(T, 1, H, W), sigma.reshape(T, 1, H, W), entry.reshape(T, H, W), template.reshape(T, H, W)


def assert_same_best(got, want):
    """got: the five tensors of ``best_results_from``; want: five numpy arrays.  Bits where the expected value is no NaN, NaN-ness
    elsewhere; entry and template equal."""
    for g, w in zip(got[:3], want[:3]):
        g = g.detach().cpu().numpy()
        assert g.shape == w.shape and g.dtype == np.float32
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan])
    for g, w in zip(got[3:], want[3:]):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("H,W", [(2, 2), (9, 34), (13, 21)])
def test_equals_the_brute_force_bit_for_bit(H, W):
    atlas = three_templates(H, W, 5.0 if (H, W) == (13, 21) else 1.5)
    for src, cols in ((2, None), (3, [0, 3, 1]), (0, [2, 2, 0]), (1, [3])):
        cols = atlas.frames if cols is None else cols
        got = atlas.best_results_from(src, cols)
        assert got[0].shape == (len(cols), 2, H, W) and got[3].shape == (len(cols), H, W) and got[4].shape == (len(cols), H, W)
        assert_same_best(got, brute_force(atlas, src, cols))
    # a joined template (forward and backward store of template 5) next to another template
    joined = joined_atlas()[0]
    for src in (6, 4):
        assert_same_best(joined.best_results_from(src), brute_force(joined, src, joined.frames))


# ---- 2. forward-only templates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(13, 21), (24, 40)])
def test_forward_only_templates_answer_backward_columns(H, W):
    atlas, (flow, occl, sigma, entry, template), amb, answered = host_case(H, W, 1.5)
    assert atlas.frames == [0, 1, 2, 3]
    old = atlas.results_from(2)
    assert_fill(old[0][0:2], old[1][0:2], old[2][0:2], np.ones((2, H, W), bool))          # today: frames 0 and 1 are all fill
    entry, template = entry.numpy(), template.numpy()
    fill = entry < 0
    assert np.array_equal(fill, bits(flow)[:, 0] == NAN_BITS) and np.array_equal(fill, template < 0)
    assert_fill(flow, occl, sigma, fill)
    won = [int((entry == r).sum()) for r in range(3)]
    print(f"{H}x{W}: fill {fill.mean():.3%} of the pixel-columns (results_from: {np.isnan(old[0][:, 0].numpy()).mean():.3%}); "
          f"candidates win {won}")
    assert fill.mean() < 0.10
    assert min(won) > 0                                                                  # every candidate wins somewhere
    assert np.array_equal(template[entry >= 0], entry[entry >= 0])                       # (template k is rank k here)
    assert np.array_equal(answered.reshape(entry.shape), ~fill)


@pytest.mark.parametrize("H,W,amp", HOST_CASES)
def test_inputs_of_the_device_comparison_are_rarely_ambiguous(H, W, amp):
    _, got, amb, answered = host_case(H, W, amp)
    share = amb.sum() / answered.sum()
    print(f"{H}x{W} amp {amp}: {int(amb.sum())} of {int(answered.sum())} answered pixel-columns are ambiguous ({share:.3%})")
    assert answered.sum() > 0.5 * answered.size and share <= AMBIGUOUS_CAP
    assert len({int(r) for r in np.unique(got[3].numpy()) if r >= 0}) == 3


# ---- 3. the two properties ---------------------------------------------------------------------------------------------------
def test_a_single_holder_equals_results_from():
    from mft_amd import TrackAtlas
    s0, s1 = two_template_stores(amp=5.0)
    atlas = TrackAtlas([(0, s0), (1, s1)])
    assert atlas._holders(0) == [0]
    for cols in (None, [2, 0, 7]):                                                       # (7: nobody's)
        got, want = atlas.best_results_from(0, cols), atlas.results_from(0, cols)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(bits(g), bits(w))
        cov = np.asarray(atlas.covered(0, cols))
        found = want[3].numpy()
        assert np.array_equal(got[3].numpy(), np.where(cov[:, None, None] & found[None], 0, -1))
        assert np.array_equal(got[4].numpy(), np.where(cov[:, None, None] & found[None], 0, -1))
    # one entry altogether: DenseTrackStore.results_from
    st = make_store(13, 21, {0: const_planes(13, 21), 1: field(3, 13, 21, 5.0), 2: field(4, 13, 21, 1.5)})
    got, want = TrackAtlas([(0, st)]).best_results_from(1), st.results_from(1)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got[:3], want[:3]))
    assert np.array_equal(got[3].numpy() >= 0, np.broadcast_to(want[3].numpy(), (3, 13, 21))) and not want[3].all()


@pytest.mark.parametrize("H,W,amp", [(13, 21, 1.5), (24, 40, 5.0)])
def test_never_worse_than_results_from(H, W, amp):
    atlas = three_templates(H, W, amp)
    for src in (1, 2, 3):
        flow, occl, sigma, entry, _ = (t.numpy() for t in atlas.best_results_from(src))
        oflow, ooccl, osigma, _, _ = (t.numpy() for t in atlas.results_from(src))
        rank = atlas.inverse(src)[2].numpy()
        answered = bits(oflow)[:, 0] != NAN_BITS                                          # found, and the winner's template covers it
        assert answered.any() and (entry[answered] >= 0).all()
        new = key_of(occl[:, 0], sigma[:, 0], entry.clip(0))
        old = key_of(ooccl[:, 0], osigma[:, 0], np.broadcast_to(rank.clip(0), entry.shape))
        assert (new[answered] <= old[answered]).all()
        print(f"{H}x{W} amp {amp} from {src}: results_from answers {answered.mean():.1%}, best_results_from {(entry >= 0).mean():.1%}; "
              f"another winner on {(new[answered] < old[answered]).mean():.1%} of the common ones")


# ---- 4. the key's corners, on exact inputs -----------------------------------------------------------------------------------
def corner_store(k, occl=0.0, sigma=0.0, device="cpu"):
    """Template 10 + k: frame 1 (the source) has zero flow and constant occlusion and sigma, frame 2 (the column) zero flow,
    occlusion 0 and sigma 0 -- the chained occlusion is the source's, the chained sigma sqrt(sigma^2 + 0)."""
    return make_store(CH, CW, {10 + k: const_planes(CH, CW), 1: const_planes(CH, CW, occl=occl, sigma=sigma), 2: const_planes(CH, CW)},
                      device=device)


def set_range(st, channel, value):
    """The stored frame 1's channel set to a constant through its (min, max) table (the words are 0)."""
    st.lohi(st.slot_of(1))[channel] = torch.tensor([value, value])
    return st


def corner_winner(stores, thr=THR):
    from mft_amd import TrackAtlas
    atlas = TrackAtlas([(10 + k, st) for k, st in enumerate(stores)])
    flow, occl, sigma, entry, template = atlas.best_results_from(1, [2], thr)
    e = np.unique(entry.numpy())
    assert e.size == 1 and e[0] >= 0 and (template.numpy() == 10 + e[0]).all() and float(np.abs(flow.numpy()).max()) <= 2.0 ** -18
    return int(e[0]), occl.numpy(), sigma.numpy()


def test_key_corners():
    w, o, s = corner_winner([corner_store(0, occl=0.9, sigma=0.125), corner_store(1, occl=0.0, sigma=4.0)])
    assert w == 1 and (o == 0).all() and (s == 4).all()                                  # visible beats occluded whatever the sigma
    w, o, s = corner_winner([corner_store(0, occl=0.9, sigma=0.125), corner_store(1, occl=0.0, sigma=4.0)], thr=1.0)
    assert w == 0 and (o == np.float32(0.9)).all() and (s == 0.125).all()                # neither occluded: the lower sigma
    assert corner_winner([corner_store(0, sigma=0.5), corner_store(1, sigma=0.25), corner_store(2, sigma=0.375)])[0] == 1
    assert corner_winner([corner_store(0, sigma=0.25), corner_store(1, sigma=0.25)])[0] == 0      # equal sigma: the lower rank
    nan = lambda k: set_range(corner_store(k), 3, float("nan"))  # noqa: E731
    huge = lambda k: set_range(corner_store(k), 3, 3.0e38)  # noqa: E731  (its square is +inf in float32)
    w, o, s = corner_winner([nan(0), huge(1)])
    assert w == 1 and (bits(s) == INF_BITS).all()                                        # a NaN sigma loses to +inf ...
    w, o, s = corner_winner([huge(0), corner_store(1, sigma=1000.0)])
    assert w == 1 and (s == 1000).all()                                                  # ... which loses to a number
    w, o, s = corner_winner([nan(0), corner_store(1, sigma=1000.0)])
    assert w == 1
    w, o, s = corner_winner([nan(0)])
    assert w == 0 and np.isnan(s).all()                                                  # alone it is the answer
    # a NaN occlusion counts as occluded: it loses to a visible candidate of any sigma, and ranks by sigma among the occluded
    nan_occl = lambda k, sigma: set_range(corner_store(k, sigma=sigma), 2, float("nan"))  # noqa: E731
    assert corner_winner([nan_occl(0, 0.125), corner_store(1, occl=0.0, sigma=4.0)])[0] == 1
    w, o, s = corner_winner([corner_store(0, occl=0.9, sigma=4.0), nan_occl(1, 0.125)])
    assert w == 1 and np.isnan(o).all() and (s == 0.125).all()
    assert corner_winner([corner_store(0, occl=0.9, sigma=0.125), nan_occl(1, 4.0)])[0] == 0
    # the only candidate that covers the column is occluded: an answer, not the fill
    from mft_amd import TrackAtlas
    lone = make_store(CH, CW, {20: const_planes(CH, CW), 1: const_planes(CH, CW, sigma=0.125)})      # visible, but it has no frame 2
    atlas = TrackAtlas([(10, corner_store(0, occl=0.9, sigma=4.0)), (20, lone)])
    flow, occl, sigma, entry, template = atlas.best_results_from(1, [2, 20])
    assert (entry[0] == 0).all() and (template[0] == 10).all() and (occl[0].numpy() == np.float32(0.9)).all() and (sigma[0] == 4).all()
    assert (entry[1] == 1).all() and (template[1] == 20).all() and (sigma[1] == 0.125).all()
    old = atlas.results_from(1, [2])                                                     # (the per-pixel rule follows `lone` into the fill)
    assert (old[4] == 20).all() and (bits(old[0]) == NAN_BITS).all()


# ---- 5. arguments ------------------------------------------------------------------------------------------------------------
def test_interface_out_and_documented_errors():
    atlas = three_templates(13, 21)
    H, W = 13, 21
    want = atlas.best_results_from(2, [1, 0])
    big = [torch.full((4, c, H, W), -7.0) for c in (2, 1, 1)]
    out = tuple(b[1:3] for b in big)
    got = atlas.best_results_from(2, [1, 0], out=out)
    assert all(g is o for g, o in zip(got[:3], out))
    for g, w, b in zip(got[:3], want[:3], big):
        assert np.array_equal(bits(g), bits(w)) and (b[0] == -7).all() and (b[3] == -7).all()
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4]) and got[3].dtype == torch.int32 and got[4].dtype == torch.int32
    # repeats and no order; an empty list; a column nobody covers
    rep = atlas.best_results_from(2, [0, 3, 0, 1])
    for g, w in zip(rep, want):
        assert np.array_equal(bits(g[0]), bits(w[1])) and np.array_equal(bits(g[2]), bits(w[1])) and np.array_equal(bits(g[3]), bits(w[0]))
    e = atlas.best_results_from(2, [])
    assert e[0].shape == (0, 2, H, W) and e[1].shape == (0, 1, H, W) and e[3].shape == (0, H, W) and e[4].shape == (0, H, W)
    u = atlas.best_results_from(2, [7, 1])
    assert_fill(u[0][0:1], u[1][0:1], u[2][0:1], np.ones((1, H, W), bool))
    assert (u[3][0] == -1).all() and (u[4][0] == -1).all() and torch.equal(u[3][1], want[3][0])
    # one column as a result
    r, found, template = atlas.best_result_from(2, 1)
    assert isinstance(r, FlowOUTrackingResult) and (r.H, r.W) == (H, W) and found.dtype == torch.bool and found.shape == (H, W)
    assert np.array_equal(bits(r.flow), bits(want[0][0])) and np.array_equal(bits(r.occlusion), bits(want[1][0]))
    assert np.array_equal(bits(r.sigma), bits(want[2][0])) and torch.equal(found, want[3][0] >= 0) and torch.equal(template, want[4][0])
    # the threshold is the inverses' and the key's
    low = atlas.best_results_from(2, [1, 0], occlusion_threshold=0.05)
    assert_same_best(low, brute_force(atlas, 2, [1, 0], 0.05))
    assert not torch.equal(low[3], want[3])
    for call in (lambda: atlas.best_results_from(7), lambda: atlas.best_results_from(7, [1]), lambda: atlas.best_result_from(7, 1),
                 lambda: atlas.best_result_from(1, 7)):
        with pytest.raises(KeyError):
            call()
    ok = lambda: [torch.zeros(2, 2, H, W), torch.zeros(2, 1, H, W), torch.zeros(2, 1, H, W)]  # noqa: E731
    bad = []
    for i, t in ((0, torch.zeros(2, 1, H, W)), (1, torch.zeros(2, H, W)), (2, torch.zeros(2, 1, H, W, dtype=torch.float64)),
                 (1, torch.zeros(3, 1, H, W)), (0, torch.zeros(2, 2, H, 2 * W)[..., ::2]), (2, np.zeros((2, 1, H, W), np.float32))):
        o = ok()
        o[i] = t
        bad.append(o)
    bad.append(ok()[:2])
    for o in bad:
        with pytest.raises(ValueError):
            atlas.best_results_from(2, [1, 0], out=o)
    with pytest.raises(KeyError):
        atlas.best_results_from(7, [1, 0], out=bad[0])                                 # the KeyError comes first
    # results_from is what it was
    old = atlas.results_from(2, [1, 0])
    assert (bits(old[0]) == NAN_BITS).all() and (bits(old[1]) == ONE_BITS).all()


# ---- 6. plumbing -------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_exported_and_checks_its_arguments():
    import ctypes
    import re
    from pathlib import Path
    from mft_amd import _lib, atlas_ops
    repo = Path(__file__).resolve().parents[1]
    name = "mftx_trackstore_flow_from_best"
    assert re.search(r"\b%s\s*\(" % name, (repo / "include" / "mftx.h").read_text()) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, name)
    variant = repo / "mft_amd" / "libmftx_lfwide.so"
    if variant.exists():
        assert hasattr(ctypes.CDLL(str(variant)), name)
    assert callable(atlas_ops.trackstore_flow_from_best) and atlas_ops.TRACKSTORE_BEST_COLUMNS == 16
    fb = lib.mftx_trackstore_flow_from_best
    buf = (ctypes.c_double * 8)()                                                     # host memory: only its address is looked at
    a = ctypes.addressof(buf)
    a16 = a if a % 16 == 0 else a + 8

    def call(tables=a16, cells=a, rank_of=a, row_of=a, frames=a, lohis=a, E=1, R=1, T=1, H=8, W=8, cpb=0, flow=a, occl=a, sigma=a, entry=a):
        return fb(tables, cells, rank_of, row_of, frames, lohis, E, R, T, H, W, 0.5, cpb, flow, occl, sigma, entry, None)

    err = lib.mftx_last_error_string
    assert call(T=0) == 0 and call(T=0, tables=None, flow=None) == 0                  # no columns: a no-op
    assert call(T=-1) == -1 and b"trackstore_flow_from_best" in err()
    assert call(E=-1) == -1 and call(E=257) == -1 and b"256" in err()
    assert call(H=1) == -1 and call(W=1) == -1 and call(cpb=-1) == -1 and call(R=0) == -1
    for arg in ("tables", "cells", "rank_of", "row_of", "frames", "lohis", "flow", "occl", "sigma", "entry"):
        assert call(**{arg: None}) == -1 and err().endswith(b"null pointer: " + arg.encode()), arg
    for arg in ("flow", "occl", "sigma", "entry"):                                    # without candidates only the results are needed
        assert call(E=0, tables=None, cells=None, rank_of=None, row_of=None, frames=None, lohis=None, **{arg: None}) == -1, arg
    assert call(H=65536, W=32768) == -1 and b"2^31" in err()
    assert call(T=65536 * 2, cpb=1) == -1 and b"column blocks" in err()
    assert call(tables=a16 + 8) == -2 and b"tables must be 16-byte aligned" in err()
    assert call(frames=a + 4) == -2 and b"frames" in err() and call(lohis=a + 4) == -2
    for arg in ("cells", "rank_of", "row_of", "flow", "occl", "sigma", "entry"):
        assert call(**{arg: a + 2}) == -2 and (arg.encode() + b" must be 4-byte aligned") in err(), arg
