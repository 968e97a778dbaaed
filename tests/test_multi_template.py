"""Host logic of the multi-template tracker (mft_amd/multi.py) with an oracle backend and a stub flow plugin -- the doubles of
tests/test_host_logic.py, restated: the lockstep pass gives every template exactly what a single MFT on that start frame gives,
and asks the flow plugin for the union of the templates' pairs only."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import mft_oracle as O

DELTAS = (np.inf, 1, 2, 4, 8, 16, 32)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


class OracleBackend:
    """No chain_select_multi: the pass falls back to chain_select per template."""

    @staticmethod
    def chain_select(Ls, Rs, thr):
        from mft_amd.MFT import is_packed, unpack_planes
        Rs = [unpack_planes(r) if is_packed(r) else r for r in Rs]
        f, o, s, idx = O.select([O.chain(l, r) for l, r in zip(Ls, Rs)], thr)
        return f, o, s, idx.to(torch.int8)


class StubFlower:
    def __init__(self):
        self.calls = []

    def compute_flow(self, src_img, dst_img, mode="flow", init_flow=None, **kw):
        l, r = gi.decode_id(src_img), gi.decode_id(dst_img)
        self.calls.append((l, r))
        flow, occl, sigma = gi.stub_flowou(l, r)
        return T(flow), {"occlusion": T(occl), "sigma": T(sigma), "debug": None}


def make_config(flower, deltas=DELTAS, **extra):
    from mft_amd.config import Config
    c = Config()
    c.deltas = list(deltas)
    c.occlusion_threshold = 0.02
    c.flow_config = Config()
    c.flow_config.of_class = lambda cfg: flower
    for k, v in extra.items():
        setattr(c, k, v)
    return c


def make_single(flower, **extra):
    from mft_amd.MFT import MFT
    return MFT(make_config(flower, keep_result_on_device=True, **extra), backend=OracleBackend(), device="cpu")


def make_multi(flower, **kw):
    from mft_amd.multi import MultiTemplateMFT
    return MultiTemplateMFT(make_config(flower), backend=OracleBackend(), device="cpu", **kw)


def frames_of(first, direction):
    return range(first, gi.SEQ_FRAMES) if direction > 0 else range(first, -1, -1)


def run_single(start, direction):
    """{frame: (result planes, last_pairs, memory keys, requested pairs)} of an MFT initialised on `start` alone."""
    fl = StubFlower()
    tr = make_single(fl)
    out = {}
    for k, f in enumerate(frames_of(start, direction)):
        fl.calls.clear()
        if k == 0:
            res = tr.init(gi.id_image(f), start_frame_i=start, time_direction=direction).result
        else:
            res = tr.track(gi.id_image(f)).result
        out[f] = (res.planes(), list(tr.last_pairs), sorted(tr.memory), list(fl.calls),
                  None if tr.last_chosen is None else tr.last_chosen.clone())
    return out


@pytest.mark.parametrize("starts,direction", [((0, 3, 5, 17), +1), ((43, 36), -1)])
def test_same_results_as_independent_trackers_and_fewer_pairs(starts, direction):
    singles = {s: run_single(s, direction) for s in starts}
    fl = StubFlower()
    mt = make_multi(fl)
    rng = np.random.default_rng(5)
    queries = {s: rng.uniform(-2, 70, size=(5, 2)).astype(np.float32) for s in starts[:-1]}     # (one template without queries)
    mt.init(starts, time_direction=direction, queries=queries, n_frames=gi.SEQ_FRAMES)
    first = min(starts) if direction > 0 else max(starts)
    saved_somewhere = False
    for f in frames_of(first, direction):
        fl.calls.clear()
        metas = mt.track(f, gi.id_image(f))
        active = [s for s in starts if (s <= f if direction > 0 else s >= f)]
        assert sorted(metas) == sorted(active)
        for s in active:
            planes, pairs, keys, _, chosen = singles[s][f]
            got = metas[s].result
            assert torch.equal(got.flow, planes[0]) and torch.equal(got.occlusion, planes[1]) and torch.equal(got.sigma, planes[2]), (s, f)
            t = mt.templates[s]
            assert t.last_pairs == pairs and sorted(t.memory) == keys, (s, f)
            assert (chosen is None and t.last_chosen is None) or torch.equal(t.last_chosen, chosen)
        # the plugin was asked for the union of the running templates' pairs, each once
        wanted = [p for s in active for p in singles[s][f][3]]
        assert len(fl.calls) == len(set(fl.calls)) and set(fl.calls) == set(wanted), f
        lefts = [l for l, _ in wanted]
        if len(lefts) != len(set(lefts)):                      # two running templates share a left frame
            assert len(fl.calls) < len(wanted), f
            saved_somewhere = True
    assert saved_somewhere
    assert mt.stats["pairs"] < sum(len(v[3]) for s in starts for v in singles[s].values())
    # the point read-out: every frame the template has seen, against the results API on the single tracker's result
    from mft_amd.point_tracking import convert_to_point_tracking
    from mft_amd.results import FlowOUTrackingResult
    tracks = mt.point_tracks()
    assert sorted(tracks) == sorted(queries)
    for s, (coords, occl) in tracks.items():
        assert coords.shape == (5, gi.SEQ_FRAMES, 2) and occl.shape == (5, gi.SEQ_FRAMES)
        for f, (planes, *_rest) in singles[s].items():
            c, o = convert_to_point_tracking(FlowOUTrackingResult(*planes, validate=False), queries[s])
            assert np.array_equal(coords[:, f], c) and np.array_equal(occl[:, f], o)
        assert np.array_equal(coords[:, s], queries[s]) and not occl[:, s].any()
        unseen = [f for f in range(gi.SEQ_FRAMES) if f not in singles[s]]
        assert not coords[:, unseen].any() and not occl[:, unseen].any()


def test_images_are_shared_between_the_rings():
    fl = StubFlower()
    mt = make_multi(fl)
    mt.init([0, 2])
    for f in range(6):
        mt.track(f, gi.id_image(f))
    a, b = mt.templates[0].memory, mt.templates[2].memory
    assert all(a[k]['img'] is b[k]['img'] for k in set(a) & set(b)) and set(a) & set(b)
    assert set(mt._imgs) == set(a) | set(b)


def test_documented_errors():
    from mft_amd.multi import MultiTemplateMFT
    fl = StubFlower()
    mt = make_multi(fl, max_templates=3)
    assert mt.max_templates == 3
    with pytest.raises(ValueError, match="max_templates"):
        mt.init([0, 1, 2, 3])
    mt.init([0, 1, 2, 2])                                       # three distinct start frames
    with pytest.raises(ValueError, match="out of order"):
        mt.track(1, gi.id_image(1))                             # the pass begins at the earliest start frame
    mt.track(0, gi.id_image(0))
    with pytest.raises(ValueError, match="out of order"):
        mt.track(2, gi.id_image(2))
    with pytest.raises(ValueError, match="out of order"):
        mt.track(0, gi.id_image(0))
    mt.track(1, gi.id_image(1))
    mt.init([5, 9], time_direction=-1)
    with pytest.raises(ValueError, match="out of order"):
        mt.track(5, gi.id_image(5))
    mt.track(9, gi.id_image(9))
    with pytest.raises(ValueError, match="flow cache"):
        mt.init([0], flow_cache=object())
    with pytest.raises(ValueError, match="n_frames"):
        mt.init([0], queries={0: np.zeros((2, 2), np.float32)})
    with pytest.raises(ValueError, match="no start frames"):
        mt.init([0], queries={4: np.zeros((2, 2), np.float32)}, n_frames=8)
    with pytest.raises(ValueError, match="no start frames"):
        mt.init([])
    sharded = MultiTemplateMFT(make_config(fl, delta_sharding=True), backend=OracleBackend(), device="cpu")
    with pytest.raises(ValueError, match="delta_sharding"):
        sharded.init([0])
    limited = MultiTemplateMFT(make_config(fl, multi_template_max=2), backend=OracleBackend(), device="cpu")
    with pytest.raises(ValueError, match="max_templates"):
        limited.init([0, 1, 2])
    with pytest.raises(NotImplementedError):
        mt.track_window([gi.id_image(0)])


def test_new_entry_points_are_declared_bound_and_exported():
    """include/mftx.h, _lib.SIGNATURES and both libraries carry the two new entry points; the package offers the class lazily."""
    import ctypes
    import re
    from pathlib import Path
    import mft_amd
    from mft_amd import _lib, ops
    repo = Path(__file__).resolve().parents[1]
    header = (repo / "include" / "mftx.h").read_text()
    for name in ("mftx_chain_select_multi", "mftx_sample_points"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
        variant = repo / "mft_amd" / "libmftx_lfwide.so"
        if variant.exists():
            assert hasattr(ctypes.CDLL(str(variant)), name)
    assert callable(ops.chain_select_multi) and callable(ops.sample_points)
    from mft_amd.multi import MultiTemplateMFT
    assert mft_amd.MultiTemplateMFT is MultiTemplateMFT
    assert _lib.load().mftx_version() == 400


def test_run_sequence_multi_equals_run_sequence_on_the_host():
    """The protocol runner on the doubles: one forward (+ one backward) lockstep pass gives run_sequence's tracklets, in groups of
    max_templates too."""
    from mft_amd import tapvid
    video = [gi.id_image(f) for f in range(20)]
    rng = np.random.default_rng(9)
    H, W = video[0].shape[:2]
    q = np.stack([rng.choice([0, 5, 10, 15], size=14), rng.integers(0, H, size=14), rng.integers(0, W, size=14)], axis=1)
    for mode in ("strided", "first"):
        want = tapvid.run_sequence(make_single(StubFlower()), video, q, mode)
        for group in (None, 3):
            fl = StubFlower()
            seen = []
            got = tapvid.run_sequence_multi(make_multi(fl), video, q, mode, max_templates=group,
                                            on_result=lambda s, d, f, r: seen.append((s, d, f)))
            assert got["tracks"].shape == want["tracks"].shape and got["occluded"].shape == want["occluded"].shape
            assert np.array_equal(got["tracks"], want["tracks"]) and np.array_equal(got["occluded"], want["occluded"])
            dirs = ("forward", "backward") if mode == "strided" else ("forward",)
            assert sorted(seen) == sorted((s, d, f) for s in (0, 5, 10, 15) for d in dirs
                                          for f in (range(s, 20) if d == "forward" else range(0, s + 1)))
