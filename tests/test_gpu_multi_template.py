"""The multi-template pass on the GPU (mft_amd/multi.py, mftx_chain_select_multi, mftx_sample_points): the kernels against
their single-template counterparts bit for bit and against the reference's own numbers, the tracker against independent MFT
runs bit for bit with the real engine, the TAP-Vid runner against the sequential protocol."""
import json
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_inputs as gi
from mft_amd import tapvid
from mft_amd.config import Config, load_config
from mft_amd.io import FlowCache
from mft_amd.synth import SyntheticVideo

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = __import__("pathlib").Path(__file__).resolve().parents[1]
THR = 0.02


def _rand_result(g, H, W, occluded=False):
    """In the manner of _rand_results of tests/test_gpu_kernels.py: flows of a few pixels (they leave the frame near the
    borders), occlusions on both sides of the 0.02 threshold (or all above it), positive sigmas."""
    occl = torch.rand(1, H, W, generator=g).mul(0.05)
    if occluded:
        occl = occl.add(0.5)
    return (torch.randn(2, H, W, generator=g).mul(3).to(DEV), occl.to(DEV), torch.rand(1, H, W, generator=g).add(0.1).to(DEV))


def _pack(planes):
    f, o, s = planes
    return torch.cat([f, o, s], 0).permute(1, 2, 0).contiguous()


def _templates(Ks, H, W, seed, all_occluded=()):
    """T templates of Ks[j] candidates: left operands of their own, right operands drawn from a shared pool (as the
    finite-delta pairs of a frame are shared) plus one of their own (the inf pair)."""
    g = torch.Generator().manual_seed(seed)
    pool = [_pack(_rand_result(g, H, W)) for _ in range(max(Ks))]
    out = []
    for j, K in enumerate(Ks):
        occ = j in all_occluded
        Ls = [_rand_result(g, H, W, occluded=occ) for _ in range(K)]
        Rs = [_pack(_rand_result(g, H, W))] + pool[: K - 1]
        out.append((Ls, Rs))
    return out


def _assert_multi_equals_single(ops, templates):
    got = ops.chain_select_multi(templates, THR, want_chosen=True)
    assert len(got) == len(templates)
    for j, ((Ls, Rs), g) in enumerate(zip(templates, got)):
        want = ops.chain_select_packed(Ls, Rs, THR, want_chosen=True)
        for name, a, b in zip(("flow", "occlusion", "sigma", "chosen"), g, want):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (j, len(Ls), name)
    return got


@pytest.mark.parametrize("H,W", [(128, 160), (125, 187)])
def test_chain_select_multi_bitwise(H, W):
    from mft_amd import ops
    tm = _templates([7, 4, 3, 1, 8, 5], H, W, seed=11, all_occluded=(5,))
    assert tm[0][1][1] is tm[1][1][1]                              # right operands shared between templates
    got = _assert_multi_equals_single(ops, tm)
    assert len({int(v) for v in got[0][3].unique()}) > 1           # the selection does choose
    assert bool((got[5][3] == 0).all()) and bool((got[4][1] == 1).any())   # all above the threshold: first candidate; flows leave the frame
    no_chosen = ops.chain_select_multi(tm, THR)
    assert all(c[3] is None and torch.equal(c[0], g[0]) for c, g in zip(no_chosen, got))
    # more templates than one launch's argument block holds (12), and the candidate-by-candidate variant (a K above 8: 6 per launch)
    _assert_multi_equals_single(ops, _templates([7, 4, 3, 1, 8, 2, 6, 5, 7, 7, 1, 3, 8, 4], H, W, seed=12))
    _assert_multi_equals_single(ops, _templates([9, 3, 16, 1, 8, 2, 7, 12], H, W, seed=13))


def test_chain_select_multi_argument_checks():
    from mft_amd import ops
    from mft_amd._lib import MftxError
    (Ls, Rs), = _templates([2], 16, 24, seed=1)
    with pytest.raises(MftxError):
        ops.chain_select_multi([(Ls, Rs[:1])], THR)
    with pytest.raises(MftxError):
        ops.chain_select_multi([(Ls, [Rs[0], Rs[1].reshape(-1)[1:-3].clone()])], THR)          # not [H, W, 4]
    flat = torch.zeros(16 * 24 * 4 + 4, device=DEV)
    with pytest.raises(MftxError, match="aligned"):
        ops.chain_select_multi([(Ls, [Rs[0], flat[1:-3].view(16, 24, 4)])], THR)              # 4 bytes off a 16-byte boundary
    with pytest.raises(MftxError):
        ops.chain_select_multi([(Ls * 9, Rs * 9)], THR)                                       # 18 candidates
    assert ops.chain_select_multi([], THR) == []


def test_sample_points_matches_reference(golden_dir):
    """Against tests/golden/results_api.npz -- outputs of the reference's own warp_forward_points / sample -- with the tolerances
    tests/test_results_api.py applies to the torch path; two templates in one call, points interleaved, a [N, frames, 4] table."""
    from mft_amd import ops
    g = np.load(golden_dir / "results_api.npz")
    d = gi.results_api_inputs()
    res = tuple(torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV) for k in ("flow", "occl", "sigma"))
    pts = torch.from_numpy(d["pts"]).to(DEV)
    n = len(pts)
    table = torch.full((n, 1, 4), -7.0, device=DEV)
    ops.sample_points([res], torch.zeros(n, dtype=torch.int32, device=DEV), pts, table, 0)
    out = table.cpu().numpy()[:, 0]
    assert np.allclose(out[:, :2], g["warp_forward_points"], atol=1e-5)
    assert np.allclose(out[:, 2], g["sample_occl"].reshape(-1), atol=1e-6)
    assert np.allclose(out[:, 3], g["sample_sigma"].reshape(-1), atol=1e-6)
    # two templates, interleaved points, one column of a [N, frames, 4] table; a point of a template that is not passed stays
    other = (res[0].flip(2).contiguous(), res[1].flip(1).contiguous(), res[2].mul(2).contiguous())
    tmpl = torch.tensor([0, 1] * n + [2], dtype=torch.int32, device=DEV)
    xy = torch.cat([pts.repeat_interleave(2, 0), pts[:1]])
    frames, col = 5, 3
    table = torch.full((2 * n + 1, frames, 4), -7.0, device=DEV)
    ops.sample_points([res, other], tmpl, xy, table, col)
    t = table.cpu().numpy()
    assert (t[:, [0, 1, 2, 4]] == -7.0).all() and (t[-1] == -7.0).all()
    assert np.array_equal(t[0:-1:2, col], out)
    single = torch.zeros((n, 4), device=DEV)
    ops.sample_points([other], torch.zeros(n, dtype=torch.int32, device=DEV), pts, single, 0)
    assert np.array_equal(t[1:-1:2, col], single.cpu().numpy())
    from mft_amd.results import FlowOUTrackingResult
    want = FlowOUTrackingResult(*other, validate=False).warp_forward_points(pts).cpu().numpy()
    assert np.allclose(t[1:-1:2, col, :2], want, atol=1e-5)
    from mft_amd._lib import MftxError
    with pytest.raises(MftxError):
        ops.sample_points([res], tmpl, xy, table, frames)                                    # column outside the table
    with pytest.raises(MftxError):
        ops.sample_points([res], tmpl[:3], xy, table, 0)


# ---------------------------------------------------------------------------
# tracker, real engine
# ---------------------------------------------------------------------------
def _config(deltas, iters, fif):
    conf = load_config(REPO / "configs" / "MFT_cfg.py")
    conf.flow_config.model = None
    conf.flow_config.synthetic_weights_seed = 0
    conf.flow_config.flow_iters = iters
    conf.flow_config.frames_in_flight = fif
    if deltas is not None:
        conf.deltas = list(deltas)
    conf.keep_result_on_device = True
    return conf


def _frames_of(first, n, direction):
    return range(first, n) if direction > 0 else range(first, -1, -1)


def _single_runs(conf, video, starts, direction):
    """{start: {frame: (flow, occl, sigma, chosen)}} of an MFT initialised on each start frame alone, no flow cache."""
    tracker = conf.tracker_class(conf)
    out = {}
    for s in starts:
        runs = out[s] = {}
        for k, f in enumerate(_frames_of(s, len(video), direction)):
            if k == 0:
                r = tracker.init(video[f], start_frame_i=s, time_direction=direction, flow_cache=None).result
                runs[f] = (r.flow.to(DEV), r.occlusion.to(DEV), r.sigma.to(DEV), None)
            else:
                r = tracker.track(video[f]).result
                runs[f] = (r.flow.clone(), r.occlusion.clone(), r.sigma.clone(), tracker.last_chosen.clone(), list(tracker.last_pairs))
    return out


def _check_pass(conf, video, starts, direction, want, pair_chunk=None):
    from mft_amd.multi import MultiTemplateMFT
    mt = MultiTemplateMFT(conf, pair_chunk=pair_chunk)
    mt.init(starts, time_direction=direction)
    first = min(starts) if direction > 0 else max(starts)
    pairs_per_frame = {}
    for f in _frames_of(first, len(video), direction):
        before = mt.stats["pairs"], mt.stats["engine_calls"]
        metas = mt.track(f, video[f])
        pairs_per_frame[f] = (mt.stats["pairs"] - before[0], mt.stats["engine_calls"] - before[1])
        assert sorted(metas) == sorted(s for s in starts if (s <= f if direction > 0 else s >= f))
        for s, meta in metas.items():
            w = want[s][f]
            r = meta.result
            assert r.flow.is_cuda
            assert torch.equal(r.flow, w[0]) and torch.equal(r.occlusion, w[1]) and torch.equal(r.sigma, w[2]), (s, f)
            if w[3] is not None:
                assert torch.equal(mt.templates[s].last_chosen, w[3]) and mt.templates[s].last_pairs == w[4], (s, f)
    assert mt.stats["chain_launches"] == sum(1 for f in pairs_per_frame if pairs_per_frame[f][0])
    return mt, pairs_per_frame


@pytest.mark.parametrize("fif", [1, 2])
def test_tracker_bitwise_vs_independent_trackers(fif):
    deltas = [np.inf, 1, 2, 4]
    video = SyntheticVideo(128, 160, n_frames=12, seed=21)
    conf = _config(deltas, 4, fif)
    want = _single_runs(conf, video, (0, 3, 5), +1)
    mt, pairs = _check_pass(conf, video, (0, 3, 5), +1, want)
    assert pairs[6] == (5, 1)               # lefts {0, 5, 4, 2} + {3, 5, 4} + {5}: five pairs instead of eight, one engine call
    assert [len(mt.templates[s].last_pairs) for s in (0, 3, 5)] == [4, 4, 4]
    want = _single_runs(conf, video, (11, 7), -1)
    _check_pass(conf, video, (11, 7), -1, want)


@pytest.mark.parametrize("fif", [1, 2])
def test_tracker_bitwise_512_chunked_engine_calls(fif):
    """512 x 512, the shipped seven deltas, 12 iterations (the tile-resident kernels run), the union of a frame's pairs split
    over several engine calls (pair_chunk = 2 instead of a stretch of video long enough to exceed 16 pairs)."""
    video = SyntheticVideo(512, 512, n_frames=11, seed=22)
    conf = _config(None, 12, fif)
    assert len(conf.deltas) == 7
    starts = (0, 2, 3)
    want = _single_runs(conf, video, starts, +1)
    mt, pairs = _check_pass(conf, video, starts, +1, want, pair_chunk=2)
    assert pairs[10] == (6, 3)              # lefts {9, 8, 6} shared, 2 (delta 8 of template 0, the start of template 2), 0, 3: three calls


# ---------------------------------------------------------------------------
# protocol
# ---------------------------------------------------------------------------
def _protocol_inputs(tmp_path, H, W, n_frames, scaling):
    vid = SyntheticVideo(H, W, n_frames=n_frames, seed=77)
    tapvid.synthetic_pickle(tmp_path / "synthetic.pkl", {"synth-a": vid}, n_tracks=14, seed=3)
    dconf = Config()
    dconf.pickles, dconf.scaling, dconf.name = [tmp_path / "synthetic.pkl"], scaling, "synthetic-" + scaling
    return dconf


@pytest.mark.parametrize("fif", [1, 2])
def test_run_sequence_multi_vs_run_sequence(tmp_path, fif):
    """Both sides read out bit-identical dense results and differ only in the fp32 operation order of one bilinear
    interpolation: EVERY coordinate within 1e-3 * 256 / W px, every occlusion score within 1e-4 (the bounds of
    tests/test_gpu_c3.py, with no share of points left out)."""
    from mft_amd.multi import MultiTemplateMFT
    dconf = _protocol_inputs(tmp_path, 128, 160, 12, "fullres")
    (el,) = list(tapvid.create_tapvid_dataset(dconf.pickles[0], ["first", "strided"], dconf.scaling))
    video = np.ascontiguousarray(el["data"]["first"]["video"][0][..., ::-1])
    H, W = video.shape[1:3]
    conf = _config([np.inf, 1, 2, 4], 4, fif)
    single = conf.tracker_class(conf)
    multi = MultiTemplateMFT(conf)
    for mode in ("strided", "first"):
        q = np.asarray(el["data"][mode]["query_points"])[0].astype(np.int64)
        cache = FlowCache(tmp_path / f"cache-{mode}", max_RAM_MB=1024, max_GPU_RAM_MB=4096, device=DEV)
        want = tapvid.run_sequence(single, video, q, mode, flow_cache=cache, device=DEV)
        for group in (None, 2):
            got = tapvid.run_sequence_multi(multi, video, q, mode, device=DEV, max_templates=group)
            assert got["tracks"].shape == want["tracks"].shape and got["occluded"].shape == want["occluded"].shape
            d = float(np.abs(got["tracks"] - want["tracks"]).max())
            do = float(np.abs(got["occluded"] - want["occluded"]).max())
            print(f"{mode} fif={fif} group={group}: max track difference {d:.3g} px (bound {1e-3 * 256 / W:.3g}), "
                  f"max occlusion difference {do:.3g} (bound 1e-4)")
            assert d <= 1e-3 * 256 / W, (mode, group, d)
            assert do <= 1e-4, (mode, group, do)
        if mode == "strided":
            assert multi.stats["readout_launches"] == multi.stats["frames"] and multi.stats["chain_launches"] <= multi.stats["frames"]


def test_run_dataset_multi_template_writes_the_same_files(tmp_path):
    dconf = _protocol_inputs(tmp_path, 128, 160, 8, "fullres")
    with open(dconf.pickles[0], "rb") as f:
        data = pickle.load(f)
    data["synth-a"]["occluded"][0, 0] = False                    # a track visible in frame 0: start frame 0 exists (write_flow)
    with open(dconf.pickles[0], "wb") as f:
        pickle.dump(data, f)
    conf = _config([np.inf, 1, 2], 4, 2)
    runs = {}
    for tag, multi in (("seq", False), ("multi", True)):
        done = tapvid.run_dataset(dconf, [conf], tmp_path / tag, tmp_path / ("cache-" + tag), mode="both", gpu_cache_limit=4,
                                  write_flow=True, multi_template=multi)
        assert [(d["mode"], d["skipped"]) for d in done] == [("first", False), ("strided", False)]
        runs[tag] = tapvid.evaluate_dataset(dconf, [conf], tmp_path / tag, mode="both", write=True)
    files = {tag: sorted(str(p.relative_to(tmp_path / tag)) for p in (tmp_path / tag).rglob("*") if p.is_file()) for tag in runs}
    assert files["seq"] == files["multi"] and any("flowous" in p for p in files["multi"])
    assert not (tmp_path / "cache-multi").exists()               # no flow cache is created
    for mode in ("first", "strided"):
        a, b = runs["seq"][mode][conf.name][0], runs["multi"][mode][conf.name][0]
        for k in a:
            if k != "seq":
                assert np.isclose(a[k], b[k], rtol=0, atol=1e-12, equal_nan=True), (mode, k, a[k], b[k])
    again = tapvid.run_dataset(dconf, [conf], tmp_path / "multi", tmp_path / "cache-multi", mode="both", cont=True, multi_template=True)
    assert all(d["skipped"] for d in again)


def test_run_MFT_tapvid_command_line_multi_template(tmp_path):
    """tools/run_MFT_tapvid.py --multi-template, the way test_run_MFT_tapvid_command_line (tests/test_gpu_c3.py) drives it."""
    out = subprocess.run([sys.executable, str(REPO / "tools" / "run_MFT_tapvid.py"), str(REPO / "dataset_configs" / "pkl-tapvid-davis-256x256_512x512.py"),
                          str(REPO / "configs" / "MFT_cfg.py"), "--synthetic", "1", "--synthetic-frames", "8", "--export", str(tmp_path / "e"),
                          "--cache", str(tmp_path / "c"), "--mode", "both", "--multi-template"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["scaling"] == "256x256_512x512" and d["results"] == 2 and d["skipped"] == 0 and d["multi_template"] is True
    assert sorted(d["metrics"]) == ["first", "strided"]
    m = d["metrics"]["strided"]["MFT_cfg"]
    assert 0.0 <= m["average_jaccard"] <= 1.0 and 0.0 <= m["occlusion_accuracy"] <= 1.0
    assert (tmp_path / "e" / "MFT_cfg" / "results" / "synth-00-first.pklz").exists()
    assert (tmp_path / "e" / "MFT_cfg" / "results" / "synth-00-strided.pklz").exists()
    assert (tmp_path / "e" / "MFT_cfg" / "eval" / "tapvid-eval.pklz").exists()
