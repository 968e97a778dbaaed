"""The dense track store (mft_amd/trackstore.py) on the host: its device="cpu" restatement against the reference's own codec
and read-out goldens, the store's bookkeeping, the declarations of the native entry points, and the tracker with
``config.track_store`` on the host doubles of tests/test_multi_template.py (restated here).  No GPU needed."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import mft_oracle as O

DELTAS = (np.inf, 1, 2, 4, 8, 16, 32)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def quant_bound(lohi_c):
    """What quantising a channel to uint16 and back may move a value -- and, bilinear sampling being a convex combination, a
    sampled value -- by: half a step, 0.01 of a step for the fp32 rounding of u * 65535 at the rounding boundary, and 2^-21
    of the channel's magnitude for the fp32 roundings of the decoder and the sampler."""
    lo, hi = float(lohi_c[0]), float(lohi_c[1])
    return 0.51 * (hi - lo) / 65535 + 2.0 ** -21 * max(abs(lo), abs(hi))


def cpu_store(H, W, **kw):
    from mft_amd.trackstore import DenseTrackStore
    return DenseTrackStore(H, W, device="cpu", **kw)


# ---- codec pin ---------------------------------------------------------------------------------------------------------------
def test_append_and_result_match_the_reference_codec_golden(golden_dir):
    g = np.load(golden_dir / "codec.npz")
    d = gi.codec_inputs()
    st = cpu_store(37, 53)
    assert st.append((T(d["flow"]), T(d["occl"]), T(d["sigma"]))) == 0 and len(st) == 1 and st.frame_ids == [0]
    assert np.array_equal(st.lohi(0).numpy(), g["lohi"])
    want_q = g["bgr"][..., 1].astype(np.uint16) * 256 + g["bgr"][..., 2]          # [4, H, W]
    got_q = st.packed(0).numpy()
    assert got_q.dtype == np.uint16 and got_q.shape == (37, 53, 4)
    for c in range(4):
        assert np.array_equal(got_q[..., c], want_q[c]), c
    assert not got_q[..., 3].any()                                               # the flat channel
    r = st.result(0)
    assert np.array_equal(r.flow.numpy(), g["dec_flow"]) and np.array_equal(r.occlusion.numpy(), g["dec_occl"])
    assert np.array_equal(r.sigma.numpy(), g["dec_sigma"])
    # a FlowOUTrackingResult is taken as well, and the codec is the oracle's
    from mft_amd.results import FlowOUTrackingResult
    from mft_amd.trackstore import compress_channel, decompress_channel
    st2 = cpu_store(37, 53)
    st2.append(FlowOUTrackingResult(T(d["flow"]), T(d["occl"]), T(d["sigma"])), frame_i=5)
    assert st2.frame_ids == [5] and st2.slot_of(5) == 0 and np.array_equal(st2.packed(0).numpy(), got_q)
    x = np.random.default_rng(0).normal(0, 30, size=(9, 11)).astype(np.float32)
    q, lo, hi = compress_channel(x)
    oq, olo, ohi = O.quantize_u16(x)
    assert np.array_equal(q, oq) and lo == olo and hi == ohi
    assert np.array_equal(decompress_channel(q, lo, hi), O.dequantize_u16(oq, olo, ohi))


# ---- query against the reference's own read-out ------------------------------------------------------------------------------
def test_query_matches_reference_readout_within_the_quantisation_bound(golden_dir):
    g = np.load(golden_dir / "results_api.npz")
    d = gi.results_api_inputs()
    st = cpu_store(40, 56)
    st.append((T(d["flow"]), T(d["occl"]), T(d["sigma"])), frame_i=3)
    table = st.query(d["pts"])
    assert table.shape == (7, 1, 4) and table.dtype == torch.float32
    table = table.numpy()[:, 0]
    b = [quant_bound(st.lohi(0)[c]) for c in range(4)]
    assert b[0] < 1e-3 and b[2] < 1e-5                                            # a real bound, not a loose one
    assert np.abs(table[:, 0] - g["warp_forward_points"][:, 0]).max() <= 1e-5 + b[0]
    assert np.abs(table[:, 1] - g["warp_forward_points"][:, 1]).max() <= 1e-5 + b[1]
    assert np.abs(table[:, 2] - g["sample_occl"][0]).max() <= 1e-6 + b[2]
    assert np.abs(table[:, 3] - g["sample_sigma"][0]).max() <= 1e-6 + b[3]
    coords, occl = st.tracks(d["pts"], frames=[3])
    assert coords.shape == (7, 1, 2) and occl.shape == (7, 1)
    assert np.array_equal(coords[:, 0], table[:, 0:2]) and np.array_equal(occl[:, 0], table[:, 2])
    # the out-of-frame taps are zeros, not the channel's minimum: sigma >= 0.2 everywhere, and a point 2 px left of the frame
    # sees nothing of it
    assert st.lohi(0)[3, 0] >= 0.2 and table[3, 3] == 0.0 and table[3, 2] == 0.0


# ---- store behaviour ---------------------------------------------------------------------------------------------------------
def seq_planes(f, H=24, W=40):
    flow, occl, sigma = gi.stub_flowou(0, f, H, W)
    return T(flow), T(occl), T(sigma)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_nine_frames_in_chunks_of_four(order):
    from mft_amd.point_tracking import convert_to_point_tracking
    H, W = 24, 40
    frames = list(range(10, 19)) if order == "ascending" else list(range(18, 9, -1))
    st = cpu_store(H, W, frames_per_chunk=4)
    for k, f in enumerate(frames):
        assert st.append(seq_planes(f, H, W), f) == k
    assert len(st) == 9 and st.frame_ids == frames and [st.slot_of(f) for f in frames] == list(range(9))
    assert st.nbytes == 3 * 4 * (H * W * 8 + 32)                                   # three chunks of four
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-3, 44, size=(20, 2)), [[0, 0], [39, 23], [5, 7], [-1, -1], [39.5, 23.5]]]).astype(np.float32)
    full = st.query(pts)
    assert full.shape == (len(pts), 9, 4)
    for k, f in enumerate(frames):                                                 # column k is frame frames[k]: the results API
        r = st.result(f)                                                           # on the quantise-then-dequantise result
        c, o = convert_to_point_tracking(r, pts)
        assert np.array_equal(full[:, k, 0:2].numpy(), c) and np.array_equal(full[:, k, 2].numpy(), o)
        q = [O.quantize_u16(p) for p in (lambda t: (t[0][0].numpy(), t[0][1].numpy(), t[1][0].numpy(), t[2][0].numpy()))(seq_planes(f, H, W))]
        want = [O.dequantize_u16(*e) for e in q]
        assert np.array_equal(r.flow.numpy(), np.stack(want[0:2])) and np.array_equal(r.occlusion.numpy()[0], want[2])
        assert np.array_equal(r.sigma.numpy()[0], want[3])
    for sel in ([frames[7], frames[0], frames[4]], frames[::-1], [frames[2]], frames[3:8]):
        got = st.query(pts, frames=sel)
        assert got.shape == (len(pts), len(sel), 4)
        assert torch.equal(got, full[:, [frames.index(f) for f in sel]])
    out = torch.full((len(pts), 2, 4), -7.0)
    assert st.query(pts, frames=frames[1:3], out=out) is out and torch.equal(out, full[:, 1:3])
    assert st.query(pts, frames=[]).shape == (len(pts), 0, 4) and st.query(np.zeros((0, 2), np.float32)).shape == (0, 9, 4)


def test_documented_errors():
    H, W = 24, 40
    st = cpu_store(H, W, frames_per_chunk=4, max_bytes=2 * 4 * (H * W * 8 + 32))
    for f in range(8):
        st.append(seq_planes(f, H, W), f)
    with pytest.raises(ValueError, match="stored already"):
        st.append(seq_planes(3, H, W), 3)
    with pytest.raises(MemoryError, match="max_bytes"):
        st.append(seq_planes(8, H, W), 8)                                          # a third chunk
    assert len(st) == 8 and st.frame_ids == list(range(8)) and st.nbytes == 2 * 4 * (H * W * 8 + 32)
    with pytest.raises(KeyError):
        st.query(np.zeros((1, 2), np.float32), frames=[2, 8])
    with pytest.raises(KeyError):
        st.result(-1)
    with pytest.raises(KeyError):
        st.slot_of(99)
    with pytest.raises(IndexError):
        st.packed(8)
    with pytest.raises(ValueError):
        st.append((torch.zeros(2, H, W + 1), torch.zeros(1, H, W + 1), torch.zeros(1, H, W + 1)), 20)
    with pytest.raises(ValueError):
        cpu_store(1, 5)


# ---- declarations ------------------------------------------------------------------------------------------------------------
NEW = ("mftx_trackstore_workspace_bytes", "mftx_trackstore_append", "mftx_trackstore_query", "mftx_trackstore_unpack")


def test_entry_points_are_declared_bound_and_exported():
    import ctypes
    import re
    from pathlib import Path
    from mft_amd import _lib, ops
    repo = Path(__file__).resolve().parents[1]
    header = (repo / "include" / "mftx.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
        variant = repo / "mft_amd" / "libmftx_lfwide.so"
        if variant.exists():
            assert hasattr(ctypes.CDLL(str(variant)), name), name
    assert _lib.load().mftx_version() == 400
    assert _lib.load().mftx_trackstore_workspace_bytes() >= 8 * 4
    assert callable(ops.trackstore_append) and callable(ops.trackstore_query) and callable(ops.trackstore_unpack)
    mk = (repo / "mft_amd" / "csrc" / "Makefile").read_text()
    rule = re.search(r"^trackstore\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) (.*?) -c \$< -o \$@", mk, re.M)
    assert rule, "no Makefile rule for trackstore.o"
    for flag in ("-ffp-contract=off", "-fno-slp-vectorize", "$(NOPK)"):
        assert flag in rule.group(1).split(), flag
    assert re.search(r"^OBJS\s*:=.*\btrackstore\.o\b", mk, re.M)
    tune = (repo / "tools" / "build_tuning.sh").read_text()
    assert '"trackstore.hip|trackstore.o|-ffp-contract=off -fno-slp-vectorize $NOPK"' in tune
    # argument checks that need no device: they come before anything is launched
    lib = _lib.load()
    assert lib.mftx_trackstore_append(None, None, None, 8, 8, None, None, None, 0, None) == -1
    assert b"trackstore_append" in lib.mftx_last_error_string()
    assert lib.mftx_trackstore_unpack(None, None, 8, 8, None, None, None, None) == -1
    assert lib.mftx_trackstore_query(None, None, 1, 4, None, -1, 8, 8, 1, None, None, 4, 0, None) == -1
    assert lib.mftx_trackstore_query(None, None, 1, 4, None, 3, 1, 8, 1, None, None, 12, 0, None) == -1      # H < 2
    assert lib.mftx_trackstore_query(None, None, 1, 4, None, 0, 8, 8, 5, None, None, 4, 0, None) == 0        # T == 0: a no-op
    assert lib.mftx_trackstore_query(None, None, 1, 4, None, 5, 8, 8, 0, None, None, 4, 0, None) == 0        # N == 0


# ---- tracker on the host doubles ---------------------------------------------------------------------------------------------
class OracleBackend:
    @staticmethod
    def chain_select(Ls, Rs, thr):
        from mft_amd.MFT import is_packed, unpack_planes
        Rs = [unpack_planes(r) if is_packed(r) else r for r in Rs]
        f, o, s, idx = O.select([O.chain(l, r) for l, r in zip(Ls, Rs)], thr)
        return f, o, s, idx.to(torch.int8)


class StubFlower:
    def compute_flow(self, src_img, dst_img, mode="flow", init_flow=None, **kw):
        flow, occl, sigma = gi.stub_flowou(gi.decode_id(src_img), gi.decode_id(dst_img))
        return T(flow), {"occlusion": T(occl), "sigma": T(sigma), "debug": None}


def make_config(deltas=DELTAS, **extra):
    from mft_amd.config import Config
    c = Config()
    c.deltas = list(deltas)
    c.occlusion_threshold = 0.02
    c.flow_config = Config()
    flower = StubFlower()
    c.flow_config.of_class = lambda cfg: flower
    for k, v in extra.items():
        setattr(c, k, v)
    return c


def run_tracker(frames, direction, **extra):
    from mft_amd.MFT import MFT
    tr = MFT(make_config(keep_result_on_device=True, **extra), backend=OracleBackend(), device="cpu")
    out = {}
    for k, f in enumerate(frames):
        if k == 0:
            res = tr.init(gi.id_image(f), start_frame_i=f, time_direction=direction).result
        else:
            res = tr.track(gi.id_image(f)).result
        out[f] = tuple(p.clone() for p in res.planes())
    return tr, out


@pytest.mark.parametrize("direction", [+1, -1])
def test_tracker_with_track_store_on_the_host_doubles(direction):
    from mft_amd.point_tracking import convert_to_point_tracking
    from mft_amd.results import FlowOUTrackingResult
    from mft_amd.trackstore import DenseTrackStore
    frames = list(range(2, 14)) if direction > 0 else list(range(13, 1, -1))
    off, want = run_tracker(frames, direction)
    assert off.track_store is None
    tr, got = run_tracker(frames, direction, track_store=True, track_store_frames_per_chunk=5)
    for f in frames:                                                              # nothing else changes
        assert all(torch.equal(a, b) for a, b in zip(got[f], want[f])), f
    st = tr.track_store
    assert isinstance(st, DenseTrackStore) and st.frame_ids == frames and len(st) == 12 and st.frames_per_chunk == 5
    assert st.nbytes == 3 * 5 * (gi.SEQ_H * gi.SEQ_W * 8 + 32)
    rng = np.random.default_rng(11)
    q = rng.uniform(-2, 98, size=(9, 2)).astype(np.float32)
    coords, occl = st.tracks(q)
    assert coords.shape == (9, 12, 2) and occl.shape == (9, 12)
    assert np.array_equal(coords[:, 0], q) and not occl[:, 0].any()                # the identity result of the start frame
    for k, f in enumerate(frames):
        planes = [want[f][0][0], want[f][0][1], want[f][1][0], want[f][2][0]]
        qd = [T(O.dequantize_u16(*O.quantize_u16(p.numpy()))) for p in planes]
        r = FlowOUTrackingResult(torch.stack(qd[0:2]), qd[2][None], qd[3][None], validate=False)
        c, o = convert_to_point_tracking(r, q)
        assert np.array_equal(coords[:, k], c) and np.array_equal(occl[:, k], o), f
        # ... which stays within the quantisation bound of the read-out of the exact result
        ce, oe = convert_to_point_tracking(FlowOUTrackingResult(*want[f], validate=False), q)
        b = [quant_bound(st.lohi(k)[ch]) for ch in range(3)]
        assert np.abs(c[:, 0] - ce[:, 0]).max() <= 1e-5 + b[0] and np.abs(c[:, 1] - ce[:, 1]).max() <= 1e-5 + b[1]
        assert np.abs(o - oe).max() <= 1e-6 + b[2]
    # init() on a used tracker starts a fresh store
    tr.init(gi.id_image(4), start_frame_i=4)
    assert tr.track_store is not st and tr.track_store.frame_ids == [4] and tr.track_store.frames_per_chunk == 5
    tr.track(gi.id_image(5))
    assert tr.track_store.frame_ids == [4, 5]


def test_track_store_limits_and_refusals():
    from mft_amd.MFT import MFT
    from mft_amd.multi import MultiTemplateMFT
    frame_bytes = gi.SEQ_H * gi.SEQ_W * 8 + 32
    tr = MFT(make_config(keep_result_on_device=True, track_store=True, track_store_frames_per_chunk=2,
                         track_store_max_bytes=2 * frame_bytes), backend=OracleBackend(), device="cpu")
    tr.init(gi.id_image(0))
    tr.track(gi.id_image(1))
    assert tr.track_store.max_bytes == 2 * frame_bytes and len(tr.track_store) == 2
    with pytest.raises(MemoryError):
        tr.track(gi.id_image(2))
    sharded = MFT(make_config(track_store=True, delta_sharding=True), backend=OracleBackend(), device="cpu")
    with pytest.raises(ValueError, match="track_store"):
        sharded.init(gi.id_image(0))
    multi = MultiTemplateMFT(make_config(track_store=True), backend=OracleBackend(), device="cpu")
    with pytest.raises(ValueError, match="track_store"):
        multi.init([0])
