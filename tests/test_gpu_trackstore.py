"""The dense track store on the device (csrc/trackstore.hip through mft_amd/ops.py and mft_amd/trackstore.py): every comparison
is against code that was there before it -- ``quantize_u16`` / ``dequantize_u16`` for the codec, ``sample_points`` on the
dequantised planes for the read-out, the reference's goldens, the host restatement of the store, and the tracker without it."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import golden_inputs as gi
from mft_amd import _lib, ops
from mft_amd._lib import MftxError
from mft_amd.config import load_config
from mft_amd.results import FlowOUTrackingResult
from mft_amd.synth import SyntheticVideo
from mft_amd.trackstore import DenseTrackStore

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
DEV = "cuda"
SIZES = [(37, 53), (40, 56), (64, 64)]          # odd H * W (plane tails unaligned), the results-API golden's size, aligned


def quant_bound(lohi_c):
    """tests/test_trackstore.py: half a step + 0.01 step (fp32 rounding of u * 65535 at the boundary) + 2^-21 of the magnitude."""
    lo, hi = float(lohi_c[0]), float(lohi_c[1])
    return 0.51 * (hi - lo) / 65535 + 2.0 ** -21 * max(abs(lo), abs(hi))


def field(seed, H, W):
    """Seeded smooth planes (numpy): flow that leaves the frame here and there, occlusion in [0, 1], positive sigma."""
    r = gi._rng(77, seed, H, W)
    flow = gi.smooth_field(r, 2, H, W, cells=4, amp=5.0 + seed) + np.array([0.7 * seed, -0.4 * seed], np.float32)[:, None, None]
    occl = np.clip(gi.smooth_field(r, 1, H, W, cells=5, amp=0.6), 0, 1).astype(np.float32)
    sigma = (0.05 + np.abs(gi.smooth_field(r, 1, H, W, cells=5, amp=0.7))).astype(np.float32)
    return flow.astype(np.float32), occl, sigma


def cuda(planes):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in planes)


def channels(planes):
    return planes[0][0], planes[0][1], planes[1][0], planes[2][0]


def bits(t):
    """uint16 / float32 tensors as integers: equality of bits, and torch.equal on a dtype every build supports."""
    return t.view(torch.int16 if t.dtype == torch.uint16 else torch.int32).contiguous()


def chan(packed, c):
    """Channel c of a packed frame as a contiguous uint16 plane (the strided copy is made on the int16 view)."""
    return packed.view(torch.int16)[..., c].contiguous().view(torch.uint16)


def assert_frame_is_the_codecs(planes, packed, lohi):
    for c, x in enumerate(channels(planes)):
        q, lh = ops.quantize_u16(x)
        assert torch.equal(bits(packed[..., c]), bits(q)), c
        assert torch.equal(lohi[c], lh), c


def new_frame(H, W):
    return (torch.full((H, W, 4), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16), torch.full((4, 2), -7.0, device=DEV))


# ---- append ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_append_is_quantize_u16_per_channel(H, W):
    planes = cuda(field(1, H, W))
    packed, lohi = new_frame(H, W)
    ops.trackstore_append(planes, packed, lohi)
    assert_frame_is_the_codecs(planes, packed, lohi)
    # the identity result: all four channels flat
    ident = FlowOUTrackingResult.identity((H, W), device=DEV).planes()
    packed, lohi = new_frame(H, W)
    ops.trackstore_append(ident, packed, lohi)
    assert not packed.cpu().numpy().any() and not lohi.cpu().numpy().any()
    assert_frame_is_the_codecs(ident, packed, lohi)
    # planes that are views into one [4, H, W] buffer (H * W odd: 4-byte aligned only), one of them flat but not zero
    buf = torch.cat([p.reshape(-1, H, W) for p in cuda(field(2, H, W))])
    buf[3] = -3.25
    views = (buf[0:2], buf[2:3], buf[3:4])
    if (H * W) % 4:
        assert views[1].data_ptr() % 16 and views[2].data_ptr() % 16
    packed, lohi = new_frame(H, W)
    ops.trackstore_append(views, packed, lohi)
    assert_frame_is_the_codecs(views, packed, lohi)
    assert lohi[3].tolist() == [-3.25, -3.25] and not packed[..., 3].cpu().numpy().any()


def test_append_and_unpack_vs_reference_codec_golden(golden_dir):
    g = np.load(golden_dir / "codec.npz")
    d = gi.codec_inputs()
    st = DenseTrackStore(37, 53, device=DEV, frames_per_chunk=3)
    st.append(cuda((d["flow"], d["occl"], d["sigma"])), frame_i=8)
    assert np.array_equal(st.lohi(0).cpu().numpy(), g["lohi"])
    want_q = g["bgr"][..., 1].astype(np.uint16) * 256 + g["bgr"][..., 2]
    assert np.array_equal(st.packed(0).cpu().numpy(), want_q.transpose(1, 2, 0))
    r = st.result(8)
    assert r.flow.is_cuda and np.array_equal(r.flow.cpu().numpy(), g["dec_flow"])
    assert np.array_equal(r.occlusion.cpu().numpy(), g["dec_occl"]) and np.array_equal(r.sigma.cpu().numpy(), g["dec_sigma"])


# ---- unpack ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_unpack_is_dequantize_u16_per_channel(H, W):
    planes = cuda(field(3, H, W))
    packed, lohi = new_frame(H, W)
    ops.trackstore_append(planes, packed, lohi)
    lh = lohi.cpu().numpy()
    want = [ops.dequantize_u16(chan(packed, c), float(lh[c, 0]), float(lh[c, 1])) for c in range(4)]
    buf = torch.full((4 * H * W + 1,), -7.0, device=DEV)                              # outputs at 4-byte aligned offsets
    out = (buf[1:1 + 2 * H * W].view(2, H, W), buf[1 + 2 * H * W:1 + 3 * H * W].view(1, H, W), buf[1 + 3 * H * W:].view(1, H, W))
    got = ops.trackstore_unpack(packed, lohi, out=out)
    assert got[0].data_ptr() % 16 == 4 and buf[0].item() == -7.0
    for c, x in enumerate(channels(got)):
        assert torch.equal(bits(x), bits(want[c])), c
    fresh = ops.trackstore_unpack(packed, lohi)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(fresh, got))


# ---- query -------------------------------------------------------------------------------------------------------------------
FRAMES = [12, 11, 10, 9, 8, 7, 6, 5, 4]            # nine frames, appended in this order


def special_points(H, W):
    return np.array([[3.25, 7.5], [0.0, 0.0], [W - 1.0, H - 1.0], [5.0, 9.0], [-2.0, 4.0], [W + 4.5, 10.0], [W - 0.5, H - 0.5],
                     [-0.5, -0.5], [W - 1.0, 0.0], [0.0, H - 1.0], [-1.0, -1.0], [float(W), float(H)], [1.0e5, -1.0e5],
                     [20.0, -0.25]], np.float32)


def points(N, H, W):
    sp = special_points(H, W)
    if N <= len(sp):
        return sp[:N].copy()
    r = np.random.default_rng(N)
    return np.concatenate([sp, r.uniform(-3, max(H, W) + 3, size=(N - len(sp), 2)).astype(np.float32)])


@functools.lru_cache(maxsize=None)
def nine_frames(H, W):
    """(store with frames_per_chunk = 4, {frame: planes dequantised by dequantize_u16 with the store's (lo, hi)})."""
    st = DenseTrackStore(H, W, device=DEV, frames_per_chunk=4)
    for f in FRAMES:
        st.append(cuda(field(f, H, W)), f)
    deq = {}
    for f in FRAMES:
        k = st.slot_of(f)
        lh = st.lohi(k).cpu().numpy()
        ch = [ops.dequantize_u16(chan(st.packed(k), c), float(lh[c, 0]), float(lh[c, 1])) for c in range(4)]
        deq[f] = (torch.stack(ch[0:2]), ch[2][None], ch[3][None])
    return st, deq


def reference_table(deq, frames, xy):
    """[N, len(frames), 4]: one ``sample_points`` launch per frame on its dequantised planes."""
    N = int(xy.shape[0])
    table = torch.zeros((N, len(frames), 4), device=DEV)
    tmpl = torch.zeros(N, dtype=torch.int32, device=DEV)
    for j, f in enumerate(frames):
        ops.sample_points([deq[f]], tmpl, xy, table, j)
    return table


@pytest.mark.parametrize("N", [1, 7, 301])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_query_is_sample_points_on_the_dequantised_frames(H, W, N):
    st, deq = nine_frames(H, W)
    assert len(st._chunks) == 3 and st.frame_ids == FRAMES
    xy = torch.from_numpy(points(N, H, W)).to(DEV)
    want = reference_table(deq, FRAMES, xy)
    got = st.query(xy)
    assert got.shape == (N, 9, 4) and torch.equal(bits(got), bits(want))
    if N >= 7:              # out-of-frame taps are 0, not dec(0) = lo: left of the frame nothing of sigma (lo >= 0.05) is seen
        assert float(st.lohi(0)[3, 0]) >= 0.05 and (got[4, :, 3] == 0).all() and (got[4, :, 2] == 0).all()
        assert torch.equal(got[4, :, 0:2], xy[4].expand(9, 2))
    # a subset and a permutation of the frames
    for sel in ([6, 12, 9], [4, 5, 6, 7, 8, 9, 10, 11, 12], [10]):
        assert torch.equal(bits(st.query(xy, frames=sel)), bits(want[:, [FRAMES.index(f) for f in sel]]))
    # column0 > 0 into a wider table: the other columns stay as they were
    wide = torch.full((N, 14, 4), -7.0, device=DEV)
    slots = torch.tensor([st.slot_of(f) for f in FRAMES], dtype=torch.int32, device=DEV)
    ops.trackstore_query(st._chunks, st._lohi, slots, xy, wide, column0=3)
    assert torch.equal(bits(wide[:, 3:12]), bits(want)) and (wide[:, :3] == -7).all() and (wide[:, 12:] == -7).all()
    # slots outside the store are left alone, the others are written
    wide.fill_(-7.0)
    odd = torch.tensor([2, -1, 12, 5, 1 << 30], dtype=torch.int32, device=DEV)
    ops.trackstore_query(st._chunks, st._lohi, odd, xy, wide, column0=0)
    assert torch.equal(bits(wide[:, [0, 3]]), bits(want[:, [2, 5]])) and (wide[:, [1, 2, 4]] == -7).all() and (wide[:, 5:] == -7).all()
    # on a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = st.query(xy)
    s.synchronize()
    assert torch.equal(bits(other), bits(want))
    # repeated calls return identical tables
    out = torch.empty((N, 9, 4), device=DEV)
    for _ in range(20):
        assert st.query(xy, out=out) is out and torch.equal(bits(out), bits(want))


def test_query_with_more_chunks_than_one_launch_carries():
    """195 chunks of one frame each: the chunk descriptors of a launch hold 192, the rest goes out in a second launch."""
    H, W = 37, 53
    _, deq = nine_frames(H, W)
    st = DenseTrackStore(H, W, device=DEV, frames_per_chunk=1)
    for k in range(195):
        st.append(cuda(field(FRAMES[k % 9], H, W)), k)
    assert len(st._chunks) == 195
    xy = torch.from_numpy(points(70, H, W)).to(DEV)
    want = reference_table(deq, FRAMES, xy)
    got = st.query(xy)
    assert torch.equal(bits(got), bits(want[:, [k % 9 for k in range(195)]]))
    sel = [194, 3, 192, 191, 0]
    assert torch.equal(bits(st.query(xy, frames=sel)), bits(want[:, [k % 9 for k in sel]]))


def test_query_vs_reference_golden_and_host_store(golden_dir):
    g = np.load(golden_dir / "results_api.npz")
    d = gi.results_api_inputs()
    planes = (d["flow"], d["occl"], d["sigma"])
    dev_st, cpu_st = DenseTrackStore(40, 56, device=DEV), DenseTrackStore(40, 56, device="cpu")
    dev_st.append(cuda(planes), 3)
    cpu_st.append(tuple(torch.from_numpy(p) for p in planes), 3)
    # host and device stores agree: bitwise on what is stored ...
    assert np.array_equal(dev_st.packed(0).cpu().numpy(), cpu_st.packed(0).numpy())
    assert np.array_equal(dev_st.lohi(0).cpu().numpy(), cpu_st.lohi(0).numpy())
    r_dev, r_cpu = dev_st.result(3), cpu_st.result(3)
    assert all(np.array_equal(a.cpu().numpy(), b.numpy()) for a, b in zip(r_dev.planes(), r_cpu.planes()))
    # ... and on the read-out within the fp32 op-order tolerances of grid_sample (tests/test_results_api.py)
    pts = np.concatenate([d["pts"], points(301, 40, 56)])
    t_dev, t_cpu = dev_st.query(pts).cpu().numpy()[:, 0], cpu_st.query(pts).numpy()[:, 0]
    finite = np.abs(pts).max(axis=1) < 1e4             # (|x| = 1e5: one ulp of the coordinate itself is 8e-3)
    assert np.abs(t_dev[finite, 0:2] - t_cpu[finite, 0:2]).max() <= 1e-5 and np.abs(t_dev[:, 2:4] - t_cpu[:, 2:4]).max() <= 1e-6
    # against the reference's own read-out of the exact result
    b = [quant_bound(cpu_st.lohi(0)[c]) for c in range(4)]
    t = t_dev[:7]
    assert np.abs(t[:, 0] - g["warp_forward_points"][:, 0]).max() <= 1e-5 + b[0]
    assert np.abs(t[:, 1] - g["warp_forward_points"][:, 1]).max() <= 1e-5 + b[1]
    assert np.abs(t[:, 2] - g["sample_occl"][0]).max() <= 1e-6 + b[2]
    assert np.abs(t[:, 3] - g["sample_sigma"][0]).max() <= 1e-6 + b[3]
    coords, occl = dev_st.tracks(d["pts"], frames=[3])
    assert np.array_equal(coords[:, 0], t[:, 0:2]) and np.array_equal(occl[:, 0], t[:, 2])


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _lib.load()
    H, W, N, Tn = 37, 53, 5, 3
    st, _ = nine_frames(H, W)
    flow, occl, sigma = cuda(field(1, H, W))
    packed, lohi = new_frame(H, W)
    ws = torch.empty(lib.mftx_trackstore_workspace_bytes(), dtype=torch.uint8, device=DEV)
    stream = ops._stream()

    def append(flow=flow.data_ptr(), occl=occl.data_ptr(), sigma=sigma.data_ptr(), H=H, W=W, packed=packed.data_ptr(),
               lohi=lohi.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel()):
        _lib.check(lib.mftx_trackstore_append(flow, occl, sigma, H, W, packed, lohi, ws, ws_bytes, stream), "append")

    append()
    for bad in (dict(flow=None), dict(occl=None), dict(sigma=None), dict(packed=None), dict(lohi=None), dict(ws=None),
                dict(H=1), dict(W=1), dict(ws_bytes=ws.numel() - 1), dict(flow=flow.data_ptr() + 2), dict(packed=packed.data_ptr() + 4)):
        with pytest.raises(MftxError):
            append(**bad)

    out = ops.trackstore_unpack(packed, lohi)

    def unpack(packed=packed.data_ptr(), lohi=lohi.data_ptr(), H=H, W=W, flow=out[0].data_ptr(), occl=out[1].data_ptr(),
               sigma=out[2].data_ptr()):
        _lib.check(lib.mftx_trackstore_unpack(packed, lohi, H, W, flow, occl, sigma, stream), "unpack")

    unpack()
    for bad in (dict(packed=None), dict(lohi=None), dict(flow=None), dict(occl=None), dict(sigma=None), dict(H=1), dict(W=1),
                dict(sigma=out[2].data_ptr() + 1)):
        with pytest.raises(MftxError):
            unpack(**bad)

    carr = _lib.ptr_array([c.data_ptr() for c in st._chunks])
    larr = _lib.ptr_array([c.data_ptr() for c in st._lohi])
    holed = _lib.ptr_array([st._chunks[0].data_ptr(), None, st._chunks[2].data_ptr()])
    slots = torch.tensor([0, 4, 8], dtype=torch.int32, device=DEV)
    xy = torch.from_numpy(points(N, H, W)).to(DEV)
    flat = torch.full((N * 6 * 4 + 4,), -7.0, device=DEV)
    assert flat.data_ptr() % 16 == 0

    def query(chunks=carr[0], lohis=larr[0], n_chunks=3, fpc=4, slots=slots.data_ptr(), T=Tn, H=H, W=W, N=N, xy=xy.data_ptr(),
              table=flat.data_ptr(), row_stride=24, column0=1):
        _lib.check(lib.mftx_trackstore_query(chunks, lohis, n_chunks, fpc, slots, T, H, W, N, xy, table, row_stride, column0, stream),
                   "query")

    query()
    for bad in (dict(chunks=None), dict(lohis=None), dict(slots=None), dict(xy=None), dict(table=None), dict(chunks=holed[0]),
                dict(H=1), dict(W=1), dict(T=-1), dict(N=-1), dict(n_chunks=0), dict(fpc=0),
                dict(row_stride=22), dict(row_stride=12), dict(column0=4), dict(column0=-1),
                dict(table=flat.data_ptr() + 4), dict(table=flat.data_ptr() + 8)):
        with pytest.raises(MftxError):
            query(**bad)
    torch.cuda.synchronize()
    seen = flat.clone()
    query(T=0)                                         # no-ops: 0 is returned, nothing is written
    query(N=0)
    query(T=0, table=None, slots=None)
    torch.cuda.synchronize()
    assert torch.equal(flat, seen) and (flat[-4:] == -7).all()
    with pytest.raises(MftxError):                     # the torch front end: host tensors, wrong shapes
        ops.trackstore_query(st._chunks, st._lohi, slots.cpu(), xy, torch.zeros((N, 3, 4), device=DEV))
    with pytest.raises(MftxError):
        ops.trackstore_query(st._chunks, st._lohi, slots, xy, torch.zeros((N, 2, 4), device=DEV))
    with pytest.raises(MftxError):
        ops.trackstore_append((flow, occl, sigma), packed[:-1], lohi)
    with pytest.raises(KeyError):
        st.query(xy, frames=[4, 99])


# ---- tracker, real engine ----------------------------------------------------------------------------------------------------
def _config(fif, **extra):
    conf = load_config(REPO / "configs" / "MFT_cfg.py")
    conf.flow_config.model = None
    conf.flow_config.synthetic_weights_seed = gi.WEIGHT_SEED          # make_weights(seed): stand-in weights
    conf.flow_config.flow_iters = 4
    conf.flow_config.frames_in_flight = fif
    conf.deltas = [np.inf, 1, 2]
    conf.keep_result_on_device = True
    for k, v in extra.items():
        setattr(conf, k, v)
    return conf


def _run(conf, video):
    tracker = conf.tracker_class(conf)
    out = []
    for k in range(len(video)):
        r = tracker.init(video[0]).result if k == 0 else tracker.track(video[k]).result
        out.append(tuple(p.to(DEV).clone() for p in r.planes()))
    return tracker, out


@pytest.mark.parametrize("fif", [1, 2])
def test_tracker_with_track_store_real_engine(fif):
    from mft_amd.point_tracking import convert_to_point_tracking
    H, W = 128, 160
    video = SyntheticVideo(H, W, n_frames=6, seed=21)
    off, want = _run(_config(fif), video)
    assert off.track_store is None
    tr, got = _run(_config(fif, track_store=True), video)
    for k in range(6):
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got[k], want[k])), k
    st = tr.track_store
    assert len(st) == 6 and st.frame_ids == list(range(6)) and st.frames_per_chunk == 64
    assert st.nbytes == 64 * (H * W * 8 + 4 * 2 * 4)
    q = np.concatenate([special_points(H, W), np.random.default_rng(4).uniform(0, [W, H], size=(86, 2)).astype(np.float32)])
    xy = torch.from_numpy(q).to(DEV)
    table = st.query(xy)
    # ... the per-frame sample_points of the dequantised stored frames, bitwise
    deq = {}
    for k in range(6):
        assert_frame_is_the_codecs(want[k], st.packed(k), st.lohi(k))
        lh = st.lohi(k).cpu().numpy()
        ch = [ops.dequantize_u16(chan(st.packed(k), c), float(lh[c, 0]), float(lh[c, 1])) for c in range(4)]
        deq[k] = (torch.stack(ch[0:2]), ch[2][None], ch[3][None])
    assert torch.equal(bits(table), bits(reference_table(deq, list(range(6)), xy)))
    # ... and within the quantisation bound of the read-out of the exact results
    coords, occl = st.tracks(q)
    inside = np.abs(q).max(axis=1) < 1e4
    for k in range(6):
        c, o = convert_to_point_tracking(FlowOUTrackingResult(*want[k], validate=False), xy)
        b = [quant_bound(st.lohi(k)[ch].cpu()) for ch in range(3)]
        assert np.abs(coords[inside, k, 0] - c[inside, 0]).max() <= 1e-5 + b[0], k
        assert np.abs(coords[inside, k, 1] - c[inside, 1]).max() <= 1e-5 + b[1], k
        assert np.abs(occl[:, k] - o).max() <= 1e-6 + b[2], k
