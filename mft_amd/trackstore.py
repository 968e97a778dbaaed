"""DenseTrackStore -- every frame's dense (template -> frame) result kept in 16 bits, any point's track read out afterwards.

MFT tracks every pixel, but the tracker keeps only the frames its deltas still need (``MFT.cleanup_memory``), and the point
read-outs that exist (``mftx_sample_points``) want the queries before the video is tracked.  This store keeps what the tracker
computed: each appended result is quantised the way the reference's flow cache quantises its entries (``.flowouX16``: per-channel
min / max, uint16, round-half-even -- MFT/utils/io.py:495-512, read back by :548-551) into ONE 8-byte word per pixel
(fx, fy, occlusion, sigma), 8 B/px instead of 16 B/px, and ``query`` answers "these N points over these T frames" in one
kernel call straight from the quantised frames (csrc/trackstore.hip).  The precision is what the reference accepts for every
flow that passes through its disk cache: half a quantisation step of each channel's range.

    store = DenseTrackStore(H, W)                     # or: config.track_store = True -> tracker.track_store
    store.append(result, frame_i)                     # on the current stream, no host wait
    table = store.query(points)                       # device [N, T, 4]: x, y, occlusion, sigma per frame, append order
    coords, occl = store.tracks(points, frames=[...]) # numpy, the shape MultiTemplateMFT.point_tracks() gives
    result = store.result(frame_i)                    # the dequantised FlowOUTrackingResult, on the device
    table, cell = store.locate(points_on_57, 57)      # the stored map inverted: template x, y, occlusion, sigma; cell -1 = none
    coords, occl, found = store.tracks_from(points_on_57, 57)     # ... and those template points followed over the frames
    table, cell = store.inverse(57)                   # locate at EVERY pixel of frame 57: [H, W, 4], [H, W]
    flow, occl, sigma, found = store.results_from(57) # dense results from frame 57 to every stored frame: [T, 2, H, W], ...
    result, found = store.result_from(57, 80)         # ... one of them as a FlowOUTrackingResult
    a = store.appearance(video, reference=video[0])   # the video read along every track: a.count, a.sum, a.sumsq, a.mean, a.var

``device="cpu"`` is a host restatement of the same operations (numpy / torch), which pins the semantics without a GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from .results import FlowOUTrackingResult

U16_MAX = 2 ** 16 - 1


def compress_channel(xs):
    """One channel -> (uint16 array, min, max): the quantisation of a ``.flowouX16`` entry, in float32 as numpy evaluates it
    (a channel whose range is below 1e-8 becomes all zeros)."""
    x = np.asarray(xs, dtype=np.float32)
    lo, hi = x.min(), x.max()
    if np.abs(hi - lo) < 1e-8:
        unit = np.zeros_like(x)
    else:
        unit = (x - lo) / (hi - lo)
    return np.round(unit * U16_MAX).astype(np.uint16), lo, hi


def decompress_channel(q, lo, hi):
    """The inverse: uint16 array + the channel's (min, max) -> float32."""
    lo, hi = np.float32(lo), np.float32(hi)
    return (np.asarray(q).astype(np.float32) / U16_MAX) * (hi - lo) + lo


# ---- locate: the stored map inverted at a point given on a stored frame -------------------------------------------------------
# The definition ("locate"), in numpy float32 with + - * / only and in the order csrc/trackstore.hip (ts_solve_cell,
# ts_mix, ts_locate_key) evaluates it: the two agree bit for bit (tests/test_gpu_track_locate.py).
LOCATE_EPS = np.float32(2.0 ** -10)       # px: the widening of a cell's box and the residual a candidate may have
LOCATE_NEWTON_STEPS = 6
_ONE, _ZERO, _HALF = np.float32(1), np.float32(0), np.float32(0.5)


def _clamp01(t):
    return np.where(t < _ZERO, _ZERO, np.where(t > _ONE, _ONE, t))        # (a NaN stays one)


def _solve_cells(c, qx, qy):
    """c = (ax, ay, bx, by, cx, cy, dx, dy): float32 [K] corner images A = M(i, j), B = M(i, j+1), C = M(i+1, j), D = M(i+1, j+1) of
    K cells; (qx, qy): the query, float32 scalars -> (u [K], v [K], candidate [K]): the clamped solution of
    A + u (B - A) + v (C - A) + u v (A - B - C + D) = Q after LOCATE_NEWTON_STEPS Newton steps from the cell's centre."""
    ax, ay, bx, by, cx, cy, dx, dy = c
    ex, ey, gx, gy = bx - ax, by - ay, cx - ax, cy - ay
    hx, hy = ((ax - bx) - cx) + dx, ((ay - by) - cy) + dy
    u = np.full(ax.shape, _HALF, np.float32)
    v = u.copy()
    with np.errstate(all="ignore"):
        for _ in range(LOCATE_NEWTON_STEPS):
            uv = u * v
            rx = (((ax + u * ex) + v * gx) + uv * hx) - qx
            ry = (((ay + u * ey) + v * gy) + uv * hy) - qy
            j00, j01, j10, j11 = ex + v * hx, gx + u * hx, ey + v * hy, gy + u * hy
            det = j00 * j11 - j01 * j10
            du, dv = (rx * j11 - ry * j01) / det, (ry * j00 - rx * j10) / det
            u, v = u - du, v - dv
        finite = np.isfinite(u) & np.isfinite(v)
        u, v = _clamp01(u), _clamp01(v)
        uv = u * v
        rx = (((ax + u * ex) + v * gx) + uv * hx) - qx
        ry = (((ay + u * ey) + v * gy) + uv * hy) - qy
        ok = finite & (np.abs(rx) <= LOCATE_EPS) & (np.abs(ry) <= LOCATE_EPS)
    return u, v, ok


def _mix(a, b, c, d, u, v):
    """The sampler's weights (1-u)(1-v), u(1-v), (1-u)v, uv and its order of summation."""
    w00, w01, w10, w11 = (_ONE - u) * (_ONE - v), u * (_ONE - v), (_ONE - u) * v, u * v
    return a * w00 + b * w01 + c * w10 + d * w11


def _locate_host(planes, q, thr, table, cell):
    """planes = (fx, fy, occlusion, sigma) float32 [H, W] of ONE dequantised frame; q float32 [K, 2] -> rows of table [K, 4] and
    cell [K] (numpy, written in place)."""
    fx, fy, oc, sg = planes
    H, W = fx.shape
    mx = np.arange(W, dtype=np.float32)[None, :] + fx
    my = np.arange(H, dtype=np.float32)[:, None] + fy

    def corners(p):
        return p[:-1, :-1].ravel(), p[:-1, 1:].ravel(), p[1:, :-1].ravel(), p[1:, 1:].ravel()

    (ax, bx, cx, dx), (ay, by, cy, dy) = corners(mx), corners(my)
    lox, hix = np.fmin(np.fmin(ax, bx), np.fmin(cx, dx)) - LOCATE_EPS, np.fmax(np.fmax(ax, bx), np.fmax(cx, dx)) + LOCATE_EPS
    loy, hiy = np.fmin(np.fmin(ay, by), np.fmin(cy, dy)) - LOCATE_EPS, np.fmax(np.fmax(ay, by), np.fmax(cy, dy)) + LOCATE_EPS
    occ, sig = corners(oc), corners(sg)
    for n in range(q.shape[0]):
        qx, qy = q[n, 0], q[n, 1]
        table[n], cell[n] = np.nan, -1
        idx = np.flatnonzero((qy >= loy) & (qy <= hiy))                                   # the prefilter: rows first, then
        idx = idx[(qx >= lox[idx]) & (qx <= hix[idx])]                                    # columns among the cells that are left
        if idx.size == 0:
            continue
        u, v, ok = _solve_cells((ax[idx], ay[idx], bx[idx], by[idx], cx[idx], cy[idx], dx[idx], dy[idx]), qx, qy)
        if not ok.any():
            continue
        idx, u, v = idx[ok], u[ok], v[ok]
        o = _mix(*(p[idx] for p in occ), u, v)
        s = _mix(*(p[idx] for p in sig), u, v)
        key_sigma = np.where(s > _ZERO, s, _ZERO)           # what the device key holds: a sigma that is not > 0 counts as +0
        w = np.lexsort((idx, key_sigma, o > thr))[0]        # smallest (occluded, sigma, cell)
        i, j = divmod(int(idx[w]), W - 1)
        table[n] = (np.float32(j) + u[w], np.float32(i) + v[w], o[w], s[w])
        cell[n] = idx[w]


def _as_points(points, device, name=None):
    """points: anything (N, 2)-like -> float32 [N, 2] on ``device``, contiguous.  With ``name`` (of the method asking) any other
    shape is a ``ValueError``; without it the points are reshaped to (-1, 2)."""
    if not isinstance(points, torch.Tensor):
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)))
    if name is None:
        points = points.reshape(-1, 2)
    elif points.dim() != 2 or int(points.shape[1]) != 2:
        raise ValueError(f"{name}: points must be (N, 2), not {tuple(points.shape)}")
    return points.to(device=device, dtype=torch.float32).contiguous()


def _frame_ids(frame, name, n=None):
    """``frame``: one frame id, or a host sequence of them (of exactly ``n`` where ``n`` is given) -> (ids: a 1-D array, lead: () for
    the single id, (len(ids),) for a sequence).  Anything else is a ``ValueError``."""
    ids = np.asarray(frame)
    if ids.ndim == 0:
        return ids.reshape(1), ()
    if ids.ndim == 1 and (n is None or ids.shape[0] == n):
        return ids, (int(ids.shape[0]),)
    raise ValueError(f"{name}: frame must be one frame id or " + ("a sequence of them" if n is None else f"{n} of them"))


def _tracks_to_host(tracks, extra):
    """tracks [N, T, 4] and ``extra`` [N] on the device -> numpy (tracks [N, T, 4], extra [N] as float32) in ONE download."""
    N, T = int(tracks.shape[0]), int(tracks.shape[1])
    both = torch.cat([tracks.reshape(N, T * 4), extra.to(torch.float32)[:, None]], dim=1).cpu().numpy()
    return both[:, :T * 4].reshape(N, T, 4), both[:, T * 4]


def chain_behind_inverse(table, q, grid, ok):
    """The rule by which results are chained (MFT/MFT.py:233-239) with an inverse as the left result: table [N, 4] = the inverse's
    (Px, Py, o_src, s_src) per pixel, q [N, T, 4] = the read-out (qx, qy, o_dst, s_dst) of that point per column, grid [N, 2] the
    pixels' centres, ok [N] or [N, T] bool -> planar (flow [T, 2, N], occlusion [T, N], sigma [T, N]): flow = q - pixel,
    occlusion = max(o_src, o_dst), sigma = sqrt(s_src^2 + s_dst^2), and NaN, 1, +inf where not ok."""
    flow = q[:, :, 0:2] - grid[:, None, :]
    occl = torch.maximum(table[:, None, 2], q[:, :, 2])
    s_src, s_dst = table[:, None, 3], q[:, :, 3]
    # (the root taken in float64 and rounded once: the correctly rounded float32 root on every device -- torch's own float32
    # sqrt is an ulp off numpy's for some arguments on the host)
    sigma = torch.sqrt((s_src * s_src + s_dst * s_dst).to(torch.float64)).to(torch.float32)
    if ok.dim() == 1:
        ok = ok[:, None]
    nan, one, inf = (torch.full((), v, dtype=torch.float32, device=q.device) for v in (float("nan"), 1.0, float("inf")))
    flow = torch.where(ok[:, :, None], flow, nan)            # (each name rebound at once: no second copy of a plane stays alive)
    occl = torch.where(ok, occl, one)
    sigma = torch.where(ok, sigma, inf)
    return flow.permute(1, 2, 0), occl.t(), sigma.t()


class TrackAppearance:
    """What ``DenseTrackStore.appearance`` returns, on the store's device.  ``count`` int32 [H, W]: the columns in which the
    template pixel is visible; ``sum`` / ``sumsq`` float32 [C, H, W]: the sums over those columns of d = sample - reference and of
    d * d; ``reference`` uint8 [H, W, C] or None (= 0); ``frames``: the columns' frame ids; with ``stack=True`` ``warped`` uint8
    [T, H, W, C] and ``visible`` bool [T, H, W], else None.  ``mean`` and ``var`` are derived from them in torch."""

    def __init__(self, frames, count, sum, sumsq, reference=None, warped=None, visible=None):
        self.frames, self.count, self.sum, self.sumsq = list(frames), count, sum, sumsq
        self.reference, self.warped, self.visible = reference, warped, visible

    def _mean_d(self):
        return (self.sum / self.count.to(torch.float32)).permute(1, 2, 0)          # 0 / 0 = NaN where the pixel was never visible

    @property
    def mean(self):
        """float32 [H, W, C]: reference + sum / count -- the template's mean appearance over the columns where each pixel is
        visible; NaN where count is 0."""
        m = self._mean_d()
        return m if self.reference is None else self.reference.to(torch.float32) + m

    @property
    def var(self):
        """float32 [H, W, C]: max(sumsq / count - (sum / count)^2, 0); NaN where count is 0."""
        m = self._mean_d()
        return ((self.sumsq / self.count.to(torch.float32)).permute(1, 2, 0) - m * m).clamp(min=0)


def _as_images(images, T, H, W, name):
    """images: one uint8 tensor [T, H, W, C] or a sequence of T uint8 (H, W, C) numpy arrays / tensors, C = 1 .. 4 -> (the tensor,
    or the list with numpy arrays wrapped as tensors; C).  Nothing is copied or moved.  Anything else is a ``ValueError``."""
    def one(img, C):
        if isinstance(img, np.ndarray):
            if img.dtype != np.uint8:
                raise ValueError(f"{name}: images must be uint8, not {img.dtype}")
            img = torch.from_numpy(np.ascontiguousarray(img))
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
            raise ValueError(f"{name}: images must be uint8 numpy arrays or tensors")
        if img.dim() != 3 or tuple(img.shape[:2]) != (H, W) or not 1 <= int(img.shape[2]) <= 4 or (C and int(img.shape[2]) != C):
            raise ValueError(f"{name}: an image must be ({H}, {W}, C) with one C = 1 .. 4 for all, not {tuple(img.shape)}")
        return img

    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8:
            raise ValueError(f"{name}: images must be uint8, not {images.dtype}")
        if images.dim() != 4 or tuple(images.shape[:3]) != (T, H, W) or not 1 <= int(images.shape[3]) <= 4:
            raise ValueError(f"{name}: images must be [{T}, {H}, {W}, C] with C = 1 .. 4, not {tuple(images.shape)}")
        return images, int(images.shape[3])
    images = list(images)
    if len(images) != T:
        raise ValueError(f"{name}: {len(images)} images for {T} frames")
    out, C = [], 0
    for img in images:
        out.append(one(img, C))
        C = int(out[-1].shape[2])
    return out, C


class DenseTrackStore:
    def __init__(self, H, W, device="cuda", frames_per_chunk=64, max_bytes=None):
        """A store of H x W frames.  Storage grows by chunks of ``frames_per_chunk`` frames (torch allocations on ``device``);
        ``max_bytes`` (optional) bounds ``nbytes``: the append that would exceed it raises ``MemoryError`` instead."""
        self.H, self.W = int(H), int(W)
        if self.H < 2 or self.W < 2:
            raise ValueError("DenseTrackStore: H and W must be >= 2")
        self.device = torch.device(device)
        self.frames_per_chunk = int(frames_per_chunk)
        if self.frames_per_chunk < 1:
            raise ValueError("DenseTrackStore: frames_per_chunk must be at least 1")
        self.max_bytes = None if max_bytes is None else int(max_bytes)
        self.frame_ids = []          # in append order: frame_ids[slot] is the frame held by that slot
        self._slot_of = {}
        self._chunks = []            # uint16 [frames_per_chunk, H, W, 4]
        self._lohi = []              # float32 [frames_per_chunk, 4, 2]

    # ------------------------------------------------------------------ bookkeeping
    @property
    def native(self):
        return self.device.type != "cpu"

    @property
    def chunk_bytes(self):
        return self.frames_per_chunk * (self.H * self.W * 8 + 4 * 2 * 4)

    @property
    def nbytes(self):
        """Bytes of storage held: whole chunks, packed frames plus their (min, max) tables."""
        return len(self._chunks) * self.chunk_bytes

    def __len__(self):
        return len(self.frame_ids)

    def slot_of(self, frame_i):
        """The slot that holds frame ``frame_i`` (``KeyError`` if it was never appended)."""
        return self._slot_of[int(frame_i)]

    def packed(self, slot):
        """View [H, W, 4] uint16 of the slot's quantised frame."""
        slot = self._check_slot(slot)
        return self._chunks[slot // self.frames_per_chunk][slot % self.frames_per_chunk]

    def lohi(self, slot):
        """View [4, 2] float32: (min, max) of flow x, flow y, occlusion, sigma of the slot's frame."""
        slot = self._check_slot(slot)
        return self._lohi[slot // self.frames_per_chunk][slot % self.frames_per_chunk]

    def _check_slot(self, slot):
        slot = int(slot)
        if not 0 <= slot < len(self.frame_ids):
            raise IndexError(f"DenseTrackStore: no slot {slot} ({len(self.frame_ids)} frames stored)")
        return slot

    def _grow(self):
        if self.max_bytes is not None and self.nbytes + self.chunk_bytes > self.max_bytes:
            raise MemoryError(f"DenseTrackStore: another chunk of {self.frames_per_chunk} frames ({self.chunk_bytes} bytes) would "
                              f"exceed max_bytes = {self.max_bytes} ({self.nbytes} bytes held)")
        self._chunks.append(torch.empty((self.frames_per_chunk, self.H, self.W, 4), dtype=torch.uint16, device=self.device))
        self._lohi.append(torch.zeros((self.frames_per_chunk, 4, 2), dtype=torch.float32, device=self.device))

    # ------------------------------------------------------------------ append
    @property
    def next_needs_chunk(self):
        """Whether the next frame opens a new chunk (``chunk_bytes`` more of storage)."""
        return len(self.frame_ids) == len(self._chunks) * self.frames_per_chunk

    def _next_slot(self, frame_i):
        """-> (frame id, the slot the next frame takes), its chunk allocated; nothing is registered yet."""
        frame_i = len(self.frame_ids) if frame_i is None else int(frame_i)
        if frame_i in self._slot_of:
            raise ValueError(f"DenseTrackStore: frame {frame_i} is stored already (slot {self._slot_of[frame_i]})")
        if self.next_needs_chunk:
            self._grow()
        return frame_i, len(self.frame_ids)

    def reserve(self, frame_i=None):
        """Take the next slot for frame ``frame_i`` whose words are written from OUTSIDE -- a multi-template pass quantises the
        results of all its templates in one call (``ops.trackstore_append_multi``) -> (slot, packed view [H, W, 4] uint16, lohi
        view [4, 2] float32).  The frame counts as stored from here on; the caller writes both views, on the stream the
        store's readers use, before anything reads them.  Ids and ``max_bytes`` as for ``append``."""
        frame_i, slot = self._next_slot(frame_i)
        self.frame_ids.append(frame_i)
        self._slot_of[frame_i] = slot
        return slot, self.packed(slot), self.lohi(slot)

    def unreserve(self, frame_i):
        """Give the LAST slot back: frame ``frame_i`` was reserved and its words were never written (the call that was to write
        them failed).  The chunk stays allocated.  ``ValueError`` unless the frame holds the last slot."""
        frame_i = int(frame_i)
        if not self.frame_ids or self.frame_ids[-1] != frame_i:
            raise ValueError(f"DenseTrackStore: frame {frame_i} does not hold the last slot")
        self.frame_ids.pop()
        del self._slot_of[frame_i]

    def append(self, result_or_planes, frame_i=None):
        """Store one result -- a ``FlowOUTrackingResult`` or its (flow[2,H,W], occl[1,H,W], sigma[1,H,W]) planes -- as frame
        ``frame_i`` (default: the number of frames stored so far) and return its slot.  Frames may come in any order, each id
        once (``ValueError``).  On the device this enqueues two kernels on the current stream and never waits for the GPU."""
        planes = result_or_planes.planes() if hasattr(result_or_planes, "planes") else tuple(result_or_planes)
        flow, occl, sigma = planes
        if tuple(flow.shape) != (2, self.H, self.W) or tuple(occl.shape) != (1, self.H, self.W) or \
                tuple(sigma.shape) != (1, self.H, self.W):
            raise ValueError(f"DenseTrackStore: planes must be [2,H,W], [1,H,W], [1,H,W] with H x W = {self.H} x {self.W}")
        frame_i, slot = self._next_slot(frame_i)
        chunk, k = slot // self.frames_per_chunk, slot % self.frames_per_chunk
        if self.native:
            from . import ops
            planes = tuple(torch.as_tensor(p).to(device=self.device, dtype=torch.float32).contiguous() for p in planes)
            ops.trackstore_append(planes, self._chunks[chunk][k], self._lohi[chunk][k])
        else:
            pk, lh = self._chunks[chunk].numpy(), self._lohi[chunk].numpy()
            src = [torch.as_tensor(p).detach().cpu().numpy() for p in planes]
            for c, x in enumerate((src[0][0], src[0][1], src[1][0], src[2][0])):
                q, lo, hi = compress_channel(x)
                pk[k, :, :, c] = q
                lh[k, c] = (lo, hi)
        self.frame_ids.append(frame_i)
        self._slot_of[frame_i] = slot
        return slot

    # ------------------------------------------------------------------ read-out
    def _slots(self, frames):
        if frames is None:
            return list(range(len(self.frame_ids)))
        return [self.slot_of(f) for f in frames]           # KeyError for a frame that was never appended

    def query(self, points, frames=None, out=None):
        """points (N, 2) xy on the template frame; frames: a sequence of frame ids (default: all, in append order) ->
        float32 tensor [N, T, 4] on the store's device: (x, y, occlusion, sigma) of every point in every requested frame --
        ``warp_forward_points`` and ``sample`` of the results API on the dequantised frames.  ``out``: a [N, T, 4] tensor to
        write into.  On the device: one kernel call, and with ``points`` a device tensor no host synchronisation."""
        slots = self._slots(frames)
        xy = _as_points(points, self.device)
        N, T = int(xy.shape[0]), len(slots)
        if out is None:
            out = torch.zeros((N, T, 4), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (N, T, 4) or out.dtype != torch.float32 or out.device != xy.device:
            raise ValueError(f"DenseTrackStore.query: out must be a float32 [{N}, {T}, 4] tensor on {self.device}")
        if N == 0 or T == 0:
            return out
        if self.native:
            from . import ops
            if frames is None:
                st = torch.arange(T, dtype=torch.int32, device=self.device)
            else:
                st = torch.tensor(slots, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
            ops.trackstore_query(self._chunks, self._lohi, st, xy, out, 0)
        else:
            for j, slot in enumerate(slots):
                r = self._result_of_slot(slot)
                out[:, j, 0:2] = r.warp_forward_points(xy)
                _, o, s = r.sample(xy)
                out[:, j, 2], out[:, j, 3] = o[0], s[0]
        return out

    def tracks(self, points, frames=None):
        """-> numpy (coords [N, T, 2], occlusion [N, T]), the shape ``MultiTemplateMFT.point_tracks()`` gives.  ONE download;
        it synchronises."""
        table = self.query(points, frames).cpu().numpy()
        return table[:, :, 0:2].copy(), table[:, :, 2].copy()

    def _result_of_slot(self, slot):
        if self.native:
            from . import ops
            return FlowOUTrackingResult(*ops.trackstore_unpack(self.packed(slot), self.lohi(slot)), validate=False)
        pk, lh = self.packed(slot).numpy(), self.lohi(slot).numpy()
        ch = [torch.from_numpy(np.ascontiguousarray(decompress_channel(pk[:, :, c], lh[c, 0], lh[c, 1]))) for c in range(4)]
        return FlowOUTrackingResult(torch.stack(ch[0:2]), ch[2][None], ch[3][None], validate=False)

    def result(self, frame_i):
        """The stored frame, dequantised: a ``FlowOUTrackingResult`` on the store's device (for ``draw_edit`` /
        ``warp_forward_device`` after the fact, and for export)."""
        return self._result_of_slot(self.slot_of(frame_i))

    # ------------------------------------------------------------------ the inverse: points given on a stored frame
    def locate(self, points, frame, occlusion_threshold=0.5, out=None):
        """points (N, 2) xy given ON stored frame(s) ``frame`` -- one frame id, or a host sequence of N ids, any order -> (table,
        cell) on the store's device: float32 [N, 4] = (template x, template y, occlusion, sigma) of the template point whose
        image on that frame is the query, and int32 [N] = the template cell i * (W - 1) + j it lies in.  Where several
        template points map to the query the one that is not occluded (occlusion <= ``occlusion_threshold``), then of lowest
        sigma, then of lowest cell wins; where none does, cell is -1 and the row is NaN.  ``out``: a (table, cell) pair to
        write into.  On the device: one call, and with ``points`` a device tensor no host synchronisation."""
        xy = _as_points(points, self.device, "DenseTrackStore.locate")
        N = int(xy.shape[0])
        ids, lead = _frame_ids(frame, "DenseTrackStore.locate", N)
        slots = [self.slot_of(f) for f in ids] * (1 if lead else N)      # KeyError for a frame that was never appended
        if out is None:
            out = (torch.empty((N, 4), dtype=torch.float32, device=self.device), torch.empty((N,), dtype=torch.int32, device=self.device))
        table, cell = out
        if tuple(table.shape) != (N, 4) or table.dtype != torch.float32 or tuple(cell.shape) != (N,) or cell.dtype != torch.int32 \
                or table.device != xy.device or cell.device != xy.device or not table.is_contiguous() or not cell.is_contiguous():
            raise ValueError(f"DenseTrackStore.locate: out must be contiguous (float32 [{N}, 4], int32 [{N}]) tensors on {self.device}")
        if N == 0:
            return table, cell
        if self.native:
            from . import ops
            ops.trackstore_locate(self._chunks, self._lohi, slots, xy, table, cell, occlusion_threshold)
        else:
            q, slots = xy.numpy(), np.asarray(slots)
            tb, cl = table.numpy(), cell.numpy()
            for slot in np.unique(slots):
                r = self._result_of_slot(int(slot))
                planes = (r.flow[0].numpy(), r.flow[1].numpy(), r.occlusion[0].numpy(), r.sigma[0].numpy())
                sel = np.flatnonzero(slots == slot)
                t, c = np.empty((sel.size, 4), np.float32), np.empty(sel.size, np.int32)
                _locate_host(planes, q[sel], np.float32(occlusion_threshold), t, c)
                tb[sel], cl[sel] = t, c
        return table, cell

    def tracks_from(self, points, frame, frames=None, occlusion_threshold=0.5):
        """points given on stored frame(s) ``frame`` (as for ``locate``), followed over ``frames`` (default: all, in append
        order) -> numpy (coords [N, T, 2], occlusion [N, T], found [N]): ``locate``, then ``query`` of the located template
        points.  A point that no template point maps to has found False, NaN coordinates and occlusion 1.  ONE download; it
        synchronises."""
        table, cell = self.locate(points, frame, occlusion_threshold)
        found = cell >= 0
        template = torch.where(found[:, None], table[:, 0:2], torch.zeros((), dtype=torch.float32, device=self.device))
        tracks, found = _tracks_to_host(self.query(template, frames), found)
        found = found > 0
        coords, occl = tracks[:, :, 0:2].copy(), tracks[:, :, 2].copy()
        coords[~found], occl[~found] = np.nan, 1.0
        return coords, occl, found

    # ------------------------------------------------------------------ the dense inverse: every pixel of a stored frame
    def _pixel_grid(self):
        """float32 [H * W, 2] on the store's device: the pixel centres (x, y), row-major."""
        idx = torch.arange(self.H * self.W, device=self.device)
        return torch.stack([idx % self.W, torch.div(idx, self.W, rounding_mode="floor")], dim=1).to(torch.float32)

    def inverse(self, frame, occlusion_threshold=0.5, out=None):
        """Stored frame ``frame`` inverted at every pixel: ``locate`` with the H * W pixel centres as its points, bit for bit ->
        (table [H, W, 4] float32, cell [H, W] int32) on the store's device: table[y, x] = (template x, template y, occlusion,
        sigma) of the template point whose image is pixel (x, y) of that frame, cell[y, x] its template cell, -1 (and a row of
        NaN) where nothing maps to the pixel.  A sequence of G frame ids gives [G, H, W, 4] and [G, H, W].  ``out``: a
        (table, cell) pair to write into.  On the device: ONE call whatever G is -- every template cell writes itself onto the
        pixels its image covers (csrc/trackstore.hip, ts_atlas_scatter_kernel in its identity mode) -- and no host
        synchronisation."""
        ids, lead = _frame_ids(frame, "DenseTrackStore.inverse")
        slots = [self.slot_of(f) for f in ids]                  # KeyError for a frame that was never appended
        H, W = self.H, self.W
        if out is None:
            out = (torch.empty(lead + (H, W, 4), dtype=torch.float32, device=self.device),
                   torch.empty(lead + (H, W), dtype=torch.int32, device=self.device))
        table, cell = out
        if tuple(table.shape) != lead + (H, W, 4) or table.dtype != torch.float32 or tuple(cell.shape) != lead + (H, W) \
                or cell.dtype != torch.int32 or table.device.type != self.device.type or cell.device.type != self.device.type \
                or not table.is_contiguous() or not cell.is_contiguous():
            raise ValueError(f"DenseTrackStore.inverse: out must be contiguous (float32 {list(lead + (H, W, 4))}, int32 "
                             f"{list(lead + (H, W))}) tensors on {self.device}")
        G = len(slots)
        if G == 0:
            return table, cell
        if self.native:
            from . import ops
            ops.trackstore_invert(self._chunks, self._lohi, slots, table.view(G, H, W, 4), cell.view(G, H, W), occlusion_threshold)
        else:
            grid = self._pixel_grid()
            tb, cl = table.view(G, H * W, 4), cell.view(G, H * W)
            for k, slot in enumerate(slots):
                self.locate(grid, self.frame_ids[slot], occlusion_threshold, out=(tb[k], cl[k]))
        return table, cell

    def results_from(self, src, frames=None, occlusion_threshold=0.5):
        """The dense results FROM stored frame ``src`` to ``frames`` (a sequence of stored frame ids; default: all, in append
        order) -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W], found [H, W] bool) on the store's device.
        Pixel p = (x, y) of ``src`` is taken back to its template point by ``inverse(src)`` -- (Px, Py, o_src, s_src) -- and that
        point forward by ``query`` -- (qx, qy, o_dst, s_dst) on frame t: flow = (qx - x, qy - y), occlusion = max(o_src, o_dst),
        sigma = sqrt(s_src^2 + s_dst^2), the rule by which results are chained (MFT/MFT.py:233-239) with the inverse as the left
        result.  A pixel nothing maps to has found False, NaN flow, occlusion 1 and sigma +inf.  On the device the read-out and the
        chaining are ONE ``mftx_trackstore_flow_from`` call behind ``inverse`` (a one-row table, every found pixel entry 0), bit for
        bit the composition below.  No host synchronisation."""
        H, W = self.H, self.W
        slots = self._slots(frames)                             # KeyError before any work
        table, cell = self.inverse(src, occlusion_threshold)
        if self.native:
            from . import ops
            T = len(slots)
            flow = torch.empty((T, 2, H, W), dtype=torch.float32, device=self.device)
            occl, sigma = (torch.empty((T, 1, H, W), dtype=torch.float32, device=self.device) for _ in range(2))
            found = cell >= 0
            if T:
                entry = torch.where(found, 0, -1).to(torch.int32)
                frame_ptrs, lohi_ptrs = ops.trackstore_slot_addresses(self._chunks, self._lohi, slots)
                ops.trackstore_flow_from(table, entry, [0], frame_ptrs[None], lohi_ptrs[None], flow, occl, sigma)
            return flow, occl, sigma, found
        table, found = table.view(H * W, 4), cell.view(H * W) >= 0
        zero = torch.zeros((), dtype=torch.float32, device=self.device)
        template = torch.where(found[:, None], table[:, 0:2], zero)
        q = self.query(template, [self.frame_ids[s] for s in slots])                     # [H * W, T, 4]
        T = int(q.shape[1])
        flow, occl, sigma = chain_behind_inverse(table, q, self._pixel_grid(), found)
        return flow.reshape(T, 2, H, W), occl.reshape(T, 1, H, W), sigma.reshape(T, 1, H, W), found.view(H, W)

    def result_from(self, src, dst, occlusion_threshold=0.5):
        """-> (``FlowOUTrackingResult`` of the flow from stored frame ``src`` to stored frame ``dst``, found [H, W] bool): one
        frame of ``results_from``, ready for ``warp_forward_device`` / ``warp_backward`` (mask the pixels that are not found:
        their flow is NaN)."""
        flow, occl, sigma, found = self.results_from(src, [dst], occlusion_threshold)
        return FlowOUTrackingResult(flow[0], occl[0], sigma[0], validate=False), found

    # ------------------------------------------------------------------ the video read along the tracks
    def _sample_image(self, result, img, px, py):
        """img float32 [C, H, W] sampled at (px, py) [H, W] = pixel + ``result.flow``: ``result.warp_backward(img)`` -- on the device
        ``mftx_warp_backward``, on the host the reference's own formulation (MFT/results.py:116-136), torch's ``grid_sample``."""
        if self.native:
            return result.warp_backward(img)
        from .results import _normalize_coords
        normed = _normalize_coords(torch.stack([px, py], dim=-1)[None], self.H, self.W)
        return torch.nn.functional.grid_sample(img[None], normed, align_corners=True)[0]

    def _compose_appearance(self, slots, images, reference, occlusion_threshold, sigma_max, stack, fill):
        """The definition of ``appearance`` as a composition, column after column, in torch on the store's device (``images`` and
        ``reference`` are there already) -> (sum, sumsq, count, warped, visible).  The host store's path; on a device store what the
        fused kernel is held to bit for bit (tests/test_gpu_track_appearance.py)."""
        H, W, dev, T = self.H, self.W, self.device, len(slots)
        C = int(images.shape[3]) if isinstance(images, torch.Tensor) else int(images[0].shape[2])
        ref = torch.zeros((C, H, W), dtype=torch.float32, device=dev) if reference is None else reference.permute(2, 0, 1).to(torch.float32)
        xs = torch.arange(W, dtype=torch.float32, device=dev)[None, :].expand(H, W)
        ys = torch.arange(H, dtype=torch.float32, device=dev)[:, None].expand(H, W)
        smax = float("inf") if sigma_max is None else float(sigma_max)
        total, totalsq = (torch.zeros((C, H, W), dtype=torch.float32, device=dev) for _ in range(2))
        count = torch.zeros((H, W), dtype=torch.int32, device=dev)
        warped = torch.empty((T, H, W, C), dtype=torch.uint8, device=dev) if stack else None
        visible = torch.empty((T, H, W), dtype=torch.bool, device=dev) if stack else None
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        filled = torch.full((), int(fill), dtype=torch.uint8, device=dev)
        for k, slot in enumerate(slots):
            r = self._result_of_slot(slot)
            px, py = xs + r.flow[0], ys + r.flow[1]
            c = self._sample_image(r, images[k].permute(2, 0, 1).to(torch.float32).contiguous(), px, py)
            vis = (r.occlusion[0] <= occlusion_threshold) & (r.sigma[0] <= smax) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
            d = c - ref
            total = torch.where(vis, total + d, total)              # (d * d is a product of its own: nothing here contracts)
            totalsq = torch.where(vis, totalsq + d * d, totalsq)
            count += vis
            if stack:
                level = torch.where(vis, c, zero).clamp(0, 255).round().to(torch.uint8)           # (round: ties to even)
                warped[k] = torch.where(vis[:, :, None], level.permute(1, 2, 0), filled)
                visible[k] = vis
        return total, totalsq, count, warped, visible

    def appearance(self, images, frames=None, reference=None, occlusion_threshold=0.5, sigma_max=None, stack=False, fill=0):
        """The video read along every track: per template pixel, what the frames show where the pixel goes -> ``TrackAppearance``.

        frames: stored frame ids (default: all, in append order; an id may come more than once, and then counts as often);
        images: a sequence of T images, ``images[k]`` belonging to ``frames[k]``, each (H, W, C) uint8 with C = 1 .. 4 -- numpy arrays
        or tensors on any device (moved to the store's) -- or ONE uint8 tensor [T, H, W, C]; reference: (H, W, C) uint8, usually
        the template frame, or None (= 0).  A ``KeyError`` for a frame that was never appended and a ``ValueError`` for a wrong
        shape, dtype, C or fill come before any work.

        For column k with r = ``result(frames[k])``, at template pixel (x, y): px = x + r.flow[0], py = y + r.flow[1];
        c = ``r.warp_backward(images[k] as float32 [C, H, W])`` -- the bilinear sample at (px, py), 0 outside;
        visible = (occlusion <= occlusion_threshold) & (sigma <= sigma_max) & (0 <= px <= W - 1) & (0 <= py <= H - 1), every
        comparison false on NaN (``sigma_max=None``: +inf, which lets a +inf sigma pass); d = c - reference; and over k in the order
        of ``frames``, in float32: sum += d, sumsq += d * d, count += 1 where visible.  With ``stack=True`` also
        warped[k] = uint8(rint(clamp(c, 0, 255))) where visible and ``fill`` elsewhere -- the video stabilised to the template --
        and visible[k].

        The sums are taken RELATIVE to ``reference`` to keep float32 meaningful: with the template frame as the reference d is a
        photometric residual of a few levels, whose squares sum exactly enough over hundreds of frames; raw sums of squares of
        values up to 255 (65025 each) would leave float32 a handful of significant levels.  ``mean`` = reference + sum / count (a
        clean plate) and ``var`` of the result are derived from them.

        On the device: one table upload and ONE ``mftx_trackstore_appearance`` launch whatever T is (csrc/trackstore.hip:
        ts_appearance_kernel: 8 + C bytes read per pixel and frame, no float stack materialised), bit for bit the composition
        above (``_compose_appearance``); no host synchronisation when ``images`` are device tensors.  The host store runs the
        composition with torch's ``grid_sample``: count and visible are EQUAL to the device's, the samples differ by the samplers'
        order of operations."""
        name = "DenseTrackStore.appearance"
        slots = self._slots(frames)                             # KeyError before any work
        H, W, T = self.H, self.W, len(slots)
        images, C = _as_images(images, T, H, W, name)
        if reference is not None:
            if isinstance(reference, np.ndarray) and reference.dtype == np.uint8:
                reference = torch.from_numpy(np.ascontiguousarray(reference))
            if not isinstance(reference, torch.Tensor) or reference.dtype != torch.uint8 or reference.dim() != 3 \
                    or tuple(reference.shape[:2]) != (H, W) or not 1 <= int(reference.shape[2]) <= 4 or (T and int(reference.shape[2]) != C):
                raise ValueError(f"{name}: reference must be uint8 ({H}, {W}, C) with the images' C")
            C = int(reference.shape[2])
        if not 0 <= int(fill) <= 255:
            raise ValueError(f"{name}: fill must be 0 .. 255")
        C = C or 1                                              # (no image and no reference: one channel of zeros)
        dev = self.device
        images = images.to(dev).contiguous() if isinstance(images, torch.Tensor) else [i.to(dev).contiguous() for i in images]
        reference = None if reference is None else reference.to(dev).contiguous()
        ids = [self.frame_ids[s] for s in slots]
        if T == 0:
            z = torch.zeros((2, C, H, W), dtype=torch.float32, device=dev)
            return TrackAppearance(ids, torch.zeros((H, W), dtype=torch.int32, device=dev), z[0], z[1], reference,
                                   torch.zeros((0, H, W, C), dtype=torch.uint8, device=dev) if stack else None,
                                   torch.zeros((0, H, W), dtype=torch.bool, device=dev) if stack else None)
        if self.native:
            from . import atlas_ops, ops
            total, totalsq = (torch.empty((C, H, W), dtype=torch.float32, device=dev) for _ in range(2))
            count = torch.empty((H, W), dtype=torch.int32, device=dev)
            warped = torch.empty((T, H, W, C), dtype=torch.uint8, device=dev) if stack else None
            visible = torch.empty((T, H, W), dtype=torch.bool, device=dev) if stack else None
            frame_ptrs, lohi_ptrs = ops.trackstore_slot_addresses(self._chunks, self._lohi, slots)
            atlas_ops.trackstore_appearance(frame_ptrs, lohi_ptrs, images, reference, total, totalsq, count, warped, visible,
                                            occlusion_threshold, sigma_max, fill)
        else:
            total, totalsq, count, warped, visible = self._compose_appearance(slots, images, reference, occlusion_threshold, sigma_max,
                                                                              stack, fill)
        return TrackAppearance(ids, count, total, totalsq, reference, warped, visible)
