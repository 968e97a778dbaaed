"""Overlays of the demo (``demo.py:116-146``) without OpenCV: tracked-point dots and the first-frame edit carried
along the tracked flow.  Visualisation only.  The functions are numpy on the host, the splatting itself is
``FlowOUTrackingResult.warp_forward`` (``MFT/results.py:190-248``); ``DeviceOverlay`` renders the same two overlays with
libmftx's splat kernels from results that stay on the device."""
from __future__ import annotations

import numpy as np
import torch

RED = (0, 0, 255)          # BGR, MFT/utils/vis_utils.py:27


def to_gray_3ch(img):
    """BGR uint8 -> 3-channel gray (cv2.cvtColor BGR2GRAY -> GRAY2BGR, MFT/utils/vis_utils.py:240-242):
    Y = 0.299 R + 0.587 G + 0.114 B in cv2's 14-bit fixed point (4899, 9617, 1868), rounded."""
    img = np.asarray(img).astype(np.int64)
    y = (img[..., 0] * 1868 + img[..., 1] * 9617 + img[..., 2] * 4899 + (1 << 13)) >> 14
    return np.repeat(y.astype(np.uint8)[..., None], 3, axis=2)


def blend_with_alpha_premult(img1_premult, img2, img1_alpha):
    """MFT/utils/vis_utils.py:755-765."""
    img1_alpha = np.asarray(img1_alpha)
    if img1_alpha.max() > 1.0001:
        img1_alpha = img1_alpha.astype(np.float32) / 255.0
    if img1_alpha.ndim == 2:
        img1_alpha = img1_alpha[..., None]
    result = np.asarray(img1_premult).astype(np.float32) + np.asarray(img2).astype(np.float32) * (1 - img1_alpha)
    return result.clip(0, 255).astype(np.uint8)


def draw_dots(frame, coords, occlusions, radius=3, color=RED):
    """A filled dot at every visible tracked point (demo.py:116-126; occlusion > 0.5 = hidden).
    coords (N, 2) xy, occlusions (N,)."""
    canvas = np.array(frame, copy=True)
    H, W = canvas.shape[:2]
    coords = coords.detach().cpu().numpy() if isinstance(coords, torch.Tensor) else np.asarray(coords)
    occl = occlusions.detach().cpu().numpy() if isinstance(occlusions, torch.Tensor) else np.asarray(occlusions)
    r = int(np.ceil(radius))
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    for (x, y), o in zip(coords.reshape(-1, 2), occl.reshape(-1)):
        if o > 0.5 or not (np.isfinite(x) and np.isfinite(y)):
            continue
        cx, cy = int(round(float(x))), int(round(float(y)))
        disc = (dx + cx - x) ** 2 + (dy + cy - y) ** 2 <= (radius + 0.5) ** 2
        ys, xs = dy[disc] + cy, dx[disc] + cx
        ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
        canvas[ys[ok], xs[ok]] = color
    return canvas


def draw_edit(frame, result, edit):
    """The RGBA first-frame edit (``cv2.imread(..., IMREAD_UNCHANGED)``: B, G, R, A) splatted along the tracked flow
    onto the gray current frame, for template pixels that are visible and inside the edit (demo.py:128-146)."""
    edit = np.asarray(edit)
    visible = (result.occlusion[0] < 0.5).cpu()
    mask = torch.logical_and(visible, torch.from_numpy(edit[:, :, 3] > 0))
    alpha = edit[:, :, 3:4].astype(np.float32) / 255.0
    premult = edit[:, :, :3].astype(np.float32) * alpha
    color = np.clip(np.asarray(result.warp_forward(premult, mask=mask)), 0, 255).astype(np.uint8)
    alpha_t = np.asarray(result.warp_forward(edit[:, :, 3:4], mask=mask))
    return blend_with_alpha_premult(color, to_gray_3ch(frame), alpha_t)


def get_queries(frame_shape, spacing):
    """Regular grid of query points, (N, 2) xy float32 (demo.py:105-114)."""
    H, W = frame_shape
    xs, ys = np.meshgrid(np.arange(0, W, spacing), np.arange(0, H, spacing))
    return torch.from_numpy(np.vstack((xs.flatten(), ys.flatten())).T).float()


class DeviceOverlay:
    """The two demo overlays rendered on the GPU, frame by frame, from device results (``csrc/splat.hip``): per ``render``
    one ``sample_points`` launch, the dots (``ops.overlay_dots``) and the edit splat + composite (``ops.overlay_edit``), all
    on the caller's current stream, then copy kernels into a small ring of pinned host buffers.  Nothing here waits on the
    host; ``download`` hands finished frames back as numpy arrays.  The point frames are bitwise ``draw_dots`` on the
    sampled tracks; the edit frames are ``draw_edit`` up to the last level of its float-to-uint8 truncation (the sums here
    are integers: the same frame every run).

    edit: (H, W, 4) uint8 B, G, R, A, or None (``render`` then returns None for the edit frame); queries: (N, 2) xy."""

    def __init__(self, edit, queries, H, W, radius=3, color=RED, depth=4, device="cuda"):
        from . import ops
        self.H, self.W, self.radius, self.color = int(H), int(W), radius, tuple(color)
        self.device = torch.device(device)
        q = queries if isinstance(queries, torch.Tensor) else torch.from_numpy(np.asarray(queries))
        self.queries = q.to(self.device, torch.float32).reshape(-1, 2).contiguous()
        self._tmpl = torch.zeros(self.queries.shape[0], dtype=torch.int32, device=self.device)
        self.edit = None
        if edit is not None:
            edit = np.ascontiguousarray(edit)
            assert edit.shape == (self.H, self.W, 4) and edit.dtype == np.uint8, "edit must be (H, W, 4) uint8"
            self.alpha_div = ops.edit_alpha_divisor(edit)
            self.edit = torch.from_numpy(edit).to(self.device)
            self.acc = ops.splat_accumulator(4, self.H, self.W, self.device)    # every composite leaves it zeroed again
        self._free = [self._new_slot() for _ in range(depth)]       # pinning is slow: once, here
        self._queue, self._n = [], 0

    def _new_slot(self):
        H, W, N = self.H, self.W, int(self.queries.shape[0])
        dev = lambda: torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)              # noqa: E731
        host = lambda: torch.empty(H, W, 3, dtype=torch.uint8, pin_memory=True)                # noqa: E731
        slot = {"frame": dev(), "points": dev(), "h_points": host(), "event": None, "index": -1,
                "table": torch.zeros(max(N, 1), 4, dtype=torch.float32, device=self.device)[:N],
                "h_table": torch.zeros(max(N, 1), 4, dtype=torch.float32, pin_memory=True)[:N]}
        if self.edit is not None:
            slot["edit"], slot["h_edit"] = dev(), host()
        return slot

    def _frame_on_device(self, frame, slot):
        from . import ops
        if not isinstance(frame, torch.Tensor):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        assert tuple(frame.shape) == (self.H, self.W, 3) and frame.dtype == torch.uint8, "frame must be (H, W, 3) uint8"
        if frame.is_cuda:
            return frame.contiguous()
        if frame.is_pinned() and frame.is_contiguous() and frame.data_ptr() % 16 == 0:
            return ops.copy_bytes(frame, slot["frame"])
        slot["frame"].copy_(frame, non_blocking=True)         # pageable memory: torch stages it
        return slot["frame"]

    def render(self, frame, result):
        """frame: (H, W, 3) uint8 BGR -- a device tensor, a pinned host tensor (uploaded by a copy kernel) or an array;
        result: the frame's device ``FlowOUTrackingResult``.  Enqueues everything and returns the DEVICE tensors
        (points_u8, edit_u8), valid until ``download`` has handed the frame out and the ring comes round."""
        from . import ops
        slot = self._free.pop(0) if self._free else self._new_slot()
        fr = self._frame_on_device(frame, slot)
        flow, occl, sigma = (t.to(torch.float32).contiguous() for t in result.planes())
        if self.queries.shape[0]:
            ops.sample_points([(flow, occl, sigma)], self._tmpl, self.queries, slot["table"], 0)
            ops.copy_bytes(slot["table"], slot["h_table"])
        ops.overlay_dots(fr, slot["table"], self.radius, self.color, out=slot["points"])
        ops.copy_bytes(slot["points"], slot["h_points"])
        if self.edit is not None:
            ops.overlay_edit(flow, occl, self.edit, fr, self.acc, self.alpha_div, out=slot["edit"])
            ops.copy_bytes(slot["edit"], slot["h_edit"])
        slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(self.device))
        slot["index"], self._n = self._n, self._n + 1
        self._queue.append(slot)
        return slot["points"], slot.get("edit")

    def pending(self):
        return len(self._queue)

    def download(self, wait=False, tracks=False):
        """The frames rendered so far whose copies have landed, oldest first, as [(points_u8, edit_u8 | None), ...] numpy
        arrays (with ``tracks``: a third entry, the (N, 4) table x, y, occlusion, sigma the dots were drawn from).
        Never blocks unless ``wait``: then every pending frame is waited for."""
        out = []
        while self._queue:
            slot = self._queue[0]
            if wait:
                slot["event"].synchronize()
            elif not slot["event"].query():
                break
            self._queue.pop(0)
            item = (slot["h_points"].numpy().copy(), slot["h_edit"].numpy().copy() if self.edit is not None else None)
            if tracks:
                item += (slot["h_table"].numpy().copy(),)
            out.append(item)
            self._free.append(slot)
        return out
