"""TrackAtlas -- several ``DenseTrackStore``s of ONE video joined into one answer: every pixel of any frame followed.

A ``DenseTrackStore`` answers every question about one template in one time direction, so ``locate`` / ``inverse`` return "not
found" wherever no point of THAT template maps to -- a disoccluded region, something that entered the video after the template
frame -- and a template in the middle of a video has its forward and backward halves in two stores.  An atlas holds one entry
``(template_frame, store)`` per store and answers from whichever entry sees the query best::

    atlas = TrackAtlas.from_passes(forward_pass, backward_pass)       # every store of MultiTemplateMFT passes (C.multi_template_stores)
    atlas = TrackAtlas([(template_frame, store), ...])                # or any DenseTrackStores, e.g. MFT.track_store of single runs
    table, cell, entry = atlas.locate(points, 57)                     # device [N, 4], [N], [N]; frame: one id or N ids
    table, cell, entry = atlas.inverse(57)                            # device [H, W, 4], [H, W], [H, W]; a list of G frames: [G, ...]
    tracks = atlas.query(template_frame, points, frames=None)         # device [N, T, 4]: points given ON that template frame
    coords, occl, found, template = atlas.tracks_from(points, 57)     # numpy (N, T, 2), (N, T), (N,), (N,): ONE download
    flow, occl, sigma, found, template = atlas.results_from(57)       # device [T, 2, H, W], [T, 1, H, W] x 2, [H, W] x 2: EVERY pixel
    result, found, template = atlas.result_from(57, 80)               # ... one column as a FlowOUTrackingResult
    flow, occl, sigma, entry, template = atlas.best_results_from(57)  # ... the template chosen per pixel AND column: [T, H, W] x 2
    result, found, template = atlas.best_result_from(57, 12)          # ... one column of that
    table, entry, template = atlas.best_query_from(points, 57)        # device [N, T, 4], [N, T] x 2: that choice for POINTS; frame: one id or N ids
    coords, occl, found, template = atlas.best_tracks_from(points, 57)  # numpy (N, T, 2), (N, T) x 3: ONE download
    atlas.covered(template_frame)                                    # list of bool: the frames some entry of that template holds

The definition (and the ``device="cpu"`` path; there is no new arithmetic): for a query on frame ``f`` every entry whose store holds
``f`` answers with its own ``store.locate(point, f, thr)``; among the entries that found it the smallest
``(occlusion > thr, bits of (sigma > 0 ? sigma : +0), rank)`` wins -- ``locate``'s own key with the rank put between sigma and cell:
visible before occluded, then lowest sigma as MFT's selection has it, then the earliest template.  ``occlusion`` and ``sigma`` are
the row's values.  Entries are ranked by ``(template_frame, position in the argument)``.  On a template's own frame its identity
result has sigma 0, so that template wins wherever it is visible.

On the device the sparse ``locate`` is ONE ``mftx_trackstore_locate`` call (the points repeated per entry, the entries' frames as
its groups) and a reduction by that key; the dense ``inverse`` is ONE ``mftx_trackstore_invert_atlas`` call, which scatters all
entries of a video frame onto one key plane.  The two are different code and agree bit for bit.

``results_from`` is the dense counterpart of ``tracks_from``: ``inverse``, then every pixel's template point followed by ``query`` on
its own winner's template and chained behind the inverse as ``DenseTrackStore.results_from`` chains.  On the device that second
step is ONE ``mftx_trackstore_flow_from`` call, which goes from the inverse's plane straight to planar results.

``results_from`` picks ONE entry per source pixel and follows it through every column, so a column that entry's template does not
cover is fill even where another template sees the pixel and holds the column -- from a template's own frame back to an earlier
frame that is every pixel.  ``best_results_from`` makes every entry that holds the source frame a candidate and lets the smallest
(occluded, chained sigma, rank) win each (pixel, column): per-entry inverses, then ONE ``mftx_trackstore_flow_from_best`` launch
(mft_amd/atlas_ops.py).

``tracks_from`` has ``results_from``'s rule for sparse points, and ``best_query_from`` / ``best_tracks_from`` are its
``best_results_from``: per (point, column) the same key among all entries that hold the point's frame, each candidate with its OWN
``store.locate`` row, the position chained in the place of the flow.  The points may be given on several frames in one call.  On the
device: the ``mftx_trackstore_locate`` call of ``locate`` with its rows kept un-reduced, then ONE
``mftx_trackstore_tracks_from_best`` launch (mft_amd/atlas_ops.py) over tiles of at most 64 points of one source frame.
"""
from __future__ import annotations

import numpy as np
import torch

from .trackstore import _as_points, _frame_ids, _tracks_to_host, chain_behind_inverse

MAX_ENTRIES = 256                 # 8 bits of the dense inverse's key
MAX_CELLS = 1 << 24               # ... and 24 for the cell: (H - 1)(W - 1)
_NOT_FOUND = torch.iinfo(torch.int64).max


def _same_device(a, b):
    """'cuda' and 'cuda:0' name one card when 0 is the current device: an index that is not given is the current one."""
    if a.type != b.type:
        return False
    if a.index == b.index or a.type != "cuda":
        return a.index == b.index
    current = torch.cuda.current_device()
    return (current if a.index is None else a.index) == (current if b.index is None else b.index)


class TrackAtlas:
    def __init__(self, entries):
        """entries: a sequence of ``(template_frame, DenseTrackStore)``, all stores of one H x W and on one device, each store's
        first frame being its template frame (``ValueError`` otherwise, and for more than 256 entries or more than 2^24 cells)."""
        entries = [(int(f), st) for f, st in entries]
        if not entries:
            raise ValueError("TrackAtlas: no entries")
        if len(entries) > MAX_ENTRIES:
            raise ValueError(f"TrackAtlas: {len(entries)} entries; at most {MAX_ENTRIES}")
        first = entries[0][1]
        self.H, self.W, self.device = first.H, first.W, first.device
        if (self.H - 1) * (self.W - 1) > MAX_CELLS:
            raise ValueError(f"TrackAtlas: {self.H} x {self.W} frames have more than 2^24 cells")
        for f, st in entries:
            if (st.H, st.W) != (self.H, self.W) or not _same_device(st.device, self.device):
                raise ValueError(f"TrackAtlas: all stores must be {self.H} x {self.W} on {self.device}, not {st.H} x {st.W} on {st.device}")
            if len(st) == 0 or st.frame_ids[0] != f:
                raise ValueError(f"TrackAtlas: the first frame of template {f}'s store must be frame {f} itself "
                                 f"(it holds {st.frame_ids[:1] or 'nothing'})")
        order = sorted(range(len(entries)), key=lambda i: (entries[i][0], i))
        self.entries = [entries[i] for i in order]                      # entries[rank] = (template_frame, store)
        self.frames = sorted(set().union(*[st.frame_ids for _, st in self.entries]))

    @classmethod
    def from_passes(cls, *passes):
        """Every store of ``MultiTemplateMFT`` passes of ONE video (``C.multi_template_stores``: ``pass.track_stores``), in the order
        the passes are given: a template run forward and backward has its forward store at the lower rank."""
        return cls([(s, st) for p in passes for s, st in p.track_stores.items()])

    # ------------------------------------------------------------------ helpers
    @property
    def native(self):
        return self.device.type != "cpu"

    def _holders(self, f):
        """The ranks of the entries whose store holds frame ``f``, ascending (``KeyError`` if none does)."""
        ranks = [r for r, (_, st) in enumerate(self.entries) if int(f) in st._slot_of]
        if not ranks:
            raise KeyError(f"TrackAtlas: no entry holds frame {int(f)}")
        return ranks

    def _frame_views(self, rank, f):
        st = self.entries[rank][1]
        slot = st.slot_of(f)
        return st.packed(slot), st.lohi(slot)

    def _upload(self, a):
        """A small host array -> the atlas's device, through pinned memory: no host synchronisation."""
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.pin_memory().to(self.device, non_blocking=True) if self.native else t

    def _reduce(self, tq, cq, ranks, thr):
        """tq [E, n, 4], cq [E, n]: the answers of the entries ``ranks`` (ascending) to n queries -> the winner's (table [n, 4],
        cell [n], entry [n]) by the smallest (occlusion > thr, bits of (sigma > 0 ? sigma : +0), rank) among the entries that
        found the query."""
        zero = torch.zeros((), dtype=torch.float32, device=self.device)
        s = tq[:, :, 3]
        bits = torch.where(s > 0, s, zero).contiguous().view(torch.int32).to(torch.int64)
        occluded = (tq[:, :, 2] > torch.tensor(thr, dtype=torch.float32)).to(torch.int64)
        rk = self._upload(np.asarray(ranks, dtype=np.int64))
        key = (occluded << 39) | (bits << 8) | rk[:, None]
        key = torch.where(cq >= 0, key, torch.full((), _NOT_FOUND, dtype=torch.int64, device=self.device))
        best, arg = key.min(dim=0)                      # (the keys of the entries that found a query differ in the rank)
        found = best != _NOT_FOUND
        row = tq.gather(0, arg[None, :, None].expand(1, -1, 4))[0]
        cell = cq.gather(0, arg[None, :])[0]
        nan = torch.full((), float("nan"), dtype=torch.float32, device=self.device)
        minus = torch.full((), -1, dtype=torch.int32, device=self.device)
        return (torch.where(found[:, None], row, nan), torch.where(found, cell, minus),
                torch.where(found, (best & 0xff).to(torch.int32), minus))

    # ------------------------------------------------------------------ locate
    def locate(self, points, frame, occlusion_threshold=0.5):
        """points (N, 2) xy given ON video frame(s) ``frame`` -- one frame id, or a host sequence of N ids -> (table [N, 4], cell [N],
        entry [N]) on the atlas's device: the winning entry's ``store.locate`` row (ITS template's x, y, occlusion, sigma) and
        cell, and its rank (``atlas.entries[rank]``).  Where no entry finds the query: entry = cell = -1 and a row of NaN.  A
        frame that no entry holds is a ``KeyError``.  On the device: one kernel call and a reduction, and with ``points`` a
        device tensor no host synchronisation."""
        xy = _as_points(points, self.device, "TrackAtlas.locate")
        N = int(xy.shape[0])
        ids, lead = _frame_ids(frame, "TrackAtlas.locate", N)
        if lead:
            groups = [(int(f), np.flatnonzero(ids == f)) for f in np.unique(ids)]
        else:
            groups = [(int(ids[0]), None)]                                      # (frame, the points given on it: all)
        holders = [self._holders(f) for f, _ in groups]                        # KeyError before any work
        table = torch.empty((N, 4), dtype=torch.float32, device=self.device)
        cell = torch.empty((N,), dtype=torch.int32, device=self.device)
        entry = torch.empty((N,), dtype=torch.int32, device=self.device)
        if N == 0:
            return table, cell, entry
        thr = float(occlusion_threshold)
        if self.native:
            from . import ops
            # one call: the queries of group after group, within a group entry after entry, each entry's frame a group of the kernel's
            views, which, index = [], [], []
            for (f, pts), ranks in zip(groups, holders):
                n = N if pts is None else len(pts)
                for r in ranks:
                    which.append(np.full(n, len(views), np.int64))
                    views.append(self._frame_views(r, f))
                    index.append(np.arange(N) if pts is None else pts)
            if not lead:
                xq = xy.repeat(len(views), 1)
            else:
                xq = xy.index_select(0, self._upload(np.concatenate(index).astype(np.int64)))
            Q = int(xq.shape[0])
            tq = torch.empty((Q, 4), dtype=torch.float32, device=self.device)
            cq = torch.empty((Q,), dtype=torch.int32, device=self.device)
            ops.trackstore_locate_frames(views, np.concatenate(which), xq, tq, cq, thr)
        q0 = 0
        for (f, pts), ranks in zip(groups, holders):
            n, E = N if pts is None else len(pts), len(ranks)
            if self.native:
                t, c = tq[q0:q0 + E * n].view(E, n, 4), cq[q0:q0 + E * n].view(E, n)
                q0 += E * n
            else:
                x = xy if pts is None else xy[torch.from_numpy(pts)]
                answers = [self.entries[r][1].locate(x, f, thr) for r in ranks]
                t, c = torch.stack([a[0] for a in answers]), torch.stack([a[1] for a in answers])
            wt, wc, we = self._reduce(t, c, ranks, thr)
            if pts is None:
                table, cell, entry = wt, wc, we
            else:
                at = self._upload(pts.astype(np.int64))
                table.index_copy_(0, at, wt)
                cell.index_copy_(0, at, wc)
                entry.index_copy_(0, at, we)
        return table, cell, entry

    # ------------------------------------------------------------------ the dense inverse
    def inverse(self, frame, occlusion_threshold=0.5):
        """Video frame ``frame`` inverted at every pixel: ``locate`` with the H * W pixel centres as its points, bit for bit ->
        (table [H, W, 4], cell [H, W], entry [H, W]) on the atlas's device; a sequence of G frame ids gives [G, H, W, 4] and
        [G, H, W].  On the device: ONE call whatever G and the number of entries are (``mftx_trackstore_invert_atlas``: all
        entries of a frame scattered onto one key plane, 8 + 28 bytes per pixel and plane of workspace and results instead of that per
        entry), and no host synchronisation."""
        ids, lead = _frame_ids(frame, "TrackAtlas.inverse")
        fs = [int(f) for f in ids]
        holders = [self._holders(f) for f in fs]                               # KeyError before any work
        H, W, G = self.H, self.W, len(fs)
        table = torch.empty((G, H, W, 4), dtype=torch.float32, device=self.device)
        cell = torch.empty((G, H, W), dtype=torch.int32, device=self.device)
        entry = torch.empty((G, H, W), dtype=torch.int32, device=self.device)
        if G and self.native:
            from . import ops
            views = [self._frame_views(r, f) for f, ranks in zip(fs, holders) for r in ranks]
            first_of = np.concatenate([[0], np.cumsum([len(ranks) for ranks in holders])])
            ops.trackstore_invert_atlas(views, first_of, [r for ranks in holders for r in ranks], table, cell, entry,
                                        float(occlusion_threshold))
        elif G:
            grid = self.entries[0][1]._pixel_grid()
            for g, f in enumerate(fs):
                t, c, e = self.locate(grid, f, occlusion_threshold)
                table[g], cell[g], entry[g] = t.view(H, W, 4), c.view(H, W), e.view(H, W)
        return table.view(lead + (H, W, 4)), cell.view(lead + (H, W)), entry.view(lead + (H, W))

    # ------------------------------------------------------------------ forward read-out
    def _columns(self, template_frame, frames):
        """-> (frames, per column the rank of the lowest-ranked entry of that template that holds the frame, or -1)."""
        ranks = [r for r, (f, _) in enumerate(self.entries) if f == int(template_frame)]
        if not ranks:
            raise KeyError(f"TrackAtlas: no entry of template frame {int(template_frame)}")
        frames = list(self.frames) if frames is None else [int(f) for f in frames]
        return frames, [next((r for r in ranks if f in self.entries[r][1]._slot_of), -1) for f in frames]

    def query(self, template_frame, points, frames=None):
        """points (N, 2) xy given ON template frame ``template_frame``, followed through ``frames`` (default: ``atlas.frames``) ->
        float32 [N, T, 4] on the atlas's device: per column ``store.query`` of the lowest-ranked entry of that template that
        holds the frame -- which joins a forward and a backward store of one template -- and a row of NaN for a frame that no
        entry of the template holds.  ``KeyError`` for a template frame without an entry.  No host synchronisation."""
        frames, owner = self._columns(template_frame, frames)
        xy = _as_points(points, self.device, "TrackAtlas.query")
        N, T = int(xy.shape[0]), len(frames)
        out = torch.full((N, T, 4), float("nan"), dtype=torch.float32, device=self.device)
        if N == 0:
            return out
        for r in sorted(set(owner) - {-1}):
            cols = [k for k, o in enumerate(owner) if o == r]
            part = self.entries[r][1].query(xy, [frames[k] for k in cols])
            if len(cols) == T:
                return part
            out.index_copy_(1, self._upload(np.asarray(cols, dtype=np.int64)), part)
        return out

    def tracks_from(self, points, frame, frames=None, occlusion_threshold=0.5):
        """points given on video frame(s) ``frame`` (as for ``locate``), followed over ``frames`` (default: ``atlas.frames``) -> numpy
        (coords [N, T, 2], occlusion [N, T], found [N], template [N]): ``locate``, then ``query`` of the located template points
        on the winner's template.  Columns the winner's template does not cover and points that are not found get NaN
        coordinates and occlusion 1; ``template`` is the winner's template frame, or -1.  ONE download; it synchronises.  To
        keep it at one download, ALL N points are read out on every distinct template frame of the atlas and each point keeps
        its winner's row: E_templates x N x T rows of work and E_templates temporary [N, T, 4] tables -- meant for sparse
        points (a click, a query grid), not for every pixel of a frame."""
        table, cell, entry = self.locate(points, frame, occlusion_threshold)
        N = int(table.shape[0])
        found = entry >= 0
        zero = torch.zeros((), dtype=torch.float32, device=self.device)
        at = torch.where(found[:, None], table[:, 0:2], zero)
        tmpl_of = self._upload(np.asarray([f for f, _ in self.entries], dtype=np.int64))
        minus = torch.full((), -1, dtype=torch.int64, device=self.device)
        template = torch.where(found, tmpl_of[entry.clamp(min=0).to(torch.int64)], minus)
        cols = list(self.frames) if frames is None else [int(f) for f in frames]
        T = len(cols)
        tracks = torch.full((N, T, 4), float("nan"), dtype=torch.float32, device=self.device)
        covered = {}
        for s in sorted({f for f, _ in self.entries}):
            covered[s] = np.asarray(self._columns(s, cols)[1]) >= 0
            if N and T:
                tracks = torch.where((template == s)[:, None, None], self.query(s, at, cols), tracks)
        tracks, template = _tracks_to_host(tracks, template)
        template = template.astype(np.int64)
        found = template >= 0
        coords, occl = tracks[:, :, 0:2].copy(), tracks[:, :, 2].copy()
        lost = np.ones((N, T), bool)
        for s, cov in covered.items():
            lost[template == s] = ~cov
        coords[lost], occl[lost] = np.nan, 1.0
        return coords, occl, found, template

    # ------------------------------------------------------------------ dense results from any frame
    def covered(self, template_frame, frames=None):
        """Per frame of ``frames`` (default: ``atlas.frames``) whether some entry of template ``template_frame`` holds it -- a list
        of bool: where it is False, ``query`` / ``results_from`` have nothing to read for that template ("not covered", as
        opposed to a point that is lost).  ``KeyError`` for a template frame without an entry."""
        return [r >= 0 for r in self._columns(template_frame, frames)[1]]

    def _templates(self):
        """-> (the distinct template frames, ascending; per rank the index of its template among them)."""
        templates = sorted({f for f, _ in self.entries})
        return templates, [templates.index(f) for f, _ in self.entries]

    def _flow_tables(self, cols):
        """The host tables of ``ops.trackstore_flow_from`` for the columns ``cols`` -> (row_of [ranks], frame_ptrs [R, T], lohi_ptrs
        [R, T]): a row per distinct template, column t holding the addresses of the stored frame ``query`` reads for that template
        and frame -- the lowest-ranked entry's that holds it -- and 0 where no entry of the template does."""
        from . import ops
        templates, row_of = self._templates()
        frame_ptrs, lohi_ptrs = np.zeros((len(templates), len(cols)), np.int64), np.zeros((len(templates), len(cols)), np.int64)
        for k, s in enumerate(templates):
            owner = np.asarray(self._columns(s, cols)[1], dtype=np.int64)
            for r in np.unique(owner[owner >= 0]):
                st = self.entries[r][1]
                at = np.flatnonzero(owner == r)
                frame_ptrs[k, at], lohi_ptrs[k, at] = ops.trackstore_slot_addresses(st._chunks, st._lohi, [st.slot_of(cols[c]) for c in at])
        return row_of, frame_ptrs, lohi_ptrs

    def _compose_results(self, table, entry, cols):
        """The definition of ``results_from`` in torch, on the atlas's device: table [H, W, 4] and entry [H, W] of ``inverse``, the
        located template points followed by ``query`` on each pixel's own template and chained behind the inverse by the rule
        (and the code) of ``DenseTrackStore.results_from`` -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W]).  Every
        pixel is read out on every distinct template and keeps its winner's row."""
        H, W, T = self.H, self.W, len(cols)
        N = H * W
        templates, row_of = self._templates()
        tb, rank = table.reshape(N, 4), entry.reshape(N)
        found = rank >= 0
        zero = torch.zeros((), dtype=torch.float32, device=self.device)
        at = torch.where(found[:, None], tb[:, 0:2], zero)
        row = self._upload(np.asarray(row_of, dtype=np.int64))[rank.clamp(min=0).to(torch.int64)]
        q = torch.full((N, T, 4), float("nan"), dtype=torch.float32, device=self.device)
        ok = torch.zeros((N, T), dtype=torch.bool, device=self.device)
        for k, s in enumerate(templates):
            mine = found & (row == k)
            cov = np.asarray(self.covered(s, cols), dtype=bool)
            if T and cov.any():
                q = torch.where(mine[:, None, None], self.query(s, at, cols), q)
                ok = torch.where(mine[:, None], self._upload(cov)[None, :], ok)
        flow, occl, sigma = chain_behind_inverse(tb, q, self.entries[0][1]._pixel_grid(), ok)
        return flow.reshape(T, 2, H, W), occl.reshape(T, 1, H, W), sigma.reshape(T, 1, H, W)

    def results_from(self, src, frames=None, occlusion_threshold=0.5, out=None):
        """The dense results FROM video frame ``src`` to ``frames`` (default: ``atlas.frames``), every pixel followed on the template
        that sees it best -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W], found [H, W] bool, template [H, W]
        int32) on the atlas's device.  ``inverse(src)`` takes pixel (x, y) back to its winner's template point (Px, Py, o_src,
        s_src); it is found iff an entry won it, and ``template`` is the winner's template frame (-1: not found).  That point is
        followed by ``query`` on the winner's template -- (qx, qy, o_dst, s_dst) per column -- and chained as
        ``DenseTrackStore.results_from`` chains: flow = (qx - x, qy - y), occlusion = max(o_src, o_dst), sigma =
        sqrt(s_src^2 + s_dst^2).  A pixel that is not found, and a found pixel in a column that no entry of its template holds
        (``covered``), get NaN flow, occlusion 1 and sigma +inf.  ``out``: a (flow, occlusion, sigma) triple of contiguous
        float32 tensors of those shapes on the atlas's device to write into.  ``KeyError`` for a ``src`` that no entry holds,
        ``ValueError`` for an ``out`` that does not fit, both before any work.  On the device: ``inverse``, one table upload
        and ONE ``mftx_trackstore_flow_from`` call; no host synchronisation."""
        self._holders(src)                                                      # KeyError before any work
        cols = list(self.frames) if frames is None else [int(f) for f in frames]
        H, W, T = self.H, self.W, len(cols)
        shapes = ((T, 2, H, W), (T, 1, H, W), (T, 1, H, W))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        else:
            out = tuple(out)
            if len(out) != 3 or any(not isinstance(o, torch.Tensor) or tuple(o.shape) != s or o.dtype != torch.float32 or
                                    not _same_device(o.device, self.device) or not o.is_contiguous() for o, s in zip(out, shapes)):
                raise ValueError(f"TrackAtlas.results_from: out must be contiguous float32 tensors {[list(s) for s in shapes]} on {self.device}")
        table, _, entry = self.inverse(src, occlusion_threshold)
        found = entry >= 0
        tmpl_of = self._upload(np.asarray([f for f, _ in self.entries], dtype=np.int32))
        template = torch.where(found, tmpl_of[entry.clamp(min=0).to(torch.int64)], torch.full((), -1, dtype=torch.int32, device=self.device))
        if T and self.native:
            from . import ops
            ops.trackstore_flow_from(table, entry, *self._flow_tables(cols), *out)
        elif T:
            for o, v in zip(out, self._compose_results(table, entry, cols)):
                o.copy_(v)
        return out[0], out[1], out[2], found, template

    def result_from(self, src, dst, occlusion_threshold=0.5):
        """-> (``FlowOUTrackingResult`` of the flow from video frame ``src`` to video frame ``dst``, found [H, W] bool, template
        [H, W] int32): one column of ``results_from``, ready for ``warp_forward_device`` / ``warp_backward`` (mask the pixels
        that are not found, and those whose template does not cover ``dst``: their flow is NaN).  ``KeyError`` for a ``src`` or
        a ``dst`` that no entry holds."""
        from .results import FlowOUTrackingResult
        self._holders(src)
        self._holders(dst)
        flow, occl, sigma, found, template = self.results_from(src, [dst], occlusion_threshold)
        return FlowOUTrackingResult(flow[0], occl[0], sigma[0], validate=False), found, template

    # ------------------------------------------------------------------ ... the template chosen per pixel AND destination frame
    def _entry_inverses(self, src, ranks, thr):
        """Every candidate's OWN dense inverse of frame ``src`` -> (tables [E, H, W, 4], cells [E, H, W]): ``store.inverse(src, thr)`` of
        the entries ``ranks``, bit for bit.  On the device ONE ``ops.trackstore_invert_atlas`` call with one entry per plane."""
        E, H, W = len(ranks), self.H, self.W
        tables = torch.empty((E, H, W, 4), dtype=torch.float32, device=self.device)
        cells = torch.empty((E, H, W), dtype=torch.int32, device=self.device)
        if self.native:
            from . import ops
            ops.trackstore_invert_atlas([self._frame_views(r, src) for r in ranks], np.arange(E + 1), ranks, tables, cells,
                                        torch.empty_like(cells), thr)
        else:
            for k, r in enumerate(ranks):
                self.entries[r][1].inverse(src, thr, out=(tables[k], cells[k]))
        return tables, cells

    def _compose_best(self, tables, cells, ranks, cols, thr):
        """The definition of ``best_results_from`` in torch, on the atlas's device: tables [E, H, W, 4] and cells [E, H, W] of
        ``_entry_inverses`` for the candidates ``ranks`` (ascending).  Candidate after candidate: its located template points
        followed by ``query`` on its template, chained behind ITS inverse by ``chain_behind_inverse``, keyed, and kept where the key
        is smaller than the best so far -> (flow [T, 2, H, W], occlusion [T, 1, H, W], sigma [T, 1, H, W], entry [T, H, W] int32)."""
        H, W, T = self.H, self.W, len(cols)
        N = H * W
        dev = self.device
        nan, one, inf, zero = (torch.full((), v, dtype=torch.float32, device=dev) for v in (float("nan"), 1.0, float("inf"), 0.0))
        flow, occl, sigma = nan.expand(T, 2, N).clone(), one.expand(T, N).clone(), inf.expand(T, N).clone()
        best = torch.full((T, N), _NOT_FOUND, dtype=torch.int64, device=dev)
        none = torch.full((), _NOT_FOUND, dtype=torch.int64, device=dev)
        limit = torch.tensor(thr, dtype=torch.float32, device=dev)
        grid = self.entries[0][1]._pixel_grid()
        for k, r in enumerate(ranks):
            s = self.entries[r][0]
            cov = np.asarray(self.covered(s, cols), dtype=bool)
            if not (T and cov.any()):
                continue
            tb, found = tables[k].reshape(N, 4), cells[k].reshape(N) >= 0
            ok = found[:, None] & self._upload(cov)[None, :]
            q = self.query(s, torch.where(found[:, None], tb[:, 0:2], zero), cols)
            f, o, sg = chain_behind_inverse(tb, q, grid, ok)                                    # [T, 2, N], [T, N], [T, N]
            field = torch.where(sg > 0, sg, zero).contiguous().view(torch.int32).to(torch.int64)
            field = torch.where(torch.isnan(sg), torch.full((), 0x7fffffff, dtype=torch.int64, device=dev), field)
            key = ((~(o <= limit)).to(torch.int64) << 39) | (field << 8) | int(r)
            key = torch.where(ok.t(), key, none)
            better = key < best
            best = torch.where(better, key, best)
            flow, occl, sigma = torch.where(better[:, None, :], f, flow), torch.where(better, o, occl), torch.where(better, sg, sigma)
        entry = torch.where(best != none, (best & 0xff).to(torch.int32), torch.full((), -1, dtype=torch.int32, device=dev))
        return flow.reshape(T, 2, H, W), occl.reshape(T, 1, H, W), sigma.reshape(T, 1, H, W), entry.reshape(T, H, W)

    def _best_tables(self, ranks, cols):
        """The host tables of ``atlas_ops.trackstore_flow_from_best`` -> (rank_of [E], row_of [E], frame_ptrs [R, T], lohi_ptrs [R, T])."""
        row_of, frame_ptrs, lohi_ptrs = self._flow_tables(cols)
        return list(ranks), [row_of[r] for r in ranks], frame_ptrs, lohi_ptrs

    def best_results_from(self, src, frames=None, occlusion_threshold=0.5, out=None):
        """``results_from`` with the template chosen per pixel AND destination frame -> (flow [T, 2, H, W], occlusion [T, 1, H, W],
        sigma [T, 1, H, W], entry [T, H, W] int32, template [T, H, W] int32) on the atlas's device.  ``results_from`` follows each
        pixel on the one entry that sees it best on ``src`` and fills the columns that entry's template does not cover, although
        another template may see the pixel on ``src`` AND hold the destination -- from a template's own frame back to an earlier
        frame that is every pixel.  Here the candidates are ALL entries that hold ``src``, in ascending rank; candidate k takes
        pixel p back by its own ``store.inverse(src)`` (it finds p iff its cell is >= 0), follows that template point by ``query``
        on its template and chains as ``results_from`` chains.  It has an answer for (p, column t) iff it finds p and its template
        covers t, and among those the smallest key wins,

            key = (occluded << 39) | (sigma_field << 8) | rank,   occluded = not (o <= occlusion_threshold),
            sigma_field = 0x7fffffff for a NaN sigma, the float32 bits of s for s > 0, 0 otherwise,

        with o and s the CHAINED occlusion and sigma: visible before occluded, then the lowest chained sigma, then the lowest rank.
        This is deliberately NOT ``locate``'s key in two respects: a NaN occlusion counts as occluded, and a NaN sigma sorts behind
        every number, +inf included -- in a choice among alternatives a NaN must never beat a number.  ``entry`` is the winner's
        rank and ``template`` its template frame; where no candidate has an answer: NaN flow, occlusion 1, sigma +inf, -1, -1.
        The winner of ``inverse`` is one of the candidates, so a pixel-column ``results_from`` answers is answered here, by a key
        that is no larger.  ``out``: a (flow, occlusion, sigma) triple as for ``results_from``; ``entry`` and ``template`` are
        allocated by the call.  ``KeyError`` for a ``src`` that no entry holds, ``ValueError`` for an ``out`` that does not fit, both
        before any work.  On the device: the E candidates' inverses in ONE ``mftx_trackstore_invert_atlas`` call (one entry per
        plane; 32 bytes of planes and workspace per pixel and candidate -- 84 MB for 10 candidates at 512 x 512, 2.1 GB for 32 at
        1080 x 1920 -- freed when the call returns), one table upload and ONE ``mftx_trackstore_flow_from_best`` launch; no host
        synchronisation."""
        ranks = self._holders(src)                                              # KeyError before any work
        cols = list(self.frames) if frames is None else [int(f) for f in frames]
        H, W, T = self.H, self.W, len(cols)
        shapes = ((T, 2, H, W), (T, 1, H, W), (T, 1, H, W))
        if out is not None:
            out = tuple(out)
            if len(out) != 3 or any(not isinstance(o, torch.Tensor) or tuple(o.shape) != s or o.dtype != torch.float32 or
                                    not _same_device(o.device, self.device) or not o.is_contiguous() for o, s in zip(out, shapes)):
                raise ValueError(f"TrackAtlas.best_results_from: out must be contiguous float32 tensors {[list(s) for s in shapes]} on {self.device}")
        thr = float(occlusion_threshold)
        if T:
            tables, cells = self._entry_inverses(src, ranks, thr)           # (before the results are allocated: its workspace is the peak)
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        entry = torch.full((T, H, W), -1, dtype=torch.int32, device=self.device)
        if T:
            if self.native:
                from . import atlas_ops
                atlas_ops.trackstore_flow_from_best(tables, cells, *self._best_tables(ranks, cols), *out, entry, thr)
            else:
                *planes, entry = self._compose_best(tables, cells, ranks, cols, thr)
                for o, v in zip(out, planes):
                    o.copy_(v)
        tmpl_of = self._upload(np.asarray([f for f, _ in self.entries], dtype=np.int32))
        template = torch.where(entry >= 0, tmpl_of[entry.clamp(min=0).to(torch.int64)], torch.full((), -1, dtype=torch.int32, device=self.device))
        return out[0], out[1], out[2], entry, template

    # ------------------------------------------------------------------ ... and per POINT and destination frame
    def _point_groups(self, frame, N, name):
        """``frame`` as for ``locate`` -> (groups: per distinct source frame, ascending, (frame, the rows of the points given on it, or
        None for all of them); holders: per group the ranks of its candidates).  ``KeyError`` for a frame that no entry holds."""
        ids, lead = _frame_ids(frame, name, N)
        if lead:
            groups = [(int(f), np.flatnonzero(ids == f)) for f in np.unique(ids)]
            if len(groups) == 1:
                groups = [(groups[0][0], None)]                              # (N ids of one frame: the points as they are)
        else:
            groups = [(int(ids[0]), None)]
        return groups, [self._holders(f) for f, _ in groups]

    def _locate_candidates(self, xy, groups, holders, thr):
        """Step A of ``best_query_from``: every candidate's OWN ``store.locate`` of its group's points, un-reduced -> (rows [Q, 4],
        cells [Q]): group after group and, within a group of n points, candidate after candidate (row = the group's first +
        k * n + i).  On the device ONE ``ops.trackstore_locate_frames`` call, the call ``locate`` makes."""
        N = int(xy.shape[0])
        sizes = [N if pts is None else len(pts) for _, pts in groups]
        Q = sum(n * len(ranks) for n, ranks in zip(sizes, holders))
        tq = torch.empty((Q, 4), dtype=torch.float32, device=self.device)
        cq = torch.empty((Q,), dtype=torch.int32, device=self.device)
        if Q == 0:
            return tq, cq
        if self.native:
            from . import ops
            views, which, index = [], [], []
            for (f, pts), ranks, n in zip(groups, holders, sizes):
                for r in ranks:
                    which.append(np.full(n, len(views), np.int64))
                    views.append(self._frame_views(r, f))
                    index.append(np.arange(N) if pts is None else pts)
            if len(groups) == 1 and groups[0][1] is None:
                xq = xy.repeat(len(views), 1)
            else:
                xq = xy.index_select(0, self._upload(np.concatenate(index).astype(np.int64)))
            ops.trackstore_locate_frames(views, np.concatenate(which), xq, tq, cq, thr)
        else:
            q0 = 0
            for (f, pts), ranks, n in zip(groups, holders, sizes):
                x = xy if pts is None else xy[torch.from_numpy(pts)]
                for r in ranks:
                    self.entries[r][1].locate(x, f, thr, out=(tq[q0:q0 + n], cq[q0:q0 + n]))
                    q0 += n
        return tq, cq

    def _compose_best_points(self, tq, cq, groups, holders, cols, thr, N):
        """The definition of ``best_query_from`` in torch, on the atlas's device: tq [Q, 4] and cq [Q] of ``_locate_candidates``.  Frame
        group after frame group and candidate after candidate: its located template points followed by ``query`` on its template,
        chained behind ITS located row by ``chain_behind_inverse`` with a grid of zeros (the position in the place of the flow),
        keyed as ``_compose_best`` keys, and kept where the key is smaller than the best so far -> (table [N, T, 4], entry [N, T]
        int32)."""
        T, dev = len(cols), self.device
        nan, one, inf, zero = (torch.full((), v, dtype=torch.float32, device=dev) for v in (float("nan"), 1.0, float("inf"), 0.0))
        none = torch.full((), _NOT_FOUND, dtype=torch.int64, device=dev)
        limit = torch.tensor(thr, dtype=torch.float32, device=dev)
        table = torch.empty((N, T, 4), dtype=torch.float32, device=dev)
        entry = torch.empty((N, T), dtype=torch.int32, device=dev)
        q0 = 0
        for (_, pts), ranks in zip(groups, holders):
            n = N if pts is None else len(pts)
            pos, occl, sigma = nan.expand(T, 2, n).clone(), one.expand(T, n).clone(), inf.expand(T, n).clone()
            best = torch.full((T, n), _NOT_FOUND, dtype=torch.int64, device=dev)
            origin = torch.zeros((n, 2), dtype=torch.float32, device=dev)
            for r in ranks:
                tb, found = tq[q0:q0 + n], cq[q0:q0 + n] >= 0
                q0 += n
                s = self.entries[r][0]
                cov = np.asarray(self.covered(s, cols), dtype=bool)
                if not (T and n and cov.any()):
                    continue
                ok = found[:, None] & self._upload(cov)[None, :]
                q = self.query(s, torch.where(found[:, None], tb[:, 0:2], zero), cols)
                p, o, sg = chain_behind_inverse(tb, q, origin, ok)                               # [T, 2, n], [T, n], [T, n]
                field = torch.where(sg > 0, sg, zero).contiguous().view(torch.int32).to(torch.int64)
                field = torch.where(torch.isnan(sg), torch.full((), 0x7fffffff, dtype=torch.int64, device=dev), field)
                key = ((~(o <= limit)).to(torch.int64) << 39) | (field << 8) | int(r)
                key = torch.where(ok.t(), key, none)
                better = key < best
                best = torch.where(better, key, best)
                pos, occl, sigma = torch.where(better[:, None, :], p, pos), torch.where(better, o, occl), torch.where(better, sg, sigma)
            rows = torch.cat([pos, occl[:, None], sigma[:, None]], dim=1).permute(2, 0, 1)      # [n, T, 4]
            won = torch.where(best != none, (best & 0xff).to(torch.int32), torch.full((), -1, dtype=torch.int32, device=dev)).t()
            if pts is None:
                table.copy_(rows)
                entry.copy_(won)
            else:
                at = self._upload(pts.astype(np.int64))
                table.index_copy_(0, at, rows)
                entry.index_copy_(0, at, won)
        return table, entry

    def _points_tables(self, groups, holders, cols, N):
        """The host tables of ``atlas_ops.trackstore_tracks_from_best`` -> (group sizes, candidates per group, rank_of, row_of, order,
        frame_ptrs [R, T], lohi_ptrs [R, T])."""
        row_of, frame_ptrs, lohi_ptrs = self._flow_tables(cols)
        sizes = [N if pts is None else len(pts) for _, pts in groups]
        order = np.concatenate([np.arange(N) if pts is None else pts for _, pts in groups]) if groups else np.zeros(0, np.int64)
        ranks = [r for rs in holders for r in rs]
        return sizes, [len(rs) for rs in holders], ranks, [row_of[r] for r in ranks], order, frame_ptrs, lohi_ptrs

    def best_query_from(self, points, frame, frames=None, occlusion_threshold=0.5, out=None):
        """points (N, 2) xy given ON video frame(s) ``frame`` -- one frame id, or a host sequence of N ids, exactly as for ``locate`` --
        followed over ``frames`` (default: ``atlas.frames``) with the template chosen per point AND column -> (table [N, T, 4]
        float32 = (x, y, occlusion, sigma), entry [N, T] int32, template [N, T] int32) on the atlas's device: the sparse sibling of
        ``best_results_from``.  ``tracks_from`` follows each point on the ONE entry that wins ``locate`` and fills the columns that
        entry's template does not cover.  Here, for point n given on frame f, the candidates are ALL entries that hold f, in
        ascending rank; candidate k takes the point back by its OWN ``store.locate(point, f, thr)`` -- (Px, Py, o_src, s_src) and a
        cell -- follows (Px, Py) by ``query`` on its template -- (qx, qy, o_dst, s_dst) per column -- and chains by
        ``chain_behind_inverse`` with the position in the place of the flow: (qx, qy, max(o_src, o_dst) with a NaN of either kept,
        sqrt(s_src^2 + s_dst^2) correctly rounded).  It has an answer for (n, column t) iff its cell is >= 0 and its template covers
        t, and among those the smallest key of ``best_results_from`` wins, unchanged.  ``entry`` is the winner's rank and
        ``template`` its template frame; where no candidate has an answer the row is NaN, NaN, 1, +inf, -1, -1.  The occlusion is
        the CHAINED maximum, where ``tracks_from`` returns the destination's alone.  ``out``: a (table, entry) pair of contiguous
        tensors of those shapes and dtypes on the atlas's device; ``template`` is allocated by the call.  ``KeyError`` for a frame
        that no entry holds, ``ValueError`` for an ``out`` that does not fit or malformed ``points`` / ``frame``, all before any
        work.  N = 0 or T = 0 returns empty results and launches nothing.  On the device: ONE ``mftx_trackstore_locate`` call (the
        points repeated per candidate, its rows kept un-reduced), one table upload and ONE ``mftx_trackstore_tracks_from_best``
        launch (mft_amd/atlas_ops.py); with ``points`` a device tensor no host synchronisation."""
        xy = _as_points(points, self.device, "TrackAtlas.best_query_from")
        N = int(xy.shape[0])
        groups, holders = self._point_groups(frame, N, "TrackAtlas.best_query_from")          # ValueError, KeyError before any work
        cols = list(self.frames) if frames is None else [int(f) for f in frames]
        T = len(cols)
        if out is not None:
            out = tuple(out)
            want = (((N, T, 4), torch.float32), ((N, T), torch.int32))
            if len(out) != 2 or any(not isinstance(o, torch.Tensor) or tuple(o.shape) != s or o.dtype != d or
                                    not _same_device(o.device, self.device) or not o.is_contiguous() for o, (s, d) in zip(out, want)):
                raise ValueError(f"TrackAtlas.best_query_from: out must be contiguous (float32 [{N}, {T}, 4], int32 [{N}, {T}]) tensors "
                                 f"on {self.device}")
        else:
            out = (torch.empty((N, T, 4), dtype=torch.float32, device=self.device),
                   torch.empty((N, T), dtype=torch.int32, device=self.device))
        table, entry = out
        if N == 0 or T == 0:
            return table, entry, torch.empty((N, T), dtype=torch.int32, device=self.device)
        thr = float(occlusion_threshold)
        tq, cq = self._locate_candidates(xy, groups, holders, thr)
        if self.native:
            from . import atlas_ops
            atlas_ops.trackstore_tracks_from_best(tq, cq, *self._points_tables(groups, holders, cols, N), (self.H, self.W), table, entry, thr)
        else:
            t, e = self._compose_best_points(tq, cq, groups, holders, cols, thr, N)
            table.copy_(t)
            entry.copy_(e)
        tmpl_of = self._upload(np.asarray([f for f, _ in self.entries], dtype=np.int32))
        template = torch.where(entry >= 0, tmpl_of[entry.clamp(min=0).to(torch.int64)], torch.full((), -1, dtype=torch.int32, device=self.device))
        return table, entry, template

    def best_tracks_from(self, points, frame, frames=None, occlusion_threshold=0.5):
        """``tracks_from`` with the template chosen per point AND column: ``best_query_from`` brought to the host -> numpy (coords
        [N, T, 2], occlusion [N, T], found [N, T] bool, template [N, T] int64).  Where no candidate answers a point-column:
        NaN coordinates, occlusion 1, found False, template -1.  With a single holder of the source frame the coordinates are
        ``tracks_from``'s bit for bit; the occlusion is the chained maximum max(o_src, o_dst), where ``tracks_from`` returns the
        destination's o_dst alone.  ONE download; it synchronises."""
        table, _, template = self.best_query_from(points, frame, frames, occlusion_threshold)
        N, T = int(table.shape[0]), int(table.shape[1])
        both = torch.cat([table.reshape(N, T * 4), template.to(torch.float32)], dim=1).cpu().numpy()
        tracks, template = both[:, :T * 4].reshape(N, T, 4), both[:, T * 4:].astype(np.int64)
        return tracks[:, :, 0:2].copy(), tracks[:, :, 2].copy(), template >= 0, template

    def best_result_from(self, src, dst, occlusion_threshold=0.5):
        """-> (``FlowOUTrackingResult`` of the flow from video frame ``src`` to video frame ``dst``, found [H, W] bool, template
        [H, W] int32): one column of ``best_results_from``; found = some candidate answers the pixel for ``dst`` (mask the others:
        their flow is NaN).  ``KeyError`` for a ``src`` or a ``dst`` that no entry holds."""
        from .results import FlowOUTrackingResult
        self._holders(src)
        self._holders(dst)
        flow, occl, sigma, entry, template = self.best_results_from(src, [dst], occlusion_threshold)
        return FlowOUTrackingResult(flow[0], occl[0], sigma[0], validate=False), entry[0] >= 0, template[0]
