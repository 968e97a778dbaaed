"""Many templates of ONE video tracked in a single pass -- what the TAP-Vid protocol needs (``mft_amd/tapvid.py``:
every query frame is a template, each tracked to the end of the video) and what the reference does as a loop of
complete tracker runs (``MFT/runners/run_MFT_tapvid.py:164-195``).

All templates of one time direction advance through the video in LOCKSTEP.  At frame ``t`` every running template has the
plan a single ``MFT`` on its start frame would have (``MFT._plan``: the delta-skip rule, ``inf`` -> start frame,
de-duplication, ``inf`` first then ascending delta).  The finite-delta pairs ``(t - delta, t)`` are the same for all
templates; only the ``inf`` pair ``(start, t)`` is a template's own.  So per frame:

  * the UNION of the plans' (left, t) pairs goes through the flow plugin once, in batches of at most 16 pairs (one
    engine pass each; the frame is encoded once);
  * ONE ``mftx_chain_select_multi`` launch chains and selects for all templates (a right operand shared by many templates
    is read from HBM once and from the caches afterwards);
  * ONE ``mftx_sample_points`` launch reads all query points out into a device-side track table, downloaded once by
    ``point_tracks()``;
  * nothing in ``track()`` waits for the GPU.

The results are the single tracker's, bit for bit: a pair's bits do not depend on the batch it rides in (the kernels are
batch-invariant and are pinned for the same nominal batch, ``set_nominal_pairs``), and the chain + selection arithmetic of
the multi-template kernel is, operation for operation, that of the single-template one (``csrc/chain.hip``).
"""
from __future__ import annotations

import logging
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .MFT import MFT, HipBackend, is_packed, pack_planes
from .point_tracking import convert_to_point_tracking
from .results import FlowOUTrackingResult

logger = logging.getLogger(__name__)

DEFAULT_MAX_TEMPLATES = 32


class HipMultiBackend(HipBackend):
    """``HipBackend`` plus the two multi-template entry points of libmftx."""

    @staticmethod
    def chain_select_multi(templates, thr):
        return ops.chain_select_multi(templates, thr, want_chosen=True)

    @staticmethod
    def sample_points(results, tmpl, xy, table, column):
        return ops.sample_points(results, tmpl, xy, table, column)


class _Template(MFT):
    """One template's bookkeeping: ``MFT``'s plan, memory ring and keep rule (``_plan``, ``cleanup_memory``,
    ``is_before_start``) on a start frame of its own.  It owns no flow plugin -- the pass does -- and ``C`` is the pass's,
    read at every use (runners swap it)."""

    def __init__(self, owner, start_frame_i, time_direction):
        self._owner = owner
        self.flower = None                       # (cleanup_memory: nothing to retain here, the pass retains the union)
        self.start_frame_i = self.current_frame_i = int(start_frame_i)
        self.time_direction = time_direction
        self.memory = {}
        self.last_pairs = []
        self.last_chosen = None
        self._window_ids = set()
        self.queries = None                      # (n, 2) xy float32 on the pass's device, or None
        self.rows = slice(0, 0)                  # this template's rows of the pass's track table

    C = property(lambda self: self._owner.C)

    @property
    def started(self):
        return bool(self.memory)


class MultiTemplateMFT(MFT):
    """``MFT`` for many templates (start frames) of one video and one time direction::

        mt = MultiTemplateMFT(config)
        mt.init(start_frames, time_direction=+1, queries={start: xy (n, 2)}, n_frames=len(video))
        for frame_i in range(min(start_frames), len(video)):
            metas = mt.track(frame_i, video[frame_i])      # {start_frame: meta}, meta.result on the device
        tracks = mt.point_tracks()                          # {start_frame: (coords (n, n_frames, 2), occlusion (n, n_frames))}

    Frames are passed in order of ``time_direction``, beginning at the earliest start frame; the call that passes a
    template's start frame initialises it (identity result, like ``MFT.init``).  Every template's results, ``last_pairs``,
    ``last_chosen`` and memory ring (``templates[start].memory``) are those of an ``MFT`` initialised on that start frame
    alone -- bit for bit with the HIP backend.

    What a template costs: its memory ring, up to ``max finite delta + 1`` results of ``16 * H * W`` bytes -- 138 MB at
    512 x 512 with the shipped deltas (33 results of 4.2 MB); the frames' images and features are shared between the
    templates.  ``max_templates`` (argument, else ``C.multi_template_max``, else 32) bounds a pass: ``init`` raises
    ``ValueError`` beyond it, and the caller runs more start frames in several passes (``tapvid.run_sequence_multi`` does).

    ``C.multi_template_stores`` keeps a ``DenseTrackStore`` per template (``track_stores[start]``, 8 bytes per pixel and frame):
    the store an ``MFT`` with ``C.track_store`` on that start frame alone would hold, word for word, filled by one
    ``trackstore_append_multi`` call per frame.  ``C.track_store_frames_per_chunk`` applies per store,
    ``C.track_store_max_bytes`` to their sum.  ``TrackAtlas.from_passes`` (mft_amd/trackatlas.py) joins the stores of a
    forward and a backward pass.  ``C.track_store`` itself stays refused (it names the single tracker's one store).

    Not supported, and refused rather than ignored: ``C.delta_sharding`` (a multi-GPU pass) and a flow cache -- within one
    pass no pair is requested twice, so a cache would have nothing to return.

    With a ``backend`` that has no ``chain_select_multi`` (the oracle backend of the host tests) the pass calls
    ``backend.chain_select`` per template and reads points out through ``convert_to_point_tracking``.

    ``meta.result`` stays on the device and SHARES its planes with the template's memory ring: move it (``.cpu()``) or read
    it, do not write into it.  ``pair_chunk`` lowers the number of pairs per engine call (at most 16)."""

    def __init__(self, config, backend=None, device='cuda', max_templates=None, pair_chunk=None):
        super().__init__(config, backend=backend if backend is not None else HipMultiBackend(), device=device)
        self._max_templates_arg = max_templates
        self.pair_chunk = min(int(pair_chunk), ops.RaftEngine.MAX_GATHER) if pair_chunk else ops.RaftEngine.MAX_GATHER
        if self.pair_chunk < 1:
            raise ValueError("pair_chunk must be at least 1")
        self.templates = {}

    @property
    def max_templates(self):
        for v in (self._max_templates_arg, self.C.multi_template_max):
            if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v > 0:
                return int(v)
        return DEFAULT_MAX_TEMPLATES

    # ------------------------------------------------------------------ init
    def init(self, start_frames, time_direction=1, queries=None, n_frames=None, flow_cache=None, **kwargs):
        """start_frames: the templates' frame ids; queries (optional): {start_frame: (n, 2) xy on that frame} -- with it
        ``n_frames`` (the length of the video: the track table has one column per frame id) is required.  Nothing is
        computed here: a template is initialised by the ``track`` call that passes its start frame."""
        assert time_direction in [+1, -1]
        if flow_cache is not None:
            raise ValueError("MultiTemplateMFT takes no flow cache: within one pass no pair is requested twice")
        if self.C.track_store:
            raise ValueError("MultiTemplateMFT takes no C.track_store: its queries are read out during the pass (point_tracks)")
        if self.C.delta_sharding:
            raise ValueError("MultiTemplateMFT does not support C.delta_sharding (multi-GPU): run one pass per GPU instead")
        starts = sorted({int(s) for s in start_frames}, reverse=time_direction < 0)
        if not starts:
            raise ValueError("MultiTemplateMFT.init: no start frames")
        if len(starts) > self.max_templates:
            raise ValueError(f"MultiTemplateMFT.init: {len(starts)} start frames exceed max_templates = {self.max_templates}; "
                             "run them in several passes")
        self.time_direction = time_direction
        self.start_frame_i = starts[0]            # the pass begins at the earliest start frame (in time direction)
        self.current_frame_i = None
        self.flow_cache = None
        self._reset_guard_state()
        if hasattr(self.flower, "reset_cache"):
            self.flower.reset_cache()
        if hasattr(self.flower, "set_nominal_pairs"):     # the SINGLE tracker's value: the same kernels, the same bits
            self.flower.set_nominal_pairs(len(set(self.C.deltas)) if self.C.deltas else 1)
        self.templates = {s: _Template(self, s, time_direction) for s in starts}      # in the order they start
        self._order = starts
        self._imgs = {}
        self._window_ids = set()
        self.stats = dict(frames=0, pairs=0, engine_calls=0, chain_launches=0, readout_launches=0, store_append_calls=0)
        self._native = hasattr(self.backend, "chain_select_multi")
        self.track_stores = {}                    # C.multi_template_stores: {start_frame: DenseTrackStore}, made as the templates start
        self._table = self._q_tmpl = self._q_xy = None
        self._host_tracks = {}
        self.n_frames = None
        queries = {int(k): v for k, v in (queries or {}).items() if v is not None and len(v)}
        if queries:
            if set(queries) - set(starts):
                raise ValueError("MultiTemplateMFT.init: queries for frames that are no start frames")
            if n_frames is None:
                raise ValueError("MultiTemplateMFT.init: queries need n_frames (the columns of the track table)")
            self.n_frames = int(n_frames)
            row, idx, xy = 0, [], []
            for j, s in enumerate(starts):
                if s not in queries:
                    continue
                q = torch.as_tensor(np.asarray(queries[s]) if not isinstance(queries[s], torch.Tensor) else queries[s])
                q = q.to(torch.float32).reshape(-1, 2)
                t = self.templates[s]
                t.queries = q.to(self.device) if self._native else q
                t.rows = slice(row, row + len(q))
                row += len(q)
                idx.append(torch.full((len(q),), j, dtype=torch.int32))
                xy.append(q)
                if not self._native:
                    self._host_tracks[s] = (np.zeros((len(q), self.n_frames, 2), np.float32),
                                            np.zeros((len(q), self.n_frames), np.float32))
            if self._native:
                self._q_tmpl = torch.cat(idx).to(self.device)
                self._q_xy = torch.cat(xy).contiguous().to(self.device)
                self._table = torch.zeros((row, self.n_frames, 4), dtype=torch.float32, device=self.device)
        return self

    # ----------------------------------------------------------------- track
    def track(self, frame_i, input_img, debug=False, **kwargs):
        """Advance every running template to ``frame_i`` and initialise the templates that start there.
        -> {start_frame: meta} for every template running after the call."""
        frame_i = int(frame_i)
        expect = self.start_frame_i if self.current_frame_i is None else self.current_frame_i + self.time_direction
        if frame_i != expect:
            raise ValueError(f"MultiTemplateMFT.track: frame {frame_i} out of order (expected {expect}); frames go in order of "
                             "time_direction, beginning at the earliest start frame")
        H, W = input_img.shape[:2]
        if self.current_frame_i is None:
            self.img_H, self.img_W = H, W
        elif (H, W) != (self.img_H, self.img_W):
            raise ValueError("MultiTemplateMFT.track: all frames of a pass have one size")
        if self.n_frames is not None and not 0 <= frame_i < self.n_frames:
            raise ValueError(f"MultiTemplateMFT.track: frame {frame_i} outside the track table (n_frames = {self.n_frames})")
        starting = self.templates.get(frame_i)
        if starting is not None:
            # a private copy, as in MFT.init: the caller may recycle its buffer, and a start frame stays for the whole pass
            input_img = input_img.copy() if hasattr(input_img, "copy") else input_img.clone()
        running = [t for t in self.templates.values() if t.started]
        plans = [t._plan(frame_i) for t in running]

        # the union of the plans' pairs, each once, through the flow plugin
        lefts_needed = list(dict.fromkeys(left_id for plan in plans for _, left_id, _ in plan))
        rights = {}
        for c0 in range(0, len(lefts_needed), self.pair_chunk):
            chunk = lefts_needed[c0: c0 + self.pair_chunk]
            res = self._flows_for_pairs([(l, self._imgs[l], frame_i, input_img) for l in chunk], packed_out=True, planar=False)
            for l, r in zip(chunk, res):
                r = r[3] if len(r) > 3 else tuple(r[:3])
                rights[l] = pack_planes(r) if self._native and not is_packed(r) else r
            self.stats["engine_calls"] += 1
        self.stats["pairs"] += len(lefts_needed)

        # chain + selection for all running templates
        thr = self.C.occlusion_threshold
        per_template = [([t.memory[left_id]['result'].planes() for _, left_id, _ in plan], [rights[left_id] for _, left_id, _ in plan])
                        for t, plan in zip(running, plans)]
        if not running:
            selected = []
        elif self._native:
            selected = self.backend.chain_select_multi(per_template, thr)
            self.stats["chain_launches"] += 1
        else:
            selected = [self.backend.chain_select(Ls, Rs, thr) for Ls, Rs in per_template]
            self.stats["chain_launches"] += len(running)
        # the guard runs before any bookkeeping changes (MFT._finish_frame); never a host wait here
        self._check_nonfinite(synced=False)
        identity = FlowOUTrackingResult.identity((H, W), device=self.device) if starting is not None else None
        if self.C.multi_template_stores:           # ... and so do the stores: a MemoryError leaves the pass as it was
            self._append_stores(frame_i, [(t.start_frame_i, sel[:3]) for t, sel in zip(running, selected)] +
                                ([(frame_i, identity.planes())] if starting is not None else []), H, W)

        metas = {}
        for t, plan, (flow, occl, sigma, chosen) in zip(running, plans, selected):
            result = FlowOUTrackingResult(flow, occl, sigma, validate=False)
            t.current_frame_i = frame_i
            t.last_pairs = [(left_id, frame_i) for _, left_id, _ in plan]
            t.last_chosen = chosen
            t.memory[frame_i] = {'img': input_img, 'result': result}
            t.cleanup_memory()
            metas[t.start_frame_i] = self._meta(result)
        if starting is not None:
            result = identity
            starting.memory = {frame_i: {'img': input_img, 'result': result}}
            metas[frame_i] = self._meta(result)
        self.current_frame_i = frame_i
        self._imgs[frame_i] = input_img
        keep = set().union(*[set(t.memory) for t in self.templates.values()])
        for k in [k for k in self._imgs if k not in keep]:
            del self._imgs[k]
        if hasattr(self.flower, "retain"):
            self.flower.retain(keep)
        self._read_out(frame_i)
        self.stats["frames"] += 1
        return metas

    def _append_stores(self, frame_i, results, H, W):
        """C.multi_template_stores: results = [(start_frame, (flow, occl, sigma))] of every template at ``frame_i``, the starting
        one's identity included -> each template's ``DenseTrackStore`` (``track_stores[start]``, made here for the starting one)
        gets its frame: what ``MFT`` with ``C.track_store`` keeps for that start frame alone, word for word.  With the HIP
        backend ONE ``trackstore_append_multi`` call quantises all of them; otherwise each store appends through its own path.
        ``C.track_store_max_bytes`` bounds the SUM over the stores: ``MemoryError`` before anything of this frame is stored."""
        from .trackstore import DenseTrackStore
        kw = {}
        if self.C.track_store_frames_per_chunk:
            kw["frames_per_chunk"] = int(self.C.track_store_frames_per_chunk)
        stores = {s: self.track_stores[s] if s in self.track_stores else DenseTrackStore(H, W, device=self.device, **kw)
                  for s, _ in results}
        cap = self.C.track_store_max_bytes
        if isinstance(cap, (int, float)) and not isinstance(cap, bool):
            held = sum(st.nbytes for st in self.track_stores.values())
            more = sum(st.chunk_bytes for st in stores.values() if st.next_needs_chunk)
            if held + more > int(cap):
                raise MemoryError(f"MultiTemplateMFT: frame {frame_i} needs {more} more bytes of track stores, which would exceed "
                                  f"track_store_max_bytes = {int(cap)} ({held} bytes held by {len(self.track_stores)} stores)")
        # nothing of the frame stays behind if a store cannot take it or the call fails: the reservations are given back and a
        # store made for a template that starts here is not kept
        done = []
        try:
            if self._native:
                slots = []
                for s, _ in results:
                    slots.append(stores[s].reserve(frame_i))
                    done.append(s)
                ops.trackstore_append_multi([(planes, packed, lohi) for (_, planes), (_, packed, lohi) in zip(results, slots)])
            else:
                for s, planes in results:
                    stores[s].append(planes, frame_i)
                    done.append(s)
        except BaseException:
            for s in done:
                stores[s].unreserve(frame_i)
            raise
        self.track_stores.update(stores)
        self.stats["store_append_calls"] += 1 if self._native else len(results)

    @staticmethod
    def _meta(result):
        meta = SimpleNamespace()
        # an object of its own over the SAME planes: the consumer may move it in place (meta.result.cpu()) without touching the ring
        meta.result = FlowOUTrackingResult(result.flow, result.occlusion, result.sigma, validate=False)
        return meta

    def _read_out(self, frame_i):
        """All query points of all started templates at ``frame_i`` -> column ``frame_i`` of the track table.  The templates are
        ordered by their start, so the started ones are a prefix and the kernel leaves the other templates' points alone."""
        if self.n_frames is None:
            return
        started = [self.templates[s] for s in self._order if self.templates[s].started]
        if self._native:
            if any(t.queries is not None for t in started):
                self.backend.sample_points([t.memory[frame_i]['result'].planes() for t in started], self._q_tmpl, self._q_xy,
                                           self._table, frame_i)
                self.stats["readout_launches"] += 1
            return
        for t in started:
            if t.queries is not None:
                coords, occl = convert_to_point_tracking(t.memory[frame_i]['result'], t.queries)
                self._host_tracks[t.start_frame_i][0][:, frame_i] = coords
                self._host_tracks[t.start_frame_i][1][:, frame_i] = occl

    def point_tracks(self):
        """{start_frame: (coords (n, n_frames, 2), occlusion (n, n_frames))} as numpy arrays, for every template with queries:
        column ``f`` is the template's read-out at frame ``f`` (zeros where the pass has not taken it).  ONE download; it
        synchronises, and reads the flow plugin's non-finite counter while it is at it (``FloatingPointError``)."""
        if self._native and self._table is not None:
            table = self._table.cpu().numpy()
            out = {t.start_frame_i: (table[t.rows, :, 0:2].copy(), table[t.rows, :, 2].copy())
                   for t in self.templates.values() if t.queries is not None}
        else:
            out = {s: (c.copy(), o.copy()) for s, (c, o) in self._host_tracks.items()}
        off = (isinstance(self.C.raise_on_nonfinite, bool) and not self.C.raise_on_nonfinite) or \
            (isinstance(self.C.nonfinite_check_every, (int, float)) and not isinstance(self.C.nonfinite_check_every, bool)
             and self.C.nonfinite_check_every <= 0)
        if not off:
            self.check_nonfinite()
        return out

    # ------------------------------------------------- not part of this class
    def track_window(self, *a, **kw):
        raise NotImplementedError("MultiTemplateMFT has no look-ahead windows (no multi-GPU sharding of a multi-template pass)")

    def flush_window(self):
        return []

    def cleanup_memory(self):
        raise NotImplementedError("the memory rings belong to the templates (MultiTemplateMFT.templates[start].memory)")
