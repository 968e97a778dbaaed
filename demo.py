#!/usr/bin/env python3
"""Track every pixel of a video with MFT and write the point / edit overlays -- the reference's ``demo.py`` on
the MI355X engine.

    python demo.py --video <dir of PNG frames | frames.npy> [--edit edit.png] [--out demo_out/] [--synthetic] [--gpu-overlays | --track-store [--query-frame Q] [--edit-frame Q]]

Differences forced by the environment: no OpenCV here, so the input is a directory of PNG frames or a ``.npy``
frame array (video containers work when cv2 is importable) and the overlays are written as numbered PNGs instead of
an mp4; ``--synthetic`` tracks the seeded synthetic video with seeded stand-in weights (no checkpoint ships with
this build).  Frames go to the GPU through a pinned upload ring (``mft_amd/video.py:FrameRing``).  With ``--gpu-overlays``
both overlays are rendered on the GPU inside the tracking loop (``mft_amd/vis.py:DeviceOverlay``) and written as they
arrive: no dense result is downloaded or kept.  With ``--track-store`` the tracker keeps every frame's dense result on the GPU in
16 bits (``mft_amd/trackstore.py``: 8 bytes per pixel) and nothing is downloaded inside the loop; afterwards ONE read-out gives the
points of all frames, and the edit overlay is drawn from the stored frames.  ``--query-frame Q`` takes the query grid on frame Q
instead of frame 0: the stored map of frame Q is inverted at the grid (``DenseTrackStore.tracks_from``), and grid points that no
template point maps to are drawn as occluded.  ``--edit-frame Q`` takes the RGBA edit as painted on frame Q instead of frame 0:
every frame's overlay is then splatted along the dense flow from frame Q to it (``DenseTrackStore.result_from``: frame Q's stored
map inverted at every pixel, then followed forward), and pixels of frame Q that no template point maps to carry no edit.
"""
import argparse
import logging
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

from mft_amd.config import load_config  # noqa: E402
from mft_amd.point_tracking import convert_to_point_tracking  # noqa: E402
from mft_amd import video as vio  # noqa: E402
from mft_amd import vis  # noqa: E402

logger = logging.getLogger("demo")


def parse_arguments():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-v', '--verbose', action='store_true')
    ap.add_argument('--video', type=Path, default=Path('demo_in/frames'), help='directory of PNG frames or .npy / .npz frame array')
    ap.add_argument('--edit', type=Path, default=Path('demo_in/edit.png'), help='RGBA png with a first-frame edit')
    ap.add_argument('--config', type=Path, default=REPO / 'configs' / 'MFT_cfg.py')
    ap.add_argument('--out', type=Path, default=Path('demo_out/'))
    ap.add_argument('--grid_spacing', type=int, default=30)
    ap.add_argument('--synthetic', type=int, default=0, metavar='N', help='track N frames of the seeded synthetic video')
    ap.add_argument('--synthetic_weights_seed', type=int, default=None, help='run on seeded stand-in weights')
    ap.add_argument('--gpu-overlays', action='store_true', help='render the overlays on the GPU while tracking; dense results stay on the device')
    ap.add_argument('--track-store', action='store_true', help='keep every dense result on the GPU in 16 bits; read the points out after the pass')
    ap.add_argument('--query-frame', type=int, default=None, metavar='Q', help='with --track-store: take the query grid on frame Q instead of frame 0')
    ap.add_argument('--edit-frame', type=int, default=None, metavar='Q', help='with --track-store: the edit is painted on frame Q instead of frame 0')
    return ap.parse_args()


def run(args):
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO,
                        format="[%(asctime)s] %(levelname)s:%(name)s:%(message)s")
    config = load_config(args.config)
    if args.synthetic or args.synthetic_weights_seed is not None:
        config.flow_config.model = None
        config.flow_config.synthetic_weights_seed = args.synthetic_weights_seed or 0
    config.keep_result_on_device = True
    if args.track_store:
        if args.gpu_overlays:
            raise SystemExit("--track-store and --gpu-overlays are two ways to avoid the per-frame download: choose one")
        config.track_store = True
    elif args.query_frame is not None or args.edit_frame is not None:
        raise SystemExit("--query-frame and --edit-frame read the track store: give --track-store too")
    tracker = config.tracker_class(config)
    if args.synthetic:
        from mft_amd.synth import SyntheticVideo
        src = SyntheticVideo(512, 512, n_frames=args.synthetic, seed=0)
        frames = [src[i] for i in range(args.synthetic)]
        name = "synthetic"
    else:
        frames = list(vio.get_video_frames(args.video))
        name = args.video.stem
    logger.info("tracking %d frames", len(frames))
    if args.gpu_overlays:
        return run_gpu_overlays(args, tracker, frames, name)
    if args.track_store:
        return run_track_store(args, tracker, frames, name)
    from mft_amd.results import FlowOUTrackingResult
    results, host_results, queries = [], [], None
    drain = vio.ResultDrain()
    import torch
    up = [torch.cuda.current_stream()]                   # the streams frames are uploaded on (FrameRing's reuse guard)
    if getattr(tracker.flower, "_enc_stream", None) is not None:
        up.append(tracker.flower._enc_stream)
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=up)):
        if i == 0:
            meta = tracker.init(dev_frame)
            meta.result = meta.result.cuda()
            queries = vis.get_queries(frames[0].shape[:2], args.grid_spacing).cuda()
        else:
            meta = tracker.track(dev_frame)
        coords, occlusions = convert_to_point_tracking(meta.result, queries)
        drain.submit(meta.result)
        host_results.append(FlowOUTrackingResult(*drain.collect(copy=True), validate=False))
        results.append((coords, occlusions))
    edit = vio.imread_unchanged(args.edit) if args.edit.exists() else None
    for i, frame in enumerate(frames):
        coords, occlusions = results[i]
        result = host_results[i]
        vio.imwrite_bgr(args.out / f"{name}_points" / f"{i:05d}.png", vis.draw_dots(frame, coords, occlusions))
        if edit is not None:
            vio.imwrite_bgr(args.out / f"{name}_edit" / f"{i:05d}.png", vis.draw_edit(frame, result, edit))
    logger.info("wrote %s", args.out)
    return 0


def run_track_store(args, tracker, frames, name):
    """The tracker keeps the dense results (``config.track_store``): the loop only tracks.  Afterwards one ``tracks()`` call reads
    the query grid out of all stored frames, and ``store.result(i)`` dequantises a frame on the device for the edit overlay
    (``store.result_from(Q, i)`` where the edit is painted on frame Q)."""
    up = [torch.cuda.current_stream()]
    if getattr(tracker.flower, "_enc_stream", None) is not None:
        up.append(tracker.flower._enc_stream)
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=up)):
        if i == 0:
            tracker.init(dev_frame)
        else:
            tracker.track(dev_frame)
    store = tracker.track_store
    logger.info("track store: %d frames, %.1f MB on the device", len(store), store.nbytes / 1e6)
    queries = vis.get_queries(frames[0].shape[:2], args.grid_spacing)
    if args.query_frame is None:
        coords, occlusions = store.tracks(queries, frames=range(len(frames)))
    else:
        coords, occlusions, found = store.tracks_from(queries, args.query_frame, frames=range(len(frames)))
        logger.info("query grid on frame %d: %d of %d points are images of template points", args.query_frame, int(found.sum()), len(found))
    edit = vio.imread_unchanged(args.edit) if args.edit.exists() else None
    for i, frame in enumerate(frames):
        vio.imwrite_bgr(args.out / f"{name}_points" / f"{i:05d}.png", vis.draw_dots(frame, coords[:, i], occlusions[:, i]))
        if edit is not None:
            if args.edit_frame is None:
                result = store.result(i)
            else:                     # frame Q -> frame i; a pixel of frame Q that nothing maps to counts as occluded: no edit there
                result, found = store.result_from(args.edit_frame, i)
                if i == 0:
                    logger.info("edit on frame %d: %d of %d pixels are images of template points", args.edit_frame, int(found.sum()), found.numel())
            vio.imwrite_bgr(args.out / f"{name}_edit" / f"{i:05d}.png", vis.draw_edit(frame, result, edit))
    logger.info("wrote %s", args.out)
    return 0


def run_gpu_overlays(args, tracker, frames, name):
    """The same loop with the overlays rendered on the device: per frame the tracker's result feeds ``DeviceOverlay.render``
    on the tracking stream, and the finished uint8 frames are written as their downloads land."""
    edit = vio.imread_unchanged(args.edit) if args.edit.exists() else None
    up = [torch.cuda.current_stream()]
    if getattr(tracker.flower, "_enc_stream", None) is not None:
        up.append(tracker.flower._enc_stream)
    written = 0

    def write(done):
        nonlocal written
        for points, edited in done:
            vio.imwrite_bgr(args.out / f"{name}_points" / f"{written:05d}.png", points)
            if edited is not None:
                vio.imwrite_bgr(args.out / f"{name}_edit" / f"{written:05d}.png", edited)
            written += 1

    overlay = None
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=up)):
        if i == 0:
            meta = tracker.init(dev_frame)
            meta.result = meta.result.cuda()
            H, W = frames[0].shape[:2]
            overlay = vis.DeviceOverlay(edit, vis.get_queries((H, W), args.grid_spacing), H, W)
        else:
            meta = tracker.track(dev_frame)
        overlay.render(dev_frame, meta.result)
        write(overlay.download())
    if overlay is not None:
        write(overlay.download(wait=True))
    logger.info("wrote %s", args.out)
    return 0


if __name__ == '__main__':
    sys.exit(run(parse_arguments()))
