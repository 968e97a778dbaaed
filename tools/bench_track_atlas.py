#!/usr/bin/env python3
"""What the track atlas costs (mft_amd/trackatlas.py, MultiTemplateMFT with C.multi_template_stores; csrc/trackstore.hip).

(a) The pass: a 512 x 512, 50-frame forward pass of 10 start frames (every fifth frame; stand-in weights, the shipped
    configuration), run three ways in ONE process, a, b, c, a, b, c, ...: without stores, with stores through
    ``mftx_trackstore_append_multi``, and with stores through one ``mftx_trackstore_append`` per template.  A host clock around work
    that ends in a device synchronise; medians.  Also the append calls alone, 10 frames per call, events around batches.
(b) The dense inverse: ``mftx_trackstore_invert_atlas`` (through ``TrackAtlas.inverse``) against the composition -- per-entry
    ``store.inverse`` plus the key minimum in torch -- a, b, a, b, a, b with events around batches, medians, the peak bytes each
    allocates, and the two results compared bit for bit: 10 entries at 512 x 512 on the pass's own stores (the last frame) and
    32 entries of seeded smooth fields at 1080 x 1920.
(c) Coverage: the share of pixels of the last frame that ``inverse`` finds with the template-0 store alone and with the
    10-template atlas, on the pass's results.

Writes profiles/track_atlas.json.

    python tools/bench_track_atlas.py [--out profiles/track_atlas.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from mft_amd import multi, ops  # noqa: E402
from mft_amd.config import load_config  # noqa: E402
from mft_amd.multi import MultiTemplateMFT  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402
from mft_amd.trackatlas import TrackAtlas  # noqa: E402
from mft_amd.trackstore import DenseTrackStore  # noqa: E402
from bench_track_inverse import batch_for, device_ms  # noqa: E402
from bench_track_locate import smooth_results  # noqa: E402

DEV = "cuda"
ROUNDS = 3


def config(**extra):
    conf = load_config(REPO / "configs" / "MFT_cfg.py")
    conf.flow_config.model = None
    conf.flow_config.synthetic_weights_seed = 0
    conf.keep_result_on_device = True
    for k, v in extra.items():
        setattr(conf, k, v)
    return conf


def run_pass(mt, video, starts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mt.init(starts, time_direction=+1)
    for f in range(min(starts), len(video)):
        mt.track(f, video[f])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def append_per_template(frames):
    for planes, packed, lohi in frames:
        ops.trackstore_append(planes, packed, lohi)


def pass_legs(video, starts):
    plain, stored = MultiTemplateMFT(config()), MultiTemplateMFT(config(multi_template_stores=True))
    batched = ops.trackstore_append_multi
    legs = {"without_stores": (plain, batched), "stores_append_multi": (stored, batched), "stores_append_per_template": (stored, append_per_template)}
    times = {k: [] for k in legs}
    for rnd in range(ROUNDS + 1):                            # one untimed round of each first
        for k, (mt, fn) in legs.items():
            multi.ops.trackstore_append_multi = fn
            try:
                dt = run_pass(mt, video, starts)
            finally:
                multi.ops.trackstore_append_multi = batched
            if rnd:
                times[k].append(dt)
            if k == "stores_append_per_template":
                per_template_stores = dict(mt.track_stores)
            elif k == "stores_append_multi":
                multi_stores = dict(mt.track_stores)
    same = all(torch.equal(multi_stores[s].packed(k).view(torch.int16), per_template_stores[s].packed(k).view(torch.int16)) and
               torch.equal(multi_stores[s].lohi(k).view(torch.int32), per_template_stores[s].lohi(k).view(torch.int32))
               for s in starts for k in range(len(multi_stores[s])))
    n = len(video) - min(starts)
    res = {"frames": n, "templates": len(starts), "rounds": ROUNDS, "stores_same_bits_both_ways": bool(same),
           "store_bytes": int(sum(st.nbytes for st in multi_stores.values())),
           "append_calls_per_pass": int(stored.stats["store_append_calls"])}
    for k, t in times.items():
        res[k] = {"pass_s": float(np.median(t)), "pass_s_min_max": [float(min(t)), float(max(t))], "frames_per_s": float(n / np.median(t))}
    # the append calls alone: the ten templates' results of the last frame into scratch slots
    results = [stored.templates[s].memory[len(video) - 1]["result"].planes() for s in starts]
    H, W = results[0][0].shape[1:]
    packed = torch.empty((len(starts), H, W, 4), dtype=torch.uint16, device=DEV)
    lohi = torch.zeros((len(starts), 4, 2), device=DEV)
    frames = [(p, packed[j], lohi[j]) for j, p in enumerate(results)]
    fa, fb = (lambda: ops.trackstore_append_multi(frames)), (lambda: append_per_template(frames))
    na, nb = batch_for(fa), batch_for(fb)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(device_ms(lambda: [fa() for _ in range(na)]) * 1e3 / na)
        tb.append(device_ms(lambda: [fb() for _ in range(nb)]) * 1e3 / nb)
    res["append_10_frames_us"] = {"append_multi": float(np.median(ta)), "append_per_template": float(np.median(tb)),
                                  "append_multi_min_max": [float(min(ta)), float(max(ta))],
                                  "append_per_template_min_max": [float(min(tb)), float(max(tb))]}
    return res, multi_stores


def composition(atlas, f, thr=0.5):
    """Per-entry ``store.inverse`` plus the key minimum in torch: what ``mftx_trackstore_invert_atlas`` fuses."""
    ranks = atlas._holders(f)
    per = [atlas.entries[r][1].inverse(f, thr) for r in ranks]
    H, W = atlas.H, atlas.W
    t, c, e = atlas._reduce(torch.stack([p[0] for p in per]).view(len(ranks), H * W, 4),
                            torch.stack([p[1] for p in per]).view(len(ranks), H * W), ranks, thr)
    return t.view(H, W, 4), c.view(H, W), e.view(H, W)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def inverse_legs(atlas, f):
    fa, fb = (lambda: atlas.inverse(f)), (lambda: composition(atlas, f))
    a, b = fa(), fb()
    same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))
    found = float((a[1] >= 0).float().mean())
    del a, b
    res = {"entries": len(atlas._holders(f)), "H": atlas.H, "W": atlas.W, "same_bits": bool(same), "found_share": found,
           "invert_atlas_peak_bytes": peak_bytes(fa), "composition_peak_bytes": peak_bytes(fb)}
    na, nb = batch_for(fa), batch_for(fb)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(device_ms(lambda: [fa() for _ in range(na)]) * 1e3 / na)
        tb.append(device_ms(lambda: [fb() for _ in range(nb)]) * 1e3 / nb)
    res.update(invert_atlas_us=float(np.median(ta)), invert_atlas_us_min_max=[float(min(ta)), float(max(ta))],
               composition_us=float(np.median(tb)), composition_us_min_max=[float(min(tb)), float(max(tb))],
               composition_over_invert_atlas=float(np.median(tb) / np.median(ta)))
    return res


def smooth_atlas(H, W, n):
    fields = smooth_results(H, W, n)
    identity = (torch.zeros(2, H, W, device=DEV), torch.zeros(1, H, W, device=DEV), torch.zeros(1, H, W, device=DEV))
    entries = []
    for k in range(n):
        st = DenseTrackStore(H, W, device=DEV, frames_per_chunk=2)
        st.append(identity, 0)
        st.append(fields[k], 1)
        entries.append((0, st))
    return TrackAtlas(entries)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_atlas.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_atlas.py measures on the GPU"
    torch.cuda.set_device(0)
    vid = SyntheticVideo(512, 512, n_frames=args.frames, seed=100)
    video = [np.ascontiguousarray(vid[i]) for i in range(args.frames)]
    starts = list(range(0, args.frames, args.stride))
    report = {"what": "MultiTemplateMFT with a store per template; TrackAtlas.inverse (mftx_trackstore_invert_atlas) against per-entry "
                      "inverse plus the key minimum in torch; a, b, a, b, ... in one process, medians of %d" % ROUNDS,
              "device": torch.cuda.get_device_name(0)}
    report["pass_512x512"], stores = pass_legs(video, starts)
    atlas = TrackAtlas([(s, stores[s]) for s in starts])
    last = args.frames - 1
    report["inverse_512x512_pass_stores"] = inverse_legs(atlas, last)
    alone = stores[0].inverse(last)[1] >= 0
    joint = atlas.inverse(last)
    report["coverage_last_frame"] = {"frame": last, "template_0_alone": float(alone.float().mean()),
                                     "atlas_of_%d_templates" % len(starts): float((joint[1] >= 0).float().mean()),
                                     "pixels_won_per_template": {str(s): int((joint[2] == r).sum()) for r, s in enumerate(starts)}}
    del atlas, stores, alone, joint
    torch.cuda.empty_cache()
    report["inverse_1080x1920_smooth_fields"] = inverse_legs(smooth_atlas(1080, 1920, 32), 1)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
