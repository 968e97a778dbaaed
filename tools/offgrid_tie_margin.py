#!/usr/bin/env python3
"""How close to a tie are the chosen deltas of tests/test_gpu_offgrid.py's sequences?  CPU only (the oracle, no HIP).

The off-grid tracker test leaves pixels where the HIP tracker and the oracle tracker chose a different delta out of its plane
comparisons, and caps that exclusion at 0.1 % per frame.  The cap only means something if the inputs are not dominated by
near-ties.  This tool runs the oracle tracker twice per size -- once as it is, once with every flow, occlusion and sigma its flow
function returns perturbed by Gaussian noise (absolute for flow and occlusion, relative for sigma) -- and prints, per frame, how
many pixels flip their chosen delta.  It also prints what the test asserts about the sequence itself: the pixels whose chained
position leaves the image in the last frame and the share of fractional chained positions.  With --fp64 the unperturbed tracker
is run in float64 too and the fp32-vs-fp64 differences (the yardstick of the test's tolerances) are printed.

    python tools/offgrid_tie_margin.py                      # all sizes of the test, noise 1e-5 and 1e-4
    python tools/offgrid_tie_margin.py --sizes 125x187 --noise 1e-5 --fp64
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from mft_amd.synth import SyntheticVideo            # noqa: E402
from mft_amd.weights import make_weights            # noqa: E402
from oracle import mft_oracle as O                  # noqa: E402

SIZES = [(125, 187), (127, 129), (130, 131), (129, 133), (121, 122), (128, 136)]       # tests/test_gpu_offgrid.py: SIZES
DELTAS = (np.inf, 1, 2, 4)
ITERS = 12
N_TRACKED = 6
WEIGHT_SEED = 7                                     # tests/golden_inputs.py: WEIGHT_SEED


def run(frames, sd, noise=0.0, seed=0):
    gen = torch.Generator().manual_seed(seed)

    def flow_fn(l, r, li, ri):
        f, o, s = O.compute_flow(sd, li, ri, ITERS)
        if noise:
            f = f + noise * torch.randn(f.shape, generator=gen, dtype=f.dtype)
            o = o + noise * torch.randn(o.shape, generator=gen, dtype=o.dtype)
            s = s * (1 + noise * torch.randn(s.shape, generator=gen, dtype=s.dtype))
        return f, o, s

    tr = O.Tracker(flow_fn, deltas=DELTAS)
    tr.init(frames[0])
    with torch.no_grad():
        return [tr.track(f) for f in frames[1:]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", nargs="*", default=[f"{h}x{w}" for h, w in SIZES], help="HxW ...")
    ap.add_argument("--noise", nargs="*", type=float, default=[1e-5, 1e-4])
    ap.add_argument("--fp64", action="store_true", help="also run the oracle in float64 and print the fp32-vs-fp64 differences")
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    sd = {k: torch.from_numpy(v) for k, v in make_weights(WEIGHT_SEED).items()}
    for size in args.sizes:
        H, W = (int(v) for v in size.lower().split("x"))
        vid = SyntheticVideo(H, W, n_frames=8, seed=0)
        frames = [vid[i] for i in range(N_TRACKED + 1)]
        base = run(frames, sd)
        rf = base[-1].result[0]
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        px, py = xx + rf[0], yy + rf[1]
        outside = int(((px < 0) | (py < 0) | (px >= W) | (py >= H)).sum())
        frac = float(((rf[0] != rf[0].round()) | (rf[1] != rf[1].round())).float().mean())
        print(f"{H}x{W}: H*W%4={H * W % 4}  outside pixels in the last frame {outside}  fractional positions {100 * frac:.1f} %")
        for noise in args.noise:
            pert = run(frames, sd, noise=noise, seed=1)
            flips = [int((a.chosen != b.chosen).sum()) for a, b in zip(base, pert)]
            print(f"    noise {noise:g}: flipped pixels per frame {flips}  worst {100 * max(flips) / (H * W):.3f} %")
        if args.fp64:
            with O.precision(torch.float64):
                wide = run(frames, O.cast_weights(sd, torch.float64))
            for i, (a, b) in enumerate(zip(base, wide), 1):
                same = a.chosen == b.chosen
                e = (a.result[0].double() - b.result[0]).pow(2).sum(0).sqrt()[same]
                do = (a.result[1].double() - b.result[1]).abs()[0][same].max()
                ds = ((a.result[2].double() - b.result[2]).abs() / b.result[2].clamp_min(1e-6))[0][same].max()
                print(f"    fp32 vs fp64 frame {i}: flips {int((~same).sum())}  EPE mean {float(e.mean()):.2e} max {float(e.max()):.2e}"
                      f"  occlusion {float(do):.2e}  sigma rel {float(ds):.2e}")


if __name__ == "__main__":
    main()
