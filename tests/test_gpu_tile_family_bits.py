"""The BITS of the tile-resident family (csrc/tile_conv.hip: tile_conv_kernel, tile_conv2p_kernel, gru_half_kernel, ou_head_kernel,
their pack kernels, and pack_flow_branch_kernel for the shared fragment word), pinned across commits: sha256 digests of every
output's raw bytes against tests/golden/tile_family_bits.json.  A change to this family that claims "same bits" passes this file
unchanged; one that changes the rounding re-records the file and says why.

Inputs come from a closed formula in numpy integer arithmetic -- no random generator, so no library version enters:
    x[i] = (((i * 2654435761 + salt * 40503) mod 2^32) >> 8) / 2^24 - 0.5,   times a power of two
(a multiple of 2^-24 of magnitude <= 1/2: exact in fp32).  Weights likewise, then packed on the device by the project's pack calls.

The ops-level cases are the smallest that reach every instantiation class.  THE LAUNCHER, not the caller, picks the cells per tile
there, and the cases rely on its choice on the MI355X's 256 CUs: 32 cells at P = 1, 64 cells at P = 4 and 128 cells at P = 7, all
at 64 x 64 cells (tile_conv_cells, and launch_gru_half's own rule for the GRU pass).  The epilogues TC_GRU_ZR / TC_GRU_Q, the
gather loader of the OU heads and forced cells per tile are reached through the engine only: three engine digests, which ALSO move
when another engine kernel's rounding legitimately changes -- the pull request that changes it re-records them and says why.  The
ops-level digests move with this family alone.

Re-recording (on an MI355X, from a library built from the commit whose bits are to be kept):
    MFTX_LIB=<that build>/mft_amd/libmftx.so python tests/test_gpu_tile_family_bits.py --record --commit <its hash>
Needs gfx950: other devices have other CU counts (other cells per tile: the same bits, but not the instantiations meant) and skip."""
import functools
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = Path(__file__).resolve().parent / "golden" / "tile_family_bits.json"
GROUPS = ["tile_conv2d", "two_pass", "gru_half", "flow_head", "ou_heads", "pack", "engine"]


def series(shape, salt, scale):
    """The formula of the module docstring as a float32 device tensor of the given shape; scale: a power of two."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    v = ((i * np.uint64(2654435761) + np.uint64(salt * 40503)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    x = (v.astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(scale / (1 << 24))
    return torch.from_numpy(x.reshape(shape)).to(DEV)


def digest(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().contiguous().cpu().numpy().tobytes())
    return m.hexdigest()


# ---- the cases, group by group: {case name: digest} ------------------------------------------------------------------------
LAYERS = [(3, 3, 128, 128), (3, 3, 128, 256)] + [(kh, kw, cin, cout) for kh, kw in ((1, 5), (5, 1)) for cin in (128, 256) for cout in (128, 256)]
BIG = {(3, 3, 128, 256), (1, 5, 256, 256), (5, 1, 256, 128)}


def _conv_case(ops, kh, kw, cin, cout, P, h, w, mode, plant=False):
    M = P * h * w
    x = series((M, cin), 1, 1.0)
    if plant:
        x[7, 3], x[20, 64], x[33, 127] = float("inf"), float("-inf"), float("nan")
    wt = series((cout, cin, kh, kw), 2 + kh + cin + cout, 2.0 ** -4)
    b = series((cout,), 3, 0.5)
    xs = ops.split_activations(x)
    x1, x2 = (xs, None) if cin == 128 else (xs[:, :128].contiguous(), xs[:, 128:].contiguous())
    wtile = ops.pack_tile_conv_weights(ops.pack_conv_weight(wt), cout, cin)
    if mode == "linear":
        return digest(ops.tile_conv2d(x1, wtile, b, P, h, w, cout, kh, kw, x2=x2, addend=series((M, cout), 4, 1.0)))
    return digest(ops.tile_conv2d(x1, wtile, b, P, h, w, cout, kh, kw, act="relu", x2=x2, out_split=True))


def group_tile_conv2d(ops):
    out = {}
    for kh, kw, cin, cout in LAYERS:
        sizes = [(1, 9, 5), (2, 21, 37)] + ([(4, 64, 64), (7, 64, 64)] if (kh, kw, cin, cout) in BIG else [])
        for P, h, w in sizes:
            for mode in ("linear", "relu_split"):
                out[f"{kh}x{kw}_{cin}to{cout}/P{P}_{h}x{w}/{mode}"] = _conv_case(ops, kh, kw, cin, cout, P, h, w, mode)
    out["3x3_128to256/P1_9x5/relu_split/inf_nan"] = _conv_case(ops, 3, 3, 128, 256, 1, 9, 5, "relu_split", plant=True)
    return out


def group_two_pass(ops):
    out = {}
    for cout in (192, 126):
        N = 192 if cout == 192 else 128
        wtile = ops.pack_tile_conv_weights(ops.pack_conv_weight(series((cout, 256, 3, 3), 10 + cout, 2.0 ** -5)), N, 256)
        b = series((cout,), 11, 0.5)
        for P, h, w in ((1, 24, 40), (3, 9, 70), (4, 64, 64), (7, 64, 64)):
            M = P * h * w
            xs = ops.split_activations(series((M, 256), 12, 1.0))
            sentinel = ops.split_activations(torch.full((M, N), 7.25, device=DEV))      # (channels 126, 127 of cout = 126 keep it)
            out[f"{cout}/P{P}_{h}x{w}"] = digest(ops.tile_conv2d(xs, wtile, b, P, h, w, cout, 3, 3, act="relu", out_split=True, out=sentinel))
    return out


def group_gru_half(ops):
    out = {}
    for P, h, w, vertical in ((1, 16, 24, False), (1, 16, 24, True), (2, 9, 150, False), (1, 150, 7, True), (7, 64, 64, False), (7, 64, 64, True)):
        M = P * h * w
        kh, kw = (5, 1) if vertical else (1, 5)
        hf = series((M, 128), 20, 2.0)
        mo = series((M, 128), 21, 2.0).abs()
        pack = lambda salt, n: ops.pack_tile_conv_weights(ops.pack_conv_weight(series((n, 256, kh, kw), salt, 2.0 ** -4)), n, 256)      # noqa: E731
        hf_new, h_out, _ = ops.gru_half(ops.split_activations(hf), ops.split_activations(mo), pack(22, 256), pack(23, 128),
                                        series((M, 256), 24, 1.0), series((M, 128), 25, 1.0), hf, P, h, w, vertical=vertical)
        tag = f"{'vertical' if vertical else 'horizontal'}/P{P}_{h}x{w}"
        out[tag + "/h_fp32"], out[tag + "/h_split"] = digest(hf_new), digest(h_out)
    return out


def group_flow_head(ops):
    out = {}
    wtile = ops.pack_tile_conv_weights(ops.pack_conv_weight(series((256, 128, 3, 3), 30, 2.0 ** -4)), 256, 128)
    wproj = ops.pack_flow_head_weights(ops.pack_conv_weight(series((2, 256, 3, 3), 31, 2.0 ** -4)))
    b1, b2 = series((256,), 32, 0.25), series((2,), 33, 0.25)
    for P, h, w in ((1, 3, 5), (2, 21, 37), (7, 64, 64)):
        M = P * h * w
        coords = series((M, 2), 35, 16.0)
        delta = ops.flow_head(ops.split_activations(series((M, 128), 34, 2.0)), h, w, wtile, b1, wproj, b2, coords=coords)
        out[f"P{P}_{h}x{w}/delta"], out[f"P{P}_{h}x{w}/coords"] = digest(delta), digest(coords)
    return out


def group_ou_heads(ops):
    out = {}
    wtile, wproj = ops.pack_ou_heads_weights(ops.pack_conv_weight(series((256, 712, 3, 3), 40, 2.0 ** -5)),
                                             ops.pack_conv_weight(series((3, 256, 3, 3), 41, 2.0 ** -4)))
    b1, b2 = series((256,), 42, 0.25), series((3,), 43, 1.0)
    for P, h, w in ((1, 5, 3), (2, 21, 37), (7, 64, 64)):
        got = ops.ou_heads(ops.split_activations(series((P * h * w, 712), 44, 2.0)), h, w, wtile, b1, wproj, b2)
        out[f"P{P}_{h}x{w}"] = digest(got[:, :3])
    return out


def group_pack(ops):
    out = {}
    for N, taps, cin in ((128, 9, 128), (256, 9, 128), (256, 5, 256), (128, 5, 256), (192, 9, 256), (128, 9, 256)):
        out[f"tile_conv/{N}_{taps}_{cin}"] = digest(ops.pack_tile_conv_weights(series((-(-N // 128) * 128, taps, cin), 50 + N + taps, 2.0 ** -3), N, cin))
    out["flow_head"] = digest(ops.pack_flow_head_weights(series((2, 9, 256), 51, 2.0 ** -3)))
    wtile, wproj = ops.pack_ou_heads_weights(series((256, 9, 712), 52, 2.0 ** -3), series((3, 9, 256), 53, 2.0 ** -3))
    out["ou_heads/wtile"], out["ou_heads/wproj"] = digest(wtile), digest(wproj)
    out["flow_branch"] = digest(ops.pack_flow_branch_weights(series((98, 128), 54, 2.0 ** -3), series((64, 9, 128), 55, 2.0 ** -3)))
    return out


@functools.lru_cache(maxsize=None)
def _engine_weights():
    from mft_amd.weights import make_weights
    return {k: torch.from_numpy(v).to(DEV) for k, v in make_weights(7).items()}


def _engine(ops, options, P, h, w, iters=2):
    eng = ops.RaftEngine(_engine_weights(), DEV, options=options)
    f1 = series((P, h * w, 256), 60, 2.0)
    f2 = f1 + series((P, h * w, 256), 61, 0.5)
    net, inp = series((P, h * w, 128), 62, 2.0), series((P, h * w, 128), 63, 2.0).abs()
    outs = eng.refine(f1, f2, net, inp, h, w, iters)[:3]
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    return digest(*outs)


ENGINE_SAME = {"cells64": {"tile_conv": 2, "tile_cells": 64}, "cells32": {"tile_conv": 2, "tile_cells": 32},
               "unfused_gru": {"tile_conv": 2, "tile_cells": 128, "fuse_gru": 0}}      # ... must give the digest of P3_24x40/cells128


def group_engine(ops):
    out = {"P3_24x40/cells128": _engine(ops, {"tile_conv": 2, "tile_cells": 128}, 3, 24, 40)}
    for tag, options in ENGINE_SAME.items():
        out["P3_24x40/" + tag] = _engine(ops, options, 3, 24, 40)
    out["P3_24x40/materialised_ou"] = _engine(ops, {"tile_conv": 2, "tile_cells": 128, "fuse_ou": 2}, 3, 24, 40)
    out["P1_33x47/defaults"] = _engine(ops, {}, 1, 33, 47)
    return out


def compute(group):
    from mft_amd import ops
    return {f"{group}/{k}": v for k, v in globals()["group_" + group](ops).items()}


# ---- the test ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    if arch != "gfx950":
        pytest.skip(f"the cases rely on the MI355X's launcher choices (gfx950, 256 CUs); this is {arch}")
    return json.loads(GOLDEN.read_text())["digests"]


@pytest.mark.parametrize("group", GROUPS)
def test_tile_family_bits(golden, group):
    got = compute(group)
    want = {k: v for k, v in golden.items() if k.startswith(group + "/")}
    assert sorted(got) == sorted(want), "the recorded cases and the test's differ: re-record (module docstring)"
    bad = [k for k in got if got[k] != want[k]]
    for k in bad:
        print(f"{k}: got {got[k]}, recorded {want[k]}")
    assert not bad, f"{len(bad)} of {len(got)} digests of '{group}' differ from the recorded ones (printed above)"
    if group == "engine":      # cells per tile and the unfused GRU pass: the same bits as 128-cell tiles with the fused pass
        for tag in ENGINE_SAME:
            assert got["engine/P3_24x40/" + tag] == got["engine/P3_24x40/cells128"], tag


if __name__ == "__main__":
    import argparse
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    ap = argparse.ArgumentParser(description="record tests/golden/tile_family_bits.json from the library in use (MFTX_LIB)")
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--commit", default="unknown", help="the commit the library in use was built from")
    ap.add_argument("--out", default=str(GOLDEN))
    args = ap.parse_args()
    digests = {}
    for grp in GROUPS:
        digests.update(compute(grp))
    prop = torch.cuda.get_device_properties(0)
    doc = {"commit": args.commit, "device": f"{prop.name} ({prop.gcnArchName}, {prop.multi_processor_count} CUs)", "rocm": torch.version.hip,
           "digests": digests}
    if args.record:
        Path(args.out).write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
        print(f"recorded {len(digests)} digests to {args.out}")
    else:
        print(json.dumps(doc, indent=1, sort_keys=True))
