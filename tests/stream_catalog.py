"""One entry per public function of mft_amd/ops.py that hands ``_stream()`` to the library, for tests/test_gpu_streams_ops.py.

An entry gives
  fixed(ops)               what is built once, before anything is stalled: weights, integer tables, query points;
  inputs(ops, seed)        the PAYLOAD the call reads, as a dict of tensors: two seeds give two valid input sets of equal shapes;
  call(ops, fx, inp, v)    the call on the dict's device tensors -> the list of tensors it wrote (v: 0 or 1, see ``tables``).

Safety rule.  Only payload differs between two input sets: float values, and the 8- and 16-bit samples of images and of stored
(quantised) frames, every value of which is valid.  Everything an address is computed from -- integer tables, slot lists, first_of,
entry planes, template ids, pointer tables -- lives in ``fixed`` or is derived from the addresses of the dict's tensors, which are
rewritten in place and never reallocated.  Sampling coordinates that are payload (flows, lookup coordinates, query points) stay
within a few cells of the frame; the kernels clamp or zero-fill whatever leaves it (tests/corr_reference.py: hostile_coords).  A
read of old bytes therefore stays inside its buffer and computes an older valid answer; nothing here can fault.

``tables``: the entry uploads a host table through a pinned temporary; ``call(..., v)`` with v = 0 and v = 1 gives two calls with
different host tables (and outputs of their own) that the test runs back to back behind ONE stall.
``host_wait``: the call waits for the host by contract (it returns a host value), so nothing can be asserted about what was
still enqueued when it returned; the reason is in ``host_wait``.
"""
from collections import namedtuple

import numpy as np
import torch

import golden_inputs as gi

DEV = "cuda"
Entry = namedtuple("Entry", "name covers fixed inputs call tables host_wait", defaults=(False, None))

P, H8, W8 = 2, 17, 23          # two pairs on an odd 1/8 grid (tests/refine_reference.py: the smallest shape that is odd both ways)
N8 = H8 * W8
HF, WF = 37, 53                # a frame with H * W odd (tests/test_gpu_trackstore.py: SIZES[0])


def _g(seed):
    return torch.Generator().manual_seed(1000 + seed)


def _randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=_g(seed)) * scale


def _grid():
    ys, xs = torch.meshgrid(torch.arange(H8, dtype=torch.float32), torch.arange(W8, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], -1).reshape(1, N8, 2)


def _coords(seed, spread=3.0):
    return (_grid() + spread * _randn(seed + 50, P, N8, 2)).contiguous()


def field(seed, H=HF, W=WF):
    """(flow [2,H,W], occlusion [1,H,W], sigma [1,H,W]) float32 CPU tensors: the smooth planes of tests/test_gpu_trackstore.py."""
    r = gi._rng(91, seed, H, W)
    flow = gi.smooth_field(r, 2, H, W, cells=4, amp=3.0) + np.array([0.7 * (seed % 5), -0.4 * (seed % 5)], np.float32)[:, None, None]
    occl = np.clip(gi.smooth_field(r, 1, H, W, cells=5, amp=0.6), 0, 1).astype(np.float32)
    sigma = (0.05 + np.abs(gi.smooth_field(r, 1, H, W, cells=5, amp=0.7))).astype(np.float32)
    return tuple(torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))) for a in (flow, occl, sigma))


def _results(seed, K, prefix):
    """K results as a flat dict {prefix + 'k' + part: tensor}."""
    out = {}
    for k in range(K):
        f, o, s = field(seed * 16 + k)
        out.update({f"{prefix}{k}f": f, f"{prefix}{k}o": o, f"{prefix}{k}s": s})
    return out


def _triples(inp, K, prefix):
    return [(inp[f"{prefix}{k}f"], inp[f"{prefix}{k}o"], inp[f"{prefix}{k}s"]) for k in range(K)]


def _packed_of(f, o, s):
    return torch.cat([f, o, s]).permute(1, 2, 0).contiguous()


ENTRIES = []


def entry(name, covers=None, tables=False, host_wait=None):
    def deco(cls):
        ENTRIES.append(Entry(name, tuple(covers or (name,)), cls.fixed, cls.inputs, cls.call, tables, host_wait))
        return cls
    return deco


def nothing(ops):
    return None


# ---- copy and weight forms -------------------------------------------------------------------------------------------------------
@entry("copy_bytes")
class _CopyBytes:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"src": _randn(seed, 125 * 187 + 3)})

    @staticmethod
    def call(ops, fx, inp, v=0):
        dst = torch.empty_like(inp["src"])
        ops.copy_bytes(inp["src"], dst)
        return [dst]


@entry("copy_bytes to pinned", covers=("copy_bytes",))
class _CopyBytesPinned:
    fixed = staticmethod(lambda ops: {"dst": torch.zeros(125 * 187 + 3).pin_memory()})
    inputs = _CopyBytes.inputs

    @staticmethod
    def call(ops, fx, inp, v=0):
        ops.copy_bytes(inp["src"], fx["dst"])                 # (one pinned destination: the test copies it before the next run)
        return [fx["dst"]]


@entry("count_not_below", host_wait="count_not_below returns the count as a host integer: it reads the counter back")
class _CountNotBelow:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"x": _randn(seed, 4099)})

    @staticmethod
    def call(ops, fx, inp, v=0):
        return [torch.tensor([ops.count_not_below(inp["x"], 1.0)], dtype=torch.int32, device=DEV)]


@entry("split_weights")
class _SplitWeights:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"w": _randn(seed, 128, 9, 32)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.split_weights(inp["w"], check_range=False)])


@entry("split_weights check_range", covers=("split_weights",),
       host_wait="split_weights(check_range=True) counts the out-of-range weights on the host first (count_not_below)")
class _SplitWeightsChecked:
    fixed = nothing
    inputs = _SplitWeights.inputs
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.split_weights(inp["w"], check_range=True)])


@entry("split_activations")
class _SplitActivations:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"x": _randn(seed, N8, 64)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.split_activations(inp["x"])])


@entry("encoder_prep")
class _EncoderPrep:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"img": torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (HF, WF, 3), dtype=np.uint8))})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.encoder_prep(inp["img"])])


@entry("instance_norm")
class _InstanceNorm:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"x": _randn(seed, N8, 64), "res": torch.relu(_randn(seed + 1, N8, 64))})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.instance_norm(inp["x"], 1, inp["res"])])          # (in place on x)


# ---- correlation -------------------------------------------------------------------------------------------------------------------
def _fmaps(ops, seed):
    f1 = _randn(seed, P, N8, 256)
    return {"f1": f1, "f2": (f1 + 0.5 * _randn(seed + 7, P, N8, 256)).contiguous()}


@entry("corr_pyramid arith 0", covers=("corr_pyramid",))
class _CorrPyramid0:
    fixed = nothing
    inputs = staticmethod(_fmaps)
    call = staticmethod(lambda ops, fx, inp, v=0: ops.corr_pyramid(inp["f1"], inp["f2"], H8, W8, arith=ops.ARITH_F32))


@entry("corr_pyramid arith 1", covers=("corr_pyramid",))
class _CorrPyramid1:
    fixed = nothing
    inputs = staticmethod(_fmaps)
    call = staticmethod(lambda ops, fx, inp, v=0: ops.corr_pyramid(inp["f1"], inp["f2"], H8, W8, arith=ops.ARITH_SPLIT))


def _levels(ops, seed):
    """The four stored levels as payload (computed here, before anything is stalled) and the lookup coordinates."""
    d = _fmaps(ops, seed)
    lv = ops.corr_pyramid(d["f1"].to(DEV), d["f2"].to(DEV), H8, W8, arith=ops.ARITH_SPLIT)
    torch.cuda.synchronize()
    out = {f"lv{l}": t for l, t in enumerate(lv)}
    out["coords"] = _coords(seed)
    return out


@entry("corr_lookup")
class _CorrLookup:
    fixed = nothing
    inputs = staticmethod(_levels)
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.corr_lookup([inp[f"lv{l}"] for l in range(4)], inp["coords"], H8, W8)])


def _convc1_fixed(ops):
    wpk = ops.pack_conv_weight(_randn(3, 256, 324, 1, 1, scale=0.05).to(DEV))
    return {"wf": ops.pack_lookup_convc1_weights(wpk), "bias": _randn(4, 256).to(DEV)}


@entry("corr_lookup_convc1")
class _CorrLookupConvc1:
    fixed = staticmethod(_convc1_fixed)
    inputs = staticmethod(_levels)
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.corr_lookup_convc1([inp[f"lv{l}"] for l in range(4)], inp["coords"], H8, W8,
                                                                          fx["wf"], fx["bias"], out_split=True)])


@entry("fmap_pyramid")
class _FmapPyramid:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"f2": _randn(seed, P, N8, 256)})
    call = staticmethod(lambda ops, fx, inp, v=0: ops.fmap_pyramid(inp["f2"], H8, W8)[1:])


def _ondemand_inputs(ops, seed):
    d = _fmaps(ops, seed)
    lv = ops.fmap_pyramid(d["f2"].to(DEV), H8, W8)
    torch.cuda.synchronize()
    return {"f1": d["f1"], "f2l0": lv[0], "f2l1": lv[1], "f2l2": lv[2], "f2l3": lv[3], "coords": _coords(seed)}


@entry("corr_lookup_ondemand")
class _CorrLookupOndemand:
    fixed = nothing
    inputs = staticmethod(_ondemand_inputs)
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.corr_lookup_ondemand(inp["f1"], [inp[f"f2l{l}"] for l in range(4)], inp["coords"], H8, W8)])


# ---- the pack_* wrappers that launch kernels (their payload is the weight) --------------------------------------------------------
@entry("pack_lookup_convc1_weights")
class _PackLookup:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"w": _randn(seed, 256, 1, 352, scale=0.05)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.pack_lookup_convc1_weights(inp["w"])])


@entry("pack_tile_conv_weights")
class _PackTile:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"w": _randn(seed, 256, 9, 128, scale=0.05)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.pack_tile_conv_weights(inp["w"], 256, 128, check_range=False)])


@entry("pack_flow_head_weights")
class _PackFlowHead:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"w": _randn(seed, 128, 9, 256, scale=0.05)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.pack_flow_head_weights(inp["w"], check_range=False)])


@entry("pack_ou_heads_weights")
class _PackOuHeads:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"w1": _randn(seed, 256, 9, 736, scale=0.02), "w2": _randn(seed + 1, 128, 9, 256, scale=0.05)})
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.pack_ou_heads_weights(inp["w1"], inp["w2"], check_range=False)))


@entry("pack_flow_branch_weights")
class _PackFlowBranch:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"w98": _randn(seed, 98, 128, scale=0.1), "w2": _randn(seed + 1, 128, 9, 128, scale=0.05)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.pack_flow_branch_weights(inp["w98"], inp["w2"], check_range=False)])


# ---- convolutions and heads --------------------------------------------------------------------------------------------------------
def _conv_fixed(ops):
    wpk = ops.pack_conv_weight(_randn(5, 96, 64, 3, 3, scale=0.05).to(DEV))
    return {"wpk": wpk, "wsplit": ops.split_weights(wpk), "bias": _randn(6, 96).to(DEV)}


@entry("conv2d")
class _Conv2d:
    fixed = staticmethod(_conv_fixed)
    inputs = staticmethod(lambda ops, seed: {"x": _randn(seed, P * N8, 64)})

    @staticmethod
    def call(ops, fx, inp, v=0):
        return [ops.conv2d(inp["x"], fx["wpk"], fx["bias"], P, H8, W8, 96, 3, 3, act="relu"),
                ops.conv2d(inp["x"], fx["wsplit"], fx["bias"], P, H8, W8, 96, 3, 3, act="relu", arith=ops.ARITH_SPLIT),
                ops.conv2d(inp["x"], fx["wpk"], fx["bias"], P, H8, W8, 96, 3, 3, tile=2)]


def _tile_fixed(ops):
    wpk = ops.pack_conv_weight(_randn(8, 256, 128, 3, 3, scale=0.05).to(DEV))
    return {"wtile": ops.pack_tile_conv_weights(wpk, 256, 128), "bias": _randn(9, 256).to(DEV)}


def _split_rows(cols, scale=1.0):
    def make(ops, seed):
        x = ops.split_activations((_randn(seed, P * N8, cols) * scale).to(DEV))
        torch.cuda.synchronize()
        return {"x": x}
    return make


@entry("tile_conv2d")
class _TileConv2d:
    fixed = staticmethod(_tile_fixed)
    inputs = staticmethod(_split_rows(128))
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.tile_conv2d(inp["x"], fx["wtile"], fx["bias"], P, H8, W8, 256, 3, 3, act="relu")])


def _gru_fixed(ops):
    pack = lambda wt, n: ops.pack_tile_conv_weights(ops.pack_conv_weight(wt.to(DEV)), n, 256)      # noqa: E731
    return {"wzr": pack(_randn(10, 256, 256, 1, 5, scale=0.04), 256), "wq": pack(_randn(11, 128, 256, 1, 5, scale=0.04), 128)}


def _gru_inputs(ops, seed):
    hf = torch.tanh(_randn(seed, P * N8, 128)).to(DEV)
    out = {"hf": hf, "hs": ops.split_activations(hf), "mo": ops.split_activations(torch.relu(_randn(seed + 1, P * N8, 128)).to(DEV)),
           "pre_zr": _randn(seed + 2, P * N8, 256, scale=0.5), "pre_q": _randn(seed + 3, P * N8, 128, scale=0.5)}
    torch.cuda.synchronize()
    return out


@entry("gru_half")
class _GruHalf:
    fixed = staticmethod(_gru_fixed)
    inputs = staticmethod(_gru_inputs)
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.gru_half(inp["hs"], inp["mo"], fx["wzr"], fx["wq"], inp["pre_zr"], inp["pre_q"],
                                                                    inp["hf"], P, H8, W8)))


def _ou_fixed(ops):
    w1 = _randn(12, 256, 712, 3, 3, scale=0.02)
    w2 = torch.zeros(3, 256, 3, 3)
    w2[0:2, 0:128] = _randn(13, 2, 128, 3, 3, scale=0.05)
    w2[2:3, 128:256] = _randn(14, 1, 128, 3, 3, scale=0.05)
    wtile, wproj = ops.pack_ou_heads_weights(ops.pack_conv_weight(w1.to(DEV)), ops.pack_conv_weight(w2.to(DEV)))
    return {"wtile": wtile, "wproj": wproj, "b1": _randn(15, 256, scale=0.1).to(DEV), "b2": _randn(16, 3).to(DEV)}


@entry("ou_heads")
class _OuHeads:
    fixed = staticmethod(_ou_fixed)
    inputs = staticmethod(_split_rows(712))
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.ou_heads(inp["x"], H8, W8, fx["wtile"], fx["b1"], fx["wproj"], fx["b2"])])


def _fh_fixed(ops):
    return {"wtile": ops.pack_tile_conv_weights(ops.pack_conv_weight(_randn(17, 256, 128, 3, 3, scale=0.05).to(DEV)), 256, 128),
            "wproj": ops.pack_flow_head_weights(ops.pack_conv_weight(_randn(18, 2, 256, 3, 3, scale=0.05).to(DEV))),
            "b1": _randn(19, 256, scale=0.1).to(DEV), "b2": _randn(20, 2, scale=0.1).to(DEV)}


def _fh_inputs(ops, seed):
    d = _split_rows(128)(ops, seed)
    d["coords"] = _randn(seed + 1, P * N8, 2)
    return d


@entry("flow_head")
class _FlowHead:
    fixed = staticmethod(_fh_fixed)
    inputs = staticmethod(_fh_inputs)

    @staticmethod
    def call(ops, fx, inp, v=0):
        delta = ops.flow_head(inp["x"], H8, W8, fx["wtile"], fx["b1"], fx["wproj"], fx["b2"], coords=inp["coords"])
        return [delta, inp["coords"]]                                                              # (coords += delta in place)


def _fb_fixed(ops):
    w98 = _randn(21, 128, 2, 7, 7, scale=0.1).permute(2, 3, 1, 0).reshape(98, 128).contiguous().to(DEV)
    return {"wflow": ops.pack_flow_branch_weights(w98, ops.pack_conv_weight(_randn(22, 64, 128, 3, 3, scale=0.05).to(DEV))),
            "b1": _randn(23, 128, scale=0.1).to(DEV), "b2": _randn(24, 64, scale=0.1).to(DEV)}


@entry("flow_branch")
class _FlowBranch:
    fixed = staticmethod(_fb_fixed)
    inputs = staticmethod(lambda ops, seed: {"coords": _coords(seed, 4.0)})

    @staticmethod
    def call(ops, fx, inp, v=0):
        hx = torch.zeros(P * N8, 384, device=DEV)
        return [ops.flow_branch(inp["coords"], H8, W8, fx["wflow"], fx["b1"], fx["b2"], hx=hx), hx]


def _up_inputs(ops, seed):
    return {"flow_lr": _randn(seed, P * N8, 2, scale=2.0), "ou": _randn(seed + 1, P * N8, 4), "mask": _randn(seed + 2, P * N8, 576)}


@entry("convex_upsample planar", covers=("convex_upsample",))
class _Upsample:
    fixed = nothing
    inputs = staticmethod(_up_inputs)
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.convex_upsample(inp["flow_lr"], inp["ou"], inp["mask"], P, H8, W8, pads=(3, 2, 1, 4))))


@entry("convex_upsample packed", covers=("convex_upsample",))
class _UpsamplePacked:
    fixed = nothing
    inputs = staticmethod(_up_inputs)
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.convex_upsample(inp["flow_lr"], inp["ou"], inp["mask"], P, H8, W8, pads=(3, 2, 1, 4),
                                                                           want_packed=True)))


# ---- chaining and selection --------------------------------------------------------------------------------------------------------
K = 3
THR = 0.5


def _lr(ops, seed):
    return dict(_results(seed, K, "L"), **_results(seed + 3, K, "R"))


@entry("chain")
class _Chain:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: dict(_results(seed, 1, "L"), **_results(seed + 3, 1, "R")))
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.chain(_triples(inp, 1, "L")[0], _triples(inp, 1, "R")[0])))


@entry("warp_backward")
class _WarpBackward:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"flow": field(seed)[0], "img": _randn(seed, 3, HF, WF)})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.warp_backward(inp["flow"], inp["img"])])


@entry("select")
class _Select:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: _results(seed, K, "C"))
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.select(_triples(inp, K, "C"), THR, want_chosen=True)))


@entry("chain_select")
class _ChainSelect:
    fixed = nothing
    inputs = staticmethod(_lr)
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.chain_select(_triples(inp, K, "L"), _triples(inp, K, "R"), THR, want_chosen=True)))


def _lr_packed(ops, seed):
    d = _results(seed, K, "L")
    d.update({f"R{k}": _packed_of(*field((seed + 3) * 16 + k)) for k in range(K)})
    return d


@entry("chain_select_packed")
class _ChainSelectPacked:
    fixed = nothing
    inputs = staticmethod(_lr_packed)
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.chain_select_packed(_triples(inp, K, "L"), [inp[f"R{k}"] for k in range(K)], THR,
                                                                               want_chosen=True)))


@entry("chain_select_multi")
class _ChainSelectMulti:
    fixed = nothing
    inputs = staticmethod(_lr_packed)

    @staticmethod
    def call(ops, fx, inp, v=0):
        Ls, Rs = _triples(inp, K, "L"), [inp[f"R{k}"] for k in range(K)]
        res = ops.chain_select_multi([(Ls, Rs), (Ls[:2], Rs[1:])], THR, want_chosen=True)       # (a right operand under both templates)
        return [t for r in res for t in r]


def _points(n, seed=0):
    r = np.random.default_rng(100 + seed)
    xy = r.uniform(-2, max(HF, WF) + 2, size=(n, 2)).astype(np.float32)
    xy[0] = (3.25, 7.5)
    xy[1] = (WF - 1.0, HF - 1.0)
    return torch.from_numpy(xy)


@entry("sample_points")
class _SamplePoints:
    fixed = staticmethod(lambda ops: {"tmpl": (torch.arange(67, dtype=torch.int32) % 2).to(DEV), "xy": _points(67).to(DEV)})
    inputs = staticmethod(lambda ops, seed: _results(seed, 2, "S"))

    @staticmethod
    def call(ops, fx, inp, v=0):
        table = torch.full((67, 3, 4), -7.0, device=DEV)
        return [ops.sample_points(_triples(inp, 2, "S"), fx["tmpl"], fx["xy"], table, 1)]


# ---- splat and overlays --------------------------------------------------------------------------------------------------------------
@entry("splat_forward")
class _Splat:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"flow": field(seed)[0], "img": torch.rand(HF, WF, 3, generator=_g(seed))})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.splat_forward(inp["flow"], inp["img"], 1.0)])


def _overlay_inputs(ops, seed):
    r = np.random.default_rng(200 + seed)
    f, o, _ = field(seed)
    edit = r.integers(0, 256, (HF, WF, 4), dtype=np.uint8)
    return {"flow": f, "occl": o, "edit": torch.from_numpy(edit), "frame": torch.from_numpy(r.integers(0, 256, (HF, WF, 3), dtype=np.uint8))}


@entry("overlay_edit")
class _OverlayEdit:
    fixed = nothing
    inputs = staticmethod(_overlay_inputs)

    @staticmethod
    def call(ops, fx, inp, v=0):
        acc = ops.splat_accumulator(4, HF, WF, DEV)
        return [ops.overlay_edit(inp["flow"], inp["occl"], inp["edit"], inp["frame"], acc, 255.0), acc]


def _dots_inputs(ops, seed):
    r = np.random.default_rng(300 + seed)
    table = np.concatenate([r.uniform(0, [WF, HF], size=(41, 2)), r.uniform(0, 0.4, size=(41, 1)), np.full((41, 1), 0.3)], 1).astype(np.float32)
    return {"table": torch.from_numpy(table), "frame": torch.from_numpy(r.integers(0, 256, (HF, WF, 3), dtype=np.uint8))}


@entry("overlay_dots")
class _OverlayDots:
    fixed = nothing
    inputs = staticmethod(_dots_inputs)
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.overlay_dots(inp["frame"], inp["table"], radius=2.5)])


# ---- codec -------------------------------------------------------------------------------------------------------------------------
@entry("quantize_u16")
class _Quantize:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"x": field(seed)[0][0].contiguous()})
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.quantize_u16(inp["x"])))


@entry("dequantize_u16")
class _Dequantize:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: {"q": torch.from_numpy(np.random.default_rng(seed).integers(0, 65536, (HF, WF), dtype=np.uint16))})
    call = staticmethod(lambda ops, fx, inp, v=0: [ops.dequantize_u16(inp["q"], -3.5, 9.25)])


# ---- track store -------------------------------------------------------------------------------------------------------------------
@entry("trackstore_append")
class _Append:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: _results(seed, 1, "A"))

    @staticmethod
    def call(ops, fx, inp, v=0):
        packed = torch.full((HF, WF, 4), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16)
        lohi = torch.full((4, 2), -7.0, device=DEV)
        return list(ops.trackstore_append(_triples(inp, 1, "A")[0], packed, lohi))


@entry("trackstore_append_multi")
class _AppendMulti:
    fixed = nothing
    inputs = staticmethod(lambda ops, seed: _results(seed, 3, "A"))

    @staticmethod
    def call(ops, fx, inp, v=0):
        packed = torch.full((3, HF, WF, 4), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16)
        lohi = torch.full((3, 4, 2), -7.0, device=DEV)
        ops.trackstore_append_multi([(t, packed[j], lohi[j]) for j, t in enumerate(_triples(inp, 3, "A"))])
        return [packed, lohi]


FPC, CHUNKS = 2, 2             # a store of two chunks, two frames each


def _store(ops, seed):
    """The store's chunks as payload: quantised frames [FPC, H, W, 4] uint16 and their (min, max) tables [FPC, 4, 2], appended here,
    before anything is stalled.  Frame 0 of the store is the identity (a template maps onto itself), the others are smooth flows."""
    out = {}
    for c in range(CHUNKS):
        packed = torch.zeros((FPC, HF, WF, 4), dtype=torch.int16, device=DEV).view(torch.uint16)
        lohi = torch.zeros((FPC, 4, 2), device=DEV)
        for j in range(FPC):
            f, o, s = field(seed * 16 + c * FPC + j)
            if c == 0 and j == 0:
                f = torch.zeros_like(f)
            ops.trackstore_append(tuple(t.to(DEV) for t in (f, o * 0.4, s)), packed[j], lohi[j])
        out[f"chunk{c}"], out[f"lohi{c}"] = packed, lohi
    torch.cuda.synchronize()
    return out


def _chunks(inp):
    return [inp[f"chunk{c}"] for c in range(CHUNKS)], [inp[f"lohi{c}"] for c in range(CHUNKS)]


@entry("trackstore_unpack")
class _Unpack:
    fixed = nothing
    inputs = staticmethod(_store)
    call = staticmethod(lambda ops, fx, inp, v=0: list(ops.trackstore_unpack(inp["chunk1"][1], inp["lohi1"][1])))


NQ = 67
SLOTS = ([3, 0, 2], [1, 2, 0])                                 # the slot list of the first and of the second call behind one stall
POINT_SLOTS = (np.arange(NQ) % 4, (np.arange(NQ) * 3 + 1) % 4)


@entry("trackstore_query", tables=True)
class _Query:
    fixed = staticmethod(lambda ops: {"slots": [torch.tensor(s, dtype=torch.int32, device=DEV) for s in SLOTS],
                                      "xy": [_points(NQ, v).to(DEV) for v in (0, 1)]})
    inputs = staticmethod(_store)

    @staticmethod
    def call(ops, fx, inp, v=0):
        table = torch.full((NQ, 4, 4), -7.0, device=DEV)
        return [ops.trackstore_query(*_chunks(inp), fx["slots"][v], fx["xy"][v], table, column0=1)]


@entry("trackstore_locate", covers=("trackstore_locate", "trackstore_locate_frames"), tables=True)
class _Locate:
    fixed = staticmethod(lambda ops: {"xy": [_points(NQ, v).to(DEV) for v in (0, 1)]})
    inputs = staticmethod(_store)

    @staticmethod
    def call(ops, fx, inp, v=0):
        out = list(ops.trackstore_locate(*_chunks(inp), POINT_SLOTS[v], fx["xy"][v], torch.full((NQ, 4), -7.0, device=DEV),
                                         torch.full((NQ,), -7, dtype=torch.int32, device=DEV)))
        frames = [(inp[f"chunk{c}"][j], inp[f"lohi{c}"][j]) for c in range(CHUNKS) for j in range(FPC)]
        out += list(ops.trackstore_locate_frames(frames, POINT_SLOTS[1 - v], fx["xy"][v], torch.full((NQ, 4), -7.0, device=DEV),
                                                 torch.full((NQ,), -7, dtype=torch.int32, device=DEV)))
        return out


@entry("trackstore_invert", tables=True)
class _Invert:
    fixed = nothing
    inputs = staticmethod(_store)

    @staticmethod
    def call(ops, fx, inp, v=0):
        G = len(SLOTS[v])
        return list(ops.trackstore_invert(*_chunks(inp), SLOTS[v], torch.full((G, HF, WF, 4), -7.0, device=DEV),
                                          torch.full((G, HF, WF), -7, dtype=torch.int32, device=DEV)))


# (frames by slot, first_of, rank_of) per call: the same number of frames and of planes in both, so that the tables of the two calls have
# one layout and only their contents differ (a table read in place of the other still names frames of the store)
ATLAS = (([3, 1, 2, 0], [0, 2, 4], [0, 1, 0, 1]), ([0, 2, 1, 3], [0, 1, 4], [0, 0, 1, 2]))


@entry("trackstore_invert_atlas", tables=True)
class _InvertAtlas:
    fixed = nothing
    inputs = staticmethod(_store)

    @staticmethod
    def call(ops, fx, inp, v=0):
        slots, first_of, rank_of = ATLAS[v]
        G = len(first_of) - 1
        frames = [(inp[f"chunk{s // FPC}"][s % FPC], inp[f"lohi{s // FPC}"][s % FPC]) for s in slots]
        return list(ops.trackstore_invert_atlas(frames, first_of, rank_of, torch.full((G, HF, WF, 4), -7.0, device=DEV),
                                                torch.full((G, HF, WF), -7, dtype=torch.int32, device=DEV),
                                                torch.full((G, HF, WF), -7, dtype=torch.int32, device=DEV)))


def _flow_from_fixed(ops):
    """The plane ``trackstore_flow_from`` follows: template points on the pixel grid pushed about by a smooth field, and an entry plane
    with ranks 0, 1 and -1 (not found).  Address material: it is the same for every input set."""
    f, o, s = field(900)
    ys, xs = torch.meshgrid(torch.arange(HF, dtype=torch.float32), torch.arange(WF, dtype=torch.float32), indexing="ij")
    table = torch.stack([xs + 0.5 * f[0], ys + 0.5 * f[1], o[0] * 0.3, s[0]], -1).contiguous()
    entry_plane = ((xs.int() // 7 + ys.int() // 5) % 3 - 1).to(torch.int32).contiguous()
    return {"table": table.to(DEV), "entry": entry_plane.to(DEV)}


FLOW_COLUMNS = ([[0, 1, 3, -1, 2], [2, 2, -1, 0, 1]], [[3, -1, 0, 1, 1], [1, 0, 2, -1, 3]])      # slot per (row, column) and call; -1: not covered


@entry("trackstore_flow_from", covers=("trackstore_flow_from",), tables=True)
class _FlowFrom:
    fixed = staticmethod(_flow_from_fixed)
    inputs = staticmethod(_store)

    @staticmethod
    def call(ops, fx, inp, v=0):
        slots = np.asarray(FLOW_COLUMNS[v])
        frame_ptrs, lohi_ptrs = ops.trackstore_slot_addresses(*_chunks(inp), slots)
        T = slots.shape[1]
        return list(ops.trackstore_flow_from(fx["table"], fx["entry"], [0, 1] if v == 0 else [1, 0], frame_ptrs, lohi_ptrs,
                                             torch.full((T, 2, HF, WF), -7.0, device=DEV), torch.full((T, 1, HF, WF), -7.0, device=DEV),
                                             torch.full((T, 1, HF, WF), -7.0, device=DEV), columns_per_block=2))


# ---- what the catalog does not hold ------------------------------------------------------------------------------------------------
# Methods of the handles that tests/test_gpu_streams_handles.py stalls, by the name the completeness test finds them under.
HANDLE_TESTS = {          # (tests/test_gpu_streams_ops.py holds every value to a test function of that file)
    "EncoderEngine.forward": "test_encoder_forward_is_ordered",
    "RaftEngine.refine": "test_refine_is_ordered",
    "RaftEngine.prepare_frame": "test_refine_is_ordered",                 # its "lists prepared" schedule
    "RaftEngine.nonfinite_snapshot": "test_nonfinite_snapshot_carries_its_own_call",
}

# Functions whose body names _stream() and that need no entry, each with its reason.
EXEMPT = {
    "_locate_call": "private: the body of trackstore_locate and trackstore_locate_frames, both in the catalog",
}


def covered():
    return {name for e in ENTRIES for name in e.covers}
