"""Torch-tensor front end of the C ABI (device memory + streams are PyTorch's;
all arithmetic happens in libmftx's HIP kernels).

Every function checks device / dtype / contiguity, passes raw device pointers
and the current HIP stream, and raises ``MftxError`` on a non-zero return --
same contract as the reference's one native op
(``MFT/RAFT/alt_cuda_corr/correlation.cpp:19-33``: CHECK_CUDA, CHECK_CONTIGUOUS,
RuntimeError).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, MftxError, check

ACT = {None: 0, "none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_visible(t):
    """A tensor a kernel may address: device memory, or pinned host memory (mapped into the device's address space)."""
    return isinstance(t, torch.Tensor) and (t.is_cuda or t.is_pinned())


def copy_bytes(src: torch.Tensor, dst: torch.Tensor):
    """dst <- src by a copy KERNEL on the current stream (``mftx_copy_bytes``): either side may be pinned host memory.  No
    SDMA queue is involved, so uploads and downloads enqueued this way do not serialise behind each other."""
    if not (_device_visible(src) and _device_visible(dst)):
        raise MftxError("copy_bytes: tensors must be on the device or in pinned host memory")
    if not (src.is_contiguous() and dst.is_contiguous()) or src.numel() * src.element_size() != dst.numel() * dst.element_size():
        raise MftxError("copy_bytes: contiguous tensors of the same size in bytes")
    nbytes = src.numel() * src.element_size()
    if nbytes:                                    # (an empty tensor has no storage: its data_ptr() is null, which the library refuses)
        check(_lib.load().mftx_copy_bytes(src.data_ptr(), dst.data_ptr(), nbytes, _stream()), "mftx_copy_bytes")
    return dst


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MftxError(f"{name} must be a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise MftxError(f"{name} must be {dtype}")
    if not t.is_contiguous():
        raise MftxError(f"{name} must be contiguous")
    return t.data_ptr()


# ---------------------------------------------------------------------------
# weight packing (host plumbing, once per checkpoint)
# ---------------------------------------------------------------------------

def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, kh, kw] -> [round_up(Cout,128), kh*kw, round_up(Cin,32)], zero
    padded: the K axis (tap, cin) is contiguous per output channel, which is what
    the NT implicit-GEMM kernel streams (csrc/conv_gemm.hip)."""
    cout, cin, kh, kw = w.shape
    n_pad = -(-cout // 128) * 128
    c_pad = -(-cin // 32) * 32
    out = torch.zeros(n_pad, kh * kw, c_pad, dtype=torch.float32, device=w.device)
    out[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    return out.contiguous()


ARITH_F32, ARITH_SPLIT = 0, 1


class SplitRangeError(MftxError):
    """An operand of the split arithmetic is not below 65504 in magnitude (or not finite)."""


def count_not_below(x: torch.Tensor, limit: float) -> int:
    """Number of elements of a float32 device tensor with !(|x| < limit) -- NaN counts; limit = inf counts the
    non-finite ones (``mftx_count_not_below``).  Synchronises (reads one counter back)."""
    lib = _lib.load()
    if x.numel() == 0:
        return 0
    x = x if x.is_contiguous() else x.contiguous()
    cnt = torch.zeros(1, dtype=torch.int32, device=x.device)
    check(lib.mftx_count_not_below(_chk(x, "x"), x.numel(), float(limit), cnt.data_ptr(), _stream()), "mftx_count_not_below")
    return int(cnt.item())


def split_weights(wpk: torch.Tensor, check_range: bool = True) -> torch.Tensor:
    """Packed fp32 conv weights -> the split-fp16 form (same shape and size) that ``conv2d(arith=ARITH_SPLIT)``
    and the refinement engine's split arithmetic stream (csrc/conv_gemm.hip: split_weights_kernel).
    check_range (weights: always; it costs one host sync at load): values that are not below 65504 in magnitude have no
    finite fp16 high half -- ``SplitRangeError`` instead of NaN products later."""
    lib = _lib.load()
    if check_range:
        bad = count_not_below(wpk, _lib.SPLIT_LIMIT)
        if bad:
            raise SplitRangeError(f"split arithmetic: {bad} of {wpk.numel()} values are not below {_lib.SPLIT_LIMIT:g} "
                                  "in magnitude (fp16 range of the high halves); use arith='fp32'")
    out = torch.empty_like(wpk)
    check(lib.mftx_split_weights(_chk(wpk, "wpk"), out.data_ptr(), wpk.numel(), _stream()), "mftx_split_weights")
    return out


def split_activations(x: torch.Tensor) -> torch.Tensor:
    """fp32 [M, C] (C % 8 == 0) -> the split form the engine stores GEMM inputs in: every 8 channels of a row as
    [hi x 8 | lo x 8] fp16 (same shape and dtype as a container).  The same kernel as ``split_weights``; no range check
    (activations out of range surface as NaN, see ``mftx_count_not_below``)."""
    return split_weights(x, check_range=False)


def unsplit_activations(x: torch.Tensor) -> torch.Tensor:
    """Inverse of ``split_activations`` (exact: hi + lo / 2048 is representable in fp32)."""
    m, c = x.shape
    h = x.contiguous().view(torch.float16).reshape(m, c // 8, 2, 8).float()
    return (h[:, :, 0] + h[:, :, 1] * (1.0 / 2048.0)).reshape(m, c)


def pack_raft_weights(sd: dict, device) -> list:
    """The 30 tensors ``mftx_raft_create`` expects, in WeightSlot order
    (csrc/raft_engine.hip).  z|r gates and the two OU heads are fused into single
    GEMMs by stacking / block-placing their weights (exact: the extra terms are
    multiplications by zero weights)."""
    g = lambda k: sd[k].to(device=device, dtype=torch.float32)  # noqa: E731
    u, o = "update_block.", "occlusion_block."
    out = []

    def conv(name):
        out.append(pack_conv_weight(g(name + ".weight")))
        out.append(g(name + ".bias").contiguous())

    conv(u + "encoder.convc1")
    conv(u + "encoder.convc2")
    # convf1: [128, 2, 7, 7] -> [(ky, kx, c), co] for the direct kernel
    out.append(g(u + "encoder.convf1.weight").permute(2, 3, 1, 0).reshape(98, 128).contiguous())
    out.append(g(u + "encoder.convf1.bias").contiguous())
    conv(u + "encoder.convf2")
    conv(u + "encoder.conv")
    # GRU gates: input channels are [h(128) | inp(128) | motion(128)].  The inp columns are split off
    # (they are evaluated once per pair, csrc/raft_engine.hip); the remaining [h | motion] columns form
    # the per-iteration GEMM.
    dyn = list(range(0, 128)) + list(range(256, 384))
    for sfx in ("1", "2"):
        wzr = torch.cat([g(u + f"gru.convz{sfx}.weight"), g(u + f"gru.convr{sfx}.weight")], 0)
        out.append(pack_conv_weight(wzr[:, dyn].contiguous()))
        out.append(pack_conv_weight(wzr[:, 128:256].contiguous()))
        out.append(torch.cat([g(u + f"gru.convz{sfx}.bias"), g(u + f"gru.convr{sfx}.bias")]).contiguous())
        wq = g(u + f"gru.convq{sfx}.weight")
        out.append(pack_conv_weight(wq[:, dyn].contiguous()))
        out.append(pack_conv_weight(wq[:, 128:256].contiguous()))
        out.append(g(u + f"gru.convq{sfx}.bias").contiguous())
    conv(u + "flow_head.conv1")
    conv(u + "flow_head.conv2")
    conv(u + "mask.0")
    conv(u + "mask.2")
    w1 = torch.cat([g(o + "occl_head.conv1.weight"), g(o + "uncertainty_head.conv1.weight")], 0)
    out.append(pack_conv_weight(w1))
    out.append(torch.cat([g(o + "occl_head.conv1.bias"), g(o + "uncertainty_head.conv1.bias")]).contiguous())
    w2 = torch.zeros(3, 256, 3, 3, dtype=torch.float32, device=device)
    w2[0:2, 0:128] = g(o + "occl_head.conv2.weight")
    w2[2:3, 128:256] = g(o + "uncertainty_head.conv2.weight")
    out.append(pack_conv_weight(w2))
    out.append(torch.cat([g(o + "occl_head.conv2.bias"), g(o + "uncertainty_head.conv2.bias")]).contiguous())
    assert len(out) == _lib.NUM_RAFT_WEIGHTS
    return out


_ENC_CONVS = ["conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.1.conv1", "layer1.1.conv2",
              "layer2.0.conv1", "layer2.0.conv2", "layer2.0.downsample.0", "layer2.1.conv1", "layer2.1.conv2",
              "layer3.0.conv1", "layer3.0.conv2", "layer3.0.downsample.0", "layer3.1.conv1", "layer3.1.conv2",
              "conv2"]


def _bn_name(conv_name):
    """BatchNorm that follows a conv of BasicEncoder (core/extractor.py:6-62,118-166)."""
    if conv_name == "conv1":
        return "norm1"
    if conv_name.endswith("downsample.0"):
        return conv_name[:-1] + "1"
    if conv_name == "conv2":
        return None
    blk, c = conv_name.rsplit(".", 1)
    return f"{blk}.norm{c[-1]}"


def pack_encoder_weights(sd: dict, prefix: str, batch_norm: bool, device) -> list:
    """(packed weight, bias) per conv of a BasicEncoder, in EncConv order
    (csrc/encoder.hip).  Eval-mode batch norm (cnet) is folded into the conv:
    BN(conv_w(x) + b) = conv_{w*s}(x) + (b*s + t), s = gamma/sqrt(var+eps), t = beta - mean*s.
    The 7x7 stem is repacked as 7 row taps over 28-float (7 pixels x RGB0) windows; the cnet
    head is split into its tanh (net) and relu (inp) halves (core/raft.py:146-149)."""
    g = lambda k: sd[f"{prefix}.{k}"].to(device=device, dtype=torch.float32)  # noqa: E731
    out = []
    for name in _ENC_CONVS:
        w, b = g(name + ".weight"), g(name + ".bias")
        bn = _bn_name(name) if batch_norm else None
        if bn is not None:
            s_ = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + 1e-5)
            t_ = g(bn + ".bias") - g(bn + ".running_mean") * s_
            w = w * s_.reshape(-1, 1, 1, 1)
            b = b * s_ + t_
        if name == "conv1":                       # [64,3,7,7] -> [128][ky][kx*4 + c], c = 3 zero
            w4 = torch.zeros(64, 7, 7, 4, dtype=torch.float32, device=device)
            w4[..., :3] = w.permute(0, 2, 3, 1)
            pk = torch.zeros(128, 7, 32, dtype=torch.float32, device=device)
            pk[:64, :, :28] = w4.reshape(64, 7, 28)
            out += [pk.contiguous(), b.contiguous()]
        elif name == "conv2" and batch_norm:       # cnet head: net | inp halves
            out += [pack_conv_weight(w[:128].contiguous()), b[:128].contiguous(),
                    pack_conv_weight(w[128:].contiguous()), b[128:].contiguous()]
        else:
            out += [pack_conv_weight(w.contiguous()), b.contiguous()]
    return out


class EncoderEngine:
    """Handle on the native encoder runtime (``mftx_encoder_*``): fnet or cnet."""

    def __init__(self, state_dict: dict, prefix: str, instance_norm: bool, device, arith=None, graph=True):
        """graph: replay the layers between pre-processing and head as a hipGraph (``mftx_encoder_set_graph``)."""
        lib = _lib.load()
        self.device = torch.device(device)
        self.instance_norm = instance_norm
        self.weights = pack_encoder_weights(state_dict, prefix, not instance_norm, self.device)
        arr, self._keep = _lib.ptr_array([_chk(t, "weight") for t in self.weights])
        handle = C.c_void_p()
        check(lib.mftx_encoder_create(arr, len(self.weights), int(instance_norm), C.byref(handle)),
              "mftx_encoder_create")
        self._h = handle
        self._ws = None
        if not graph:
            check(lib.mftx_encoder_set_graph(self._h, 0), "mftx_encoder_set_graph")
        self.arith = ARITH_SPLIT if arith is None else int(arith)
        if self.arith == ARITH_SPLIT:           # split-fp16 products: the convolutions stream split weights
            self.split = [split_weights(t) for t in self.weights[0::2]]
            sarr, self._keep_split = _lib.ptr_array([t.data_ptr() for t in self.split])
            check(lib.mftx_encoder_set_split_weights(self._h, sarr, len(self.split)), "mftx_encoder_set_split_weights")
        elif self.arith != ARITH_F32:
            raise MftxError(f"unknown arithmetic {arith!r}")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().mftx_encoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def forward(self, img_u8: torch.Tensor, out=None):
        """img_u8: uint8 [H0, W0, 3] BGR on the device -> pixel-major maps at 1/8 resolution.
        out: optional pre-allocated (out0, out1) to write into (contiguous [h*w, C] views)."""
        lib = _lib.load()
        H0, W0 = img_u8.shape[:2]
        h, w = -(-H0 // 8), -(-W0 // 8)
        need = lib.mftx_encoder_workspace_bytes(H0, W0)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out is not None:
            outs = out
            want = ((h * w, 256), None) if self.instance_norm else ((h * w, 128), (h * w, 128))
            for t, shp in zip(outs, want):
                if shp is not None and (t is None or tuple(t.shape) != shp):
                    raise MftxError(f"encoder output must be {shp}")
        elif self.instance_norm:
            outs = (torch.empty(h * w, 256, dtype=torch.float32, device=self.device), None)
        else:
            outs = (torch.empty(h * w, 128, dtype=torch.float32, device=self.device),
                    torch.empty(h * w, 128, dtype=torch.float32, device=self.device))
        check(lib.mftx_encoder_forward(self._h, _chk(img_u8, "img", torch.uint8), H0, W0, _chk(outs[0], "out0"),
                                       _chk(outs[1], "out1") if outs[1] is not None else None,
                                       self._ws.data_ptr(), self._ws.numel(), _stream()), "mftx_encoder_forward")
        return outs


def encoder_prep(img_u8: torch.Tensor) -> torch.Tensor:
    """The encoders' pre-processing kernel alone (``mftx_encoder_prep``): uint8 [H0, W0, 3] BGR on the device ->
    fp32 [Hp, Wp + 6, 4]: RGB0 of the replicate-padded frame as 2 (v / 255) - 1, three zero columns on either side."""
    lib = _lib.load()
    if img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise MftxError("encoder_prep: img must be [H0, W0, 3]")
    H0, W0 = int(img_u8.shape[0]), int(img_u8.shape[1])
    Hp, Wp = -(-H0 // 8) * 8, -(-W0 // 8) * 8
    out = torch.empty(Hp, Wp + 6, 4, dtype=torch.float32, device=img_u8.device)
    check(lib.mftx_encoder_prep(_chk(img_u8, "img", torch.uint8), H0, W0, out.data_ptr(), _stream()), "mftx_encoder_prep")
    return out


def instance_norm(x: torch.Tensor, mode: int, res: torch.Tensor = None, split: bool = False) -> torch.Tensor:
    """The encoders' normalisation pass alone (``mftx_instance_norm``), IN PLACE on x [rows, C] (returned): mode 0
    relu(n(x)), 1 relu(res + relu(n(x))), 2 n(x).  split: x is written -- and res read -- in split form."""
    lib = _lib.load()
    if x.dim() != 2:
        raise MftxError("instance_norm: x must be [rows, C]")
    rows, Cc = int(x.shape[0]), int(x.shape[1])
    if res is not None and tuple(res.shape) != (rows, Cc):
        raise MftxError("instance_norm: res must have the shape of x")
    need = lib.mftx_instance_norm_workspace_bytes(Cc)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    check(lib.mftx_instance_norm(_chk(x, "x"), rows, Cc, _chk(res, "res") if res is not None else None, int(mode),
                                 int(bool(split)), ws.data_ptr(), ws.numel(), _stream()), "mftx_instance_norm")
    return x


# ---------------------------------------------------------------------------
# per-op wrappers
# ---------------------------------------------------------------------------

def pyramid_layout(h: int, w: int):
    """(stride[4] floats per query cell, (hb0, wb0, hb1, wb1) block grids) of the correlation pyramid
    (include/mftx.h, mftx_corr_pyramid)."""
    stride, grid = (C.c_longlong * 4)(), (C.c_int * 4)()
    check(_lib.load().mftx_corr_pyramid_layout(h, w, stride, grid), "mftx_corr_pyramid_layout")
    return list(stride), tuple(grid)


def _level_index(l: int, h: int, w: int, device):
    """Flat offset inside a query's level-l slice of every (y, x) of the level, row-major order."""
    stride, (hb0, wb0, hb1, wb1) = pyramid_layout(h, w)
    hl, wl = h >> l, w >> l
    ys, xs = torch.meshgrid(torch.arange(hl, device=device), torch.arange(wl, device=device), indexing="ij")
    if l < 2:
        wb = (wb0, wb1)[l]
        idx = ((ys >> 2) * wb + (xs >> 3)) * 32 + (ys & 3) * 8 + (xs & 7)
    else:
        idx = ys * wl + xs
    return idx.reshape(-1), stride[l]


def unblock_level(t: torch.Tensor, l: int, h: int, w: int) -> torch.Tensor:
    """Level l as mftx_corr_pyramid stores it [P, h*w, stride_l] -> row-major [P, h*w, h_l*w_l]
    (the reference's layout; tests and tools only)."""
    idx, _ = _level_index(l, h, w, t.device)
    return t[..., idx].contiguous()


def block_level(t: torch.Tensor, l: int, h: int, w: int) -> torch.Tensor:
    """Inverse of ``unblock_level``: row-major [P, h*w, h_l*w_l] -> the stored layout, padding zero."""
    idx, stride = _level_index(l, h, w, t.device)
    out = torch.zeros(t.shape[:-1] + (stride,), dtype=t.dtype, device=t.device)
    out[..., idx] = t
    return out


def corr_pyramid(f1: torch.Tensor, f2: torch.Tensor, h: int, w: int, arith: int = ARITH_F32):
    """f1, f2: pixel-major [P, h*w, C] -> 4 levels [P, h*w, stride_l] in the stored layout
    (``unblock_level`` gives the reference's row-major view).  ``arith``: ARITH_F32 (fp32 MFMA) or ARITH_SPLIT
    (split-fp16 products, what the refinement engine runs by default)."""
    lib = _lib.load()
    P, N, Cc = f1.shape
    assert N == h * w and f2.shape == f1.shape
    stride, _ = pyramid_layout(h, w)
    lv = [torch.empty(P, N, stride[l], dtype=torch.float32, device=f1.device) for l in range(4)]
    if arith == ARITH_SPLIT:
        scratch = torch.empty_like(f2)
        check(lib.mftx_corr_pyramid_split(_chk(f1, "f1"), _chk(f2, "f2"), P, Cc, h, w,
                                          *[t.data_ptr() for t in lv], scratch.data_ptr(), _stream()), "mftx_corr_pyramid_split")
        return lv
    if arith != ARITH_F32:
        raise MftxError("corr_pyramid: arith must be ARITH_F32 or ARITH_SPLIT")
    check(lib.mftx_corr_pyramid(_chk(f1, "f1"), _chk(f2, "f2"), P, Cc, h, w,
                                *[t.data_ptr() for t in lv], _stream()), "mftx_corr_pyramid")
    return lv


def corr_lookup(lv, coords: torch.Tensor, h: int, w: int, r: int = 4):
    """lv: the 4 levels in the stored layout; coords pixel-major [P, h*w, 2] (x, y) -> [P, h*w, 324]."""
    lib = _lib.load()
    P = coords.shape[0]
    stride, _ = pyramid_layout(h, w)
    for l, t in enumerate(lv):
        if tuple(t.shape) != (P, h * w, stride[l]):
            raise MftxError(f"corr_lookup: level {l} must be [{P}, {h * w}, {stride[l]}]")
    out = torch.empty(P, h * w, 324, dtype=torch.float32, device=coords.device)
    check(lib.mftx_corr_lookup(*[_chk(t, "level") for t in lv], _chk(coords, "coords"), P, h, w, r,
                               out.data_ptr(), 324, _stream()), "mftx_corr_lookup")
    return out


def pack_lookup_convc1_weights(wpk: torch.Tensor) -> torch.Tensor:
    """convc1's weight in the ``pack_conv_weight`` form [256, 1, 352] -> the fragment stream of the fused
    lookup + convc1 kernel (``mftx_pack_lookup_convc1_weights``; opaque bytes)."""
    lib = _lib.load()
    if wpk.dim() != 3 or wpk.shape[0] != 256 or wpk.shape[1] != 1 or wpk.shape[2] < 324:
        raise MftxError("pack_lookup_convc1_weights: expected the packed convc1 weight [256, 1, >= 324]")
    out = torch.empty(_lib.LOOKUP_CONVC1_WEIGHT_BYTES, dtype=torch.uint8, device=wpk.device)
    check(lib.mftx_pack_lookup_convc1_weights(_chk(wpk, "wpk"), wpk.shape[2], out.data_ptr(), _stream()),
          "mftx_pack_lookup_convc1_weights")
    return out


def pack_tile_conv_weights(wpk: torch.Tensor, N: int, cin: int, check_range: bool = True) -> torch.Tensor:
    """A layer's weight in the ``pack_conv_weight`` form [>= N, taps, cin_pad] -> the weight stream of the tile-resident
    conv kernel (``mftx_pack_tile_conv_weights``; opaque bytes, N * taps * cin * 4 of them).  Operands of the split
    arithmetic: with ``check_range`` a value not below 65504 raises ``SplitRangeError``."""
    lib = _lib.load()
    if wpk.dim() != 3 or wpk.shape[0] < N or wpk.shape[2] < cin:
        raise MftxError("pack_tile_conv_weights: expected the packed weight [>= N, taps, >= cin]")
    if check_range:
        bad = count_not_below(wpk, _lib.SPLIT_LIMIT)
        if bad:
            raise SplitRangeError(f"pack_tile_conv_weights: {bad} weights are not below {_lib.SPLIT_LIMIT} in magnitude")
    taps = wpk.shape[1]
    out = torch.empty(N * taps * cin * 4, dtype=torch.uint8, device=wpk.device)
    check(lib.mftx_pack_tile_conv_weights(_chk(wpk, "wpk"), N, taps, cin, wpk.shape[2], out.data_ptr(), _stream()),
          "mftx_pack_tile_conv_weights")
    return out


def tile_conv2d(x: torch.Tensor, wtile: torch.Tensor, bias, P, h, w, N, kh, kw, act=None, x2=None, addend=None,
                out_split=False, out=None):
    """``conv2d(..., arith=ARITH_SPLIT, a_split=True)`` on the tile-resident kernel (``mftx_tile_conv2d``): x (and x2)
    [P*h*w, 128] in split form, wtile from ``pack_tile_conv_weights`` -> [P*h*w, N] (fp32, or split form)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(P * h * w, N, dtype=torch.float32, device=x.device)
    d = ConvDesc()
    d.a0, d.lda0, d.c0 = _chk(x, "x"), x.shape[1], x.shape[1]
    if x2 is not None:
        d.a1, d.lda1, d.c1 = _chk(x2, "x2"), x2.shape[1], x2.shape[1]
    else:
        d.a1, d.lda1, d.c1 = None, 0, 0
    d.wpk = None
    d.bias = _chk(bias, "bias") if bias is not None else None
    d.out, d.ldo = _chk(out, "out"), out.shape[1]
    d.P, d.h, d.w, d.N, d.kh, d.kw = P, h, w, N, kh, kw
    d.act, d.out_scale = ACT[act], 1.0
    d.addend, d.ld_addend = (_chk(addend, "addend"), addend.shape[1]) if addend is not None else (None, 0)
    d.arith, d.a_split, d.out_split = ARITH_SPLIT, 1, int(bool(out_split))
    check(lib.mftx_tile_conv2d(C.byref(d), _chk(wtile, "wtile", torch.uint8), _stream()), "mftx_tile_conv2d")
    return out


def gru_half(h_split, motion_split, wzr_tile, wq_tile, pre_zr, pre_q, hf, P, h, w, vertical=False):
    """One SepConvGRU pass as one kernel (``mftx_gru_half``): h_split / motion_split [M, 128] in split form, the gates' weights
    as ``pack_tile_conv_weights`` streams (cin = 256), pre_zr [M, 256] / pre_q [M, 128] the pre-activation addends, hf [M, 128]
    the fp32 h -> (new h in fp32 [M, 128], new h in split form [M, 128], the kernel's scratch [M, 128]: the z gate's
    sums before the context part and the sigmoid)."""
    M = P * h * w
    z = torch.empty(M, 128, dtype=torch.float32, device=hf.device)
    h_out = torch.empty(M, 128, dtype=torch.float32, device=hf.device)
    hf_out = torch.empty(M, 128, dtype=torch.float32, device=hf.device)
    check(_lib.load().mftx_gru_half(_chk(h_split, "h"), h_split.shape[1], _chk(motion_split, "motion"), motion_split.shape[1],
                                    _chk(wzr_tile, "wzr", torch.uint8), _chk(wq_tile, "wq", torch.uint8), _chk(pre_zr, "pre_zr"),
                                    _chk(pre_q, "pre_q"), _chk(z, "z"), _chk(hf, "hf"), _chk(hf_out, "hf_out"), _chk(h_out, "h_out"), 128, P, h, w,
                                    1 if vertical else 0, _stream()), "mftx_gru_half")
    return hf_out, h_out, z


def pack_flow_head_weights(w2pk: torch.Tensor, check_range: bool = True) -> torch.Tensor:
    """flow_head.conv2's weight in the ``pack_conv_weight`` form [>= 2, 9, 256] -> the projection matrix of the fused
    flow head (``mftx_pack_flow_head_weights``; opaque bytes)."""
    lib = _lib.load()
    if w2pk.dim() != 3 or w2pk.shape[0] < 2 or tuple(w2pk.shape[1:]) != (9, 256):
        raise MftxError("pack_flow_head_weights: expected the packed weight [>= 2, 9, 256]")
    if check_range and count_not_below(w2pk, _lib.SPLIT_LIMIT):
        raise SplitRangeError(f"pack_flow_head_weights: weights not below {_lib.SPLIT_LIMIT} in magnitude")
    out = torch.empty(_lib.FLOW_HEAD_WEIGHT_BYTES, dtype=torch.uint8, device=w2pk.device)
    check(lib.mftx_pack_flow_head_weights(_chk(w2pk, "w2pk"), out.data_ptr(), _stream()), "mftx_pack_flow_head_weights")
    return out


def pack_ou_heads_weights(w1pk: torch.Tensor, w2pk: torch.Tensor, check_range: bool = True):
    """The occlusion + uncertainty heads' layers in the ``pack_conv_weight`` form -- first layers stacked [>= 256, 9, cin_pad >= 712],
    second layers block-diagonal [>= 3, 9, 256] -> (wtile, wproj) of ``mftx_ou_heads`` (opaque bytes)."""
    lib = _lib.load()
    if w1pk.dim() != 3 or w1pk.shape[0] < 256 or w1pk.shape[1] != 9 or w1pk.shape[2] < 712:
        raise MftxError("pack_ou_heads_weights: expected the packed first layers [>= 256, 9, >= 712]")
    if w2pk.dim() != 3 or w2pk.shape[0] < 3 or tuple(w2pk.shape[1:]) != (9, 256):
        raise MftxError("pack_ou_heads_weights: expected the packed second layers [>= 3, 9, 256]")
    if check_range and (count_not_below(w1pk, _lib.SPLIT_LIMIT) or count_not_below(w2pk, _lib.SPLIT_LIMIT)):
        raise SplitRangeError(f"pack_ou_heads_weights: weights not below {_lib.SPLIT_LIMIT} in magnitude")
    wtile = torch.empty(_lib.OU_HEADS_WTILE_BYTES, dtype=torch.uint8, device=w1pk.device)
    wproj = torch.empty(_lib.FLOW_HEAD_WEIGHT_BYTES, dtype=torch.uint8, device=w1pk.device)
    check(lib.mftx_pack_ou_heads_weights(_chk(w1pk, "w1pk"), w1pk.shape[2], _chk(w2pk, "w2pk"), wtile.data_ptr(), wproj.data_ptr(), _stream()),
          "mftx_pack_ou_heads_weights")
    return wtile, wproj


def ou_heads(a_split: torch.Tensor, h: int, w: int, wtile: torch.Tensor, b1, wproj: torch.Tensor, b2):
    """Both layers of the occlusion and uncertainty heads (``mftx_ou_heads``): a_split [P*h*w, 712] split-form rows ->
    [P*h*w, 4] = occlusion logits 0, 1, log-variance, (unused)."""
    lib = _lib.load()
    M = a_split.shape[0]
    P = M // (h * w)
    T = torch.empty(M, 27, dtype=torch.float32, device=a_split.device)
    out = torch.zeros(M, 4, dtype=torch.float32, device=a_split.device)
    check(lib.mftx_ou_heads(_chk(a_split, "a"), a_split.shape[1], P, h, w, _chk(wtile, "wtile", torch.uint8), _chk(b1, "b1"),
                            _chk(wproj, "wproj", torch.uint8), _chk(b2, "b2"), T.data_ptr(), out.data_ptr(), 4, _stream()), "mftx_ou_heads")
    return out


def flow_head(hsplit: torch.Tensor, h: int, w: int, wtile: torch.Tensor, b1, wproj: torch.Tensor, b2, coords=None):
    """delta = conv2(relu(conv1(h))) of the flow head without materialising the 256 hidden channels (``mftx_flow_head``):
    hsplit [P*h*w, >= 128] split-form rows -> delta [P*h*w, 2]; coords (optional, [P*h*w, 2]) += delta in place."""
    lib = _lib.load()
    M = hsplit.shape[0]
    P = M // (h * w)
    T = torch.empty(M, 18, dtype=torch.float32, device=hsplit.device)
    delta = torch.empty(M, 2, dtype=torch.float32, device=hsplit.device)
    check(lib.mftx_flow_head(_chk(hsplit, "hsplit"), hsplit.stride(0), P, h, w, _chk(wtile, "wtile", torch.uint8), _chk(b1, "b1"),
                             _chk(wproj, "wproj", torch.uint8), _chk(b2, "b2"), T.data_ptr(), delta.data_ptr(),
                             _chk(coords, "coords") if coords is not None else None, _stream()), "mftx_flow_head")
    return delta


def pack_flow_branch_weights(w98: torch.Tensor, w2pk: torch.Tensor, check_range: bool = True) -> torch.Tensor:
    """convf1's weight as [98 = (ky, kx, c), 128] and convf2's in the ``pack_conv_weight`` form [>= 64, 9, 128] -> the
    fragment streams of the fused flow-branch kernel (``mftx_pack_flow_branch_weights``; opaque bytes).  The weights are
    operands of the split arithmetic: with ``check_range`` a value not below 65504 raises ``SplitRangeError``."""
    lib = _lib.load()
    if tuple(w98.shape) != (98, 128) or w2pk.dim() != 3 or w2pk.shape[0] < 64 or tuple(w2pk.shape[1:]) != (9, 128):
        raise MftxError("pack_flow_branch_weights: expected convf1 as [98, 128] and convf2 as [>= 64, 9, 128]")
    if check_range:
        bad = count_not_below(w98, _lib.SPLIT_LIMIT) + count_not_below(w2pk, _lib.SPLIT_LIMIT)
        if bad:
            raise SplitRangeError(f"pack_flow_branch_weights: {bad} weights are not below {_lib.SPLIT_LIMIT} in magnitude")
    out = torch.empty(_lib.FLOW_BRANCH_WEIGHT_BYTES, dtype=torch.uint8, device=w98.device)
    check(lib.mftx_pack_flow_branch_weights(_chk(w98, "w98"), _chk(w2pk, "w2pk"), out.data_ptr(), _stream()),
          "mftx_pack_flow_branch_weights")
    return out


def flow_branch(coords: torch.Tensor, h: int, w: int, wflow: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                out: torch.Tensor = None, hx: torch.Tensor = None) -> torch.Tensor:
    """relu(convf2(relu(convf1(coords - grid)))) without materialising convf1's 128 channels (``mftx_flow_branch``;
    split-fp16 arithmetic): coords [P, h*w, 2], wflow from ``pack_flow_branch_weights`` -> [P*h*w, 64] in SPLIT form
    (``unsplit_activations`` decodes it).  hx (optional): [P*h*w, 384] split-form rows whose channels 382, 383 receive
    the flow itself."""
    lib = _lib.load()
    P = coords.shape[0]
    if out is None:
        out = torch.empty(P * h * w, 64, dtype=torch.float32, device=coords.device)
    check(lib.mftx_flow_branch(_chk(coords, "coords"), P, h, w, _chk(wflow, "wflow", torch.uint8), _chk(b1, "b1"),
                               _chk(b2, "b2"), out.data_ptr(), out.stride(0),
                               hx.data_ptr() if hx is not None else None, hx.stride(0) if hx is not None else 0, _stream()),
          "mftx_flow_branch")
    return out


def corr_lookup_convc1(lv, coords: torch.Tensor, h: int, w: int, wfused: torch.Tensor, bias: torch.Tensor,
                       out_split: bool = False):
    """relu(convc1(lookup(coords)) + bias) without materialising the lookup (``mftx_corr_lookup_convc1``; split-fp16
    arithmetic): lv as ``corr_lookup``, coords [P, h*w, 2], wfused from ``pack_lookup_convc1_weights`` -> [P*h*w, 256]
    (fp32, or the split form when out_split)."""
    lib = _lib.load()
    P = coords.shape[0]
    stride, _ = pyramid_layout(h, w)
    for l, t in enumerate(lv):
        if tuple(t.shape) != (P, h * w, stride[l]):
            raise MftxError(f"corr_lookup_convc1: level {l} must be [{P}, {h * w}, {stride[l]}]")
    out = torch.empty(P * h * w, 256, dtype=torch.float32, device=coords.device)
    check(lib.mftx_corr_lookup_convc1(*[_chk(t, "level") for t in lv], _chk(coords, "coords"), P, h, w,
                                      _chk(wfused, "wfused", torch.uint8), _chk(bias, "bias"), out.data_ptr(), 256,
                                      int(bool(out_split)), _stream()), "mftx_corr_lookup_convc1")
    return out


def fmap_pyramid(f2: torch.Tensor, h: int, w: int):
    """f2 pixel-major [P, h*w, C] -> [f2, pooled level 1, 2, 3] ([P, h_l*w_l, C]); the feature pyramid of the
    on-demand correlation (AlternateCorrBlock, core/corr.py:78-82)."""
    lib = _lib.load()
    P, N, Cc = f2.shape
    assert N == h * w
    lv = [torch.empty(P, (h >> l) * (w >> l), Cc, dtype=torch.float32, device=f2.device) for l in (1, 2, 3)]
    check(lib.mftx_fmap_pyramid(_chk(f2, "f2"), P, Cc, h, w, *[t.data_ptr() for t in lv], _stream()), "mftx_fmap_pyramid")
    return [f2] + lv


def corr_lookup_ondemand(f1: torch.Tensor, f2_levels, coords: torch.Tensor, h: int, w: int, r: int = 4):
    """f1 [P, h*w, 256], f2_levels from ``fmap_pyramid``, coords [P, h*w, 2] -> [P, h*w, 324] (as ``corr_lookup``)."""
    lib = _lib.load()
    P, N, Cc = f1.shape
    out = torch.empty(P, N, 324, dtype=torch.float32, device=f1.device)
    check(lib.mftx_corr_lookup_ondemand(_chk(f1, "f1"), *[_chk(t, "f2 level") for t in f2_levels], _chk(coords, "coords"),
                                        P, Cc, h, w, r, out.data_ptr(), 324, _stream()), "mftx_corr_lookup_ondemand")
    return out


def conv2d(x: torch.Tensor, wpk: torch.Tensor, bias, P, h, w, N, kh, kw, act=None, out_scale=1.0, x2=None,
           addend=None, stride=0, hin=0, win=0, pad_y=0, pad_x=0, residual_mode=0, arith=ARITH_F32, a_split=False,
           out_split=False, out=None, tile=None, lda0=None, c0=None):
    """x: pixel-major [P*h*w, C0] (optionally concatenated with x2 [P*h*w, C1]) ->
    [P*h*w, N].  arith = ARITH_SPLIT: wpk is the output of ``split_weights``.  tile: force the workgroup tile shape
    (``mftx_conv2d_tile``; tests and micro-benchmarks -- every shape gives the same bits).  lda0 / c0: row stride and
    channel count of x instead of ``x.shape[1]`` -- overlapping windows, as the encoders' stem reads its input: 28 floats
    (7 pixels x RGB0) every 4 floats (lda0 = 4, c0 = 28, kh = 7, kw = 1, pad_x = -1; csrc/encoder.hip)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(P * h * w, N, dtype=torch.float32, device=x.device)
    d = ConvDesc()
    d.a0, d.lda0, d.c0 = _chk(x, "x"), x.shape[1] if lda0 is None else int(lda0), x.shape[1] if c0 is None else int(c0)
    if x2 is not None:
        d.a1, d.lda1, d.c1 = _chk(x2, "x2"), x2.shape[1], x2.shape[1]
    else:
        d.a1, d.lda1, d.c1 = None, 0, 0
    d.wpk = _chk(wpk, "wpk")
    d.bias = _chk(bias, "bias") if bias is not None else None
    d.out, d.ldo = _chk(out, "out"), out.shape[1]
    d.P, d.h, d.w, d.N, d.kh, d.kw = P, h, w, N, kh, kw
    d.act, d.out_scale = ACT[act], out_scale
    d.addend, d.ld_addend = (_chk(addend, "addend"), addend.shape[1]) if addend is not None else (None, 0)
    d.stride, d.hin, d.win, d.pad_y, d.pad_x, d.residual_mode = stride, hin, win, pad_y, pad_x, residual_mode
    d.arith = arith
    d.a_split, d.out_split = int(bool(a_split)), int(bool(out_split))      # operands in split form (see split_activations)
    if tile is None:
        check(lib.mftx_conv2d(C.byref(d), _stream()), "mftx_conv2d")
    else:
        check(lib.mftx_conv2d_tile(C.byref(d), int(tile), _stream()), "mftx_conv2d_tile")
    return out


def convex_upsample(flow_lr, ou, mask, P, h, w, pads=(0, 0, 0, 0), want_packed=False):
    """flow_lr [M,2], ou [M,ld>=3], mask [M,576] -> flow [P,2,H0,W0], occl, sigma [P,1,H0,W0]
    (+ packed [P,H0,W0,4] = (fx, fy, occl, sigma) per pixel)."""
    lib = _lib.load()
    pl, pr, pt, pb = pads
    H0, W0 = 8 * h - pt - pb, 8 * w - pl - pr
    dev = flow_lr.device
    flow = torch.empty(P, 2, H0, W0, dtype=torch.float32, device=dev)
    occl = torch.empty(P, 1, H0, W0, dtype=torch.float32, device=dev)
    sigma = torch.empty(P, 1, H0, W0, dtype=torch.float32, device=dev)
    packed = torch.empty(P, H0, W0, 4, dtype=torch.float32, device=dev) if want_packed else None
    check(lib.mftx_convex_upsample(_chk(flow_lr, "flow_lr"), _chk(ou, "ou"), ou.shape[1], _chk(mask, "mask"),
                                   P, h, w, pl, pr, pt, pb, flow.data_ptr(), occl.data_ptr(), sigma.data_ptr(),
                                   packed.data_ptr() if want_packed else None, _stream()), "mftx_convex_upsample")
    return (flow, occl, sigma, packed) if want_packed else (flow, occl, sigma)


def _planes(res, H, W):
    flow, occl, sigma = res
    if flow.shape != (2, H, W) or occl.shape != (1, H, W) or sigma.shape != (1, H, W):
        raise MftxError("FlowOU planes must be [2,H,W], [1,H,W], [1,H,W]")
    return _chk(flow, "flow"), _chk(occl, "occlusion"), _chk(sigma, "sigma")


def _new_result(H, W, device):
    return (torch.empty(2, H, W, dtype=torch.float32, device=device),
            torch.empty(1, H, W, dtype=torch.float32, device=device),
            torch.empty(1, H, W, dtype=torch.float32, device=device))


def chain(L, R):
    """chain_results: L, R = (flow[2,H,W], occl[1,H,W], sigma[1,H,W]) -> same triple."""
    lib = _lib.load()
    _, H, W = L[0].shape
    out = _new_result(H, W, L[0].device)
    check(lib.mftx_chain(*_planes(L, H, W), *_planes(R, H, W), H, W, *[t.data_ptr() for t in out], _stream()),
          "mftx_chain")
    return out


def warp_backward(flow, img):
    """flow [2,H,W], img [C,H,W] -> img sampled at grid + flow, [C,H,W]."""
    lib = _lib.load()
    Cc, H, W = img.shape
    if flow.shape != (2, H, W):
        raise MftxError("warp_backward: flow must be [2,H,W] matching img")
    out = torch.empty_like(img)
    check(lib.mftx_warp_backward(_chk(flow, "flow"), _chk(img, "img"), Cc, H, W, out.data_ptr(), _stream()),
          "mftx_warp_backward")
    return out


def select(cands, thr, want_chosen=False):
    """cands: list of chained triples ordered [inf, 1, 2, ...]."""
    lib = _lib.load()
    K = len(cands)
    _, H, W = cands[0][0].shape
    cols = list(zip(*[_planes(c, H, W) for c in cands]))
    arrs = [_lib.ptr_array(list(c)) for c in cols]
    out = _new_result(H, W, cands[0][0].device)
    chosen = torch.empty(H, W, dtype=torch.int8, device=out[0].device) if want_chosen else None
    check(lib.mftx_select(K, arrs[0][0], arrs[1][0], arrs[2][0], float(thr), H, W, *[t.data_ptr() for t in out],
                          chosen.data_ptr() if want_chosen else None, _stream()), "mftx_select")
    return out + (chosen,)


def chain_select(Ls, Rs, thr, want_chosen=False):
    """Fused chain + select over K (L, R) pairs ordered [inf, 1, 2, ...]."""
    lib = _lib.load()
    K = len(Ls)
    assert len(Rs) == K
    _, H, W = Ls[0][0].shape
    lcols = list(zip(*[_planes(c, H, W) for c in Ls]))
    rcols = list(zip(*[_planes(c, H, W) for c in Rs]))
    arrs = [_lib.ptr_array(list(c)) for c in lcols + rcols]
    out = _new_result(H, W, Ls[0][0].device)
    chosen = torch.empty(H, W, dtype=torch.int8, device=out[0].device) if want_chosen else None
    check(lib.mftx_chain_select(K, *[a[0] for a in arrs], float(thr), H, W, *[t.data_ptr() for t in out],
                                chosen.data_ptr() if want_chosen else None, _stream()), "mftx_chain_select")
    return out + (chosen,)


def chain_select_packed(Ls, Rs, thr, want_chosen=False):
    """Fused chain + select with the right operands in the packed per-pixel format: Ls = K x (flow[2,H,W],
    occl[1,H,W], sigma[1,H,W]), Rs = K x [H,W,4] (fx, fy, occl, sigma)."""
    lib = _lib.load()
    K = len(Ls)
    assert len(Rs) == K
    _, H, W = Ls[0][0].shape
    lcols = list(zip(*[_planes(c, H, W) for c in Ls]))
    for r in Rs:
        if tuple(r.shape) != (H, W, 4):
            raise MftxError("packed FlowOU must be [H, W, 4]")
    arrs = [_lib.ptr_array(list(c)) for c in lcols] + [_lib.ptr_array([_chk(r, "packed") for r in Rs])]
    out = _new_result(H, W, Ls[0][0].device)
    chosen = torch.empty(H, W, dtype=torch.int8, device=out[0].device) if want_chosen else None
    check(lib.mftx_chain_select_packed(K, *[a[0] for a in arrs], float(thr), H, W, *[t.data_ptr() for t in out],
                                       chosen.data_ptr() if want_chosen else None, _stream()), "mftx_chain_select_packed")
    return out + (chosen,)


def chain_select_multi(templates, thr, want_chosen=False):
    """``chain_select_packed`` for many templates in one launch (``mftx_chain_select_multi``): templates = T x (Ls, Rs) with
    Ls = K_j x (flow[2,H,W], occl[1,H,W], sigma[1,H,W]) and Rs = K_j x [H,W,4]; the same right operand may appear under
    several templates.  -> T x (flow, occl, sigma, chosen | None), each bitwise what ``chain_select_packed(Ls, Rs, thr)`` gives."""
    lib = _lib.load()
    templates = list(templates)
    if not templates:
        return []
    _, H, W = templates[0][0][0][0].shape
    Ks, cols, rs = [], [], []
    for Ls, Rs in templates:
        if len(Ls) != len(Rs) or not 1 <= len(Ls) <= _lib.MAX_CANDIDATES:
            raise MftxError(f"chain_select_multi: every template needs 1..{_lib.MAX_CANDIDATES} (left, right) pairs")
        Ks.append(len(Ls))
        cols += [_planes(c, H, W) for c in Ls]
        for r in Rs:
            if tuple(r.shape) != (H, W, 4):
                raise MftxError("packed FlowOU must be [H, W, 4]")
            rs.append(_chk(r, "packed"))
    T = len(templates)
    dev = templates[0][0][0][0].device
    # one allocation per plane kind for all templates (the outputs are views of it)
    flow = torch.empty(T, 2, H, W, dtype=torch.float32, device=dev)
    occl = torch.empty(T, 1, H, W, dtype=torch.float32, device=dev)
    sigma = torch.empty(T, 1, H, W, dtype=torch.float32, device=dev)
    chosen = torch.empty(T, H, W, dtype=torch.int8, device=dev) if want_chosen else None
    larrs = [_lib.ptr_array(list(c)) for c in zip(*cols)] + [_lib.ptr_array(rs)]
    oarrs = [_lib.ptr_array([t[j].data_ptr() for j in range(T)]) for t in (flow, occl, sigma)]
    carr = _lib.ptr_array([chosen[j].data_ptr() for j in range(T)]) if want_chosen else (None, None)
    check(lib.mftx_chain_select_multi(T, (C.c_int * T)(*Ks), *[a[0] for a in larrs], float(thr), H, W,
                                      *[a[0] for a in oarrs], carr[0], _stream()), "mftx_chain_select_multi")
    return [(flow[j], occl[j], sigma[j], chosen[j] if want_chosen else None) for j in range(T)]


def sample_points(results, tmpl, xy, table, column):
    """Point read-out of many results in one launch (``mftx_sample_points``): results = T x (flow[2,H,W], occl[1,H,W],
    sigma[1,H,W]); tmpl [N] int32 and xy [N,2] float32 on the device -- point i lies at xy[i] on results[tmpl[i]]; table: a
    float32 device tensor [N, frames, 4] (or [N, 4]) the caller owns.  Row i, column ``column`` of it receives
    (x + flow x, y + flow y, occlusion, sigma) -- ``warp_forward_points`` and ``sample`` of the reference's results API;
    nothing else of the table is touched.  Returns ``table``."""
    lib = _lib.load()
    results = list(results)
    N = int(tmpl.shape[0])
    if not results or N == 0:
        return table
    _, H, W = results[0][0].shape
    cols = list(zip(*[_planes(r, H, W) for r in results]))
    arrs = [_lib.ptr_array(list(c)) for c in cols]
    if tuple(xy.shape) != (N, 2) or tmpl.dim() != 1:
        raise MftxError("sample_points: tmpl must be [N], xy [N, 2]")
    if table.dim() == 2:
        frames = 1
    elif table.dim() == 3:
        frames = int(table.shape[1])
    else:
        raise MftxError("sample_points: the table must be [N, frames, 4] or [N, 4]")
    if int(table.shape[0]) != N or int(table.shape[-1]) != 4 or not 0 <= int(column) < frames:
        raise MftxError("sample_points: the table must be [N, frames, 4] with 0 <= column < frames")
    check(lib.mftx_sample_points(len(results), arrs[0][0], arrs[1][0], arrs[2][0], H, W, N, _chk(tmpl, "tmpl", torch.int32),
                                 _chk(xy, "xy"), _chk(table, "table"), 4 * frames, int(column), _stream()),
          "mftx_sample_points")
    return table


# ---------------------------------------------------------------------------
# forward splat + demo overlays (csrc/splat.hip): 64-bit integer fixed point, bitwise reproducible
# ---------------------------------------------------------------------------

class SplatPlan(NamedTuple):
    S: int            # weight bits: q_w = rint(w * 2^S)
    V: int            # value bits: v_q = rint(v * 2^V); 0 for integer values
    L: int            # ceil(log2(4 H W)): no destination receives more than 2^L contributions
    native: bool      # False: too few bits left for the integer path (S < 16, or V < 12 for float values)


def splat_plan(H: int, W: int, k: int, floating: bool) -> SplatPlan:
    """Fixed-point formats of a forward splat of values |v| < 2^k on an H x W frame (pure host arithmetic).

    Weights are at most 1 and at most 4 H W <= 2^L contributions reach one destination, so every accumulator word stays
    within 2^(L + k + V + S) <= 2^62: overflow is excluded by construction, not by testing.  Integer values keep V = 0 and
    take S = min(24, 62 - L - k); float values take S = 24 (every bit of an fp32 weight product that matters) and
    V = min(23, 62 - L - k - 24).  ``native`` is False where that leaves S < 16, or V < 12 for float values: the native
    path then refuses and the caller uses ``FlowOUTrackingResult.warp_forward``."""
    H, W, k = int(H), int(W), int(k)
    if H < 1 or W < 1 or k < 0:
        raise ValueError("splat_plan: need H, W >= 1 and k >= 0")
    L = (4 * H * W - 1).bit_length()
    if floating:
        S, V = 24, min(23, 62 - L - k - 24)
        return SplatPlan(S, V, L, V >= 12)
    S = min(24, 62 - L - k)
    return SplatPlan(S, 0, L, S >= 16)


def value_bits(bound: float) -> int:
    """The smallest k >= 0 with bound < 2^k."""
    bound = float(bound)
    if not math.isfinite(bound) or bound < 0:
        raise MftxError("splat: the value bound must be finite and non-negative")
    return max(0, math.frexp(bound)[1])           # bound = m 2^e with 0.5 <= m < 1


def splat_accumulator(C: int, H: int, W: int, device) -> torch.Tensor:
    """A zeroed accumulator [C + 1, H, W] int64 (plane C: the weight sums)."""
    return torch.zeros(C + 1, H, W, dtype=torch.int64, device=device)


def splat_forward(flow, img, value_bound, mask=None, border=None, acc=None):
    """Forward splat of ``img`` [H, W, C] (float32 or uint8, device) along ``flow`` [2, H, W] -> float32 [H, W, C]
    (``mftx_splat_forward`` + ``mftx_splat_resolve``): what ``FlowOUTrackingResult.warp_forward`` computes, with the sums in
    64-bit integers.  ``value_bound``: max |img| (float32 values beyond it can overflow the accumulator; uint8 needs none);
    mask: [H, W] bool / uint8 of kept template pixels; pixels nothing reached are 0 or ``border``.  ``acc``: a zeroed
    ``splat_accumulator(C, H, W)`` to reuse -- the resolve clears it behind itself.  No host synchronisation."""
    lib = _lib.load()
    if img.dim() != 3:
        raise MftxError("splat_forward: img must be [H, W, C]")
    H, W, Cc = (int(s) for s in img.shape)
    if tuple(flow.shape) != (2, H, W):
        raise MftxError("splat_forward: flow must be [2,H,W] matching img")
    if img.dtype == torch.uint8:
        dtype, plan = 1, splat_plan(H, W, 8, False)
    else:
        dtype, plan = 0, splat_plan(H, W, value_bits(value_bound), True)
    if not plan.native:
        raise MftxError(f"splat_forward: {H} x {W} with this value range leaves S = {plan.S}, V = {plan.V} bits "
                        "for the integer accumulator (needs S >= 16 and V >= 12 for float values): use warp_forward")
    mp = None
    if mask is not None:
        if tuple(mask.shape) != (H, W) or mask.dtype not in (torch.bool, torch.uint8):
            raise MftxError("splat_forward: mask must be [H,W] bool or uint8")
        mp = _chk(mask, "mask", mask.dtype)
    if acc is None:
        acc = splat_accumulator(Cc, H, W, img.device)
    elif tuple(acc.shape) != (Cc + 1, H, W):
        raise MftxError("splat_forward: acc must be [C+1,H,W]")
    out = torch.empty(H, W, Cc, dtype=torch.float32, device=img.device)
    check(lib.mftx_splat_forward(_chk(flow, "flow"), _chk(img, "img", img.dtype), dtype, mp, Cc, H, W, plan.S, plan.V,
                                 _chk(acc, "acc", torch.int64), _stream()), "mftx_splat_forward")
    check(lib.mftx_splat_resolve(acc.data_ptr(), Cc, H, W, plan.V, 0.0 if border is None else float(border), 1,
                                 out.data_ptr(), _stream()), "mftx_splat_resolve")
    return out


def edit_alpha_divisor(edit) -> float:
    """``vis.blend_with_alpha_premult`` rescales the warped alpha only if its maximum exceeds 1.0001: the divisor is 255
    unless every non-zero alpha of the edit equals 1.  Decided once, on the host, from the edit (numpy [H, W, 4] uint8)."""
    return 255.0 if int(edit[..., 3].max(initial=0)) > 1 else 1.0


def overlay_edit(flow, occl, edit, frame, acc, alpha_div=255.0, out=None):
    """The BGRA edit [H, W, 4] uint8 splatted along the flow for visible template pixels and blended onto the gray frame
    [H, W, 3] uint8 -> [H, W, 3] uint8 (``mftx_overlay_edit``: ``vis.draw_edit``).  ``acc``: a zeroed
    ``splat_accumulator(4, H, W)``, zero again afterwards."""
    lib = _lib.load()
    H, W = int(frame.shape[0]), int(frame.shape[1])
    if tuple(frame.shape) != (H, W, 3) or tuple(edit.shape) != (H, W, 4):
        raise MftxError("overlay_edit: frame must be [H,W,3] and edit [H,W,4]")
    if tuple(flow.shape) != (2, H, W) or occl.numel() != H * W or tuple(acc.shape) != (5, H, W):
        raise MftxError("overlay_edit: flow must be [2,H,W], occlusion [1,H,W], acc [5,H,W]")
    plan = splat_plan(H, W, 16, False)
    if not plan.native:
        raise MftxError(f"overlay_edit: {H} x {W} leaves S = {plan.S} weight bits (needs 16): use vis.draw_edit")
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=frame.device)
    elif tuple(out.shape) != (H, W, 3):
        raise MftxError("overlay_edit: out must be [H,W,3]")
    check(lib.mftx_overlay_edit(_chk(flow, "flow"), _chk(occl, "occlusion"), _chk(edit, "edit", torch.uint8),
                                _chk(frame, "frame", torch.uint8), H, W, plan.S, float(alpha_div),
                                _chk(acc, "acc", torch.int64), _chk(out, "out", torch.uint8), _stream()), "mftx_overlay_edit")
    return out


def overlay_dots(frame, table, radius=3, color=(0, 0, 255), out=None):
    """A dot of ``color`` (BGR) at every visible point of ``table`` [N, 4] float32 = (x, y, occlusion, sigma), as
    ``sample_points`` writes it, on a copy of ``frame`` [H, W, 3] uint8 (``mftx_overlay_dots``: ``vis.draw_dots``).
    ``out=frame`` draws in place."""
    lib = _lib.load()
    H, W = int(frame.shape[0]), int(frame.shape[1])
    if tuple(frame.shape) != (H, W, 3):
        raise MftxError("overlay_dots: frame must be [H,W,3]")
    if table.dim() != 2 or int(table.shape[1]) != 4:
        raise MftxError("overlay_dots: the table must be [N, 4]")
    if out is None:
        out = torch.empty_like(frame)
    elif tuple(out.shape) != (H, W, 3):
        raise MftxError("overlay_dots: out must be [H,W,3]")
    N = int(table.shape[0])
    check(lib.mftx_overlay_dots(_chk(frame, "frame", torch.uint8), _chk(out, "out", torch.uint8), H, W,
                                _chk(table, "table") if N else None, 4, N, float(radius), int(color[0]), int(color[1]),
                                int(color[2]), _stream()), "mftx_overlay_dots")
    return out


_quant_ws = {}


def quantize_u16(x):
    """One channel of a cache entry -> (uint16 tensor of x's shape, lohi float32[2] = (min, max)),
    both on the device (``compress_channel`` of MFT/utils/io.py:495-506).  No host sync."""
    lib = _lib.load()
    if isinstance(x, torch.Tensor) and x.is_cuda:
        x = x.contiguous()
        if x.data_ptr() % 16:        # a plane sliced out of a batched result: the kernels load 16 bytes per lane
            x = x.clone()
    _chk(x, "x")
    if x.numel() == 0:
        raise MftxError("quantize_u16: empty channel")
    ws = _quant_ws.get(x.device)
    if ws is None:
        ws = _quant_ws[x.device] = torch.empty(lib.mftx_quantize_workspace_bytes(), dtype=torch.uint8, device=x.device)
    q = torch.empty(x.shape, dtype=torch.uint16, device=x.device)
    lohi = torch.empty(2, dtype=torch.float32, device=x.device)
    check(lib.mftx_quantize_u16(x.data_ptr(), x.numel(), q.data_ptr(), lohi.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream()), "mftx_quantize_u16")
    return q, lohi


def dequantize_u16(q, lo, hi):
    """uint16 device tensor + the channel's (min, max) -> float32 (``decompress_channel``,
    MFT/utils/io.py:548-551)."""
    lib = _lib.load()
    if isinstance(q, torch.Tensor) and q.is_cuda:
        q = q.contiguous()
        if q.data_ptr() % 16:
            q = q.clone()
    _chk(q, "q", torch.uint16)
    x = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    check(lib.mftx_dequantize_u16(q.data_ptr(), q.numel(), float(lo), float(hi), x.data_ptr(), _stream()),
          "mftx_dequantize_u16")
    return x


# ---------------------------------------------------------------------------
# dense track store (csrc/trackstore.hip): frames kept as 8 bytes per pixel, point read-out from the quantised data
# ---------------------------------------------------------------------------

_trackstore_ws = {}


def _trackstore_frame(packed, lohi, H, W):
    if tuple(packed.shape) != (H, W, 4) or tuple(lohi.shape) != (4, 2):
        raise MftxError("trackstore: packed must be [H,W,4] uint16 and lohi [4,2] float32")
    return _chk(packed, "packed", torch.uint16), _chk(lohi, "lohi")


def trackstore_append(planes, packed, lohi):
    """One result (flow[2,H,W], occl[1,H,W], sigma[1,H,W]) -> ``packed`` [H,W,4] uint16 = (fx, fy, occl, sigma) per pixel and
    ``lohi`` [4,2] float32 = each channel's (min, max), both the caller's device tensors (``mftx_trackstore_append``).  Per
    channel bitwise ``quantize_u16`` of that plane; the planes may be views into a larger buffer.  No host sync."""
    lib = _lib.load()
    _, H, W = planes[0].shape
    H, W = int(H), int(W)
    fp, op, sp = _planes(planes, H, W)
    pp, lp = _trackstore_frame(packed, lohi, H, W)
    dev = packed.device
    ws = _trackstore_ws.get(dev)
    if ws is None:
        ws = _trackstore_ws[dev] = torch.empty(lib.mftx_trackstore_workspace_bytes(), dtype=torch.uint8, device=dev)
    check(lib.mftx_trackstore_append(fp, op, sp, H, W, pp, lp, ws.data_ptr(), ws.numel(), _stream()), "mftx_trackstore_append")
    return packed, lohi


TRACKSTORE_APPEND_MULTI_FRAMES = 64      # frames per argument block of mftx_trackstore_append_multi (csrc/trackstore.hip: TSM_F)
_trackstore_multi_ws = {}


def trackstore_append_multi(frames):
    """``trackstore_append`` for T results in one call (``mftx_trackstore_append_multi``): frames = T x (planes, packed, lohi) as
    for ``trackstore_append``, all of one H x W and on one device.  Two launches per 64 frames; frame j's ``packed`` and ``lohi``
    are bitwise what ``trackstore_append`` gives for it alone.  The workspace is kept per device and grows with T (it is used
    on the current stream only, like ``trackstore_append``'s).  No host sync."""
    lib = _lib.load()
    frames = list(frames)
    T = len(frames)
    if T == 0:
        return
    _, H, W = frames[0][0][0].shape
    H, W = int(H), int(W)
    cols = [_planes(planes, H, W) for planes, _, _ in frames]
    outs = [_trackstore_frame(packed, lohi, H, W) for _, packed, lohi in frames]
    dev = frames[0][1].device
    need = lib.mftx_trackstore_append_multi_workspace_bytes(T)
    ws = _trackstore_multi_ws.get(dev)
    if ws is None or ws.numel() < need:
        ws = _trackstore_multi_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    arrs = [_lib.ptr_array(list(c)) for c in zip(*cols)] + [_lib.ptr_array(list(c)) for c in zip(*outs)]
    check(lib.mftx_trackstore_append_multi(T, arrs[0][0], arrs[1][0], arrs[2][0], H, W, arrs[3][0], arrs[4][0], ws.data_ptr(),
                                           ws.numel(), _stream()), "mftx_trackstore_append_multi")


def trackstore_unpack(packed, lohi, out=None):
    """One stored frame -> (flow[2,H,W], occl[1,H,W], sigma[1,H,W]) on the device (``mftx_trackstore_unpack``): per channel
    bitwise ``dequantize_u16`` with the (min, max) of ``lohi``, which stay on the device.  ``out``: planes to write into."""
    lib = _lib.load()
    H, W = int(packed.shape[0]), int(packed.shape[1])
    pp, lp = _trackstore_frame(packed, lohi, H, W)
    if out is None:
        out = _new_result(H, W, packed.device)
    fp, op, sp = _planes(out, H, W)
    check(lib.mftx_trackstore_unpack(pp, lp, H, W, fp, op, sp, _stream()), "mftx_trackstore_unpack")
    return out


def _trackstore_chunks(chunks, lohi_chunks, name):
    """The chunk list every read-out takes -- uint16 device tensors [frames_per_chunk, H, W, 4] with float32 [frames_per_chunk, 4, 2]
    beside them -- validated -> (frames_per_chunk, H, W, chunk addresses, lohi addresses)."""
    chunks, lohi_chunks = list(chunks), list(lohi_chunks)
    if not chunks or len(chunks) != len(lohi_chunks):
        raise MftxError(f"{name}: as many lohi tables as chunks, at least one")
    fpc, H, W = (int(s) for s in chunks[0].shape[:3])
    for c, l in zip(chunks, lohi_chunks):
        if tuple(c.shape) != (fpc, H, W, 4) or tuple(l.shape) != (fpc, 4, 2):
            raise MftxError(f"{name}: chunks must be [frames_per_chunk,H,W,4] with lohi [frames_per_chunk,4,2]")
    return fpc, H, W, [_chk(c, "chunk", torch.uint16) for c in chunks], [_chk(l, "lohi chunk") for l in lohi_chunks]


def _slot_addresses(slots, chunk_ptrs, lohi_ptrs, frames_per_chunk, frame_bytes):
    """Slot s is frame s % frames_per_chunk of chunk s // frames_per_chunk: int64 slots, all of the store -> (packed addresses,
    lohi addresses)."""
    chunk, within = slots // frames_per_chunk, slots % frames_per_chunk
    return np.asarray(chunk_ptrs, dtype=np.int64)[chunk] + within * frame_bytes, np.asarray(lohi_ptrs, dtype=np.int64)[chunk] + within * 32


def trackstore_slot_addresses(chunks, lohi_chunks, slots):
    """The device addresses of stored frames: chunks / lohi_chunks as for ``trackstore_query``; slots: HOST integers, -1 for
    "no frame" -> (packed addresses, lohi addresses) as int64 arrays of the slots' shape, 0 where the slot is -1."""
    fpc, H, W, cptr, lptr = _trackstore_chunks(chunks, lohi_chunks, "trackstore_slot_addresses")
    slots = np.asarray(slots, dtype=np.int64)
    if slots.size and (slots.min() < -1 or slots.max() >= fpc * len(cptr)):
        raise MftxError("trackstore_slot_addresses: slots must be slots of the store, or -1")
    held = slots >= 0
    packed, lohi = _slot_addresses(np.where(held, slots, 0), cptr, lptr, fpc, H * W * 8)
    return np.where(held, packed, 0), np.where(held, lohi, 0)


def _pack_tables(int64_parts, int32_parts):
    """Host tables (1-D arrays) laid out for one upload -> (ONE int64 array: the int64 parts, then the int32 parts in its tail, so
    that pointer tables sit at multiples of 8 bytes and the others at multiples of 4; the byte offset of each part, in the order
    given)."""
    n64, n32 = sum(map(len, int64_parts)), sum(map(len, int32_parts))
    buf = np.zeros(n64 + (n32 + 1) // 2, np.int64)
    tail = buf[n64:].view(np.int32)
    offsets, at = [], 0
    for part in int64_parts:
        buf[at:at + len(part)] = part
        offsets.append(8 * at)
        at += len(part)
    at = 0
    for part in int32_parts:
        tail[at:at + len(part)] = part
        offsets.append(8 * n64 + 4 * at)
        at += len(part)
    return buf, tuple(offsets)


def _upload_tables(device, int64_parts, int32_parts):
    """``_pack_tables``, sent up through pinned memory without a host synchronisation -> (the device tensor, which the caller keeps
    alive until its call is enqueued; each part's device address)."""
    buf, offsets = _pack_tables(int64_parts, int32_parts)
    tables = torch.from_numpy(buf).pin_memory().to(device, non_blocking=True)
    return tables, tuple(tables.data_ptr() + o for o in offsets)


def trackstore_query(chunks, lohi_chunks, slots, xy, table, column0=0):
    """Point read-out of stored frames in one call (``mftx_trackstore_query``).  chunks: uint16 device tensors
    [frames_per_chunk, H, W, 4] with lohi_chunks float32 [frames_per_chunk, 4, 2] beside them (slot s = frame
    s % frames_per_chunk of chunk s // frames_per_chunk); slots [T] int32 and xy [N,2] float32 on the device; table: a float32
    device tensor [N, frames, 4] the caller owns.  Row i, column ``column0 + j`` receives (x + flow x, y + flow y, occlusion,
    sigma) of point i on the frame in slots[j] -- bitwise ``sample_points`` on that frame's ``trackstore_unpack``-ed planes;
    nothing else of the table is touched.  Returns ``table``."""
    lib = _lib.load()
    fpc, H, W, cptr, lptr = _trackstore_chunks(chunks, lohi_chunks, "trackstore_query")
    if xy.dim() != 2 or int(xy.shape[1]) != 2 or slots.dim() != 1:
        raise MftxError("trackstore_query: slots must be [T], xy [N, 2]")
    N, T = int(xy.shape[0]), int(slots.shape[0])
    if table.dim() != 3 or int(table.shape[0]) != N or int(table.shape[2]) != 4:
        raise MftxError("trackstore_query: the table must be [N, frames, 4]")
    carr, larr = _lib.ptr_array(cptr), _lib.ptr_array(lptr)
    if N == 0 or T == 0:          # (empty tensors have no storage to point at)
        return table
    check(lib.mftx_trackstore_query(carr[0], larr[0], len(cptr), fpc, _chk(slots, "slots", torch.int32), T, H, W, N,
                                    _chk(xy, "xy"), _chk(table, "table"), 4 * int(table.shape[1]), int(column0), _stream()),
          "mftx_trackstore_query")
    return table


def _locate_parts(point_slots, chunk_ptrs, lohi_ptrs, frames_per_chunk, frame_bytes):
    """-> (G, (frames, lohis), (group_start, order, group_of)): the tables of ``locate_tables`` before they are laid out."""
    slots = np.asarray(point_slots, dtype=np.int64).reshape(-1)
    N = int(slots.shape[0])
    order = np.argsort(slots, kind="stable")
    sorted_slots = slots[order]
    first = np.flatnonzero(np.concatenate([[True], sorted_slots[1:] != sorted_slots[:-1]]))
    G = int(first.shape[0])
    group_start = np.concatenate([first, [N]])
    group_of = np.empty(N, np.int32)
    group_of[order] = np.repeat(np.arange(G, dtype=np.int32), np.diff(group_start))
    return G, _slot_addresses(sorted_slots[first], chunk_ptrs, lohi_ptrs, frames_per_chunk, frame_bytes), (group_start, order, group_of)


def locate_tables(point_slots, chunk_ptrs, lohi_ptrs, frames_per_chunk, frame_bytes):
    """The tables of ``mftx_trackstore_locate`` for N queries whose frames sit in the slots ``point_slots`` (host integers, any
    order) as ONE int64 host array, and where its parts begin: -> (buf, G, (frames, lohis, group_start, order, group_of) byte
    offsets).  Queries are grouped by slot (stable, slots ascending): frames / lohis [G] addresses (``chunk_ptrs[c]`` +
    the frame's offset in its chunk), then int32 group_start [G + 1], order [N], group_of [N]."""
    G, int64_parts, int32_parts = _locate_parts(point_slots, chunk_ptrs, lohi_ptrs, frames_per_chunk, frame_bytes)
    buf, offsets = _pack_tables(int64_parts, int32_parts)
    return buf, G, offsets


def _locate_call(name, slots_what, H, W, chunk_ptrs, lohi_ptrs, frames_per_chunk, point_slots, xy, table, cell, occlusion_threshold):
    """``mftx_trackstore_locate`` over the frames ``_slot_addresses`` finds in the slots ``point_slots``."""
    lib = _lib.load()
    if xy.dim() != 2 or int(xy.shape[1]) != 2:
        raise MftxError(f"{name}: xy must be [N, 2]")
    N = int(xy.shape[0])
    slots = np.asarray(point_slots, dtype=np.int64).reshape(-1)
    if int(slots.shape[0]) != N or (N and (slots.min() < 0 or slots.max() >= frames_per_chunk * len(chunk_ptrs))):
        raise MftxError(f"{name}: {slots_what}")
    if tuple(table.shape) != (N, 4) or tuple(cell.shape) != (N,):
        raise MftxError(f"{name}: the table must be [N, 4], cell [N]")
    xp, tp, cp = _chk(xy, "xy"), _chk(table, "table"), _chk(cell, "cell", torch.int32)
    if N == 0:
        return table, cell
    G, int64_parts, int32_parts = _locate_parts(slots, chunk_ptrs, lohi_ptrs, frames_per_chunk, H * W * 8)
    tables, (frames, lohis, group_start, order, group_of) = _upload_tables(xy.device, int64_parts, int32_parts)
    keys = torch.empty(N, dtype=torch.int64, device=xy.device)
    check(lib.mftx_trackstore_locate(frames, lohis, group_start, G, order, group_of, H, W, N, xp, float(occlusion_threshold),
                                     keys.data_ptr(), tp, cp, _stream()), "mftx_trackstore_locate")
    return table, cell


def trackstore_locate(chunks, lohi_chunks, point_slots, xy, table, cell, occlusion_threshold=0.5):
    """The stored map inverted at points given on stored frames, in one call (``mftx_trackstore_locate``).  chunks /
    lohi_chunks as for ``trackstore_query``; point_slots: N HOST integers, the slot of the frame each point is given on (any
    order, repeats welcome); xy [N,2] float32 on the device.  Row n of ``table`` (float32 device [N,4]) receives the template
    point (x, y) whose image on that frame is xy[n], and occlusion and sigma there; ``cell`` (int32 device [N]) the template
    cell it lies in, -1 (and a row of NaN) where nothing maps to xy[n].  The group tables go up through one pinned buffer;
    no host synchronisation.  Returns (table, cell)."""
    fpc, H, W, cptr, lptr = _trackstore_chunks(chunks, lohi_chunks, "trackstore_locate")
    return _locate_call("trackstore_locate", "point_slots must be N slots of the store", H, W, cptr, lptr, fpc, point_slots, xy,
                        table, cell, occlusion_threshold)


def trackstore_invert(chunks, lohi_chunks, slots, table, cell, occlusion_threshold=0.5):
    """Stored frames inverted densely, in one call (``mftx_trackstore_invert``): ``trackstore_locate`` with every pixel centre
    (x, y) of the frame as a query, bit for bit, computed as a scatter from the template's cells.  chunks / lohi_chunks as for
    ``trackstore_query``; slots: G HOST integers, the slots of the frames to invert (repeats welcome).  ``table`` (float32 device
    [G,H,W,4]) receives per pixel the template point (x, y) whose image it is, and occlusion and sigma there; ``cell`` (int32
    device [G,H,W]) the template cell, -1 (and a row of NaN) where nothing maps to the pixel.  The two pointer tables go up
    through one pinned buffer; no host synchronisation.  Returns (table, cell)."""
    lib = _lib.load()
    fpc, H, W, cptr, lptr = _trackstore_chunks(chunks, lohi_chunks, "trackstore_invert")
    slots = np.asarray(slots, dtype=np.int64).reshape(-1)
    G = int(slots.shape[0])
    if G and (slots.min() < 0 or slots.max() >= fpc * len(cptr)):
        raise MftxError("trackstore_invert: slots must be slots of the store")
    if tuple(table.shape) != (G, H, W, 4) or tuple(cell.shape) != (G, H, W):
        raise MftxError("trackstore_invert: the table must be [G, H, W, 4], cell [G, H, W]")
    tp, cp = _chk(table, "table"), _chk(cell, "cell", torch.int32)
    if G == 0:
        return table, cell
    tables, (frames, lohis) = _upload_tables(table.device, _slot_addresses(slots, cptr, lptr, fpc, H * W * 8), ())
    keys = torch.empty(G * H * W, dtype=torch.int64, device=table.device)
    check(lib.mftx_trackstore_invert(frames, lohis, G, H, W, float(occlusion_threshold), keys.data_ptr(), tp, cp, _stream()),
          "mftx_trackstore_invert")
    return table, cell


def _trackstore_frame_ptrs(frames, name):
    """frames: J x (packed [H,W,4] uint16, lohi [4,2] float32) device views, of any stores -> (H, W, packed addresses, lohi
    addresses) as int64 arrays."""
    frames = list(frames)
    if not frames:
        raise MftxError(f"{name}: at least one stored frame")
    H, W = int(frames[0][0].shape[0]), int(frames[0][0].shape[1])
    ptrs = [_trackstore_frame(p, l, H, W) for p, l in frames]
    return H, W, np.asarray([p for p, _ in ptrs], dtype=np.int64), np.asarray([l for _, l in ptrs], dtype=np.int64)


def trackstore_locate_frames(frames, point_frame, xy, table, cell, occlusion_threshold=0.5):
    """``trackstore_locate`` over stored frames of ANY stores, in one call (``mftx_trackstore_locate``): frames = J x (packed
    [H,W,4], lohi [4,2]) device views; point_frame: N HOST integers, the index into ``frames`` of the frame each point is given
    on.  xy, table, cell as for ``trackstore_locate``.  One pinned buffer, no host synchronisation.  Returns (table, cell)."""
    H, W, pptr, lptr = _trackstore_frame_ptrs(frames, "trackstore_locate_frames")
    return _locate_call("trackstore_locate_frames", "point_frame must be N indices into frames", H, W, pptr, lptr, 1, point_frame,
                        xy, table, cell, occlusion_threshold)         # (every frame a chunk of its own)


TRACKSTORE_ATLAS_ENTRIES = 256           # entries per plane of mftx_trackstore_invert_atlas (8 bits of its key)
TRACKSTORE_ATLAS_CELLS = 1 << 24         # ... and cells per frame (24 bits)


def trackstore_invert_atlas(frames, first_of, rank_of, table, cell, entry, occlusion_threshold=0.5):
    """Stored frames of several stores inverted densely onto one plane per video frame, in one call
    (``mftx_trackstore_invert_atlas``): frames = J x (packed [H,W,4], lohi [4,2]) device views; first_of: G + 1 HOST integers --
    plane g is built from frames[first_of[g] : first_of[g + 1]], listed in ascending rank; rank_of: J HOST integers, what
    ``entry`` reports for each frame.  ``table`` (float32 device [G,H,W,4]), ``cell`` and ``entry`` (int32 device [G,H,W]) receive per
    pixel the winner's row, its template cell and its rank, -1 (and a row of NaN) where no entry finds the pixel.  H and W come
    from ``table`` (a call may have no frames at all).  The tables go up through one pinned buffer; no host synchronisation.
    Returns (table, cell, entry)."""
    lib = _lib.load()
    frames = list(frames)
    first_of = np.asarray(first_of, dtype=np.int64).reshape(-1)
    rank_of = np.asarray(rank_of, dtype=np.int64).reshape(-1)
    G, J = int(first_of.shape[0]) - 1, len(frames)
    if table.dim() != 4 or int(table.shape[3]) != 4 or int(table.shape[0]) != G or tuple(cell.shape) != tuple(table.shape[:3]) \
            or tuple(entry.shape) != tuple(table.shape[:3]):
        raise MftxError("trackstore_invert_atlas: the table must be [G, H, W, 4], cell and entry [G, H, W], first_of [G + 1]")
    H, W = int(table.shape[1]), int(table.shape[2])
    if G < 0 or int(rank_of.shape[0]) != J or first_of[0] != 0 or first_of[-1] != J or (np.diff(first_of) < 0).any():
        raise MftxError("trackstore_invert_atlas: first_of must ascend from 0 to the number of frames, rank_of name every frame")
    if G and np.diff(first_of).max() > TRACKSTORE_ATLAS_ENTRIES:
        raise MftxError(f"trackstore_invert_atlas: more than {TRACKSTORE_ATLAS_ENTRIES} entries in a plane")
    if (H - 1) * (W - 1) > TRACKSTORE_ATLAS_CELLS:
        raise MftxError("trackstore_invert_atlas: more than 2^24 cells")
    tp, cp, ep = _chk(table, "table"), _chk(cell, "cell", torch.int32), _chk(entry, "entry", torch.int32)
    if J:
        fH, fW, pptr, lptr = _trackstore_frame_ptrs(frames, "trackstore_invert_atlas")
        if (fH, fW) != (H, W):
            raise MftxError("trackstore_invert_atlas: the frames must be of the table's H x W")
    else:
        pptr = lptr = np.zeros(0, np.int64)
    if G == 0:
        return table, cell, entry
    tables, (fr, lh, fo, ro) = _upload_tables(table.device, (pptr, lptr), (first_of, rank_of))
    keys = torch.empty(G * H * W, dtype=torch.int64, device=table.device)
    check(lib.mftx_trackstore_invert_atlas(fr if J else None, lh if J else None, fo, ro if J else None, G, J, H, W,
                                           float(occlusion_threshold), keys.data_ptr(), tp, cp, ep, _stream()),
          "mftx_trackstore_invert_atlas")
    return table, cell, entry


TRACKSTORE_FLOW_COLUMNS = 16             # columns per workgroup of mftx_trackstore_flow_from unless the caller says otherwise


def trackstore_flow_from(table, entry, row_of, frame_ptrs, lohi_ptrs, flow, occl, sigma, columns_per_block=0):
    """One plane of ``trackstore_invert_atlas`` followed densely over T columns, in one call (``mftx_trackstore_flow_from``).
    table (float32 device [H,W,4]) and entry (int32 device [H,W]): the plane; row_of: n_ranks HOST integers, rank -> row (a row
    is a distinct template); frame_ptrs / lohi_ptrs: HOST int64 [R, T], the addresses (``trackstore_slot_addresses``) of the
    stored H x W frame column t is read from on row r's template and of its lohi table, both 0 where that template does not
    cover the column.  ``flow`` (float32 device [T,2,H,W]), ``occl`` and ``sigma`` ([T,1,H,W]) receive per pixel and column the
    winner's ``trackstore_query`` of its template point chained behind the inverse (flow = q - pixel, occlusion = maximum, sigma =
    root of the sum of squares), and NaN, 1, +inf where the pixel is not found or the column not covered.
    ``columns_per_block``: the columns a workgroup walks (0: TRACKSTORE_FLOW_COLUMNS).  The tables go up through one pinned
    buffer; no host synchronisation.  Returns (flow, occl, sigma)."""
    lib = _lib.load()
    row_of = np.asarray(row_of, dtype=np.int64).reshape(-1)
    frame_ptrs, lohi_ptrs = np.asarray(frame_ptrs, dtype=np.int64), np.asarray(lohi_ptrs, dtype=np.int64)
    if table.dim() != 3 or int(table.shape[2]) != 4 or tuple(entry.shape) != tuple(table.shape[:2]):
        raise MftxError("trackstore_flow_from: the table must be [H, W, 4], entry [H, W]")
    H, W = int(table.shape[0]), int(table.shape[1])
    if frame_ptrs.ndim != 2 or frame_ptrs.shape != lohi_ptrs.shape or frame_ptrs.shape[0] < 1 or ((frame_ptrs == 0) != (lohi_ptrs == 0)).any():
        raise MftxError("trackstore_flow_from: frame_ptrs and lohi_ptrs must be [R, T] with R >= 1, zero in the same places")
    R, T = (int(s) for s in frame_ptrs.shape)
    n_ranks = int(row_of.shape[0])
    if n_ranks < 1 or row_of.min() < 0 or row_of.max() >= R:
        raise MftxError("trackstore_flow_from: row_of must name a row for at least one rank")
    if tuple(flow.shape) != (T, 2, H, W) or tuple(occl.shape) != (T, 1, H, W) or tuple(sigma.shape) != (T, 1, H, W):
        raise MftxError("trackstore_flow_from: flow must be [T, 2, H, W], occl and sigma [T, 1, H, W]")
    tp, ep = _chk(table, "table"), _chk(entry, "entry", torch.int32)
    fp, op, sp = _chk(flow, "flow"), _chk(occl, "occl"), _chk(sigma, "sigma")
    if T == 0:
        return flow, occl, sigma
    tables, (frames, lohis, rows) = _upload_tables(table.device, (frame_ptrs.reshape(-1), lohi_ptrs.reshape(-1)), (row_of,))
    check(lib.mftx_trackstore_flow_from(tp, ep, rows, frames, lohis, n_ranks, R, T, H, W, int(columns_per_block), fp, op, sp,
                                        _stream()), "mftx_trackstore_flow_from")
    return flow, occl, sigma


class RaftEngine:
    """Handle on the native refinement runtime (``mftx_raft_*``)."""

    # WeightSlot indices (csrc/raft_engine.hip) of the weights that feed GEMM layers
    GEMM_SLOTS = (0, 2, 6, 8, 10, 11, 13, 14, 16, 17, 19, 20, 22, 26, 28, 30)

    OPTIONS = {"fork": 0, "presplit": 1, "group": 2, "fuse_lookup": 3, "graph": 4, "fuse_flow": 5, "tile_conv": 6, "fuse_head": 7, "tile_volume": 8, "fuse_gru": 9, "tile_cells": 10, "fuse_ou": 11, "tile_conv2p": 12}      # MFTX_RAFT_OPT_*
    # WeightSlot -> (N, cin) of the layers with a tile-resident kernel (csrc/tile_conv.hip): GRU gates (per-iteration and
    # context parts, both passes), flow head and mask head first layers
    # ... and (round 6) the motion encoder's convc2 (N = 192) and conv (126 of 128), 3 x 3 over 256 channels: two channel passes
    TILE_SLOTS = {2: (192, 256), 8: (128, 256), 10: (256, 256), 11: (256, 128), 13: (128, 256), 14: (128, 128), 16: (256, 256),
                  17: (256, 128), 19: (128, 256), 20: (128, 128), 22: (256, 128), 26: (256, 128)}

    def __init__(self, state_dict: dict, device, ondemand_corr=False, arith=ARITH_SPLIT, options=None):
        """options: {"fork" | "presplit" | "group" | "fuse_lookup" | "graph" | "fuse_flow" | "tile_conv" | "fuse_head" | "tile_volume": int} scheduling options of this handle
        (``mftx_raft_set_option``; defaults are the measured best)."""
        lib = _lib.load()
        self.device = torch.device(device)
        self.weights = pack_raft_weights(state_dict, self.device)   # keep alive: the engine holds raw pointers
        arr, self._keep = _lib.ptr_array([_chk(t, "weight") for t in self.weights])
        handle = C.c_void_p()
        check(lib.mftx_raft_create(arr, len(self.weights), C.byref(handle)), "mftx_raft_create")
        self._h = handle
        self._ws = None
        self.arith = int(arith)
        if self.arith == ARITH_SPLIT:          # split-fp16 products: the GEMM layers stream split weights
            self.split = [split_weights(t) if i in self.GEMM_SLOTS else None for i, t in enumerate(self.weights)]
            sarr, self._keep_split = _lib.ptr_array([t.data_ptr() if t is not None else None for t in self.split])
            check(lib.mftx_raft_set_split_weights(self._h, sarr, len(self.split)), "mftx_raft_set_split_weights")
            # lookup + convc1 as one kernel (the 324 features never leave the CU): convc1's weights as its fragment stream
            self.wfused = pack_lookup_convc1_weights(self.weights[0])
            check(lib.mftx_raft_set_lookup_fused(self._h, self.wfused.data_ptr()), "mftx_raft_set_lookup_fused")
            # the flow branch (convf1 -> convf2) as one kernel: both weights as its fragment streams
            self.wflow = pack_flow_branch_weights(self.weights[4], self.weights[6])
            check(lib.mftx_raft_set_flow_fused(self._h, self.wflow.data_ptr()), "mftx_raft_set_flow_fused")
            # the layers whose input tile fits a CU's LDS: weights as the streams of the tile-resident kernel
            self.wtile = [pack_tile_conv_weights(t, *self.TILE_SLOTS[i]) if i in self.TILE_SLOTS else None
                          for i, t in enumerate(self.weights)]
            tarr, self._keep_tile = _lib.ptr_array([t.data_ptr() if t is not None else None for t in self.wtile])
            check(lib.mftx_raft_set_tile_weights(self._h, tarr, len(self.wtile)), "mftx_raft_set_tile_weights")
            # ... and the flow head's last layer as the projection epilogue of its first (the 256 hidden channels stay in LDS)
            self.wproj = pack_flow_head_weights(self.weights[24])
            check(lib.mftx_raft_set_flow_head(self._h, self.wproj.data_ptr()), "mftx_raft_set_flow_head")
            # ... and the occlusion + uncertainty heads as one tile-resident kernel (five channel passes, projection epilogue)
            self.wou, self.wouproj = pack_ou_heads_weights(self.weights[30], self.weights[32])
            check(lib.mftx_raft_set_ou_heads(self._h, self.wou.data_ptr(), self.wouproj.data_ptr()), "mftx_raft_set_ou_heads")
        elif self.arith != ARITH_F32:
            raise MftxError(f"unknown arithmetic {arith!r}")
        # device-side count of non-finite output pixels, incremented by the last kernel of every refinement (no host sync;
        # read by nonfinite_count() when the caller synchronises anyway)
        # (16 bytes, the counter in word 0: the size mftx_copy_bytes moves, see nonfinite_snapshot)
        self._nonfinite = torch.zeros(4, dtype=torch.int32, device=self.device)
        check(lib.mftx_raft_set_nonfinite_counter(self._h, self._nonfinite.data_ptr()), "mftx_raft_set_nonfinite_counter")
        options = dict(options or {})
        self._gather = bool(options.pop("gather", 1))     # (Python-side: per-pair map lists instead of stacked batch tensors, A/B)
        for k, v in options.items():
            self.set_option(k, v)
        self.ondemand_corr = bool(ondemand_corr)
        if self.ondemand_corr:                 # raft_params.alternate_corr: no stored correlation volume
            check(lib.mftx_raft_set_ondemand(self._h, 1), "mftx_raft_set_ondemand")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().mftx_raft_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def debug_refine(self, fmap1, fmap2, net, inp, h, w, iters, pads=(0, 0, 0, 0), flow_init=None):
        """``refine`` with the debug payload of ``RAFT.forward(vis_debug=True)`` (core/raft.py:159-176, 255-257):
        -> (flow, occl, sigma), {'costvolume_pyramid': 4 x [P*h*w, 1, h_l, w_l], 'coords_left': [P, 2, h, w],
        'iterations': (iters + 1) x {'coords': [P, 2, h, w]}}, everything on the CPU like the reference's."""
        lib = _lib.load()
        P = fmap1.shape[0]
        M = P * h * w
        trace = torch.empty(iters + 1, M, 2, dtype=torch.float32, device=self.device)
        check(lib.mftx_raft_set_coords_trace(self._h, trace.data_ptr()), "mftx_raft_set_coords_trace")
        try:
            out = self.refine(fmap1, fmap2, net, inp, h, w, iters, pads=pads, flow_init=flow_init)
        finally:
            check(lib.mftx_raft_set_coords_trace(self._h, None), "mftx_raft_set_coords_trace")
        if self.ondemand_corr:
            pyramid = None                      # (alternate_corr keeps no volume, as in the reference)
        else:
            stride, _ = pyramid_layout(h, w)
            pyramid = []
            for l in range(4):
                lvl = self.region(f"lvl{l}", P, h, w, stride[l]).reshape(P, h * w, stride[l])
                pyramid.append(unblock_level(lvl, l, h, w).reshape(M, 1, h >> l, w >> l).cpu())
        to_map = lambda t: t.reshape(P, h, w, 2).permute(0, 3, 1, 2).contiguous().cpu()      # noqa: E731
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        debug = {"costvolume_pyramid": pyramid,
                 "coords_left": torch.stack([xs, ys])[None].repeat(P, 1, 1, 1),
                 "iterations": [{"coords": to_map(trace[i])} for i in range(iters + 1)]}
        return out, debug

    PLAN_FIELDS = ("presplit", "fuse_lookup", "tiles_on", "gru_fused", "ctx_supplied", "two_pass", "flow", "pair_second", "head_fused",
                   "defer_update", "ou_fused", "ou_materialised", "use_graph", "side_stream")      # mftx_raft_plan's order
    FLOW_SCHEDULES = ("fused", "side", "first", "after_lookup", "with_lookup")                    # MFTX_FLOW_*

    def plan(self, P, h, w, ctx_supplied=False):
        """The launch schedule ``refine`` would run for P pairs of h x w cells (``mftx_raft_plan``; launches nothing): a dict of
        PLAN_FIELDS -> bool, and "flow" -> one of FLOW_SCHEDULES."""
        out = (C.c_int * len(self.PLAN_FIELDS))()
        check(_lib.load().mftx_raft_plan(self._h, P, h, w, int(bool(ctx_supplied)), out, len(out)), "mftx_raft_plan")
        plan = {k: bool(v) for k, v in zip(self.PLAN_FIELDS, out)}
        plan["flow"] = self.FLOW_SCHEDULES[out[self.PLAN_FIELDS.index("flow")]]
        return plan

    def graph_stats(self):
        """(graphs captured, graph launches) of this handle (``mftx_raft_graph_stats``)."""
        c, r = C.c_ulonglong(), C.c_ulonglong()
        check(_lib.load().mftx_raft_graph_stats(self._h, C.byref(c), C.byref(r)), "mftx_raft_graph_stats")
        return int(c.value), int(r.value)

    def nonfinite_count(self, reset=False):
        """Output pixels with a non-finite flow / occlusion / sigma since the last reset (one 4-byte read: synchronises)."""
        n = int(self._nonfinite[0].item())
        if reset and n:
            self._nonfinite.zero_()
        return n

    def nonfinite_snapshot(self, host_words):
        """Enqueue, on the current stream, a copy of the counter into ``host_words`` (4 int32 of PINNED host memory, the count in
        word 0) -- no host wait: whoever later waits for an event recorded behind this call may read the word."""
        copy_bytes(self._nonfinite, host_words)

    def set_option(self, name, value):
        if name not in self.OPTIONS:
            raise MftxError(f"unknown engine option {name!r} (known: {', '.join(sorted(self.OPTIONS))}, gather)")
        check(_lib.load().mftx_raft_set_option(self._h, self.OPTIONS[name], int(value)), "mftx_raft_set_option")
        if name == "tile_conv":
            self._tile_conv = int(value)
        if name == "tile_volume":
            self._tile_volume = int(value)

    def workspace(self, P, h, w):
        need = _lib.load().mftx_raft_workspace_bytes_for(self._h, P, h, w)
        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None:      # graphs captured on the old buffer would keep pointing into freed memory
                check(_lib.load().mftx_raft_clear_graphs(self._h), "mftx_raft_clear_graphs")
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    REGIONS = ("lvl0", "lvl1", "lvl2", "lvl3", "coords1", "corr", "cor1", "corflo", "flo1", "hx", "z", "rh", "fh",
               "delta", "mask", "ouin", "ouh", "ou", "flow_lr")

    #: regions stored in split form when the engine runs the split arithmetic (they feed GEMMs), and their row strides
    SPLIT_REGIONS = {"cor1": 256, "corflo": 256, "flo1": 128, "hx": 384, "rh": 128, "ouin": 712}

    def region(self, name, P, h, w, cols, split=None):
        """A workspace region as [P*h*w, cols] fp32 (parity tests): a view, or -- for the regions the split arithmetic
        keeps in split form -- the decoded values.  split: None = decode SPLIT_REGIONS where ``plan(P, h, w)["presplit"]`` says
        activations are kept in split form (with presplit = 0 they are fp32 like everything else); True / False = decode the
        region's first ``cols`` columns as one row / do not, whatever the name (``fh``, below).  A region that is not decoded is
        viewed with ``cols`` floats per cell, so ``cols`` must be its whole row there (``ou``: 4, ``hx``: 384).

        What a region holds after ``refine`` returns (RefineCall::core; tests/refine_reference.py: REGION_MAP is this table, and
        tests/test_gpu_refine_family.py holds every entry against fp64).  Last iteration = the one the call ended with.

        ==========  =======  ==============================================================  ================================
        region      columns  holds                                                           on which plans
        ==========  =======  ==============================================================  ================================
        lvl0..lvl3           the correlation pyramid (``pyramid_layout``)                    every plan but ``ondemand_corr``
        corr        0:324    the lookup features the last iteration started from             every plan
        cor1        0:256    relu(convc1), last iteration (split)                            every plan
        corflo      0:256    relu(convc2) 0:192 | relu(convf2) 192:256, last iteration       every plan
                             (split)
        hx          0:128    h after the last vertical GRU pass (split)                      every plan
        hx          128:256  the caller's inp (split: its split round trip)                  every plan
        hx          256:384  motion features 0:126 | the flow they were formed from, x y     every plan
                             (split)
        delta       0:2      the last iteration's update                                     every plan
        coords1     0:2      the coordinates after the last update                           every plan
        fh          0:256    relu(mask.0) (split where presplit; not in SPLIT_REGIONS: until every plan
                             the mask head runs it is the flow head's fp32 scratch)
        mask        0:576    0.25 * mask.2(...)                                              every plan
        ou          0:3      occlusion logits 0:2 | uncertainty 2 (column 3 unused)          every plan
        flow_lr     0:2      coords1 - grid, unless ``refine(want_flow_lr=True)`` took it    every plan
        flo1        0:128    relu(convf1), last iteration (split)                            plan["flow"] != "fused" (fused:
                                                                                             the second coordinate buffer)
        z, rh       0:128    the vertical pass's z gate; r * h (rh split)                    not plan["gru_fused"]
        ouin        0:712    net | inp | corr | flow_lr | delta | motion (split)             plan["ou_materialised"]
        ouh         0:256    relu(conv1) of the occlusion | uncertainty head                 not plan["ou_fused"] (fused: the
                                                                                             projection's partial sums)
        ==========  =======  ==============================================================  ================================
        """
        offs = (C.c_size_t * 19)()
        check(_lib.load().mftx_raft_workspace_layout_for(self._h, P, h, w, offs, 19), "mftx_raft_workspace_layout_for")
        off = offs[self.REGIONS.index(name)]
        M = P * h * w
        if split is None:
            split = self.arith == ARITH_SPLIT and name in self.SPLIT_REGIONS and self.plan(P, h, w)["presplit"]
        if split:
            ld = self.SPLIT_REGIONS.get(name, cols)
            raw = self._ws[off: off + 4 * M * ld].view(torch.float32).reshape(M, ld)
            return unsplit_activations(raw)[:, :cols]
        return self._ws[off: off + 4 * M * cols].view(torch.float32).reshape(M, cols)

    MAX_GATHER = 16

    def can_gather(self, P):
        """``refine`` accepts LISTS of per-pair maps (no stacking into batch tensors) -- the split arithmetic with the
        stored, tile-resident correlation volume, up to 16 pairs."""
        return (self.arith == ARITH_SPLIT and not self.ondemand_corr and P <= self.MAX_GATHER and
                getattr(self, "_tile_volume", 1) != 0 and getattr(self, "_gather", True))

    def prepare_frame(self, fmap, inp, h, w, context=True, split=True):
        """What a refinement computes from its LEFT frame alone (``mftx_raft_frame_prepare``), on the current stream:
        -> (ctx, fsplit): ctx = the four context parts (zr1 [N,256], q1 [N,128], zr2 [N,256], q2 [N,128]) or None, fsplit = the split
        form of fmap [N,256] or None.  ``refine(..., prepared=...)`` takes them in place of recomputing them for every pair.
        The context parts need ``tile_conv`` pinned (0 or 2) on this handle."""
        lib = _lib.load()
        N = h * w
        dev = self.device
        ctx = fsplit = scratch = None
        if context:
            ctx = tuple(torch.empty(N, c, dtype=torch.float32, device=dev) for c in (256, 128, 256, 128))
            scratch = torch.empty(lib.mftx_raft_frame_prepare_bytes(h, w), dtype=torch.uint8, device=dev)
        if split:
            fsplit = torch.empty(N, 256, dtype=torch.float32, device=dev)
        cp = [t.data_ptr() for t in ctx] if context else [None] * 4
        check(lib.mftx_raft_frame_prepare(self._h, h, w, _chk(fmap, "fmap") if split else None, _chk(inp, "inp") if context else None,
                                          *cp, fsplit.data_ptr() if split else None,
                                          scratch.data_ptr() if context else None, scratch.numel() if context else 0, _stream()),
              "mftx_raft_frame_prepare")
        return ctx, fsplit

    def refine(self, fmap1, fmap2, net, inp, h, w, iters, pads=(0, 0, 0, 0), want_flow_lr=False, flow_init=None,
               packed=None, planar=True, prepared=None):
        """fmap1/fmap2 [P, h*w, 256], net/inp [P, h*w, 128] pixel-major ->
        flow [P,2,H0,W0], occl [P,1,H0,W0], sigma [P,1,H0,W0] (+ flow_lr [P,h*w,2]).
        flow_init: optional [P, h*w, 2] initial flow at 1/8 resolution (core/raft.py:153-154).
        packed: optional pre-allocated [P,H0,W0,4] that also receives (fx, fy, occl, sigma) per pixel;
        planar=False (with packed): only the packed result is written, flow = occl = sigma = None.
        prepared (per-pair map lists only): {"ctx": [the P left frames' context parts, 4 tensors each] | None, "f1s": [the P left
        frames' split maps] | None, "f2s": the shared right frame's split map | None} from ``prepare_frame``: the same bits."""
        lib = _lib.load()
        gathered = isinstance(fmap1, (list, tuple))      # per-pair maps [h*w, 256] / [h*w, 128] (mftx_raft_refine_gather)
        P = len(fmap1) if gathered else fmap1.shape[0]
        pl, pr, pt, pb = pads
        H0, W0 = 8 * h - pt - pb, 8 * w - pl - pr
        dev = self.device
        if not planar and packed is None:
            raise MftxError("refine: planar=False needs a packed output")
        flow = torch.empty(P, 2, H0, W0, dtype=torch.float32, device=dev) if planar else None
        occl = torch.empty(P, 1, H0, W0, dtype=torch.float32, device=dev) if planar else None
        sigma = torch.empty(P, 1, H0, W0, dtype=torch.float32, device=dev) if planar else None
        flow_lr = torch.empty(P, h * w, 2, dtype=torch.float32, device=dev) if want_flow_lr else None
        if flow_init is not None and tuple(flow_init.shape) != (P, h * w, 2):
            raise MftxError("flow_init must be [P, h*w, 2]")
        if packed is not None and tuple(packed.shape) != (P, H0, W0, 4):
            raise MftxError("packed must be [P, H0, W0, 4]")
        ws = self.workspace(P, h, w)

        def tail():      # flow_init ... stream: what every entry point takes behind the maps (evaluated in argument order)
            return (_chk(flow_init, "flow_init") if flow_init is not None else None, pl, pr, pt, pb,
                    flow.data_ptr() if planar else None, occl.data_ptr() if planar else None, sigma.data_ptr() if planar else None,
                    _chk(packed, "packed") if packed is not None else None, flow_lr.data_ptr() if want_flow_lr else None,
                    ws.data_ptr(), ws.numel(), _stream())

        if gathered:
            if not self.can_gather(P) or not (len(fmap2) == len(net) == len(inp) == P):
                raise MftxError("refine: per-pair map lists need the split arithmetic with the tile-resident volume and P <= 16")
            arrs = [_lib.ptr_array([_chk(t, "map") for t in lst]) for lst in (fmap1, fmap2, net, inp)]
            maps = [a[0] for a in arrs]
            if prepared:
                ctx, f1s, f2s = prepared.get("ctx"), prepared.get("f1s"), prepared.get("f2s")
                if (ctx is not None and len(ctx) != P) or (f1s is not None and len(f1s) != P):
                    raise MftxError("refine: prepared parts for every pair, or none")
                carr = _lib.ptr_array([_chk(t, "context part") for parts in ctx for t in parts]) if ctx is not None else (None, None)
                sarr = _lib.ptr_array([_chk(t, "split map") for t in f1s]) if f1s is not None else (None, None)
                check(lib.mftx_raft_refine_gather_ex(self._h, P, h, w, iters, *maps, carr[0], sarr[0],
                                                     _chk(f2s, "split map") if f2s is not None else None, *tail()),
                      "mftx_raft_refine_gather_ex")
            else:
                check(lib.mftx_raft_refine_gather(self._h, P, h, w, iters, *maps, *tail()), "mftx_raft_refine_gather")
        elif prepared:
            raise MftxError("refine: prepared parts go with per-pair map lists")
        else:
            check(lib.mftx_raft_refine(self._h, P, h, w, iters, _chk(fmap1, "fmap1"), _chk(fmap2, "fmap2"),
                                       _chk(net, "net"), _chk(inp, "inp"), *tail()), "mftx_raft_refine")
        return (flow, occl, sigma, flow_lr) if want_flow_lr else (flow, occl, sigma)
