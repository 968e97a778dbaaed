"""The encoders (csrc/encoder.hip) layer by layer against fp64, at small and odd sizes.

a. ``enc_prep_kernel`` alone (``ops.encoder_prep``), bit for bit against numpy in fp32.
b. The three ``instnorm_*`` kernels alone (``ops.instance_norm``) against a two-pass fp64 reference: row counts below, at and off
   the slab count and the rows-per-pass, all three modes, fp32 and split-form output, an all-equal channel, a channel whose
   statistics cancel, a channel holding a NaN.
c. The stem exactly as the engine describes it (28-float windows every 4 floats, 7 row taps, stride 2) against fp64.
d. The stride-2 convolutions of the residual stages in split arithmetic with split-form operands.
e. Both encoders restated in Python from ``ops.encoder_prep`` / ``ops.conv2d`` / ``ops.instance_norm`` with the engine's descriptors:
   the restated head equals ``EncoderEngine.forward`` bit for bit (plain launches, graph capture, graph replay), which makes the
   stage maps the engine's own; every stage map is then held against ``O.encoder_stages`` in fp64.
f. One engine fed changing sizes.
g. Argument errors of the encoder entry points, called raw.

Bounds against fp64 are multiples of the reference arithmetic's own rounding noise on the same input (fp32 torch against fp64 torch):
K_MEAN = 4 for means, K_MAX = 8 for maxima, the constants of tests/test_gpu_offgrid.py, set before the first run; a bound may be
raised only with the explanation written next to it, never above 16.  Observed ratios: profiles/encoder_noise.txt.

Needs an MI355X."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mft_oracle as O
from test_gpu_offgrid import K_MAX, K_MEAN

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, SPLIT = 0, 1
ARITH_NAME = {F32: "fp32", SPLIT: "split"}
SPLIT_REP = 2.0 ** -22          # representation error of the 22-bit split form, relative (hi: 11 bits, lo: 11 more)
SPLIT_FLOOR = 2.0 ** -36        # ... and absolute, where the low half is itself a subnormal fp16 (test_split_weights_format)


@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


@pytest.fixture(scope="module")
def sd_dev(weights_np):
    return {k: torch.from_numpy(v).to(DEV) for k, v in weights_np.items()}


def _threads():
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))


def _ratio(hip, noise):
    return hip / noise if noise > 0 else (0.0 if hip == 0 else float("inf"))


# =====================================================================================================================
# a. pre-processing
# =====================================================================================================================

# the pad of each axis is 0, odd and even: 16 -> 0, 17 -> 7, 23 -> 1, 21 -> 3, 18 -> 6, 24 / 40 -> 0, 125 -> 3, 187 -> 5
PREP_SIZES = [(16, 16), (17, 23), (21, 18), (24, 40), (125, 187)]


def _frame_all_bytes(H, W, seed):
    """Random bytes with all 256 values present in every channel (its first 256 pixels: three different permutations)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    flat = img.reshape(-1, 3)
    for c, (k, off) in enumerate(((1, 0), (37, 11), (101, 200))):
        flat[:256, c] = (np.arange(256) * k + off) % 256
    return img


def _prep_reference(img):
    H0, W0 = img.shape[:2]
    l, r, t, b = O.pad_amounts(H0, W0)
    v = np.pad(img[:, :, ::-1], ((t, b), (l, r), (0, 0)), mode="edge").astype(np.float32)
    x = np.float32(2) * (v / np.float32(255)) - np.float32(1)
    out = np.zeros((H0 + t + b, W0 + l + r + 6, 4), np.float32)
    out[:, 3:-3, :3] = x
    return out, (l, r, t, b)


@pytest.mark.parametrize("H,W", PREP_SIZES)
def test_encoder_prep_bitwise(ops, H, W):
    """BGR -> RGB, 2 (v / 255) - 1, replicate pad with the smaller half left / top, three zero columns either side, zero 4th
    channel: equal to numpy's fp32 bit for bit.  That is derivable: the division is correctly rounded on both sides, 2 q is exact,
    so whether the compiler contracts 2 q - 1 into an FMA cannot change the result."""
    img = _frame_all_bytes(H, W, 100 + H)
    for c in range(3):
        assert len(np.unique(img[:, :, c])) == 256
    want, (l, r, t, b) = _prep_reference(img)
    ph, pw = (-H) % 8, (-W) % 8
    assert (l, t) == (pw // 2, ph // 2) and (l + r, t + b) == (pw, ph)
    got = ops.encoder_prep(torch.from_numpy(img).to(DEV)).cpu().numpy()
    assert got.shape == want.shape == (H + ph, W + pw + 6, 4)
    assert not got[:, :3].any() and not got[:, -3:].any(), "guard columns"
    assert not got[:, :, 3].any(), "4th channel"
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    # the first frame pixel lies at (pad_top, 3 + pad_left); with pad > 1 an even split and pad // 2 differ by a whole pixel
    x00 = np.float32(2) * (img[0, 0, ::-1].astype(np.float32) / np.float32(255)) - np.float32(1)
    assert np.array_equal(got[t, 3 + l, :3], x00) and np.array_equal(got[0, 3, :3], x00)
    xlast = np.float32(2) * (img[-1, -1, ::-1].astype(np.float32) / np.float32(255)) - np.float32(1)
    assert np.array_equal(got[t + H - 1, 3 + l + W - 1, :3], xlast) and np.array_equal(got[-1, -4, :3], xlast)


# =====================================================================================================================
# b. instance norm
# =====================================================================================================================

# C = 96: 24 float4 columns, 10 rows per pass, 16 idle threads in the partial kernel.  rows: fewer than the 256 slabs (most
# slabs empty), the slab count and its neighbours, not divisible by the slab count or the rows-per-pass
IN_CHANNELS = [64, 96, 128, 256]
IN_ROWS = [1, 4, 6, 255, 256, 257, 1031, 4099]
CH_EQUAL, CH_CANCEL, CH_NAN = 1, 2, 3
EQUAL_VALUE = 3.3
GUARD = 64                      # floats of canary on either side of x


def _norm_input(rows, Cc):
    g = torch.Generator().manual_seed(rows * 7 + Cc)
    x = torch.randn(rows, Cc, generator=g) * torch.exp(torch.randn(Cc, generator=g)) + 3 * torch.randn(Cc, generator=g)
    x[:, CH_EQUAL] = EQUAL_VALUE
    x[:, CH_CANCEL] = 1000 + 1e-3 * torch.randn(rows, generator=g)
    res = torch.randn(rows, Cc, generator=g)
    return x, res


def _norm_formula(x, res, mode, eps=1e-5):
    """nn.InstanceNorm2d's formula (biased variance, two passes) in the dtype of x, then the mode's epilogue."""
    m = x.mean(0)
    y = (x - m) / torch.sqrt(((x - m) ** 2).mean(0) + eps)
    if mode == 2:
        return y
    y = torch.relu(y)
    return torch.relu(res + y) if mode == 1 else y


@pytest.mark.parametrize("rows", IN_ROWS)
@pytest.mark.parametrize("Cc", IN_CHANNELS)
def test_instance_norm_vs_fp64(ops, Cc, rows):
    """error(HIP, fp64) <= K * error(the same formula in fp32 torch, fp64) over the ordinary channels (K_MAX for the maximum,
    K_MEAN for the mean) and over all finite channels; with split-form output the 2^-22 |ref| of the representation comes on top.
    The all-equal channel is exact (the fp64 sum of `rows` equal floats is exact at these sizes, so the mean rounds back to the
    value: zeros, or relu(res) in mode 1).  The cancelling channel (mean 1000, standard deviation 1e-3: 16 fp32 ulps) is bounded
    by what its fp32 mean costs -- half an ulp of 1000, 2^-15, times 1 / sqrt(var + eps), about 9e-3 -- plus the rounding of fp64
    sums and of the fp32 result: statistics summed in fp32 miss that by two orders of magnitude (errors of order 1).  A NaN stays in its channel.  Same bits on a second run;
    without split form nothing outside x is read into the result or written."""
    x, res = _norm_input(rows, Cc)
    ordinary = [c for c in range(Cc) if c not in (CH_EQUAL, CH_CANCEL, CH_NAN)]
    finite = [c for c in range(Cc) if c != CH_NAN]
    x64 = x.double()
    rstd_cancel = float(1 / torch.sqrt(x64[:, CH_CANCEL].var(unbiased=False) + 1e-5)) if rows > 1 else 0.0
    x_nan = x.clone()
    x_nan[rows // 2, CH_NAN] = float("nan")
    failures = []
    for split in (False, True):
        # the residual as the kernel sees it: with split-form operands, the value its split form holds
        res_dev = ops.split_activations(res.to(DEV)) if split else res.to(DEV)
        res_eff = (ops.unsplit_activations(res_dev) if split else res_dev).cpu()
        for mode in (0, 1, 2):
            ref = _norm_formula(x64, res_eff.double(), mode)
            noise = (_norm_formula(x, res_eff, mode).double() - ref).abs()

            def run(src, fill=0.0):
                buf = torch.full((GUARD + rows * Cc + GUARD,), fill, device=DEV)
                xd = buf[GUARD:GUARD + rows * Cc].view(rows, Cc)
                xd.copy_(src)
                out = ops.instance_norm(xd, mode, res_dev if mode == 1 else None, split=split)
                assert out is xd
                return buf

            buf = run(x, 7.5)
            raw = buf[GUARD:GUARD + rows * Cc].view(rows, Cc)
            got = (ops.unsplit_activations(raw) if split else raw).cpu()
            assert bool((buf[:GUARD] == 7.5).all()) and bool((buf[-GUARD:] == 7.5).all()), "canaries"
            again = run(x, float("nan") if not split else 7.5)
            assert torch.equal(again[GUARD:-GUARD].view(torch.int32), buf[GUARD:-GUARD].view(torch.int32)), \
                (split, mode, "second run / other guard values")
            if not split:
                assert bool(torch.isnan(again[:GUARD]).all()) and bool(torch.isnan(again[-GUARD:]).all()), "canaries"
            # ---- the all-equal channel: exact
            want_eq = torch.relu(res_eff[:, CH_EQUAL]) if mode == 1 else torch.zeros(rows)
            assert torch.equal(got[:, CH_EQUAL], want_eq), (split, mode, "all-equal channel")
            # ---- the NaN stays in its channel
            nan_raw = run(x_nan, 7.5)[GUARD:-GUARD].view(rows, Cc)
            got_nan = (ops.unsplit_activations(nan_raw) if split else nan_raw).cpu()
            assert bool(torch.isnan(got_nan[:, CH_NAN]).all()), (split, mode, "NaN channel")
            assert torch.equal(got_nan[:, finite], got[:, finite]), (split, mode, "NaN leaked")
            # ---- against fp64
            err = (got.double() - ref).abs()
            if split:
                err = (err - SPLIT_REP * ref.abs()).clamp_min(0)
            for name, cols in (("ordinary", ordinary), ("finite", finite)):
                for q, k, h, n in (("max", K_MAX, float(err[:, cols].max()), float(noise[:, cols].max())),
                                   ("mean", K_MEAN, float(err[:, cols].mean()), float(noise[:, cols].mean()))):
                    print(f"instnorm-noise C {Cc:3d} rows {rows:4d} mode {mode} {'split' if split else 'fp32 '} {name:8s} {q:4s} "
                          f"hip/fp64 {h:.3e}  fp32/fp64 {n:.3e}  ratio {_ratio(h, n):6.2f}  (bound {k:g})")
                    if not h <= k * n:
                        failures.append((split, mode, name, q, h, n))
            # (the two further terms: E[x^2] - mean^2 in fp64 -- any summation order errs by at most (rows + 2) 2^-53 of each of the
            # two, and a relative error d of var + eps is d / 2 of the result; fp32 rounding of rstd, of the product and, in mode 1,
            # of the sum with res, of magnitude up to ~5)
            n_cancel = _norm_formula(x64, None, 2)[:, CH_CANCEL].abs()
            dvar = 2 * (rows + 2) * 2.0 ** -53 * float((x64[:, CH_CANCEL] ** 2).mean())
            cancel_bound = 2.0 ** -15 * rstd_cancel + 0.5 * dvar * rstd_cancel ** 2 * n_cancel + 2.0 ** -21 * (n_cancel + 5.0)
            e = (got[:, CH_CANCEL].double() - ref[:, CH_CANCEL]).abs()
            if not bool((e <= cancel_bound).all()):
                failures.append((split, mode, "cancelling channel", float(e.max()), float(cancel_bound.max())))
    assert not failures, failures


def test_instance_norm_wrapper_refuses_bad_shapes(ops):
    x = torch.zeros(8, 64, device=DEV)
    with pytest.raises(ops.MftxError):
        ops.instance_norm(x, 1)                                  # mode 1 without res
    with pytest.raises(ops.MftxError):
        ops.instance_norm(x, 0, res=torch.zeros(8, 32, device=DEV))
    with pytest.raises(ops.MftxError):
        ops.instance_norm(torch.zeros(8, 60, device=DEV), 0)     # C % 8
    with pytest.raises(ops.MftxError):
        ops.instance_norm(torch.zeros(8, 264, device=DEV), 0)    # C > 256
    with pytest.raises(ops.MftxError):
        ops.instance_norm(x, 3)
    assert not x.any()


# =====================================================================================================================
# c. the stem as the engine launches it
# =====================================================================================================================

STEM_SIZES = [(16, 16), (17, 23), (24, 40), (16, 264)]


def _stem_conv(ops, prep, wk, bias, arith, act):
    """mftx_encoder_forward's stem descriptor (csrc/encoder.hip): windows of 28 floats (7 pixels x RGB0) every 4 floats, 7 row
    taps, stride 2, 3 rows of zero padding, none in x (the three guard columns are the padding)."""
    Hp, Wq = prep.shape[:2]
    Wp = Wq - 6
    return ops.conv2d(prep.view(-1, 4), wk, bias, 1, Hp // 2, Wp // 2, 64, 7, 1, act=act, stride=2, hin=Hp, win=Wp + 6,
                      pad_y=3, pad_x=-1, arith=arith, lda0=4, c0=28)


def _nchw(t, h, w):
    """pixel-major [h*w, C] on the device -> [1, C, h, w] fp64 on the host."""
    return t.reshape(h, w, -1).permute(2, 0, 1)[None].cpu().double()


def _regions(err):
    """max error over the border columns / rows and the interior of a [1, C, h, w] map (the stem's 7-wide windows reach the
    zero padding from the two outermost cells of every side)."""
    h, w = err.shape[-2:]
    r = {"left": err[..., :, :2], "right": err[..., :, -2:], "top": err[..., :2, :], "bottom": err[..., -2:, :]}
    out = {k: float(v.max()) for k, v in r.items()}
    out["interior"] = float(err[..., 2:-2, 2:-2].max()) if h > 4 and w > 4 else 0.0
    return out


@pytest.mark.parametrize("arith", [F32, SPLIT])
@pytest.mark.parametrize("prefix", ["fnet", "cnet"])
@pytest.mark.parametrize("H,W", STEM_SIZES)
def test_stem_conv_vs_fp64(ops, sd_dev, H, W, prefix, arith):
    """The 7 x 7 stride-2 stem on the engine's own input (ops.encoder_prep), weights (pack_encoder_weights, cnet's with the batch
    norm folded in) and descriptor -- fnet's without activation, cnet's with its ReLU -- against F.conv2d(stride 2, padding 3) in
    fp64 on the same operands; the yardstick is fp32 F.conv2d on the CPU."""
    _threads()
    img = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    prep = ops.encoder_prep(torch.from_numpy(img).to(DEV))
    pk, bias = ops.pack_encoder_weights(sd_dev, prefix, prefix == "cnet", DEV)[0:2]
    act = "relu" if prefix == "cnet" else None
    out = _stem_conv(ops, prep, ops.split_weights(pk) if arith == SPLIT else pk, bias, arith, act)
    Hp, Wp = prep.shape[0], prep.shape[1] - 6
    got = _nchw(out, Hp // 2, Wp // 2)
    # the same operands on the host: the normalised padded frame (test a pins it), the packed weight back in [64, 3, 7, 7]
    x32 = prep[:, 3:-3, :3].permute(2, 0, 1)[None].cpu()
    w32 = pk[:64, :, :28].reshape(64, 7, 7, 4)[..., :3].permute(0, 3, 1, 2).contiguous().cpu()
    assert not pk[:64, :, :28].reshape(64, 7, 7, 4)[..., 3].any() and not pk[64:].any() and not pk[:, :, 28:].any()
    b32 = bias.cpu()
    fn = torch.relu if act else (lambda t: t)
    ref = fn(F.conv2d(x32.double(), w32.double(), b32.double(), stride=2, padding=3))
    noise = (fn(F.conv2d(x32, w32, b32, stride=2, padding=3)).double() - ref).abs()
    err = (got - ref).abs()
    where = {k: (v, _regions(noise)[k]) for k, v in _regions(err).items()}
    print(f"stem-noise {H}x{W} {prefix} {ARITH_NAME[arith]:5s} max hip/fp64 {float(err.max()):.3e} fp32/fp64 {float(noise.max()):.3e} "
          f"ratio {_ratio(float(err.max()), float(noise.max())):5.2f} (bound {K_MAX:g})  mean hip/fp64 {float(err.mean()):.3e} "
          f"fp32/fp64 {float(noise.mean()):.3e} ratio {_ratio(float(err.mean()), float(noise.mean())):5.2f} (bound {K_MEAN:g})  "
          + "  ".join(f"{k} {a:.2e}/{b:.2e}" for k, (a, b) in where.items()))
    assert float(err.max()) <= K_MAX * float(noise.max()), ("max error by region (hip, fp32 noise)", where)
    assert float(err.mean()) <= K_MEAN * float(noise.mean()), ("max error by region (hip, fp32 noise)", where)
    for k, (a, _) in where.items():                       # a wrong border tap is an error of the size of a product, not of a rounding
        assert a <= K_MAX * float(noise.max()), (k, where)


# =====================================================================================================================
# d. strided convolutions in split arithmetic with split-form operands
# =====================================================================================================================

@pytest.mark.parametrize("hin,win", [(8, 8), (32, 48), (17, 23)])
@pytest.mark.parametrize("cin,cout,k", [(64, 96, 3), (64, 96, 1), (96, 128, 3), (96, 128, 1)])
def test_conv2d_strided_split_form_operands(ops, cin, cout, k, hin, win):
    """The stride-2 layers of the residual stages (3 x 3 and the 1 x 1 shortcut) as the engine runs them in split arithmetic: a
    pre-split A operand gives the bits of A split in registers (as test_conv2d_split_form_operands asserts at stride 1), a
    split-form output decodes to the fp32 output within the representation error, and the residual tail relu(relu(conv + b) + res)
    after a split-form convolution meets the bound of test_conv2d_split_arith_vs_fp64's family against fp64."""
    _threads()
    h, w = (hin + 1) // 2, (win + 1) // 2
    g = torch.Generator().manual_seed(cin + cout + k + hin)
    x = torch.randn(hin * win, cin, generator=g) * torch.exp(torch.randn(hin * win, cin, generator=g))
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.1
    res = torch.randn(h * w, cout, generator=g)
    xd, bd, resd = x.to(DEV), b.to(DEV), res.to(DEV)
    ws = ops.split_weights(ops.pack_conv_weight(wt.to(DEV)))
    kw = dict(stride=2, hin=hin, win=win, arith=ops.ARITH_SPLIT)
    base = ops.conv2d(xd, ws, bd, 1, h, w, cout, k, k, **kw)
    xs = ops.split_activations(xd)
    pre = ops.conv2d(xs, ws, bd, 1, h, w, cout, k, k, a_split=True, **kw)
    assert torch.equal(pre, base), int((pre != base).sum())
    outs = ops.unsplit_activations(ops.conv2d(xs, ws, bd, 1, h, w, cout, k, k, a_split=True, out_split=True, **kw))
    assert bool(((outs.double() - base.double()).abs() <= SPLIT_REP * base.double().abs() + SPLIT_FLOOR).all())
    # against fp64: the plain layer, and the residual tail
    x64 = x.reshape(1, hin, win, cin).permute(0, 3, 1, 2).double()
    ref = F.conv2d(x64, wt.double(), b.double(), stride=2, padding=k // 2)
    assert ref.shape[-2:] == (h, w)
    e = float((_nchw(base, h, w) - ref).abs().max())
    assert e <= 3e-6 * float(ref.abs().max()), (e, float(ref.abs().max()))
    tail = ops.conv2d(xs, ws, bd, 1, h, w, cout, k, k, act="relu", a_split=True, residual_mode=1, addend=resd, **kw)
    tail_reg = ops.conv2d(xd, ws, bd, 1, h, w, cout, k, k, act="relu", residual_mode=1, addend=resd, **kw)
    assert torch.equal(tail, tail_reg)
    ref_tail = torch.relu(torch.relu(ref) + res.reshape(1, h, w, cout).permute(0, 3, 1, 2).double())
    e = float((_nchw(tail, h, w) - ref_tail).abs().max())
    assert e <= 3e-6 * float(ref_tail.abs().max()), (e, float(ref_tail.abs().max()))


# =====================================================================================================================
# e. the encoders layer by layer
# =====================================================================================================================

# EncConv order (csrc/encoder.hip)
(EC_STEM, EC_L1B0C1, EC_L1B0C2, EC_L1B1C1, EC_L1B1C2, EC_L2B0C1, EC_L2B0C2, EC_L2B0DS, EC_L2B1C1, EC_L2B1C2, EC_L3B0C1, EC_L3B0C2,
 EC_L3B0DS, EC_L3B1C1, EC_L3B1C2, EC_HEAD, EC_HEAD2) = range(17)


class Pipeline:
    """mftx_encoder_forward restated: Enc::conv, Enc::norm, Enc::block and the stem / head sequence of csrc/encoder.hip with the
    same descriptors and split flags, on tensors of its own instead of the workspace.  ``run`` keeps every stage map."""

    def __init__(self, ops, sd, prefix, instance_norm, arith):
        self.ops, self.inorm, self.arith = ops, instance_norm, arith
        w = ops.pack_encoder_weights(sd, prefix, not instance_norm, DEV)
        self.b = w[1::2]
        self.wg = [ops.split_weights(t) for t in w[0::2]] if arith == SPLIT else w[0::2]

    @property
    def sp(self):
        return self.arith == SPLIT

    def conv(self, slot, x, hin, win, cout, h, w, k, stride, act, residual=None, a_split=False, out_split=False):
        return self.ops.conv2d(x, self.wg[slot], self.b[slot], 1, h, w, cout, k, k, act=act, stride=stride, hin=hin, win=win,
                               addend=residual, residual_mode=1 if residual is not None else 0, arith=self.arith,
                               a_split=self.sp and a_split, out_split=self.sp and out_split)

    def norm(self, x, mode, res=None):
        return self.ops.instance_norm(x, mode, res, split=self.sp)

    def block(self, c1, c2, ds, x, hin, win, planes, h, w, stride, shortcuts, name):
        if self.inorm:
            tmp = self.norm(self.conv(c1, x, hin, win, planes, h, w, 3, stride, None, a_split=True), 0)
            out = self.conv(c2, tmp, h, w, planes, h, w, 3, 1, None, a_split=True)
            shortcut = x
            if stride != 1:
                shortcut = self.norm(self.conv(ds, x, hin, win, planes, h, w, 1, stride, None, a_split=True), 2)
                shortcuts[name] = shortcut
            return self.norm(out, 1, shortcut)
        tmp = self.conv(c1, x, hin, win, planes, h, w, 3, stride, "relu", out_split=True)
        shortcut = x
        if stride != 1:
            shortcut = self.conv(ds, x, hin, win, planes, h, w, 1, stride, None)
            shortcuts[name] = shortcut
        return self.conv(c2, tmp, h, w, planes, h, w, 3, 1, "relu", residual=shortcut, a_split=True)

    def run(self, img_dev):
        """-> (stages: eight [rows, C] maps in O.ENCODER_STAGES order, as the engine stores them; shortcuts; head outputs as
        EncoderEngine.forward returns them; (h, w) of every stage)."""
        prep = self.ops.encoder_prep(img_dev)
        Hp, Wp = prep.shape[0], prep.shape[1] - 6
        h1, w1, h2, w2, h3, w3 = Hp // 2, Wp // 2, Hp // 4, Wp // 4, Hp // 8, Wp // 8
        a = _stem_conv(self.ops, prep, self.wg[EC_STEM], self.b[EC_STEM], self.arith, None if self.inorm else "relu")
        if self.inorm:
            a = self.norm(a, 0)
        stages, shortcuts = [a], {}
        c = self.block(EC_L1B0C1, EC_L1B0C2, -1, a, h1, w1, 64, h1, w1, 1, shortcuts, "layer1.0")
        a = self.block(EC_L1B1C1, EC_L1B1C2, -1, c, h1, w1, 64, h1, w1, 1, shortcuts, "layer1.1")
        stages += [c, a]
        c = self.block(EC_L2B0C1, EC_L2B0C2, EC_L2B0DS, a, h1, w1, 96, h2, w2, 2, shortcuts, "layer2.0")
        a = self.block(EC_L2B1C1, EC_L2B1C2, -1, c, h2, w2, 96, h2, w2, 1, shortcuts, "layer2.1")
        stages += [c, a]
        c = self.block(EC_L3B0C1, EC_L3B0C2, EC_L3B0DS, a, h2, w2, 128, h3, w3, 2, shortcuts, "layer3.0")
        a = self.block(EC_L3B1C1, EC_L3B1C2, -1, c, h3, w3, 128, h3, w3, 1, shortcuts, "layer3.1")
        stages += [c, a]
        if self.inorm:
            head = (self.conv(EC_HEAD, a, h3, w3, 256, h3, w3, 1, 1, None, a_split=True), None)
            stages.append(head[0])
        else:
            head = (self.conv(EC_HEAD, a, h3, w3, 128, h3, w3, 1, 1, "tanh"), self.conv(EC_HEAD2, a, h3, w3, 128, h3, w3, 1, 1, "relu"))
            stages.append(torch.cat(head, 1))
        grids = [(h1, w1)] * 3 + [(h2, w2)] * 2 + [(h3, w3)] * 3
        return stages, shortcuts, head, grids

    def decode(self, stage_index, t):
        """A stage map as fp32 values: with the split arithmetic fnet's normalised maps (every stage but the head) are stored in
        split form; cnet's stage maps are fp32 (only its blocks' inner maps are split)."""
        if self.sp and self.inorm and stage_index < 7:
            return self.ops.unsplit_activations(t)
        return t


@pytest.fixture(scope="module")
def enc(ops, sd_dev):
    out = {}
    for prefix, inorm in (("fnet", True), ("cnet", False)):
        for arith in (F32, SPLIT):
            out[prefix, arith] = SimpleNamespace(
                pipe=Pipeline(ops, sd_dev, prefix, inorm, arith),
                plain=ops.EncoderEngine(sd_dev, prefix, inorm, DEV, arith=arith, graph=False),
                graphed=ops.EncoderEngine(sd_dev, prefix, inorm, DEV, arith=arith, graph=True))
    return out


ENC_SIZES = [(16, 16), (17, 23), (24, 40), (61, 67), (16, 264), (264, 16)]
FLAT_SIZES = [(16, 16), (17, 23), (16, 264)]             # the constant and near-constant frames run here only
FRAMES = ["random", "vstep", "checker", "hramp", "zero", "c200", "pixel"]
FLAT_FRAMES = ("zero", "c200", "pixel")


def _frame(kind, H, W):
    img = np.zeros((H, W, 3), np.uint8)
    xs = np.arange(W)[None, :, None]
    if kind == "random":
        img = np.random.default_rng(H * 31 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "c200":
        img[:] = 200
    elif kind == "pixel":
        img[H // 2, W // 3] = 255
    elif kind == "vstep":
        img[:, W // 2:] = 210
        img[:, :W // 2] = 40
    elif kind == "checker":
        img[:] = (((np.arange(H)[:, None, None] + xs) & 1) * 255).astype(np.uint8)
    elif kind == "hramp":
        img[:] = (xs * 255 // (W - 1)).astype(np.uint8)
    else:
        assert kind == "zero"
    return img


_ORACLE = {}


def _oracle_stages(weights_cpu, H, W, kind, prefix):
    """(fp32 oracle stages, fp64 oracle stages, fp32 shortcuts, fp64 shortcuts), computed once per input; the head of cnet
    with its tanh | relu applied, as the engine returns it."""
    key = (H, W, kind, prefix)
    if key not in _ORACLE:
        img = _frame(kind, H, W)
        norm = "instance" if prefix == "fnet" else "batch"

        def finish(st):
            if prefix == "cnet":
                st[-1] = torch.cat([torch.tanh(st[-1][:, :128]), torch.relu(st[-1][:, 128:])], 1)
            return st
        with torch.no_grad():
            s32 = {}
            st32 = finish(O.encoder_stages(O.normalise_image(O.preprocess(img)), weights_cpu, prefix, norm, s32))
            with O.precision(torch.float64):
                s64 = {}
                st64 = finish(O.encoder_stages(O.normalise_image(O.preprocess(img)), O.cast_weights(weights_cpu, torch.float64),
                                               prefix, norm, s64))
        assert st64[0].dtype == torch.float64 and st32[0].dtype == torch.float32
        _ORACLE[key] = (st32, st64, s32, s64)
    return _ORACLE[key]


def _same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("prefix", ["fnet", "cnet"])
@pytest.mark.parametrize("H,W", ENC_SIZES)
def test_encoder_stages_vs_fp64(ops, enc, weights_cpu, H, W, prefix):
    """First, bit for bit: the restated pipeline's head output equals EncoderEngine.forward's with plain launches and with graphs
    (three consecutive calls on the first frame of a size: plain, capture, replay; replays from then on) -- so the stage maps are
    the engine's own.  Then, per stage map (and per normalised shortcut of the stride-2 blocks) and arithmetic, against
    O.encoder_stages in fp64:  max error <= K_MAX * noise_max, mean error <= K_MEAN * noise_mean, the noise being the fp32
    oracle's error on that stage."""
    _threads()
    failures = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fi, kind in enumerate(FRAMES):
            if kind in FLAT_FRAMES and (H, W) not in FLAT_SIZES:
                continue
            img = torch.from_numpy(_frame(kind, H, W)).to(DEV)
            st32, st64, sc32, sc64 = _oracle_stages(weights_cpu, H, W, kind, prefix)
            for arith in (F32, SPLIT):
                e = enc[prefix, arith]
                stages, shortcuts, head, grids = e.pipe.run(img)
                assert _same_bits(e.plain.forward(img), head), (kind, ARITH_NAME[arith], "plain launches")
                for call in range(3 if fi == 0 else 1):
                    assert _same_bits(e.graphed.forward(img), head), (kind, ARITH_NAME[arith], "graph", call)
                maps = [(name, e.pipe.decode(i, t), grids[i], st32[i], st64[i]) for i, (name, t) in enumerate(zip(O.ENCODER_STAGES, stages))]
                for name, t in shortcuts.items():
                    i = O.ENCODER_STAGES.index(name)
                    dec = ops.unsplit_activations(t) if (e.pipe.sp and e.pipe.inorm) else t
                    maps.append((name + ".sc", dec, grids[i], sc32[name], sc64[name]))
                assert len(maps) == 10
                for name, t, (h, w), r32, r64 in maps:
                    assert tuple(r64.shape[-2:]) == (h, w) and t.shape == (h * w, r64.shape[1]), (name, t.shape, r64.shape)
                    err = (_nchw(t, h, w) - r64).abs()
                    noise = (r32.double() - r64).abs()
                    hm, hx, nm, nx = float(err.mean()), float(err.max()), float(noise.mean()), float(noise.max())
                    print(f"encoder-noise {H}x{W} {kind:7s} {prefix} {ARITH_NAME[arith]:5s} {name:11s} max hip/fp64 {hx:.3e}  fp32/fp64 {nx:.3e}  "
                          f"ratio {_ratio(hx, nx):6.2f}  (bound {K_MAX:g})   mean hip/fp64 {hm:.3e}  fp32/fp64 {nm:.3e}  ratio {_ratio(hm, nm):6.2f}  "
                          f"(bound {K_MEAN:g})")
                    if not hx <= K_MAX * nx:
                        failures.append((kind, ARITH_NAME[arith], name, "max", hx, nx))
                    if not hm <= K_MEAN * nm:
                        failures.append((kind, ARITH_NAME[arith], name, "mean", hm, nm))
    side.synchronize()
    assert not failures, failures


# =====================================================================================================================
# f. one engine across sizes
# =====================================================================================================================

@pytest.mark.parametrize("graph", [False, True])
def test_one_engine_across_sizes(ops, sd_dev, graph):
    """(24, 40), then (61, 67) -- the workspace regrows --, then (24, 40) again on the same engine: the third result is the first,
    bit for bit; two more rounds take the graph cache (keyed by size and workspace) through capture and replay at both sizes."""
    imgs = {s: torch.from_numpy(_frame("random", *s)).to(DEV) for s in ((24, 40), (61, 67))}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for prefix, inorm in (("fnet", True), ("cnet", False)):
            eng = ops.EncoderEngine(sd_dev, prefix, inorm, DEV, graph=graph)
            first = {}
            for call, s in enumerate([(24, 40), (61, 67), (24, 40), (61, 67), (24, 40), (61, 67), (24, 40)]):
                out = tuple(t.clone() if t is not None else None for t in eng.forward(imgs[s]))
                assert out[0].shape[0] == -(-s[0] // 8) * -(-s[1] // 8)
                if s in first:
                    assert _same_bits(out, first[s]), (prefix, call, s)
                else:
                    first[s] = out
    side.synchronize()


# =====================================================================================================================
# g. argument errors, raw through ctypes
# =====================================================================================================================

E_ARG, E_ALIGN, E_WORKSPACE, E_STATE = -1, -2, -3, -4


def test_encoder_entry_points_argument_errors(ops, sd_dev):
    """mftx_encoder_create / _forward / _set_split_weights and mftx_instance_norm / mftx_encoder_prep refuse bad arguments with the
    library's negative codes before any launch, and a valid call on the same engine afterwards still gives the reference bits."""
    from mft_amd import _lib
    lib = _lib.load()
    H, W = 24, 40
    img = torch.from_numpy(_frame("random", H, W)).to(DEV)
    for prefix, inorm in (("fnet", True), ("cnet", False)):
        eng = ops.EncoderEngine(sd_dev, prefix, inorm, DEV, graph=False)
        want = tuple(t.clone() if t is not None else None for t in eng.forward(img))
        n = len(eng.weights)
        ptrs = [t.data_ptr() for t in eng.weights]
        handle = C.c_void_p()
        # ---- create
        for bad_n in (n - 2, n + 2, 0):
            assert lib.mftx_encoder_create(_lib.ptr_array(ptrs)[0], bad_n, int(inorm), C.byref(handle)) == E_ARG, bad_n
        assert lib.mftx_encoder_create(_lib.ptr_array(ptrs)[0], n, int(not inorm), C.byref(handle)) == E_ARG     # the other encoder's count
        assert lib.mftx_encoder_create(None, n, int(inorm), C.byref(handle)) == E_ARG
        assert lib.mftx_encoder_create(_lib.ptr_array(ptrs)[0], n, int(inorm), None) == E_ARG
        for i, bad in ((0, None), (n - 1, None), (3, ptrs[3] + 4)):
            p = list(ptrs)
            p[i] = bad
            assert lib.mftx_encoder_create(_lib.ptr_array(p)[0], n, int(inorm), C.byref(handle)) == E_ALIGN, (i, bad)
        assert handle.value is None
        # ---- forward
        ws = eng._ws
        need = lib.mftx_encoder_workspace_bytes(H, W)
        assert ws.numel() >= need and ws.data_ptr() % 256 == 0
        big = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
        out0 = torch.empty_like(want[0])
        out1 = torch.empty_like(want[1]) if want[1] is not None else None
        good = [eng._h, img.data_ptr(), H, W, out0.data_ptr(), out1.data_ptr() if out1 is not None else None, ws.data_ptr(), need, None]
        cases = [(2, 15, E_ARG), (3, 15, E_ARG), (2, 0, E_ARG), (7, need - 1, E_WORKSPACE), (6, big.data_ptr() + 16, E_ALIGN),
                 (1, None, E_ARG), (4, None, E_ARG), (6, None, E_ARG), (0, None, E_STATE)]
        if not inorm:
            cases.append((5, None, E_ARG))
        for i, bad, code in cases:
            a = list(good)
            a[i] = bad
            if i == 6 and bad is not None:
                a[7] = need + 256
            assert lib.mftx_encoder_forward(*a) == code, (i, bad, lib.mftx_last_error_string())
            assert lib.mftx_last_error_string()
            assert lib.mftx_encoder_forward(*good) == 0
            assert torch.equal(out0, want[0]) and (out1 is None or torch.equal(out1, want[1])), (i, bad)
            out0.zero_()
        # ---- set_split_weights: a wrong count leaves the arithmetic as it was
        split = [t.data_ptr() for t in eng.split]
        for bad_n in (len(split) - 1, len(split) + 1, 0):
            assert lib.mftx_encoder_set_split_weights(eng._h, _lib.ptr_array(split)[0], bad_n) == E_ARG
        p = list(split)
        p[2] = None
        assert lib.mftx_encoder_set_split_weights(eng._h, _lib.ptr_array(p)[0], len(split)) == E_ALIGN
        assert lib.mftx_encoder_set_split_weights(None, _lib.ptr_array(split)[0], len(split)) == E_STATE
        assert _same_bits(eng.forward(img), want)
        # ---- a destroyed handle
        assert lib.mftx_encoder_create(_lib.ptr_array(ptrs)[0], n, int(inorm), C.byref(handle)) == 0 and handle.value
        lib.mftx_encoder_destroy(handle)
        a = list(good)
        a[0] = handle
        assert lib.mftx_encoder_forward(*a) == E_STATE
        assert lib.mftx_encoder_set_graph(handle, 1) == E_STATE
        assert _same_bits(eng.forward(img), want)

    # ---- mftx_encoder_prep
    prep_want = ops.encoder_prep(img)
    prep = torch.zeros_like(prep_want)
    assert lib.mftx_encoder_prep(None, H, W, prep.data_ptr(), None) == E_ARG
    assert lib.mftx_encoder_prep(img.data_ptr(), H, W, None, None) == E_ARG
    assert lib.mftx_encoder_prep(img.data_ptr(), 0, W, prep.data_ptr(), None) == E_ARG
    assert lib.mftx_encoder_prep(img.data_ptr(), H, -1, prep.data_ptr(), None) == E_ARG
    assert lib.mftx_encoder_prep(img.data_ptr(), H, W, prep.data_ptr() + 4, None) == E_ALIGN
    assert not prep.any()
    assert lib.mftx_encoder_prep(img.data_ptr(), H, W, prep.data_ptr(), None) == 0 and torch.equal(prep, prep_want)

    # ---- mftx_instance_norm
    rows, Cc = 37, 96
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(rows + 1, Cc, generator=g).to(DEV)
    res = torch.randn(rows + 1, Cc, generator=g).to(DEV)
    want = ops.instance_norm(x0[:rows].clone(), 1, res[:rows].clone())
    need = lib.mftx_instance_norm_workspace_bytes(Cc)
    assert need >= 256 * Cc * 16 + Cc * 8
    for bad_c in (0, 4, 60, 100, 264, 512, -8):
        assert lib.mftx_instance_norm_workspace_bytes(bad_c) == 0, bad_c
    ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
    x = x0.clone()
    good = [x.data_ptr(), rows, Cc, res.data_ptr(), 1, 0, ws.data_ptr(), need, None]
    cases = [(0, None, E_ARG), (6, None, E_ARG), (1, 0, E_ARG), (1, -3, E_ARG), (2, 100, E_ARG), (2, 4, E_ARG), (2, 0, E_ARG),
             (2, 264, E_ARG), (2, 512, E_ARG), (4, -1, E_ARG), (4, 3, E_ARG), (3, None, E_ARG),
             (0, x.data_ptr() + 4, E_ALIGN), (3, res.data_ptr() + 8, E_ALIGN), (6, ws.data_ptr() + 8, E_ALIGN),
             (7, need - 1, E_WORKSPACE), (7, 0, E_WORKSPACE)]
    for i, bad, code in cases:
        a = list(good)
        a[i] = bad
        assert lib.mftx_instance_norm(*a) == code, (i, bad, lib.mftx_last_error_string())
        assert torch.equal(x, x0), (i, bad, "a refused call wrote to x")
    # split form asks for 32-byte aligned maps: 16 is not enough (row 0 + 16 bytes)
    a = list(good)
    a[5] = 1
    a[0] = x.data_ptr() + 16
    assert lib.mftx_instance_norm(*a) == E_ALIGN
    a[0], a[3] = x.data_ptr(), res.data_ptr() + 16
    assert lib.mftx_instance_norm(*a) == E_ALIGN
    assert torch.equal(x, x0)
    # modes 0 and 2 take no residual map
    for mode in (0, 2):
        y = x0.clone()
        assert lib.mftx_instance_norm(y.data_ptr(), rows, Cc, None, mode, 0, ws.data_ptr(), need, None) == 0
        assert torch.equal(y[:rows], ops.instance_norm(x0[:rows].clone(), mode)) and torch.equal(y[rows], x0[rows])
    assert lib.mftx_instance_norm(*good) == 0
    assert torch.equal(x[:rows], want) and torch.equal(x[rows], x0[rows])
