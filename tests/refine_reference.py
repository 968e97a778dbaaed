"""Reference side of the refinement-engine tests (tests/test_refine_reference.py on the CPU, tests/test_gpu_refine_family.py on the
GPU): seeded cases, the fp32 and the fp64 oracle run of each with every stage the engine materialises (``O.raft_refine``'s trace),
the table that says which workspace region of ``RaftEngine.REGIONS`` equals which trace entry and on which schedules, the
comparison, and -- for the CPU self-tests -- seeded faults and a second fp32 realisation with permuted channels.

Bounds (both test files): error against fp64 <= K_MAX x the fp32 oracle's maximum error and <= K_MEAN x its mean error, per region;
for regions the engine stores in split form the representation error SPLIT_REP |ref| + SPLIT_FLOOR is taken off first."""
import contextlib
import functools
import os
from collections import namedtuple

import numpy as np
import torch

import corr_reference as cr
from oracle import mft_oracle as O
from test_gpu_encoder import SPLIT_FLOOR, SPLIT_REP, _ratio
from test_gpu_offgrid import K_MAX, K_MEAN

WEIGHT_SEED = 7

Case = namedtuple("Case", "P h w kind init")
Case.__str__ = lambda c: f"{c.P}x{c.h}x{c.w}-{c.kind}-{c.init or 'none'}"      # noqa: E731

# (1, 16, 16): the smallest legal size, level 3 of the pyramid is 2 x 2, smaller than any tile; (2, 17, 23): both odd, two pairs, odd
# pooled sizes; (3, 24, 40): the shape of the cross-schedule tests, ragged tiles both ways; (1, 33, 47): several tiles both ways, odd
# everywhere; (1, 16, 70) / (1, 70, 16): longer than a tile along the 1 x 5 / the 5 x 1 pass
SHAPES = [(1, 16, 16), (2, 17, 23), (3, 24, 40), (1, 33, 47), (1, 16, 70), (1, 70, 16)]
VARIED = [(2, 17, 23), (1, 33, 47)]                    # the shapes every input kind and every flow_init kind runs on
KINDS = ("rand", "same", "zero", "hot")
INITS = (None, "far", "quarter")
CASES = ([Case(*s, "rand", None) for s in SHAPES] + [Case(*s, k, None) for s in VARIED for k in KINDS[1:]]
         + [Case(*s, "rand", i) for s in VARIED for i in INITS[1:]])
ITERS = (1, 2, 3, 12)
FORCED_K = (1, 2, 6, 12)


def threads():
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))


@functools.lru_cache(maxsize=None)
def weights():
    from mft_amd.weights import make_weights
    return {k: torch.from_numpy(v) for k, v in make_weights(WEIGHT_SEED).items()}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Pixel-major fp32 CPU tensors of a case: f1, f2 [P, N, 256], net, inp [P, N, 128], flow_init [P, N, 2] or None.  Read-only.
    rand: the inputs of test_gpu_kernels._engine_outputs (same generator, same order) at the case's shape."""
    P, N = case.P, case.h * case.w
    g = torch.Generator().manual_seed(11)
    f1 = torch.randn(P, N, 256, generator=g)
    f2 = f1 + 0.3 * torch.randn(P, N, 256, generator=g)
    net = torch.tanh(torch.randn(P, N, 128, generator=g))
    inp = torch.relu(torch.randn(P, N, 128, generator=g))
    if case.kind == "same":
        f2 = f1.clone()
    elif case.kind == "zero":                          # the correlation is exactly 0
        f1, f2 = torch.zeros_like(f1), torch.zeros_like(f1)
    elif case.kind == "hot":                           # saturated gates
        net = torch.where(net >= 0, torch.tensor(0.999), torch.tensor(-0.999))
        inp = inp * 8
    elif case.kind != "rand":
        raise ValueError(case.kind)
    g = torch.Generator().manual_seed(23)
    if case.init is None:
        init = None
    elif case.init == "far":                           # most windows partly or wholly off the map at some level
        init = (torch.rand(P, N, 2, generator=g) * 2 - 1) * 40
    elif case.init == "quarter":                       # multiples of 1/4; every third cell a whole number
        init = torch.round(torch.randn(P, N, 2, generator=g) * 12) / 4
        init[:, ::3] = torch.round(init[:, ::3])
    else:
        raise ValueError(case.init)
    return dict(f1=f1, f2=f2, net=net, inp=inp, flow_init=init)


# ---------------------------------------------------------------------------------------------------------------------------
# the region table
# ---------------------------------------------------------------------------------------------------------------------------
# region: a name of RaftEngine.REGIONS, or None for what comes back from refine() (flow_lr and the three outputs)
# lo, hi: the region's columns; key: the entry of the trace's last dict (trace_regions) it equals
# when: plan -> bool, the schedules on which the region holds that after a call (ALWAYS: every schedule)
# split: stored in split form where the plan keeps activations so (plan["presplit"])
Region = namedtuple("Region", "region lo hi key when split")
ALWAYS = None
REGION_MAP = {           # in pipeline order (the order "first region to trip" refers to)
    "corr":    Region("corr", 0, 324, "corr", ALWAYS, False),
    "cor1":    Region("cor1", 0, 256, "cor1", ALWAYS, True),
    "flo1":    Region("flo1", 0, 128, "flo1", lambda p: p["flow"] != "fused", True),        # (fused: never stored; the other coords buffer)
    "corflo":  Region("corflo", 0, 256, "corflo", ALWAYS, True),
    "motion":  Region("hx", 256, 384, "motion", ALWAYS, True),
    "inp":     Region("hx", 128, 256, "inp", ALWAYS, True),
    "z":       Region("z", 0, 128, "z", lambda p: not p["gru_fused"], False),               # the vertical pass's, both from its gate GEMM's epilogue
    "rh":      Region("rh", 0, 128, "rh", lambda p: not p["gru_fused"], True),
    "h":       Region("hx", 0, 128, "net", ALWAYS, True),
    "delta":   Region("delta", 0, 2, "delta", ALWAYS, False),
    "coords1": Region("coords1", 0, 2, "coords1", ALWAYS, False),
    "fh":      Region("fh", 0, 256, "mask_hidden", ALWAYS, True),                           # (the flow head's hidden layer until the mask head's replaces it)
    "mask":    Region("mask", 0, 576, "mask", ALWAYS, False),
    "ouin":    Region("ouin", 0, 712, "ou_input", lambda p: p["ou_materialised"], True),
    "ouh":     Region("ouh", 0, 256, "ou_hidden", lambda p: not p["ou_fused"], False),      # (fused: the projection's partial sums)
    "ou":      Region("ou", 0, 3, "ou", ALWAYS, False),
    "flow_lr": Region(None, 0, 2, "flow_lr", ALWAYS, False),
}
ROW_WIDTH = {"hx": 384, "ou": 4}                       # floats per cell where a region's row is wider than the columns listed (RaftEngine.region's cols)
OUTPUTS = ("flow", "occl", "sigma")
ALWAYS_VALID = tuple(k for k, r in REGION_MAP.items() if r.when is ALWAYS)


def valid_regions(plan):
    return [k for k, r in REGION_MAP.items() if r.when is ALWAYS or r.when(plan)]


# ---------------------------------------------------------------------------------------------------------------------------
# oracle runs
# ---------------------------------------------------------------------------------------------------------------------------
KEEP_EARLY = ("net", "coords1", "delta")               # what is kept of the iterations before the last (teacher forcing, drift)


def _nchw(t, h, w):
    return t.reshape(h, w, -1).permute(2, 0, 1)[None].contiguous()


def _pmaj(t):
    return t[0].permute(1, 2, 0).reshape(t.shape[-2] * t.shape[-1], -1)


def run_oracle(sd, data, P, h, w, iters, dtype, refine=None, unperm=None):
    """The oracle in `dtype` over the P pairs of `data` (as `inputs` returns) -> {"trace": [per iteration {key: [P h w, C]}], "flow":
    [P, 2, 8h, 8w], "occl", "sigma": [P, 1, 8h, 8w]}; the last iteration's dict holds every key of REGION_MAP (plus "ou" = the
    occlusion and uncertainty logits side by side, "inp"), the earlier ones KEEP_EARLY.  refine: a stand-in for O.raft_refine (the
    seeded faults); unperm: {key: column index} applied to a trace entry (the permuted realisation)."""
    threads()
    refine = refine or O.raft_refine
    traces, outs = [], []
    ctx = O.precision(dtype) if dtype != torch.float32 else contextlib.nullcontext()
    with ctx, torch.no_grad():
        sdt = O.cast_weights(sd, dtype)
        for p in range(P):
            a = {k: _nchw(v[p].to(dtype), h, w) for k, v in data.items() if v is not None}
            tr = []
            pred = refine(sdt, a["f1"], a["f2"], a["net"], a["inp"], iters, flow_init=a.get("flow_init"), trace=tr)
            assert len(tr) == iters
            tr[-1]["ou"] = torch.cat([tr[-1]["occl"], tr[-1]["unc"]], 1)
            tr[-1]["inp"] = a["inp"]
            tr = [{k: _pmaj(v) for k, v in d.items() if i == iters - 1 or k in KEEP_EARLY} for i, d in enumerate(tr)]
            traces.append(tr)
            outs.append(O.postprocess(pred, 8 * h, 8 * w))
    trace = [{k: torch.cat([t[i][k] for t in traces]) for k in traces[0][i]} for i in range(iters)]
    for k, idx in (unperm or {}).items():
        for d in trace:
            if k in d:
                d[k] = d[k][:, idx]
    out = {"trace": trace}
    for j, k in enumerate(OUTPUTS):
        out[k] = torch.stack([o[j] for o in outs])
    return out


@functools.lru_cache(maxsize=10)
def reference(case, iters):
    """(fp32 run, fp64 run) of a case, computed once (the cache holds the last ten: tests are ordered case by case)."""
    data = inputs(case)
    return tuple(run_oracle(weights(), data, case.P, case.h, case.w, iters, dt) for dt in (torch.float32, torch.float64))


def forced_state(case, k):
    """The state iteration k of the fp64 run starts from, rounded to fp32: `inputs(case)` with net and flow_init replaced."""
    data = dict(inputs(case))
    if k > 1:
        prev = reference(case, k)[1]["trace"][k - 2]
        N = case.h * case.w
        grid = torch.stack([torch.arange(N) % case.w, torch.arange(N) // case.w], 1).double().repeat(case.P, 1)
        data["net"] = prev["net"].float().reshape(case.P, N, 128)
        data["flow_init"] = (prev["coords1"] - grid).float().reshape(case.P, N, 2)
    return data


@functools.lru_cache(maxsize=4)
def reference_forced(case, k):
    """Teacher forcing: (the fp32 oracle's ONE iteration from `forced_state(case, k)`, the fp64 run's iteration k) -- the one-step
    noise, and the target, of an engine started from the same state."""
    r64 = reference(case, k)[1]
    r32 = run_oracle(weights(), forced_state(case, k), case.P, case.h, case.w, 1, torch.float32)
    return r32, r64


def region_tensors(run):
    """A run -> {name of REGION_MAP or OUTPUTS: tensor}: the last iteration's entries under the table's names."""
    last = run["trace"][-1]
    out = {name: last[r.key] for name, r in REGION_MAP.items()}
    out.update({k: run[k] for k in OUTPUTS})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------
def compare(got, r32, r64, split_region=False):
    """-> (max error, mean error of `got` against fp64, max error, mean error of the fp32 oracle against fp64: the noise).
    split_region: `got` was decoded from the engine's split form -- its representation error SPLIT_REP |ref| + SPLIT_FLOOR does not
    count."""
    ref = r64.double()
    err = (got.double().reshape(ref.shape) - ref).abs()
    if split_region:
        err = (err - (SPLIT_REP * ref.abs() + SPLIT_FLOOR)).clamp_min(0)
    noise = (r32.double() - ref).abs()
    return float(err.max()), float(err.mean()), float(noise.max()), float(noise.mean())


# Raised bounds (K_MAX, K_MEAN), each with its reason; never above 16, never from what the engine gives.
#   ouh with the fp32 MFMA arithmetic -- the OU heads' first layer is the longest sum of the engine: 9 taps x 712 channels = 6408 terms
#   per output.  The fp32 MFMA GEMM adds them one after the other into one fp32 accumulator; the fp32 reference (torch on the CPU) adds
#   them in blocks, whose error grows with the square root of the block length, not of 6408.  `sequential_ou_hidden` is that
#   one-accumulator sum on the CPU, fed the fp32 oracle's own input: where this was written it reached 7.4 x the noise in the maximum
#   and 4.06 x in the mean (saturated gates, one iteration; tests/test_refine_reference.py prints it) -- a correct sequential fp32 sum
#   has no margin under 8 and 4 there.  Twice the constants, for this region in this arithmetic only: the split arithmetic (products
#   exact to 2^-23, the same accumulator) was never the reason and stays at 8 and 4, as do the heads' outputs (ou, occl, sigma).
BOUNDS_FP32_ARITH = {"ouh": (16.0, 8.0)}


def bound(name, fp32_arith=False):
    """(K_MAX, K_MEAN) of a region or output; fp32_arith: the engine runs the fp32 MFMA arithmetic (ARITH_F32)."""
    return BOUNDS_FP32_ARITH.get(name, (K_MAX, K_MEAN)) if fp32_arith else (K_MAX, K_MEAN)


def within(stats, k_max=K_MAX, k_mean=K_MEAN):
    """The bound on what `compare` returns; zero noise demands zero error.  NaN fails."""
    emax, emean, nmax, nmean = stats
    return emax <= k_max * nmax and emean <= k_mean * nmean


def sequential_ou_hidden(run32, P, h, w):
    """relu(conv1) of both OU heads from the run's own 712-channel input, every output summed term by term into one fp32 accumulator
    (taps outermost, product rounded, then added): an independent fp32 realisation of the layer with the summation order of a
    plain GEMM K loop -> [P h w, 256]."""
    sd = weights()
    o = "occlusion_block."
    W = torch.cat([sd[o + "occl_head.conv1.weight"], sd[o + "uncertainty_head.conv1.weight"]], 0)      # [256, 712, 3, 3]
    b = torch.cat([sd[o + "occl_head.conv1.bias"], sd[o + "uncertainty_head.conv1.bias"]])
    x = torch.nn.functional.pad(run32["trace"][-1]["ou_input"].float().reshape(P, h, w, 712), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(P, h, w, 256)
    for ky in range(3):
        for kx in range(3):
            xs = x[:, ky:ky + h, kx:kx + w]
            for c in range(712):
                acc = acc + xs[..., c:c + 1] * W[:, c, ky, kx]
    return torch.relu(acc + b).reshape(-1, 256)


def line(tag, name, stats, k_max=K_MAX, k_mean=K_MEAN):
    emax, emean, nmax, nmean = stats
    return (f"refine-noise {tag} {name:8s} max hip/fp64 {emax:.3e} fp32/fp64 {nmax:.3e} ratio {_ratio(emax, nmax):6.2f} (bound {k_max:g})  "
            f"mean hip/fp64 {emean:.3e} fp32/fp64 {nmean:.3e} ratio {_ratio(emean, nmean):6.2f} (bound {k_mean:g})")


def inp_bits_ok(got, inp, split):
    """hx[:, 128:256] holds the caller's inp: its bits, or -- in split form -- its split round trip."""
    want = inp.reshape(got.shape)
    if split:
        want = torch.from_numpy(cr.split_roundtrip(want.numpy()).astype(np.float32))
    return torch.equal(got.float(), want.float())


# ---------------------------------------------------------------------------------------------------------------------------
# seeded faults (fp32 oracle only: tests/test_refine_reference.py shows that every one is caught)
# ---------------------------------------------------------------------------------------------------------------------------
def _loop(sd, fmap1, fmap2, net, inp, iters, flow_init=None, trace=None, stale=False, twice=False, fp16_at=None):
    """O.raft_refine restated around O's own stages (bit for bit equal without a fault: test_loop_restatement_equals_the_oracle), with
    the three faults that live in the loop itself."""
    _, _, h, w = fmap1.shape
    pyr = O.corr_pyramid(O.corr_volume(fmap1, fmap2))
    coords0 = O.pixel_grid(h, w)[None]
    coords1 = coords0.clone()
    if flow_init is not None:
        coords1 = coords1 + flow_init
    pending = torch.zeros_like(coords1)
    for itr in range(iters):
        if fp16_at == itr:
            net = net.half().to(net.dtype)
        corr = O.corr_lookup(pyr, coords1)
        flow = coords1 - coords0
        rec = {}
        net, mask, delta, motion = O.update_block(sd, net, inp, corr, flow, rec)
        if stale:                                       # the update of iteration k arrives at iteration k + 1
            coords1, pending = coords1 + pending, delta
        else:
            coords1 = coords1 + delta
        if twice and itr == iters - 1:
            coords1 = coords1 + delta
        rec.update(corr=corr, motion=motion, net=net, delta=delta, coords1=coords1)
        trace.append(rec)
    flow_lr = coords1 - coords0
    occl, unc = O.ou_block(sd, net, inp, corr, flow_lr, delta, motion, trace[-1])
    trace[-1].update(mask=mask, occl=occl, unc=unc, flow_lr=flow_lr)
    return dict(flow=O.convex_upsample(flow_lr, mask, 8.0), occlusion=O.convex_upsample(occl, mask, 1.0),
                uncertainty=O.convex_upsample(unc, mask, 1.0), coords=flow_lr)


@contextlib.contextmanager
def _patched(name, make):
    """The oracle's stage `name` wrapped by make(original) for the length of the block (the callers look it up in the module)."""
    orig = getattr(O, name)
    setattr(O, name, make(orig))
    try:
        yield
    finally:
        setattr(O, name, orig)


def _swap(sd, a, b):
    sd = dict(sd)
    for s in (".weight", ".bias"):
        sd[a + s], sd[b + s] = sd[b + s], sd[a + s]
    return sd


def _with_sd(edit):
    return lambda sd, *a, **kw: O.raft_refine(edit(dict(sd)), *a, **kw)


def _fault_taps(sd):
    for g in "zrq":
        sd[f"update_block.gru.conv{g}1.weight"] = sd[f"update_block.gru.conv{g}1.weight"].flip(-1)
        sd[f"update_block.gru.conv{g}2.weight"] = sd[f"update_block.gru.conv{g}2.weight"].flip(-2)
    return sd


def _fault_q2(sd):
    for s in (".weight", ".bias"):
        t = sd["update_block.gru.convq2" + s].clone()
        t[37] = 0
        sd["update_block.gru.convq2" + s] = t
    return sd


def _fault_mask(sd):
    for s in (".weight", ".bias"):
        sd["update_block.mask.2" + s] = sd["update_block.mask.2" + s] * 4
    return sd


def _fault_unc(sd):
    for s in (".weight", ".bias"):
        sd["occlusion_block.uncertainty_head.conv1" + s] = sd["occlusion_block.occl_head.conv1" + s]
    return sd


def _fault_motion(sd, *a, **kw):
    def make(orig):
        def motion_encoder(*b, **k):
            m = orig(*b, **k)
            return torch.cat([m[:, :126], m[:, 127:128], m[:, 126:127]], 1)
        return motion_encoder
    with _patched("motion_encoder", make):
        return O.raft_refine(sd, *a, **kw)


def _fault_levels(sd, *a, **kw):
    def make(orig):
        def corr_lookup(*b, **k):
            c = orig(*b, **k)
            return torch.cat([c[:, :162], c[:, 243:324], c[:, 162:243]], 1)
        return corr_lookup
    with _patched("corr_lookup", make):
        return O.raft_refine(sd, *a, **kw)


def _fault_convf1(sd, *a, **kw):
    def make(orig):
        def _conv(x, sd_, name, padding):
            if name.endswith(".convf1"):
                x = x.clone()
                x[..., -1] = 0
            return orig(x, sd_, name, padding)
        return _conv
    with _patched("_conv", make):
        return O.raft_refine(sd, *a, **kw)


# name -> a stand-in for O.raft_refine.  ("between iterations" at one iteration: net is rounded where the only iteration starts.)
FAULTS = {
    "z and r gates exchanged in the vertical pass": _with_sd(lambda sd: _swap(sd, "update_block.gru.convz2", "update_block.gru.convr2")),
    "1x5 and 5x1 taps reversed": _with_sd(_fault_taps),
    "one output channel of convq2 zeroed": _with_sd(_fault_q2),
    "delta of iteration k applied at iteration k+1": lambda *a, **kw: _loop(*a, stale=True, **kw),
    "delta applied twice on the last iteration": lambda *a, **kw: _loop(*a, twice=True, **kw),
    "motion channels 126 and 127 exchanged": _fault_motion,
    "the mask's 0.25 omitted": _with_sd(_fault_mask),
    "pyramid levels 2 and 3 exchanged in the lookup": _fault_levels,
    "last column zero-padded one cell early in convf1": _fault_convf1,
    "uncertainty head fed the occlusion head's hidden channels": _with_sd(_fault_unc),
    "net rounded to fp16 once between iterations": lambda sd, f1, f2, net, inp, iters, **kw: _loop(sd, f1, f2, net, inp, iters, fp16_at=min(1, iters - 1), **kw),
}


# ---------------------------------------------------------------------------------------------------------------------------
# the same mathematics in another summation order
# ---------------------------------------------------------------------------------------------------------------------------
def permuted_realisation(sd, data, seed=3):
    """-> (state dict, inputs, unperm): the input channels of convc2, conv, the twelve GRU convolutions, both head first layers and
    the OU heads' first layers permuted, each together with the layer (or the caller's map) that produces them.  unperm: for
    run_oracle, it brings the trace back to the original channel order."""
    g = torch.Generator().manual_seed(seed)
    rp = lambda n: torch.randperm(n, generator=g)      # noqa: E731
    pc1, pcor, pflo, pm, ph, pi = rp(256), rp(192), rp(64), rp(126), rp(128), rp(128)
    pcf = torch.cat([pcor, 192 + pflo])
    pm128 = torch.cat([pm, torch.tensor([126, 127])])
    gru_in = torch.cat([ph, 128 + pi, 256 + pm128])
    ou_in = torch.cat([ph, 128 + pi, 256 + torch.arange(328), 584 + pm128])
    sd = dict(sd)

    def perm(name, out=None, cin=None):
        w_, b_ = sd[name + ".weight"], sd[name + ".bias"]
        if out is not None:
            w_, b_ = w_[out], b_[out]
        if cin is not None:
            w_ = w_[:, cin]
        sd[name + ".weight"], sd[name + ".bias"] = w_.contiguous(), b_.contiguous()

    e, u, o = "update_block.encoder.", "update_block.", "occlusion_block."
    perm(e + "convc1", out=pc1)
    perm(e + "convc2", out=pcor, cin=pc1)
    perm(e + "convf2", out=pflo)
    perm(e + "conv", out=pm, cin=pcf)
    for gate in "zrq":
        for sfx in "12":
            perm(f"{u}gru.conv{gate}{sfx}", out=ph, cin=gru_in)
    perm(u + "flow_head.conv1", cin=ph)
    perm(u + "mask.0", cin=ph)
    perm(o + "occl_head.conv1", cin=ou_in)
    perm(o + "uncertainty_head.conv1", cin=ou_in)
    data = dict(data, net=data["net"][..., ph].contiguous(), inp=data["inp"][..., pi].contiguous())
    inv = torch.argsort
    unperm = {"cor1": inv(pc1), "corflo": inv(pcf), "motion": inv(pm128), "h_horizontal": inv(ph), "net": inv(ph), "z": inv(ph),
              "rh": inv(ph), "inp": inv(pi), "ou_input": inv(ou_in)}
    return sd, data, unperm
