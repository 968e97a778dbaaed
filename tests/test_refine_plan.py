"""CPU-only: the refinement's launch schedule (csrc/raft_engine.hip: RefinePlan) as ``mftx_raft_plan`` reports it, held to the
contracts that include/mftx.h and the engine's comments state.

The handles here stand on HOST buffers and nothing is launched: ``mftx_raft_create`` and every ``mftx_raft_set_*`` call check
their pointers for null / 16-byte alignment and store them -- none of them dereferences one or calls into HIP (an empty graph
cache has nothing to destroy), and ``mftx_raft_plan`` reads the handle only.  Without a device the library takes the chip to
have 256 CUs, the number an MI355X reports, so the one size-dependent decision (``tile_conv = 1``) reads the same on both."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SPLIT, F32 = "split", "f32"
# enum WeightSlot of csrc/raft_engine.hip, as far as the tests name slots (the same numbering as ops.RaftEngine.TILE_SLOTS / GEMM_SLOTS)
W_CONVC2, W_CONV, W_ZR1_DYN, W_Q1_DYN, W_ZR2_DYN, W_Q2_DYN = 2, 8, 10, 13, 16, 19
GRU_TILE_SLOTS = (W_ZR1_DYN, W_Q1_DYN, W_ZR2_DYN, W_Q2_DYN)


@pytest.fixture(scope="module")
def ops_mod():
    if not (REPO / "mft_amd" / "libmftx.so").exists():
        subprocess.run(["make", "-C", str(REPO / "mft_amd" / "csrc"), "-j8"], check=True, capture_output=True)
    from mft_amd import _lib, ops
    _lib.load()
    return ops


class Handle:
    """A ``RaftEngine`` over host memory: only what ``plan`` / ``set_option`` need (the handle), none of its device state."""

    def __init__(self, ops, arith=SPLIT, options=None, drop_tile=(), ondemand=False, trace=False):
        from mft_amd import _lib
        self.lib = lib = _lib.load()
        n = _lib.NUM_RAFT_WEIGHTS
        self.buf = C.create_string_buffer(64 * (n + 8) + 16)
        base = (C.addressof(self.buf) + 15) & ~15
        ptrs = [base + 64 * i for i in range(n + 8)]          # 16-byte aligned host addresses, one per weight / stream
        arr, self.keep = _lib.ptr_array(ptrs[:n])
        h = C.c_void_p()
        assert lib.mftx_raft_create(arr, n, C.byref(h)) == 0
        self.eng = ops.RaftEngine.__new__(ops.RaftEngine)     # (its __del__ destroys the handle)
        self.eng._h = h
        if arith == SPLIT:
            sarr, self.keep_s = _lib.ptr_array([p if i in ops.RaftEngine.GEMM_SLOTS else None for i, p in enumerate(ptrs[:n])])
            assert lib.mftx_raft_set_split_weights(h, sarr, n) == 0
        # every weight stream, whatever the arithmetic: fp32 MFMA must ignore them
        tarr, self.keep_t = _lib.ptr_array([p if i in ops.RaftEngine.TILE_SLOTS and i not in drop_tile else None
                                            for i, p in enumerate(ptrs[:n])])
        assert lib.mftx_raft_set_tile_weights(h, tarr, n) == 0
        assert lib.mftx_raft_set_lookup_fused(h, ptrs[n]) == 0
        assert lib.mftx_raft_set_flow_fused(h, ptrs[n + 1]) == 0
        assert lib.mftx_raft_set_flow_head(h, ptrs[n + 2]) == 0
        assert lib.mftx_raft_set_ou_heads(h, ptrs[n + 3], ptrs[n + 4]) == 0
        for k, v in dict({"tile_conv": 2}, **(options or {})).items():
            self.eng.set_option(k, v)
        if ondemand:
            assert lib.mftx_raft_set_ondemand(h, 1) == 0
        if trace:
            assert lib.mftx_raft_set_coords_trace(h, ptrs[n + 5]) == 0

    def plan(self, P=2, h=24, w=40, ctx_supplied=False):
        return self.eng.plan(P, h, w, ctx_supplied)


def plan(ops, arith=SPLIT, options=None, shape=(2, 24, 40), ctx_supplied=False, **kw):
    return Handle(ops, arith, options, **kw).plan(*shape, ctx_supplied=ctx_supplied)


def test_defaults_run_everything_fused(ops_mod):
    p = plan(ops_mod)
    assert p == {"presplit": True, "fuse_lookup": True, "tiles_on": True, "gru_fused": True, "ctx_supplied": False, "two_pass": True,
                 "flow": "fused", "pair_second": False, "head_fused": True, "defer_update": True, "ou_fused": True,
                 "ou_materialised": False, "use_graph": True, "side_stream": True}
    # fp32 MFMA: none of the split-arithmetic kernels whatever streams are set; round 1's grouped launches, under the graph
    p = plan(ops_mod, F32)
    assert p == {"presplit": False, "fuse_lookup": False, "tiles_on": False, "gru_fused": False, "ctx_supplied": False, "two_pass": False,
                 "flow": "with_lookup", "pair_second": True, "head_fused": False, "defer_update": False, "ou_fused": False,
                 "ou_materialised": True, "use_graph": True, "side_stream": False}
    # split arithmetic with fp32 activations (presplit = 0) has no split-form tensors for those kernels to read either
    p = plan(ops_mod, options={"presplit": 0})
    assert not any(p[k] for k in ("presplit", "fuse_lookup", "tiles_on", "gru_fused", "two_pass", "head_fused", "ou_fused"))
    assert p["flow"] == "side" and not p["pair_second"]


@pytest.mark.parametrize("missing", GRU_TILE_SLOTS)
def test_one_missing_gru_stream_unfuses_both_passes(ops_mod, missing):
    """One fused and one unfused pass would read a buffer the other never wrote: ONE decision for both."""
    assert missing in ops_mod.RaftEngine.TILE_SLOTS and ops_mod.RaftEngine.TILE_SLOTS[missing][1] == 256      # (a gate over [h | motion])
    p = plan(ops_mod, drop_tile=(missing,), ctx_supplied=True)
    assert p["tiles_on"] and not p["gru_fused"] and not p["ctx_supplied"]


def test_supplied_context_parts_need_the_fused_gru(ops_mod):
    assert plan(ops_mod, ctx_supplied=True)["ctx_supplied"]
    assert not plan(ops_mod, ctx_supplied=False)["ctx_supplied"]
    for options in ({"fuse_gru": 0}, {"tile_conv": 0}, {"presplit": 0}):
        p = plan(ops_mod, options=options, ctx_supplied=True)
        assert not p["gru_fused"] and not p["ctx_supplied"], options
    assert not plan(ops_mod, F32, ctx_supplied=True)["ctx_supplied"]


@pytest.mark.parametrize("arith", (SPLIT, F32))
def test_group_0_is_one_launch_per_layer(ops_mod, arith):
    for fork in (-1, 0, 1, 2):
        for fuse_lookup in (0, 1):
            p = plan(ops_mod, arith, {"group": 0, "fork": fork, "fuse_lookup": fuse_lookup})
            assert p["flow"] == "after_lookup" and not p["pair_second"], (fork, fuse_lookup)


def test_fp32_is_never_forked_and_grouped_only_with_group_1(ops_mod):
    for fork in (-1, 0, 1, 2):
        for group in (0, 1):
            p = plan(ops_mod, F32, {"fork": fork, "group": group, "fuse_flow": 0})
            assert not p["side_stream"], (fork, group)
            assert p["flow"] == ("with_lookup" if group else "after_lookup"), (fork, group)
            assert p["pair_second"] == bool(group), (fork, group)


def test_fork_option_with_the_split_arithmetic(ops_mod):
    flow = lambda **o: plan(ops_mod, options=dict({"fuse_flow": 0}, **o))["flow"]       # noqa: E731
    assert flow() == flow(fork=1) == "side"
    assert flow(fuse_lookup=0) == flow(fork=1, fuse_lookup=0) == "side"
    # 0 and 2: in order on one stream -- after the fused lookup, or grouped with the plain one
    assert flow(fork=0) == "after_lookup" and flow(fork=0, fuse_lookup=0) == "with_lookup"
    # 2 means "flow branch first" with the fused lookup only
    assert flow(fork=2) == "first" and flow(fork=2, fuse_lookup=0) == "with_lookup"
    # the fused flow branch needs no stream of its own whatever the option says
    for fork in (-1, 0, 1, 2):
        assert plan(ops_mod, options={"fork": fork})["flow"] == "fused"
    assert not plan(ops_mod, options={"fuse_flow": 0, "fork": 0})["pair_second"]


def test_profiler_runs_everything_in_order(ops_mod):
    from mft_amd import _lib
    lib = _lib.load()
    split, f32 = Handle(ops_mod, options={"fuse_flow": 0, "fuse_lookup": 0}), Handle(ops_mod, F32)
    assert split.plan()["flow"] == "side" and f32.plan()["flow"] == "with_lookup"
    lib.mftx_profile_begin()              # (no launch has been bracketed: begin and end touch no device)
    try:
        ps, pf = split.plan(), f32.plan()
    finally:
        lib.mftx_profile_end(None, None, None, 0)
    assert ps["flow"] == "after_lookup" and not ps["use_graph"]
    assert pf["flow"] == "after_lookup" and not pf["use_graph"]
    assert split.plan()["flow"] == "side" and split.plan()["use_graph"]


@pytest.mark.parametrize("arith", (SPLIT, F32))
def test_ondemand_has_no_fused_lookup_no_graph_and_its_own_lookup_launch(ops_mod, arith):
    for options in ({}, {"fuse_flow": 0}, {"fuse_flow": 0, "fork": 0}, {"fuse_flow": 0, "fork": 2}):
        p = plan(ops_mod, arith, options, ondemand=True)
        assert not p["fuse_lookup"] and not p["use_graph"] and p["flow"] not in ("with_lookup", "first"), options
    assert plan(ops_mod, SPLIT, {"fuse_flow": 0, "fork": 0}, ondemand=True)["flow"] == "after_lookup"


def test_fuse_head_2_and_a_trace_never_defer(ops_mod):
    p = plan(ops_mod, options={"fuse_head": 2})
    assert p["head_fused"] and p["flow"] == "fused" and not p["defer_update"]
    p = plan(ops_mod, trace=True)
    assert p["head_fused"] and p["flow"] == "fused" and not p["defer_update"] and not p["use_graph"]
    assert not plan(ops_mod, F32, trace=True)["use_graph"]
    # nothing to defer to without the fused flow branch, nothing to defer without the fused head
    assert not plan(ops_mod, options={"fuse_flow": 0})["defer_update"]
    p = plan(ops_mod, options={"fuse_head": 0})
    assert not p["head_fused"] and not p["defer_update"]


def test_fuse_ou_2_materialises_the_input(ops_mod):
    p = plan(ops_mod, options={"fuse_ou": 2})
    assert p["ou_fused"] and p["ou_materialised"]
    p = plan(ops_mod, options={"fuse_ou": 0})
    assert not p["ou_fused"] and p["ou_materialised"]
    p = plan(ops_mod, F32, {"fuse_ou": 2})
    assert not p["ou_fused"] and p["ou_materialised"]


def test_tile_conv_1_follows_the_batch(ops_mod):
    """7 pairs of 64 x 64 cells: 224 tiles of 128 cells per kernel shape on 256 CUs, at least 5/8 of a round; one pair of 32 x 32: 8."""
    h = Handle(ops_mod, options={"tile_conv": 1})
    big, small = h.plan(7, 64, 64), h.plan(1, 32, 32)
    assert big["tiles_on"] and big["gru_fused"] and big["two_pass"] and big["head_fused"] and big["ou_fused"]
    assert not any(small[k] for k in ("tiles_on", "gru_fused", "two_pass", "head_fused", "ou_fused"))
    assert small["fuse_lookup"] and small["flow"] == "fused"          # (these two are no tile-resident layers)
    assert not Handle(ops_mod, F32, {"tile_conv": 1}).plan(7, 64, 64)["tiles_on"]
    assert not Handle(ops_mod, options={"tile_conv": 0}).plan(7, 64, 64)["tiles_on"]


def test_graph_option_and_two_pass_option(ops_mod):
    assert not plan(ops_mod, options={"graph": 0})["use_graph"]
    assert not plan(ops_mod, options={"tile_conv2p": 0})["two_pass"]
    assert not plan(ops_mod, drop_tile=(W_CONVC2,))["two_pass"] and not plan(ops_mod, drop_tile=(W_CONV,))["two_pass"]


def test_argument_errors(ops_mod):
    from mft_amd._lib import MftxError
    h = Handle(ops_mod)
    assert h.lib.mftx_raft_set_option(h.eng._h, 13, 1) != 0 and h.lib.mftx_raft_set_option(h.eng._h, -1, 1) != 0
    with pytest.raises(MftxError):
        h.eng.set_option("no_such_option", 1)
    out = (C.c_int * 14)()
    assert h.lib.mftx_raft_plan(h.eng._h, 2, 24, 40, 0, out, 13) != 0
    assert h.lib.mftx_raft_plan(h.eng._h, 0, 24, 40, 0, out, 14) != 0
    assert h.lib.mftx_raft_plan(None, 2, 24, 40, 0, out, 14) != 0
    assert h.lib.mftx_raft_plan(h.eng._h, 2, 24, 40, 0, out, 14) == 0
