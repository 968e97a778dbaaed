"""FlowOUTrackingResult's point-query and warping methods against outputs of the reference's own
methods on seeded inputs (tests/golden/results_api.npz, tools/make_goldens.py results).  The torch
paths (warp_forward, sample, warp_forward_points, invalid_mask) run anywhere; warp_backward is a HIP
kernel and is checked in the gpu-marked test."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from mft_amd.results import FlowOUTrackingResult


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "results_api.npz")


def make(device="cpu"):
    d = gi.results_api_inputs()
    T = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
    return d, FlowOUTrackingResult(T(d["flow"]), T(d["occl"]), T(d["sigma"]))


def test_warp_forward_matches_reference(g):
    d, res = make()
    out = res.warp_forward(d["img"])
    assert isinstance(out, np.ndarray) and out.shape == d["img"].shape
    assert np.allclose(out, g["warp_forward"], atol=1e-6)
    out = res.warp_forward(torch.from_numpy(d["img"]), mask=d["mask"], border=-1.0)
    assert np.allclose(out, g["warp_forward_masked"], atol=1e-6)
    assert (out == -1.0).any()                    # pixels nothing was splatted onto
    with pytest.raises(AssertionError):
        res.warp_forward(d["img"][:-1])


def test_point_queries_match_reference(g):
    d, res = make()
    assert np.allclose(res.warp_forward_points(d["pts"]).numpy(), g["warp_forward_points"], atol=1e-5)
    f, o, s = res.sample(torch.from_numpy(d["pts"]))
    assert np.allclose(f.numpy(), g["sample_flow"], atol=1e-5)
    assert np.allclose(o.numpy(), g["sample_occl"], atol=1e-6) and np.allclose(s.numpy(), g["sample_sigma"], atol=1e-6)
    assert np.array_equal(res.invalid_mask().numpy(), g["invalid_mask"]) and g["invalid_mask"].any()


@pytest.mark.gpu
def test_warp_backward_and_device_paths_match_reference(g):
    d, res = make("cuda")
    img = torch.from_numpy(d["img"]).permute(2, 0, 1).contiguous().cuda()
    assert np.allclose(res.warp_backward(img).cpu().numpy(), g["warp_backward"], atol=1e-5)
    assert np.allclose(res.warp_forward(d["img"]), g["warp_forward"], atol=1e-5)
    assert np.allclose(res.warp_forward_points(d["pts"]).cpu().numpy(), g["warp_forward_points"], atol=1e-5)


@pytest.mark.parametrize("H,W", [(125, 187), (127, 129), (130, 131), (129, 133), (121, 122), (128, 136), (1, 1), (3, 5)])
def test_pending_host_result_planes_start_on_16_bytes_at_any_size(H, W):
    """The host buffer of a PendingHostResult (what MFT.track() returns by default): three disjoint plane views of the right
    shapes, each starting a multiple of 16 bytes into the buffer -- the copy kernel that fills them moves 16 bytes per lane --
    whatever H * W % 4 is, with fewer than 8 floats of padding in all; without a pending event it is a plain CPU result."""
    import pickle
    from mft_amd.results import PendingHostResult
    (o_flow, o_occl, o_sigma), total = PendingHostResult.plane_offsets(H, W)
    n = H * W
    assert o_flow == 0 and o_occl % 4 == 0 and o_sigma % 4 == 0
    assert o_occl >= 2 * n and o_sigma >= o_occl + n and total == o_sigma + n and total - 4 * n < 8
    host = torch.arange(total, dtype=torch.float32)
    r = PendingHostResult(host, None, shape=(H, W))
    assert (r.H, r.W) == (H, W) and r.ready() and r.wait() is r
    assert r.flow.shape == (2, H, W) and r.occlusion.shape == (1, H, W) and r.sigma.shape == (1, H, W)
    for t, off in ((r.flow, o_flow), (r.occlusion, o_occl), (r.sigma, o_sigma)):
        assert t.is_contiguous() and t.data_ptr() == host.data_ptr() + 4 * off
        assert torch.equal(t.reshape(-1), host[off:off + t.numel()])
    c, p = r.clone(), pickle.loads(pickle.dumps(r))
    for q in (c, p):
        assert type(q) is FlowOUTrackingResult and torch.equal(q.flow, r.flow) and torch.equal(q.sigma, r.sigma)
    legacy = PendingHostResult(torch.zeros(4, H, W), None)            # one contiguous [4, H, W] tensor is still accepted
    assert (legacy.H, legacy.W) == (H, W) and legacy.occlusion.shape == (1, H, W)
