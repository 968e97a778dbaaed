"""The tracker on seeded weights, as the lane and the stream-ordering tests build it (tests/test_gpu_lanes.py,
tests/test_gpu_streams_tracker.py): one place, so that the two cannot drift apart."""
UNSET = object()


def make_tracker(weights_np, lanes, iters, deltas, async_encode=UNSET, arith=None, split_streams=None, keep_on_device=True,
                 track_store=False, multi=False, nonfinite_check_every=None):
    """-> (tracker, flow plugin).  async_encode UNSET: the key is absent from the flow configuration (the plugin's default branch).
    multi: a ``MultiTemplateMFT`` (track_store then means a store per template)."""
    from mft_amd.config import Config
    from mft_amd.MFT import MFT
    from mft_amd.multi import MultiTemplateMFT
    from mft_amd.raft import RAFTWrapper
    c = Config()
    c.flow_iters = iters
    if async_encode is not UNSET:
        c.async_encode = async_encode
    c.frames_in_flight = lanes
    if arith:
        c.raft_params = Config()
        c.raft_params.arith = arith
    if split_streams:
        c.split_streams = split_streams
    fl = RAFTWrapper(c, state_dict=weights_np)
    t = Config()
    t.deltas = list(deltas)
    t.occlusion_threshold = 0.02
    t.keep_result_on_device = keep_on_device
    t.flow_config = Config()
    t.flow_config.of_class = lambda cfg: fl
    if nonfinite_check_every:
        t.nonfinite_check_every = nonfinite_check_every
    if multi:
        t.multi_template_stores = bool(track_store)
        return MultiTemplateMFT(t), fl
    if track_store:
        t.track_store = True
    return MFT(t), fl
