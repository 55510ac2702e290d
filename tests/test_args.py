"""droid_backends._args on the CPU: the grow-only scratch cache, and the one order in which every operator checks its
tensors (is a tensor, dtype, contiguous, on a HIP device, on one device).  Nothing here reaches a kernel: every call is
refused before the library is asked for anything."""
import pytest
import torch


def test_scratch_cache_grows_only_and_keeps_keys_apart(backends):
    from droid_backends._args import ScratchCache
    cache, cpu = ScratchCache(), torch.device("cpu")
    small = cache.get_bytes((0, 1), 100, cpu)
    assert small.dtype == torch.uint8 and small.device == cpu and small.numel() == 4096   # max(int(1.25 * n), 4096)
    big = cache.get_bytes((0, 2), 10001, cpu)
    assert big.numel() == int(1.25 * 10001) == 12501
    assert cache.get_bytes((0, 2), 10001, cpu) is big and cache.get_bytes((0, 2), 12501, cpu) is big   # equal, then up to all of it
    assert cache.get_bytes((0, 2), 7, cpu) is big and cache.get_bytes((0, 2), 0, cpu) is big           # smaller
    grown = cache.get_bytes((0, 2), 12502, cpu)                                                          # larger: replaced
    assert grown is not big and grown.numel() == int(1.25 * 12502) and cache[(0, 2)] is grown
    assert cache[(0, 1)] is small and small.data_ptr() != grown.data_ptr()                              # two keys, two buffers
    assert sorted(cache) == [(0, 1), (0, 2)] and dict(cache.items()) == {(0, 1): small, (0, 2): grown}  # a mapping
    for name in ("_prox_ws", "_pc_ws", "_gm_ws"):
        assert isinstance(getattr(backends, name), ScratchCache)
    assert len({id(backends._prox_ws), id(backends._pc_ws), id(backends._gm_ws)}) == 3


def test_one_stream_helper_for_every_module(backends):
    from droid_backends import _args, ba_binding, se3
    assert backends._stream is _args._stream and se3._stream is _args._stream and ba_binding._stream is _args._stream
    assert backends._ws_key is _args._ws_key and backends._ptr is _args._ptr
    assert _args._ptr(None) is None and _args._ptr(torch.zeros(1)) != 0


def _pc_args():
    poses = torch.zeros((9, 7))
    return [poses, torch.ones((9, 6, 8)), torch.ones(4), torch.tensor([0, 3, 5]), 0.1]


def test_each_step_of_the_fixed_order(backends):
    pc = backends.point_cloud
    poses, disps, K, index, thresh = _pc_args()
    with pytest.raises(TypeError, match=r"^point_cloud: index must be a tensor, got list$"):
        pc(poses, disps, K, [0, 3, 5], thresh)
    with pytest.raises(RuntimeError, match=r"^point_cloud: disps must be float32, got torch.float16$"):
        pc(poses, disps.half(), K, index, thresh)
    with pytest.raises(RuntimeError, match=r"^point_cloud: disps must be contiguous$"):
        pc(poses, torch.ones((9, 8, 6)).transpose(1, 2), K, index, thresh)
    with pytest.raises(RuntimeError, match=r"^point_cloud: poses must be a HIP \(cuda\) tensor: droid_backends has no CPU path$"):
        pc(poses, disps, K, index, thresh)
    # the other spellings of a dtype: int64, and a choice of two
    with pytest.raises(RuntimeError, match=r"^frame_distance: ii must be int64 \(torch.long\), got torch.int32$"):
        backends.frame_distance(poses, disps, K, index.int(), index, 0.3)
    with pytest.raises(RuntimeError, match=r"^graph_mean: src must be float16 or float32, got torch.float64$"):
        backends.graph_mean(torch.zeros((1, 3, 2, 2, 2), dtype=torch.float64), index)
    # the same vocabulary where an operator calls the steps itself (se3: records are made contiguous, never refused)
    with pytest.raises(TypeError, match=r"^SE3.exp: xi must be a tensor, got list$"):
        backends.SE3.exp([0.0] * 6)
    with pytest.raises(RuntimeError, match=r"^SE3.inv: data must be a HIP \(cuda\) tensor: droid_backends has no CPU path$"):
        backends.SE3(poses.t().contiguous().t()).inv()


def test_on_one_device_is_the_last_step():
    """Without a second device the step is driven directly: a HIP-placed stand-in cannot be built on the CPU, so the
    tensors here are `meta` ones told to answer is_cuda."""
    from droid_backends._args import check_tensors

    class OnDevice(torch.Tensor):
        is_cuda = True

    a = torch.zeros(2, device="meta").as_subclass(OnDevice)
    b = torch.zeros(2).as_subclass(OnDevice)
    check_tensors("op", [(a, "a", torch.float32)], on=(a, "a"))
    with pytest.raises(RuntimeError, match=r"^op: b is on cpu, a on meta$"):
        check_tensors("op", [(a, "a", torch.float32), (b, "b", torch.float32)], on=(a, "a"))
    with pytest.raises(RuntimeError, match=r"^op: b must be contiguous$"):   # an earlier step of a later tensor wins
        check_tensors("op", [(a, "a", None), (torch.zeros((2, 2)).t().as_subclass(OnDevice), "b", None)], on=(a, "a"))


def test_the_earlier_step_wins(backends):
    pc = backends.point_cloud
    poses, disps, K, index, thresh = _pc_args()
    with pytest.raises(RuntimeError, match="point_cloud: disps must be float32"):       # CPU and wrong dtype: the dtype
        pc(poses, disps.double(), K, index, thresh)
    with pytest.raises(RuntimeError, match="point_cloud: index must be int64"):         # dtype before contiguity
        pc(poses, torch.ones((9, 8, 6)).transpose(1, 2), K, index.int(), thresh)
    with pytest.raises(TypeError, match="point_cloud: poses must be a tensor"):         # is a tensor before a dtype
        pc(None, disps.double(), K, index, thresh)
    with pytest.raises(RuntimeError, match="point_cloud: disps must be contiguous"):    # contiguity before the device
        pc(poses, torch.ones((9, 8, 6)).transpose(1, 2), K, index, thresh)
    with pytest.raises(RuntimeError, match=r"point_cloud: index must be \[n\]"):        # an operator's shapes sit between
        pc(poses, torch.ones((9, 8, 6)).transpose(1, 2), K, index[None], thresh)        # the dtype and the contiguity step
    with pytest.raises(RuntimeError, match="depth_filter: thresh must be float32"):     # an older operator: the same order
        backends.depth_filter(poses, disps.transpose(1, 2), K, index, torch.ones(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ba: targets must be contiguous"):
        t = torch.zeros((2, 2, 8, 6)).transpose(2, 3)
        backends.ba(poses, disps, K, disps, t, t.contiguous(), disps[:3], index[:2], index[:2], 0, 3, 1, 1e-4, 0.1, False)
    with pytest.raises(RuntimeError, match="scatter_mean: index must be int64"):
        backends.scatter_mean(torch.zeros((1, 3, 4)).transpose(1, 2), index.int())
