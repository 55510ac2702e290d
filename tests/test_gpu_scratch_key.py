"""The scratch of point_cloud and graph_mean is keyed like every other one, by droid_backends._ws_key: `cuda` without an
index and `cuda:<current>` name one device and share one buffer, a second stream gets a second one, and the results do
not depend on which buffer served the call."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _point_cloud_call(backends, dev):
    g = torch.Generator().manual_seed(5)
    poses = torch.zeros((3, 7))
    poses[:, 6] = 1
    poses[:, 0] = torch.tensor([0.0, 0.05, 0.1])
    disps = 1.0 + 0.01 * torch.rand((3, 6, 8), generator=g)
    K = torch.tensor([8.0, 8.0, 4.0, 3.0])
    index = torch.tensor([0, 2])
    pc = backends.point_cloud(poses.to(dev), disps.to(dev), K.to(dev), index.to(dev), 0.5, min_count=1)
    return [pc.points, pc.src, pc.offsets, pc.matrices]


def _graph_mean_call(backends, dev):
    g = torch.Generator().manual_seed(6)
    net = torch.rand((3, 2, 2, 2), generator=g)   # E = 3 rows, a plane of 8 elements
    ii = torch.tensor([4, 1, 4])                   # 2 sources
    return [backends.graph_mean(net.to(dev), ii.to(dev), num_groups=2, nbuf=5)]


@pytest.mark.parametrize("call, cache", [(_point_cloud_call, "_pc_ws"), (_graph_mean_call, "_gm_ws")])
def test_one_scratch_per_device_and_stream(backends, call, cache):
    cache = getattr(backends, cache)
    cur = torch.cuda.current_device()
    key = backends._ws_key(torch.device("cuda"))
    assert key == backends._ws_key(torch.device("cuda", cur)) == (cur, torch.cuda.current_stream().cuda_stream)
    first = call(backends, torch.device("cuda"))
    ws = cache[key]
    again = call(backends, torch.device("cuda", cur))
    assert cache[key] is ws and [k for k in cache if k[1] == key[1]] == [key]   # one entry for both spellings
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        key2 = backends._ws_key(torch.device("cuda"))
        other = call(backends, torch.device("cuda"))
    side.synchronize()
    assert key2 == (cur, side.cuda_stream) and key2 != key
    assert cache[key2].data_ptr() != ws.data_ptr() and cache[key] is ws          # a second entry for the second stream
    torch.cuda.synchronize()
    assert first[-1].numel() > 0
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)                            # bit for bit
