"""_lib.call on the GPU: a tensor of another dtype or device than the header declares is refused before anything is launched, and the
device guard inside the call is enough for tensors on a second device.  Nothing here launches a kernel except the second-device test."""
import pytest
import torch

from pytorch3d_amd import _C, _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.0


def _points_backward_args(dev):
    """p3d_rasterize_points_backward on P = 3 points and idxs (1, 2, 2, 1); the output pre-filled with a sentinel."""
    pts = torch.zeros((3, 3), dtype=torch.float32, device=dev)
    idxs = torch.zeros((1, 2, 2, 1), dtype=torch.int32, device=dev)
    gz, gd = (torch.zeros((1, 2, 2, 1), dtype=torch.float32, device=dev) for _ in range(2))
    out = torch.full((3, 3), SENTINEL, dtype=torch.float32, device=dev)
    return [pts, idxs, gz, gd, 3, 1, 2, 2, 1, out]


def test_wrong_dtype_is_rejected_before_launch():
    args = _points_backward_args(DEV)
    args[1] = args[1].to(torch.int64)
    with pytest.raises(RuntimeError, match=r"p3d_rasterize_points_backward: argument 1 is declared `const int32_t\*`.*int64"):
        _lib.call("p3d_rasterize_points_backward", "rasterize_points_backward", DEV, *args)
    torch.cuda.synchronize()
    assert bool((args[-1] == SENTINEL).all())


def test_wrong_device_is_rejected_before_launch():
    others = [torch.device("cpu")] + ([torch.device("cuda:1")] if torch.cuda.device_count() >= 2 else [])
    for other in others:
        args = _points_backward_args(DEV)
        args[2] = args[2].to(other)
        with pytest.raises(RuntimeError, match=r"p3d_rasterize_points_backward: argument 2 is declared `const float\*` and the call is "
                                               r"for cuda:0.*on " + str(other)):
            _lib.call("p3d_rasterize_points_backward", "rasterize_points_backward", DEV, *args)
        torch.cuda.synchronize()
        assert bool((args[-1] == SENTINEL).all())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_second_device_gives_the_bits_of_the_first():
    """The operators no longer enter the tensors' device themselves: the guard inside _lib.call does."""
    gen = torch.Generator().manual_seed(11)
    dists = torch.randn((1, 2, 2, 2), generator=gen) * 1e-4
    p2f = torch.tensor([0, -1, 3, 2, -1, -1, 1, 0], dtype=torch.int64).reshape(1, 2, 2, 2)
    grad = torch.randn((1, 2, 2), generator=gen)
    got = []
    assert torch.cuda.current_device() == 0
    for dev in (torch.device("cuda:0"), torch.device("cuda:1")):
        d, p, g = dists.to(dev), p2f.to(dev), grad.to(dev)
        alphas = _C.sigmoid_alpha_blend(d, p, 1e-4)
        gd = _C.sigmoid_alpha_blend_backward(g, alphas, d, p, 1e-4)
        assert alphas.device == dev and gd.device == dev and torch.cuda.current_device() == 0
        got.append((alphas.cpu(), gd.cpu()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert bool((got[0][0] > 0).any()) and bool((got[0][1] != 0).any())
