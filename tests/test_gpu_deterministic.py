"""The deterministic backwards (torch.use_deterministic_algorithms(True), not warn-only; include/p3d_amd.h: *_ordered).

Five families -- the mesh rasterizer's backward (per face and through `faces`), the face-vertex scatter, the point rasterizer's
backward (plain and fused with the compositor), the compositors' grad_features, interpolate_face_attributes' grad_face_attrs --
  1. work under the flag, through the ctypes and the pybind boundary;
  2. return the SAME BITS whatever the stream, the neighbours on the device, the previous contents of the allocator's blocks, the row
     cover, the boundary flavour, and across fresh processes;
  3. pass the value gates of the atomic path unchanged (tests/_util.assert_face_grads_vs_truth; the oracle / float64 comparisons of
     tests/test_gpu_points_composite_interp.py and tests/test_gpu_render_points.py, restated with their tolerances);
  4. end to end through the package's autograd nodes;
  5. at the size of the bench batch.
Every test runs with the strict flag set (fixture) and restores it; the float64 / oracle legs run with the flag lifted for their own
torch calls only.
"""
import contextlib
import hashlib
import math
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":  # the child of test_bits_repeat_across_processes
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import _util as U
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SOFTRAS_BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


@pytest.fixture(autouse=True)
def _strict():
    with _flag(True):
        yield


def _pybind():
    from pytorch3d_amd import build_bind

    return build_bind.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs that make the order of a float sum matter
# ---------------------------------------------------------------------------------------------------------------------------------
def _ndc(i, S1, S2):  # rasterization_utils.cuh:16-42
    rng = 2.0 * S1 / S2 if S1 > S2 else 2.0
    return -rng / 2.0 + (rng * i + rng / 2.0) / S1


def mesh_scene(K, seed=0, size=(96, 128)):
    """Three meshes of very different sizes on a non-square image: [0] one triangle over the whole frame (a segment of ~12 000 samples:
    ~190 waves) in front of a soup; [1] 3 072 triangles of a third of a pixel, one per pixel centre (blur 0: segments of one sample) and a soup
    behind them; [2] faces beside the frame (an all-background image, rows that stay zero).  -> dict of GPU tensors."""
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(seed)
    H, W = size
    big = torch.tensor([[[-3.0, -3.0, 0.4], [3.0, -3.0, 0.5], [0.0, 3.5, 0.6]]])
    soup0 = U.smooth_soup(300, gen, size=1.5)
    ys, xs = torch.meshgrid(torch.arange(16, 64), torch.arange(32, 96), indexing="ij")
    cx, cy = _ndc(xs.reshape(-1).float(), W, H), _ndc(ys.reshape(-1).float(), H, W)
    h = 0.3 * 2.0 / H
    z = 0.3 + 0.1 * torch.rand(cx.shape[0], generator=gen)
    tiny = torch.stack([torch.stack([cx - h, cy - h, z], 1), torch.stack([cx + h, cy - h, z + 0.01], 1), torch.stack([cx, cy + h, z + 0.02], 1)], 1)
    soup1 = U.smooth_soup(200, gen, size=1.0)
    off = U.smooth_soup(50, gen, size=0.5)
    off[:, :, 0] += 6.0
    parts = [torch.cat([big, soup0]), torch.cat([tiny, soup1]), off]
    fv = torch.cat(parts).contiguous()
    count = torch.tensor([p.shape[0] for p in parts])
    first = torch.cumsum(count, 0) - count
    F = fv.shape[0]
    # an index list for the (V, 3) form (only the scatter reads it): every corner its own vertex, then corners merged in a fixed
    # pattern -- pairs of neighbouring faces, and one vertex shared by a seventh of all faces -- and a few vertices nobody uses
    V = F * 3 + 5
    faces = torch.arange(F * 3).reshape(F, 3)
    faces[1::2, 0] = faces[0::2, 0][: faces[1::2].shape[0]]
    faces[5::7, 1] = 3
    nbr = torch.full((F,), -1, dtype=torch.int64)
    fv, first, count, nbr = fv.to(d), first.to(d), count.to(d), nbr.to(d)
    with _flag(False):
        (p2f, zbuf, bary, dists), cover = _C._rasterize_meshes_covered(fv, first, count, nbr, size, 0.0, K, 16, 4000, True, True, False)
    gz = torch.randn(zbuf.shape, generator=gen).to(d)
    gb = torch.randn(bary.shape, generator=gen).to(d)
    gd = torch.randn(dists.shape, generator=gen).to(d)
    return dict(fv=fv, faces=faces.to(d), V=V, p2f=p2f, cover=cover, gz=gz, gb=gb, gd=gd, F=F, K=K, size=size)


def point_scene(K, seed=0, size=(96, 128), C=3):
    """Three clouds: [0] one point of radius 0.9 in front (thousands of pixels) over 1 500 points of radius 0.05; [1] 3 000 points
    of a third of a pixel on pixel centres; [2] points beside the frame.  A few points of [0] lie outside every pixel too."""
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(seed)
    H, W = size
    c0 = torch.cat([torch.tensor([[0.05, -0.02, 0.2]]), torch.cat([torch.rand(1500, 2, generator=gen) * 2.6 - 1.3, torch.rand(1500, 1, generator=gen) + 0.5], 1)])
    r0 = torch.cat([torch.tensor([0.9]), torch.full((1500,), 0.05)])
    ys, xs = torch.meshgrid(torch.arange(20, 70), torch.arange(30, 90), indexing="ij")
    c1 = torch.stack([_ndc(xs.reshape(-1).float(), W, H), _ndc(ys.reshape(-1).float(), H, W), 0.5 + torch.rand(3000, generator=gen)], 1)
    r1 = torch.full((3000,), 0.3 * 2.0 / H)
    c2 = torch.cat([torch.rand(40, 2, generator=gen) + 5.0, torch.rand(40, 1, generator=gen) + 0.5], 1)
    r2 = torch.full((40,), 0.05)
    pts = torch.cat([c0, c1, c2]).to(d)
    rad = torch.cat([r0, r1, r2]).to(d)
    count = torch.tensor([c0.shape[0], c1.shape[0], c2.shape[0]])
    first = (torch.cumsum(count, 0) - count).to(d)
    count = count.to(d)
    feats = torch.rand(pts.shape[0], C, generator=gen).to(d)
    inv_r2 = _C.inv_r2_of(0.9)
    with _flag(False):
        idx, zbuf, dists, images = _C.rasterize_points_composite(pts, first, count, size, rad, feats, inv_r2, K, 16, 3000, "alpha")
    gz = torch.randn(zbuf.shape, generator=gen).to(d)
    gd = torch.randn(dists.shape, generator=gen).to(d)
    gi = torch.randn(images.shape, generator=gen).to(d)
    return dict(pts=pts, feats=feats, idx=idx, dists=dists, gz=gz, gd=gd, gi=gi, inv_r2=inv_r2, K=K, P=pts.shape[0], C=C)


def _ops(K):
    """name -> (fn(flavour module, use_cover) -> tuple of tensors, output floats, workspace bytes, has a pybind form)."""
    from pytorch3d_amd import _C, _lib

    lib = _lib.load()
    m = mesh_scene(K)
    p = point_scene(K)
    hits_m = int((m["p2f"] >= 0).sum())
    hits_p = int((p["idx"] >= 0).sum())
    N, H, W, _ = p["idx"].shape
    # compositors and interp on the point scene's fragments: permuted views, as the renderers pass them
    alphas = (1 - p["dists"] * p["inv_r2"]).clamp(0, 1).permute(0, 3, 1, 2)
    pidx = p["idx"].long().permute(0, 3, 1, 2)
    gen = torch.Generator().manual_seed(5)
    C = 9
    featsT = torch.rand(p["P"], C, generator=gen).to(_dev()).t()
    go = torch.randn(N, C, H, W, generator=gen).to(_dev())
    D = 5
    p2f_flat = m["p2f"].reshape(-1)
    bary = torch.rand(p2f_flat.shape[0], 3, generator=gen).to(_dev())
    attrs = torch.randn(m["F"], 3, D, generator=gen).to(_dev())
    gpa = torch.randn(p2f_flat.shape[0], D, generator=gen).to(_dev())
    gfv = torch.randn(m["F"], 3, 3, generator=gen).to(_dev())

    def mesh(mod, cover):
        if mod is _C:
            return (_C.rasterize_meshes_backward(m["fv"], m["p2f"] if cover else m["p2f"].clone(), m["gz"], m["gb"], m["gd"], True, True,
                                                 _cover=m["cover"] if cover else None),)
        return (mod.rasterize_meshes_backward(m["fv"], m["p2f"], m["gz"], m["gb"], m["gd"], True, True),)

    def mesh_verts(mod, cover):
        return (_C._mesh_backward(m["fv"], m["faces"], m["V"], m["p2f"], m["gz"], m["gb"], m["gd"], True, True, m["cover"] if cover else None),)

    def scatter(mod, cover):
        return (_C.scatter_face_grads(gfv, m["faces"], m["V"]),)

    def points(mod, cover):
        return (mod.rasterize_points_backward(p["pts"], p["idx"], p["gz"], p["gd"]),)

    def fused(mode):
        return lambda mod, cover: _C.rasterize_points_composite_backward(p["pts"], p["feats"], p["idx"], p["dists"], p["gi"], p["inv_r2"], mode)

    def comp(name):
        return lambda mod, cover: getattr(mod, "accum_" + name + "_backward")(go, featsT, alphas, pidx)

    def interp(mod, cover):
        if mod is _C and cover:  # the image-shaped form and the flat one: one entry, the same bits
            return _C.interp_face_attrs_backward(p2f_flat, bary, attrs, gpa, image_shape=tuple(m["p2f"].shape))
        return mod.interp_face_attrs_backward(p2f_flat, bary, attrs, gpa)

    F, V, P = m["F"], m["V"], p["P"]
    ops = {
        "mesh": (mesh, F * 9, lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(F, 0, hits_m), True),
        "mesh_verts": (mesh_verts, V * 3, lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(F, 1, hits_m), False),
        "scatter": (scatter, V * 3, lib.p3d_scatter_face_grads_ordered_workspace_bytes(F), False),
        "points": (points, P * 3, lib.p3d_rasterize_points_backward_ordered_workspace_bytes(hits_p), True),
        "interp": (interp, F * 3 * D, lib.p3d_interp_face_attrs_backward_ordered_workspace_bytes(D, hits_m), True),
    }
    if K <= 16:  # the fused forward / backward pair is PointsRenderer's (K <= 16: render_points.MAX_FUSED_K)
        for mode in ("alpha", "norm"):
            ops["fused_" + mode] = (fused(mode), P * (3 + p["C"]),
                                    lib.p3d_rasterize_points_composite_backward_ordered_workspace_bytes(N, H, W, K, p["C"], hits_p), False)
    for name in ("alphacomposite", "weightedsumnorm", "weightedsum"):
        ops[name] = (comp(name), C * P, lib.p3d_composite_backward_ordered_workspace_bytes(N, K, H, W, C, hits_p), True)
    return ops


FAMILIES = ["mesh", "mesh_verts", "scatter", "points", "fused_alpha", "fused_norm", "alphacomposite", "weightedsumnorm", "weightedsum", "interp"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the operators work under the flag, through both flavours
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_family_returns_a_gradient_under_the_strict_flag():
    from pytorch3d_amd import _C

    assert torch.are_deterministic_algorithms_enabled() and not torch.is_deterministic_algorithms_warn_only_enabled()
    ops = _ops(8)
    assert sorted(ops) == sorted(FAMILIES)
    pb = _pybind()
    for name, (fn, _, _, has_pybind) in ops.items():
        for mod in (_C, pb) if has_pybind else (_C,):
            outs = fn(mod, True)
            assert all(bool(torch.isfinite(o).all()) for o in outs), name
            assert any(float(o.abs().max()) > 0 for o in outs), name


def test_float64_interp_keeps_its_refusal_and_says_so():
    from pytorch3d_amd import _C

    d = _dev()
    p2f = torch.zeros(4, dtype=torch.int64, device=d)
    for mod in (_C, _pybind()):
        with pytest.raises(RuntimeError, match="float64"):
            mod.interp_face_attrs_backward(p2f, torch.rand(4, 3, device=d, dtype=torch.float64), torch.rand(2, 3, 2, device=d, dtype=torch.float64),
                                           torch.rand(4, 2, device=d, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. bits repeat
# ---------------------------------------------------------------------------------------------------------------------------------
def _busy(n=6):
    """Unrelated kernels on the current stream (not waited for)."""
    a = torch.rand(2048, 2048, device=_dev())
    for _ in range(n):
        a = (a @ a).clamp_(0, 1)
    return a


@pytest.mark.parametrize("K", [1, 8, 50])
def test_bits_repeat_in_one_process(K):
    from pytorch3d_amd import _C

    ops = _ops(K)
    pb = _pybind()
    main = torch.cuda.current_stream()
    for name, (fn, out_floats, ws_bytes, has_pybind) in ops.items():
        base = [o.clone() for o in fn(_C, True)]
        runs = {}
        # on a second stream, unrelated kernels beside it on the first
        side = torch.cuda.Stream()
        side.wait_stream(main)
        keep = _busy()
        with torch.cuda.stream(side):
            runs["second stream"] = [o.clone() for o in fn(_C, True)]
        main.wait_stream(side)
        torch.cuda.synchronize()
        del keep
        # after NaN-filled blocks of the output's and the workspace's size went back to the allocator
        junk = [torch.full((max(out_floats, 1),), float("nan"), device=_dev()), torch.full((max(ws_bytes // 4, 64),), float("nan"), device=_dev())]
        torch.cuda.synchronize()
        del junk
        runs["after NaN blocks"] = [o.clone() for o in fn(_C, True)]
        runs["no cover / flat form"] = [o.clone() for o in fn(_C, False)]
        if has_pybind:
            runs["pybind"] = [o.clone() for o in fn(pb, False)]
        torch.cuda.synchronize()
        for tag, outs in runs.items():
            for i, (a, b) in enumerate(zip(base, outs)):
                assert a.shape == b.shape and torch.equal(a, b), (f"{name} K={K}: output {i} differs in {int((a != b).sum())} of {a.numel()} words: {tag}")
        assert all(bool(torch.isfinite(o).all()) for o in base), name


def test_rows_nobody_hits_are_zero_and_empty_inputs_work():
    from pytorch3d_amd import _C

    d = _dev()
    m = mesh_scene(8)
    g = _C.rasterize_meshes_backward(m["fv"], m["p2f"], m["gz"], m["gb"], m["gd"], True, True)
    hit = torch.zeros(m["F"], dtype=torch.bool, device=d)
    hit[m["p2f"][m["p2f"] >= 0]] = True
    assert int((~hit).sum()) >= 50 and int(hit.sum()) > 3000
    assert float(g[~hit].abs().max()) == 0.0
    assert int((m["p2f"][2] >= 0).sum()) == 0, "the third image is meant to be all background"
    p = point_scene(8)
    gp = _C.rasterize_points_backward(p["pts"], p["idx"], p["gz"], p["gd"])
    hitp = torch.zeros(p["P"], dtype=torch.bool, device=d)
    hitp[p["idx"][p["idx"] >= 0].long()] = True
    assert int((~hitp).sum()) >= 40 and float(gp[~hitp].abs().max()) == 0.0
    # an image without any primitive, F = 0, P = 0
    none = torch.full_like(m["p2f"], -1)
    assert float(_C.rasterize_meshes_backward(m["fv"], none, m["gz"], m["gb"], m["gd"], True, True).abs().max()) == 0.0
    assert float(_C._mesh_backward(m["fv"], m["faces"], m["V"], none, m["gz"], m["gb"], m["gd"], True, True, None).abs().max()) == 0.0
    assert _C.rasterize_meshes_backward(m["fv"][:0], none, m["gz"], m["gb"], m["gd"], True, True).shape == (0, 3, 3)
    assert float(_C.scatter_face_grads(torch.zeros(0, 3, 3, device=d), torch.zeros(0, 3, dtype=torch.int64, device=d), 7).abs().max()) == 0.0
    nonep = torch.full_like(p["idx"], -1)
    assert float(_C.rasterize_points_backward(p["pts"], nonep, p["gz"], p["gd"]).abs().max()) == 0.0
    assert _C.rasterize_points_backward(p["pts"][:0], nonep, p["gz"], p["gd"]).shape == (0, 3)
    a, b = _C.rasterize_points_composite_backward(p["pts"], p["feats"], nonep, p["dists"], p["gi"], p["inv_r2"], "alpha")
    assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0
    gf, ga = _C.accum_alphacomposite_backward(torch.randn(3, 4, 9, 11, device=d), torch.rand(4, 20, device=d), torch.rand(3, 5, 9, 11, device=d),
                                              torch.full((3, 5, 9, 11), -1, dtype=torch.int64, device=d))
    assert float(gf.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0
    gb, gfa = _C.interp_face_attrs_backward(torch.full((100,), -1, dtype=torch.int64, device=d), torch.rand(100, 3, device=d),
                                            torch.rand(6, 3, 4, device=d), torch.rand(100, 4, device=d))
    assert float(gb.abs().max()) == 0.0 and float(gfa.abs().max()) == 0.0


def _child_digest(which):
    """sha256 of the gradients of the mesh case (both forms) or the fused point case, computed in THIS process."""
    from pytorch3d_amd import _C

    torch.use_deterministic_algorithms(True)
    if which == "mesh":
        m = mesh_scene(8)
        outs = [_C.rasterize_meshes_backward(m["fv"], m["p2f"], m["gz"], m["gb"], m["gd"], True, True),
                _C._mesh_backward(m["fv"], m["faces"], m["V"], m["p2f"], m["gz"], m["gb"], m["gd"], True, True, m["cover"])]
    else:
        p = point_scene(8)
        outs = list(_C.rasterize_points_composite_backward(p["pts"], p["feats"], p["idx"], p["dists"], p["gi"], p["inv_r2"], "alpha"))
    h = hashlib.sha256()
    for o in outs:
        h.update(o.cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("which", ["mesh", "fused_points"])
def test_bits_repeat_across_processes(which):
    """Two fresh children, one after the other, each under its own timeout; the chain stops at the first that fails.  A comparison,
    not a retry."""
    digests = []
    for _ in range(2):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], capture_output=True, text=True, timeout=200)
        assert res.returncode == 0, res.stderr[-2000:]
        digests.append(res.stdout.strip().splitlines()[-1])
    assert len(digests[0]) == 64 and digests[0] == digests[1], digests
    assert digests[0] == _child_digest(which)  # and the parent, with everything else it has run, agrees


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. values: the gates of the atomic path, unchanged
# ---------------------------------------------------------------------------------------------------------------------------------
MESH_VALUE_SIZE, MESH_VALUE_K, MESH_VALUE_BLUR = (48, 48), 4, 1e-3


def mesh_value_inputs():
    """tests/test_gpu_meshes.py::test_backward_vs_oracle's batch."""
    from pytorch3d_amd import PackedMeshes

    verts, faces = U.hetero_batch(3, seed=4, fmin=200, fmax=800)
    m = PackedMeshes(verts, faces)
    fv = m.verts_packed()[m.faces_packed()]
    first, count = m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh()
    return m, fv, first, count, torch.full((fv.shape[0],), -1, dtype=torch.int64)


@pytest.mark.parametrize("persp,clip", [(False, False), (True, False), (False, True), (True, True)])
def test_mesh_values_pass_the_gate_of_the_atomic_path(persp, clip):
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(21)
    m, fv, first, count, nbr = mesh_value_inputs()
    with _flag(False):
        fwd = [o.cpu() for o in _C.rasterize_meshes(fv.to(d), first.to(d), count.to(d), nbr.to(d), MESH_VALUE_SIZE, MESH_VALUE_BLUR, MESH_VALUE_K,
                                                    8, 1000, persp, clip, False)]
    gz = torch.randn(fwd[1].shape, generator=gen)
    gb = torch.randn(fwd[2].shape, generator=gen)
    gd = torch.randn(fwd[3].shape, generator=gen)
    faces, V = m.faces_packed(), m.verts_packed().shape[0]
    dev = [t.to(d) for t in (fv, fwd[0], gz, gb, gd)]
    for flavour in (_C, _pybind()):
        got = flavour.rasterize_meshes_backward(*dev, persp, clip).cpu()
        with _flag(False):
            worst = U.assert_face_grads_vs_truth(f"ordered backward persp={persp} clip={clip} {getattr(flavour, '__name__', 'pybind')}", got, fv,
                                                 fwd[0], gz, gb, gd, persp, clip)
        print(f"[ordered (F,3,3) persp={persp} clip={clip}] largest |error| / scale = {worst:.3e} (gate 5e-3)")
    gv = _C._mesh_backward(dev[0], faces.to(d), V, dev[1], dev[2], dev[3], dev[4], persp, clip, None).cpu()
    with _flag(False):
        worst = U.assert_face_grads_vs_truth(f"ordered backward to the vertices persp={persp} clip={clip}", gv, fv, fwd[0], gz, gb, gd, persp, clip,
                                             faces=faces, num_verts=V)
        atomic = _C.rasterize_meshes_backward(*dev, persp, clip).cpu()
    print(f"[ordered (V,3) persp={persp} clip={clip}] largest |error| / scale = {worst:.3e} (gate 5e-3); ordered vs atomic (F,3,3): "
          f"{int((atomic != got).sum())} of {got.numel()} words differ")
    # the scatter on its own: the (V, 3) form is the (F, 3, 3) form scattered in the same order
    assert torch.equal(_C.scatter_face_grads(got.to(d), faces.to(d), V).cpu(), gv)


@pytest.mark.parametrize("size", [(40, 56), (45, 59)])
def test_point_values(size):
    """tests/test_gpu_points_composite_interp.py::test_points_backward_and_autograd's inputs and tolerance."""
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(8)
    pts = torch.cat([torch.rand(2000, 2, generator=gen) * 2.4 - 1.2, torch.rand(2000, 1, generator=gen) * 1.9 + 0.1], 1)
    clouds = p3d.PackedPointclouds([pts[:900].to(d), pts[900:].to(d)])
    idx, zbuf, dists = p3d.rasterize_points(clouds, image_size=size, radius=0.05, points_per_pixel=5)
    gz = torch.randn(zbuf.shape, generator=gen)
    gd = torch.randn(dists.shape, generator=gen)
    ref = orc.rasterize_points_backward(pts, idx.cpu(), gz, gd, acc64=True)
    scale = ref.abs().max().item()
    for flavour in (_C, _pybind()):
        got = flavour.rasterize_points_backward(pts.to(d), idx, gz.to(d), gd.to(d)).cpu()
        print(f"[ordered points {size}] max |error| = {float((got - ref).abs().max()):.3e}, scale {scale:.3e}")
        assert torch.allclose(got, ref, rtol=1e-4, atol=5e-6 * max(scale, 1.0))


@pytest.mark.parametrize("mode", ["alphacomposite", "weightedsumnorm", "weightedsum"])
@pytest.mark.parametrize("K", [4, 10, 16, 17, 24, 32, 40])
@pytest.mark.parametrize("permuted", [False, True])
def test_compositor_values(mode, K, permuted):
    """tests/test_gpu_points_composite_interp.py::test_compositors' inputs and tolerances."""
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(K)
    N, C, P, H, W = 2, (5 if K != 10 else 9), 300, 13, 17
    feat = torch.rand(C, P, generator=gen)
    if permuted:
        feat = torch.rand(P, C, generator=gen).t()
        alphas = torch.rand(N, H, W, K, generator=gen).permute(0, 3, 1, 2)
        idx = torch.randint(-1, P, (N, H, W, K), generator=gen).permute(0, 3, 1, 2)
    else:
        alphas = torch.rand(N, K, H, W, generator=gen)
        idx = torch.randint(-1, P, (N, K, H, W), generator=gen)
    go = torch.randn(N, C, H, W, generator=gen)
    rgf, rga = orc.composite_backward(mode, go, feat, alphas, idx)
    outs = []
    for flavour in (_C, _pybind()):
        gf, ga = getattr(flavour, "accum_" + mode + "_backward")(go.to(d), feat.to(d), alphas.to(d), idx.to(d))
        assert tuple(gf.shape) == (C, P) and (gf.stride() == ((1, C) if permuted else (P, 1)))
        assert torch.allclose(gf.cpu(), rgf, atol=2e-5, rtol=1e-4)
        assert torch.allclose(ga.cpu(), rga, atol=2e-5 * max(1.0, rga.abs().max().item()), rtol=1e-4)
        outs.append((gf.cpu(), ga.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # a contiguous copy of the same logical tensors: the same bits (the order is that of the logical (N, K, H, W) index)
    gf2, ga2 = getattr(_C, "accum_" + mode + "_backward")(go.to(d), feat.contiguous().to(d), alphas.contiguous().to(d), idx.contiguous().to(d))
    assert torch.equal(gf2.cpu(), outs[0][0]) and torch.equal(ga2.cpu(), outs[0][1])
    print(f"[ordered {mode} K={K}] max |grad_features error| = {float((outs[0][0] - rgf).abs().max()):.3e} (gate 2e-5 + 1e-4 rel)")


@pytest.mark.parametrize("D", [1, 3, 4, 7, 8, 32])
def test_interp_values(D):
    """tests/test_gpu_points_composite_interp.py::test_interp_face_attrs' inputs and tolerances."""
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(D)
    P, F = 5000, 60
    p2f = torch.randint(-1, F, (P,), generator=gen)
    bary = torch.rand(P, 3, generator=gen)
    attrs = torch.randn(F, 3, D, generator=gen)
    g = torch.randn(P, D, generator=gen)
    rgb, rgf = orc.interp_backward(p2f, bary, attrs, g)
    outs = []
    for flavour in (_C, _pybind()):
        gb, gf = flavour.interp_face_attrs_backward(p2f.to(d), bary.to(d), attrs.to(d), g.to(d))
        assert torch.allclose(gb.cpu(), rgb, atol=1e-5, rtol=1e-5)
        assert torch.allclose(gf.cpu(), rgf, atol=1e-4, rtol=1e-4)
        outs.append(gf.cpu())
    shaped = _C.interp_face_attrs_backward(p2f.to(d), bary.to(d), attrs.to(d), g.to(d), image_shape=(2, 25, 20, 5))[1].cpu()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], shaped)
    print(f"[ordered interp D={D}] max |grad_face_attrs error| = {float((outs[0] - rgf).abs().max()):.3e} (gate 1e-4 + 1e-4 rel)")


@pytest.mark.parametrize("mode", ["alpha", "norm"])
@pytest.mark.parametrize("K,C", [(1, 3), (8, 4), (10, 3), (16, 3)])
def test_fused_point_values(K, C, mode):
    """tests/test_gpu_render_points.py::test_fused_backward_vs_operator_chain_and_float64's inputs, float64 restatement and tolerance."""
    import test_gpu_render_points as RP
    from pytorch3d_amd import PackedPointclouds, _C, render_points_alpha
    from pytorch3d_amd.rasterize_points import rasterize_points

    d = _dev()
    size = (40, 56)
    gen = torch.Generator().manual_seed(K * 10 + C + size[0])
    r = 0.25
    clouds = [RP._cloud(400, gen, zlo=0.1), RP._cloud(650, gen, zlo=0.1)]
    fl = [torch.rand(c.shape[0], C, generator=gen) for c in clouds]
    pts = torch.cat(clouds).to(d).requires_grad_(True)
    feats = torch.cat(fl).to(d).requires_grad_(True)
    pc = PackedPointclouds([pts[:400], pts[400:]])
    g_img = torch.randn((2,) + size + (C,), generator=gen)
    if mode == "norm":  # (see there: pixels whose weights sum to rounding noise get no upstream gradient)
        with torch.no_grad():
            i0, _, d0 = rasterize_points(pc, image_size=size, radius=r, points_per_pixel=K, bin_size=8, max_points_per_bin=700)
        asum = torch.where(i0 >= 0, 1 - d0 * _C.inv_r2_of(r), torch.zeros_like(d0)).sum(-1)
        g_img = g_img * ((asum > 0.05) | (i0[..., 0] < 0)).cpu()[..., None]
    img, idx, zbuf, dists = render_points_alpha(pc, feats, image_size=size, radius=r, points_per_pixel=K, bin_size=8, max_points_per_bin=700,
                                                compositor=mode)
    (img * g_img.to(d)).sum().backward()
    gp, gf = pts.grad.clone(), feats.grad.clone()
    assert float(gp[:, 2].abs().max()) == 0.0
    with _flag(False):
        _, gp64, gf64 = RP._f64_chain_grads(pts.detach().cpu(), feats.detach().cpu(), idx.cpu(), size, r, g_img, mode)
    for name, a, b in (("points", gp.cpu().double(), gp64), ("features", gf.cpu().double(), gf64)):
        scale = float(b.abs().max())
        print(f"[ordered fused {mode} K={K} C={C}] {name}: max |error| = {float((a - b).abs().max()):.3e}, gate {2e-4 * scale + 1e-6:.3e}")
        assert float((a - b).abs().max()) <= 2e-4 * scale + 1e-6, name


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. end to end through the package's own nodes
# ---------------------------------------------------------------------------------------------------------------------------------
def _mesh_loss(out):
    p2f, zbuf, bary, dists = out
    mask = (p2f >= 0).float()
    return (zbuf * mask).sum() + (bary * mask[..., None]).sum() * 0.5 + (torch.sigmoid(-dists / 1e-4) * mask).sum()


@pytest.mark.parametrize("node", ["face_verts", "mesh_verts", "world"])
def test_end_to_end_meshes(node):
    """SURVEY.md 8(d) config 3's loop at a smaller size: a scalar loss on the fragments, backward, twice; verts.grad bit-equal."""
    import pytorch3d_amd as p3d
    from pytorch3d_amd.rasterize_meshes import gather_face_verts, rasterize_meshes_world, _RasterizeFaceVerts

    d = _dev()
    verts, faces = U.hetero_batch(4, seed=2, fmin=300, fmax=3000)
    grads = []
    for _ in range(2):
        vs = [v.to(d).requires_grad_(True) for v in verts]
        m = p3d.PackedMeshes(vs, [f.to(d) for f in faces])
        kw = dict(image_size=(96, 160), blur_radius=SOFTRAS_BLUR, faces_per_pixel=8, perspective_correct=True, clip_barycentric_coords=True)
        if node == "mesh_verts":
            out = p3d.rasterize_meshes(m, **kw)
        elif node == "world":
            eye = torch.eye(4, device=d)[None]
            out = rasterize_meshes_world(m, eye, eye, **kw)
        else:  # the gather node + the per-face node, as with clipping
            fv = gather_face_verts(m.verts_packed(), m.faces_packed())
            F = fv.shape[0]
            out = _RasterizeFaceVerts.apply(fv, m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh(),
                                            torch.full((F,), -1, dtype=torch.int64, device=d), (96, 160), SOFTRAS_BLUR, 8, 16, 10000, True, True, False)
        _mesh_loss(out).backward()
        _busy(2)
        grads.append(torch.cat([v.grad for v in vs]).clone())
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1]), f"{int((grads[0] != grads[1]).sum())} words differ"


@pytest.mark.parametrize("mode", ["alpha", "norm"])
def test_end_to_end_points(mode):
    """SURVEY.md 8(d) config 4's chain: render_points, a scalar loss on the image; points.grad and features.grad bit-equal."""
    from pytorch3d_amd import PackedPointclouds, render_points_alpha

    d = _dev()
    gen = torch.Generator().manual_seed(3)
    base = [torch.cat([torch.rand(n, 2, generator=gen) * 2.2 - 1.1, torch.rand(n, 1, generator=gen) + 0.2], 1) for n in (5000, 300, 12000)]
    feats0 = torch.rand(sum(b.shape[0] for b in base), 3, generator=gen)
    target = torch.rand(3, 72, 128, 3, generator=gen).to(d)
    grads = []
    for _ in range(2):
        ps = [b.to(d).requires_grad_(True) for b in base]
        f = feats0.to(d).requires_grad_(True)
        img, _, _, _ = render_points_alpha(PackedPointclouds(ps), f, image_size=(72, 128), radius=0.06, points_per_pixel=8, compositor=mode)
        ((img - target) ** 2).sum().backward()
        _busy(2)
        grads.append((torch.cat([p.grad for p in ps]).clone(), f.grad.clone()))
    for a, b in zip(grads[0], grads[1]):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)


def test_end_to_end_interp_and_compositors():
    import pytorch3d_amd as p3d

    d = _dev()
    gen = torch.Generator().manual_seed(4)
    m = mesh_scene(8)
    F = m["F"]
    grads = []
    for _ in range(2):
        attrs = torch.randn(F, 3, 6, generator=torch.Generator().manual_seed(9)).to(d).requires_grad_(True)
        bary = torch.rand(tuple(m["p2f"].shape) + (3,), generator=torch.Generator().manual_seed(10)).to(d).requires_grad_(True)
        out = p3d.interpolate_face_attributes(m["p2f"], bary, attrs)
        (out ** 2).sum().backward()
        _busy(2)
        grads.append((attrs.grad.clone(), bary.grad.clone()))
    for a, b in zip(grads[0], grads[1]):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)
    p = point_scene(8)
    for fn in (p3d.alpha_composite, p3d.norm_weighted_sum, p3d.weighted_sum):
        grads = []
        for _ in range(2):
            feats = p["feats"].t().detach().clone().requires_grad_(True)
            alphas = (1 - p["dists"] * p["inv_r2"]).clamp(0, 1).permute(0, 3, 1, 2).detach().requires_grad_(True)
            img = fn(p["idx"].long().permute(0, 3, 1, 2), alphas, feats)
            (img ** 2).sum().backward()
            grads.append((feats.grad.clone(), alphas.grad.clone()))
        for a, b in zip(grads[0], grads[1]):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    del gen


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. full size: the bench batch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_full_size_bench_batch():
    """64 meshes, 512^2, K = 8, the bench generator and its upstream gradients: gated as in 3., bit-equal
    over two runs, both forms."""
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    d = _dev()
    B, H, K = 64, 512, 8
    verts, faces = U.hetero_batch(B, seed=0, torus_div=U.CONFIG3_TORUS_DIV)
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces])
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    F = int(fv.shape[0])
    first, count = m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh()
    nbr = torch.full((F,), -1, dtype=torch.int64, device=d)
    with _flag(False):
        p2f = _C.rasterize_meshes(fv, first, count, nbr, (H, H), SOFTRAS_BLUR, K, 32, int(max(10000, F / 5)), True, True, False)[0]
    gen = torch.Generator().manual_seed(231)  # bench.py's upstream gradients (rank 0)
    gz = torch.randn((B, H, H, K), generator=gen).to(d)
    gb = torch.randn((B, H, H, K, 3), generator=gen).to(d)
    gd = torch.randn((B, H, H, K), generator=gen).to(d)
    a = _C.rasterize_meshes_backward(fv, p2f, gz, gb, gd, True, True)
    b = _C.rasterize_meshes_backward(fv, p2f.clone(), gz, gb, gd, True, True)
    assert torch.equal(a, b)
    V = m.verts_packed().shape[0]
    va = _C._mesh_backward(fv, m.faces_packed(), V, p2f, gz, gb, gd, True, True, None)
    vb = _C._mesh_backward(fv, m.faces_packed(), V, p2f, gz, gb, gd, True, True, None)
    assert torch.equal(va, vb)
    del b, vb
    torch.cuda.empty_cache()
    with _flag(False):
        atomic = _C.rasterize_meshes_backward(fv, p2f, gz, gb, gd, True, True)
        worst = U.assert_face_grads_vs_truth("ordered backward, bench batch", a, fv, p2f, gz, gb, gd, True, True, reference=atomic)
        worst_v = U.assert_face_grads_vs_truth("ordered backward to the vertices, bench batch", va, fv, p2f, gz, gb, gd, True, True,
                                               faces=m.faces_packed(), num_verts=V)
    print(f"[ordered, bench batch: {F} faces, {int((p2f >= 0).sum())} samples] largest |error| / scale: (F,3,3) {worst:.3e}, (V,3) {worst_v:.3e} "
          f"(gate 5e-3); words that differ from the atomic result: {int((atomic != a).sum())} of {a.numel()}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        print(_child_digest(sys.argv[2]))
