"""Camera gradients through the fused world -> NDC transform: p3d_transform_backward_cameras against a
float64 restatement, its bits across calls and streams, the autograd nodes that return it, the L2 entry and the drop-in.

Tolerance per matrix entry e (kernel against float64):   |got - g64| <= 2 * E32 + D * 2^-24 * S[e]
  E32   the largest error of the float32 torch formulation (transform_points_reference + autograd) on the same input
        against the same float64, measured here; twice, because the kernel multiplies by 1 / w where torch divides;
  D     the depth of the kernel's summation tree (csrc/transform.hip, restated by rasterize_meshes.camera_grad_tree_depth);
  S[e]  the float64 sum of the absolute per-vertex contributions to e: D * 2^-24 * S is the first-order bound of a
        summation of that depth."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "one_vertex": (1,),
    "v63": (63,),
    "v64": (64,),
    "v65": (65,),
    "inside_across_border": (5, 130, 64),
    "empty_middle": (40, 0, 40),
    "stage2_loops": (64 * 300 + 7,),
}


def _dev():
    return torch.device("cuda:0")


def _matrices(kind, n):
    """(n, 4, 4) world -> view and view -> NDC, float64 on the CPU, row-vector convention; every mesh its own pair."""
    if kind == "perspective":
        g = np.load(os.path.join(U.GOLDEN, "cow_ref.npz"))
        a0, b0 = torch.from_numpy(g["world_to_view"]).double(), torch.from_numpy(g["projection"]).double()
    else:
        gen = torch.Generator().manual_seed(7)
        a0 = torch.eye(4, dtype=torch.float64)
        a0[:3, :3] = U.random_rotation(gen).double()
        a0[3, :3] = torch.tensor([0.1, -0.2, 3.0], dtype=torch.float64)
        # orthographic: x, y scaled and shifted, w == 1
        b0 = torch.tensor([[1 / 1.5, 0, 0, 0], [0, 1 / 1.2, 0, 0], [0, 0, 0.1, 0], [0.05, -0.03, -0.1, 1]], dtype=torch.float64)
    a, b = a0[None].repeat(n, 1, 1), b0[None].repeat(n, 1, 1)
    for i in range(n):
        a[i, 3, 0] += 0.1 * i
        a[i, 3, 2] += 0.3 * i
        b[i, 0, 0] *= 1.0 + 0.05 * i
    return a, b


def _case(counts, kind, shared):
    """Inputs of one layout on the device (float32) and the float64 truth: what autograd gives through
    transform_points_reference in double, the float32 torch error E32 and the sums S of absolute contributions."""
    from pytorch3d_amd.rasterize_meshes import transform_points_reference

    d = _dev()
    counts_t = torch.tensor(counts, dtype=torch.int64)
    V, N = int(counts_t.sum()), len(counts)
    num = 1 if shared else N
    first = torch.cumsum(counts_t, 0) - counts_t
    idx = torch.repeat_interleave(torch.arange(N), counts_t)
    gen = torch.Generator().manual_seed(231)
    g_ndc = torch.randn(V, 3, generator=gen)
    verts = torch.randn(V, 3, generator=gen) * 0.4
    a64, b64 = _matrices(kind, num)
    mats = torch.stack([a64, b64], 1).float().contiguous()  # (num, 2, 4, 4): the kernel's input
    a64, b64 = mats[:, 0].double(), mats[:, 1].double()      # the truth starts from the SAME float32 values

    def torch_route(dtype):
        a, b = a64.to(dtype).clone().requires_grad_(True), b64.to(dtype).clone().requires_grad_(True)
        ndc = transform_points_reference(verts.to(dtype), idx if num > 1 else torch.zeros(V, dtype=torch.int64), a, b)
        ga, gb = torch.autograd.grad(ndc, [a, b], g_ndc.to(dtype))
        return torch.stack([ga, gb], 1).double()

    if V:
        g64, g32 = torch_route(torch.float64), torch_route(torch.float32)
    else:
        g64 = g32 = torch.zeros(num, 2, 4, 4, dtype=torch.float64)
    # the per-vertex contributions by hand in float64 (the formulas of DESIGN 8.9): their sum must be autograd's, their absolute sum is S
    seg = idx if num > 1 else torch.zeros(V, dtype=torch.int64)
    p = torch.cat([verts.double(), torch.ones(V, 1, dtype=torch.float64)], 1)
    A, B = a64[seg], b64[seg]
    vh = torch.bmm(p[:, None], A)[:, 0]
    view = torch.cat([vh[:, :3] / vh[:, 3:], torch.ones(V, 1, dtype=torch.float64)], 1)
    nh = torch.bmm(view[:, None], B)[:, 0]
    gx, gy, gz = g_ndc.double().unbind(1)
    w = nh[:, 3]
    gn = torch.stack([gx / w, gy / w, torch.zeros_like(w), -(gx * nh[:, 0] + gy * nh[:, 1]) / (w * w)], 1)
    gv = torch.einsum("vj,vij->vi", gn, B[:, :3, :])
    gv[:, 2] += gz
    gh = torch.cat([gv / vh[:, 3:], -((gv * vh[:, :3]).sum(1) / (vh[:, 3] * vh[:, 3]))[:, None]], 1)
    contrib = torch.stack([p[:, :, None] * gh[:, None, :], view[:, :, None] * gn[:, None, :]], 1)  # (V, 2, 4, 4)
    by_hand = torch.zeros(num, 2, 4, 4, dtype=torch.float64).index_add_(0, seg, contrib)
    S = torch.zeros(num, 2, 4, 4, dtype=torch.float64).index_add_(0, seg, contrib.abs())
    assert torch.allclose(by_hand, g64, rtol=1e-9, atol=1e-12 * float(S.max()) if V else 0.0), "the restatement disagrees with autograd"
    return {"V": V, "N": N, "num": num, "verts": verts.to(d), "first": first.to(d), "mats": mats.to(d), "g_ndc": g_ndc.to(d),
            "g64": g64, "E32": float((g32 - g64).abs().max()), "S": S,
            "count": V if shared else int(counts_t.max())}


def _run_kernel(c, want_verts=True, stream=None, workspace_bytes=None):
    """p3d_transform_backward_cameras on the case -> (grad_verts_world or None, grad_matrices, return code)."""
    from pytorch3d_amd import _C, _lib

    lib, d = _lib.load(), _dev()
    V, N, num = c["V"], c["N"], c["num"]
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(d):
        need = lib.p3d_transform_backward_workspace_bytes(V, N, num)
        nbytes = need if workspace_bytes is None else workspace_bytes
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=d)
        gw = torch.full((V, 3), float("nan"), device=d) if want_verts else None
        gm = torch.full((num, 2, 4, 4), float("nan"), device=d)
        rc = lib.p3d_transform_backward_cameras(_C._ptr(c["verts"]), _C._ptr(c["first"]), _C._ptr(c["mats"]), _C._ptr(c["g_ndc"]), V, N, num,
                                                _C._ptr(gw), _C._ptr(gm), _C._ptr(ws), nbytes, _C._stream(d))
    if stream is not None:
        stream.synchronize()
    return gw, gm, rc


def _assert_within_bound(tag, got, c):
    from pytorch3d_amd.rasterize_meshes import camera_grad_tree_depth

    D = camera_grad_tree_depth(c["count"])
    err = (got.detach().double().cpu() - c["g64"]).abs()
    bound = 2 * c["E32"] + D * 2.0 ** -24 * c["S"]
    worst = int(torch.argmax(err / bound.clamp_min(1e-300)))  # the entry that uses most of its bound
    print(f"[camera grad] {tag}: E32 {c['E32']:.3e}, kernel error {float(err.max()):.3e}, D {D}, "
          f"tightest entry: error {float(err.flatten()[worst]):.3e} <= bound {float(bound.flatten()[worst]):.3e}")
    assert bool((err <= bound).all()), f"{tag}: {int((err > bound).sum())} entries beyond the bound"


def _launched(fn):
    """Names of the library's launches during fn()."""
    from pytorch3d_amd import _lib

    lib = _lib.load()
    lib.p3d_profile_reset()
    lib.p3d_profile_enable(1)
    try:
        out = fn()
    finally:
        lib.p3d_profile_enable(0)
    names = set(_lib.profile_snapshot())
    lib.p3d_profile_reset()
    return out, names


@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_kernel_vs_float64_restatement(layout, kind):
    from pytorch3d_amd import _C, _lib

    counts = LAYOUTS[layout]
    for shared in ((False, True) if len(counts) > 1 else (False,)):
        c = _case(counts, kind, shared)
        gw, gm, rc = _run_kernel(c)
        assert rc == 0
        _assert_within_bound(f"{layout} {kind} num_matrices={c['num']}", gm, c)
        assert bool((gm[:, 1, :, 2] == 0).all()), "column 2 of grad_B is not exactly 0"
        if not shared:
            for n, cnt in enumerate(counts):
                if cnt == 0:
                    assert bool((gm[n] == 0).all()), "an empty mesh must get an exactly zero row"
        # the vertex gradient of the same pass: the bits of p3d_transform_verts_backward
        want = torch.empty((c["V"], 3), device=_dev())
        _lib.check(_lib.load().p3d_transform_verts_backward(_C._ptr(c["verts"]), _C._ptr(c["first"]), _C._ptr(c["mats"]), _C._ptr(c["g_ndc"]),
                                                            c["V"], c["N"], c["num"], _C._ptr(want), _C._stream(_dev())), "verts_backward")
        assert torch.equal(gw, want)
        # ... and a null grad_verts_world skips it without changing a bit of the matrices
        _, gm2, rc2 = _run_kernel(c, want_verts=False)
        assert rc2 == 0 and torch.equal(gm2, gm)


def test_no_vertices_no_launch_all_zero():
    c = _case((0,), "perspective", False)
    (gw, gm, rc), names = _launched(lambda: _run_kernel(c))
    assert rc == 0 and names == set(), names
    assert bool((gm == 0).all())
    c3 = _case((0, 0, 0), "orthographic", False)
    _, gm3, rc3 = _run_kernel(c3)
    assert rc3 == 0 and gm3.shape == (3, 2, 4, 4) and bool((gm3 == 0).all())


@pytest.mark.parametrize("layout", ["inside_across_border", "stage2_loops"])
def test_same_bits_on_every_call_and_stream(layout):
    c = _case(LAYOUTS[layout], "perspective", False)
    _, first_call, rc = _run_kernel(c)
    assert rc == 0
    _, second_call, _ = _run_kernel(c)
    torch.cuda.synchronize()
    _, other_stream, _ = _run_kernel(c, stream=torch.cuda.Stream(_dev()))
    assert torch.equal(first_call, second_call) and torch.equal(first_call, other_stream)
    torch.use_deterministic_algorithms(True)
    try:
        _, det, rc = _run_kernel(c)
        # the autograd node neither refuses nor takes another route in this mode
        from pytorch3d_amd.rasterize_meshes import _TransformVerts

        mats = c["mats"].clone().requires_grad_(True)
        _TransformVerts.apply(c["verts"], c["first"], mats).backward(c["g_ndc"])
    finally:
        torch.use_deterministic_algorithms(False)
    assert rc == 0 and torch.equal(det, first_call) and torch.equal(mats.grad, first_call)


@pytest.mark.parametrize("shared", [False, True])
def test_autograd_returns_the_matrix_gradient(shared):
    from pytorch3d_amd.rasterize_meshes import _TransformVerts

    c = _case(LAYOUTS["inside_across_border"], "perspective", shared)
    mats = c["mats"].clone().requires_grad_(True)
    verts = c["verts"].clone().requires_grad_(True)
    out = _TransformVerts.apply(verts, c["first"], mats)
    out.backward(c["g_ndc"])
    assert mats.grad is not None and mats.grad.shape == mats.shape
    _assert_within_bound(f"autograd num_matrices={c['num']}", mats.grad, c)
    gw, gm, _ = _run_kernel(c)
    assert torch.equal(verts.grad, gw) and torch.equal(mats.grad, gm)
    # frozen cameras: today's call, the same vertex gradient
    v2 = c["verts"].clone().requires_grad_(True)
    (out2, names) = _launched(lambda: _TransformVerts.apply(v2, c["first"], c["mats"]).backward(c["g_ndc"]))
    assert "transform_verts_bwd" in names and not any(n.startswith("transform_cameras_bwd") for n in names), names
    assert torch.equal(v2.grad, gw)


def test_short_workspace_is_refused_before_any_launch():
    c = _case(LAYOUTS["inside_across_border"], "perspective", False)
    from pytorch3d_amd import _lib

    need = _lib.load().p3d_transform_backward_workspace_bytes(c["V"], c["N"], c["num"])
    assert need >= (math.ceil(c["V"] / 64) + c["N"]) * 128
    (gw, gm, rc), names = _launched(lambda: _run_kernel(c, workspace_bytes=need - 16))
    assert rc == -1 and names == set(), (rc, names)  # P3D_ERR_INVALID_ARG
    assert bool(torch.isnan(gm).all()) and bool(torch.isnan(gw).all()), "outputs were written"
    (_, gm, rc), names = _launched(lambda: _run_kernel(c))
    assert rc == 0 and names == {"transform_cameras_bwd_partial", "transform_cameras_bwd_reduce"}, names


# ---------------------------------------------------------------------------------------------------------------------
# L2: rasterize_meshes_world with matrices that require grad
# ---------------------------------------------------------------------------------------------------------------------
def _l2_scene(d):
    v0, f0 = U.ico_sphere(2)
    v1, f1 = U.torus(0.35, 0.9, 10, 14)
    gen = torch.Generator().manual_seed(3)
    w2v = torch.eye(4)[None].repeat(2, 1, 1)
    w2v[0, :3, :3] = U.random_rotation(gen)
    w2v[1, :3, :3] = U.random_rotation(gen)
    w2v[0, 3, :3] = torch.tensor([0.05, -0.1, 2.7])
    w2v[1, 3, :3] = torch.tensor([-0.15, 0.1, 3.0])
    f = 1.0 / math.tan(math.radians(60.0) / 2.0)
    v2n = torch.zeros(2, 4, 4)
    for n, s in enumerate((1.0, 1.15)):  # (x, y, z, 1) @ v2n = (f x, f y, z, z): a pinhole
        v2n[n, 0, 0] = v2n[n, 1, 1] = f * s
        v2n[n, 2, 2] = v2n[n, 2, 3] = 1.0
    return [v0.to(d), (v1 * 0.9).to(d)], [f0.to(d), f1.to(d)], w2v.to(d), v2n.to(d)


@pytest.mark.parametrize("shared_projection", [False, True])
def test_l2_world_entry_is_one_fused_path_with_camera_gradients(shared_projection):
    import pytorch3d_amd as p3d
    from pytorch3d_amd.rasterize_meshes import _PackedVertsView, transform_points_reference

    d = _dev()
    verts, faces, w2v0, v2n0 = _l2_scene(d)
    if shared_projection:
        v2n0 = v2n0[:1]
    sigma = 1e-4
    # (plain NDC barycentrics: the perspective-correct ones have a vanishing denominator just outside faces seen edge-on, one such
    # sample makes an entry of 1e18 and "5e-4 * the largest entry" then compares nothing else)
    kw = dict(image_size=48, blur_radius=math.log(1.0 / 1e-4 - 1.0) * sigma, faces_per_pixel=4, perspective_correct=False,
              clip_barycentric_coords=True)

    def leaves():
        return ([v.clone().requires_grad_(True) for v in verts], w2v0.clone().requires_grad_(True), v2n0.clone().requires_grad_(True))

    vl, w2v, v2n = leaves()
    out, names = _launched(lambda: p3d.rasterize_meshes_world(p3d.PackedMeshes(vl, faces), w2v, v2n, **kw))
    assert "transform_gather_face_verts" in names, names  # the one-node path, not the torch formulation
    frozen = p3d.rasterize_meshes_world(p3d.PackedMeshes(verts, faces), w2v0, v2n0, **kw)
    for a, b in zip(out, frozen):
        assert torch.equal(a.detach(), b)
    assert 0.05 < float((out[0][..., 0] >= 0).float().mean()) < 0.9
    gen = torch.Generator().manual_seed(231)
    g1, g2, g3 = (torch.randn(o.shape, generator=gen).to(d) for o in (out[1], out[3], out[2]))
    got = torch.autograd.grad([out[1], out[3], out[2]], [w2v, v2n] + vl, [g1, g2, g3])  # sum zbuf g1 + sum dists g2 + sum bary g3

    vl2, w2v2, v2n2 = leaves()
    m2 = p3d.PackedMeshes(vl2, faces)
    ndc = transform_points_reference(m2.verts_packed(), m2.verts_packed_to_mesh_idx(), w2v2, v2n2)
    o2 = p3d.rasterize_meshes(_PackedVertsView(m2, ndc), **kw)
    want = torch.autograd.grad([o2[1], o2[3], o2[2]], [w2v2, v2n2] + vl2, [g1, g2, g3])
    for name, a, b in zip(["world_to_view", "view_to_ndc", "verts[0]", "verts[1]"], got, want):
        assert a.shape == b.shape
        scale = float(b.abs().max())
        close = torch.isclose(a, b, rtol=5e-3, atol=5e-4 * scale)
        print(f"[camera grad L2] {name}: largest entry {scale:.3e}, max |fused - torch route| {float((a - b).abs().max()):.3e}, "
              f"entries beyond rtol 5e-3 / atol 5e-4 * largest: {int((~close).sum())} / {close.numel()}")
        assert bool(close.all()), name


# ---------------------------------------------------------------------------------------------------------------------
# drop-in: the unmodified reference classes with cameras that require grad, in a process of their own
# ---------------------------------------------------------------------------------------------------------------------
def test_shim_keeps_the_fused_paths_for_cameras_that_require_grad():
    res = subprocess.run([sys.executable, os.path.join(U.ROOT, "tests", "shim_camera_grad_case.py")], capture_output=True, text=True,
                         timeout=300, cwd=U.ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    j = json.loads([line for line in res.stdout.splitlines() if line.startswith("{")][-1])
    if "skipped" in j:
        pytest.skip(j["skipped"])
    print(json.dumps(j))
    kept = "MeshRasterizer.forward: no vertex behind z_clip, un-clipped fused path kept"
    assert j["mesh_fov_T"]["calls"][kept] == [1, 0] and kept not in j["mesh_fov_T_zclip"]["calls"]
    for case, patch in (("mesh_fov_T", "MeshRasterizer.forward"), ("mesh_fov_T_zclip", "MeshRasterizer.forward"),
                        ("mesh_perspective_focal", "MeshRasterizer.forward"), ("points_T", "PointsRenderer.forward")):
        rec = j[case]
        assert rec["calls"][patch] == [1, 0], (case, rec["calls"])  # the fused branch ran, no fallback
        assert rec["grad_finite"] and rec["grad_max"] > 0.0, case
        assert rec["beyond_tolerance"] == 0, (case, rec)
