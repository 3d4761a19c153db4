"""sample_points_from_meshes on the HIP kernels of csrc/sample_points.hip against tests/golden/sample_points_ref.npz (the reference's
own code on recorded uniforms) and the float64 restatement of tests/sample_points_case.py, through the gates the CPU tests use
(sample_points_case.gate_*: tests/test_cpu_sample_points.py shows that they reject a lower-bound choice, the 1e-6 clamp and swapped
weights).  Gates: sample_face_idxs equal to the golden, samples equal to it BIT FOR BIT, bary bit-equal to the torch formulation;
normals, textures and gradients within four times the largest error the float32 torch formulation makes on the CPU against the float64
truth; the table within D(F) 2^-24 total of the float64 prefix sums of the same float32 areas, D(F) = 19 + 4 ceil(ceil(F / 256) / 256)
(csrc/sample_points.hip), and the kernel's choice EXACTLY the host's searchsorted on that same table -- accuracy is gated against
float64 and selection against the gated table, so no share of samples is left out; the star (300 samples on one face) within in-degree
x 2^-23 x the largest term.
"""
import contextlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import sample_points_case as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_CAP = 4096 * 256  # csrc/p3d_common.h: stream_blocks -- one pass of a grid-stride loop


def _dev():
    return torch.device("cuda:0")


def _p3d():
    import pytorch3d_amd as p3d

    return p3d


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _poison(N, S):
    d = _dev()
    nan = float("nan")
    return (torch.full((N, S, 3), nan, device=d), torch.full((N, S, 3), nan, device=d), torch.full((N, S), -7, dtype=torch.int64, device=d),
            torch.full((N, S, 3), nan, device=d))


def _run(verts, faces, first, nf, S, u, return_normals=True, table=None):
    """The tensor-level function on the GPU into poisoned outputs -> numpy (samples, normals, idx, bary)."""
    d = _dev()
    out = _p3d().sample_points_packed(verts.to(d), faces.to(d), first.to(d), nf.to(d), S, u.to(d), return_normals, _table_out=table,
                                      _out=_poison(int(nf.numel()), S))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


# ---- 1. the ragged batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", C.SAMPLE_COUNTS)
def test_ragged_batch_matches_the_golden(S):
    p3d, d = _p3d(), _dev()
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    u = torch.from_numpy(g["uniforms_%d" % S])
    samples, normals, idx, bary = _run(verts, faces, first, nf, S, u)

    class WithFeatures(p3d.PackedMeshes):  # per-vertex features as textures, interpolated by the package's kernel
        textures = torch.from_numpy(g["features"]).to(d)

        def sample_textures(self, fragments):
            return p3d.interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, self.textures[self.faces_packed()])

    verts_list, faces_list = C.ragged_batch()
    meshes = WithFeatures([v.to(d) for v in verts_list], [f.to(d) for f in faces_list])
    s2, textures = p3d.sample_points_from_meshes(meshes, S, return_textures=True, uniforms=u.to(d))
    assert C.bits_equal(s2.cpu().numpy(), samples)
    C.gate_ragged(S, samples, normals, idx, bary, textures.cpu().numpy(), g)


# ---- 2. edge uniforms --------------------------------------------------------------------------------------------------------------
def test_edge_uniforms():
    verts, faces = C.edge_mesh()
    u = C.edge_uniforms()
    samples, normals, idx, _ = _run(verts, faces, torch.tensor([0]), torch.tensor([faces.shape[0]]), u.shape[1], u)
    C.gate_edges(u, samples, normals, idx)


# ---- 3. / 4. the table, its levels and the loops ---------------------------------------------------------------------------------------
def _gate_table(verts, faces, first, nf, u, idx, table):
    """The table read back from the workspace: non-decreasing inside a mesh, restarting at each mesh, within D(F) 2^-24 total of the
    float64 prefix sums of the kernels' own float32 areas; and the choice exactly the host's searchsorted on that table."""
    areas32 = _p3d().face_areas_normals(verts.to(_dev()), faces.to(_dev()))[0].cpu().numpy()  # the same arithmetic, by contract
    C.gate_table(areas32, faces, first, nf, u, idx, table)


def test_table_of_the_ragged_batch():
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    u = C.uniforms(5, 4099, 31)
    table = []
    _, _, idx, _ = _run(verts, faces, first, nf, u.shape[1], u, table=table)
    _gate_table(verts, faces, first, nf, u, idx, table[0].cpu().numpy())


def _soup(F, V, seed):
    gen = torch.Generator().manual_seed(seed)
    verts = torch.rand(V, 3, generator=gen) * 2 - 1
    a = torch.randint(0, V, (F,), generator=gen)
    b = (a + 1 + torch.randint(0, V - 2, (F,), generator=gen)) % V
    c = torch.where((a + 1) % V == b, (a + 2) % V, (a + 1) % V)
    return verts, torch.stack([a, b, c], 1)


def test_every_scan_level_runs_its_second_round():
    """Level 1 is one block of kScanBlock = 256 faces; level 2 scans the ceil(F / 256) block records in rounds of 256, so its second
    round begins at F > 256 * 256 = 65 536 faces in the batch, and the grid-stride loops of the finish kernels (4096 blocks of 256
    lanes: csrc/p3d_common.h stream_blocks) go round again at F > 1 048 576.  The batch: 37 faces, then ONE mesh of 1 048 576 + 2 * 256 + 77
    faces (4 099 block records: 17 rounds of level 2, a second pass of the finish loops), then 300 faces and one face -- the meshes'
    boundaries fall at packed faces 37 (inside the first wave), 1 049 202 (lane 50 of wave 1 of a block) and 1 049 502.  The backward
    runs its per-face finish over the same F."""
    big = GRID_CAP + 2 * C.SCAN_BLOCK + 77
    counts = [37, big, 300, 1]
    verts_list, faces_list = zip(*[_soup(n, 50 + n // 4, 40 + i) for i, n in enumerate(counts)])
    verts, faces, first, nf = C.pack(list(verts_list), list(faces_list))
    assert (int(first[2]) % C.SCAN_BLOCK) // 64 == 1 and int(first[2]) % 64 == 50 and C.scan_depth(faces.shape[0]) == 19 + 4 * 17
    S = 513
    u = C.uniforms(4, S, 32)
    table = []
    samples, normals, idx, bary = _run(verts, faces, first, nf, S, u, table=table)
    _gate_table(verts, faces, first, nf, u, idx, table[0].cpu().numpy())
    w = C.weights64(u.numpy())
    # |v| <= 1 and the weights sum to 1: a weight carries at most three roundings (sqrt, 1 - u2, the product), a product one more and
    # the two sums one each -- 6 x 2^-24 in all; twice that is the gate
    assert np.abs(samples - C.samples64(verts, faces, idx, w)).max() <= 12 * 2.0 ** -24
    # the backward over the same F: the per-face finish and the vertex scatter
    d = _dev()
    x = verts.to(d).requires_grad_(True)
    s, n, i2, b2 = _p3d().sample_points_packed(x, faces.to(d), first.to(d), nf.to(d), S, u.to(d), True)
    gen = torch.Generator().manual_seed(6)
    gs, gn = torch.randn(4, S, 3, generator=gen), torch.randn(4, S, 3, generator=gen)
    torch.autograd.backward([s, n], [gs.to(d), gn.to(d)])
    C.gate_grads(verts, faces, i2.cpu().numpy(), b2.cpu().numpy(), x.grad.cpu().numpy(), gs, gn, "second rounds")


def test_sample_count_past_the_grid_cap():
    """One pass of the sampling kernel's grid-stride loop covers 4096 x 256 = 1 048 576 samples: 2 meshes x 524 588 samples go round again."""
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    sel = torch.tensor([1, 3])
    S = GRID_CAP // 2 + 300
    u = C.uniforms(2, S, 33)
    table = []
    samples, normals, idx, bary = _run(verts, faces, first[sel], nf[sel], S, u, table=table)
    t = table[0].cpu().numpy()
    rows32 = [t[int(a):int(a) + int(n)] for a, n in zip(first[sel].tolist(), nf[sel].tolist())]
    assert np.array_equal(idx, C.choose(rows32, first[sel].tolist(), u[:, :, 0].numpy(), dtype=np.float32))
    w32 = C.formulation_weights32(u.numpy())
    assert C.bits_equal(bary, w32)
    f = faces[torch.from_numpy(idx)]
    wt = torch.from_numpy(w32)
    want = (wt[..., 0:1] * verts[f[..., 0]] + wt[..., 1:2] * verts[f[..., 1]]) + wt[..., 2:3] * verts[f[..., 2]]
    assert C.bits_equal(samples, want.numpy())
    truth = C.normals64(verts, faces, idx)
    assert np.abs(normals - truth).max() <= C.measure(C.formulation_normals32(verts, faces, idx), truth)


# ---- 5. the distribution -------------------------------------------------------------------------------------------------------------
def test_distribution_follows_the_areas():
    verts, faces = C.areas_mesh()
    S = 200000
    u = C.uniforms(1, S, 21)  # the inputs that pass on the torch formulation alone (tests/test_cpu_sample_points.py)
    _, _, idx, _ = _run(verts, faces, torch.tensor([0]), torch.tensor([12]), S, u, return_normals=False)
    C.gate_distribution(idx, C.areas64(verts, faces))


# ---- 6. gradients ------------------------------------------------------------------------------------------------------------------
def _grad(verts, faces, first, nf, u, gs, gn, ordered=False, stream=None):
    d = _dev()
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx, _flag(ordered):
        x = verts.to(d).requires_grad_(True)
        samples, normals, idx, bary = _p3d().sample_points_packed(x, faces.to(d), first.to(d), nf.to(d), u.shape[1], u.to(d), gn is not None)
        outs, grads = [], []
        if gs is not None:
            outs.append(samples), grads.append(gs.to(d))
        if gn is not None:
            outs.append(normals), grads.append(gn.to(d))
        torch.autograd.backward(outs, grads)
        if stream is not None:
            stream.synchronize()
    torch.cuda.synchronize()
    return x.grad.cpu(), idx.cpu().numpy(), bary.cpu().numpy()


def _ragged_grad_inputs(which):
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    u = torch.from_numpy(g["uniforms_257"])
    gen = torch.Generator().manual_seed(5)
    gs = torch.randn(5, 257, 3, generator=gen) if which != "normals" else None
    gn = torch.randn(5, 257, 3, generator=gen) if which != "samples" else None
    return verts, faces, first, nf, u, gs, gn


def _profiled(fn):
    from pytorch3d_amd import _lib

    _lib.load().p3d_profile_reset()
    _lib.load().p3d_profile_enable(1)
    try:
        out = fn()
        ran = set(_lib.profile_snapshot())
    finally:
        _lib.load().p3d_profile_enable(0)
        _lib.load().p3d_profile_reset()
    return out, ran


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("which", ["samples", "normals", "both"])
def test_gradients_against_the_float64_restatement(which, ordered):
    verts, faces, first, nf, u, gs, gn = _ragged_grad_inputs(which)
    (got, idx, w), ran = _profiled(lambda: _grad(verts, faces, first, nf, u, gs, gn, ordered))
    C.gate_grads(verts, faces, idx, w, got.numpy(), gs, gn, which + (" ordered" if ordered else " atomic"))
    # the path taken, by the names the built-in timing records
    atomic = {"sample_points_face_sums", "scatter_face_grads"}
    in_order = {"sample_points_face_sums_ordered_pass1", "sample_points_face_sums_ordered_pass2", "scatter_face_grads_ordered_pass1"}
    assert "sample_points_backward_finish" in ran and "sample_points_forward" in ran and "sample_points_cdf" in ran
    assert (in_order <= ran and not (atomic & ran)) if ordered else (atomic <= ran and not (in_order & ran)), sorted(ran)


@pytest.mark.parametrize("ordered", [False, True])
def test_star_gradient_within_its_bound(ordered):
    verts, faces, u, gs = C.star()
    got, idx, w = _grad(verts, faces, torch.tensor([0]), torch.tensor([1]), u, gs, None, ordered)
    C.gate_star(idx, w, got.numpy())


def test_ordered_backward_gives_the_same_bits_on_two_runs_and_two_streams():
    verts, faces, first, nf, u, gs, gn = _ragged_grad_inputs("both")
    star = C.star()
    torch.cuda.synchronize()
    for args in ((verts, faces, first, nf, u, gs, gn), (star[0], star[1], torch.tensor([0]), torch.tensor([1]), star[2], star[3], None)):
        one = _grad(*args, ordered=True)[0]
        again = _grad(*args, ordered=True)[0]
        other = _grad(*args, ordered=True, stream=torch.cuda.Stream(device=_dev()))[0]
        assert torch.equal(one, again) and torch.equal(one, other)
    # with the flag off the call neither raises nor warns
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _grad(verts, faces, first, nf, u, gs, gn, ordered=False)


# ---- 7. the public function and the patch ----------------------------------------------------------------------------------------------
def _packed_meshes():
    d = _dev()
    verts_list, faces_list = C.ragged_batch()
    return _p3d().PackedMeshes([v.to(d) for v in verts_list], [f.to(d) for f in faces_list])


def test_value_errors_tuple_orders_and_generator():
    p3d, d, S = _p3d(), _dev(), 33
    empty = p3d.PackedMeshes([torch.rand(3, 3, device=d)], [torch.zeros((0, 3), dtype=torch.int64, device=d)])
    with pytest.raises(ValueError, match="Meshes are empty."):
        p3d.sample_points_from_meshes(empty, S)
    m = _packed_meshes()
    with pytest.raises(ValueError, match="Meshes do not contain textures."):
        p3d.sample_points_from_meshes(m, S, return_textures=True)
    bad = m.update_verts_packed(m.verts_packed().clone())
    bad.verts_packed()[5, 2] = float("inf")
    with pytest.raises(ValueError, match="Meshes contain nan or inf."):
        p3d.sample_points_from_meshes(bad, S)
    out = p3d.sample_points_from_meshes(bad, S, return_face_idxs=True, check_finite=False)  # mesh 1 holds the vertex: zero rows, no fault
    assert out[0].shape == (5, S, 3) and bool((out[1][1] == -1).all()) and not out[0][1].any() and bool((out[1][3] >= 0).all())
    u = C.uniforms(5, S, 1).to(d)
    s = p3d.sample_points_from_meshes(m, S, uniforms=u)
    s1, n1 = p3d.sample_points_from_meshes(m, S, True, uniforms=u)
    s2, n2, i2 = p3d.sample_points_from_meshes(m, S, return_normals=True, uniforms=u, return_face_idxs=True)
    assert torch.is_tensor(s) and torch.equal(s, s1) and torch.equal(s, s2) and torch.equal(n1, n2) and i2.dtype == torch.int64
    a = p3d.sample_points_from_meshes(m, S, generator=torch.Generator(device=d).manual_seed(7))
    b = p3d.sample_points_from_meshes(m, S, generator=torch.Generator(device=d).manual_seed(7))
    c = p3d.sample_points_from_meshes(m, S, generator=torch.Generator(device=d).manual_seed(8))
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(3)
    e = p3d.sample_points_from_meshes(m, S)
    torch.manual_seed(3)
    assert torch.equal(e, p3d.sample_points_from_meshes(m, S))


def test_check_finite_off_never_waits_for_the_device():
    p3d, d = _p3d(), _dev()
    m = _packed_meshes()
    x = m.verts_packed().clone().requires_grad_(True)
    m = m.update_verts_packed(x)
    gen = torch.Generator(device=d).manual_seed(1)
    p3d.sample_points_from_meshes(m, 64, True, check_finite=False, generator=gen)  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s, n = p3d.sample_points_from_meshes(m, 257, return_normals=True, check_finite=False, generator=gen)
        (s.sum() + n.sum()).backward()
        with pytest.raises(RuntimeError):  # the default keeps the reference's check, and that one waits
            p3d.sample_points_from_meshes(m, 257, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


def test_shim_patches_sample_points_from_meshes():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_sample_points_case.py"), "cuda:0"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["patched_everywhere"] and rec["restored"]
    assert rec["golden_ok"], rec.get("golden_error")
    assert rec["fused_calls"] == 4 and rec["fallback_calls"] == 0
