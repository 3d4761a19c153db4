"""vert_align on the GPU: csrc/vert_align.hip against the reference's chain (F.grid_sample and copies, restated in
pytorch3d_amd.vert_align.vert_align_torch and run on the CPU) BIT FOR BIT on lattice inputs -- every map size, channel width, wave
packing, mode and layout --, against the reference's recorded results (tests/golden/mesh_refine_ref.npz) through the gates of
tests/mesh_refine_case.py, the ordered backward under torch.use_deterministic_algorithms(True), a hot pixel, non-finite coordinates,
and a refinement stage built from the unmodified reference classes through the shim."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import mesh_refine_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _C

VA = importlib.import_module("pytorch3d_amd.vert_align")  # (the package re-exports the FUNCTION vert_align over the sub-module)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")

MAPS = ((1, 1), (1, 5), (5, 9), (8, 8), (14, 14))
CHANNELS = (1, 3, 4, 5, 64, 65, 260)
BATCHES = (1, 3)
VERTS = (1, 63, 64, 65, 130)
MODE_IDS = ["%s-%s-%s" % (i, p, "ac" if a else "nc") for i, p, a in C.VA_MODES]


def _both(feats, verts, grad_out, modes, return_packed=False, to_dev=lambda t: t.to(DEV)):
    """({out, gverts, gf...} on the GPU through p3d.vert_align, the same on the CPU through the reference's chain)."""
    res = []
    for fn, move in ((p3d.vert_align, to_dev), (VA.vert_align_torch, lambda t: t)):
        leaves = [move(t).requires_grad_(True) for t in [verts] + list(feats)]
        out = fn(leaves[1:], leaves[0], return_packed, *modes)
        grads = torch.autograd.grad(out, leaves, move(grad_out))
        res.append(dict(zip(["out", "gverts"] + ["gf%d" % i for i in range(len(feats))], (out,) + grads)))
    return res


def _equal(got, want, where):
    for q in want:
        assert got[q].shape == want[q].shape and torch.equal(got[q].cpu(), want[q]), (where, q, (got[q].cpu() - want[q]).abs().max().item())


@pytest.mark.parametrize("name", C.va_cases())
def test_fixture_cases_through_the_gates(name):
    before = VA.CALLS["fused"]
    got = C.run_va(name, p3d.vert_align, DEV)
    assert VA.CALLS["fused"] == before + 1 and got["out"].device == DEV
    assert C.gate(name, got, show=print) == []


@pytest.mark.parametrize("modes", C.VA_MODES, ids=MODE_IDS)
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: "%dx%d" % hw)
def test_kernel_equals_the_chain_bit_for_bit_on_the_lattice(hw, modes):
    H, W = hw
    gen = torch.Generator().manual_seed(H * 100 + W)
    before = VA.CALLS["fused"]
    for C_ in CHANNELS:
        for N in BATCHES:
            for V in VERTS:
                feat = C.features((N, C_, H, W), "lattice", gen)
                verts = C.lattice_coords((N, V, 3), gen)
                grad_out = C.features((N, V, C_), "lattice", gen)
                got, want = _both([feat], verts, grad_out, modes)
                _equal(got, want, (C_, N, V))
                assert (got["gverts"][..., 2] == 0).all()  # z
                if modes[0] == "nearest":
                    assert (got["gverts"] == 0).all()
                if modes[1] == "border" and modes[2]:  # align_corners: |c| >= 1 is at or beyond an end -- clipped, gradient 0
                    clipped = (verts[..., :2].abs() >= 1).to(DEV)
                    assert (got["gverts"][..., :2][clipped] == 0).all()
    assert VA.CALLS["fused"] == before + len(CHANNELS) * len(BATCHES) * len(VERTS)  # every combination took the kernels


@pytest.mark.parametrize("modes", C.VA_MODES, ids=MODE_IDS)
def test_layouts_are_read_through_their_strides(modes):
    gen = torch.Generator().manual_seed(9)
    N, V, H, W = 3, 65, 5, 9
    verts = C.lattice_coords((N, V, 3), gen)
    for C_ in (3, 4, 64, 260):
        feat = C.features((N, C_, H, W), "lattice", gen)
        grad_out = C.features((N, V, C_), "lattice", gen)
        want = _both([feat], verts, grad_out, modes)[1]
        wide = torch.full((N, C_ + 9, H, W), float("nan"))
        wide[:, 5:5 + C_] = feat
        wide_cl = wide.to(DEV).contiguous(memory_format=torch.channels_last)
        layouts = {"nchw": feat.to(DEV), "channels_last": feat.to(DEV).contiguous(memory_format=torch.channels_last),
                   "slice": wide.to(DEV)[:, 5:5 + C_], "slice_channels_last": wide_cl[:, 5:5 + C_]}
        assert layouts["slice"].storage_offset() > 0 and not layouts["slice"].is_contiguous()
        for label, f in layouts.items():
            leaves = [verts.to(DEV).requires_grad_(True), f.detach().requires_grad_(True)]
            out = p3d.vert_align(leaves[1], leaves[0], False, *modes)
            gv, gf = torch.autograd.grad(out, leaves, grad_out.to(DEV))
            _equal({"out": out, "gverts": gv, "gf0": gf}, want, (label, C_))


def test_three_maps_write_their_column_blocks_of_one_output():
    gen = torch.Generator().manual_seed(10)
    N, V = 2, 65
    feats = [C.features((N, c, h, w), "lattice", gen) for c, h, w in ((3, 5, 9), (64, 8, 8), (5, 14, 14))]
    feats[1] = feats[1].contiguous(memory_format=torch.channels_last)  # (its block starts at column 3: the dword path all the same)
    big = torch.full((N, V, 4), float("nan"))
    big[..., :3] = C.lattice_coords((N, V, 3), gen)
    grad_out = C.features((N, V, 72), "lattice", gen)
    for modes in (("bilinear", "zeros", True), ("bilinear", "border", False), ("nearest", "zeros", False)):
        got, want = _both(feats, big[..., :3], grad_out, modes, to_dev=lambda t: t.to(DEV))  # verts: a slice of an (N, V, 4) tensor
        _equal(got, want, modes)


class _FakeMeshes:
    def __init__(self, padded, sizes):
        self.padded, self.sizes = padded, sizes

    def verts_padded(self):
        return self.padded

    def verts_padded_to_packed_idx(self):
        V = self.padded.shape[1]
        return torch.cat([torch.arange(s) + i * V for i, s in enumerate(self.sizes)]).to(self.padded.device)


class _FakeClouds:
    def __init__(self, padded):
        self.padded = padded

    def points_padded(self):
        return self.padded


@pytest.mark.parametrize("modes", [("bilinear", "zeros", True), ("bilinear", "border", False), ("nearest", "border", True)])
def test_packed_rows_come_straight_from_the_index_and_padding_is_never_read(modes):
    gen = torch.Generator().manual_seed(11)
    N, V, sizes = 3, 70, [70, 1, 33]
    feat = C.features((N, 5, 8, 8), "lattice", gen)
    clean = C.lattice_coords((N, V, 3), gen)
    poisoned = clean.clone()
    for i, s in enumerate(sizes):
        poisoned[i, s:] = float("nan")
    grad_out = C.features((sum(sizes), 5), "lattice", gen)
    idx = _FakeMeshes(clean, sizes).verts_padded_to_packed_idx()
    # the CPU chain on the clean padding (the poisoned one would put NaN into its gradients through 0 * NaN)
    leaves = [clean.clone().requires_grad_(True), feat.clone().requires_grad_(True)]
    want_out = VA.vert_align_torch(leaves[1], _FakeMeshes(leaves[0], sizes), True, *modes)
    want_gv, want_gf = torch.autograd.grad(want_out, leaves, grad_out)
    dl = [poisoned.to(DEV).requires_grad_(True), feat.to(DEV).requires_grad_(True)]
    out = p3d.vert_align(dl[1], _FakeMeshes(dl[0], sizes), True, *modes)
    gv, gf = torch.autograd.grad(out, dl, grad_out.to(DEV))
    assert out.shape == (sum(sizes), 5) and torch.equal(out.cpu(), want_out) and torch.equal(gf.cpu(), want_gf)
    keep = torch.zeros(N * V, dtype=torch.bool)
    keep[idx] = True
    assert torch.equal(gv.cpu().reshape(-1, 3)[keep], want_gv.reshape(-1, 3)[keep]) and (gv.cpu().reshape(-1, 3)[~keep] == 0).all()
    # a Pointclouds-like object: every padded row
    cloud_out = p3d.vert_align(feat.to(DEV), _FakeClouds(clean.to(DEV)), True, *modes)
    assert torch.equal(cloud_out.cpu(), VA.vert_align_torch(feat, _FakeClouds(clean), True, *modes))


def _hot_pixel(kind, gen, interp):
    V = 5000
    feat = C.features((1, 4, 2, 2), kind, gen)
    verts = torch.full((1, V, 3), -1.0)  # bilinear, align_corners: source (0, 0) -- nw weighs 1, the other three corners 0 and in range
    if kind == "random":
        verts[..., :2] += torch.rand((1, V, 2), generator=gen) * 0.5
    return feat, verts, C.features((1, V, 4), kind, gen), (interp, "zeros", True)


def test_hot_pixel_atomic_form_within_the_reference_error():
    gen = torch.Generator().manual_seed(12)
    feat, verts, grad_out, modes = _hot_pixel("random", gen, "bilinear")
    before = dict(_C.VERT_ALIGN_CALLS)
    got, want32 = _both([feat], verts, grad_out, modes)
    assert _C.VERT_ALIGN_CALLS["atomic"] == before["atomic"] + 1 and _C.VERT_ALIGN_CALLS["ordered"] == before["ordered"]
    leaves = [verts.double().requires_grad_(True), feat.double().requires_grad_(True)]
    out64 = VA.vert_align_torch(leaves[1], leaves[0], False, *modes)
    gv64, gf64 = torch.autograd.grad(out64, leaves, grad_out.double())
    for q, w64 in (("out", out64.detach()), ("gverts", gv64), ("gf0", gf64)):
        ref_err = (want32[q].double() - w64).abs().max().item()  # the chain's own float32 error on this input
        tol = max(C.MARGIN * ref_err, C.ulp32(w64.abs().max()))
        err = (got[q].cpu().double() - w64).abs().max().item()
        print("hot pixel %s: %.3g from float64 (the chain: %.3g, bound %.3g)" % (q, err, ref_err, tol))
        assert err <= tol


@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
def test_ordered_form_runs_under_the_deterministic_flag_with_the_same_bits(interp):
    gen = torch.Generator().manual_seed(13)
    feat, verts, grad_out, modes = _hot_pixel("lattice", gen, interp)
    want = _both([feat], verts, grad_out, modes)[1]
    before = dict(_C.VERT_ALIGN_CALLS)
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for stream in (None, None, None, torch.cuda.Stream(DEV)):
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(stream):
                leaves = [verts.to(DEV).requires_grad_(True), feat.to(DEV).requires_grad_(True)]
                out = p3d.vert_align(leaves[1], leaves[0], False, *modes)
                gv, gf = torch.autograd.grad(out, leaves, grad_out.to(DEV))
            if stream is not None:
                stream.synchronize()
            runs.append({"out": out, "gverts": gv, "gf0": gf})
    finally:
        torch.use_deterministic_algorithms(False)
    assert _C.VERT_ALIGN_CALLS["ordered"] == before["ordered"] + 4 and _C.VERT_ALIGN_CALLS["atomic"] == before["atomic"]
    for r in runs:
        _equal(r, want, interp)  # 5000 samples of one pixel: 78 waves in one segment, summed by pass 2 of ordered_sum.h
    # a general case too: random coordinates over a 14 x 14 map, three runs with the same bits
    feat = torch.randn((2, 5, 14, 14), generator=gen).to(DEV)
    verts = (torch.rand((2, 700, 3), generator=gen) * 2.5 - 1.25).to(DEV)
    go = torch.randn((2, 700, 5), generator=gen).to(DEV)
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for _ in range(3):
            f = feat.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(p3d.vert_align(f, verts, False, *modes), f, go)
            grads.append(g)
    finally:
        torch.use_deterministic_algorithms(False)
    f = feat.clone().requires_grad_(True)
    (atomic,) = torch.autograd.grad(p3d.vert_align(f, verts, False, *modes), f, go)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    assert (grads[0] - atomic).abs().max().item() <= 1e-4 * atomic.abs().max().item()


@pytest.mark.parametrize("modes", C.VA_MODES, ids=MODE_IDS)
def test_non_finite_coordinates_give_the_documented_rows(modes):
    gen = torch.Generator().manual_seed(14)
    nan, inf = float("nan"), float("inf")
    feat = C.features((1, 5, 5, 9), "lattice", gen)
    verts = C.lattice_coords((1, 12, 3), gen)
    clean = verts.clone()
    for row, (x, y) in enumerate(((nan, 0.0), (inf, 0.25), (-inf, 0.0), (1e30, 0.5), (0.0, nan), (-1e30, inf))):
        verts[0, 2 * row, 0], verts[0, 2 * row, 1] = x, y
    odd = torch.arange(1, 12, 2)
    grad_out = C.features((1, 12, 5), "lattice", gen)
    leaves = [verts.to(DEV).requires_grad_(True), feat.to(DEV).requires_grad_(True)]
    out = p3d.vert_align(leaves[1], leaves[0], False, *modes)
    gv, gf = torch.autograd.grad(out, leaves, grad_out.to(DEV))
    want = C.contract_vert_align([feat], verts, grad_out, *modes)  # the documented contract, restated on the CPU
    assert torch.equal(out.cpu(), want["out"]) and torch.equal(gv.cpu(), want["gverts"]) and torch.equal(gf.cpu(), want["gf0"])
    assert torch.isfinite(out).all() and torch.isfinite(gv).all() and torch.isfinite(gf).all()
    if modes[1] == "zeros":
        assert (out[0, ::2] == 0).all() and (gv[0, ::2] == 0).all()
    # the neighbouring rows are what they are without the bad ones
    ref = VA.vert_align_torch(feat, clean, False, *modes)
    assert torch.equal(out.cpu()[0, odd], ref[0, odd])


def test_wide_maps_without_adjacent_channels_take_the_ordered_form_by_default():
    gen = torch.Generator().manual_seed(16)
    verts = C.lattice_coords((2, 65, 3), gen).to(DEV)
    edge = _C.VERT_ALIGN_STRIDED_ORDERED_MIN_C
    for C_, layout, path in ((edge, "nchw", "ordered"), (edge - 1, "nchw", "atomic"), (2 * edge, "channels_last", "atomic")):
        feat = C.features((2, C_, 5, 9), "lattice", gen).to(DEV)
        if layout == "channels_last":
            feat = feat.contiguous(memory_format=torch.channels_last)
        feat.requires_grad_(True)
        before = dict(_C.VERT_ALIGN_CALLS)
        p3d.vert_align(feat, verts).sum().backward()
        other = "atomic" if path == "ordered" else "ordered"
        assert _C.VERT_ALIGN_CALLS[path] == before[path] + 1 and _C.VERT_ALIGN_CALLS[other] == before[other], (C_, layout)


def test_unsupported_inputs_take_the_chain_on_the_gpu():
    gen = torch.Generator().manual_seed(15)
    feat, verts = torch.randn((2, 3, 5, 9), generator=gen).to(DEV), (torch.rand((2, 9, 3), generator=gen) * 2 - 1).to(DEV)
    before = dict(VA.CALLS)
    assert p3d.vert_align(feat, verts, padding_mode="reflection").shape == (2, 9, 3)
    assert p3d.vert_align(feat.double(), verts.double()).dtype == torch.float64
    assert VA.CALLS["chain"] == before["chain"] + 2 and VA.CALLS["fused"] == before["fused"]
    with pytest.raises(ValueError, match="inconsistent batch dimension"):
        p3d.vert_align(feat[:1], verts)
    assert p3d.vert_align(feat, verts[:, :0]).shape == (2, 0, 3) and p3d.vert_align(feat[:, :0], verts).shape == (2, 9, 0)


def test_refinement_stage_through_the_shim():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_mesh_refine_case.py"), "cuda:0"], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["plain_leaves_vert_align_alone"] and rec["patched"]
    assert rec["stage_misses"] == [] and rec["stage_fallback_calls"] == 0
    assert rec["stage_fused_calls"] == {"vert_align": 1, "GraphConv.forward": 3}
    assert rec["restored"]
