"""The VolumeSampler without a GPU: the torch formulation and a float32 restatement of the kernels' contract through the fixture's
gates, deliberately wrong variants refused by the same gates, the C ABI's status codes without a launch, the build list, the
kernel_path decisions.  Cases, inputs and gates: tests/volume_sampler_case.py; fixture: tests/golden/volume_sampler_ref.npz."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import volume_sampler_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _lib, volume_sampler  # noqa: E402

CASES = C.cases()
ENTRIES = ("p3di_volume_sample_forward", "p3di_volume_sample_backward", "p3di_volume_sample_workspace_bytes", "p3di_volume_sample_keys",
           "p3di_volume_sample_ordered_backward")


def restated(dens, feats, o, d, l, sample_mode="bilinear", padding_mode="zeros", align_corners=True, wrong=None):
    """csrc/implicit_abi.h's contract of the VolumeSampler in torch, differentiated by autograd: the source index per axis, the border
    clamp with its zeroed gradient, the empty sample under zeros padding, eight corners in ATen's order with the weights (wx wy) wz.
    `wrong` switches one mistake in: swap_xz, flip_align, trunc, border_grad, half_away."""
    pts = o[..., None, :] + l[..., :, None] * d[..., None, :]
    N = pts.shape[0]
    D, H, W = dens.shape[2:]
    align = (not align_corners) if wrong == "flip_align" else align_corners
    axes = (2, 1, 0) if wrong == "swap_xz" else (0, 1, 2)
    idx, w, inside = [], [], []
    for a, S in zip(axes, (W, H, D)):
        c = pts[..., a]
        i = ((c + 1) / 2) * (S - 1) if align else ((c + 1) * S - 1) / 2
        ok = torch.ones_like(i, dtype=torch.bool)
        if padding_mode == "border":
            clamped = torch.nan_to_num(i.detach(), nan=0.0, posinf=float(S - 1), neginf=0.0).clamp(0, S - 1)
            free = (i.detach() > 0) & (i.detach() < S - 1)
            i = clamped + (i - i.detach()) if wrong == "border_grad" else torch.where(free, i, clamped)
            i = torch.where(torch.isfinite(i), i, clamped)
        else:
            ok = torch.isfinite(i) & (i.abs() < 2.0e9)
            i = torch.where(ok, i, torch.full_like(i, -5.0))
        if sample_mode == "nearest":
            r = (torch.sign(i) * torch.floor(i.abs() + 0.5) if wrong == "half_away" else torch.round(i)).detach()
            idx.append((r.long(), r.long() + 1))
            w.append((torch.ones_like(i), torch.zeros_like(i)))
        else:
            f = (torch.trunc(i) if wrong == "trunc" else torch.floor(i)).detach()
            idx.append((f.long(), f.long() + 1))
            w.append((((f + 1) - i), (i - f)))
        inside.append(tuple(ok & (k >= 0) & (k < S) for k in idx[-1]))

    def sample(vol):
        if vol is None:
            return pts.new_zeros(pts.shape[:-1] + (0,))
        vol = vol.expand(N, *vol.shape[1:])
        out = pts.new_zeros((N, vol.shape[1]) + tuple(pts.shape[1:-1]))
        for k in range(1 if sample_mode == "nearest" else 8):
            kx, ky, kz = k & 1, (k >> 1) & 1, k >> 2
            m = inside[0][kx] & inside[1][ky] & inside[2][kz]
            x, y, z = idx[0][kx].clamp(0, W - 1), idx[1][ky].clamp(0, H - 1), idx[2][kz].clamp(0, D - 1)
            vals = torch.stack([vol[n][:, z[n], y[n], x[n]] for n in range(N)])  # (N, C, ...)
            weight = (w[0][kx] * w[1][ky]) * w[2][kz]
            out = out + torch.where(m[:, None], vals * weight[:, None], torch.zeros_like(vals))
        return out.movedim(1, -1)

    return sample(dens), sample(feats)


def test_fixture_holds_every_case_and_the_cases_hold_every_size():
    fix = C.fixture()
    for case in CASES:
        for q in C.QUANTITIES:
            assert (C.key(case.id, q) in fix) == (case.Cf is not None or "features" not in q), (case.id, q)
    assert os.path.getsize(C.FIXTURE) < 2 ** 20
    assert {(c.mode, c.padding, c.align) for c in CASES if c.kind == "rays"} == set(C.MODES) and len(C.MODES) == 8
    for kind in ("rays", "edges", "lattice"):
        assert {(c.mode, c.padding, c.align) for c in CASES if c.kind == kind} == set(C.MODES)
    assert {c.P for c in CASES} >= set(C.RAY_P) and {c.grid for c in CASES} >= set(C.GRIDS)
    assert {c.Cf for c in CASES} >= set(C.FEATURE_DIMS) and {c.Cd for c in CASES} == {1, 2} and {c.N for c in CASES} == {1, 2, 3}
    assert any(c.R == 257 for c in CASES) and any(c.shared and c.N == 3 for c in CASES)
    assert all(0.0 < C.e_ref(q) < 2e-6 for q in C.QUANTITIES)
    for case in CASES:
        _, _, o, d, l, _, _ = C.inputs(case)
        assert C.clear_of_planes(case, o, d, l), case.id


def test_edge_and_lattice_cases_hold_what_they_promise():
    edge = C.inputs(C.case_by_id("edges-bil-zer-ac"))[2]
    flat = edge.reshape(-1)
    assert not torch.isnan(C.inputs(C.case_by_id("edges-bil-bor-ac"))[2]).any() and C.nan_equals_minus_inf_under_border(restated) == []
    assert torch.isnan(flat).any() and torch.isposinf(flat).any() and torch.isneginf(flat).any() and (flat == 1.0).any() and (flat == -1.0).any()
    assert (flat.abs() >= 1e10).any()
    for a in range(3):
        assert not torch.isfinite(edge[..., a]).all() and (edge[..., a] == 1.0).any()
    for case in (c for c in CASES if c.kind == "lattice"):
        _, _, o, d, l, _, _ = C.inputs(case)
        dist, same = C.plane_clearance(case, o, d, l)
        assert same.all() and (dist == 0.0).any(), case.id  # exact, and on planes (voxels, or ties in nearest mode)
    _, _, o, d, l, _, _ = C.inputs(C.case_by_id("collide"))
    p = o[:, :, None] + l[..., None] * d[:, :, None]
    cells = torch.floor(torch.stack([(p[..., 0] + 1) / 2 * 4, (p[..., 1] + 1) / 2 * 3, (p[..., 2] + 1) / 2 * 2], -1))
    assert (cells == cells.reshape(-1, 3)[0]).all()  # one voxel cell for all 256 points


def test_torch_formulation_and_restatement_pass_the_gates():
    assert C.failures(CASES, volume_sampler.sample_volumes_torch) == []
    assert C.failures(CASES, A.sample_volumes) == []  # CPU tensors: the chain
    assert C.failures(CASES, restated) == []


def test_lattice_cases_are_bit_equal_to_grid_sample():
    fix = C.fixture()
    for case in (c for c in CASES if c.kind == "lattice"):
        dens, feats, o, d, l, _, _ = C.inputs(case)
        for fn in (volume_sampler.sample_volumes_torch, restated):
            with torch.no_grad():
                rd, rf = fn(dens, feats, o, d, l, sample_mode=case.mode, padding_mode=case.padding, align_corners=case.align)
            assert C.same_bits(rd.numpy(), fix[C.key(case.id, "f32_densities")]) and C.same_bits(rf.numpy(), fix[C.key(case.id, "f32_features")]), case.id


@pytest.mark.parametrize("wrong", ["swap_xz", "flip_align", "trunc", "border_grad", "half_away"])
def test_wrong_variants_are_refused_by_the_gates(wrong):
    def fn(*args, **kwargs):
        return restated(*args, wrong=wrong, **kwargs)

    bad = C.failures(CASES, fn)
    assert bad, wrong
    kinds = {C.case_by_id(cid).kind for cid, _, _, _ in bad}
    if wrong == "border_grad":
        assert all(C.case_by_id(cid).padding == "border" and q in ("grad_origins", "grad_directions", "grad_lengths") for cid, q, _, _ in bad)
    if wrong == "half_away":
        assert all(C.case_by_id(cid).mode == "nearest" for cid, _, _, _ in bad) and "lattice" in kinds
    if wrong == "trunc":
        assert all(C.case_by_id(cid).mode == "bilinear" for cid, _, _, _ in bad)


def _world():
    case, fix = C.case_by_id("world"), C.fixture()
    dens, feats, _, _, _, _, _ = C.inputs(case)
    wo, wd, wl = C.world_rays()
    return case, C.MatrixVolumes(dens, feats, torch.from_numpy(fix["world/matrix"])), C.RayBundle(wo, wd, wl, None)


def test_volume_sampler_forward_is_the_whole_module_on_the_world_case():
    case, volumes, bundle = _world()
    fix = C.fixture()
    o, d = volume_sampler.local_rays(volumes, bundle.origins, bundle.directions, bundle.lengths.shape[0])
    assert C.same_bits(o.numpy(), fix["world/origins_local"]) and C.same_bits(d.numpy(), fix["world/directions_local"])

    def whole(dens, feats, o_, d_, l_, sample_mode, padding_mode, align_corners):
        return A.volume_sampler_forward(C.MatrixVolumes(dens, feats, volumes._matrix), C.RayBundle(bundle.origins, bundle.directions, l_, None),
                                        sample_mode, padding_mode)

    forward_only = ("rays_densities", "rays_features", "grad_densities", "grad_features", "grad_lengths")
    assert C.failures([case], whole, quantities=forward_only) == []

    def with_translation(dens, feats, o_, d_, l_, sample_mode, padding_mode, align_corners):  # the directions through the FULL transform
        wrong_d = volumes.world_to_local_coords(bundle.directions)
        return volume_sampler.sample_volumes_torch(dens, feats, o_, wrong_d, l_, sample_mode=sample_mode, padding_mode=padding_mode,
                                                   align_corners=align_corners)

    assert C.failures([case], with_translation, quantities=forward_only)


def test_reference_checks_and_messages():
    case, volumes, bundle = _world()
    with pytest.raises(ValueError, match="have to have the same number of dimensions"):
        A.volume_sampler_forward(volumes, C.RayBundle(bundle.origins, bundle.directions, bundle.lengths[0], None))
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        A.volume_sampler_forward(volumes, C.RayBundle(bundle.origins[0], bundle.directions[0], bundle.lengths[0], None))
    with pytest.raises(ValueError, match="may differ only in the last dimension"):
        A.volume_sampler_forward(volumes, C.RayBundle(bundle.origins, bundle.directions[:, :4], bundle.lengths, None))
    with pytest.raises(ValueError, match="has to be 3"):
        A.volume_sampler_forward(volumes, C.RayBundle(bundle.origins[..., :2], bundle.directions[..., :2], bundle.lengths, None))
    with pytest.raises(ValueError, match="same batch size as rays"):
        A.volume_sampler_forward(volumes, C.RayBundle(bundle.origins[:1], bundle.directions[:1], bundle.lengths[:1], None))
    dens, _, o, d, l, _, _ = C.inputs(C.case_by_id("rays-shared-N3-nearest"))
    rd, rf = A.sample_volumes(dens, None, o.view(3, 2, 2, 3), d.view(3, 2, 2, 3), l.view(3, 2, 2, 5))
    assert rd.shape == (3, 2, 2, 5, 1) and rf.shape == (3, 2, 2, 5, 0)


def test_kernel_path_decisions():
    dens, feats, o, d, l, _, _ = C.inputs(C.case_by_id("rays-shared-N3"))
    kp = volume_sampler.kernel_path
    assert not kp(dens, feats, o, d, l)  # CPU
    meta = [t.to("meta") for t in (dens, feats, o, d, l)]
    assert not kp(*meta)
    before = dict(volume_sampler.CALLS)
    A.sample_volumes(dens, feats, o, d, l, padding_mode="reflection")
    A.sample_volumes(dens.double(), feats.double(), o.double(), d.double(), l.double())
    assert volume_sampler.CALLS["chain"] == before["chain"] + 2 and volume_sampler.CALLS["fused"] == before["fused"]

    class Fake:  # what kernel_path asks of a tensor, answered as a float32 GPU tensor would
        def __init__(self, t, dtype=torch.float32):
            self.shape, self.dtype, self.is_cuda, self.device, self._dim = t.shape, dtype, True, "cuda:0", t.dim()

        def dim(self):
            return self._dim

    real_is_tensor = torch.is_tensor
    torch.is_tensor = lambda t: isinstance(t, Fake) or real_is_tensor(t)
    try:
        f = [Fake(t) for t in (dens, feats, o, d, l)]
        assert kp(*f) and kp(f[0], None, *f[2:]) and kp(*f, "nearest", "border")
        assert not kp(*f, "bicubic", "zeros") and not kp(*f, "bilinear", "reflection")
        assert not kp(Fake(dens, torch.float64), *f[1:]) and not kp(f[0], Fake(feats, torch.float16), *f[2:])
        assert not kp(Fake(dens.expand(2, *dens.shape[1:])), *f[1:])  # a batch of 2 against rays of 3
        assert not kp(f[0], f[1], f[2], f[3], Fake(l[:, :2]))
    finally:
        torch.is_tensor = real_is_tensor


def test_c_abi_status_codes_without_a_launch_and_lists():
    lib = _lib.load()
    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    from pytorch3d_amd import build

    assert "volume_sample.hip" in build.SOURCES and not any("volume_sample" in k for k in build.AGPR_KERNELS_TESTED)
    assert (_lib.VOLUME_SAMPLE_NEAREST, _lib.VOLUME_SAMPLE_BORDER, _lib.VOLUME_SAMPLE_CORNERS) == (1, 2, 4) and _lib.VOLUME_SAMPLE_MAX_GROUPS >= 1
    p = torch.zeros(64).data_ptr()
    st = (ctypes.c_int64 * 5)(60, 60, 20, 5, 1)
    neg = (ctypes.c_int64 * 5)(60, 60, -20, 5, 1)

    def fwd(N=1, R=1, P=1, Cd=1, Cf=1, D=3, H=4, W=5, dens=p, feats=p, o=p, d=p, l=p, flags=4, out_d=p, out_f=p, strides=st):
        return lib.p3di_volume_sample_forward(dens, strides, feats, st, Cd, Cf, D, H, W, o, d, l, N, R, P, flags, out_d, out_f, None)

    def bwd(N=1, R=1, P=1, Cd=1, Cf=1, D=3, H=4, W=5, g=p, dens=p, o=p, l=p, gd=p, go=None, gstr=st):
        return lib.p3di_volume_sample_backward(g, g, dens, st, p, st, Cd, Cf, D, H, W, o, p, l, N, R, P, 4, gd, gstr, None, st, go, None, None, None)

    def ordered(N=1, R=1, P=1, D=3, H=4, W=5, shared=0, ws=p, nbytes=1 << 30, keys=p, n_sorted=None):
        return lib.p3di_volume_sample_ordered_backward(p, p, 1, 1, D, H, W, shared, p, p, p, N, R, P, 4, keys, p, N * R * P * 8 if n_sorted is None else n_sorted, p, st, p, st, ws, nbytes, None)

    for zero in ({"N": 0}, {"R": 0}, {"P": 0}):  # no launch: runs without a GPU
        assert fwd(dens=None, o=None, out_d=None, **zero) == _lib.OK and bwd(g=None, o=None, **zero) == _lib.OK and ordered(keys=None, **zero) == _lib.OK
        assert lib.p3di_volume_sample_keys(3, 4, 5, 0, None, None, None, zero.get("N", 1), zero.get("R", 1), zero.get("P", 1), 4, None, None) == _lib.OK
    for bad in ({"D": 0}, {"H": 0}, {"W": -1}, {"N": -1}, {"R": -2}, {"P": -1}, {"Cd": 0}, {"Cf": -1}):
        assert fwd(**bad) == _lib.ERR_INVALID_ARG and bwd(**bad) == _lib.ERR_INVALID_ARG, bad
    for missing in ({"dens": None}, {"o": None}, {"feats": None}, {"out_d": None}, {"out_f": None}, {"d": None}, {"flags": 8}, {"strides": neg}):
        assert fwd(**missing) == _lib.ERR_INVALID_ARG, missing
    assert fwd(P=2, l=None) == _lib.ERR_INVALID_ARG  # lengths == NULL means P == 1
    assert bwd(g=None) == _lib.ERR_INVALID_ARG and bwd(o=None) == _lib.ERR_INVALID_ARG and bwd(gstr=neg) == _lib.ERR_INVALID_ARG
    assert bwd(gd=None, go=p, dens=None) == _lib.ERR_INVALID_ARG  # ray gradients read the volumes
    assert bwd(gd=None, go=None) == _lib.OK  # nothing asked for
    assert ordered(D=0) == _lib.ERR_INVALID_ARG and ordered(keys=None) == _lib.ERR_INVALID_ARG
    assert ordered(n_sorted=9) == _lib.ERR_INVALID_ARG and ordered(n_sorted=-1) == _lib.ERR_INVALID_ARG and ordered(n_sorted=0) == _lib.OK
    need = lib.p3di_volume_sample_workspace_bytes(2, 3, 65, 1, 1)  # (ordered() passes Cd = Cf = 1: one chunk of four channels)
    assert lib.p3di_volume_sample_workspace_bytes(2, 3, 65, 1, 4) > need >= (2 * 3 * 65 * 8 // 64) * 2 * 4 * 4 and lib.p3di_volume_sample_workspace_bytes(0, 3, 65, 1, 4) == 0
    assert ordered(N=2, R=3, P=65, nbytes=need - 1) == _lib.ERR_WORKSPACE and ordered(N=2, R=3, P=65, ws=None) == _lib.ERR_WORKSPACE
    big = 1 << 11
    assert ordered(D=big, H=big, W=big) == _lib.ERR_UNSUPPORTED and ordered(N=1 << 20, R=1 << 10, P=1) == _lib.ERR_UNSUPPORTED
    assert lib.p3di_volume_sample_keys(big, big, big, 1, p, p, p, 1, 1, 1, 4, p, None) == _lib.ERR_UNSUPPORTED
    from pytorch3d_amd import _C

    assert _C.volume_sample_fits(1, 128, 128, 128, 10, 16384, 150) and not _C.volume_sample_fits(1, big, big, big, 1, 1, 1)
    assert not _C.volume_sample_fits(1, 8, 8, 8, 1 << 20, 1 << 10, 1)


def test_shim_lists_the_patch():
    from pytorch3d_amd import shim

    assert any(m == "pytorch3d.renderer.implicit.renderer" and fn is shim._volume_sampler for m, _, fn in shim._FUNCTION_PATCHES)
    assert "VolumeSampler.forward" in shim.__doc__ and A.sample_volumes is volume_sampler.sample_volumes
