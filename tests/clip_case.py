"""Cases, seeded inputs, a torch restatement and the gates of the clipping tests (csrc/clip.hip; pytorch3d_amd/clip.py).

A CLIP case is clip_faces on (F, 3, 3) float32 faces, the mesh tables and a frustum, with a seeded gradient into face_verts alone,
into barycentric_conversion alone and into both.  A CONVERT case runs convert_clipped_rasterization_to_original_faces on S synthetic
samples of the clipped faces of the case seeded-persp (clip_faces -> convert, one chain), with a seeded gradient into the un-clipped
barycentrics, taken back to the clipped barycentrics, to a detached barycentric_conversion made a leaf of a rebuilt ClippedFaces, and
(S = 257 and 4096) to face_verts with nothing else feeding the loss.

The fixture tests/golden/clip_cases_ref.npz (tests/golden/make_golden_clip_cases.py) holds, from the reference's own clip.py:
* the index tables of every case, complete (float32 and float64 classify alike: every threshold is a number float32 holds exactly);
* the float64 TRUTH of every float quantity on the rows held(n) selects -- all of them up to 64 rows, beyond that the first and last
  16, 32 evenly spaced ones and the rows around index 1024.  A megabyte does not hold all 45 convert cases and the 2049-face scan
  case in float64; truth(case) therefore is clip_faces_torch / convert_clipped_torch below in float64, and asserts on every call that
  it equals the fixture on the held rows to 1e-12 of each row's scale and that the tables are the fixture's;
* E_ref/<quantity>: the largest error of the reference's float32 run against its float64 run over ALL rows of ALL cases, relative
  to that face's or row's largest |truth| (face_verts, barycentric_conversion, grad_face_verts, grad_conversion,
  grad_face_verts_from_samples) or to the case's largest |truth| (bary_unclipped, grad_bary_clipped).  grad_face_verts is measured
  on the clip cases (all three gradient modes); the gradient that reaches face_verts from the samples alone, whose float32 sums over
  the samples of a row cancel in gw2, has an E_ref of its own so that it does not widen the gate of the others;
* for the onplane cases (dyadic values: float32 arithmetic is exact) the reference's float32 outputs, equal to the truth bit for bit;
* the reference pipeline's outputs and its own residual of the un-clipping invariant on the two pipeline scenes.
E_ref as recorded:  face_verts 3.5e-07  barycentric_conversion 1.2e-07  grad_face_verts 1.6e-06  grad_conversion 3.2e-06
                    grad_face_verts_from_samples 2.2e-05  bary_unclipped 1.1e-07  grad_bary_clipped 1.5e-07
Gate per face or row: |got - truth| <= 4 E_ref max|truth of that face or row|; a face or row whose truth is exactly zero must come
back exactly zero (removed faces, rows no sample touches).  Per sample: |got - truth| <= 4 E_ref max|truth of the case|.

Kinds of clip cases (the smallest shapes that reach each thing):
  branch   hand-built faces for every lone vertex i1 in (0, 1, 2) x (case 3, case 4), twice each, kept and removed faces between
           them; once with perspective_correct and once without
  onplane  vertices exactly at z == z_clip (in front: w is exactly 0 or 1), pairs of vertices with equal z; dyadic throughout
  cull     all six planes with, per plane, a face only the reference's reading culls (the coordinates of vertex number `axis`) and
           one only the intended reading would (coordinate `axis` of the three vertices); cull=False with the planes set; NaN and
           +-inf in z and in x (tables and the finite neighbours only are gated there)
  meshes   empty first, middle and last mesh (first[n] == F: the reference indexes out of range there, so the generator runs it
           without the trailing empty meshes and records (F_clipped, 0) for them); a mesh whose faces all go; N = 1; nothing left
  scan     F in (1, 1023, 1024, 1025, 2049) with a case-4 face at index 1023 and a case-2 face at index 1024
  seeded   400 faces straddling the plane with perspective_correct and culling, 400 without
Not reached by any test: more than 4 * 8192 waves in the convert backward, which needs more than 134 million samples.
"""
import collections
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "clip_cases_ref.npz")
SEED = 20241021
GATE_FACTOR = 4.0
Z03 = float(np.float32(0.3))
BLOCK_QUANTITIES = ("face_verts", "barycentric_conversion", "grad_face_verts", "grad_conversion", "grad_face_verts_from_samples")
SAMPLE_QUANTITIES = ("bary_unclipped", "grad_bary_clipped")
GRAD_MODES = ("fv", "conv", "both")
TABLES = ("mesh_to_face_first_idx", "num_faces_per_mesh", "faces_clipped_to_unclipped_idx", "faces_clipped_to_conversion_idx",
          "clipped_faces_neighbor_idx")
FIELDS = ("face_verts",) + TABLES[:3] + ("barycentric_conversion",) + TABLES[3:]
WRONGS = ("keep_w3", "swap_w_persp", "drop_g2_second", "conv_untransposed", "drop_gconv_w2")
SCAN_F = (1, 1023, 1024, 1025, 2049)
CONVERT_S = (1, 63, 64, 65, 257, 4095, 4096, 4097, 20000)
PATTERNS = ("random", "onerow", "tworows", "fresh", "kept")

Case = collections.namedtuple("Case", "id kind arg frustum")
ConvertCase = collections.namedtuple("ConvertCase", "id base S pattern to_verts")
Impl = collections.namedtuple("Impl", "clip_faces convert frustum clipped")


def frustum(**kw):
    out = dict(left=None, right=None, top=None, bottom=None, znear=None, zfar=None, perspective_correct=False, cull=True, z_clip_value=None)
    out.update(kw)
    return out


BOX = dict(left=-1.0, right=1.0, top=-1.0, bottom=1.0)
SIX = dict(BOX, znear=0.5, zfar=1.0)


def cases():
    out = [Case("branch-persp", "branch", None, frustum(perspective_correct=True, z_clip_value=Z03, **BOX)),
           Case("branch-flat", "branch", None, frustum(z_clip_value=0.5)),
           Case("onplane-persp", "onplane", None, frustum(perspective_correct=True, z_clip_value=0.25)),
           Case("onplane-flat", "onplane", None, frustum(z_clip_value=0.25)),
           Case("cull-six", "cull", "finite", frustum(z_clip_value=0.25, **SIX)),
           Case("cull-off", "cull", "finite", frustum(z_clip_value=0.25, cull=False, **SIX)),
           Case("cull-only", "cull", "front", frustum(**SIX)),
           Case("cull-nonfinite", "cull", "nonfinite", frustum(z_clip_value=0.25, perspective_correct=True, **SIX))]
    for name in ("empties", "mesh-removed", "one", "nothing-left"):
        out.append(Case("meshes-" + name, "meshes", name, frustum(z_clip_value=0.5, **BOX)))
    for F in SCAN_F:
        out.append(Case("scan-F%d" % F, "scan", F, frustum(z_clip_value=0.25, perspective_correct=F % 2 == 1, **BOX)))
    out.append(Case("seeded-persp", "seeded", 400, frustum(perspective_correct=True, z_clip_value=Z03, **BOX)))
    out.append(Case("seeded-flat", "seeded", 400, frustum(z_clip_value=0.5, cull=False, **BOX)))
    return out


def convert_cases():
    out = [ConvertCase("convert-S%d-%s" % (S, p), "seeded-persp", S, p, S in (257, 4096)) for S in CONVERT_S for p in PATTERNS]
    out.append(ConvertCase("convert-noconv", "cull-only", 257, "random", False))
    return out


def case_by_id(cid):
    return next(c for c in cases() + convert_cases() if c.id == cid)


def _gen(name):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * ord(ch) for i, ch in enumerate(name)))


def _scene(g, F, zlo, zhi):
    """Triangles of NDC-ish extent with z drawn from (zlo, zhi)."""
    c = torch.rand(F, 1, 2, generator=g) * 2.0 - 1.0
    xy = c + (torch.rand(F, 3, 2, generator=g) - 0.5) * 0.9
    return torch.cat([xy, torch.rand(F, 3, 1, generator=g) * (zhi - zlo) + zlo], -1).float()


BRANCH_COMBOS = [(i1, kase) for kase in (3, 4) for i1 in (0, 1, 2)]


def _branch(case, g):
    c = case.frustum["z_clip_value"]
    fv = _scene(g, 3 * 2 * 6, c + 0.1, c + 1.0) * torch.tensor([0.8, 0.8, 1.0])  # all in front and inside the box
    for n, (i1, kase) in enumerate(BRANCH_COMBOS + BRANCH_COMBOS):  # faces 3n (kept), 3n + 1 (clipped), 3n + 2 (removed)
        gap = 0.05 + torch.rand(3, generator=g) * 0.8
        z = c - gap if kase == 3 else c + gap
        z[i1] = c + gap[i1] if kase == 3 else c - gap[i1]
        fv[3 * n + 1, :, 2] = z
        fv[3 * n + 2, :, 2] = c - gap
    return fv, torch.tensor([0, 20]), torch.tensor([20, fv.shape[0] - 20])


def _onplane(case, g):
    c = 0.25
    xy = torch.randint(-8, 9, (14, 3, 2), generator=g).float() / 8
    z = torch.tensor([[c, -0.25, -0.75], [-0.25, c, -0.75], [-0.75, -0.25, c],  # case 3, the lone front vertex on the plane: w2 = w3 = 0
                      [-0.25, c, 0.75], [0.75, -0.25, c], [c, 0.75, -0.25],  # case 4, front vertex p2 on the plane: w2 = 1, w3 = 1/2
                      [-0.25, 0.75, c], [c, -0.25, 0.75],  # case 4, front vertex p3 on the plane: w3 = 1, w2 = 1/2
                      [0.75, -0.25, -0.25], [-0.75, 1.25, -0.75],  # case 3, the two behind at equal z: w2 == w3 = 1/2
                      [-0.25, 0.75, 0.75], [1.25, 1.25, -0.75],  # case 4, the two in front at equal z
                      [c, c, c], [c, c, -0.25]])  # all on the plane: kept; two on it and one behind: case 4 with w2 = w3 = 1
    # (every w is 0, 1/2 or 1: (z1 - c) / (z1 - z2) with a power of two below)
    return torch.cat([xy, z[:, :, None]], -1), torch.tensor([0]), torch.tensor([14])


def _cull(case, g):
    planes = [case.frustum[k] for k in ("left", "right", "top", "bottom", "znear", "zfar")]
    faces = []

    def inside():
        return torch.cat([torch.rand(3, 2, generator=g) * 0.8 - 0.4, torch.rand(3, 1, generator=g) * 0.3 + 0.6], 1)

    for pl, val in enumerate(planes):
        axis, beyond = pl >> 1, val + (1.0 if pl & 1 else -1.0)
        quirk, meant, kept = inside(), inside(), inside()
        quirk[axis, :] = beyond + torch.rand(3, generator=g) * (0.5 if pl & 1 else -0.5)  # the three coordinates of vertex `axis`
        meant[:, axis] = beyond + torch.rand(3, generator=g) * (0.5 if pl & 1 else -0.5)  # coordinate `axis` of the three vertices
        if pl == 4:
            meant[2, 0] = 0.75  # (or vertex 2, all below znear with its small x and y, would go by the reference's reading too)
        faces += [quirk, kept, meant]
    fv = torch.stack(faces)
    if case.arg == "front":  # nothing behind any z plane that is not set: culling alone, no conversion
        return fv, torch.tensor([0, 9]), torch.tensor([9, 9])
    straddle = _scene(g, 8, -0.5, 1.0) * torch.tensor([0.4, 0.4, 1.0])
    fv = torch.cat([fv[:9], straddle[:4], fv[9:], straddle[4:]])
    if case.arg == "nonfinite":
        nan, inf = float("nan"), float("inf")
        for f, (v, a, val) in zip(NONFINITE_FACES, ((0, 2, nan), (1, 2, inf), (2, 2, -inf), (0, 0, nan), (1, 0, inf), (2, 0, -inf))):
            fv[f, v, a] = val
    return fv, torch.tensor([0, 13]), torch.tensor([13, fv.shape[0] - 13])


NONFINITE_FACES = (9, 10, 11, 22, 23, 24)  # the straddling faces of _cull but two: 12 and 25 stay finite between them


def _meshes(case, g):
    fv = _scene(g, 12, -0.3, 1.3) * torch.tensor([0.8, 0.8, 1.0])
    fv[0, :, 2] = torch.tensor([0.75, 0.125, 0.25])  # case 3 in front, whatever the seed
    fv[11, :, 2] = torch.tensor([0.625, 0.875, 0.25])  # case 4 at the end
    if case.arg == "empties":
        return fv, torch.tensor([0, 0, 4, 4, 12, 12]), torch.tensor([0, 4, 0, 8, 0, 0])
    if case.arg == "mesh-removed":
        fv[4:8, :, 2] -= 2.0
        return fv, torch.tensor([0, 4, 8]), torch.tensor([4, 4, 4])
    if case.arg == "nothing-left":
        fv[:, :, 2] -= 2.0
        return fv, torch.tensor([0, 5]), torch.tensor([5, 7])
    return fv, torch.tensor([0]), torch.tensor([12])


def _scan(case, g):
    F = case.arg
    fv = _scene(g, F, -0.4, 1.6)
    if F > 1023:
        fv[1023] = torch.tensor([[0.1, 0.2, 0.125], [0.3, -0.2, 0.5], [-0.2, 0.1, 0.75]])  # case 4: delta 2 on the block's last row
    if F > 1024:
        fv[1024, :, 2] = torch.tensor([0.0, 0.125, -0.5])  # case 2: delta 0 on the next block's first row
    third = F // 3
    return fv, torch.tensor([0, third, third]), torch.tensor([third, 0, F - third])


def _seeded(case, g):
    F, c = case.arg, case.frustum["z_clip_value"]
    return _scene(g, F, c - 0.9, c + 1.1), torch.tensor([0, 150, 150]), torch.tensor([150, 0, F - 150])


_BUILDERS = dict(branch=_branch, onplane=_onplane, cull=_cull, meshes=_meshes, scan=_scan, seeded=_seeded)


def inputs(case):
    """(face_verts float32 (F, 3, 3), first, count) of a clip case, CPU."""
    return _BUILDERS[case.kind](case, _gen(case.id))


def ungated_faces(case):
    return NONFINITE_FACES if case.arg == "nonfinite" else ()


def cotangents(case, Fc, T):
    g = _gen(case.id + "/cotangents")
    if case.kind == "onplane":
        return torch.randint(-8, 9, (Fc, 3, 3), generator=g).float() / 4, torch.randint(-8, 9, (T, 3, 3), generator=g).float() / 4
    return torch.randn(Fc, 3, 3, generator=g), torch.randn(T, 3, 3, generator=g)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
class Frustum:
    def __init__(self, **kw):
        self.__dict__.update(frustum(**kw))


class Clipped:
    def __init__(self, face_verts, mesh_to_face_first_idx, num_faces_per_mesh, faces_clipped_to_unclipped_idx=None,
                 barycentric_conversion=None, faces_clipped_to_conversion_idx=None, clipped_faces_neighbor_idx=None):
        self.face_verts, self.mesh_to_face_first_idx, self.num_faces_per_mesh = face_verts, mesh_to_face_first_idx, num_faces_per_mesh
        self.faces_clipped_to_unclipped_idx, self.barycentric_conversion = faces_clipped_to_unclipped_idx, barycentric_conversion
        self.faces_clipped_to_conversion_idx, self.clipped_faces_neighbor_idx = faces_clipped_to_conversion_idx, clipped_faces_neighbor_idx


def _replace_gradient(value, *carriers):
    """value's number with the derivatives of the carriers."""
    return value.detach() + sum(c - c.detach() for c in carriers)


def _interp(pa, pb, w, persp, c, wrong):
    w = w[:, None]
    out = pa * (1 - w) + pb * w
    if persp:  # xy: to world (times z), interpolate, back to the plane (divide by its z)
        A, B = pa[:, :2] * pa[:, 2:3], pb[:, :2] * pb[:, 2:3]
        xy = (A * (1 - w) + B * w) / c
        if wrong == "swap_w_persp":
            wd = w.detach()
            xy = _replace_gradient(xy, (A * wd + B * (1 - wd)) / c, (A.detach() * (1 - w) + B.detach() * w) / c)
        out = torch.cat([xy, out[:, 2:]], 1)
    return out


def _clip_points(faces, i1, c, persp, wrong):
    ar = torch.arange(faces.shape[0], device=faces.device)
    i2, i3 = (i1 + 1) % 3, (i1 + 2) % 3
    p1, p2, p3 = faces[ar, i1], faces[ar, i2], faces[ar, i3]
    w2 = (p1[:, 2] - c) / (p1[:, 2] - p2[:, 2])
    w3 = (p1[:, 2] - c) / (p1[:, 2] - p3[:, 2])
    if wrong != "keep_w3":
        w3 = w3.detach()  # a constant for autograd, as in the reference
    p4, p5 = _interp(p1, p2, w2, persp, c, wrong), _interp(p1, p3, w3, persp, c, wrong)
    eye = torch.eye(3, dtype=faces.dtype, device=faces.device)
    e1, e2, e3 = eye[i1], eye[i2], eye[i3]
    w2b = w2.detach() if wrong == "drop_gconv_w2" else w2
    b4 = e1 * (1 - w2b)[:, None] + e2 * w2b[:, None]
    b5 = e1 * (1 - w3)[:, None] + e3 * w3[:, None]
    return (p1, p2, p3, p4, p5), (e1, e2, e3, b4, b5)


def clip_faces_torch(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, frustum, wrong=None):
    """clip_faces in torch, any dtype and device, differentiated by autograd: classification by the reference's reading of the planes,
    destinations by a cumulative sum, the five points of each clipped face, rows placed by one permutation."""
    fv, fr = face_verts, frustum
    F, dev = fv.shape[0], fv.device
    culled = torch.zeros(F, dtype=torch.bool, device=dev)
    for pl, val in enumerate((fr.left, fr.right, fr.top, fr.bottom, fr.znear, fr.zfar)):
        if fr.cull and val is not None:
            x = fv[:, pl >> 1, :]  # the three coordinates of vertex number `axis`
            culled |= ((x > val) if pl & 1 else (x < val)).all(1)
    c, persp = fr.z_clip_value, bool(fr.perspective_correct)
    behind = fv[:, :, 2] < c if c is not None else torch.zeros((F, 3), dtype=torch.bool, device=dev)
    n = behind.sum(1)
    k2 = culled | (n == 3)
    k1, k3, k4 = (n == 0) & ~culled, (n == 2) & ~culled, (n == 1) & ~culled
    if not bool((k2 | k3 | k4).any()):
        return Clipped(face_verts, mesh_to_face_first_idx, num_faces_per_mesh)
    delta = 1 + k4.long() - k2.long()
    dst = torch.cat([delta.new_zeros(1), delta.cumsum(0)])  # (F + 1): dst[F] = F_clipped
    Fc = int(dst[F])
    first_c = dst[mesh_to_face_first_idx.clamp(0, F)]
    count_c = torch.cat([first_c[1:], dst[F:]]) - first_c
    ids = torch.arange(F, device=dev)
    id1, id3, id4 = ids[k1], ids[k3], ids[k4]
    T3, T4 = id3.numel(), id4.numel()
    minus = lambda m: torch.full((m,), -1, dtype=torch.int64, device=dev)
    pos = torch.cat([dst[id1], dst[id3], dst[id4], dst[id4] + 1])
    order = torch.argsort(pos)
    c2u = torch.cat([id1, id3, id4, id4])[order]
    if T3 + T4 == 0:
        return Clipped(fv[id1], first_c, count_c, c2u)
    (p1, _, _, p4, p5), (e1, _, _, b4, b5) = _clip_points(fv[id3], (~behind[id3]).long().argmax(1), c, persp, wrong)
    t3, m3 = torch.stack([p4, p5, p1], 1), torch.stack([b4, b5, e1], 2)
    (_, p2, p3, p4, p5), (_, e2, e3, b4, b5) = _clip_points(fv[id4], behind[id4].long().argmax(1), c, persp, wrong)
    p2_second = p2.detach() if wrong == "drop_g2_second" else p2
    t4a, t4b = torch.stack([p4, p2, p5], 1), torch.stack([p5, p2_second, p3], 1)
    conv = torch.cat([m3, torch.stack([b4, e2, b5], 2), torch.stack([b5, e2, e3], 2)])
    out_fv = torch.cat([fv[id1], t3, t4a, t4b])[order]
    rows = torch.arange(T3 + 2 * T4, device=dev)
    conv_idx = torch.cat([minus(id1.numel()), rows])[order]
    nbr = torch.cat([minus(id1.numel() + T3), dst[id4] + 1, dst[id4]])[order]
    return Clipped(out_fv, first_c, count_c, c2u, conv, conv_idx, nbr)


def convert_clipped_torch(pix_to_face_clipped, bary_coords_clipped, clipped_faces, wrong=None):
    """convert_clipped_rasterization_to_original_faces in torch: samples of any shape, bary_coords_clipped one axis of 3 longer."""
    cf, p2f, bary = clipped_faces, pix_to_face_clipped, bary_coords_clipped
    c2u = cf.faces_clipped_to_unclipped_idx
    if c2u is None or c2u.numel() == 0:
        return p2f, bary
    hit = p2f != -1
    p2f_u = torch.where(hit, c2u[p2f.clamp(min=0)], torch.full_like(p2f, -1))
    if cf.barycentric_conversion is None:
        return p2f_u, bary
    row = torch.where(hit, cf.faces_clipped_to_conversion_idx[p2f.clamp(min=0)], torch.full_like(p2f, -1))
    if cf.barycentric_conversion.shape[0] == 0:
        return p2f_u, bary
    M = cf.barycentric_conversion[row.clamp(min=0)]  # (..., 3, 3): [j, k] = weight of original vertex j in clipped vertex k
    out = (M * bary[..., None, :]).sum(-1)
    if wrong == "conv_untransposed":  # the sample gradient M g in place of M^T g
        out = _replace_gradient(out, (M.detach().transpose(-1, -2) * bary[..., None, :]).sum(-1), (M * bary.detach()[..., None, :]).sum(-1))
    return p2f_u, torch.where((row != -1)[..., None], out, bary)


def torch_impl(wrong=None):
    return Impl(lambda *a: clip_faces_torch(*a, wrong=wrong), lambda *a: convert_clipped_torch(*a, wrong=wrong), Frustum, Clipped)


def kernel_impl():
    from pytorch3d_amd import clip

    return Impl(lambda fv, first, count, fr: clip.clip_faces(fv, first, count, frustum=fr), clip.convert_clipped_rasterization_to_original_faces,
                clip.ClipFrustum, clip.ClippedFaces)


# ---- running a case ----------------------------------------------------------------------------------------------------------------
def _np64(t):
    return t.detach().double().cpu().numpy()


def tables_of(cf):
    return {name: None if getattr(cf, name) is None else getattr(cf, name).detach().cpu().numpy().astype(np.int64) for name in TABLES}


def run_clip(impl, case, device="cpu", dtype=torch.float32, modes=GRAD_MODES):
    """{quantity: float64 array or None} of a clip case: the tables, face_verts, barycentric_conversion, grad_face_verts/<mode>."""
    fv, first, count = inputs(case)
    fv = fv.to(device=device, dtype=dtype).requires_grad_(True)
    cf = impl.clip_faces(fv, first.to(device), count.to(device), impl.frustum(**case.frustum))
    out = tables_of(cf)
    conv = cf.barycentric_conversion
    out["face_verts"] = _np64(cf.face_verts)
    out["barycentric_conversion"] = None if conv is None else _np64(conv)
    g_fv, g_conv = cotangents(case, cf.face_verts.shape[0], 0 if conv is None else conv.shape[0])
    g_fv, g_conv = g_fv.to(device=device, dtype=dtype), g_conv.to(device=device, dtype=dtype)
    for mode in modes:
        loss = fv.new_zeros(())
        if mode in ("fv", "both"):
            loss = loss + (cf.face_verts * g_fv).sum()
        if mode in ("conv", "both") and conv is not None:
            loss = loss + (conv * g_conv).sum()
        grad = torch.autograd.grad(loss, fv, retain_graph=True, allow_unused=True)[0] if loss.requires_grad else None
        out["grad_face_verts/" + mode] = _np64(torch.zeros_like(fv) if grad is None else grad)
    return out


def convert_inputs(ccase):
    """(pix_to_face (1, 1, S, 1), bary (1, 1, S, 1, 3), gradient into the un-clipped barycentrics) from the fixture's tables of the base case."""
    fix, g, S = fixture(), _gen(ccase.id), ccase.S
    conv_idx = fix.get(key(ccase.base, TABLES[3]))
    Fc = int(fix[key(ccase.base, TABLES[2])].shape[0])
    conv_idx = np.full(Fc, -1) if conv_idx is None else conv_idx.astype(np.int64)
    owner = torch.from_numpy(np.argsort(np.where(conv_idx < 0, conv_idx.max() + 1, conv_idx), kind="stable"))  # row -> clipped face
    T = int((conv_idx >= 0).sum())
    i = torch.arange(S)
    if ccase.pattern == "random":
        p2f = torch.randint(0, Fc, (S,), generator=g)
        p2f[torch.rand(S, generator=g) < 0.25] = -1
    elif ccase.pattern == "onerow":
        p2f = owner[T // 3].expand(S).clone()
    elif ccase.pattern == "tworows":
        p2f = owner[torch.where(i % 2 == 0, 5, T - 7)]
    elif ccase.pattern == "fresh":
        p2f = owner[i % T]
    else:
        kept = torch.from_numpy(np.nonzero(conv_idx < 0)[0])
        p2f = kept[torch.randint(0, kept.numel(), (S,), generator=g)]
    return p2f.view(1, 1, S, 1), torch.rand(1, 1, S, 1, 3, generator=g), torch.randn(1, 1, S, 1, 3, generator=g)


def run_convert(impl, ccase, device="cpu", dtype=torch.float32, through=None):
    """{quantity: array} of a convert case: pix_to_face_unclipped, bary_unclipped, grad_bary_clipped, grad_conversion (None without a
    conversion), grad_face_verts_from_samples (the loss on the un-clipped barycentrics alone; None unless the case asks).  `through` may replace the
    (pix_to_face, bary) pair by views of the same values."""
    base = case_by_id(ccase.base)
    fv, first, count = inputs(base)
    fv = fv.to(device=device, dtype=dtype).requires_grad_(True)
    cf = impl.clip_faces(fv, first.to(device), count.to(device), impl.frustum(**base.frustum))
    p2f, bary, g_u = convert_inputs(ccase)
    p2f, bary, g_u = p2f.to(device), bary.to(device=device, dtype=dtype), g_u.to(device=device, dtype=dtype)
    if through is not None:
        p2f, bary = through(p2f, bary)
    bary.requires_grad_(True)
    conv = cf.barycentric_conversion
    leaf = None if conv is None else conv.detach().clone().requires_grad_(True)
    rebuilt = impl.clipped(**{name: (getattr(cf, name).detach() if name == "face_verts" else getattr(cf, name)) for name in FIELDS if name != "barycentric_conversion"},
                           barycentric_conversion=leaf)
    p2f_u, bary_u = impl.convert(p2f, bary, rebuilt)
    grads = torch.autograd.grad((bary_u * g_u).sum(), [bary] + ([] if leaf is None else [leaf]), allow_unused=True)
    out = {"pix_to_face_unclipped": p2f_u.detach().cpu().numpy().reshape(-1), "bary_unclipped": _np64(bary_u).reshape(-1, 3),
           "grad_bary_clipped": _np64(grads[0]).reshape(-1, 3), "grad_conversion": None, "grad_face_verts_from_samples": None}
    if leaf is not None:
        out["grad_conversion"] = _np64(torch.zeros_like(leaf) if grads[1] is None else grads[1])
    if ccase.to_verts:  # nothing but the conversion matrices carries the loss back to the vertices
        _, again = impl.convert(p2f, bary.detach(), cf)
        grad = torch.autograd.grad((again * g_u).sum(), fv)[0] if again.requires_grad else torch.zeros_like(fv)
        out["grad_face_verts_from_samples"] = _np64(grad)
    return out


# ---- the fixture, the truth and the gates ---------------------------------------------------------------------------------------------
def key(cid, name):
    return "%s/%s" % (cid, name)


@functools.lru_cache(maxsize=1)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def e_ref(quantity):
    return float(fixture()["E_ref/" + quantity.split("/")[0]])


def held(n):
    """The rows of an n-row quantity whose truth the fixture holds."""
    if n <= 64:
        return np.arange(n)
    rows = [np.arange(16), n - 16 + np.arange(16), np.linspace(0, n - 1, 32).astype(np.int64)]
    if n > 1040:
        rows.append(np.arange(1016, 1033))
    return np.unique(np.concatenate(rows))


def float_quantities(case):
    if isinstance(case, ConvertCase):
        return SAMPLE_QUANTITIES + ("grad_conversion", "grad_face_verts_from_samples")
    return ("face_verts", "barycentric_conversion") + tuple("grad_face_verts/" + m for m in GRAD_MODES)


def int_quantities(case):
    return ("pix_to_face_unclipped",) if isinstance(case, ConvertCase) else TABLES


def row_scale(a):
    return row_max(np.abs(np.asarray(a, dtype=np.float64)))


def row_max(a):
    """The largest entry of each row (a.shape[0] of them; zero rows give an empty result)."""
    return a.reshape(a.shape[0], int(np.prod(a.shape[1:]))).max(1, initial=0.0)


def gated_rows(case, quantity, tables):
    """Boolean mask over the rows of a block quantity: all of them but those of faces with non-finite coordinates."""
    if isinstance(case, ConvertCase):
        return np.ones(tables[quantity].shape[0], dtype=bool)
    bad = np.asarray(ungated_faces(case), dtype=np.int64)
    if quantity.startswith("grad_face_verts"):
        return ~np.isin(np.arange(inputs(case)[0].shape[0]), bad)
    c2u = tables[TABLES[2]]
    if c2u is None:  # nothing culled or clipped: the input came back
        return np.ones(inputs(case)[0].shape[0], dtype=bool)
    face_ok = ~np.isin(c2u, bad)
    if quantity == "face_verts":
        return face_ok
    conv_idx = tables[TABLES[3]]
    ok = np.ones(int((conv_idx >= 0).sum()), dtype=bool)
    ok[conv_idx[(conv_idx >= 0) & ~face_ok]] = False
    return ok


@functools.lru_cache(maxsize=None)
def _truth(cid):
    case, fix = case_by_id(cid), fixture()
    run = run_convert if isinstance(case, ConvertCase) else run_clip
    t = run(torch_impl(), case, dtype=torch.float64)
    for name in int_quantities(case):
        want = fix.get(key(cid, name))
        assert (t[name] is None) == (want is None) and (want is None or np.array_equal(t[name], want.astype(np.int64))), (cid, name)
    for q in float_quantities(case):
        want = fix.get(key(cid, q))
        assert (t[q] is None) == (want is None), (cid, q)
        if want is None:
            continue
        rows = held(t[q].shape[0])
        assert want.shape == t[q][rows].shape, (cid, q)
        if q in SAMPLE_QUANTITIES:
            assert np.abs(t[q][rows] - want).max(initial=0.0) <= 1e-12 * np.abs(want).max(initial=0.0), (cid, q)
            continue
        ok = gated_rows(case, q, t)[rows]
        with np.errstate(invalid="ignore"):  # (the rows of faces with non-finite coordinates are left out below)
            err = row_max(np.abs(t[q][rows] - want))
        assert (err[ok] <= 1e-12 * row_scale(want)[ok]).all(), (cid, q)
    return t


def truth(case):
    """The float64 truth of every quantity of a case: the restatement, tied to the fixture's rows on every first call."""
    return _truth(case.id)


def errors(case, got):
    """[(quantity, worst error / gate over the rows or samples (0 where all are exact), number beyond the gate)].  Integer tables
    count every differing entry; a missing or extra quantity and a wrong shape are failures of that quantity."""
    t, out = truth(case), []
    for name in int_quantities(case):
        same = (got[name] is None) == (t[name] is None) and (t[name] is None or np.array_equal(np.asarray(got[name]).astype(np.int64), t[name]))
        out.append((name, 0.0 if same else float("inf"), 0 if same else 1))
    for q in float_quantities(case):
        if t[q] is None or got[q] is None or np.shape(got[q]) != t[q].shape:
            same = t[q] is None and got[q] is None
            out.append((q, 0.0 if same else float("inf"), 0 if same else 1))
            continue
        with np.errstate(invalid="ignore"):
            diff = np.abs(np.asarray(got[q], dtype=np.float64) - t[q])
        if q in SAMPLE_QUANTITIES:
            err, gate = diff.reshape(-1), np.full(diff.size, GATE_FACTOR * e_ref(q) * np.abs(t[q]).max(initial=0.0))
        else:
            ok = gated_rows(case, q, t)
            err, gate = row_max(diff)[ok], (GATE_FACTOR * e_ref(q) * row_scale(t[q]))[ok]
        bad = ~(err <= gate)  # (a NaN is beyond every gate; a zero row has a zero gate)
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / gate)
        out.append((q, float(np.nan_to_num(ratio, nan=np.inf).max(initial=0.0)), int(bad.sum())))
    return out


def block_errors(got, truth, quantity):
    """(worst error / gate, rows beyond the gate) of a block-per-row quantity against a truth of one's own (the big launch)."""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert got.shape == truth.shape, (quantity, got.shape, truth.shape)
    err, gate = row_max(np.abs(got - truth)), GATE_FACTOR * e_ref(quantity) * row_scale(truth)
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / gate)
    return float(np.nan_to_num(ratio, nan=np.inf).max(initial=0.0)), int((~(err <= gate)).sum())


def failures(cases_, impl, device="cpu", dtype=torch.float32, verbose=False):
    """[(case id, quantity, worst error / gate, rows beyond the gate)] of everything beyond its gate."""
    bad = []
    for case in cases_:
        run = run_convert if isinstance(case, ConvertCase) else run_clip
        for q, ratio, n in errors(case, run(impl, case, device, dtype)):
            if verbose:
                print("%-28s %-34s worst error / gate %.3f%s" % (case.id, q, ratio, "  BEYOND: %d" % n if n else ""))
            if n:
                bad.append((case.id, q, ratio, n))
    return bad


def same_bits(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), equal_nan=True))


def branches(case):
    """{(i1, clipping case, perspective_correct)} that the faces of a clip case reach, from its inputs and the truth's tables."""
    fv = inputs(case)[0].numpy()
    t, c = truth(case), case.frustum["z_clip_value"]
    out = set()
    if t[TABLES[3]] is None:
        return out
    c2u, conv_idx, nbr = t[TABLES[2]], t[TABLES[3]], t[TABLES[4]]
    for j in np.nonzero(conv_idx >= 0)[0]:
        behind = fv[c2u[j], :, 2] < c
        kase = 4 if nbr[j] >= 0 else 3
        out.add((int(np.nonzero(behind if kase == 4 else ~behind)[0][0]), kase, bool(case.frustum["perspective_correct"])))
    return out


# ---- the pipeline scenes (part of the fixture; used by the GPU test) ------------------------------------------------------------------
PIPELINE = {"pipe-persp": True, "pipe-flat": False}
PIPELINE_IMAGE, PIPELINE_K, PIPELINE_Z_CLIP = 16, 2, 0.25


def pipeline_scene(tag):
    """(verts (V, 3), faces (12, 3)): a dozen triangles of a third of the image each, every one crossing z = 0.25."""
    g = _gen(tag)
    xy = torch.rand(12, 1, 2, generator=g) - 0.5 + (torch.rand(12, 3, 2, generator=g) - 0.5) * 1.6
    fv = torch.cat([xy, torch.rand(12, 3, 1, generator=g) * 1.2 + 0.3], -1)
    for f in range(12):
        fv[f, f % 3, 2] = -0.05 - 0.4 * float(torch.rand((), generator=g))  # one vertex behind: case 4; every third face gets a second
        if f % 3 == 0:
            fv[f, (f // 3) % 2 + 1, 2] = 0.2 - 0.3 * float(torch.rand((), generator=g))
    return fv.reshape(36, 3), torch.arange(36).view(12, 3)


def pipeline_residual(verts, faces, p2f, zbuf, bary, persp):
    """(largest |xy from the un-clipped barycentrics - pixel centre|, largest |z from them - zbuf|) over the fragments with a face, in
    float64 from float32 outputs.  verts (V, 3), faces (F, 3) of ONE mesh; outputs (1, H, W, K[, 3])."""
    v = verts.detach().double().cpu()[faces.cpu()]  # (F, 3, 3)
    p2f, zbuf, bary = p2f.cpu(), zbuf.detach().double().cpu(), bary.detach().double().cpu()
    H, W = p2f.shape[1:3]
    ys = 1.0 - (2.0 * torch.arange(H, dtype=torch.float64) + 1.0) / H
    xs = 1.0 - (2.0 * torch.arange(W, dtype=torch.float64) + 1.0) / W
    centre = torch.stack([xs[None, :, None].expand(H, W, p2f.shape[3]), ys[:, None, None].expand(H, W, p2f.shape[3])], -1)[None]
    hit = p2f >= 0
    tri, b = v[p2f[hit]], bary[hit]  # (n, 3, 3), (n, 3)
    z = (b * tri[:, :, 2]).sum(1)
    if persp:
        xy = (b[:, :, None] * tri[:, :, :2] * tri[:, :, 2:3]).sum(1) / z[:, None]
    else:
        xy = (b[:, :, None] * tri[:, :, :2]).sum(1)
    return float((xy - centre[hit]).abs().max()), float((z - zbuf[hit]).abs().max()), int(hit.sum())
