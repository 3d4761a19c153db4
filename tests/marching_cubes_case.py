"""Shared cases of the marching cubes tests: the cases of tests/golden/marching_cubes_ref.npz (recorded by
tests/golden/make_golden_marching_cubes.py from the reference's compiled CPU operator behind its own Python wrapper), its loader, the
triangle table re-derived from the record of the 256 sign configurations, a nested-loop restatement of BOTH contracts in plain Python /
numpy float32 scalars (`restate_cpu`: what the reference returns for CPU tensors; `restate_device`: what it returns for GPU tensors
after its own dedup), and `misses`, the one gate every implementation -- the restatements, the host loop, the torch formulation, the
kernels, deliberately wrong variants -- is judged by.  No test collects this file.

Numbering (the project's own): corner i of a cube is (x, y, z) = (i & 1, i >> 1 & 1, i >> 2 & 1); the configuration byte has bit i set
iff corner i is inside (value < isolevel); an edge is (axis, corner): it runs from `corner` (whose `axis` bit is 0) one step along axis
0 = x, 1 = y, 2 = z, and a table entry is 8 * axis + corner.

A case is a name; inputs(name) gives (volumes (N, D, H, W) float32, isolevel or None).  Families:
  cfg256        the 256 sign configurations as (256, 2, 2, 2) of +-1, isolevel 0: every vertex is an edge midpoint and names its edge
  rand345       randn (3, 3, 4, 5), isolevel 0
  rand579       randn (2, 5, 7, 9), isolevel 0.1 (not a float32); holds vertices whose constant coordinate is not an integer
  sphere12      a sphere's signed distance in 12^3, isolevel 0
  snap          (2, 3, 3, 3) with corners exactly at the isolevel 0.5, within 1e-5 of it on either side, and just beyond 1e-5
  degen         2 x 2 x 2 volumes whose FIRST table triangle is degenerate and a later one is not: the reference's CPU loop drops both
  isonone       isolevel None over (3, 4, 4, 4) volumes of different ranges
  mixed_empty   (5, 3, 3, 3): random, constant, all inside, all outside, random
  thin_d, thin_h, thin_w   D, H or W equal to 1: no cube, every entry `[]`
  naninf        randn (2, 3, 4, 4) with NaN, +inf and -inf entries
  chan_slice    the volumes are channel 1 of an (N, 3, D, H, W) tensor;  permuted: a permuted view -- the strided layouts are rebuilt by
                inputs() around the recorded values
The fixture holds per case <name>/vol, <name>/iso (NaN: None) and, for local = 0 (world coordinates) and 1, the reference's lists packed:
<name>/<local>/verts, faces, nv, nf (nf[n] == 0: the reference returned `[]` for volume n); and err/local/<name>: the reference's own
largest |float32 - float64| over the local coordinates of the case, its Transform3d chain run in float64 over the same world vertices.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "marching_cubes_ref.npz")
EPS = np.float32(1e-5)
STRIDED = {"chan_slice": (2, 3, 4, 5), "permuted": (2, 4, 5, 6)}


def cases():
    return ["cfg256", "rand345", "rand579", "sphere12", "snap", "degen", "isonone", "mixed_empty", "thin_d", "thin_h", "thin_w", "naninf",
            "chan_slice", "permuted"]


def config_volumes():
    """(256, 2, 2, 2): volume c has -1 at corner i iff bit i of c is set, else +1."""
    c = torch.arange(256)[:, None]
    inside = ((c >> torch.arange(8)[None]) & 1).bool()  # corner i = x + 2 y + 4 z is entry [z, y, x] of the row-major (2, 2, 2)
    return torch.where(inside, -1.0, 1.0).reshape(256, 2, 2, 2)


def sphere(size, radius=0.37):
    t = (torch.arange(size, dtype=torch.float32) + 0.25) / size - 0.5
    z, y, x = torch.meshgrid(t, t, t, indexing="ij")
    return (torch.sqrt(x * x + y * y + z * z) - radius)[None].contiguous()


def build_inputs(name, degenerate_first=None):
    """What the recorder stores as the case's inputs (tests read them from the fixture).  degenerate_first: the (K, 2, 2, 2) volumes the
    recorder found for "degen"."""
    gen = torch.Generator().manual_seed(4100 + cases().index(name))
    if name == "cfg256":
        return config_volumes(), 0.0
    if name == "rand345":
        return torch.randn((3, 3, 4, 5), generator=gen), 0.0
    if name == "rand579":
        return torch.randn((2, 5, 7, 9), generator=gen), 0.1
    if name == "sphere12":
        return sphere(12), 0.0
    if name == "snap":
        vol = torch.randn((2, 3, 3, 3), generator=gen) + 0.5
        at = torch.tensor(0.5)
        special = torch.stack([at, at + 5e-6, at - 5e-6, at + 2e-5, at - 2e-5, torch.nextafter(at, torch.tensor(0.0))])
        pick = torch.randint(0, 12, vol.shape, generator=gen)
        return torch.where(pick < 6, special[pick.clamp(max=5)], vol), 0.5
    if name == "degen":
        return degenerate_first, 0.0
    if name == "isonone":
        vol = torch.rand((3, 4, 4, 4), generator=gen)
        return vol * torch.tensor([1.0, 10.0, 0.1]).view(3, 1, 1, 1) + torch.tensor([0.0, -3.0, 7.0]).view(3, 1, 1, 1), None
    if name == "mixed_empty":
        vol = torch.randn((5, 3, 3, 3), generator=gen)
        vol[1], vol[2], vol[3] = 0.3, -5.0, 5.0
        return vol, 0.0
    if name.startswith("thin_"):
        shape = {"thin_d": (2, 1, 4, 4), "thin_h": (2, 4, 1, 4), "thin_w": (2, 4, 4, 1)}[name]
        return torch.randn(shape, generator=gen), 0.0
    if name == "naninf":
        vol = torch.randn((2, 3, 4, 4), generator=gen)
        pick = torch.randint(0, 16, vol.shape, generator=gen)
        vol[pick == 0], vol[pick == 1], vol[pick == 2] = float("nan"), float("inf"), float("-inf")
        return vol, 0.0
    if name in STRIDED:
        return torch.randn(STRIDED[name], generator=gen), 0.0
    raise KeyError(name)


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(FIXTURE) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def strided(name, vol):
    """The recorded values in the case's memory layout."""
    if name == "chan_slice":
        base = torch.full((vol.shape[0], 3) + tuple(vol.shape[1:]), 7.0, dtype=vol.dtype, device=vol.device)
        base[:, 1] = vol
        return base[:, 1]
    if name == "permuted":
        return vol.permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)
    return vol


def inputs(name, device="cpu"):
    f = fixture()
    iso = float(f[name + "/iso"])
    return strided(name, torch.from_numpy(f[name + "/vol"]).to(device)), None if iso != iso else iso


def to_lists(verts, faces, nv, nf):
    """Packed tensors and per-volume sizes -> the reference's two lists, `[]` for a volume without a face."""
    nv, nf = [int(x) for x in nv], [int(x) for x in nf]
    vs, fs = verts.split(nv, 0), faces.split(nf, 0)
    return [v if k else [] for v, k in zip(vs, nf)], [f if k else [] for f, k in zip(fs, nf)]


def expected(name, local):
    """The reference's recorded CPU lists of the case."""
    f = fixture()
    key = "%s/%d/" % (name, int(bool(local)))
    return to_lists(torch.from_numpy(f[key + "verts"]), torch.from_numpy(f[key + "faces"]), f[key + "nv"], f[key + "nf"])


def tolerance(name, local):
    """World coordinates are exact; local ones are gated at 4 x the reference's own float32 rounding over the case."""
    return 4.0 * float(fixture()["err/local/" + name]) if local else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the table, from the record of the 256 configurations
def table_from_record(verts_list, faces_list):
    """256 tuples of entries 8 * axis + corner, in the reference's order: every recorded vertex of configuration c sits at the midpoint
    of one edge of the unit cube, the coordinate at 0.5 names the axis and the other two the corner."""
    table = []
    for verts, faces in zip(verts_list, faces_list):
        entries = []
        if len(faces):
            for p in verts[faces.reshape(-1)].tolist():
                half = [a for a in range(3) if p[a] == 0.5]
                assert len(half) == 1 and all(p[a] in (0.0, 1.0) for a in range(3) if a != half[0]), p
                axis = half[0]
                entries.append(8 * axis + sum(int(p[a]) << a for a in range(3) if a != axis))
        table.append(tuple(entries))
    return table


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = table_from_record(*expected("cfg256", False))
    return _TABLE


def crossed_edges(config):
    """The entries 8 * axis + corner of the edges whose endpoints differ in the inside test."""
    return {8 * a + c for a in range(3) for c in range(8) if not (c >> a) & 1 and ((config >> c) & 1) != ((config >> (c | 1 << a)) & 1)}


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
def edge_vertex(iso, v1, v2, p1, axis, variant=None):
    """The vertex on the edge from lattice point p1 (x, y, z) one step along `axis`, in float32 scalar by scalar."""
    f = np.float32
    p1 = [f(c) for c in p1]
    p2 = [f(c + (1 if a == axis else 0)) for a, c in enumerate(p1)]
    with np.errstate(all="ignore"):
        if variant != "no_snap":
            if abs(f(iso - v1)) < EPS:
                return p1
            if abs(f(iso - v2)) < EPS:
                return p2
            if abs(f(v1 - v2)) < EPS:
                return p1
        r = f(f(iso - v1) / f(v2 - v1))
        if variant == "lerp":
            return [f(a + f(r * f(b - a))) for a, b in zip(p1, p2)]
        one_minus = f(f(1) - r)
        out = [f(f(a * one_minus) + f(b * r)) for a, b in zip(p1, p2)]
        if variant == "integer_constant":
            out = [o if a == axis else c for a, (o, c) in enumerate(zip(out, p1))]
        return out


def differ(a, b):
    """The reference's Vertex `!=`: at least 1e-5 apart in some coordinate (a NaN difference: not apart)."""
    with np.errstate(all="ignore"):
        return any(abs(np.float32(x - y)) >= EPS for x, y in zip(a, b))


def degenerate(a, b, c):
    """A triangle is kept iff its vertices differ pairwise."""
    return not (differ(a, b) and differ(b, c) and differ(c, a))


def _cubes(vol, iso, variant):
    """(x, y, z, config) of every cube, x fastest."""
    D, H, W = vol.shape
    for z in range(D - 1):
        for y in range(H - 1):
            for x in range(W - 1):
                config = 0
                for i in range(8):
                    v = vol[z + (i >> 2 & 1), y + (i >> 1 & 1), x + (i & 1)]
                    if (v <= iso) if variant == "le" else (v < iso):
                        config |= 1 << i
                yield x, y, z, config


def _entry(vol, iso, x, y, z, e, variant):
    """(owning lattice point (x, y, z), axis, vertex) of table entry e of the cube at (x, y, z)."""
    axis, c = e >> 3, e & 7
    p1 = (x + (c & 1), y + (c >> 1 & 1), z + (c >> 2 & 1))
    p2 = tuple(q + (1 if a == axis else 0) for a, q in enumerate(p1))
    return p1, axis, edge_vertex(iso, vol[p1[2], p1[1], p1[0]], vol[p2[2], p2[1], p2[0]], p1, axis, variant)


def _world(verts, faces):
    return (torch.from_numpy(np.array(verts, np.float32).reshape(-1, 3)), torch.tensor(faces, dtype=torch.int64).reshape(-1, 3))


def restate_cpu_one(vol, iso, variant=None):
    """The CPU contract for one volume (numpy (D, H, W) float32): vertices in order of first use, a triangle with two coinciding
    vertices (`degenerate`) dropped together with every later triangle of its cube -> (verts (V, 3), faces (F, 3)) in world coordinates.
    variant "drop_alone": only the degenerate triangle itself is dropped."""
    iso = np.float32(iso)
    rank, verts, faces = {}, [], []
    for x, y, z, config in _cubes(vol, iso, variant):
        tri, ps = [], []
        for j, e in enumerate(table()[config]):
            p1, axis, v = _entry(vol, iso, x, y, z, e, variant)
            tri.append((p1, axis))
            ps.append(v)
            if (j + 1) % 3:
                continue
            if not degenerate(*ps[:3]):
                for key, v in zip(tri, ps):
                    if key not in rank:
                        rank[key] = len(verts)
                        verts.append(v)
                faces.append([rank[key] for key in tri])
                tri, ps = [], []
            elif variant == "drop_alone":
                tri, ps = [], []
    return _world(verts, faces)


def restate_device_one(vol, iso, variant=None):
    """The device contract for one volume: every table triangle, cubes x fastest; one vertex per crossed lattice edge in the order of
    (lattice point x fastest, axis x y z) -> (verts, faces, ids) in world coordinates, ids[v] = g1 (W + W H + W H D) + g2 for the
    edge's two lattice points.  variants: "drop_degenerate", "first_use" (vertex order), "zyx" (axis order z y x per point)."""
    iso = np.float32(iso)
    D, H, W = vol.shape
    found, tris = {}, []
    for x, y, z, config in _cubes(vol, iso, variant):
        entries = [_entry(vol, iso, x, y, z, e, variant) for e in table()[config]]
        for k in range(0, len(entries), 3):
            t = entries[k:k + 3]
            if variant == "drop_degenerate" and degenerate(t[0][2], t[1][2], t[2][2]):
                continue
            for p1, axis, v in t:
                found.setdefault((p1, axis), v)
            tris.append([(p1, axis) for p1, axis, _ in t])

    def order(key):
        (px, py, pz), axis = key
        return ((pz * H + py) * W + px, 2 - axis if variant == "zyx" else axis)

    keys = list(found) if variant == "first_use" else sorted(found, key=order)
    rank = {key: r for r, key in enumerate(keys)}
    ids = []
    for (px, py, pz), axis in keys:
        g = (pz * H + py) * W + px
        ids.append(g * (W + W * H + W * H * D) + g + (1, W, W * H)[axis])
    verts, faces = _world([found[k] for k in keys], [[rank[k] for k in t] for t in tris])
    return verts, faces, torch.tensor(ids, dtype=torch.int64)


def to_local(verts, D, H, W):
    """The reference's map to [-1, 1]^3 in float64 (the gate's tolerance covers its float32 rounding)."""
    scale = (torch.tensor([W, H, D], dtype=torch.float64) - 1) * 0.5
    return (verts.double() / scale - 1).float()


def restate(vol, iso, local, contract, variant=None):
    """Either contract over a batch -> the reference's two lists.  iso None: (max + min) / 2 per volume in float32."""
    vol = vol.detach().cpu()
    one = restate_cpu_one if contract == "cpu" else restate_device_one
    verts_list, faces_list = [], []
    for v in vol:
        level = ((v.max() + v.min()) / 2).item() if iso is None else iso
        verts, faces = one(v.numpy(), level, variant)[:2]
        if len(faces) == 0:
            verts, faces = [], []
        elif local:
            verts = to_local(verts, *v.shape)
        verts_list.append(verts)
        faces_list.append(faces)
    return verts_list, faces_list


_RESTATED = {}


def restated(name, local, contract):
    """restate() of a fixture case, computed once (the nested loops take a second or two over all cases)."""
    key = (name, bool(local), contract)
    if key not in _RESTATED:
        _RESTATED[key] = restate(*inputs(name), local, contract)
    return _RESTATED[key]


def has_drops(name):
    """Whether the reference's CPU loop dropped a triangle somewhere in the case."""
    got, want = restated(name, False, "device")[1], expected(name, False)[1]
    return any(len(a) != len(b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# the gate
def _same(a, b, tol):
    if tol == 0.0 or not a.is_floating_point():
        return int((~((a == b) | (a.isnan() & b.isnan()) if a.is_floating_point() else a == b)).sum())
    nan = a.isnan() | b.isnan()
    return int(((a.isnan() != b.isnan()) | (~nan & ~((a - b).abs() <= tol) & (a != b))).sum())


def misses(got, want, what="", tol=0.0):
    """Every difference between two (verts list, faces list): lengths, `[]` against tensors, shapes, dtypes, then equality entry by
    entry -- NaN equal to NaN; the vertices within tol where tol > 0 (local coordinates), faces always exact."""
    out = []
    for kind, g, w in zip(("verts", "faces"), got, want):
        if len(g) != len(w):
            out.append("%s %s: %d volumes against %d" % (what, kind, len(g), len(w)))
            continue
        for i, (a, b) in enumerate(zip(g, w)):
            if torch.is_tensor(a) != torch.is_tensor(b):
                out.append("%s %s[%d]: %s against %s" % (what, kind, i, type(a).__name__, type(b).__name__))
            elif not torch.is_tensor(a):
                if a != [] or b != []:
                    out.append("%s %s[%d]: neither a tensor nor []" % (what, kind, i))
            else:
                a, b = a.detach().cpu(), b.detach().cpu()
                if a.shape != b.shape or a.dtype != b.dtype:
                    out.append("%s %s[%d]: %s %s against %s %s" % (what, kind, i, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
                elif _same(a, b, tol if kind == "verts" else 0.0):
                    out.append("%s %s[%d]: %d entries differ" % (what, kind, i, _same(a, b, tol if kind == "verts" else 0.0)))
    return out


def failures(fn, contract, names=None, device="cpu", locals_=(False, True)):
    """misses of fn(vol, iso, local) -> two lists over the named cases (default: all), against the fixture ("cpu") or against the
    restatement's device form ("device")."""
    out = []
    for name in names or cases():
        for local in locals_:
            vol, iso = inputs(name, device)
            want = expected(name, local) if contract == "cpu" else restated(name, local, "device")
            out += misses(fn(vol, iso, local), want, "%s/%d" % (name, local), tolerance(name, local))
    return out


def triangles(lists):
    """verts[faces] per volume, (F, 3, 3); None for `[]`."""
    return [v[f] if torch.is_tensor(f) else None for v, f in zip(*lists)]


def tie_misses(name, device_lists=None):
    """How the device contract is tied to the reference's CPU record (world coordinates): where the reference dropped nothing the
    triangles verts[faces] are the same bits in the same order and there are as many vertices; where it dropped, its triangles are a
    subsequence of the device form's and every run of missing ones begins with a degenerate triangle (the rule of the CPU contract:
    the degenerate triangle and every later one of its cube).  device_lists: the lists to tie (default: the restatement's)."""
    out = []
    want = expected(name, False)
    got = device_lists if device_lists is not None else restated(name, False, "device")
    for n, (a, b) in enumerate(zip(triangles(want), triangles(got))):
        kept = [t.numpy().tobytes() for t in a] if a is not None else []
        mine = list(b.cpu()) if b is not None else []
        k, run = 0, False
        for t in mine:
            if k < len(kept) and t.numpy().tobytes() == kept[k]:
                k, run = k + 1, False
                continue
            if not run and not degenerate(*[t[i].tolist() for i in range(3)]):
                out.append("%s[%d]: a triangle the reference does not have, behind no degenerate one" % (name, n))
            run = True
        if k != len(kept):
            out.append("%s[%d]: the reference's triangles are not a subsequence" % (name, n))
        if len(kept) == len(mine) and len(want[0][n]) != len(got[0][n]):
            out.append("%s[%d]: %d vertices against the reference's %d" % (name, n, len(got[0][n]), len(want[0][n])))
    return out
