"""Install pytorch3d_amd._C as `pytorch3d._C`, so the UNMODIFIED reference Python package
(pytorch3d.renderer.MeshRasterizer, PointsRasterizer, AlphaCompositor, NormWeightedCompositor,
interpolate_face_attributes, ...) runs on the MI355X kernels.

    import pytorch3d_amd.shim as shim
    shim.install()                       # reference already importable, or
    shim.install("/path/to/pytorch3d")   # a source checkout (no build needed: only _C is native)
    from pytorch3d.renderer import MeshRasterizer   # drop-in

`pytorch3d/__init__.py` does not import `_C`; the sub-packages do (`from pytorch3d import _C`),
so the module must be in sys.modules before they are imported.  Operators outside the hot path
(knn, the point_mesh *_array_dist_* operators, pulsar, ...) raise NotImplementedError when called.  The eight point_mesh operators
under `pytorch3d.loss.point_mesh_face_distance` / `point_mesh_edge_distance` ARE served (csrc/point_mesh.hip), so the unmodified
reference losses run under plain `shim.install()`.  So are `_C.sample_farthest_points` and `_C.ball_query` (csrc/fps_ball.hip): the
unmodified `pytorch3d.ops.sample_farthest_points` runs, and so does the forward of `pytorch3d.ops.ball_query`; its backward ends in
`_C.knn_points_backward`, which stays a stub -- patch_python replaces the whole function.  And `_C.points_to_volumes_forward` /
`_backward` (csrc/points_to_volumes.hip): the unmodified `pytorch3d.ops.add_pointclouds_to_volumes` runs, forward and backward.
And `_C.iou_box3d` (csrc/box3d.hip: the kernels for GPU tensors, the library's host loop for CPU tensors): the unmodified
`pytorch3d.ops.box3d_overlap` runs on both.  And `_C.gather_scatter` (csrc/graph_conv.hip): the unmodified `pytorch3d.ops.GraphConv`
runs on the GPU, forward and backward, its neighbour sums added in list order instead of by float atomics.  And `_C.sample_pdf`
(csrc/implicit.hip: the kernel for GPU tensors, the library's host loop for CPU tensors, the same bits from both): the unmodified
`pytorch3d.renderer.implicit.sample_pdf` runs on both.  And `_C.marching_cubes` (csrc/marching_cubes.hip for a GPU volume: every vertex
once, with strictly ascending edge ids, so that the wrapper's torch.unique is the identity; the library's host loop for a CPU volume):
the unmodified `pytorch3d.ops.marching_cubes` runs on both, volume by volume.

    shim.install(patch_python=True)

additionally replaces the reference's pure-torch callers and callees of the operator surface with the
fused HIP versions of this package, so that `MeshRenderer(MeshRasterizer, SoftPhongShader)` built from the UNMODIFIED
reference classes runs on them end to end:

    renderer.mesh.rasterizer.MeshRasterizer.forward           -> camera transform on the PACKED vertices in one launch
                                                                 (csrc/transform.hip) + the fused rasterize_meshes below;
                                                                 gradients to the vertices AND to camera parameters that
                                                                 require grad (R, T, focal_length, principal_point, ...)
    renderer.mesh.rasterize_meshes.rasterize_meshes           -> fused gather + rasterizer (+ HIP clipping), one autograd node
    renderer.mesh.clip.clip_faces / convert_clipped_...       -> csrc/clip.hip
    renderer.mesh.shader.SoftPhongShader.forward              -> csrc/soft_phong.hip: shading + softmax blend in one kernel
                                                                 each way (K in 1, 2, 4, 8, 16), TexturesVertex fused in
    renderer.blending.softmax_rgb_blend / hard_rgb_blend      -> csrc/blend.hip
    renderer.mesh.shading.phong_shading / flat_shading / gouraud_shading -> csrc/shade.hip (+ interp.hip)
    renderer.mesh.textures.TexturesUV / TexturesAtlas .sample_textures   -> csrc/texture*.hip, atlas.hip
    renderer.mesh.shader.Hard{Phong,Gouraud,Flat}Shader.forward -> the shader sees the nearest slot only (hard_rgb_blend keeps
                                                                 nothing else): 1 / K of the shading and texture work
    renderer.mesh.shader.SoftSilhouetteShader.forward         -> no ones_like(bary_coords) (1.6 GB at the bench batch)
    renderer.mesh.shader.HardDepthShader / SoftDepthShader .forward -> csrc/blend.hip: hard_depth / soft_depth, one kernel
                                                                 each way instead of the cat / cumsum / clamp / diff chain
    structures.meshes.Meshes.offset_verts / offset_verts_     -> one add on the packed vertices, topology shared, no host sync
                                                                 (the reference re-runs Meshes.__init__: ~70 syncs per call)
    structures.meshes.Meshes._compute_vertex_normals          -> csrc/normals.hip: vertex normals as a gather over an incidence
                                                                 list kept with the topology (no float atomics, same bits on
                                                                 every run); offset_verts hands the list on, so a fitting loop
                                                                 sorts once.  `_C.face_areas_normals_*` (face normals, flat
                                                                 shading) are HIP kernels of the same file without any patch
    loss.mesh_edge_loss / mesh_laplacian_smoothing ("uniform") / mesh_normal_consistency -> csrc/mesh_losses.hip: one autograd
                                                                 node each over tables kept with the topology, gathers and
                                                                 fixed-tree sums (no float atomics, no host round trip);
                                                                 without patch_python the reference's own normal consistency
                                                                 runs too (`_C.mesh_normal_consistency_find_verts` on the host)
    ops.laplacian_matrices.cot_laplacian / ops.mesh_filtering.taubin_smoothing -> csrc/mesh_laplacian.hip: the cotangent weights per
                                                                 face and edge and the vertex areas as gathers over tables kept per
                                                                 faces tensor (a coalesced L); Taubin smoothing as 2 num_iter
                                                                 launches over the loss tables' adjacency.  The reference's own
                                                                 mesh_laplacian_smoothing("cot" / "cotcurv") finds cot_laplacian
                                                                 served by the kernels (the patched loss keeps "uniform" alone);
                                                                 inputs that want a gradient, CPU tensors and a face that names
                                                                 one vertex twice go to the reference's functions
    ops.knn.knn_points / loss.chamfer.chamfer_distance        -> csrc/knn.hip: brute-force nearest neighbours, one lane per query;
                                                                 chamfer without normals is one autograd node with no host
                                                                 sync; inputs the kernels do not take go to this package's torch
                                                                 formulation (`_C.knn_points_idx` itself stays a stub that raises)
    loss.point_mesh_distance.point_mesh_face_distance / point_mesh_edge_distance -> csrc/point_mesh.hip: one autograd node each (face /
                                                                 edge gather, two fused brute-force forwards with fixed-tree sums,
                                                                 two backward kernels, the vertex scatter) and no host sync; other
                                                                 inputs go to this package's torch formulation
    ops.sample_points_from_meshes.sample_points_from_meshes   -> csrc/sample_points.hip: one autograd node, a deterministic function of
                                                                 ONE torch.rand((N, S, 3)) (torch's multinomial stream is not
                                                                 reproduced: same distribution, other draws); other inputs go to
                                                                 this package's torch formulation
    ops.sample_farthest_points.sample_farthest_points / ops.ball_query.ball_query -> csrc/fps_ball.hip: farthest point sampling with
                                                                 one workgroup per cloud and the cloud in registers; ball query as
                                                                 one autograd node whose backward is the nearest neighbours'; other
                                                                 inputs go to this package's torch formulation

    ops.points_to_volumes.add_pointclouds_to_volumes / add_points_features_to_volume_densities_features -> csrc/points_to_volumes.hip
                                                                 as one autograd node (ordered sum under the strict deterministic
                                                                 flag); CPU tensors go to this package's torch formulation
    ops.points_normals.estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames -> csrc/point_frames.hip: neighbours,
                                                                 covariances, the reference's symeig3x3 and its sign votes in one
                                                                 launch, nothing of size K per point in memory; Pointclouds.
                                                                 estimate_normals comes here through `ops`; K > 64, float64, CPU
                                                                 tensors, eigh and inputs that require grad go to this package's
                                                                 torch formulation
    ops.points_alignment.iterative_closest_point / corresponding_points_alignment -> csrc/points_alignment.hip: per ICP iteration six
                                                                 launches and one 4-byte host read, the 3 x 3 SVD in float64 on
                                                                 the device; CPU tensors, float64, d != 3 and inputs that require
                                                                 grad go to this package's restated chain
    ops.iou_box3d.box3d_overlap                               -> pytorch3d_amd.iou_box3d.box3d_overlap: the same operator (csrc/box3d.hip)
                                                                 behind input checks that cost one host sync instead of four
    ops.graph_conv.GraphConv.forward, ops.graph_conv.gather_scatter
                                                              -> pytorch3d_amd.graph_conv.graph_conv / gather_scatter: one autograd
                                                                 node writes w0 x + the neighbour sums (csrc/graph_conv.hip; no zero
                                                                 fill, no separate add, no atomics)
    ops.vert_align.vert_align                                 -> pytorch3d_amd.vert_align.vert_align: one launch per feature map into
                                                                 one output, strided maps, packed rows straight from the index
                                                                 (csrc/vert_align.hip); an ordered grad_feats under
                                                                 torch.use_deterministic_algorithms(True)

    ops.marching_cubes.marching_cubes                         -> pytorch3d_amd.marching_cubes.marching_cubes: the whole batch in four
                                                                 launches and one host read (the reference: three reads and a
                                                                 torch.unique per volume), isolevel=None included; CPU volumes go
                                                                 to the library's host loop, GPU sizes beyond int32 to this
                                                                 package's torch formulation

    renderer.implicit.raymarching.EmissionAbsorptionRaymarcher.forward / AbsorptionOnlyRaymarcher.forward
                                                              -> pytorch3d_amd.implicit: one autograd node over csrc/implicit.hip's
                                                                 forward and backward kernels (scans along the ray, no division, no
                                                                 atomics, no cat); the reference's input checks and its density
                                                                 bounds warning stay; CPU tensors, float64 and surface_thickness < 1
                                                                 go to this package's torch formulation of the same chain
    renderer.implicit.renderer.VolumeSampler.forward          -> pytorch3d_amd.volume_sampler: the reference's checks and its own
                                                                 world-to-local calls on the Volumes (gradients to translation and
                                                                 voxel size stay with autograd), then one autograd node over
                                                                 csrc/volume_sample.hip: ray points in registers, both grids in one
                                                                 pass, an ordered volume gradient under
                                                                 torch.use_deterministic_algorithms(True); CPU tensors, float64,
                                                                 reflection and bicubic go to the reference's chain restated
    renderer.implicit.harmonic_embedding.HarmonicEmbedding.forward -> pytorch3d_amd.harmonic_embedding: one autograd node over
                                                                 csrc/harmonic.hip on the instance's own buffers (one read of x, one
                                                                 write of the embedding, a backward without atomics); CPU tensors,
                                                                 float64 / half and a broadcast diag_cov go to the chain restated
    renderer.implicit.raysampling._jiggle_within_stratas      -> pytorch3d_amd.raysampling.stratified_depths: the stratified depths of
                                                                 the three ray samplers in one launch from the reference's own draw
                                                                 (the same depths under a seed), the expanded linspace read in place

Every replacement falls back to the reference's own function for inputs the fused kernels do not cover (CPU tensors,
colour widths other than 3, light classes other than Point / Directional / Ambient, padding modes grid_sample has and
the kernels do not).  Cameras that require grad are NOT such an input: MeshRasterizer, PointsRasterizer and the fused
PointsRenderer keep their fused paths and deliver the camera gradients.  The names are replaced in every
loaded `pytorch3d.*` module that imported them (`from .x import f` copies), `uninstall_python_patches()` restores them.
"""
import importlib
import sys
import types

from . import _C as _ours


def _our(module):
    """A sub-module of this package by name (the package re-exports FUNCTIONS named rasterize_meshes, ball_query etc. over the
    sub-modules of the same name, so `from . import ball_query` would not do)."""
    return importlib.import_module(__package__ + "." + module)


# operator of `pytorch3d._C` -> (sub-module of this package, attribute).  "_C" rows are the reference's hot path: the ctypes operators of
# pytorch3d_amd/_C.py, or under the pybind flavour the compiled module's.  Every other row is a Python wrapper that both flavours serve:
# the HIP kernel for the tensors it takes (float32 on the GPU, mostly) and a torch or host formulation of the same contract for the rest.
EXPORTS = {
    **{name: ("_C", name) for name in _ours.HOT_PATH_EXPORTS},
    # what the reference's mesh classes and losses call: face areas / normals (csrc/normals.hip), packed <-> padded (torch), and the
    # host operator of pytorch3d.loss.mesh_normal_consistency (vectorised torch on the CPU)
    **{name: ("_aux_ops", name) for name in ("face_areas_normals_forward", "face_areas_normals_backward", "packed_to_padded",
                                             "padded_to_packed", "mesh_normal_consistency_find_verts")},
    **{name: ("point_mesh", name) for name in _ours.POINT_MESH_EXPORTS},  # pytorch3d.loss.point_mesh_distance (csrc/point_mesh.hip)
    "sample_farthest_points": ("sample_farthest_points", "sample_farthest_points_op"),  # csrc/fps_ball.hip, clouds with D in (2, 3)
    "ball_query": ("ball_query", "ball_query_op"),
    "points_to_volumes_forward": ("points_to_volumes", "points_to_volumes_forward_op"),  # csrc/points_to_volumes.hip; in place
    "points_to_volumes_backward": ("points_to_volumes", "points_to_volumes_backward_op"),
    "iou_box3d": ("iou_box3d", "iou_box3d_op"),  # csrc/box3d.hip; the library's host loop for CPU boxes
    "gather_scatter": ("graph_conv", "gather_scatter_op"),  # csrc/graph_conv.hip; the table of an edge tensor is cached
    "sample_pdf": ("implicit", "sample_pdf_op"),  # csrc/implicit.hip; the library's host loop for CPU tensors; in place
    "marching_cubes": ("marching_cubes", "marching_cubes_op"),  # csrc/marching_cubes.hip; the library's host loop for CPU volumes
}


def make_module(flavour="ctypes"):
    """flavour: "ctypes" -- the operators of pytorch3d_amd/_C.py (ctypes over libp3d_amd.so; row-cover recall, short workspaces,
    CUDA tie order; no compiler needed) -- or "pybind": the same operator set compiled as a torch extension over the same C ABI
    (pytorch3d_amd/csrc/bind.cpp, built by pytorch3d_amd/build_bind.py: INTEGRATION.md section B, the reference's allocation
    pattern and nothing besides)."""
    if flavour not in ("ctypes", "pybind"):
        raise ValueError("flavour must be 'ctypes' or 'pybind'")
    mod = types.ModuleType("pytorch3d._C")
    mod.__doc__ = "pytorch3d._C provided by pytorch3d_amd (MI355X rasterization hot path), %s flavour" % flavour
    mod.__p3d_amd_flavour__ = flavour
    from . import _aux_ops

    src = _ours
    if flavour == "pybind":
        from . import build_bind

        src = build_bind.load()
    for name, (module, attr) in EXPORTS.items():
        setattr(mod, name, getattr(src if module == "_C" else _our(module), attr))
    for name in ("EPS", "MAX_FLOAT", "MAX_INT", "MAX_UINT", "MAX_USHORT", "PULSAR_MAX_GRAD_SPHERES"):
        setattr(mod, name, getattr(_ours, name))
    if flavour == "pybind":
        # the compiled boundary has the two face operators too: the same arguments that take the HIP kernels above take them there
        def compiled(name):
            theirs, ours = getattr(src, name), getattr(_aux_ops, name)

            def call(*args):
                return theirs(*args) if _aux_ops.fused_face_areas_normals(*args[-2:], *args[:-2]) else ours(*args)

            call.__name__ = name
            return call

        for name in ("face_areas_normals_forward", "face_areas_normals_backward"):
            if hasattr(src, name):
                setattr(mod, name, compiled(name))

    def __getattr__(name):  # PEP 562: anything else is outside the hot path
        if name.startswith("__"):
            raise AttributeError(name)

        def _missing(*args, **kwargs):
            raise NotImplementedError(f"pytorch3d._C.{name} is outside the rasterization hot path that "
                                      "pytorch3d_amd implements")

        return _missing

    mod.__getattr__ = __getattr__
    return mod


def install(reference_root=None, patch_python=False, flavour="ctypes"):
    """Register the shim (idempotent).  Returns the module object.  patch_python: see the module docstring; flavour: make_module."""
    if reference_root is not None and reference_root not in sys.path:
        sys.path.insert(0, reference_root)
    existing = sys.modules.get("pytorch3d._C")
    if existing is not None and getattr(existing, "__p3d_amd__", False) and getattr(existing, "__p3d_amd_flavour__", "ctypes") == flavour:
        mod = existing
    else:
        mod = make_module(flavour)
        mod.__p3d_amd__ = True
        sys.modules["pytorch3d._C"] = mod
        pkg = sys.modules.get("pytorch3d")
        if pkg is not None:
            setattr(pkg, "_C", mod)
    if patch_python:
        patch_reference_python()
    return mod


# ---------------------------------------------------------------------------------------------------------------------
# patch_python: the reference's torch formulations around the operator surface -> the fused kernels
# ---------------------------------------------------------------------------------------------------------------------
# patched MeshRasterizer.forward: rasterize un-clipped first and look for vertices behind the near plane afterwards (see there)
SPECULATE_NO_CLIPPING = True

_PATCHED = []  # (owner object, attribute name, original, replacement)
PATCH_CALLS = {}  # name -> [fused calls, fallback calls]: what actually ran (read by tests/run_reference_suite.py)


def _count(name, fused):
    c = PATCH_CALLS.setdefault(name, [0, 0])
    c[0 if fused else 1] += 1


def _replace_everywhere(orig, new):
    """Rebind every `pytorch3d.*` module attribute that IS `orig` (the defining module and all `from x import f` copies)."""
    for mname, mod in list(sys.modules.items()):
        if mod is None or not (mname == "pytorch3d" or mname.startswith("pytorch3d.")):
            continue
        for attr, val in list(vars(mod).items()):
            if val is orig:
                setattr(mod, attr, new)
                _PATCHED.append((mod, attr, orig, new))


def _is_hip_f32(t):
    import torch

    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


def _fragments_ok(fragments):
    import torch

    p2f = getattr(fragments, "pix_to_face", None)
    return (torch.is_tensor(p2f) and p2f.is_cuda and p2f.dtype == torch.int64 and p2f.dim() == 4
            and _is_hip_f32(getattr(fragments, "bary_coords", None)))


_FUSED_LIGHTS = ("PointLights", "DirectionalLights", "AmbientLights")


def _shading_ok(meshes, fragments, lights, cameras, materials, colors=None):
    if not _fragments_ok(fragments) or type(lights).__name__ not in _FUSED_LIGHTS:
        return False
    if colors is not None and not (_is_hip_f32(colors) and colors.shape[-1] == 3 and colors.dim() == 5):
        return False
    if not all(hasattr(materials, a) for a in ("ambient_color", "diffuse_color", "specular_color", "shininess")):
        return False
    if not hasattr(cameras, "get_camera_center"):
        return False
    v = meshes.verts_packed()
    return _is_hip_f32(v) and v.device == fragments.pix_to_face.device


def _wrap(name, orig, ours, usable):
    """`ours` where usable(*args, **kwargs) says so, else the reference's `orig`; counted in PATCH_CALLS either way."""
    def patched(*args, **kwargs):
        ok = False
        try:
            ok = bool(usable(*args, **kwargs))
        except Exception:  # an argument form the probe does not understand: the reference's own code decides
            ok = False
        _count(name, ok)
        return ours(*args, **kwargs) if ok else orig(*args, **kwargs)

    patched.__name__ = getattr(orig, "__name__", name)
    patched.__doc__ = getattr(orig, "__doc__", None)
    patched.__wrapped__ = orig
    patched.__p3d_amd__ = True
    return patched


def patch_reference_python():
    """Idempotent.  The reference package must be importable (install(reference_root) or an installed pytorch3d)."""
    if _PATCHED:
        return
    our_blend = _our("blending")
    our_clip = _our("clip")
    our_rm = _our("rasterize_meshes")
    our_shade = _our("shading")
    our_tex = _our("textures")

    rm = importlib.import_module("pytorch3d.renderer.mesh.rasterize_meshes")
    clip = importlib.import_module("pytorch3d.renderer.mesh.clip")
    blend = importlib.import_module("pytorch3d.renderer.blending")
    shading = importlib.import_module("pytorch3d.renderer.mesh.shading")
    textures = importlib.import_module("pytorch3d.renderer.mesh.textures")
    importlib.import_module("pytorch3d.renderer")  # every module that copied the names must be loaded before rebinding


    # rasterize_meshes(meshes, image_size, blur_radius, faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct,
    #                  clip_barycentric_coords, cull_backfaces, z_clip_value, cull_to_frustum): rasterize_meshes.py:32-250
    def rm_ok(meshes, *a, **k):
        return _is_hip_f32(meshes.verts_packed()) and meshes.faces_packed().is_cuda

    _replace_everywhere(rm.rasterize_meshes, _wrap("rasterize_meshes", rm.rasterize_meshes, our_rm.rasterize_meshes, rm_ok))

    # clip.py:324-734
    def clip_ok(face_verts_unclipped, *a, **k):
        return _is_hip_f32(face_verts_unclipped)

    _replace_everywhere(clip.clip_faces, _wrap("clip_faces", clip.clip_faces, our_clip.clip_faces, clip_ok))

    def conv_ok(pix_to_face_clipped, bary_coords_clipped, clipped_faces):
        return pix_to_face_clipped.is_cuda and _is_hip_f32(bary_coords_clipped)

    _replace_everywhere(clip.convert_clipped_rasterization_to_original_faces,
                        _wrap("convert_clipped_rasterization_to_original_faces", clip.convert_clipped_rasterization_to_original_faces,
                             our_clip.convert_clipped_rasterization_to_original_faces, conv_ok))

    # blending.py:54-88, 147-244
    def blend_ok(colors, fragments, blend_params, **k):
        import torch

        p2f = fragments.pix_to_face
        return (_is_hip_f32(colors) and colors.dim() == 5 and colors.shape[-1] == 3 and p2f.is_cuda
                and p2f.dtype == torch.int64 and tuple(colors.shape[:4]) == tuple(p2f.shape) and p2f.shape[3] >= 1)

    def soft_ok(colors, fragments, blend_params, znear=1.0, zfar=100):
        return blend_ok(colors, fragments, blend_params) and _is_hip_f32(fragments.dists) and _is_hip_f32(fragments.zbuf)

    _replace_everywhere(blend.softmax_rgb_blend, _wrap("softmax_rgb_blend", blend.softmax_rgb_blend, our_blend.softmax_rgb_blend, soft_ok))
    _replace_everywhere(blend.hard_rgb_blend, _wrap("hard_rgb_blend", blend.hard_rgb_blend, our_blend.hard_rgb_blend, blend_ok))

    # shading.py:100-225
    def phong_ok(meshes, fragments, lights, cameras, materials, texels):
        return _shading_ok(meshes, fragments, lights, cameras, materials, texels)

    def gouraud_ok(meshes, fragments, lights, cameras, materials):
        tex = getattr(meshes, "textures", None)
        return (type(tex).__name__ == "TexturesVertex" and _shading_ok(meshes, fragments, lights, cameras, materials)
                and tex.verts_features_packed().shape[-1] == 3)

    _replace_everywhere(shading.phong_shading, _wrap("phong_shading", shading.phong_shading, our_shade.phong_shading, phong_ok))
    _replace_everywhere(shading.flat_shading, _wrap("flat_shading", shading.flat_shading, our_shade.flat_shading, phong_ok))
    _replace_everywhere(shading.gouraud_shading, _wrap("gouraud_shading", shading.gouraud_shading, our_shade.gouraud_shading, gouraud_ok))

    # TexturesUV.sample_textures (textures.py:1190-1313), TexturesAtlas.sample_textures (textures.py:565-612): methods
    import torch

    uv_orig = textures.TexturesUV.sample_textures

    def uv_sample(self, fragments, **kwargs):
        ok = (_fragments_ok(fragments) and not self.isempty() and self.padding_mode in our_tex._PAD
              and self.sampling_mode in our_tex._MODE and _is_hip_f32(self.maps_padded())
              and self.maps_padded().device == fragments.pix_to_face.device)
        ids = self.maps_ids_padded() if ok and hasattr(self, "maps_ids_padded") else None
        if ok and ids is not None and self.maps_padded().shape[1] < 2:
            ok = False
        _count("TexturesUV.sample_textures", ok)
        if not ok:
            return uv_orig(self, fragments, **kwargs)
        faces_verts_uvs = torch.cat([i[j] for i, j in zip(self.verts_uvs_list(), self.faces_uvs_list())])  # textures.py:1218-1221
        return our_tex.sample_textures_uv(fragments, faces_verts_uvs.to(torch.float32), self.maps_padded(), align_corners=self.align_corners,
                                          padding_mode=self.padding_mode, sampling_mode=self.sampling_mode, maps_ids=ids)

    uv_sample.__wrapped__ = uv_orig
    textures.TexturesUV.sample_textures = uv_sample
    _PATCHED.append((textures.TexturesUV, "sample_textures", uv_orig, uv_sample))

    atlas_orig = textures.TexturesAtlas.sample_textures

    def atlas_sample(self, fragments, **kwargs):
        ok = _fragments_ok(fragments) and not self.isempty()
        at = self.atlas_packed() if ok else None
        ok = ok and _is_hip_f32(at) and at.device == fragments.pix_to_face.device and at.shape[1] >= 1 and at.shape[3] >= 1
        _count("TexturesAtlas.sample_textures", ok)
        if not ok:
            return atlas_orig(self, fragments, **kwargs)
        return our_tex.sample_textures_atlas(fragments, at)

    atlas_sample.__wrapped__ = atlas_orig
    textures.TexturesAtlas.sample_textures = atlas_sample
    _PATCHED.append((textures.TexturesAtlas, "sample_textures", atlas_orig, atlas_sample))

    # compositing.py:68-96, 148-175, 227-247: one autograd node for the three modes; no .clone() of features / alphas / indices
    # (the kernels never write them) and the renderer's permuted views go to the C ABI with their strides
    our_comp = _our("compositing")
    comp = importlib.import_module("pytorch3d.renderer.compositing")

    def comp_ok(pointsidx, alphas, pt_clds):
        return (_is_hip_f32(alphas) and _is_hip_f32(pt_clds) and pointsidx.is_cuda and pointsidx.dtype == torch.int64
                and pointsidx.dim() == 4 and tuple(pointsidx.shape) == tuple(alphas.shape) and pt_clds.dim() == 2)

    for fname in ("alpha_composite", "norm_weighted_sum", "weighted_sum"):
        _replace_everywhere(getattr(comp, fname), _wrap(fname, getattr(comp, fname), getattr(our_comp, fname), comp_ok))

    _patch_mesh_rasterizer(our_rm)
    _patch_points_rasterizer(our_rm)
    _patch_soft_phong_shader(our_shade)
    _patch_splatter_phong_shader(_our("splatter"))
    _patch_meshes_offset_verts()
    _patch_meshes_vertex_normals()
    _patch_hard_and_silhouette_shaders()
    _patch_depth_shaders(our_blend)
    for ref_module, load_first, replacements in _FUNCTION_PATCHES:
        _rebind(ref_module, load_first, replacements)


def _rebind(ref_module, load_first, replacements):
    """Replace functions of the reference module named `ref_module`, in every module that copied their names: `load_first` names the
    packages that did (pytorch3d.ops, pytorch3d.loss), which must be loaded before rebinding.  A reference checkout without one of
    these modules: nothing to patch.  replacements(ref) -> {name: replacement}; each gets the original's docstring (unless it
    brought one) and `__wrapped__`."""
    try:
        ref = importlib.import_module(ref_module)
        for package in load_first:
            importlib.import_module(package)
    except ImportError:
        return
    for name, new in replacements(ref).items():
        orig = getattr(ref, name)
        if new.__doc__ is None:
            new.__doc__ = getattr(orig, "__doc__", None)
        new.__wrapped__ = orig
        new.__p3d_amd__ = True
        _replace_everywhere(orig, new)


# The replacements of _FUNCTION_PATCHES restate the reference's signatures and defaults and hand the call to this package's function
# of the same name, which takes the HIP kernels for the inputs they cover and OUR torch formulation of the same contract for
# everything else (never the reference's function, unless said).  PATCH_CALLS counts the kernel calls as fused and the formulation
# as fallbacks; where the count follows the call, a call that raised is not counted.

def _mesh_loss(ref):
    """pytorch3d.loss.mesh_edge_loss / mesh_laplacian_smoothing / mesh_normal_consistency (loss/mesh_*.py), what every mesh-fitting
    tutorial of the reference adds to the rendered loss each step -> pytorch3d_amd.mesh_losses: one autograd node each over tables
    kept with the topology (csrc/mesh_losses.hip: gathers and fixed-tree sums, no float atomics, no host round trip).  The tables
    live in the object's __dict__ and are inherited by the copies the patched offset_verts makes, so a loop builds them once.  Exact
    Meshes, float32, on the GPU, not empty, no face that names one vertex twice and, for the Laplacian, method "uniform"; anything else
    goes to the reference's function."""
    ours = _our("mesh_losses")
    Meshes = importlib.import_module("pytorch3d.structures.meshes").Meshes

    def usable(meshes, *args, **kwargs):
        if type(meshes) is not Meshes or meshes._N == 0 or not _is_hip_f32(meshes.verts_packed()):
            return False
        empty = meshes.__dict__.get("_p3d_amd_isempty")  # a host sync: asked once per topology (see _patch_meshes_offset_verts)
        if empty is None:
            empty = bool(meshes.isempty())
            meshes.__dict__["_p3d_amd_isempty"] = empty
        # (the tables are built here on the first call and kept; a face that names one vertex twice goes to the reference)
        return not empty and not ours.topology_of(meshes).repeated

    def uniform(meshes, method="uniform"):
        return method == "uniform" and usable(meshes)

    fname = ref.__name__.rsplit(".", 1)[1]  # each of the three modules defines the function of its own name
    return {fname: _wrap(fname, getattr(ref, fname), getattr(ours, fname), uniform if fname == "mesh_laplacian_smoothing" else usable)}


def _cot_laplacian(ref):
    """pytorch3d.ops.laplacian_matrices.cot_laplacian (an uncoalesced sparse V x V matrix and a scatter_add on every call) ->
    pytorch3d_amd.mesh_losses.cot_laplacian: the face and edge kernels of csrc/mesh_laplacian.hip and the area gather over tables
    kept per faces tensor; a COALESCED L with the same dense values.  float32 on the GPU, a non-empty mesh, no face that names one
    vertex twice and no gradient wanted (the reference's losses call it under no_grad); anything else goes to the reference's
    function.  The patched pytorch3d.loss.mesh_laplacian_smoothing keeps its predicate method == "uniform": a "cot" / "cotcurv" call
    runs the reference's loss, which finds this function under its global name."""
    ours = _our("mesh_losses")

    def usable(verts, faces, eps=1e-12):
        if not ours.cot_laplacian_kernel_path(verts, faces):
            return False
        return not ours.cot_tables_of(faces, verts.shape[0]).repeated

    return {"cot_laplacian": _wrap("cot_laplacian", ref.cot_laplacian, ours.cot_laplacian, usable)}


def _taubin_smoothing(ref):
    """pytorch3d.ops.mesh_filtering.taubin_smoothing (two sparse V x V matrices, two torch.sparse.sum and two mm per iteration) ->
    pytorch3d_amd.mesh_filtering.taubin_smoothing: 2 num_iter launches over the adjacency of the loss tables kept with the topology.
    Exact Meshes, float32 on the GPU, not empty, no face that names one vertex twice, no gradient wanted; anything else goes to the
    reference's function.  The result is built as the reference builds it: Meshes(verts=list, faces=meshes.faces_list())."""
    import torch

    ours, losses = _our("mesh_filtering"), _our("mesh_losses")
    Meshes = importlib.import_module("pytorch3d.structures.meshes").Meshes

    def usable(meshes, lambd=0.53, mu=-0.53, num_iter=10):
        if type(meshes) is not Meshes or meshes._N == 0 or int(num_iter) < 0:
            return False
        verts = meshes.verts_packed()
        if not _is_hip_f32(verts) or (torch.is_grad_enabled() and verts.requires_grad):
            return False
        empty = meshes.__dict__.get("_p3d_amd_isempty")  # a host sync: asked once per topology (see _patch_meshes_offset_verts)
        if empty is None:
            empty = bool(meshes.isempty())
            meshes.__dict__["_p3d_amd_isempty"] = empty
        return not empty and not losses.topology_of(meshes).repeated

    return {"taubin_smoothing": _wrap("taubin_smoothing", ref.taubin_smoothing, ours.taubin_smoothing, usable)}


def _knn_points(ref):
    """csrc/knn.hip for float32 GPU clouds with D in {2, 3} and K <= 32.  The reference's own function ends in `_C.knn_points_idx`,
    which stays a stub that raises."""
    ours_knn = _our("knn")

    def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
        _count("knn_points", ours_knn.kernel_path(p1, p2, K))
        return ours_knn.knn_points(p1, p2, lengths1, lengths2, norm, K, version, return_nn, return_sorted)

    return {"knn_points": knn_points}


def _chamfer_distance(ref):
    import torch

    ours_knn = _our("knn")
    ours_chamfer = _our("chamfer")

    def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None, batch_reduction="mean",
                         point_reduction="mean", norm=2, single_directional=False, abs_cosine=True):
        px = x.points_padded() if ours_chamfer._is_cloud_object(x) else x
        py = y.points_padded() if ours_chamfer._is_cloud_object(y) else y
        _count("chamfer_distance", torch.is_tensor(px) and torch.is_tensor(py) and ours_knn.kernel_path(px, py, 1))
        return ours_chamfer.chamfer_distance(x, y, x_lengths, y_lengths, x_normals, y_normals, weights, batch_reduction,
                                             point_reduction, norm, single_directional, abs_cosine)

    return {"chamfer_distance": chamfer_distance}


def _point_mesh_distance(ref):
    """float32 GPU batches are one autograd node over csrc/point_mesh.hip."""
    ours = _our("point_mesh")

    def point_mesh_face_distance(meshes, pcls, min_triangle_area=ours.DEFAULT_MIN_TRIANGLE_AREA):
        _count("point_mesh_face_distance", len(meshes) == len(pcls) and ours.fused_path(meshes, pcls))
        return ours.point_mesh_face_distance(meshes, pcls, min_triangle_area)

    def point_mesh_edge_distance(meshes, pcls):
        _count("point_mesh_edge_distance", len(meshes) == len(pcls) and ours.fused_path(meshes, pcls))
        return ours.point_mesh_edge_distance(meshes, pcls)

    return {"point_mesh_face_distance": point_mesh_face_distance, "point_mesh_edge_distance": point_mesh_edge_distance}


def _sample_points_from_meshes(ref):
    """float32 GPU meshes are one autograd node over csrc/sample_points.hip.  The face choice follows this package's uniforms, not
    torch's multinomial stream.  (In the reference pytorch3d.ops alone copies the name: pytorch3d.loss never imports it.)"""
    ours = _our("sample_points")

    def sample_points_from_meshes(meshes, num_samples=10000, return_normals=False, return_textures=False, **kwargs):
        out = ours.sample_points_from_meshes(meshes, num_samples, return_normals, return_textures, **kwargs)
        _count("sample_points_from_meshes", ours.kernel_path(meshes.verts_packed()))
        return out

    return {"sample_points_from_meshes": sample_points_from_meshes}


def _sample_farthest_points(ref):
    """csrc/fps_ball.hip for float32 GPU clouds with D in {2, 3}."""
    ours_fps = _our("sample_farthest_points")

    def sample_farthest_points(points, lengths=None, K=50, random_start_point=False, **kwargs):
        out = ours_fps.sample_farthest_points(points, lengths, K, random_start_point, **kwargs)
        _count("sample_farthest_points", ours_fps.kernel_path(points))
        return out

    return {"sample_farthest_points": sample_farthest_points}


def _ball_query(ref):
    """csrc/fps_ball.hip for float32 GPU clouds with D in {2, 3}, as one autograd node whose backward is the nearest neighbours'
    kernels, which the reference's own node cannot reach (`_C.knn_points_backward` stays a stub)."""
    ours_ball = _our("ball_query")

    def ball_query(p1, p2, lengths1=None, lengths2=None, K=500, radius=0.2, return_nn=True, skip_points_outside_cube=False):
        out = ours_ball.ball_query(p1, p2, lengths1, lengths2, K, radius, return_nn, skip_points_outside_cube)
        _count("ball_query", ours_ball.kernel_path(p1, p2, int(K)))
        return out

    return {"ball_query": ball_query}


def _points_to_volumes(ref):
    """csrc/points_to_volumes.hip for GPU tensors.  The reference's `_python=True` asks for ITS Python twin, a different function
    (floor, half to even, no align_corners): such a call goes to the reference unchanged."""
    ours = _our("points_to_volumes")
    ref_clouds, ref_tensors = ref.add_pointclouds_to_volumes, ref.add_points_features_to_volume_densities_features

    def add_pointclouds_to_volumes(pointclouds, initial_volumes, mode="trilinear", min_weight=1e-4, rescale_features=True, _python=False):
        if _python:
            return ref_clouds(pointclouds, initial_volumes, mode, min_weight, rescale_features, _python=True)
        out = ours.add_pointclouds_to_volumes(pointclouds, initial_volumes, mode, min_weight, rescale_features)
        _count("add_pointclouds_to_volumes", ours.kernel_path(initial_volumes.densities()))
        return out

    def add_points_features_to_volume_densities_features(points_3d, points_features, volume_densities, volume_features,
                                                         mode="trilinear", min_weight=1e-4, mask=None, grid_sizes=None,
                                                         rescale_features=True, _python=False, align_corners=True):
        if _python:
            return ref_tensors(points_3d, points_features, volume_densities, volume_features, mode, min_weight, mask, grid_sizes,
                               rescale_features, True, align_corners)
        out = ours.add_points_features_to_volume_densities_features(points_3d, points_features, volume_densities, volume_features, mode,
                                                                    min_weight, mask, grid_sizes, rescale_features, align_corners)
        _count("add_points_features_to_volume_densities_features", ours.kernel_path(points_3d, volume_densities))
        return out

    return {"add_pointclouds_to_volumes": add_pointclouds_to_volumes,
            "add_points_features_to_volume_densities_features": add_points_features_to_volume_densities_features}


def _points_normals(ref):
    """csrc/point_frames.hip for float32 GPU clouds with neighborhood_size <= 64, the symeig workaround and no gradient asked for.
    (Pointclouds.estimate_normals resolves `ops.estimate_pointcloud_normals` at call time.)"""
    ours = _our("points_normals")

    def took_kernel(pointclouds, neighborhood_size, use_symeig_workaround):
        return ours.kernel_path(ours._clouds(pointclouds)[0], neighborhood_size, use_symeig_workaround)

    def estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True, *, use_symeig_workaround=True):
        out = ours.estimate_pointcloud_normals(pointclouds, neighborhood_size, disambiguate_directions,
                                               use_symeig_workaround=use_symeig_workaround)
        _count("estimate_pointcloud_normals", took_kernel(pointclouds, neighborhood_size, use_symeig_workaround))
        return out

    def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=50, disambiguate_directions=True, *,
                                               use_symeig_workaround=True):
        out = ours.estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size, disambiguate_directions,
                                                          use_symeig_workaround=use_symeig_workaround)
        _count("estimate_pointcloud_local_coord_frames", took_kernel(pointclouds, neighborhood_size, use_symeig_workaround))
        return out

    return {"estimate_pointcloud_normals": estimate_pointcloud_normals,
            "estimate_pointcloud_local_coord_frames": estimate_pointcloud_local_coord_frames}


def _box3d_overlap(ref):
    """The operator underneath is the one plain install() already serves; the replacement evaluates the reference's four input checks
    with one host sync.  PATCH_CALLS counts GPU calls (the kernels) as fused and CPU calls (the host loop) as fallbacks."""
    ours = _our("iou_box3d")

    def box3d_overlap(boxes1, boxes2, eps=1e-4):
        out = ours.box3d_overlap(boxes1, boxes2, eps)
        _count("box3d_overlap", ours.kernel_path(boxes1, boxes2))
        return out

    return {"box3d_overlap": box3d_overlap}


def _graph_conv(ref):
    """gather_scatter -> this package's (csrc/graph_conv.hip for float32 GPU tensors), and GraphConv.forward -> pytorch3d_amd.graph_conv.
    graph_conv: the two F.linear calls, then ONE node that writes w0 x + the neighbour sums.  The method is patched here directly."""
    ours = _our("graph_conv")

    def gather_scatter(input, edges, directed=False):
        out = ours.gather_scatter(input, edges, directed)
        _count("gather_scatter", ours.kernel_path(input))
        return out

    gather_scatter.__doc__ = getattr(ref.GatherScatter.forward, "__doc__", None)
    orig_forward = ref.GraphConv.forward

    def forward(self, verts, edges):
        out = ours.graph_conv(verts, edges, self.w0.weight, self.w0.bias, self.w1.weight, self.w1.bias, self.directed)
        _count("GraphConv.forward", ours.kernel_path(verts))
        return out

    forward.__doc__ = orig_forward.__doc__
    forward.__wrapped__ = orig_forward
    ref.GraphConv.forward = forward
    _PATCHED.append((ref.GraphConv, "forward", orig_forward, forward))
    return {"gather_scatter": gather_scatter}


def _raymarchers(ref):
    """EmissionAbsorptionRaymarcher.forward / AbsorptionOnlyRaymarcher.forward -> pytorch3d_amd.implicit behind the reference's own
    _check_raymarcher_inputs and _check_density_bounds (the warning and its two host syncs stay).  The methods are patched directly, as
    GraphConv.forward is; PATCH_CALLS counts kernel calls as fused and the torch formulation as fallbacks."""
    ours = _our("implicit")
    ea_orig, ao_orig = ref.EmissionAbsorptionRaymarcher.forward, ref.AbsorptionOnlyRaymarcher.forward

    def ea_forward(self, rays_densities, rays_features, eps=1e-10, **kwargs):
        ref._check_raymarcher_inputs(rays_densities, rays_features, None, z_can_be_none=True, features_can_be_none=False, density_1d=True)
        ref._check_density_bounds(rays_densities)
        out = ours.ea_raymarch_unchecked(rays_densities, rays_features, eps, self.surface_thickness)
        _count("EmissionAbsorptionRaymarcher.forward", ours.kernel_path(rays_densities, rays_features, self.surface_thickness))
        return out

    def ao_forward(self, rays_densities, **kwargs):
        ref._check_raymarcher_inputs(rays_densities, None, None, features_can_be_none=True, z_can_be_none=True, density_1d=True)
        ref._check_density_bounds(rays_densities[..., 0])
        out = ours.absorption_only_raymarch_unchecked(rays_densities)
        _count("AbsorptionOnlyRaymarcher.forward", ours.kernel_path(rays_densities))
        return out

    for cls, orig, new in ((ref.EmissionAbsorptionRaymarcher, ea_orig, ea_forward), (ref.AbsorptionOnlyRaymarcher, ao_orig, ao_forward)):
        new.__name__, new.__doc__, new.__wrapped__, new.__p3d_amd__ = "forward", orig.__doc__, orig, True
        cls.forward = new
        _PATCHED.append((cls, "forward", orig, new))
    return {}


def _volume_sampler(ref):
    """VolumeSampler.forward (renderer/implicit/renderer.py) -> pytorch3d_amd.volume_sampler behind the reference's own checks and its
    own step 1 (Volumes.world_to_local_coords and the module's _get_ray_directions_transform).  There is no `_C` operator under it, so
    plain install() leaves it alone.  The method is patched directly, as the raymarchers' are; PATCH_CALLS counts kernel calls as fused
    and the restated chain as fallbacks."""
    ours = _our("volume_sampler")
    orig = ref.VolumeSampler.forward

    def forward(self, ray_bundle, **kwargs):
        origins_world, directions_world, lengths = ray_bundle.origins, ray_bundle.directions, ray_bundle.lengths
        ref._validate_ray_bundle_variables(origins_world, directions_world, lengths)
        if self._volumes.densities().shape[0] != origins_world.shape[0]:
            raise ValueError("Input volumes have to have the same batch size as rays.")
        origins = self._volumes.world_to_local_coords(origins_world)
        directions = self._get_ray_directions_transform().transform_points(
            directions_world.view(lengths.shape[0], -1, 3)).view(directions_world.shape)
        args = (self._volumes.densities(), self._volumes.features(), origins, directions, lengths)
        out = ours.sample_volumes(*args, sample_mode=self._sample_mode, padding_mode=self._padding_mode,
                                  align_corners=self._volumes.get_align_corners())
        _count("VolumeSampler.forward", ours.kernel_path(*args, self._sample_mode, self._padding_mode))
        return out

    forward.__name__, forward.__doc__, forward.__wrapped__, forward.__p3d_amd__ = "forward", orig.__doc__, orig, True
    ref.VolumeSampler.forward = forward
    _PATCHED.append((ref.VolumeSampler, "forward", orig, forward))
    return {}


def _harmonic_embedding(ref):
    """HarmonicEmbedding.forward (renderer/implicit/harmonic_embedding.py) -> pytorch3d_amd.harmonic_embedding.module_forward on the
    instance's own buffers, so implicitron's and the NeRF project's instances are covered.  The method is patched directly, as the
    raymarchers' are; PATCH_CALLS counts kernel calls as fused and the restated chain as fallbacks."""
    ours = _our("harmonic_embedding")
    orig = ref.HarmonicEmbedding.forward

    def forward(self, x, diag_cov=None, **kwargs):
        out = ours.module_forward(self, x, diag_cov)
        _count("HarmonicEmbedding.forward", ours.module_path(self, x, diag_cov))
        return out

    forward.__name__, forward.__doc__, forward.__wrapped__, forward.__p3d_amd__ = "forward", orig.__doc__, orig, True
    ref.HarmonicEmbedding.forward = forward
    _PATCHED.append((ref.HarmonicEmbedding, "forward", orig, forward))
    return {}


def _stratified_depths(ref):
    """_jiggle_within_stratas of renderer/implicit/raysampling.py, the stratified depths of the three ray samplers ->
    pytorch3d_amd.raysampling.stratified_depths: the expanded linspace is read in place and the depths are written once, from the
    same draw as the reference's.  The samplers resolve the name in their module at call time."""
    ours = _our("raysampling")

    def _jiggle_within_stratas(bin_centers):
        out = ours.stratified_depths(bin_centers)
        _count("_jiggle_within_stratas", ours.kernel_path(bin_centers))
        return out

    return {"_jiggle_within_stratas": _jiggle_within_stratas}


def _vert_align(ref):
    """There is no `_C` operator under the reference's function (it is F.grid_sample and copies), so plain install() leaves it alone.
    csrc/vert_align.hip for float32 GPU calls in a mode the kernels cover, the reference's chain restated for the rest."""
    ours = _our("vert_align")

    def vert_align(feats, verts, return_packed=False, interp_mode="bilinear", padding_mode="zeros", align_corners=True):
        out = ours.vert_align(feats, verts, return_packed, interp_mode, padding_mode, align_corners)
        _count("vert_align", ours.kernel_path(feats, verts, interp_mode, padding_mode))
        return out

    return {"vert_align": vert_align}


def _cubify(ref):
    """pytorch3d.ops.cubify (a torch chain of dozens of launches and N + 2 host syncs; no `_C` operator stands under it, so plain
    install() leaves it alone) -> pytorch3d_amd.cubify: csrc/cubify.hip for float32 GPU grids, our torch formulation of the same
    contract for the rest.  `pytorch3d.ops.cubify` names the module and, on the package, the function: _rebind takes the module from
    importlib and _replace_everywhere rebinds the function in both holders."""
    ours = _our("cubify")

    def cubify(voxels, thresh, *, feats=None, device=None, align="topleft"):
        out = ours.cubify(voxels, thresh, feats=feats, device=device, align=align)
        _count("cubify", ours.kernel_path(voxels, feats, device, align))
        return out

    return {"cubify": cubify}


def _marching_cubes(ref):
    """pytorch3d.ops.marching_cubes (a Python loop over the volumes, each with `_C.marching_cubes`, three host reads and a torch.unique
    on the GPU) -> pytorch3d_amd.marching_cubes: the batch at once.  The reference's pytorch3d.ops does not copy this name (there
    `marching_cubes` is the module); _replace_everywhere rebinds it in the module and in every loaded module that did copy it."""
    ours = _our("marching_cubes")

    def marching_cubes(vol_batch, isolevel=None, return_local_coords=True):
        out = ours.marching_cubes(vol_batch, isolevel, return_local_coords)
        _count("marching_cubes", ours.kernel_path(vol_batch))
        return out

    return {"marching_cubes": marching_cubes}


def _points_alignment(ref):
    """pytorch3d.ops.iterative_closest_point / corresponding_points_alignment (per iteration a knn_points call, a chain of several dozen
    small launches around torch.svd and three host reads) -> pytorch3d_amd.points_alignment: six launches and one 4-byte read per
    iteration for float32 GPU clouds of dimension 3 without a gradient, the package's restated chain for the rest.  The results are
    the reference's own ICPSolution / SimilarityTransform classes; a Pointclouds input gets its Xt through update_padded."""
    ours = _our("points_alignment")

    def iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                                allow_reflection=False, verbose=False):
        fused = ours.kernel_path(X, Y, None, init_transform) and int(max_iterations) > 0
        out = ours.iterative_closest_point(X, Y, init_transform, max_iterations, relative_rmse_thr, estimate_scale, allow_reflection,
                                           verbose)
        _count("iterative_closest_point", fused)
        return ref.ICPSolution(out.converged, out.rmse, out.Xt, ref.SimilarityTransform(*out.RTs),
                               [ref.SimilarityTransform(*t) for t in out.t_history])

    def corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9):
        fused = ours.kernel_path(X, Y, weights)
        out = ours.corresponding_points_alignment(X, Y, weights, estimate_scale, allow_reflection, eps)
        _count("corresponding_points_alignment", fused)
        return ref.SimilarityTransform(*out)

    return {"iterative_closest_point": iterative_closest_point, "corresponding_points_alignment": corresponding_points_alignment}


# (reference module, the packages that copied its names, its replacements), in the order they are applied
_FUNCTION_PATCHES = (
    ("pytorch3d.loss.mesh_edge_loss", ("pytorch3d.loss",), _mesh_loss),
    ("pytorch3d.loss.mesh_laplacian_smoothing", ("pytorch3d.loss",), _mesh_loss),
    ("pytorch3d.loss.mesh_normal_consistency", ("pytorch3d.loss",), _mesh_loss),
    ("pytorch3d.ops.laplacian_matrices", ("pytorch3d.ops", "pytorch3d.loss.mesh_laplacian_smoothing", "pytorch3d.loss"), _cot_laplacian),
    ("pytorch3d.ops.mesh_filtering", ("pytorch3d.ops",), _taubin_smoothing),
    ("pytorch3d.ops.knn", ("pytorch3d.ops", "pytorch3d.loss.chamfer", "pytorch3d.loss"), _knn_points),
    ("pytorch3d.loss.chamfer", ("pytorch3d.loss",), _chamfer_distance),
    ("pytorch3d.loss.point_mesh_distance", ("pytorch3d.loss",), _point_mesh_distance),
    ("pytorch3d.ops.sample_points_from_meshes", ("pytorch3d.ops", "pytorch3d.loss"), _sample_points_from_meshes),
    ("pytorch3d.ops.sample_farthest_points", ("pytorch3d.ops",), _sample_farthest_points),
    ("pytorch3d.ops.ball_query", ("pytorch3d.ops",), _ball_query),
    ("pytorch3d.ops.points_to_volumes", ("pytorch3d.ops",), _points_to_volumes),
    ("pytorch3d.ops.points_normals", ("pytorch3d.ops",), _points_normals),
    ("pytorch3d.ops.points_alignment", ("pytorch3d.ops",), _points_alignment),
    ("pytorch3d.ops.iou_box3d", ("pytorch3d.ops",), _box3d_overlap),
    ("pytorch3d.ops.graph_conv", ("pytorch3d.ops",), _graph_conv),
    ("pytorch3d.ops.vert_align", ("pytorch3d.ops",), _vert_align),
    ("pytorch3d.ops.cubify", ("pytorch3d.ops",), _cubify),
    ("pytorch3d.ops.marching_cubes", ("pytorch3d.ops",), _marching_cubes),
    ("pytorch3d.renderer.implicit.raymarching", (), _raymarchers),
    ("pytorch3d.renderer.implicit.renderer", (), _volume_sampler),
    ("pytorch3d.renderer.implicit.harmonic_embedding", (), _harmonic_embedding),
    ("pytorch3d.renderer.implicit.raysampling", (), _stratified_depths),
)


def camera_matrices(cameras, kwargs):
    """(world -> view, view -> NDC, is_perspective, min znear or None) of `cameras`, or None when they have no matrix form.
    Building them is ~25 small torch launches plus a host sync for znear (`.min().item()`): cached on the camera object
    under a fingerprint of its parameters -- (name, object, in-place version counter) of every tensor attribute, the value of
    every plain one -- whenever the call overrides none of them (kwargs holds nothing but the two objects themselves).
    A new tensor assigned to an attribute, an in-place edit of one, or a different scalar all change the fingerprint."""
    import importlib

    import torch

    cam_utils = importlib.import_module("pytorch3d.renderer.cameras")
    cacheable = all(k in ("cameras", "raster_settings") for k in kwargs)
    fp = None
    if cacheable:
        # every tensor the camera holds: plain attributes AND the nn.Module registries (`_parameters`, `_buffers`: a camera whose
        # R / T were registered as nn.Parameter or buffer keeps them there, not in vars()); a camera that holds a Parameter or a
        # tensor that requires grad is being optimised -- its matrices are rebuilt on every call
        items = [(k, v) for k, v in vars(cameras).items() if not k.startswith("_p3d_amd") and k not in ("_parameters", "_buffers")]
        for reg in ("_parameters", "_buffers"):
            items += [(reg + "." + k, v) for k, v in (vars(cameras).get(reg) or {}).items()]
        if any(torch.is_tensor(v) and (isinstance(v, torch.nn.Parameter) or v.requires_grad) for _, v in items):
            cacheable = False
    if cacheable:
        # (the fingerprint holds the tensor OBJECTS, compared by identity: an id() alone could be reused by a new tensor.  Edits
        # that bypass the version counter -- `cameras.T.data.add_(...)`, an external kernel writing through data_ptr() -- are
        # not seen: INTEGRATION.md lists them as unsupported with the cache; `del cameras._p3d_amd_matrices` drops it)
        fp = tuple((k, v, v._version) if torch.is_tensor(v) else (k, v, None) for k, v in items
                   if torch.is_tensor(v) or isinstance(v, (bool, int, float, str, tuple, type(None))))
        hit = cameras.__dict__.get("_p3d_amd_matrices")
        if hit is not None and len(hit[0]) == len(fp) and all(
                a[0] == b[0] and a[2] == b[2] and (a[1] is b[1] if torch.is_tensor(a[1]) or torch.is_tensor(b[1]) else a[1] == b[1])
                for a, b in zip(hit[0], fp)):
            return hit[1]
    w2v = cameras.get_world_to_view_transform(**kwargs).get_matrix()
    proj = cam_utils.try_get_projection_transform(cameras, kwargs)
    out = None
    if proj is not None:
        v2n = proj.compose(cameras.get_ndc_camera_transform(**kwargs)).get_matrix()
        znear = cameras.get_znear()
        if isinstance(znear, torch.Tensor):
            znear = znear.min().item()
        out = (w2v, v2n, bool(cameras.is_perspective()), znear)
    if cacheable and not (out is not None and (out[0].requires_grad or out[1].requires_grad)):
        cameras.__dict__["_p3d_amd_matrices"] = (fp, out)
    return out



def _patch_mesh_rasterizer(our_rm):
    """MeshRasterizer.forward (rasterizer.py:219-276).  The reference transforms the PADDED vertices with two batched
    4x4 `transform_points` (homogeneous divides, `cat`, `update_padded` -> a new Meshes): ~4 ms of small launches and
    Python per call on the bench batch, more than the rasterization itself.  Here: both matrices from the cameras, one
    kernel on the packed vertices, then the fused rasterize_meshes (its own z-clipping / culling) on a view of the mesh's
    topology.  Cameras that are being optimised stay on this path: their matrices are rebuilt on every call (camera_matrices)
    and the transform's backward sums their gradient in the same pass as the vertices' (p3d_transform_backward_cameras), on
    the un-clipped path and on the z-clip path alike.  Falls back to the reference's forward when the cameras have no matrix
    form or need an `eps`."""
    import importlib

    import torch

    rz = importlib.import_module("pytorch3d.renderer.mesh.rasterizer")
    cam_utils = importlib.import_module("pytorch3d.renderer.cameras")
    orig = rz.MeshRasterizer.forward

    def forward(self, meshes_world, **kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        ok = cameras is not None and kwargs.get("eps", None) is None
        if ok:
            try:
                verts = meshes_world.verts_packed()
                ok = _is_hip_f32(verts) and meshes_world.faces_packed().is_cuda and len(cameras) in (1, len(meshes_world))
                if ok:
                    cm = camera_matrices(cameras, kwargs)
                    ok = cm is not None
                    if ok:
                        w2v, v2n, cam_persp, znear = cm
                        ok = w2v.device == verts.device
            except Exception:
                ok = False
        _count("MeshRasterizer.forward", ok)
        if not ok:
            return orig(self, meshes_world, **kwargs)
        rs = kwargs.get("raster_settings", self.raster_settings)
        clip_bary = rs.clip_barycentric_coords
        if clip_bary is None:
            clip_bary = rs.blur_radius > 0.0
        persp = rs.perspective_correct if rs.perspective_correct is not None else cam_persp
        if rs.z_clip_value is not None:
            z_clip = rs.z_clip_value
        else:
            z_clip = None if not persp or znear is None else znear / 2
        ndc = our_rm.transform_verts_to_ndc(meshes_world, w2v, v2n)
        view = our_rm._PackedVertsView(meshes_world, ndc)
        common = dict(image_size=rs.image_size, blur_radius=rs.blur_radius, faces_per_pixel=rs.faces_per_pixel, bin_size=rs.bin_size,
                      max_faces_per_bin=rs.max_faces_per_bin, clip_barycentric_coords=clip_bary, perspective_correct=persp,
                      cull_backfaces=rs.cull_backfaces)
        if z_clip is not None and not rs.cull_to_frustum and SPECULATE_NO_CLIPPING:
            # Near-plane clipping alone (the default for perspective cameras, rasterizer.py:244-251): a face is cut or dropped iff
            # one of its vertices has z < z_clip (clip.py:381-388, strict).  clip_faces has to tell the host how many faces
            # come out of it -- a sync in the MIDDLE of the forward, behind which the host cannot run ahead (measured: 0.4 ms of
            # idle GPU per step on the bench batch).  Nearly always nothing is behind the plane, so: queue the un-clipped, fully
            # fused rasterization (gather, rasterizer and backward-to-vertices in one node: no face gather, no clip plan, no
            # scatter launch) and ask the device afterwards whether ANY vertex was behind the plane -- one sync at the END of the
            # forward, with the whole forward already running.  If one was (rare): that result is dropped and the clipping
            # path below runs.  (A vertex no face uses can only send a mesh down the slow path, never the other way.)
            behind = (ndc[:, 2] < z_clip).any()
            out = our_rm.rasterize_meshes(view, z_clip_value=None, cull_to_frustum=False, **common)
            if not bool(behind):  # the host sync
                _count("MeshRasterizer.forward: no vertex behind z_clip, un-clipped fused path kept", True)
                return rz.Fragments(pix_to_face=out[0], zbuf=out[1], bary_coords=out[2], dists=out[3])
            _count("MeshRasterizer.forward: no vertex behind z_clip, un-clipped fused path kept", False)
            del out
        p2f, zbuf, bary, dists = our_rm.rasterize_meshes(view, z_clip_value=z_clip, cull_to_frustum=rs.cull_to_frustum, **common)
        return rz.Fragments(pix_to_face=p2f, zbuf=zbuf, bary_coords=bary, dists=dists)

    forward.__wrapped__ = orig
    rz.MeshRasterizer.forward = forward
    _PATCHED.append((rz.MeshRasterizer, "forward", orig, forward))


def _patch_points_rasterizer(our_rm):
    """PointsRasterizer.forward (renderer/points/rasterizer.py:118-168).  The reference transforms the PADDED points with two
    batched 4x4 `transform_points` (four hipBLASLt GEMMs, cat, homogeneous divides, `update_padded` -> a new Pointclouds:
    ~1 ms of GPU time and ~50 small copies per call at 1M points) before `rasterize_points`.  Here: both matrices from the
    cameras, ONE kernel on the packed points (csrc/transform.hip: p3d_transform_verts_forward / _backward, the kernel
    MeshRasterizer.forward uses for vertices: x, y to NDC, z = view depth, as rasterizer.py:140-141 keeps it) and the
    rasterizer's own autograd node; camera parameters that require grad get their gradient from the transform's backward
    (p3d_transform_backward_cameras).  Falls back to the reference's forward when the cameras have no matrix form or need
    an `eps`.

    PointsRenderer.forward (renderer/points/renderer.py:56-76) with the plain PointsRasterizer and AlphaCompositor or NormWeightedCompositor, float32
    (P, C <= 4) features, one scalar radius and K <= 16: the whole chain is pytorch3d_amd.render_points' fused node -- the image is
    formed in the fine kernel's epilogue, the backward is one kernel.  The packed tensors are taken from the cloud's lists when it has
    not packed them yet: `Pointclouds.points_packed()` builds a cloud-index entry per point with arange + bucketize, twice (points and
    features, structures/utils.py:119-154) -- ~30 launches per freshly built cloud for tensors this chain never reads."""
    import importlib

    import torch

    pr = importlib.import_module("pytorch3d.renderer.points.rasterizer")
    rr = importlib.import_module("pytorch3d.renderer.points.renderer")
    pc = importlib.import_module("pytorch3d.renderer.points.compositor")
    structures = importlib.import_module("pytorch3d.structures")
    our_rp = importlib.import_module(__package__ + ".rasterize_points")
    our_rd = importlib.import_module(__package__ + ".render_points")
    orig = pr.PointsRasterizer.forward
    orig_render = rr.PointsRenderer.forward

    def packed_of(clouds, want_features):
        """(points_packed, features_packed or None, first, count) without `_compute_packed` where the cloud still holds its lists."""
        if type(clouds) is structures.Pointclouds and clouds._points_packed is None and clouds._points_list is not None:
            pl = clouds._points_list
            fl = getattr(clouds, "_features_list", None) if want_features else None
            if len(pl) > 0 and all(torch.is_tensor(t) and t.dim() == 2 and t.shape[1] == 3 for t in pl) and (
                    not want_features or (fl is not None and len(fl) == len(pl) and all(torch.is_tensor(t) and t.dim() == 2 for t in fl))):
                count = clouds.num_points_per_cloud()  # built by the constructor
                if len(pl) == 1:
                    first = _small_zeros(pl[0].device)
                    return pl[0], (fl[0] if want_features else None), first, count
                first = torch.cumsum(count, 0) - count
                return torch.cat(pl, 0), (torch.cat(fl, 0) if want_features else None), first, count
        return (clouds.points_packed(), clouds.features_packed() if want_features else None, clouds.cloud_to_packed_first_idx(),
                clouds.num_points_per_cloud())

    def prepare(self, point_clouds, kwargs, want_features=False):
        """(ndc points, features, first, count) when this rasterizer call can run on the package's kernels, else None."""
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None or kwargs.get("eps", None) is not None:
            return None
        try:
            pts, feats, first, count = packed_of(point_clouds, want_features)
            if not (_is_hip_f32(pts) and pts.dim() == 2 and pts.shape[1] == 3 and len(cameras) in (1, len(point_clouds))):
                return None
            cm = camera_matrices(cameras, kwargs)
            if cm is None:
                return None
            w2v, v2n = cm[0], cm[1]
            if w2v.device != pts.device:
                return None
        except Exception:
            return None
        mats = _packed_matrices(our_rm, cameras, w2v, v2n, len(point_clouds), pts.device)
        return our_rm._TransformVerts.apply(pts, first.contiguous(), mats), feats, first, count

    def forward(self, point_clouds, **kwargs):
        got = prepare(self, point_clouds, kwargs)
        _count("PointsRasterizer.forward", got is not None)
        if got is None:
            return orig(self, point_clouds, **kwargs)
        ndc, _, first, count = got
        rs = kwargs.get("raster_settings", self.raster_settings)
        idx, zbuf, dists2 = our_rp.rasterize_points(_PackedPointsView(point_clouds, ndc, first, count), image_size=rs.image_size,
                                                    radius=rs.radius, points_per_pixel=rs.points_per_pixel, bin_size=rs.bin_size,
                                                    max_points_per_bin=rs.max_points_per_bin)
        return pr.PointFragments(idx=idx, zbuf=zbuf, dists=dists2)

    def render(self, point_clouds, **kwargs):
        rz = self.rasterizer
        mode = {pc.AlphaCompositor: "alpha", pc.NormWeightedCompositor: "norm"}.get(type(self.compositor))
        ok = FUSE_POINTS_RENDERER and mode is not None and type(rz).forward is forward
        got = None
        if ok:
            rs = kwargs.get("raster_settings", rz.raster_settings)
            r_w = rz.raster_settings.radius  # renderer.py:62: the weights' radius is the rasterizer's OWN setting
            ok = (isinstance(rs.radius, (float, int)) and not isinstance(rs.radius, bool) and isinstance(r_w, (float, int))
                  and not isinstance(r_w, bool) and r_w > 0 and 0 < int(rs.points_per_pixel) <= our_rd.MAX_FUSED_K)
        if ok:
            got = prepare(rz, point_clouds, kwargs, want_features=True)
            ok = got is not None and our_rd.fusable(got[1], r_w, rs.points_per_pixel)
        _count("PointsRenderer.forward", ok)
        if not ok:
            return orig_render(self, point_clouds, **kwargs)
        ndc, feats, first, count = got
        view = _PackedPointsView(point_clouds, ndc, first, count)
        images, idx, _, _ = our_rd.render_points_alpha(view, feats, image_size=rs.image_size, radius=rs.radius,
                                                       points_per_pixel=rs.points_per_pixel, bin_size=rs.bin_size,
                                                       max_points_per_bin=rs.max_points_per_bin, weight_radius=r_w,
                                                       radius_per_point=_scalar_radius(rs.radius, ndc), compositor=mode)
        background_color = kwargs.get("background_color", self.compositor.background_color)
        if background_color is not None:  # compositor.py:41-46, on (N, C, H, W) views
            images = pc._add_background_color_to_images(idx.long().permute(0, 3, 1, 2), images.permute(0, 3, 1, 2),
                                                        background_color).permute(0, 2, 3, 1)
        return images

    forward.__wrapped__ = orig
    pr.PointsRasterizer.forward = forward
    _PATCHED.append((pr.PointsRasterizer, "forward", orig, forward))
    render.__wrapped__ = orig_render
    rr.PointsRenderer.forward = render
    _PATCHED.append((rr.PointsRenderer, "forward", orig_render, render))


def _packed_matrices(our_rm, cameras, w2v, v2n, n, device):
    """rasterize_meshes._pack_matrices(w2v, v2n) -- one stack + copy per call -- kept on the camera object for as long as
    camera_matrices hands out the SAME two matrix tensors (its cache: the camera's parameters have not changed)."""
    hit = cameras.__dict__.get("_p3d_amd_packed")
    if hit is not None and hit[0] is w2v and hit[1] is v2n and hit[2] == (n, str(device)):
        return hit[3]
    mats = our_rm._pack_matrices(w2v, v2n, n, device)
    if cameras.__dict__.get("_p3d_amd_matrices") is not None and not mats.requires_grad:
        cameras.__dict__["_p3d_amd_packed"] = (w2v, v2n, (n, str(device)), mats)
    return mats


FUSE_POINTS_RENDERER = True  # (tests and profiles switch the fused PointsRenderer off to time / compare the operator chain)
_SMALL = {}


def _small_zeros(device):
    """A cached int64 zeros(1) per device: cloud_to_packed_first_idx of a single cloud (read-only here)."""
    import torch

    key = ("zeros1", str(device))
    if key not in _SMALL:
        _SMALL[key] = torch.zeros(1, dtype=torch.int64, device=device)
    return _SMALL[key]


def _scalar_radius(radius, points):
    """The (P,) radius tensor of a scalar radius; the last one is kept (a renderer is called with the same cloud size over and over,
    and the tensor is read-only inside the package)."""
    import torch

    key = ("radius", str(points.device))
    hit = _SMALL.get(key)
    if hit is not None and hit[0] == (float(radius), points.shape[0]):
        return hit[1]
    t = torch.full((points.shape[0],), float(radius), dtype=torch.float32, device=points.device)
    _SMALL[key] = ((float(radius), points.shape[0]), t)
    return t


class _PackedPointsView:
    """The accessors pytorch3d_amd.rasterize_points reads, with the packed points replaced (everything else is the cloud's)."""

    def __init__(self, clouds, points_packed, first=None, count=None):
        self._clouds, self._points, self._first, self._count = clouds, points_packed, first, count

    def __len__(self):
        return len(self._clouds)

    def points_packed(self):
        return self._points

    def cloud_to_packed_first_idx(self):
        return self._first if self._first is not None else self._clouds.cloud_to_packed_first_idx()

    def num_points_per_cloud(self):
        return self._count if self._count is not None else self._clouds.num_points_per_cloud()

    def padded_to_packed_idx(self):
        return self._clouds.padded_to_packed_idx()

    @property
    def _P(self):
        return self._clouds._P


def _patch_soft_phong_shader(our_shade):
    """SoftPhongShader.forward (shader.py:113-147): texels = meshes.sample_textures(fragments); phong_shading;
    softmax_rgb_blend -> pytorch3d_amd.shading.soft_phong_shading (the colours never reach memory).  With TexturesVertex of
    three channels the texel interpolation is fused in as well.  Falls back to the reference's forward (whose pieces are
    themselves patched) whenever the fused kernels do not cover the call."""
    import importlib

    shader = importlib.import_module("pytorch3d.renderer.mesh.shader")
    shading_mod = importlib.import_module("pytorch3d.renderer.mesh.shading")
    blend_mod = importlib.import_module("pytorch3d.renderer.blending")
    orig = shader.SoftPhongShader.forward

    def forward(self, fragments, meshes, **kwargs):
        try:
            cameras = kwargs.get("cameras", self.cameras)
            lights = kwargs.get("lights", self.lights)
            materials = kwargs.get("materials", self.materials)
            blend_params = kwargs.get("blend_params", self.blend_params)
            ok = (cameras is not None and _shading_ok(meshes, fragments, lights, cameras, materials)
                  and our_shade.soft_phong_supported(fragments) and _is_hip_f32(fragments.dists) and _is_hip_f32(fragments.zbuf)
                  and not getattr(blend_params.background_color, "requires_grad", False))
        except Exception:
            ok = False
        vcol = texels = None
        if ok:
            tex = getattr(meshes, "textures", None)
            if type(tex).__name__ == "TexturesVertex" and tex.verts_features_packed().shape[-1] == 3:
                vcol = tex.verts_features_packed()
                ok = _is_hip_f32(vcol)
            else:
                texels = meshes.sample_textures(fragments)
                ok = _is_hip_f32(texels) and texels.dim() == 5 and texels.shape[-1] == 3
        _count("SoftPhongShader.forward", ok)
        if not ok:
            if texels is not None:
                # the textures were sampled for the probe and turned out not to fit the fused kernel (channels, dtype): finish the
                # reference's own forward with them (shader.py:131-146) instead of letting it sample them a second time
                colors = shading_mod.phong_shading(meshes=meshes, fragments=fragments, texels=texels, lights=lights, cameras=cameras,
                                                   materials=materials)
                return blend_mod.softmax_rgb_blend(colors, fragments, blend_params, znear=kwargs.get("znear", getattr(cameras, "znear", 1.0)),
                                                   zfar=kwargs.get("zfar", getattr(cameras, "zfar", 100.0)))
            return orig(self, fragments, meshes, **kwargs)
        znear = kwargs.get("znear", getattr(cameras, "znear", 1.0))
        zfar = kwargs.get("zfar", getattr(cameras, "zfar", 100.0))
        return our_shade.soft_phong_shading(meshes, fragments, lights, cameras, materials, texels, blend_params, znear=znear, zfar=zfar,
                                            verts_colors_packed=vcol)

    forward.__wrapped__ = orig
    shader.SoftPhongShader.forward = forward
    _PATCHED.append((shader.SoftPhongShader, "forward", orig, forward))


def _patch_splatter_phong_shader(our_splat):
    """SplatterPhongShader.forward (shader.py:309-374): texels = meshes.sample_textures(fragments); _phong_shading_with_pixels on
    the detached fragments; SplatterBlender -> pytorch3d_amd.splatter (fused Phong + interpolation kernels, the reference's
    camera call for the screen transform, one blend kernel; no (N,H,W,K,9,5) tensors).  The sigma warning of
    check_blend_params is kept.  Falls back to the reference's forward for CPU tensors, colour widths other than 3, a
    background colour that requires grad and whatever _shading_ok rejects."""
    import importlib

    shader = importlib.import_module("pytorch3d.renderer.mesh.shader")
    cls = getattr(shader, "SplatterPhongShader", None)
    if cls is None:
        return
    orig = cls.forward

    def forward(self, fragments, meshes, **kwargs):
        try:
            cameras = self._get_cameras(**kwargs)
            lights = kwargs.get("lights", self.lights)
            materials = kwargs.get("materials", self.materials)
            blend_params = kwargs.get("blend_params", self.blend_params)
            ok = (_shading_ok(meshes, fragments, lights, cameras, materials) and hasattr(cameras, "transform_points_screen")
                  and float(blend_params.sigma) > 0.0 and not getattr(blend_params.background_color, "requires_grad", False))
        except Exception:
            ok = False
        texels = None
        if ok:
            texels = meshes.sample_textures(fragments)
            ok = _is_hip_f32(texels) and texels.dim() == 5 and texels.shape[-1] == 3
        _count("SplatterPhongShader.forward", ok)
        if not ok:
            return orig(self, fragments, meshes, **kwargs)
        colors, pixel_coords_cameras = our_splat.phong_shading_with_pixels(meshes, fragments.detach(), lights, cameras, materials,
                                                                           texels)
        self.check_blend_params(blend_params)
        return our_splat.SplatterBlender(tuple(colors.shape[:4]), colors.device)(colors, pixel_coords_cameras, cameras,
                                                                                fragments.pix_to_face < 0, blend_params)

    forward.__wrapped__ = orig
    cls.forward = forward
    _PATCHED.append((cls, "forward", orig, forward))


def _patch_hard_and_silhouette_shaders():
    """HardPhongShader / HardGouraudShader / HardFlatShader (shader.py:81-112, 150-185, 245-275) shade and texture ALL K slots of
    every pixel and then `hard_rgb_blend` keeps slot 0 (blending.py:54-88: `pix_to_face[..., 0]`, `colors[..., 0, :]`): K - 1 of K
    samples are computed, stored and differentiated for nothing.  Here the shader sees the fragments cut to their nearest slot
    (contiguous copies of 1 / K of the data; autograd routes the gradient back into slot 0 of the originals, the other slots
    get the zeros the reference's blend gives them) -- same image, same gradients, 1 / K of the shading and texture work.
    SoftSilhouetteShader (shader.py:277-300) materialises `torch.ones_like(bary_coords)` -- 1.6 GB at the bench batch -- to
    read one constant pixel of it: a stride-0 view of a single 1 serves the reference's `sigmoid_alpha_blend` as well."""
    import importlib

    import torch

    shader = importlib.import_module("pytorch3d.renderer.mesh.shader")
    rz = importlib.import_module("pytorch3d.renderer.mesh.rasterizer")
    blend = importlib.import_module("pytorch3d.renderer.blending")

    def nearest_slot(orig, name):
        def forward(self, fragments, meshes, **kwargs):
            ok = False
            try:
                p2f = fragments.pix_to_face
                ok = torch.is_tensor(p2f) and p2f.dim() == 4 and p2f.shape[3] > 1 and torch.is_tensor(fragments.bary_coords)
            except Exception:
                ok = False
            first = None
            if ok:
                try:  # fragments of another shape than the rasterizer's (a subclass, missing fields): the reference's own path
                    first = rz.Fragments(pix_to_face=fragments.pix_to_face[..., :1].contiguous(), zbuf=fragments.zbuf[..., :1].contiguous(),
                                         bary_coords=fragments.bary_coords[..., :1, :].contiguous(),
                                         dists=fragments.dists[..., :1].contiguous())
                except Exception:
                    first = None
            _count(name + ".forward", first is not None)
            if first is None:
                return orig(self, fragments, meshes, **kwargs)
            return orig(self, first, meshes, **kwargs)

        forward.__wrapped__ = orig
        return forward

    for cls_name in ("HardPhongShader", "HardGouraudShader", "HardFlatShader"):
        cls = getattr(shader, cls_name, None)
        if cls is None:
            continue
        orig = cls.forward
        new = nearest_slot(orig, cls_name)
        cls.forward = new
        _PATCHED.append((cls, "forward", orig, new))

    sil = getattr(shader, "SoftSilhouetteShader", None)
    if sil is not None:
        sil_orig = sil.forward

        def sil_forward(self, fragments, meshes, **kwargs):
            ok = False
            try:
                ok = torch.is_tensor(fragments.bary_coords) and fragments.bary_coords.dim() == 5
            except Exception:
                ok = False
            _count("SoftSilhouetteShader.forward", ok)
            if not ok:
                return sil_orig(self, fragments, meshes, **kwargs)
            b = fragments.bary_coords
            colors = torch.ones((1, 1, 1, 1, 1), dtype=b.dtype, device=b.device).expand(b.shape)  # shader.py:154 without the 12 K bytes per pixel
            blend_params = kwargs.get("blend_params", self.blend_params)
            return blend.sigmoid_alpha_blend(colors, fragments, blend_params)

        sil_forward.__wrapped__ = sil_orig
        sil.forward = sil_forward
        _PATCHED.append((sil, "forward", sil_orig, sil_forward))


def _patch_depth_shaders(our_blend):
    """HardDepthShader.forward (shader.py:392-400) and SoftDepthShader.forward (shader.py:419-445) -> pytorch3d_amd.blending's
    hard_depth_blend / soft_depth_blend: one kernel each way instead of a dozen passes over (N,H,W,K+1) tensors.  Cameras, zfar
    and sigma are resolved as the reference resolves them: cameras from the keyword or the shader (its ValueError when there
    are none), zfar from the keyword, else cameras.zfar, else 100, sigma from the shader's own blend_params.  Falls back to
    the reference's forward for CPU tensors, tensors that are not float32 / int64 / four-dimensional and a zfar that is not
    a number or a one-element tensor without grad (the reference raises its shape error for a longer one)."""
    import importlib

    import torch

    shader = importlib.import_module("pytorch3d.renderer.mesh.shader")

    def zfar_ok(zfar):
        if torch.is_tensor(zfar):
            return zfar.numel() == 1 and not zfar.requires_grad
        return isinstance(zfar, (int, float)) and not isinstance(zfar, bool)

    def frags_ok(fragments, with_dists):
        p2f, zbuf = fragments.pix_to_face, fragments.zbuf
        ok = (torch.is_tensor(p2f) and p2f.is_cuda and p2f.dtype == torch.int64 and p2f.dim() == 4
              and 1 <= p2f.shape[3] <= _ours.kMaxPointsPerPixel and _is_hip_f32(zbuf) and zbuf.shape == p2f.shape
              and zbuf.device == p2f.device)
        if ok and with_dists:
            d = fragments.dists
            ok = _is_hip_f32(d) and d.shape == p2f.shape and d.device == p2f.device
        return ok

    def make(orig, name, soft):
        def forward(self, fragments, meshes, **kwargs):
            if soft and fragments.dists is None:
                raise ValueError("SoftDepthShader requires Fragments.dists to be present.")
            cameras = shader.ShaderBase._get_cameras(self, **kwargs)
            zfar = kwargs.get("zfar", getattr(cameras, "zfar", 100.0))
            try:
                ok = zfar_ok(zfar) and frags_ok(fragments, soft) and (not soft or float(self.blend_params.sigma) > 0.0)
            except Exception:
                ok = False
            _count(name + ".forward", ok)
            if not ok:
                return orig(self, fragments, meshes, **kwargs)
            if soft:
                return our_blend.soft_depth_blend(fragments, self.blend_params, zfar=zfar)
            return our_blend.hard_depth_blend(fragments, zfar=zfar)

        forward.__wrapped__ = orig
        return forward

    for cls_name, soft in (("HardDepthShader", False), ("SoftDepthShader", True)):
        cls = getattr(shader, cls_name, None)
        if cls is None:
            continue
        orig = cls.forward
        new = make(orig, cls_name, soft)
        cls.forward = new
        _PATCHED.append((cls, "forward", orig, new))


def _patch_meshes_offset_verts():
    """Meshes.offset_verts / offset_verts_ (structures/meshes.py:1295-1360), what every mesh-fitting loop of the reference's
    tutorials calls once per step.  The reference clones the whole object -- `clone()` re-runs `Meshes.__init__` on lists
    (per mesh a boolean-mask index of the faces = one host sync each, `int(max())` and `unique()` syncs) and clones ~20
    internal tensors -- and then reads `num_verts_per_mesh().tolist()` from the device: ~4.5 ms of CPU and ~70 syncs per
    call on the 64-mesh bench batch, twice the rasterizer's forward + backward, and the syncs keep the CPU from ever running
    ahead of the GPU (profiles/r03/dropin_breakdown.py).  Here: one elementwise add on the packed vertices; the new object
    SHARES every topology tensor and cache of the old one (faces, packed / padded indices, edges, Laplacian -- none of them
    depends on the vertex positions and the Meshes API has no in-place edit of them; the reference would hand out clones),
    its vertex list is 64 views of the new packed tensor split by sizes kept on the host, the padded vertices are dropped
    (recomputed lazily by `verts_padded()`), face areas / normals and vertex normals are recomputed if and only if the
    original had them, as the reference does, and textures are cloned as `clone()` clones them.  Falls back to the
    reference's method for empty meshes and offsets of another dtype / device / shape."""
    import importlib

    import torch

    meshes_mod = importlib.import_module("pytorch3d.structures.meshes")
    Meshes = meshes_mod.Meshes
    orig = Meshes.offset_verts
    orig_ = Meshes.offset_verts_

    def usable(self, off):
        if type(self) is not Meshes:  # a subclass may keep state of its own that clone() copies and a shared __dict__ would alias
            return False
        v = self.verts_packed()
        # `isempty()` reads `valid.eq(False).all()` from the device: a host sync per call (measured in round 5: 0.95 ms of a 3.0 ms
        # step -- the host waited there for the previous step's backward).  Emptiness is a property of the topology: asked once,
        # kept on the object and inherited by the copies made below, like the vertex counts.
        empty = self.__dict__.get("_p3d_amd_isempty")
        if empty is None:
            empty = bool(self.isempty())
            self.__dict__["_p3d_amd_isempty"] = empty
        return (torch.is_tensor(off) and self._N > 0 and not empty and v.dtype == torch.float32 and off.device == v.device
                and off.dtype == torch.float32 and (off.shape == v.shape or tuple(off.shape) == (3,)))

    def host_sizes(self):
        sizes = self.__dict__.get("_p3d_amd_num_verts")
        if sizes is None:
            sizes = self.num_verts_per_mesh().tolist()  # once per topology: the copies made below inherit it
            self.__dict__["_p3d_amd_num_verts"] = sizes
        return sizes

    def apply(dst, src, off):
        update_normals = tuple(off.shape) != (3,)
        dst._verts_packed = src.verts_packed() + off
        dst._verts_list = list(dst._verts_packed.split(host_sizes(src), 0))
        dst._verts_padded = None
        if update_normals and (src._faces_areas_packed is not None or src._faces_normals_packed is not None):
            dst._compute_face_areas_normals(refresh=True)
        if update_normals and src._verts_normals_packed is not None:
            dst._compute_vertex_normals(refresh=True)
        return dst

    def offset_verts(self, vert_offsets_packed):
        ok = False
        try:
            ok = usable(self, vert_offsets_packed)
        except Exception:
            ok = False
        _count("Meshes.offset_verts", ok)
        if not ok:
            return orig(self, vert_offsets_packed)
        self.verts_list(), self.faces_list()  # the lists exist before they are shared (meshes built from padded tensors)
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        # the list OBJECTS are the copy's own (appending to / replacing an element of new.faces_list() must not show in the original);
        # the tensors in them are shared with the original, where the reference's clone() hands out copies: INTEGRATION.md
        for name in ("_faces_list", "_verts_list"):
            if isinstance(new.__dict__.get(name), list):
                new.__dict__[name] = list(new.__dict__[name])
        if self.textures is not None:
            new.textures = self.textures.clone()
        return apply(new, self, vert_offsets_packed)

    def offset_verts_(self, vert_offsets_packed):
        ok = False
        try:
            ok = usable(self, vert_offsets_packed)
        except Exception:
            ok = False
        _count("Meshes.offset_verts_", ok)
        if not ok:
            return orig_(self, vert_offsets_packed)
        return apply(self, self, vert_offsets_packed)

    offset_verts.__wrapped__ = orig
    offset_verts_.__wrapped__ = orig_
    Meshes.offset_verts = offset_verts
    Meshes.offset_verts_ = offset_verts_
    _PATCHED.append((Meshes, "offset_verts", orig, offset_verts))
    _PATCHED.append((Meshes, "offset_verts_", orig_, offset_verts_))


def _patch_meshes_vertex_normals():
    """Meshes._compute_vertex_normals (structures/meshes.py:884-926), behind verts_normals_packed() and what the patched offset_verts
    re-runs every step of a fitting loop: gather, cross product, three index_add with float atomics, normalize -- and about twice
    that in autograd.  Here: pytorch3d_amd.mesh_normals.verts_normals, two launches each way and no atomics.  The incidence list it
    gathers through depends on the faces alone: it is kept in the object's __dict__ (keyed by the packed faces tensor's address,
    shape and version) and inherited by the copies the patched offset_verts makes, so a loop sorts once.  Exact Meshes, float32, on
    the GPU, not empty; anything else goes to the reference's method."""
    import importlib

    import torch

    from . import mesh_normals

    Meshes = importlib.import_module("pytorch3d.structures.meshes").Meshes
    orig = Meshes._compute_vertex_normals

    def usable(self):
        if type(self) is not Meshes or self._N == 0:
            return False
        v, f = self.verts_packed(), self.faces_packed()
        if not (_is_hip_f32(v) and f.is_cuda and f.dtype == torch.int64 and f.device == v.device):
            return False
        empty = self.__dict__.get("_p3d_amd_isempty")  # a host sync: asked once per topology (see _patch_meshes_offset_verts)
        if empty is None:
            empty = bool(self.isempty())
            self.__dict__["_p3d_amd_isempty"] = empty
        return not empty

    def incidence(self, faces, V):
        key = (faces.data_ptr(), tuple(faces.shape), faces._version, V)
        kept = self.__dict__.get("_p3d_amd_vert_incidence")
        if kept is None or kept[0] != key:
            kept = (key,) + mesh_normals.vert_incidence(faces, V)
            self.__dict__["_p3d_amd_vert_incidence"] = kept
        return kept[1], kept[2]

    def _compute_vertex_normals(self, refresh=False):
        if not (refresh or self._verts_normals_packed is None):
            return
        ok = False
        try:
            ok = usable(self)
        except Exception:
            ok = False
        _count("Meshes._compute_vertex_normals", ok)
        if not ok:
            return orig(self, refresh)
        v, f = self.verts_packed(), self.faces_packed()
        self._verts_normals_packed = mesh_normals.verts_normals(v, f, incidence(self, f, v.shape[0]))

    _compute_vertex_normals.__wrapped__ = orig
    _compute_vertex_normals.__doc__ = orig.__doc__
    Meshes._compute_vertex_normals = _compute_vertex_normals
    _PATCHED.append((Meshes, "_compute_vertex_normals", orig, _compute_vertex_normals))


def uninstall_python_patches():
    """Put the reference's own functions back (the `_C` module stays installed)."""
    while _PATCHED:
        owner, attr, orig, _new = _PATCHED.pop()
        setattr(owner, attr, orig)
