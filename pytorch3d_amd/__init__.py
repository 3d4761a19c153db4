"""pytorch3d_amd -- PyTorch3D's differentiable-rasterization hot path, re-implemented for
AMD MI355X (CDNA4 / gfx950) as hand-written HIP behind a C ABI (include/p3d_amd.h).

    pytorch3d_amd._C                 the `pytorch3d._C` operator surface (drop-in boundary)
    pytorch3d_amd.shim.install()     register it as pytorch3d._C for the unmodified reference
    rasterize_meshes, rasterize_points, alpha_composite, norm_weighted_sum, weighted_sum,
    interpolate_face_attributes      host-side mirrors of the reference's L2 functions
    clip_faces, softmax_rgb_blend, sigmoid_alpha_blend, hard_rgb_blend, phong_shading, sample_textures_uv,
    sample_textures_atlas            the neighbouring steps, fused
    splatter_blend, SplatterBlender  SplatterPhongShader's blend, fused
    hard_depth_blend, soft_depth_blend  HardDepthShader's / SoftDepthShader's depth maps, one kernel each way
    face_areas_normals, verts_normals, vert_incidence  face / vertex normals of a packed batch, fused (vertex normals without atomics)
    mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency, mesh_loss_topology  the regularisers of a fitting loop, fused
    knn_points, knn_gather, chamfer_distance  nearest neighbours between point clouds and the chamfer loss on top, fused
    point_mesh_face_distance, point_mesh_edge_distance, point_face_distance, face_point_distance, point_edge_distance,
    edge_point_distance              distances between a point cloud and the faces / edges of a mesh, fused
    sample_points_from_meshes, sample_points_packed  points drawn from the surface of a mesh batch, a function of given uniforms, fused
    sample_farthest_points, ball_query, masked_gather  farthest point sampling (a cloud in one workgroup's registers) and ball query, fused
    add_pointclouds_to_volumes, add_points_features_to_volume_densities_features  point clouds into voxel grids, in place, fused
    estimate_pointcloud_normals, estimate_pointcloud_local_coord_frames, point_covariances  normals, curvatures and local frames of a
                                     point cloud from its K nearest neighbours, one launch, nothing of size K per point materialised
    box3d_overlap                    exact intersection volume and IoU of oriented 3D boxes, one wave per pair, no list cap
    gather_scatter, graph_conv, graph_topology  GraphConv's neighbour sums through an inverted index: list order, no atomics, one node
    vert_align                       image features pooled at the vertices: one launch per map, strided maps, packed rows direct
    cubify, cubify_packed            voxel occupancy grids to merged cube meshes: five launches and one host read, no atomics
    marching_cubes, marching_cubes_packed, marching_cubes_torch  scalar fields to isosurface meshes: four launches and one host read per
                                     batch, every vertex computed once in the order of the reference's sorted edge ids, no sort, no atomics
    sample_pdf, ea_raymarch, absorption_only_raymarch  hierarchical ray sampling and emission-absorption raymarching, fused, fwd + bwd
    sample_volumes, volume_sampler_forward  voxel grids sampled along rays (VolumeSampler): one node, both grids in one pass, fwd + bwd
    harmonic_embedding, HarmonicEmbedding  the positional encoding of NeRF-style MLPs: one read of x, one write of the embedding, fwd + bwd
    iterative_closest_point, corresponding_points_alignment, apply_similarity_transform  rigid / similarity registration of point
                                     clouds: six launches and one 4-byte host read per ICP iteration, the 3 x 3 SVD in float64 on the device
    cot_laplacian, taubin_smoothing, taubin_smooth_packed  the cotangent Laplacian's entries and Taubin smoothing as gathers over the loss
                                     tables: no sparse matrix per step, no atomics; mesh_laplacian_smoothing "cot" / "cotcurv" are fused too
    stratified_depths                one jiggled depth per bin along every ray, the centres read in place (an expand stays an expand)

Importing the package does not load the HIP library; the first operator call does, and raises
if it is missing (no CPU / eager fallback exists).
"""
from . import _C  # noqa: F401
from .ball_query import ball_query  # noqa: F401
from .blending import (BlendParams, hard_depth_blend, hard_rgb_blend, sigmoid_alpha_blend, soft_depth_blend,  # noqa: F401
                       softmax_rgb_blend)
from .chamfer import chamfer_distance  # noqa: F401
from .cubify import cubify, cubify_packed  # noqa: F401
from .compositing import alpha_composite, norm_weighted_sum, weighted_sum  # noqa: F401
from .implicit import absorption_only_raymarch, ea_raymarch, sample_pdf  # noqa: F401
from .interp_face_attrs import interpolate_face_attributes  # noqa: F401
from .harmonic_embedding import HarmonicEmbedding, harmonic_embedding, harmonic_embedding_torch  # noqa: F401
from .graph_conv import gather_scatter, graph_conv, graph_topology, topology_of_edges  # noqa: F401
from .iou_box3d import box3d_overlap  # noqa: F401
from .knn import knn_gather, knn_points  # noqa: F401
from .marching_cubes import marching_cubes, marching_cubes_packed, marching_cubes_torch  # noqa: F401
from .mesh_filtering import taubin_smooth_packed, taubin_smooth_torch, taubin_smoothing  # noqa: F401
from .mesh_losses import (cot_laplacian, cot_laplacian_torch, cot_tables, mesh_edge_loss, mesh_laplacian_smoothing,  # noqa: F401
                          mesh_loss_topology, mesh_normal_consistency)
from .mesh_normals import face_areas_normals, vert_incidence, verts_normals  # noqa: F401
from .point_mesh import (edge_point_distance, face_point_distance, point_edge_distance, point_face_distance,  # noqa: F401
                         point_mesh_edge_distance, point_mesh_face_distance)
from .points_alignment import (ICPSolution, SimilarityTransform, apply_similarity_transform,  # noqa: F401
                               corresponding_points_alignment, corresponding_points_alignment_torch, iterative_closest_point,
                               iterative_closest_point_torch)
from .points_normals import (estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals,  # noqa: F401
                             point_covariances)
from .points_to_volumes import add_pointclouds_to_volumes, add_points_features_to_volume_densities_features  # noqa: F401
from .volume_sampler import sample_volumes, volume_sampler_forward  # noqa: F401
from .raysampling import stratified_depths, stratified_depths_torch  # noqa: F401
from .rasterize_meshes import rasterize_meshes, rasterize_meshes_world  # noqa: F401
from .rasterize_points import rasterize_points  # noqa: F401
from .render_points import render_points_alpha  # noqa: F401
from .sample_farthest_points import masked_gather, sample_farthest_points  # noqa: F401
from .sample_points import sample_points_from_meshes, sample_points_packed  # noqa: F401
from .shading import (flat_shading, gouraud_shading, phong_shading, phong_shading_vertex_colors,  # noqa: F401
                      soft_phong_shading)
from .splatter import SplatterBlender, phong_shading_with_pixels, splatter_blend  # noqa: F401
from .structures import PackedMeshes, PackedPointclouds  # noqa: F401
from .textures import sample_textures_atlas, sample_textures_uv  # noqa: F401
from .vert_align import vert_align  # noqa: F401

__version__ = "0.2.0"
