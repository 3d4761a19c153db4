"""ctypes binding of libp3d_amd.so (the C ABI declared in include/p3d_amd.h).

There is no fallback: if the HIP library is missing or cannot be loaded, every operator of this
package raises.  Build it with `python -m pytorch3d_amd.build` (hipcc, gfx950).
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# P3D_LIB_PATH selects an ablation build (profiles/ scripts only; see build.py)
LIB_PATH = os.environ.get("P3D_LIB_PATH") or os.path.join(_HERE, "libp3d_amd.so")

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_uint = ctypes.c_uint
c_f32 = ctypes.c_float
c_f64 = ctypes.c_double
c_ptr = ctypes.c_void_p
c_size = ctypes.c_size_t

ABI_VERSION = 3  # P3D_ABI_VERSION of include/p3d_amd.h

# flags of p3d_rasterize_meshes_ex, p3d_rasterize_points_ex (TIE_ORDER only) / p3d_rasterize_meshes_backward_ex (include/p3d_amd.h)
RASTER_COVER_LIST = 1
RASTER_CUDA_TIE_ORDER = 2
BWD_COVER_HAS_LIST = 1
BWD_MAKE_FACE_PRE = 2
BWD_GRAD_OUT_ZEROED = 8
KNN_MAX_K = 32           # P3D_KNN_MAX_K
KNN_TILE = 512           # P3D_KNN_TILE: p2 points staged per step
KNN_ACCUMULATE_P2 = 1    # P3D_KNN_ACCUMULATE_P2
FRAMES_MAX_K = 64        # P3D_FRAMES_MAX_K: the largest neighbourhood of csrc/point_frames.hip
FRAMES_DISAMBIGUATE = 1  # P3D_FRAMES_DISAMBIGUATE
FRAMES_ROWS_PER_GROUP = 64  # P3D_FRAMES_ROWS_PER_GROUP: query rows of one workgroup of csrc/point_frames.hip
BOX3D_LDS_CAPACITY = 64     # P3D_BOX3D_LDS_CAPACITY: triangles per fragment list of csrc/box3d.hip's first launch
BOX3D_WAVES_PER_GROUP = 4   # P3D_BOX3D_WAVES_PER_GROUP: pairs per workgroup and round of that launch
BOX3D_MAX_GROUPS = 4096     # P3D_BOX3D_MAX_GROUPS: its largest grid; more pairs take the grid-stride loop
NEIGHBOR_SUM_MAX_GROUPS = 2048  # P3D_NEIGHBOR_SUM_MAX_GROUPS: the largest grid of csrc/graph_conv.hip; more row groups take the grid-stride loop
NEIGHBOR_SUM_GROUP_LANES = 256  # lanes of one of its workgroups: 256 / lanes_per_row vertices per round
VERT_ALIGN_NEAREST, VERT_ALIGN_BORDER, VERT_ALIGN_CORNERS = 1, 2, 4  # P3D_VERT_ALIGN_*: flags of csrc/vert_align.hip
VERT_ALIGN_MAX_GROUPS = 4096  # P3D_VERT_ALIGN_MAX_GROUPS: its largest grid
FPS_REGISTER_POINTS = 16384  # P3D_FPS_REGISTER_POINTS: the largest cloud the register form of farthest point sampling holds
POINT_MESH_POINT, POINT_MESH_SEGMENT, POINT_MESH_TRIANGLE = 0, 1, 2  # P3D_POINT_MESH_*: the kind of a query / target object
POINT_MESH_TILE = 64                # P3D_POINT_MESH_TILE: target records staged per wave and step
POINT_MESH_ACCUMULATE_QUERIES = 1   # P3D_POINT_MESH_ACCUMULATE_QUERIES
POINT_MESH_ACCUMULATE_TARGETS = 2   # P3D_POINT_MESH_ACCUMULATE_TARGETS

_SIGNATURES = {
    # name: (restype, [argtypes])
    "p3d_abi_version": (c_int, []),
    "p3d_error_string": (ctypes.c_char_p, [c_int]),
    "p3d_rasterize_meshes_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_int, c_int]),
    "p3d_rasterize_meshes_short_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_int, c_int, c_i64]),
    "p3d_rasterize_meshes_workspace_need_offset": (c_size, [c_i64, c_int, c_int, c_int, c_int, c_int]),
    "p3d_rasterize_meshes": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_f32, c_int, c_int, c_int,
                                     c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_meshes_naive": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_f32, c_int, c_int,
                                           c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "p3d_rasterize_meshes_coarse": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_f32, c_int, c_int, c_ptr,
                                            c_ptr, c_size, c_ptr]),
    "p3d_rasterize_fine_workspace_bytes": (c_size, [c_int, c_int, c_int, c_int]),
    "p3d_rasterize_meshes_fine": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_f32,
                                          c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_size,
                                          c_ptr]),
    "p3d_rasterize_meshes_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int,
                                              c_int, c_int, c_ptr, c_ptr]),
    "p3d_rasterize_meshes_cover_bytes": (c_size, [c_int, c_int, c_int]),
    "p3d_rasterize_meshes_cover_check": (c_int, [c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr]),
    "p3d_rasterize_meshes_cover_list_bytes": (c_size, [c_int, c_int, c_int]),
    "p3d_rasterize_meshes_ex": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_f32, c_int, c_int, c_int, c_int,
                                        c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_uint, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_meshes_verts_ex": (c_int, [c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int,
                                              c_f32, c_int, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_uint,
                                              c_ptr, c_size, c_ptr]),
    "p3d_rasterize_meshes_backward_workspace_bytes": (c_size, [c_int, c_int, c_int]),
    "p3d_gather_face_verts": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "p3d_gather_face_verts_pre": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr]),
    "p3d_rasterize_meshes_backward_ex": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int,
                                                 c_int, c_int, c_int, c_int, c_uint, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_scatter_face_grads": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "p3d_face_areas_normals_forward": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr]),
    "p3d_face_areas_normals_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "p3d_verts_normals_forward_workspace_bytes": (c_size, [c_i64]),
    "p3d_verts_normals_backward_workspace_bytes": (c_size, [c_i64]),
    "p3d_verts_normals_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "p3d_verts_normals_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr]),
    "p3d_mesh_edge_loss_forward_workspace_bytes": (c_size, [c_i64]),
    "p3d_mesh_laplacian_forward_workspace_bytes": (c_size, [c_i64]),
    "p3d_mesh_normal_consistency_forward_workspace_bytes": (c_size, [c_i64]),
    "p3d_mesh_normal_consistency_backward_workspace_bytes": (c_size, [c_i64]),
    "p3d_mesh_edge_loss_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_size, c_ptr, c_ptr]),
    "p3d_mesh_edge_loss_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_ptr]),
    "p3d_mesh_laplacian_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_size, c_ptr, c_ptr]),
    "p3d_mesh_laplacian_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_mesh_normal_consistency_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_size, c_ptr, c_ptr]),
    "p3d_mesh_normal_consistency_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_size,
                                                     c_ptr, c_ptr]),
    "p3d_transform_gather_face_verts": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr, c_ptr]),
    "p3d_transform_verts_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr, c_ptr]),
    "p3d_transform_verts_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr, c_ptr]),
    "p3d_transform_backward_workspace_bytes": (c_size, [c_i64, c_int, c_int]),
    "p3d_transform_backward_cameras": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_int, c_int]),
    "p3d_rasterize_points_short_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_int, c_int, c_i64]),
    "p3d_rasterize_points_workspace_need_offset": (c_size, [c_i64, c_int, c_int, c_int, c_int, c_int]),
    "p3d_rasterize_points_ex": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr,
                                        c_ptr, c_int, c_ptr, c_int, c_f32, c_ptr, c_uint, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_ptr,
                                     c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points_naive": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr, c_ptr,
                                           c_ptr, c_ptr]),
    "p3d_rasterize_points_coarse": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_ptr,
                                            c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points_fine": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points_composite_backward": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int,
                                                        ctypes.c_float, c_ptr, c_ptr, c_ptr]),
    "p3d_rasterize_points_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr,
                                              c_ptr]),
    "p3d_composite_forward": (c_int, [c_int, c_ptr, ctypes.POINTER(c_i64), c_ptr, c_ptr, c_int, c_int, c_i64, c_int, c_int, c_int,
                                      ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_ptr, c_ptr]),
    "p3d_composite_backward": (c_int, [c_int, c_ptr, c_ptr, ctypes.POINTER(c_i64), c_ptr, c_ptr, c_int, c_int, c_i64, c_int, c_int,
                                       c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_ptr, ctypes.POINTER(c_i64), c_ptr,
                                       c_ptr]),
    "p3d_interp_face_attrs_forward": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr]),
    "p3d_interp_face_attrs_backward": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr,
                                               c_ptr]),
    "p3d_interp_face_attrs_backward_nhwk": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_i64, c_int,
                                                    c_ptr, c_ptr, c_ptr]),
    "p3d_clip_faces_plan_bytes": (c_size, [c_i64]),
    "p3d_clip_faces_plan": (c_int, [c_ptr, c_i64, ctypes.POINTER(c_f32), c_int, c_int, c_int, c_f32, c_ptr, c_size,
                                    c_ptr]),
    "p3d_clip_faces_emit": (c_int, [c_ptr, c_i64, c_ptr, c_int, c_ptr, c_size, c_i64, c_i64, c_i64, c_f32, c_int, c_ptr,
                                    c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "p3d_clip_faces_backward": (c_int, [c_ptr, c_i64, c_ptr, c_size, c_i64, c_i64, c_f32, c_int, c_ptr, c_ptr, c_ptr,
                                        c_ptr]),
    "p3d_convert_clipped_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr]),
    "p3d_convert_clipped_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr]),
    "p3d_sigmoid_alpha_blend_forward": (c_int, [c_ptr, c_ptr, c_f32, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_sigmoid_alpha_blend_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_f32, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_softmax_rgb_blend_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_f32, c_f32, ctypes.POINTER(c_f32), c_f32,
                                              c_f32, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_softmax_rgb_blend_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_f32, c_f32, ctypes.POINTER(c_f32),
                                               c_f32, c_f32, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr,
                                               c_ptr]),
    "p3d_phong_shade_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_int, c_i64,
                                        c_ptr, c_ptr]),
    "p3d_phong_shade_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_int, c_int,
                                         c_int, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "p3d_soft_phong_supported_k": (c_int, [c_int]),
    "p3d_soft_phong_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_f32, c_f32,
                                       ctypes.POINTER(c_f32), c_f32, c_f32, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_i64,
                                       c_ptr, c_ptr]),
    "p3d_soft_phong_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_f32, c_f32,
                                        ctypes.POINTER(c_f32), c_f32, c_f32, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_i64,
                                        c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "p3d_sample_uv_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_i64, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_ptr, c_ptr]),
    "p3d_sample_uv_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_i64, c_int, c_int,
                                       c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr]),
    "p3d_sample_uv_multi_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_i64,
                                            c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr]),
    "p3d_sample_uv_multi_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int,
                                             c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr,
                                             c_ptr]),
    "p3d_sample_atlas_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr, c_ptr]),
    "p3d_sample_atlas_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr, c_ptr]),
    "p3d_hard_rgb_blend_forward": (c_int, [c_ptr, c_ptr, ctypes.POINTER(c_f32), c_i64, c_int, c_ptr, c_ptr]),
    "p3d_hard_rgb_blend_backward": (c_int, [c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_soft_depth_blend_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_f32, c_f32, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_soft_depth_blend_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_f32, c_f32, c_i64, c_int, c_ptr, c_ptr, c_ptr]),
    "p3d_hard_depth_blend_forward": (c_int, [c_ptr, c_ptr, c_f32, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_hard_depth_blend_backward": (c_int, [c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "p3d_splatter_blend_backward_workspace_bytes": (c_size, [c_int, c_int, c_int]),
    "p3d_splatter_blend_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_f32, ctypes.POINTER(c_f32), c_int, c_int, c_int, c_int,
                                           c_ptr, c_ptr]),
    "p3d_splatter_blend_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_f32, ctypes.POINTER(c_f32), c_int, c_int, c_int,
                                            c_int, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    # the deterministic backwards (include/p3d_amd.h: *_ordered)
    "p3d_rasterize_meshes_backward_ordered_workspace_bytes": (c_size, [c_i64, c_int, c_i64]),
    "p3d_rasterize_meshes_backward_ordered": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_i64,
                                                      c_int, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_scatter_face_grads_ordered_workspace_bytes": (c_size, [c_i64]),
    "p3d_scatter_face_grads_ordered": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points_backward_ordered_workspace_bytes": (c_size, [c_i64]),
    "p3d_rasterize_points_backward_ordered": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_int, c_ptr,
                                                      c_ptr, c_size, c_ptr]),
    "p3d_rasterize_points_composite_backward_ordered_workspace_bytes": (c_size, [c_int, c_int, c_int, c_int, c_int, c_i64]),
    "p3d_rasterize_points_composite_backward_ordered": (c_int, [c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int,
                                                                c_int, c_int, c_int, c_f32, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_composite_backward_ordered_workspace_bytes": (c_size, [c_int, c_int, c_int, c_int, c_int, c_i64]),
    "p3d_composite_backward_ordered": (c_int, [c_int, c_ptr, c_ptr, ctypes.POINTER(c_i64), c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_i64,
                                               c_int, c_int, c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_ptr,
                                               ctypes.POINTER(c_i64), c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_interp_face_attrs_backward_ordered_workspace_bytes": (c_size, [c_i64, c_i64]),
    "p3d_interp_face_attrs_backward_ordered": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr,
                                                       c_size, c_ptr]),
    # nearest neighbours and chamfer distance (csrc/knn.hip; the ordered scatter: csrc/ordered_bwd.hip)
    "p3d_knn_points_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr]),
    "p3d_chamfer_forward_workspace_bytes": (c_size, [c_i64, c_i64]),
    "p3d_chamfer_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                                    c_size, c_ptr]),
    "p3d_knn_points_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_uint,
                                        c_ptr, c_ptr, c_ptr]),
    "p3d_knn_points_ordered_backward_workspace_bytes": (c_size, [c_i64]),
    "p3d_knn_points_ordered_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_int,
                                                c_int, c_int, c_uint, c_ptr, c_ptr, c_size, c_ptr]),
    # point-mesh distances (csrc/point_mesh.hip; the ordered scatter: csrc/ordered_bwd.hip)
    "p3d_point_mesh_forward_workspace_bytes": (c_size, [c_i64, c_i64]),
    "p3d_point_mesh_forward": (c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_f64, c_int, c_ptr, c_ptr,
                                       c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_point_mesh_backward_workspace_bytes": (c_size, [c_int, c_i64]),
    "p3d_point_mesh_backward": (c_int, [c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_f64, c_uint,
                                        c_ptr, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    # sample_points_from_meshes (csrc/sample_points.hip; the ordered per-face sum: csrc/ordered_bwd.hip)
    "p3d_sample_points_forward_workspace_bytes": (c_size, [c_i64]),
    "p3d_sample_points_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                          c_size, c_ptr]),
    "p3d_sample_points_backward_workspace_bytes": (c_size, [c_i64, c_int, c_i64]),
    "p3d_sample_points_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_size,
                                           c_ptr]),
    # farthest point sampling and ball query (csrc/fps_ball.hip)
    "p3d_sample_farthest_points_workspace_bytes": (c_size, [c_i64, c_i64]),
    "p3d_sample_farthest_points": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_ball_query": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_f32, c_ptr, c_ptr, c_ptr]),
    # point clouds into voxel grids (csrc/points_to_volumes.hip)
    "p3d_points_to_volumes_workspace_bytes": (c_size, [c_i64, c_i64, c_i64, c_int]),
    "p3d_points_to_volumes_keys": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_ptr, c_ptr]),
    "p3d_points_to_volumes_forward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr,
                                              c_ptr, c_ptr, c_f32, c_int, c_int, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_points_to_volumes_backward": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr,
                                               c_ptr, c_ptr, c_f32, c_int, c_int, c_ptr, c_ptr, c_ptr]),
    # point-cloud covariances, curvatures and local coordinate frames (csrc/point_frames.hip)
    "p3d_point_frames_workgroups": (c_i64, [c_i64, c_i64]),
    "p3d_point_frames": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_uint, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    # box3d_overlap (csrc/box3d.hip): the device entry with its LDS capacity argument, and the host loop
    "p3d_iou_box3d_workspace_bytes": (c_size, [c_i64, c_i64]),
    "p3d_iou_box3d": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    "p3d_iou_box3d_host": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    # GraphConv / gather_scatter neighbour sums (csrc/graph_conv.hip): one entry, forward and backward
    "p3d_neighbor_sum": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_i64, c_ptr]),
    # vert_align (csrc/vert_align.hip): one feature map per call; the ordered grad_feat is keys + a stable sort + the segmented sum
    "p3d_vert_align_forward": (c_int, [c_ptr] + [c_i64] * 8 + [c_ptr] + [c_i64] * 4 + [c_ptr, c_i64, c_uint, c_ptr, c_i64, c_ptr]),
    "p3d_vert_align_backward": (c_int, [c_ptr, c_i64, c_ptr] + [c_i64] * 8 + [c_ptr] + [c_i64] * 4 + [c_ptr, c_i64, c_uint, c_ptr]
                                + [c_i64] * 4 + [c_ptr, c_ptr]),
    "p3d_vert_align_workspace_bytes": (c_size, [c_i64, c_i64]),
    "p3d_vert_align_keys": (c_int, [c_i64] * 3 + [c_ptr] + [c_i64] * 4 + [c_ptr, c_i64, c_uint, c_ptr, c_ptr]),
    "p3d_vert_align_ordered_backward": (c_int, [c_ptr] + [c_i64] * 5 + [c_ptr] + [c_i64] * 4 + [c_ptr, c_i64, c_uint, c_ptr, c_ptr, c_ptr]
                                        + [c_i64] * 4 + [c_ptr, c_size, c_ptr]),
    "p3d_profile_enable": (None, [c_int]),
    "p3d_profile_collect": (None, []),
    "p3d_profile_num_entries": (c_int, []),
    "p3d_profile_entry": (ctypes.c_char_p, [c_int, ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_double)]),
    "p3d_profile_reset": (None, []),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lock = threading.Lock()
_lib = None


class ExtensionMissing(RuntimeError):
    pass


def load():
    """Load libp3d_amd.so; raise loudly when it is absent (there is no CPU or eager fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ExtensionMissing(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m pytorch3d_amd.build` "
                "(hipcc --offload-arch=gfx950). pytorch3d_amd has no CPU/eager fallback.")
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 missing
            raise ExtensionMissing(f"cannot load {LIB_PATH}: {e}") from e
        # the version first: a library of another ABI may lack symbols of this one (or keep removed ones)
        lib.p3d_abi_version.restype, lib.p3d_abi_version.argtypes = c_int, []
        if lib.p3d_abi_version() != ABI_VERSION:
            raise ExtensionMissing(f"{LIB_PATH}: ABI version {lib.p3d_abi_version()} != {ABI_VERSION}; rebuild")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(code, where):
    if code != 0:
        msg = load().p3d_error_string(code).decode()
        raise RuntimeError(f"{where}: {msg} (p3d error {code})")


def profile_snapshot():
    """{kernel name: (launches, total_ms)} since the last reset; synchronises the recorded events."""
    lib = load()
    lib.p3d_profile_collect()
    out = {}
    for i in range(lib.p3d_profile_num_entries()):
        n = c_i64(0)
        ms = ctypes.c_double(0.0)
        name = lib.p3d_profile_entry(i, ctypes.byref(n), ctypes.byref(ms))
        if name is not None and n.value > 0:
            out[name.decode()] = (n.value, ms.value)
    return out
