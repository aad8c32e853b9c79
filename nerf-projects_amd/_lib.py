"""ctypes binding of libnerf_mi355x.so (include/nerf_mi355x.h).

Loading is explicit and loud: a missing library or a box without a gfx950 GPU raises;
there is no CPU or PyTorch fallback anywhere in this package.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NERF_MI355X_LIB") or os.path.join(HERE, "libnerf_mi355x.so")

NERF_MAX_SKIPS = 8
NERF_NUM_SLOTS = 16

EXPORTS = (
    "nerf_last_error", "nerf_version", "nerf_device_count", "nerf_ctx_create", "nerf_ctx_destroy",
    "nerf_load_weights", "nerf_num_weight_tensors", "nerf_embed", "nerf_mlp_forward", "nerf_run_network",
    "nerf_raw2outputs", "nerf_sample_pdf", "nerf_render_rays", "nerf_profile_enable", "nerf_profile_read",
    "nerf_workspace_bytes", "nerf_generate_rays", "nerf_image_metrics", "nerf_train_step", "nerf_get_weights",
    "nerf_get_gradients", "nerf_stratified_z", "nerf_resample", "nerf_render_frame", "nerf_set_precision",
    "nerf_get_precision", "nerf_precision_status", "nerf_get_adam_state", "nerf_set_adam_state",
    "nerf_shard_bounds", "nerf_render_shard", "nerf_precision_peek", "nerf_precision_check",
    "nerf_precision_detail", "nerf_profile_read_train", "nerf_set_render_precision",
    "nerf_set_view_fold", "nerf_view_fold_status", "nerf_set_ray_view_bias", "nerf_set_tile_schedule",
    "nerf_pack_rays", "nerf_density_grid", "nerf_marching_cubes", "nerf_train_forward", "nerf_train_backward",
    "nerf_zero_grad", "nerf_adam_step", "nerf_occupancy_create", "nerf_occupancy_destroy", "nerf_occupancy_cells",
    "nerf_occupancy_stats", "nerf_render_rays_occ", "nerf_render_frame_occ", "nerf_train_step_occ", "nerf_occupancy_refresh",
    "nerf_grid_create", "nerf_grid_destroy", "nerf_grid_render_rays", "nerf_grid_render_image", "nerf_grid_gen_rays",
    "nerf_grid_sample", "nerf_grid_accelerate", "nerf_grid_drop_skip", "nerf_grid_has_skip", "nerf_grid_project_sh",
    "nerf_grid_fused_backward", "nerf_grid_tv_grad", "nerf_grid_optim_step",
    "nerf_grid_fused_backward_losses", "nerf_grid_render_backward_losses", "nerf_grid_tv_grad_edge",
    "nerf_grid_lattice_density", "nerf_grid_weight_render", "nerf_grid_threshold", "nerf_grid_dilate",
    "nerf_grid_compact_workspace", "nerf_grid_compact", "nerf_grid_gather",
    "nerf_grid_components_occupancy", "nerf_grid_components_workspace", "nerf_grid_components_label",
    "nerf_grid_components_finish", "nerf_grid_components_volumes", "nerf_grid_components_keep", "nerf_grid_copy_rows",
    "nerf_grid_depth_rays", "nerf_grid_depth_image",
    "nerf_grid_render_rays_taped", "nerf_grid_render_backward", "nerf_grid_sample_backward",
    "nerf_grid_depth_rays_taped", "nerf_grid_depth_backward",
    "nerf_grid_floater_heatmap", "nerf_grid_component_view",
    "nerf_grid_half_row_halfs", "nerf_grid_pack_half", "nerf_grid_unpack_half", "nerf_grid_create_half",
    "nerf_grid_median_cut_workspace", "nerf_grid_quantize_median_cut", "nerf_grid_create_palette",
    "nerf_grid_set_background", "nerf_grid_has_background", "nerf_grid_background_rays", "nerf_grid_background_image",
    "nerf_grid_background_sparsify_plan", "nerf_grid_background_gather",
    "nerf_grid_background_rays_taped", "nerf_grid_background_backward", "nerf_grid_background_tv_grad",
    "nerf_grid_background_optim_step",
    "nerf_grid_tv_value_workspace", "nerf_grid_tv_value", "nerf_grid_tv_value_backward",
    "nerf_grid_sparsity_rays", "nerf_grid_sparsity_backward",
    "nerf_grid_dataset_batch", "nerf_grid_rays_to_ndc",
    "nerf_grid_marching_cubes", "nerf_grid_mesh_attributes",
    "nerf_octree_create", "nerf_octree_destroy", "nerf_octree_render_rays", "nerf_octree_render_image",
    "nerf_octree_build_workspace", "nerf_octree_build_from_grid", "nerf_octree_accelerate", "nerf_octree_table_levels",
    "nerf_octree_backward_rays", "nerf_octree_backward_image",
)
NERF_E_INTERNAL = -5
NERF_W_PRECISION, NERF_W_PRECISION_FALLBACK = 1, 2
NERF_GUARD_OFF, NERF_GUARD_REPORT, NERF_GUARD_FALLBACK = 0, 1, 2
NERF_OCC_EVALUATE, NERF_OCC_EMPTY = 0, 1
NERF_TILES_STATIC, NERF_TILES_CLAIMED = 0, 1
NERF_GRID_TV_DENSITY, NERF_GRID_TV_SH = 0, 1
NERF_GRID_OPTIM_RMSPROP, NERF_GRID_OPTIM_SGD = 0, 1
NERF_GRID_DEPTH_EXPECTED, NERF_GRID_DEPTH_THRESHOLD, NERF_GRID_DEPTH_RAYLEN = 0, 1, 2
NERF_GRID_FLOATER_COUNTER_INTS = 8192
NERF_GRID_HALF_LANES_DEFAULT, NERF_GRID_HALF_LANES_SINGLE, NERF_GRID_HALF_LANES_PAIR = 0, 1, 2
NERF_GRID_ORDER_IDENTITY, NERF_GRID_ORDER_PERMUTED, NERF_GRID_ORDER_RANDOM = 0, 1, 2
NERF_GRID_MESH_COLOR_NONE, NERF_GRID_MESH_COLOR_DC, NERF_GRID_MESH_COLOR_SH, NERF_GRID_MESH_COLOR_VIEW = 0, 1, 2, 3
NERF_OCTREE_RGB_SIGMOID, NERF_OCTREE_RGB_RELU_HALF = 0, 1
NERF_OCTREE_MAX_DEPTH = 24


class NerfArch(C.Structure):
    _fields_ = [("D", C.c_int32), ("W", C.c_int32), ("input_ch", C.c_int32), ("input_ch_views", C.c_int32),
                ("output_ch", C.c_int32), ("n_skips", C.c_int32), ("skips", C.c_int32 * NERF_MAX_SKIPS),
                ("use_viewdirs", C.c_int32)]


_FP = C.c_void_p  # device / host float pointers travel as integers


class RenderArgs(C.Structure):
    _fields_ = [("rays", _FP), ("n_rays", C.c_int64), ("ray_stride", C.c_int32), ("N_samples", C.c_int32),
                ("N_importance", C.c_int32), ("slot_coarse", C.c_int32), ("slot_fine", C.c_int32),
                ("lindisp", C.c_int32), ("white_bkgd", C.c_int32), ("perturb", C.c_int32),
                ("t_rand", _FP), ("u_rand", _FP), ("noise0", _FP), ("noise", _FP),
                ("rgb_map", _FP), ("disp_map", _FP), ("acc_map", _FP), ("raw", _FP), ("rgb0", _FP),
                ("disp0", _FP), ("acc0", _FP), ("z_std", _FP), ("z_vals_coarse", _FP),
                ("weights_coarse", _FP), ("z_samples", _FP), ("z_vals_fine", _FP), ("weights_fine", _FP),
                ("depth_map", _FP), ("z_vals_fine_in", _FP), ("stream", C.c_void_p)]


class TrainArgs(C.Structure):
    _fields_ = [("rays", _FP), ("target", _FP), ("n_rays", C.c_int64), ("ray_stride", C.c_int32),
                ("N_samples", C.c_int32), ("N_importance", C.c_int32), ("slot_coarse", C.c_int32),
                ("slot_fine", C.c_int32), ("lindisp", C.c_int32), ("white_bkgd", C.c_int32), ("perturb", C.c_int32),
                ("t_rand", _FP), ("u_rand", _FP), ("noise0", _FP), ("noise", _FP), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("step", C.c_int32),
                ("apply_update", C.c_int32), ("loss", _FP), ("rgb_map", _FP), ("rgb0", _FP), ("stream", C.c_void_p),
                ("z_vals_fine_in", _FP), ("stats", _FP)]


class TrainForwardArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("rays", _FP), ("n_rays", C.c_int64), ("ray_stride", C.c_int32),
                ("N_samples", C.c_int32), ("N_importance", C.c_int32), ("slot_coarse", C.c_int32),
                ("slot_fine", C.c_int32), ("lindisp", C.c_int32), ("white_bkgd", C.c_int32), ("perturb", C.c_int32),
                ("t_rand", _FP), ("u_rand", _FP), ("noise0", _FP), ("noise", _FP), ("z_vals_fine_in", _FP),
                ("rgb_map", _FP), ("disp_map", _FP), ("acc_map", _FP), ("rgb0", _FP), ("disp0", _FP), ("acc0", _FP),
                ("raw", _FP), ("stream", C.c_void_p), ("tape", C.POINTER(C.c_uint64))]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(self)


class TrainBackwardArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("tape", C.c_uint64), ("d_rgb", _FP), ("d_disp", _FP), ("d_acc", _FP),
                ("d_rgb0", _FP), ("d_disp0", _FP), ("d_acc0", _FP), ("d_raw", _FP), ("stream", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(self)


class Camera(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("c2w", C.c_float * 12), ("c2w_static", C.c_float * 12),
                ("has_static", C.c_int32), ("ndc", C.c_int32), ("ndc_focal", C.c_double), ("near", C.c_float),
                ("far", C.c_float), ("use_viewdirs", C.c_int32)]


class FrameArgs(C.Structure):
    _fields_ = [("cam", Camera), ("first_pixel", C.c_int64), ("n_pixels", C.c_int64), ("chunk", C.c_int64),
                ("N_samples", C.c_int32), ("N_importance", C.c_int32), ("slot_coarse", C.c_int32),
                ("slot_fine", C.c_int32), ("lindisp", C.c_int32), ("white_bkgd", C.c_int32), ("rgb_map", _FP),
                ("disp_map", _FP), ("acc_map", _FP), ("rgb0", _FP), ("disp0", _FP), ("acc0", _FP), ("z_std", _FP),
                ("stream", C.c_void_p), ("precision_guard", C.c_int32)]


class GridArgs(C.Structure):
    _fields_ = [("c1", C.c_double * 3), ("c2", C.c_double * 3), ("reso", C.c_int32 * 3), ("slot", C.c_int32),
                ("sigma", _FP), ("stream", C.c_void_p), ("precision_guard", C.c_int32)]


class McArgs(C.Structure):
    _fields_ = [("volume", _FP), ("reso", C.c_int32 * 3), ("iso", C.c_float), ("vertices", _FP),
                ("vertex_capacity", C.c_int64), ("triangles", _FP), ("triangle_capacity", C.c_int64),
                ("n_vertices", C.POINTER(C.c_int64)), ("n_triangles", C.POINTER(C.c_int64)), ("stream", C.c_void_p)]


class OccupancyArgs(C.Structure):
    _fields_ = [("c1", C.c_double * 3), ("c2", C.c_double * 3), ("reso", C.c_int32 * 3), ("n_lattices", C.c_int32),
                ("sigma", C.POINTER(C.c_void_p)), ("cell_mask", _FP), ("threshold", C.c_float), ("dilate", C.c_int32),
                ("outside", C.c_int32), ("stream", C.c_void_p)]


class _Sized(C.Structure):
    """A struct that begins with a checked ``size_t struct_size``."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(self)


class SparseGridDesc(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("basis_dim", C.c_int32), ("radius", C.c_float * 3),
                ("center", C.c_float * 3), ("capacity", C.c_int64), ("links", _FP), ("density_data", _FP), ("sh_data", _FP),
                ("stream", C.c_void_p)]


class GridRenderOptions(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("step_size", C.c_float), ("sigma_thresh", C.c_float),
                ("stop_thresh", C.c_float), ("background_brightness", C.c_float), ("near_clip", C.c_float),
                ("last_sample_opaque", C.c_int32), ("randomize", C.c_int32)]


class GridCamera(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("c2w", C.c_float * 12), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("ndc_coeffs", C.c_float * 2)]


class GridRaysToNdcArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n", C.c_int64), ("ndc_coeffs", C.c_float * 2),
                ("origins_out", _FP), ("dirs_out", _FP), ("stream", C.c_void_p)]


class GridRenderArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("rgb", _FP),
                ("log_transmit", _FP), ("counters", _FP), ("use_skip", C.c_int32), ("stream", C.c_void_p)]


class GridSampleArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("points", _FP), ("n", C.c_int64), ("grid_coords", C.c_int32),
                ("want_colors", C.c_int32), ("density", _FP), ("sh", _FP), ("stream", C.c_void_p)]


class GridProjectArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("raw", _FP), ("m", C.c_int64), ("n_dirs", C.c_int32), ("basis_dim", C.c_int32),
                ("P", _FP), ("sh_out", _FP), ("row0", C.c_int64), ("stream", C.c_void_p)]


class GridFusedArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("rgb_gt", _FP), ("n_rays", C.c_int64),
                ("rgb_out", _FP), ("log_transmit", _FP), ("grad_density", _FP), ("grad_sh", _FP), ("mask", _FP),
                ("beta_loss", C.c_float), ("sparsity_loss", C.c_float), ("background_nlayers", C.c_int32),
                ("use_skip", C.c_int32), ("stream", C.c_void_p)]


class GridTvArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("target", C.c_int32), ("start_dim", C.c_int32), ("end_dim", C.c_int32),
                ("start", C.c_int64), ("count", C.c_int64), ("scale", C.c_float), ("ignore_edge", C.c_int32),
                ("ignore_last_z", C.c_int32), ("use_ndc", C.c_int32), ("grad", _FP), ("mask", _FP), ("stream", C.c_void_p)]


class GridOptimArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("data", _FP), ("rms", _FP), ("grad", _FP), ("mask", _FP), ("rows", C.c_int64),
                ("cols", C.c_int32), ("kind", C.c_int32), ("beta", C.c_float), ("lr", C.c_float), ("eps", C.c_float),
                ("minval", C.c_float), ("stream", C.c_void_p)]


class GridRenderTapedArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("rgb_out", _FP),
                ("log_transmit", _FP), ("tape", _FP), ("use_skip", C.c_int32), ("stream", C.c_void_p)]


class GridRenderBackwardArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("grad_rgb", _FP),
                ("tape", _FP), ("grad_density", _FP), ("grad_sh", _FP), ("mask", _FP), ("use_skip", C.c_int32),
                ("stream", C.c_void_p)]


class GridRenderBackwardLossesArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("beta_loss", C.c_float), ("sparsity_loss", C.c_float), ("log_transmit", _FP)]


class GridSampleBackwardArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("points", _FP), ("n", C.c_int64), ("grid_coords", C.c_int32),
                ("want_colors", C.c_int32), ("grad_out_density", _FP), ("grad_out_sh", _FP), ("grad_density", _FP),
                ("grad_sh", _FP), ("stream", C.c_void_p)]


class GridLatticeArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("xs", _FP), ("ys", _FP), ("zs", _FP), ("density", _FP),
                ("stream", C.c_void_p)]


class GridWeightArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("radius", C.c_float * 3), ("center", C.c_float * 3),
                ("density", _FP), ("max_weight", _FP), ("step_size", C.c_float), ("stop_thresh", C.c_float),
                ("last_sample_opaque", C.c_int32), ("stream", C.c_void_p)]


class GridCompactArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("mask", _FP), ("links", _FP), ("block_offsets", _FP),
                ("count", _FP), ("stream", C.c_void_p)]


class GridGatherArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("xs", _FP), ("ys", _FP), ("zs", _FP), ("links", _FP),
                ("lattice_density", _FP), ("rows", C.c_int64), ("node_of_row", _FP), ("density_data", _FP), ("sh_data", _FP),
                ("stream", C.c_void_p)]


class GridOccupancyArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("use_density", C.c_int32), ("threshold", C.c_float), ("occupied", _FP),
                ("stream", C.c_void_p)]


class GridLabelArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("connectivity", C.c_int32), ("occupied", _FP),
                ("parent", _FP), ("block_offsets", _FP), ("labels", _FP), ("status", _FP), ("stream", C.c_void_p)]


class GridCopyRowsArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("cols", C.c_int32), ("old_links", _FP),
                ("new_links", _FP), ("old_rows", C.c_int64), ("new_rows", C.c_int64), ("old_density", _FP), ("old_sh", _FP),
                ("src_row", _FP), ("density", _FP), ("sh", _FP), ("stream", C.c_void_p)]


class GridDepthArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("mode", C.c_int32), ("sigma_thresh", C.c_float), ("origins", _FP), ("dirs", _FP),
                ("n_rays", C.c_int64), ("depth", _FP), ("log_transmit", _FP), ("use_skip", C.c_int32), ("stream", C.c_void_p)]


class GridDepthTapedArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("depth", _FP),
                ("log_transmit", _FP), ("tape", _FP), ("use_skip", C.c_int32), ("stream", C.c_void_p)]


class GridDepthBackwardArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("grad_depth", _FP),
                ("grad_log_transmit", _FP), ("tape", _FP), ("grad_density", _FP), ("use_skip", C.c_int32),
                ("stream", C.c_void_p)]


class GridFloaterHeatmapArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("labels", _FP), ("table", _FP), ("n_labels", C.c_int64), ("radius", C.c_float * 3),
                ("center", C.c_float * 3), ("w2c", C.c_float * 12), ("min_density", C.c_float), ("filter_occluded", C.c_int32),
                ("depth", _FP), ("out_width", C.c_int32), ("out_height", C.c_int32), ("counts", _FP), ("counters", _FP),
                ("counter_slots", _FP), ("heatmap", _FP), ("stream", C.c_void_p)]


class GridComponentViewArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("labels", _FP), ("table", _FP), ("n_labels", C.c_int64), ("radius", C.c_float * 3),
                ("center", C.c_float * 3), ("w2c", C.c_float * 12), ("keys", _FP), ("slots", _FP), ("stream", C.c_void_p)]


class GridHalfDesc(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("basis_dim", C.c_int32), ("radius", C.c_float * 3),
                ("center", C.c_float * 3), ("capacity", C.c_int64), ("links", _FP), ("density_data", _FP), ("sh_half", _FP),
                ("lanes", C.c_int32), ("stream", C.c_void_p)]


class GridPackHalfArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("basis_dim", C.c_int32), ("capacity", C.c_int64), ("row0", C.c_int64),
                ("rows", C.c_int64), ("sh_data", _FP), ("sh_half", _FP), ("clamped", _FP), ("stream", C.c_void_p)]


class GridMedianCutArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("m", C.c_int64), ("bits", C.c_int32), ("colors", _FP), ("ids", _FP),
                ("palette", _FP), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("nonfinite", C.POINTER(C.c_int64)),
                ("stream", C.c_void_p)]


class GridPaletteDesc(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("reso", C.c_int32 * 3), ("basis_dim", C.c_int32), ("radius", C.c_float * 3),
                ("center", C.c_float * 3), ("capacity", C.c_int64), ("bits", C.c_int32), ("retain", C.c_int32), ("links", _FP),
                ("density_data", _FP), ("quant_map", _FP), ("quant_colors", _FP), ("data_retained", _FP), ("stream", C.c_void_p)]


class GridBackgroundDesc(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("nlayers", C.c_int32), ("reso", C.c_int32), ("capacity", C.c_int64),
                ("links", _FP), ("data", _FP), ("stream", C.c_void_p)]


class GridBackgroundArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("rgb", _FP),
                ("log_transmit", _FP), ("stream", C.c_void_p)]


class GridBackgroundSparsifyArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("nlayers", C.c_int32), ("reso", C.c_int32), ("capacity", C.c_int64),
                ("links", _FP), ("data", _FP), ("sigma_thresh", C.c_float), ("dilate", C.c_int32), ("mask", _FP), ("keep", _FP),
                ("block_offsets", _FP), ("new_links", _FP), ("count", _FP), ("stream", C.c_void_p)]


class GridBackgroundGatherArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("nlayers", C.c_int32), ("reso", C.c_int32), ("capacity", C.c_int64),
                ("links", _FP), ("data", _FP), ("new_links", _FP), ("new_capacity", C.c_int64), ("new_data", _FP),
                ("stream", C.c_void_p)]


class GridBackgroundTapedArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("rgb", _FP),
                ("log_transmit", _FP), ("log_transmit_out", _FP), ("tape", _FP), ("tape_background", _FP),
                ("stream", C.c_void_p)]


class GridBackgroundBackwardArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("grad_rgb", _FP),
                ("log_transmit", _FP), ("tape_background", _FP), ("grad_background", _FP), ("mask_background", _FP),
                ("sparsity_loss", C.c_float), ("beta_loss", C.c_float), ("stream", C.c_void_p)]


class GridBackgroundTvArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("start", C.c_int64), ("count", C.c_int64), ("scale_sigma", C.c_float),
                ("scale_color", C.c_float), ("grad", _FP), ("mask", _FP), ("stream", C.c_void_p)]


class GridBackgroundOptimArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("data", _FP), ("rms", _FP), ("grad", _FP), ("mask", _FP), ("rows", C.c_int64),
                ("kind", C.c_int32), ("beta", C.c_float), ("lr_sigma", C.c_float), ("lr_color", C.c_float), ("eps", C.c_float),
                ("minval", C.c_float), ("stream", C.c_void_p)]


class GridTvValueArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("target", C.c_int32), ("start_dim", C.c_int32), ("end_dim", C.c_int32),
                ("ignore_edge", C.c_int32), ("cells", _FP), ("cells_int64", C.c_int32), ("n_cells", C.c_int64),
                ("partials", _FP), ("value", _FP), ("grad_value", _FP), ("grad", _FP), ("stream", C.c_void_p)]


class GridSparsityArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("sparsity", _FP),
                ("grad_sparsity", _FP), ("grad_density", _FP), ("use_skip", C.c_int32), ("stream", C.c_void_p)]


class GridDatasetBatchArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("images", _FP), ("c2w", _FP), ("n_images", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("channels", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("white_bkgd", C.c_int32), ("factor", C.c_int32), ("order", C.c_int32), ("key", C.c_uint64),
                ("begin", C.c_int64), ("n", C.c_int64), ("origins", _FP), ("dirs", _FP), ("rgb", _FP), ("indices", _FP),
                ("stream", C.c_void_p), ("ndc_coeffs", C.c_float * 2)]


class GridMcArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("mask", _FP), ("iso", C.c_float), ("vertices", _FP),
                ("vertex_capacity", C.c_int64), ("triangles", _FP), ("triangle_capacity", C.c_int64),
                ("n_vertices", C.POINTER(C.c_int64)), ("n_triangles", C.POINTER(C.c_int64)), ("stream", C.c_void_p)]


class GridMeshAttributesArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("points", _FP), ("n", C.c_int64), ("mask", _FP), ("color_mode", C.c_int32),
                ("view", C.c_float * 3), ("normals", _FP), ("colors", _FP), ("stream", C.c_void_p)]


class OctreeDesc(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("n_nodes", C.c_int64), ("data_dim", C.c_int32), ("max_depth", C.c_int32),
                ("rgb_activation", C.c_int32), ("invradius", C.c_float * 3), ("offset", C.c_float * 3), ("child", _FP),
                ("data", _FP), ("stream", C.c_void_p)]


class OctreeRenderOptions(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("step_size", C.c_float), ("sigma_thresh", C.c_float),
                ("stop_thresh", C.c_float), ("background_brightness", C.c_float)]


class OctreeRenderArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("rgb", _FP),
                ("steps", _FP), ("capped", _FP), ("stream", C.c_void_p)]


class OctreeBackwardArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("origins", _FP), ("dirs", _FP), ("n_rays", C.c_int64), ("grad_rgb", _FP),
                ("rgb_gt", _FP), ("loss_scale", C.c_float), ("grad_data", _FP), ("loss", _FP), ("rgb", _FP), ("capped", _FP),
                ("stream", C.c_void_p)]


class OctreeBuildArgs(_Sized):
    _fields_ = [("struct_size", C.c_size_t), ("workspace", _FP), ("workspace_bytes", C.c_int64),
                ("n_nodes", C.POINTER(C.c_int64)), ("child", _FP), ("parent_depth", _FP), ("data", _FP), ("stream", C.c_void_p)]


_lib = None


def library_path():
    return LIB_PATH


def load():
    """dlopen the library once and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python nerf-projects_amd/build.py` "
            "(or __graft_entry__.build()). This package has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    i32, i64, vp = C.c_int, C.c_int64, C.c_void_p
    lib.nerf_last_error.restype = C.c_char_p
    lib.nerf_last_error.argtypes = []
    lib.nerf_version.restype = C.c_char_p
    lib.nerf_version.argtypes = []
    lib.nerf_device_count.restype = i32
    lib.nerf_device_count.argtypes = []
    lib.nerf_ctx_create.restype = i32
    lib.nerf_ctx_create.argtypes = [i32, C.POINTER(vp)]
    lib.nerf_ctx_destroy.restype = None
    lib.nerf_ctx_destroy.argtypes = [vp]
    lib.nerf_load_weights.restype = i32
    lib.nerf_load_weights.argtypes = [vp, i32, C.POINTER(NerfArch), C.POINTER(vp), i32]
    lib.nerf_num_weight_tensors.restype = i32
    lib.nerf_num_weight_tensors.argtypes = [C.POINTER(NerfArch)]
    lib.nerf_embed.restype = i32
    lib.nerf_embed.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.nerf_mlp_forward.restype = i32
    lib.nerf_mlp_forward.argtypes = [vp, i32, vp, i64, vp, vp]
    lib.nerf_run_network.restype = i32
    lib.nerf_run_network.argtypes = [vp, i32, vp, vp, i64, i64, vp, vp]
    lib.nerf_raw2outputs.restype = i32
    lib.nerf_raw2outputs.argtypes = [vp, vp, i32, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp]
    lib.nerf_sample_pdf.restype = i32
    lib.nerf_sample_pdf.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp]
    lib.nerf_render_rays.restype = i32
    lib.nerf_render_rays.argtypes = [vp, C.POINTER(RenderArgs)]
    lib.nerf_profile_enable.restype = i32
    lib.nerf_profile_enable.argtypes = [vp, i32]
    lib.nerf_profile_read.restype = i32
    lib.nerf_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64), i32]
    lib.nerf_profile_read_train.restype = i32
    lib.nerf_profile_read_train.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64), i32]
    lib.nerf_generate_rays.restype = i32
    lib.nerf_generate_rays.argtypes = [vp, C.POINTER(Camera), i64, i64, vp, vp]
    lib.nerf_image_metrics.restype = i32
    lib.nerf_image_metrics.argtypes = [vp, vp, vp, i32, i32, C.c_float, vp, vp]
    lib.nerf_train_step.restype = i32
    lib.nerf_train_step.argtypes = [vp, C.POINTER(TrainArgs)]
    lib.nerf_train_forward.restype = i32
    lib.nerf_train_forward.argtypes = [vp, C.POINTER(TrainForwardArgs)]
    lib.nerf_train_backward.restype = i32
    lib.nerf_train_backward.argtypes = [vp, C.POINTER(TrainBackwardArgs)]
    lib.nerf_zero_grad.restype = i32
    lib.nerf_zero_grad.argtypes = [vp, i32, vp]
    lib.nerf_adam_step.restype = i32
    lib.nerf_adam_step.argtypes = [vp, C.POINTER(C.c_int32), i32, C.c_float, C.c_float, C.c_float, C.c_float, i32, vp]
    lib.nerf_get_weights.restype = i32
    lib.nerf_get_weights.argtypes = [vp, i32, C.POINTER(vp), i32]
    lib.nerf_get_gradients.restype = i32
    lib.nerf_get_gradients.argtypes = [vp, i32, C.POINTER(vp), i32]
    lib.nerf_stratified_z.restype = i32
    lib.nerf_stratified_z.argtypes = [vp, vp, i32, i64, i32, i32, vp, vp, vp]
    lib.nerf_resample.restype = i32
    lib.nerf_resample.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp]
    lib.nerf_render_frame.restype = i32
    lib.nerf_render_frame.argtypes = [vp, C.POINTER(FrameArgs)]
    lib.nerf_shard_bounds.restype = i32
    lib.nerf_shard_bounds.argtypes = [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    lib.nerf_render_shard.restype = i32
    lib.nerf_render_shard.argtypes = [vp, C.POINTER(FrameArgs), i32, i32, C.POINTER(i64), C.POINTER(i64)]
    lib.nerf_workspace_bytes.restype = i64
    lib.nerf_workspace_bytes.argtypes = [vp]
    lib.nerf_set_precision.restype = i32
    lib.nerf_set_precision.argtypes = [vp, i32]
    lib.nerf_pack_rays.restype = i32
    lib.nerf_pack_rays.argtypes = [vp, C.POINTER(Camera), vp, i32, vp, i32, i64, vp, vp]
    lib.nerf_set_render_precision.restype = i32
    lib.nerf_set_render_precision.argtypes = [vp, i32]
    lib.nerf_set_view_fold.restype = i32
    lib.nerf_set_view_fold.argtypes = [vp, i32]
    lib.nerf_set_ray_view_bias.restype = i32
    lib.nerf_set_ray_view_bias.argtypes = [vp, i32]
    lib.nerf_set_tile_schedule.restype = i32
    lib.nerf_set_tile_schedule.argtypes = [vp, i32]
    lib.nerf_view_fold_status.restype = i32
    lib.nerf_view_fold_status.argtypes = [vp, i32, C.POINTER(i32)]
    lib.nerf_get_precision.restype = i32
    lib.nerf_get_precision.argtypes = [vp]
    lib.nerf_get_adam_state.restype = i32
    lib.nerf_get_adam_state.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), i32]
    lib.nerf_set_adam_state.restype = i32
    lib.nerf_set_adam_state.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), i32]
    lib.nerf_precision_status.restype = i32
    lib.nerf_precision_status.argtypes = [vp, C.POINTER(i64), i32]
    lib.nerf_precision_detail.restype = i32
    lib.nerf_precision_detail.argtypes = [vp, C.POINTER(i64), i32]
    lib.nerf_precision_peek.restype = i32
    lib.nerf_precision_peek.argtypes = [vp, C.POINTER(i64)]
    lib.nerf_precision_check.restype = i32
    lib.nerf_precision_check.argtypes = [vp, vp, C.POINTER(i64)]
    lib.nerf_density_grid.restype = i32
    lib.nerf_density_grid.argtypes = [vp, C.POINTER(GridArgs)]
    lib.nerf_marching_cubes.restype = i32
    lib.nerf_marching_cubes.argtypes = [vp, C.POINTER(McArgs)]
    lib.nerf_occupancy_create.restype = i32
    lib.nerf_occupancy_create.argtypes = [vp, C.POINTER(OccupancyArgs), C.POINTER(vp)]
    lib.nerf_occupancy_destroy.restype = None
    lib.nerf_occupancy_destroy.argtypes = [vp]
    lib.nerf_occupancy_cells.restype = i32
    lib.nerf_occupancy_cells.argtypes = [vp, vp, C.POINTER(i64), vp]
    lib.nerf_occupancy_stats.restype = i32
    lib.nerf_occupancy_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), i32]
    lib.nerf_train_step_occ.restype = i32
    lib.nerf_train_step_occ.argtypes = [vp, C.POINTER(TrainArgs), vp]
    lib.nerf_occupancy_refresh.restype = i32
    lib.nerf_occupancy_refresh.argtypes = [vp, C.POINTER(OccupancyArgs)]
    lib.nerf_render_rays_occ.restype = i32
    lib.nerf_render_rays_occ.argtypes = [vp, C.POINTER(RenderArgs), vp]
    lib.nerf_render_frame_occ.restype = i32
    lib.nerf_render_frame_occ.argtypes = [vp, C.POINTER(FrameArgs), vp]
    lib.nerf_grid_create.restype = i32
    lib.nerf_grid_create.argtypes = [vp, C.POINTER(SparseGridDesc), C.POINTER(vp)]
    lib.nerf_grid_destroy.restype = None
    lib.nerf_grid_destroy.argtypes = [vp]
    lib.nerf_grid_render_rays.restype = i32
    lib.nerf_grid_render_rays.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridRenderArgs)]
    lib.nerf_grid_render_image.restype = i32
    lib.nerf_grid_render_image.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(GridRenderOptions), C.POINTER(GridRenderArgs)]
    lib.nerf_grid_gen_rays.restype = i32
    lib.nerf_grid_gen_rays.argtypes = [vp, C.POINTER(GridCamera), vp, vp, vp]
    lib.nerf_grid_rays_to_ndc.restype = i32
    lib.nerf_grid_rays_to_ndc.argtypes = [vp, C.POINTER(GridRaysToNdcArgs)]
    lib.nerf_grid_sample.restype = i32
    lib.nerf_grid_sample.argtypes = [vp, C.POINTER(GridSampleArgs)]
    lib.nerf_grid_accelerate.restype = i32
    lib.nerf_grid_accelerate.argtypes = [vp, vp]
    lib.nerf_grid_drop_skip.restype = i32
    lib.nerf_grid_drop_skip.argtypes = [vp]
    lib.nerf_grid_has_skip.restype = i32
    lib.nerf_grid_has_skip.argtypes = [vp]
    lib.nerf_grid_project_sh.restype = i32
    lib.nerf_grid_project_sh.argtypes = [vp, C.POINTER(GridProjectArgs)]
    lib.nerf_grid_fused_backward.restype = i32
    lib.nerf_grid_fused_backward.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridFusedArgs)]
    lib.nerf_grid_tv_grad.restype = i32
    lib.nerf_grid_tv_grad.argtypes = [vp, C.POINTER(GridTvArgs)]
    lib.nerf_grid_optim_step.restype = i32
    lib.nerf_grid_optim_step.argtypes = [vp, C.POINTER(GridOptimArgs)]
    lib.nerf_grid_fused_backward_losses.restype = i32
    lib.nerf_grid_fused_backward_losses.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridFusedArgs)]
    lib.nerf_grid_render_backward_losses.restype = i32
    lib.nerf_grid_render_backward_losses.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridRenderBackwardArgs),
                                                     C.POINTER(GridRenderBackwardLossesArgs)]
    lib.nerf_grid_tv_grad_edge.restype = i32
    lib.nerf_grid_tv_grad_edge.argtypes = [vp, C.POINTER(GridTvArgs)]
    lib.nerf_grid_lattice_density.restype = i32
    lib.nerf_grid_lattice_density.argtypes = [vp, C.POINTER(GridLatticeArgs)]
    lib.nerf_grid_weight_render.restype = i32
    lib.nerf_grid_weight_render.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(GridWeightArgs)]
    lib.nerf_grid_threshold.restype = i32
    lib.nerf_grid_threshold.argtypes = [vp, vp, i64, C.c_float, vp, vp]
    lib.nerf_grid_dilate.restype = i32
    lib.nerf_grid_dilate.argtypes = [vp, C.POINTER(C.c_int32), vp, vp, vp]
    lib.nerf_grid_compact_workspace.restype = i64
    lib.nerf_grid_compact_workspace.argtypes = [i64]
    lib.nerf_grid_compact.restype = i32
    lib.nerf_grid_compact.argtypes = [vp, C.POINTER(GridCompactArgs)]
    lib.nerf_grid_gather.restype = i32
    lib.nerf_grid_gather.argtypes = [vp, C.POINTER(GridGatherArgs)]
    lib.nerf_grid_components_occupancy.restype = i32
    lib.nerf_grid_components_occupancy.argtypes = [vp, C.POINTER(GridOccupancyArgs)]
    lib.nerf_grid_components_workspace.restype = i64
    lib.nerf_grid_components_workspace.argtypes = [i64]
    lib.nerf_grid_components_label.restype = i32
    lib.nerf_grid_components_label.argtypes = [vp, C.POINTER(GridLabelArgs)]
    lib.nerf_grid_components_finish.restype = i32
    lib.nerf_grid_components_finish.argtypes = [vp, vp, C.POINTER(i64), vp]
    lib.nerf_grid_components_volumes.restype = i32
    lib.nerf_grid_components_volumes.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.nerf_grid_components_keep.restype = i32
    lib.nerf_grid_components_keep.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp]
    lib.nerf_grid_copy_rows.restype = i32
    lib.nerf_grid_copy_rows.argtypes = [vp, C.POINTER(GridCopyRowsArgs)]
    lib.nerf_grid_depth_rays.restype = i32
    lib.nerf_grid_depth_rays.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridDepthArgs)]
    lib.nerf_grid_depth_image.restype = i32
    lib.nerf_grid_depth_image.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(GridRenderOptions), C.POINTER(GridDepthArgs)]
    lib.nerf_grid_render_rays_taped.restype = i32
    lib.nerf_grid_render_rays_taped.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridRenderTapedArgs)]
    lib.nerf_grid_render_backward.restype = i32
    lib.nerf_grid_render_backward.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridRenderBackwardArgs)]
    lib.nerf_grid_sample_backward.restype = i32
    lib.nerf_grid_sample_backward.argtypes = [vp, C.POINTER(GridSampleBackwardArgs)]
    lib.nerf_grid_depth_rays_taped.restype = i32
    lib.nerf_grid_depth_rays_taped.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridDepthTapedArgs)]
    lib.nerf_grid_depth_backward.restype = i32
    lib.nerf_grid_depth_backward.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridDepthBackwardArgs)]
    lib.nerf_grid_floater_heatmap.restype = i32
    lib.nerf_grid_floater_heatmap.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(GridFloaterHeatmapArgs)]
    lib.nerf_grid_component_view.restype = i32
    lib.nerf_grid_component_view.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(GridComponentViewArgs)]
    lib.nerf_grid_half_row_halfs.restype = i32
    lib.nerf_grid_half_row_halfs.argtypes = [C.c_int32]
    lib.nerf_grid_pack_half.restype = i32
    lib.nerf_grid_pack_half.argtypes = [vp, C.POINTER(GridPackHalfArgs)]
    lib.nerf_grid_unpack_half.restype = i32
    lib.nerf_grid_unpack_half.argtypes = [vp, vp, i64, C.c_int32, vp, vp]
    lib.nerf_grid_create_half.restype = i32
    lib.nerf_grid_create_half.argtypes = [vp, C.POINTER(GridHalfDesc), C.POINTER(vp)]
    lib.nerf_grid_median_cut_workspace.restype = i64
    lib.nerf_grid_median_cut_workspace.argtypes = [i64, C.c_int32]
    lib.nerf_grid_quantize_median_cut.restype = i32
    lib.nerf_grid_quantize_median_cut.argtypes = [vp, C.POINTER(GridMedianCutArgs)]
    lib.nerf_grid_create_palette.restype = i32
    lib.nerf_grid_create_palette.argtypes = [vp, C.POINTER(GridPaletteDesc), C.POINTER(vp)]
    lib.nerf_grid_set_background.restype = i32
    lib.nerf_grid_set_background.argtypes = [vp, C.POINTER(GridBackgroundDesc)]
    lib.nerf_grid_has_background.restype = i32
    lib.nerf_grid_has_background.argtypes = [vp]
    lib.nerf_grid_background_rays.restype = i32
    lib.nerf_grid_background_rays.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridBackgroundArgs)]
    lib.nerf_grid_background_image.restype = i32
    lib.nerf_grid_background_image.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(GridRenderOptions),
                                               C.POINTER(GridBackgroundArgs)]
    lib.nerf_grid_background_sparsify_plan.restype = i32
    lib.nerf_grid_background_sparsify_plan.argtypes = [vp, C.POINTER(GridBackgroundSparsifyArgs)]
    lib.nerf_grid_background_gather.restype = i32
    lib.nerf_grid_background_gather.argtypes = [vp, C.POINTER(GridBackgroundGatherArgs)]
    lib.nerf_grid_background_rays_taped.restype = i32
    lib.nerf_grid_background_rays_taped.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridBackgroundTapedArgs)]
    lib.nerf_grid_background_backward.restype = i32
    lib.nerf_grid_background_backward.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridBackgroundBackwardArgs)]
    lib.nerf_grid_background_tv_grad.restype = i32
    lib.nerf_grid_background_tv_grad.argtypes = [vp, C.POINTER(GridBackgroundTvArgs)]
    lib.nerf_grid_background_optim_step.restype = i32
    lib.nerf_grid_background_optim_step.argtypes = [vp, C.POINTER(GridBackgroundOptimArgs)]
    lib.nerf_grid_tv_value_workspace.restype = i64
    lib.nerf_grid_tv_value_workspace.argtypes = [i64]
    lib.nerf_grid_tv_value.restype = i32
    lib.nerf_grid_tv_value.argtypes = [vp, C.POINTER(GridTvValueArgs)]
    lib.nerf_grid_tv_value_backward.restype = i32
    lib.nerf_grid_tv_value_backward.argtypes = [vp, C.POINTER(GridTvValueArgs)]
    lib.nerf_grid_sparsity_rays.restype = i32
    lib.nerf_grid_sparsity_rays.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridSparsityArgs)]
    lib.nerf_grid_sparsity_backward.restype = i32
    lib.nerf_grid_sparsity_backward.argtypes = [vp, C.POINTER(GridRenderOptions), C.POINTER(GridSparsityArgs)]
    lib.nerf_grid_dataset_batch.restype = i32
    lib.nerf_grid_dataset_batch.argtypes = [vp, C.POINTER(GridDatasetBatchArgs)]
    lib.nerf_grid_marching_cubes.restype = i32
    lib.nerf_grid_marching_cubes.argtypes = [vp, C.POINTER(GridMcArgs)]
    lib.nerf_grid_mesh_attributes.restype = i32
    lib.nerf_grid_mesh_attributes.argtypes = [vp, C.POINTER(GridMeshAttributesArgs)]
    lib.nerf_octree_create.restype = i32
    lib.nerf_octree_create.argtypes = [vp, C.POINTER(OctreeDesc), C.POINTER(vp)]
    lib.nerf_octree_destroy.restype = None
    lib.nerf_octree_destroy.argtypes = [vp]
    lib.nerf_octree_render_rays.restype = i32
    lib.nerf_octree_render_rays.argtypes = [vp, C.POINTER(OctreeRenderOptions), C.POINTER(OctreeRenderArgs)]
    lib.nerf_octree_render_image.restype = i32
    lib.nerf_octree_render_image.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(OctreeRenderOptions), C.POINTER(OctreeRenderArgs)]
    lib.nerf_octree_backward_rays.restype = i32
    lib.nerf_octree_backward_rays.argtypes = [vp, C.POINTER(OctreeRenderOptions), C.POINTER(OctreeBackwardArgs)]
    lib.nerf_octree_backward_image.restype = i32
    lib.nerf_octree_backward_image.argtypes = [vp, C.POINTER(GridCamera), C.POINTER(OctreeRenderOptions), C.POINTER(OctreeBackwardArgs)]
    lib.nerf_octree_accelerate.restype = i32
    lib.nerf_octree_accelerate.argtypes = [vp, C.c_int32, vp]
    lib.nerf_octree_table_levels.restype = i32
    lib.nerf_octree_table_levels.argtypes = [vp]
    lib.nerf_octree_build_workspace.restype = i64
    lib.nerf_octree_build_workspace.argtypes = [C.c_int32]
    lib.nerf_octree_build_from_grid.restype = i32
    lib.nerf_octree_build_from_grid.argtypes = [vp, C.POINTER(OctreeBuildArgs)]
    _lib = lib
    return lib


def check(rc):
    """Preserve the reference's exception convention: errors (negative codes) are Python exceptions. Positive codes are
    the library's warnings (NERF_W_*: the work was done); they become RuntimeWarnings and are returned."""
    if rc < 0:
        msg = load().nerf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"nerf_mi355x error {rc}: {msg}")
    if rc > 0:
        import warnings
        warnings.warn(load().nerf_last_error().decode("utf-8", "replace"), RuntimeWarning, stacklevel=3)
    return rc
