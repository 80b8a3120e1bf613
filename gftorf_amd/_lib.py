"""ctypes binding of libgftorf_rast.so (include/gftorf_rast.h).

The product path has no CPU fallback: if the HIP library is missing this module
raises, it never routes anywhere else.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgftorf_rast.so")
ABI_VERSION = 16
DEFORM_MAX_INPUTS = 96          # GFT_DEFORM_MAX_INPUTS (include/gftorf_deform.h)
ACC_STRIDE = 16

_lib = None

_fp = C.c_void_p  # every tensor pointer travels as void*


class Config(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("D", C.c_int32), ("M", C.c_int32), ("M_p", C.c_int32),
        ("W", C.c_int32), ("H", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("near_n", C.c_float), ("far_n", C.c_float), ("depth_range", C.c_float),
        ("phase_offset", C.c_float), ("dc_offset", C.c_float),
        ("use_view_dependent_phase", C.c_int32), ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("want_backward", C.c_int32),
        ("acc_zeroed", C.c_int32),
        ("grads_zeroed", C.c_int32),
        ("grads_accumulate", C.c_int32),
        ("bg_stride_c", C.c_int64), ("bg_stride_y", C.c_int64), ("bg_stride_x", C.c_int64),
    ]


FORWARD_FIELDS = [
    "bg", "means3D", "colors_precomp", "phasors_precomp", "opacities", "scales", "rotations",
    "cov3D_precomp", "viewmatrix", "projmatrix", "campos", "shs", "shs_p",
    "geom", "img", "binning",
    "out_color", "out_phasor", "out_depth", "out_normal", "out_acc", "out_entropy",
    "out_depth_distortion", "out_amp_distortion", "pixels", "out_distribution", "radii", "acc",
]

BACKWARD_FIELDS = [
    "bg", "means3D", "radii", "scales", "rotations", "cov3D_precomp", "viewmatrix", "projmatrix",
    "campos", "shs", "shs_p", "opacities", "pixels",
    "dL_dout_color", "dL_dout_phasor", "dL_dout_depth", "dL_dout_acc", "dL_dout_depth_distortion",
    "geom", "img", "binning", "acc",
    "dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dcov3D", "dL_dsh", "dL_dsh_p",
    "dL_dscales", "dL_drotations", "dL_dphase_offset", "dL_ddc_offset", "det_partials", "dirty_rows", "rows_report",
    "phase_offset_dev", "dc_offset_dev",
]

LAYOUT_FIELDS = [
    "geom_rec_a", "geom_rec_b", "geom_depth", "geom_tiles", "geom_rect", "geom_dirgrad", "geom_clamped", "geom_need",
    "geom_blockhist", "geom_total",
    "img_pix_state", "img_ranges", "img_tile_max", "img_ctrl", "img_tile_cnt", "img_tile_cut", "img_super_tab", "img_tile_cursor",
    "img_tile_order", "img_front_len", "img_unit_flag", "img_resume_state", "img_pix_sums", "img_snaps", "img_total",
    "bin_keys", "bin_point_list", "bin_total",
]

PROFILE_FIELDS = ["preprocess_fwd_ms", "tile_count_ms", "tile_scatter_ms", "tile_sort_ms",
                  "render_fwd_ms", "render_bwd_ms", "preprocess_bwd_ms", "memset_ms"]


class ForwardIO(C.Structure):
    _fields_ = [(n, _fp) for n in FORWARD_FIELDS] + [("grads_zero", _fp), ("grads_zero_bytes", C.c_size_t), ("tile_hints", _fp), ("tile_weights", _fp),
                                                           ("cell_sched", _fp), ("phase_offset_dev", _fp), ("dc_offset_dev", _fp)]


class BackwardIO(C.Structure):
    _fields_ = [(n, _fp) for n in BACKWARD_FIELDS]


class Layout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in LAYOUT_FIELDS]


class ForwardHints(C.Structure):
    """gft_forward_hints"""
    _fields_ = [("binning_instances", C.c_int64), ("max_tile_list", C.c_int64), ("whole_lists", C.c_int64),
                ("use_cell_sched", C.c_int64)]


class ForwardReport(C.Structure):
    """gft_forward_report"""
    _fields_ = [("num_rendered", C.c_int64), ("max_tile_list", C.c_int64), ("list_entries", C.c_int64), ("hinted_tiles", C.c_int64),
                ("sched_misses", C.c_int64)]


class Profile(C.Structure):
    _fields_ = [(n, C.c_double) for n in PROFILE_FIELDS] + [("forward_calls", C.c_int64),
                                                           ("backward_calls", C.c_int64)]


# ---- fused input assembly (include/gftorf_assemble.h) -------------------------------------------
ASSEMBLE_PTRS_IN = ["xyz", "screenspace", "opacity", "scaling", "rotation", "rotation_raw", "feat_color",
                    "feat_phasor", "motion_mask", "d_xyz", "d_rot", "d_sh", "d_sh_p"]
ASSEMBLE_SCALARS = ["d_xyz_scalar", "d_rot_scalar", "d_sh_scalar", "d_sh_p_scalar"]
ASSEMBLE_PTRS_OUT = ["scratch", "out_means3D", "out_means2D", "out_opacity", "out_scales", "out_rotations",
                     "out_shs", "out_shs_p"]
ASSEMBLE_RAW_FLAGS = ["opacity_is_raw", "scaling_is_raw"]          # (round 6: the model's own tensors as sources)
ASSEMBLE_PARTS = ["feat_dc_color", "feat_rest_color", "phase_dc", "phase_rest", "amp_dc", "amp_rest"]
ASSEMBLE_FIELDS = ASSEMBLE_PTRS_IN + ASSEMBLE_SCALARS + ASSEMBLE_PTRS_OUT + ["num_offset_rows"] + ASSEMBLE_RAW_FLAGS + ASSEMBLE_PARTS
ASSEMBLE_BWD_HEAD = ["scratch", "rotation_raw", "d_rot"]
ASSEMBLE_BWD_TAIL = ["g_means3D", "g_means2D", "g_opacity", "g_scales", "g_rotations", "g_shs", "g_shs_p",
                     "g_xyz", "g_screenspace", "g_opacity_in", "g_scaling", "g_rotation", "g_rotation_raw",
                     "g_feat_color", "g_feat_phasor", "g_d_xyz", "g_d_rot", "g_d_sh", "g_d_sh_p"]
ASSEMBLE_BWD_RAW = ["opacity_raw", "scaling_raw", "g_feat_dc_color", "g_feat_rest_color", "g_phase_dc", "g_phase_rest", "g_amp_dc", "g_amp_rest"]
ASSEMBLE_BWD_FIELDS = ASSEMBLE_BWD_HEAD + ["d_rot_scalar"] + ASSEMBLE_BWD_TAIL + ["static_from_raw"] + ASSEMBLE_BWD_RAW


class AssembleIO(C.Structure):
    _fields_ = ([(n, _fp) for n in ASSEMBLE_PTRS_IN] + [(n, C.c_float) for n in ASSEMBLE_SCALARS] +
                [(n, _fp) for n in ASSEMBLE_PTRS_OUT] + [("num_offset_rows", C.c_int64)] +
                [(n, C.c_int32) for n in ASSEMBLE_RAW_FLAGS] + [(n, _fp) for n in ASSEMBLE_PARTS])


class AssembleBwdIO(C.Structure):
    _fields_ = ([(n, _fp) for n in ASSEMBLE_BWD_HEAD] + [("d_rot_scalar", C.c_float)] +
                [(n, _fp) for n in ASSEMBLE_BWD_TAIL] + [("static_from_raw", C.c_int32)] + [(n, _fp) for n in ASSEMBLE_BWD_RAW])


class DeformParams(C.Structure):
    """gft_deform_params / gft_deform_grads (include/gftorf_deform.h): same field order."""
    _fields_ = [("linear_w", _fp * 8), ("linear_b", _fp * 8), ("xyz_w", _fp), ("xyz_b", _fp), ("r_w", _fp), ("r_b", _fp),
                ("g_w", _fp), ("g_b", _fp), ("b_w", _fp), ("b_b", _fp)]


DEFORM_FIELDS = [f[0] for f in DeformParams._fields_]


class AdamTensor(C.Structure):
    """gft_adam_tensor (include/gftorf_optim.h)"""
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("n", C.c_int64), ("lr", C.c_double),
                ("step", C.c_int64)]

EXPORTS = [
    "gft_abi_version", "gft_lazy_sort", "gft_last_error", "gft_geom_bytes", "gft_image_bytes", "gft_cell_sched_words", "gft_binning_bytes", "gft_acc_bytes",
    "gft_det_partials_bytes", "gft_get_layout", "gft_binning_capacity", "gft_set_binning_mode", "gft_binning_mode", "gft_set_render_mode", "gft_forward_preprocess", "gft_forward_render", "gft_forward", "gft_forward_enqueue", "gft_backward", "gft_grads_rezero",
    "gft_mark_visible", "gft_profile_enable", "gft_profile_reset", "gft_profile_read",
    "gft_assemble_scratch_bytes", "gft_assemble_forward", "gft_assemble_num_dynamic", "gft_assemble_backward",
    "gft_knn_scratch_bytes", "gft_knn_mean_dist2", "gft_adam_step",
    "gft_deform_inputs", "gft_deform_packed_bytes", "gft_deform_saved_bytes", "gft_deform_scratch_bytes", "gft_deform_pack",
    "gft_deform_forward", "gft_deform_backward", "gft_deform_compact", "gft_deform_rows_work_bytes", "gft_deform_backward_rows",
    "gft_deform_dw_splits", "gft_deform_rows_splits_capacity",
    "gft_ssim_blocks", "gft_ssim_l2_forward", "gft_ssim_l2_backward",
    "gft_image_loss_forward", "gft_image_loss_backward", "gft_pixel_loss_blocks", "gft_pixel_loss_forward", "gft_pixel_loss_backward",
    "gft_grad_norm_scratch_bytes", "gft_grad_norm", "gft_grad_scale",
    "gft_densify_stats", "gft_rows_rank_scratch_bytes", "gft_rows_rank", "gft_rows_rank_dev", "gft_rows_gather", "gft_rows_any_nonzero",
    "gft_densify_plan_scratch_bytes", "gft_densify_classify", "gft_densify_layout", "gft_rows_remap",
    "gft_split_children",
]
# include/gftorf_flow.h (the scene-flow term; no struct, so the ABI version is unchanged)
FLOW_EXPORTS = ["gft_flow_loss_blocks", "gft_flow_loss_forward", "gft_flow_loss_backward", "gft_flow_points", "gft_flow_project",
                "gft_flow_project_backward"]
# include/gftorf_features.h (the feature blend over a drawn frame; no struct, so the ABI version is unchanged)
FEATURE_EXPORTS = ["gft_render_features", "gft_render_features_backward", "gft_feature_partials_bytes",
                   "gft_render_features_backward_det"]
# include/gftorf_detsum.h (the fixed-order sum of the reproducible backwards; no struct, so the ABI version is unchanged)
DETSUM_EXPORTS = ["gft_detsum_index_bytes", "gft_backward_det"]
# include/gftorf_reg.h (the per-Gaussian regularisers of the loss; no struct, so the ABI version is unchanged)
REG_EXPORTS = ["gft_reg_blocks", "gft_reg_result_words", "gft_reg_forward", "gft_reg_backward"]
REG_PARTIAL_WORDS = 8           # GFT_REG_PARTIAL_WORDS
REG_MEANS, REG_COUNTS, REG_RECIPS, REG_TOTAL = 0, 4, 6, 10      # GFT_REG_*: words of the result block
# include/gftorf_rigid.h (exact K-NN, the rigidity and isometry priors; no struct, so the ABI version is unchanged)
RIGID_EXPORTS = ["gft_rigid_knn_scratch_bytes", "gft_rigid_knn", "gft_rigid_blocks", "gft_rigid_result_words", "gft_rigid_forward",
                 "gft_rigid_backward"]
RIGID_MAX_K, RIGID_PARTIAL_WORDS, RIGID_MEANS, RIGID_TOTAL = 32, 2, 0, 2           # GFT_RIGID_*
# include/gftorf_tof.h (the ToF depth and the training log's scalars; no struct, so the ABI version is unchanged)
TOF_EXPORTS = ["gft_tof_depth", "gft_tof_log_blocks", "gft_tof_log_row"]
TOF_PARTIAL_WORDS = 12          # GFT_TOF_PARTIAL_WORDS
TOF_LOG_WORDS, TOF_LOG_MAX_EXTRAS = 24, 8                       # GFT_TOF_LOG_WORDS, GFT_TOF_LOG_MAX_EXTRAS
# GFT_TOF_LOG_*: the float words of a row in order, then the uint32 words and the extras
TOF_LOG_FLOATS = ("sp", "sp_tof", "gsp", "sp_err", "sp_tof_err", "depth_err", "tof_depth_err", "amp_err", "dd", "gs_sp",
                  "gs_sp_visible")
TOF_LOG_VISIBLE, TOF_LOG_PRESENT, TOF_LOG_NUM_EXTRAS, TOF_LOG_SEQ, TOF_LOG_EXTRAS = 11, 12, 13, 14, 16
TOF_HAS_GT_DEPTH, TOF_HAS_DD, TOF_HAS_AMP, TOF_HAS_VISIBLE = 1, 2, 4, 8
# include/gftorf_query.h (an iteration's deformation queries as one batch; no struct, so the ABI version is unchanged)
QUERY_EXPORTS = ["gft_query_inputs", "gft_query_combine", "gft_query_combine_backward"]
QUERY_MAX_TIMES, QUERY_MAX_OUTPUTS = 4, 4                       # GFT_QUERY_MAX_TIMES, GFT_QUERY_MAX_OUTPUTS
# include/gftorf_metrics.h (a view's evaluation metrics; no struct, so the ABI version is unchanged)
METRICS_EXPORTS = ["gft_metrics_blocks", "gft_view_metrics", "gft_metrics_reset"]
# GFT_METRICS_*: the eight values in the order of a row's first floats and of the accumulator's doubles
METRICS_VALUES = ("l1", "psnr", "l1_p", "l2_p", "psnr_p", "l1_d", "l2_d", "l2_d_tof")
METRICS_MAX_PLANES, METRICS_PARTIAL_WORDS = 8, 36               # GFT_METRICS_MAX_PLANES, GFT_METRICS_PARTIAL_WORDS
METRICS_ROW_MSE, METRICS_ROW_PSNR, METRICS_ROW_PRESENT, METRICS_ROW_PLANES, METRICS_ROW_WORDS = 8, 16, 24, 25, 28
METRICS_ACC_SUMS, METRICS_ACC_VIEWS, METRICS_ACC_PRESENT, METRICS_ACC_WORDS = 0, 16, 17, 18
METRICS_HAS_COLOUR, METRICS_HAS_TOF, METRICS_HAS_DEPTH, METRICS_HAS_TOF_DEPTH = 1, 2, 4, 8
# include/gftorf_present.h (a rendered view's display images; no struct, so the ABI version is unchanged)
PRESENT_EXPORTS = ["gft_present_blocks", "gft_present_sheet_bytes", "gft_present_magma", "gft_present_view", "gft_present_ranges",
                   "gft_present_ranges_reset", "gft_present_seismic", "gft_present_quad"]
# GFT_PRESENT_*: the images of a sheet in the order they lie in it: (name, bytes per pixel, numpy dtype, shape of an H x W view)
PRESENT_IMAGES = (("color", 3, "uint8", lambda H, W: (H, W, 3)), ("real", 3, "uint8", lambda H, W: (H, W, 3)),
                  ("imag", 3, "uint8", lambda H, W: (H, W, 3)), ("amp", 1, "uint8", lambda H, W: (H, W)),
                  ("quad", 4, "uint8", lambda H, W: (4, H, W)), ("depth", 4, "uint8", lambda H, W: (H, W, 4)),
                  ("depth_tof", 4, "uint8", lambda H, W: (H, W, 4)), ("depth_norm", 4, "uint8", lambda H, W: (H, W, 4)),
                  ("dd", 1, "uint8", lambda H, W: (H, W)), ("depth_tof_f", 4, "float32", lambda H, W: (H, W)),
                  ("depth_norm_f", 4, "float32", lambda H, W: (H, W)))
PRESENT_HAS_COLOR, PRESENT_HAS_PHASOR, PRESENT_HAS_QUAD, PRESENT_HAS_DEPTH, PRESENT_HAS_ACC, PRESENT_HAS_DD = 1, 2, 4, 8, 16, 32
PRESENT_ALIGN, PRESENT_PARTIAL_WORDS, PRESENT_RANGE_WORDS, PRESENT_MAGMA_ROWS = 16, 2, 6, 257      # GFT_PRESENT_*
PRESENT_SEISMIC_ROWS = 257                                                                         # GFT_PRESENT_SEISMIC_ROWS
# include/gftorf_flowviz.h (the optical-flow debug images; no struct, so the ABI version is unchanged)
FLOWVIZ_EXPORTS = ["gft_flowviz_blocks", "gft_flowviz_wheel", "gft_flowviz_images"]
FLOWVIZ_WHEEL_ROWS, FLOWVIZ_IMAGES, FLOWVIZ_RUN = 55, 3, 4      # GFT_FLOWVIZ_WHEEL_ROWS, GFT_FLOWVIZ_IMAGES, GFT_FLOWVIZ_RUN
# include/gftorf_debugviz.h (the training loop's debug images; no struct, so the ABI version is unchanged)
DEBUGVIZ_EXPORTS = ["gft_debugviz_blocks", "gft_debugviz_sheet_bytes", "gft_debugviz_images"]
# GFT_DEBUGVIZ_*: the images of a debug sheet in the order they lie in it: (name, bytes per pixel, shape of an H x W view)
DEBUGVIZ_IMAGES = (("depth", 4, lambda H, W: (H, W, 4)), ("amp", 1, lambda H, W: (H, W)), ("amp_error", 1, lambda H, W: (H, W)),
                   ("scattering_phase", 1, lambda H, W: (H, W)), ("scattering_phase_error", 1, lambda H, W: (H, W)),
                   ("scattering_phase_tof_depth", 1, lambda H, W: (H, W)), ("scattering_phase_tof_depth_error", 1, lambda H, W: (H, W)),
                   ("scattering_phase_gt", 1, lambda H, W: (H, W)), ("depth_error", 1, lambda H, W: (H, W)),
                   ("phase_depth", 4, lambda H, W: (H, W, 4)), ("phase_depth_gt", 4, lambda H, W: (H, W, 4)),
                   ("phase_depth_error", 1, lambda H, W: (H, W)), ("color", 3, lambda H, W: (H, W, 3)),
                   ("color_gt", 3, lambda H, W: (H, W, 3)), ("color_error", 3, lambda H, W: (H, W, 3)), ("dd", 1, lambda H, W: (H, W)),
                   ("quad", 4, lambda H, W: (4, H, W)), ("quad_gt", 4, lambda H, W: (4, H, W)), ("quad_error", 4, lambda H, W: (4, H, W)))
(DEBUGVIZ_HAS_PHASOR, DEBUGVIZ_HAS_GT_PHASOR, DEBUGVIZ_HAS_DEPTH, DEBUGVIZ_HAS_PHASE_DEPTH, DEBUGVIZ_HAS_GT_PHASE_DEPTH, DEBUGVIZ_HAS_DD,
 DEBUGVIZ_HAS_COLOR, DEBUGVIZ_HAS_QUAD, DEBUGVIZ_HAS_GT_QUAD) = 1, 2, 4, 8, 16, 32, 64, 128, 256
DEBUGVIZ_ALIGN, DEBUGVIZ_PARTIAL_WORDS, DEBUGVIZ_RANGE_WORDS, DEBUGVIZ_RUN = 16, 16, 8, 4               # GFT_DEBUGVIZ_*
# include/gftorf_tracks.h (the F-ToRF motion tracks; no struct, so the ABI version is unchanged)
TRACKS_EXPORTS = ["gft_tracks_integrate", "gft_tracks_table_bytes", "gft_tracks_table"]
TRACKS_PARTS = ("index", "xy", "motion", "step_ok")             # GFT_TRACKS_*: the parts of a table in the order they lie in it
# include/gftorf_ply.h (the rows of the model's PLY files; no struct, so the ABI version is unchanged)
PLY_EXPORTS = ["gft_ply_pack", "gft_ply_unpack"]
PLY_ROWS, PLY_MAX_SOURCES, PLY_MAX_COLUMNS = 64, 16, 240        # GFT_PLY_ROWS, GFT_PLY_MAX_SOURCES, GFT_PLY_MAX_COLUMNS
# include/gftorf_pcd.h (the input point cloud; no struct, so the ABI version is unchanged)
PCD_EXPORTS = ["gft_pcd_unproject", "gft_pcd_row_bytes", "gft_pcd_pack", "gft_pcd_unpack", "gft_pcd_create"]
PCD_ROWS, PCD_MAX_ROW_BYTES, PCD_STATUS_WORDS = 256, 128, 2     # GFT_PCD_ROWS, GFT_PCD_MAX_ROW_BYTES, GFT_PCD_STATUS_WORDS
PCD_MODES = ("torf_init", "ftorf_init", "proxy")                # GFT_PCD_TORF_INIT, GFT_PCD_FTORF_INIT, GFT_PCD_PROXY
# GFT_PCD_FIELDS: the entries of gft_pcd_unpack's offset table in order
PCD_FIELDS = ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "phase", "amplitude", "seg_red", "seg_green", "seg_blue")
# include/gftorf_png.h (PNG files formed on the device; its one struct is new, so the ABI version is unchanged)
PNG_EXPORTS = ["gft_png_bound", "gft_png_scratch_bytes", "gft_png_encode"]
PNG_SEGMENT, PNG_MAX_IMAGES, PNG_CHUNK_SLOT = 32768, 64, 32800  # GFT_PNG_SEGMENT, GFT_PNG_MAX_IMAGES, GFT_PNG_CHUNK_SLOT
# include/gftorf_views.h (the training views on the device; no struct, so the ABI version is unchanged)
VIEWS_EXPORTS = ["gft_views_layout", "gft_views_draw", "gft_views_select_plane", "gft_views_select_plane_backward"]
VIEWS_MAX_GROUPS, VIEWS_ALIGN, VIEWS_HEADER_BYTES, VIEWS_CHUNKS = 8, 16, 16, 1024      # GFT_VIEWS_*
VIEWS_INDEX_WORD, VIEWS_CURSOR_WORD = 0, 1                      # GFT_VIEWS_INDEX_WORD, GFT_VIEWS_CURSOR_WORD
VIEWS_KINDS = ("f32", "u8")                                     # GFT_VIEWS_F32, GFT_VIEWS_U8
# include/gftorf_schedule.h (the run's schedule on the device; its two structs are new, so the ABI version is unchanged)
SCHEDULE_EXPORTS = ["gft_schedule_tick"]
SCHEDULE_MAX_DESTS, SCHEDULE_STATE_WORDS = 1024, 8              # GFT_SCHEDULE_MAX_DESTS, GFT_SCHEDULE_STATE_WORDS
SCHEDULE_KINDS = ("f64", "f32")                                 # GFT_SCHEDULE_F64, GFT_SCHEDULE_F32
# GFT_SCHEDULE_*: the int64 words of the state block
SCHEDULE_COUNTER, SCHEDULE_ITERATION, SCHEDULE_TICKET, SCHEDULE_OVERRUN, SCHEDULE_OVERRUNS = 0, 1, 2, 3, 4


class PngImage(C.Structure):
    """gft_png_image (include/gftorf_png.h)"""
    _fields_ = [("src", _fp), ("row_stride", C.c_int64), ("out_offset", C.c_int64), ("H", C.c_int32), ("W", C.c_int32),
                ("channels", C.c_int32), ("reserved", C.c_int32)]


class ScheduleDest(C.Structure):
    """gft_schedule_dest (include/gftorf_schedule.h)"""
    _fields_ = [("address", _fp), ("column", C.c_int32), ("kind", C.c_int32)]


class Schedule(C.Structure):
    """gft_schedule"""
    _fields_ = [("state", _fp), ("table", _fp), ("N", C.c_int64), ("C", C.c_int32), ("D", C.c_int32), ("first_iter", C.c_int64),
                ("dests", _fp), ("bg", _fp), ("n", C.c_int64), ("T", C.c_int64)]


def load():
    """dlopen libgftorf_rast.so and declare prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "gftorf_amd: %s is missing. Build it with `python -m gftorf_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the rasterizer." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.gft_abi_version.restype = C.c_int
    if lib.gft_abi_version() != ABI_VERSION:
        raise RuntimeError("gftorf_amd: libgftorf_rast.so ABI %d != expected %d, rebuild"
                           % (lib.gft_abi_version(), ABI_VERSION))
    lib.gft_last_error.restype = C.c_char_p
    lib.gft_geom_bytes.restype = C.c_size_t
    lib.gft_geom_bytes.argtypes = [C.c_int32]
    lib.gft_image_bytes.restype = C.c_size_t
    lib.gft_image_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.gft_cell_sched_words.restype = C.c_size_t
    lib.gft_cell_sched_words.argtypes = [C.c_int32, C.c_int32]
    lib.gft_binning_bytes.restype = C.c_size_t
    lib.gft_binning_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.gft_acc_bytes.restype = C.c_size_t
    lib.gft_acc_bytes.argtypes = [C.c_int32]
    lib.gft_det_partials_bytes.restype = C.c_size_t
    lib.gft_det_partials_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.gft_binning_capacity.restype = C.c_int64
    lib.gft_binning_capacity.argtypes = [C.c_size_t, C.c_int32, C.c_int32]
    lib.gft_set_binning_mode.restype = C.c_int
    lib.gft_set_binning_mode.argtypes = [C.c_int]
    lib.gft_set_render_mode.restype = C.c_int
    lib.gft_set_render_mode.argtypes = [C.c_int]
    lib.gft_binning_mode.restype = C.c_int
    lib.gft_binning_mode.argtypes = [C.POINTER(Config)]
    lib.gft_get_layout.restype = C.c_int
    lib.gft_get_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(Layout)]
    lib.gft_forward_preprocess.restype = C.c_int
    lib.gft_forward_preprocess.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(ForwardIO),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.gft_forward_render.restype = C.c_int
    _ptrs = C.POINTER(C.c_void_p)
    lib.gft_adam_step.restype = C.c_int
    # stream, count, tensors, rows, row_mask, lr, step, factors, beta1, beta2, eps, weight_decay, grad_scale
    lib.gft_adam_step.argtypes = [C.c_void_p, C.c_int32, C.POINTER(AdamTensor), C.c_int64, C.c_void_p, _ptrs, _ptrs, C.c_void_p,
                                  C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.gft_grad_norm_scratch_bytes.restype = C.c_size_t
    lib.gft_grad_norm_scratch_bytes.argtypes = [C.c_int64, C.c_int32]
    lib.gft_grad_norm.restype = C.c_int
    lib.gft_grad_norm.argtypes = [C.c_void_p, C.c_int32, _ptrs, C.POINTER(C.c_int64), C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.gft_grad_scale.restype = C.c_int
    lib.gft_grad_scale.argtypes = [C.c_void_p, C.c_int32, _ptrs, C.POINTER(C.c_int64), C.c_void_p]
    lib.gft_deform_packed_bytes.restype = C.c_size_t
    lib.gft_deform_packed_bytes.argtypes = []
    lib.gft_deform_saved_bytes.restype = C.c_size_t
    lib.gft_deform_saved_bytes.argtypes = [C.c_int64]
    lib.gft_deform_scratch_bytes.restype = C.c_size_t
    lib.gft_deform_scratch_bytes.argtypes = [C.c_int64]
    lib.gft_deform_pack.restype = C.c_int
    lib.gft_deform_inputs.restype = C.c_int
    lib.gft_deform_inputs.argtypes = [C.c_int, C.c_int]
    lib.gft_deform_pack.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(DeformParams), C.c_void_p]
    lib.gft_deform_forward.restype = C.c_int
    lib.gft_deform_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    lib.gft_deform_backward.restype = C.c_int
    lib.gft_deform_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(DeformParams)]
    lib.gft_deform_compact.restype = C.c_int
    lib.gft_deform_compact.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 9
    lib.gft_deform_rows_work_bytes.restype = C.c_size_t
    lib.gft_deform_rows_work_bytes.argtypes = [C.c_int64]
    lib.gft_deform_dw_splits.restype = C.c_int
    lib.gft_deform_dw_splits.argtypes = [C.c_int64]
    lib.gft_deform_rows_splits_capacity.restype = C.c_int
    lib.gft_deform_rows_splits_capacity.argtypes = [C.c_int64]
    lib.gft_deform_backward_rows.restype = C.c_int
    lib.gft_deform_backward_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(DeformParams), C.c_void_p]
    lib.gft_ssim_blocks.restype = C.c_int64
    lib.gft_ssim_blocks.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.gft_ssim_l2_forward.restype = C.c_int
    lib.gft_ssim_l2_forward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                                        C.c_void_p, C.c_void_p]
    lib.gft_ssim_l2_backward.restype = C.c_int
    lib.gft_ssim_l2_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    _kind_sizes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    lib.gft_image_loss_forward.restype = C.c_int
    lib.gft_image_loss_forward.argtypes = _kind_sizes + [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    lib.gft_image_loss_backward.restype = C.c_int
    lib.gft_image_loss_backward.argtypes = _kind_sizes + [C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                                          C.c_float, C.c_void_p]
    lib.gft_pixel_loss_blocks.restype = C.c_int64
    lib.gft_pixel_loss_blocks.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.gft_pixel_loss_forward.restype = C.c_int
    lib.gft_pixel_loss_forward.argtypes = _kind_sizes + [C.c_float, C.c_void_p]
    lib.gft_pixel_loss_backward.restype = C.c_int
    lib.gft_pixel_loss_backward.argtypes = _kind_sizes + [C.c_void_p, C.c_float, C.c_void_p]
    _flow_cams = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5           # stream, H, W, depth, K, w2v, K_tof, w2v_tof
    lib.gft_flow_loss_blocks.restype = C.c_int64
    lib.gft_flow_loss_blocks.argtypes = [C.c_int32, C.c_int32]
    lib.gft_flow_loss_forward.restype = C.c_int
    lib.gft_flow_loss_forward.argtypes = _flow_cams + [C.c_void_p] * 4 + [C.c_float, C.c_void_p]
    lib.gft_flow_loss_backward.restype = C.c_int
    lib.gft_flow_loss_backward.argtypes = _flow_cams + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_void_p]
    lib.gft_flow_points.restype = C.c_int
    lib.gft_flow_points.argtypes = _flow_cams + [C.c_void_p, C.c_void_p]
    lib.gft_flow_project.restype = C.c_int
    lib.gft_flow_project.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    lib.gft_flow_project_backward.restype = C.c_int
    lib.gft_flow_project_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    _feat_frame = [C.c_void_p, C.POINTER(Config)] + [C.c_void_p] * 3 + [C.c_int64, C.c_int32]   # stream, cfg, scratch, R, C
    lib.gft_render_features.restype = C.c_int
    lib.gft_render_features.argtypes = _feat_frame + [C.c_void_p] * 3
    lib.gft_render_features_backward.restype = C.c_int
    lib.gft_render_features_backward.argtypes = _feat_frame + [C.c_void_p] * 3
    lib.gft_feature_partials_bytes.restype = C.c_size_t
    lib.gft_feature_partials_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.gft_render_features_backward_det.restype = C.c_int
    lib.gft_render_features_backward_det.argtypes = _feat_frame + [C.c_void_p] * 4     # dL_dout, index, partials, dL_dfeatures
    lib.gft_detsum_index_bytes.restype = C.c_size_t
    lib.gft_detsum_index_bytes.argtypes = [C.c_int32, C.c_int64]
    # stream, n_dxyz, P, pixels, d_xyz, opacity, motion_mask, opacity_is_raw, scaling, scaling_cols, scaling_is_raw, visible,
    # visible_is_radii
    _reg_inputs = ([C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                    C.c_int32, C.c_void_p, C.c_int32])
    _reg_weights = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.gft_reg_blocks.restype = C.c_int64
    lib.gft_reg_blocks.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    lib.gft_reg_result_words.restype = C.c_int64
    lib.gft_reg_result_words.argtypes = []
    lib.gft_reg_forward.restype = C.c_int
    lib.gft_reg_forward.argtypes = _reg_inputs + [C.c_void_p] + _reg_weights + [C.c_void_p, C.c_void_p]
    lib.gft_reg_backward.restype = C.c_int
    lib.gft_reg_backward.argtypes = _reg_inputs + _reg_weights + [C.c_void_p] * 6
    lib.gft_rigid_knn_scratch_bytes.restype = C.c_size_t
    lib.gft_rigid_knn_scratch_bytes.argtypes = [C.c_int32]
    # stream, P, K, points, idx, dist2, scratch
    lib.gft_rigid_knn.restype = C.c_int
    lib.gft_rigid_knn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gft_rigid_blocks.restype = C.c_int64
    lib.gft_rigid_blocks.argtypes = [C.c_int64, C.c_int32]
    lib.gft_rigid_result_words.restype = C.c_int64
    lib.gft_rigid_result_words.argtypes = []
    # stream, P, K, idx, w, prev, curr, d0, weights_dev, w_rigid, w_iso, partials, result
    lib.gft_rigid_forward.restype = C.c_int
    lib.gft_rigid_forward.argtypes = [C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 6 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    # stream, P, K, idx, offsets, edges, w, prev, curr, d0, weights_dev, w_rigid, w_iso, g_loss, g_curr, g_prev
    lib.gft_rigid_backward.restype = C.c_int
    lib.gft_rigid_backward.argtypes = [C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 8 + [C.c_float, C.c_float] + [C.c_void_p] * 3
    # stream, pixels, tof, plane_stride, depth_range_dev, depth_range, phase_offset_dev, phase_offset, out
    lib.gft_tof_depth.restype = C.c_int
    lib.gft_tof_depth.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p]
    lib.gft_tof_log_blocks.restype = C.c_int64
    lib.gft_tof_log_blocks.argtypes = [C.c_int64, C.c_int64]
    # stream, pixels, P, phasor, stride, depth, gt_phasor, stride, depth_range_dev, depth_range, phase_offset_dev, phase_offset,
    # tof_multiplier, gt_depth, depth_distortion, amp, amp_stride, visible, visible_is_radii, extras, num_extras, partials, rows,
    # slots, cursor
    lib.gft_tof_log_row.restype = C.c_int
    lib.gft_tof_log_row.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_int32, _ptrs, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    # stream, P, xyz, mask, rank, count_dev, n, K, scale, times_dev, times_host, x, t
    lib.gft_query_inputs.restype = C.c_int
    lib.gft_query_inputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                     C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    # stream, n, K, M, d / g_out, coeffs_dev, coeffs_host, out / g_d
    lib.gft_query_combine.restype = C.c_int
    lib.gft_query_combine.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), _ptrs]
    lib.gft_query_combine_backward.restype = C.c_int
    lib.gft_query_combine_backward.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _ptrs, C.c_void_p, C.POINTER(C.c_float),
                                               C.c_void_p]
    lib.gft_metrics_blocks.restype = C.c_int64
    lib.gft_metrics_blocks.argtypes = [C.c_int64]
    # stream, pixels_a, channels_a, image, stride, gt_image, stride, pixels_b, channels_b, tof, stride, gt_tof, stride, depth,
    # gt_depth, phasor, stride, depth_range_dev, depth_range, phase_offset_dev, phase_offset, partials, row, accum
    lib.gft_view_metrics.restype = C.c_int
    lib.gft_view_metrics.argtypes = ([C.c_void_p] + [C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] * 2 +
                                     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p])
    lib.gft_metrics_reset.restype = C.c_int
    lib.gft_metrics_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.gft_present_blocks.restype = C.c_int64
    lib.gft_present_blocks.argtypes = [C.c_int64]
    lib.gft_present_sheet_bytes.restype = C.c_int64
    lib.gft_present_sheet_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    lib.gft_present_magma.restype = C.POINTER(C.c_uint8)
    lib.gft_present_magma.argtypes = []
    # stream, H, W, image, stride, phasor, stride, planes, depth, acc, dd, ranges_dev, ranges_host, depth_range_dev, depth_range,
    # phase_offset_dev, phase_offset, znear, zfar, tof_multiplier, partials, sheet
    lib.gft_present_view.restype = C.c_int
    lib.gft_present_view.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_float, C.c_void_p, C.c_float,
                                     C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.gft_present_ranges.restype = C.c_int
    lib.gft_present_ranges.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.gft_present_ranges_reset.restype = C.c_int
    lib.gft_present_ranges_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.gft_present_seismic.restype = C.POINTER(C.c_uint8)
    lib.gft_present_seismic.argtypes = []
    # stream, H, W, phasor, stride, permutation, has_gt, tonemap, out
    lib.gft_present_quad.restype = C.c_int
    lib.gft_present_quad.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                     C.c_void_p]
    lib.gft_flowviz_blocks.restype = C.c_int64
    lib.gft_flowviz_blocks.argtypes = [C.c_int64]
    lib.gft_flowviz_wheel.restype = C.POINTER(C.c_uint8)
    lib.gft_flowviz_wheel.argtypes = []
    # stream, H, W, flow, stride, gt, stride, partials, out
    lib.gft_flowviz_images.restype = C.c_int
    lib.gft_flowviz_images.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.gft_debugviz_blocks.restype = C.c_int64
    lib.gft_debugviz_blocks.argtypes = [C.c_int64]
    lib.gft_debugviz_sheet_bytes.restype = C.c_int64
    lib.gft_debugviz_sheet_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    # stream, H, W, phasor, stride, planes, gt_phasor, stride, depth, phase_depth, gt_phase_depth, dd, image, stride, gt_image, stride,
    # gt_quad, stride, permutation, quad_index_dev, quad_index, ranges_dev, ranges_host, znear, zfar, tof_multiplier, partials, sheet
    lib.gft_debugviz_images.restype = C.c_int
    lib.gft_debugviz_images.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int32), C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float,
                                        C.c_float, C.c_void_p, C.c_void_p]
    # stream, P, n, T, U, initial_pos, flow, flow_index, K, world_view, mask, rank, H, W, xy, pos_last, motion, mean_z, step_ok
    lib.gft_tracks_integrate.restype = C.c_int
    lib.gft_tracks_integrate.argtypes = ([C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 7 +
                                         [C.c_int32, C.c_int32] + [C.c_void_p] * 5)
    lib.gft_tracks_table_bytes.restype = C.c_int64
    lib.gft_tracks_table_bytes.argtypes = [C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
    # stream, P, T, S, mask, rank, xy, step_ok, motion, table
    lib.gft_tracks_table.restype = C.c_int
    lib.gft_tracks_table.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 6
    _ints = C.POINTER(C.c_int32)
    # stream, P, count, sources, widths, channels, K_full, K_sibr, out_full, out_sibr
    lib.gft_ply_pack.restype = C.c_int
    lib.gft_ply_pack.argtypes = [C.c_void_p, C.c_int64, C.c_int32, _ptrs, _ints, _ints, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    # stream, rows, row0, K_file, chunk, count, dests, widths, table
    lib.gft_ply_unpack.restype = C.c_int
    lib.gft_ply_unpack.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, _ptrs, _ints, _ints]
    lib.gft_png_bound.restype = C.c_int64
    lib.gft_png_bound.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.gft_png_scratch_bytes.restype = C.c_int64
    lib.gft_png_scratch_bytes.argtypes = [C.c_int32, C.POINTER(PngImage)]
    # stream, count, images, level, out, out_bytes, sizes, scratch, scratch_bytes
    lib.gft_png_encode.restype = C.c_int
    lib.gft_png_encode.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PngImage), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_int64]
    # stream, mode, H, W, stride, tof, rendered, rendered_f64, view, width_m, height_m, znear, depth_range_dev, depth_range,
    # phase_offset_dev, phase_offset, xyz, dist, amp, sh_color, color, sh_amp, amplitude, status
    lib.gft_pcd_unproject.restype = C.c_int
    lib.gft_pcd_unproject.argtypes = ([C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_float, C.c_void_p,
                                       C.c_float] + [C.c_void_p] * 8)
    lib.gft_pcd_row_bytes.restype = C.c_int32
    lib.gft_pcd_row_bytes.argtypes = [C.c_int32, C.c_int32]
    # stream, P, xyz, colors, colors_f64, phases, amplitudes, seg, seg_f64, body, colors_back, seg_back, status
    lib.gft_pcd_pack.restype = C.c_int
    lib.gft_pcd_pack.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # stream, rows, row0, row_bytes, chunk, offsets, xyz, normals, colors, phases, amplitudes, seg
    lib.gft_pcd_unpack.restype = C.c_int
    lib.gft_pcd_unpack.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, _ints] + [C.c_void_p] * 6
    # stream, P, n, xyz, colors, colors_f64, phases, amplitudes, seg, seg_f64, log_scale, opacity, inv_c0, scaling_cols, then the
    # twelve outputs
    lib.gft_pcd_create.restype = C.c_int
    lib.gft_pcd_create.argtypes = ([C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_int32] + [C.c_void_p] * 12)
    _longs = C.POINTER(C.c_int64)
    # F, J, count, kinds, C, H, W, current_bytes, slab_offsets, current_offsets
    lib.gft_views_layout.restype = C.c_int64
    lib.gft_views_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, _ints, _ints, _ints, _ints, _longs, _longs, _longs]
    # stream, F, J, count, kinds, C, H, W, arena, current, V, index, order, cursor, N, ticket
    lib.gft_views_draw.restype = C.c_int
    lib.gft_views_draw.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _ints, _ints, _ints, _ints, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    # stream, C, plane, x / g_out, index, index_dev, modulo, table, T, out / g_x
    for fn in (lib.gft_views_select_plane, lib.gft_views_select_plane_backward):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    # stream, schedule
    lib.gft_schedule_tick.restype = C.c_int
    lib.gft_schedule_tick.argtypes = [C.c_void_p, C.POINTER(Schedule)]
    lib.gft_densify_stats.restype = C.c_int
    lib.gft_densify_stats.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    lib.gft_rows_rank_scratch_bytes.restype = C.c_size_t
    lib.gft_rows_rank_scratch_bytes.argtypes = [C.c_int64]
    lib.gft_rows_rank.restype = C.c_int
    lib.gft_rows_rank.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.gft_rows_rank_dev.restype = C.c_int
    lib.gft_rows_rank_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gft_rows_any_nonzero.restype = C.c_int
    lib.gft_rows_any_nonzero.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.gft_rows_gather.restype = C.c_int
    lib.gft_rows_gather.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.gft_densify_plan_scratch_bytes.restype = C.c_size_t
    lib.gft_densify_plan_scratch_bytes.argtypes = [C.c_int64]
    # stream, P, grad_norm, grad, max_scaling, max_grad, dense_threshold, row_class, clone_rows, split_rows, scratch, counts
    lib.gft_densify_classify.restype = C.c_int
    lib.gft_densify_classify.argtypes = ([C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_float, C.c_float] + [C.c_void_p] * 4 +
                                         [C.POINTER(C.c_int64)])
    # stream, P, C, S, N, row_class, clone_rows, split_rows, opacity, max_scaling, child_max_scaling, min_opacity, use_size,
    # screen_dead, big_threshold, small_threshold, seg, seg_cols, source_row, kind, child, map_new, map_state, motion_mask,
    # motion_rank, scratch, counts
    lib.gft_densify_layout.restype = C.c_int
    lib.gft_densify_layout.argtypes = ([C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32] + [C.c_void_p] * 6 +
                                       [C.c_float, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int32] +
                                       [C.c_void_p] * 8 + [C.POINTER(C.c_int64)])
    # stream, n_out, map, src, src_rows, extra, dst, row_bytes
    lib.gft_rows_remap.restype = C.c_int
    lib.gft_rows_remap.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    # stream, P, S, N, split_rows, xyz, rotation, scaling, z, new_xyz
    lib.gft_split_children.restype = C.c_int
    lib.gft_split_children.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32] + [C.c_void_p] * 6
    lib.gft_knn_scratch_bytes.restype = C.c_size_t
    lib.gft_knn_scratch_bytes.argtypes = [C.c_int32]
    lib.gft_knn_mean_dist2.restype = C.c_int
    lib.gft_knn_mean_dist2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gft_assemble_scratch_bytes.restype = C.c_size_t
    lib.gft_assemble_scratch_bytes.argtypes = [C.c_int32]
    lib.gft_assemble_forward.restype = C.c_int
    lib.gft_assemble_forward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(AssembleIO)]
    lib.gft_assemble_backward.restype = C.c_int
    lib.gft_assemble_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(AssembleBwdIO)]
    lib.gft_assemble_num_dynamic.restype = C.c_int
    lib.gft_assemble_num_dynamic.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]
    lib.gft_forward.restype = C.c_int
    lib.gft_forward.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(ForwardIO), C.POINTER(ForwardHints),
                                C.POINTER(ForwardReport)]
    lib.gft_forward_render.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(ForwardIO), C.c_int64, C.c_int64]
    lib.gft_forward_enqueue.restype = C.c_int
    lib.gft_forward_enqueue.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(ForwardIO), C.POINTER(ForwardHints), C.c_void_p]
    lib.gft_backward.restype = C.c_int
    lib.gft_backward.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(BackwardIO), C.c_int64]
    lib.gft_backward_det.restype = C.c_int
    lib.gft_backward_det.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(BackwardIO), C.c_int64, C.c_void_p]
    lib.gft_grads_rezero.restype = C.c_int
    lib.gft_grads_rezero.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(BackwardIO)]
    lib.gft_mark_visible.restype = C.c_int
    lib.gft_mark_visible.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_float, C.c_float, C.c_void_p]
    lib.gft_profile_enable.restype = C.c_int
    lib.gft_profile_enable.argtypes = [C.c_int]
    lib.gft_profile_reset.restype = C.c_int
    lib.gft_profile_read.restype = C.c_int
    lib.gft_profile_read.argtypes = [C.POINTER(Profile)]
    _lib = lib
    return lib


def raw_stream(dev):
    """hipStream_t of torch's current stream on `dev` as an integer (the C ABI takes void*).  The private fast path
    costs ~0.3 us, torch.cuda.current_stream(dev).cuda_stream ~4 us: a training iteration asks ~40 times."""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    except Exception:
        return torch.cuda.current_stream(dev).cuda_stream


class on_device:
    """`with torch.cuda.device(dev)` only when dev is not already the current device (the context manager costs
    ~10 us, the check ~1 us)."""

    def __init__(self, dev):
        import torch
        self.ctx = None
        idx = dev.index
        if idx is not None and idx != torch.cuda.current_device():
            self.ctx = torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def last_error():
    return load().gft_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != 0:
        raise RuntimeError(last_error())


def get_layout(P, W, H, R=0):
    L = Layout()
    check(load().gft_get_layout(P, W, H, R, C.byref(L)))
    return L


def profile_enable(on=True):
    load().gft_profile_enable(1 if on else 0)


def profile_reset():
    load().gft_profile_reset()


def profile_read():
    p = Profile()
    check(load().gft_profile_read(C.byref(p)))
    d = {n: getattr(p, n) for n in PROFILE_FIELDS}
    d["forward_calls"] = p.forward_calls
    d["backward_calls"] = p.backward_calls
    return d
