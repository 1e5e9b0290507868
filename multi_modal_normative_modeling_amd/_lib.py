"""ctypes binding of libnmhip.so (include/nmhip.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, the
caller gets an exception.  ``oracle/`` is never imported from here.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

NM_MAX_MOD = 8
NM_MAX_EXP = 4
# every integer NM_* constant below mirrors include/nmhip.h (tests/test_cabi_cpu.py holds them to it)
# the row-split launch's Adam sweep (csrc/nm_rowsplit.hip: SwTab, SW_NV): weight passes and vector segments per modality,
# and the vector elements (biases, logvar_out, alpha) nm_rowsplit_ok admits -- 3 per thread of k = 2 workgroups of 512
NM_RS_MAX_PASSES = 128
NM_RS_MAX_VSEGS = 144
NM_RS_MAX_VEC = 3 * 2 * 512
# the group map of a row-split launch (nm_rowsplit_groups): slots per launch, the entry of a padding slot
NM_RS_MAX_GROUPS = 128
NM_RS_GROUP_PAD = 65535
NM_MAX_HID = 8
NM_MAX_CLS = 5
NM_MAX_CLS_WIDTH = 512
NM_MAX_CLASSES = 4
NM_BATCH = 256
NM_MAX_WIDTH = 127
NM_MAX_LATENT = 64
NM_WIDE_MAX_WIDTH = 4096
NM_WIDE_MAX_LATENT = 128
NM_LOSS_STRIDE = 16

NM_COMBINE = {"poe": 0, "gpoe": 1, "moe": 2, "mopoe": 3, "poe2v": 4}

NM_F_BACKWARD = 1
NM_F_ADAM = 2
NM_F_GRADS = 4
NM_F_EXPORT = 8
NM_F_PROFILE = 16
NM_F_ZGIVEN = 32
NM_F_TRACE = 64
NM_LOSS_TC = 11
NM_LOSS_REG = 12
NM_LOSS_CE = 13
NM_LOSS_CONTRAST = 14
NM_F_BNSTATS = 256
NM_F_SPLIT = 512
NM_F_FAULT_INJECT = 1024
NM_F_PLAIN = 2048
# values of a job's hand-off error word (nm_split_errors): a hand-off timed out / the row-split kernel refused the shape /
# the plain-training kernel refused a job that does not pass nm_plain_ok
NM_SYNC_ERR_TIMEOUT = 1
NM_SYNC_ERR_SHAPE = 2
NM_SYNC_ERR_PLAIN = 3
NM_METRICS_MAX_N = 8192
NM_METRICS_STRIDE = 8
# nm_roi_effect: the Y rows its kernel stages in LDS at a time (tests put group sizes around it)
NM_ROI_Y_CHUNK = 128
# nm_roi_significance: the most label permutations, the permutations a workgroup of its sum pass takes, the rank rows it
# stages at a time (tests put n_perm and the heights around them)
NM_ROI_MAX_PERM = 65535
NM_ROI_PERM_CHUNK = 64
NM_ROI_ROW_CHUNK = 256
# nm_auc_bootstrap: the most resamples (the close pass holds them in LDS), the resamples a workgroup of its resample pass
# takes (tests put n_boot around it)
NM_BOOT_MAX = 16384
NM_BOOT_CHUNK = 64
# nm_column_regress: the model kinds, the most nuisance covariates, the Newton steps a Logit may take and their tolerance
NM_REG_OLS = 0
NM_REG_LOGIT = 1
NM_REG_MAX_COV = 4
NM_REG_MAX_ITER = 35
NM_REG_TOL = 1e-8
# nm_normative_z: the widest table (its rows pass holds mean and sd of every column in LDS), the rows a workgroup of that
# pass scores (tests put the heights around it)
NM_NORM_MAX_D = 4096
NM_NORM_ROWS_PER_WG = 32
# nm_cohort_quantiles: the most probabilities of a call (they travel as a kernel argument)
NM_CENT_MAX_Q = 32
# nm_operating_points: the rule kinds, the most rules of a call, the widest ROC grid, the longest threshold grid of a rule
NM_OP_ROC = 0
NM_OP_F1 = 1
NM_OP_PR = 2
NM_OP_COST = 3
NM_OP_EER = 4
NM_OP_F1MAX = 5
NM_OP_SPEC = 6
NM_OP_MAX_RULES = 16
NM_OP_MAX_GRID = 1024
NM_OP_MAX_LINSPACE = 65536
# nm_devpass_subsets: the most entries per job (every non-empty set of NM_MAX_EXP experts)
NM_MAX_SUBSETS = 15
# nm_devpass_draws: the most latent draws per row
NM_MAX_DRAWS = 64
# nm_devpass_iw: the most latent draws per row (no accumulators between the draws), and the columns of its row export
NM_MAX_IW_DRAWS = 1024
NM_IW_ROW_COLUMNS = 8
NM_E2E_ROW_COLUMNS = 8
NM_FI_ROW_COLUMNS = 8
# nm_decode_pass: the most covariate cells of a request
NM_MAX_CELLS = 64
# nm_chart_pass: the most rows of a request, and the columns of a chart row (mean, var_latent, n_rows, status)
NM_CHART_MAX_ROWS = 1 << 20
NM_CHART_COLUMNS = 4

# status codes (nmhip.h; nm_status_string gives the text)
NM_OK = 0
NM_E_NULL = -1
NM_E_MODALITIES = -2
NM_E_LAYERS = -3
NM_E_WIDTH = -4
NM_E_LATENT = -5
NM_E_LATENT_COV = -6
NM_E_PITCH = -7
NM_E_GEOMETRY = -8
NM_E_COMBINE = -9
NM_E_OFFSETS = -10
NM_E_REG_HEAD = -11
NM_E_METRICS = -12
NM_E_CLS_HEAD = -13
NM_E_COUNTS = -14
NM_E_SHADOW = -15
NM_E_RESIDENCY = -16
NM_E_PREP = -17
NM_E_OUTPUT = -18
NM_E_WIDE_TC = -19
NM_E_ROWSPLIT = -20
NM_E_N_PARAMS = -21
NM_E_DEVPASS = -22

LIB_PATH = Path(__file__).resolve().parent / "libnmhip.so"


class NmModality(C.Structure):
    _fields_ = [
        ("D", C.c_int32), ("Kx", C.c_int32), ("x_pitch", C.c_int32), ("Cz", C.c_int32),
        ("x_f32", C.c_void_p), ("xb", C.c_void_p), ("cz", C.c_void_p),
        ("enc_w", C.c_int64 * NM_MAX_HID), ("enc_b", C.c_int64 * NM_MAX_HID),
        ("mu_w", C.c_int64), ("mu_b", C.c_int64), ("lv_w", C.c_int64), ("lv_b", C.c_int64),
        ("logvar_out", C.c_int64),
        ("dec_w", C.c_int64 * NM_MAX_HID), ("dec_b", C.c_int64 * NM_MAX_HID),
        ("out_w", C.c_int64), ("out_b", C.c_int64),
        ("alpha", C.c_int64),
        ("enc_s", C.c_int64 * NM_MAX_HID), ("heads_s", C.c_int64), ("dec_s", C.c_int64 * NM_MAX_HID), ("out_s", C.c_int64),
        ("out_loc", C.c_void_p), ("out_sqerr", C.c_void_p), ("out_rowdev", C.c_void_p),
        ("dloc_extra", C.c_void_p), ("dloc_rowcoef", C.c_void_p),
    ]


class NmJob(C.Structure):
    _fields_ = [
        ("M", C.c_int32), ("M_enc", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("Z", C.c_int32),
        ("H", C.c_int32 * NM_MAX_HID),
        ("combine", C.c_int32), ("single_bypass", C.c_int32), ("n_rows", C.c_int32), ("non_linear", C.c_int32),
        ("act_slope", C.c_float), ("out_kind", C.c_int32), ("n_private", C.c_int32),
        ("var_floor", C.c_float), ("tc_weight", C.c_float), ("w_off", C.c_int64), ("dephase", C.c_int32), ("shared_cov", C.c_int32), ("wide", C.c_int32),
        ("loss_cap", C.c_int32), ("eps_cap", C.c_int32),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
        ("adam_off", C.c_int64), ("lr_table", C.c_void_p), ("lr_cap", C.c_int32),
        ("kl_weight", C.c_float), ("ll_weight", C.c_float),
        ("params", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("grads", C.c_void_p),
        ("eps", C.c_void_p), ("seed", C.c_uint64),
        ("loss_log", C.c_void_p), ("wsh", C.c_void_p), ("workspace", C.c_void_p), ("workspace_stride", C.c_int64),
        ("out_mu", C.c_void_p), ("out_logvar", C.c_void_p), ("out_z", C.c_void_p), ("dz_extra", C.c_void_p),
        ("reg_head", C.c_int32), ("reg_lambda", C.c_float), ("reg_w", C.c_int64 * 3), ("reg_b", C.c_int64 * 3),
        ("reg_s", C.c_int64), ("reg_resid", C.c_void_p), ("reg_dres", C.c_void_p),
        ("fi_target", C.c_void_p), ("out_fi_pred", C.c_void_p),
        ("cls_layers", C.c_int32), ("cls_classes", C.c_int32), ("cls_width", C.c_int32 * NM_MAX_CLS),
        ("cls_train", C.c_int32), ("cls_use_mu", C.c_int32),
        ("cls_w", C.c_int64 * (NM_MAX_CLS + 1)), ("cls_b", C.c_int64 * (NM_MAX_CLS + 1)),
        ("cls_bn_w", C.c_int64 * NM_MAX_CLS), ("cls_bn_b", C.c_int64 * NM_MAX_CLS),
        ("cls_bn_mean", C.c_int64 * NM_MAX_CLS), ("cls_bn_var", C.c_int64 * NM_MAX_CLS),
        ("cls_dropout", C.c_float), ("cls_margin", C.c_float), ("cls_w_ce", C.c_float), ("cls_w_contrast", C.c_float),
        ("labels", C.c_void_p), ("out_logits", C.c_void_p), ("dz_out", C.c_void_p),
        ("rowcoef_out", C.c_void_p * NM_MAX_MOD),
        ("gpart", C.c_void_p), ("gpart_stride", C.c_int64), ("n_params", C.c_int64),
        ("mod", NmModality * NM_MAX_MOD),
    ]


class NmSubset(C.Structure):
    """nm_subset_t: one entry of nm_devpass_subsets' [n_jobs][n_subsets] table (device memory)."""
    _fields_ = [("mask", C.c_uint32), ("reserved", C.c_uint32), ("present", C.c_void_p),
                ("out_loc", C.c_void_p * NM_MAX_EXP), ("out_sqerr", C.c_void_p * NM_MAX_EXP),
                ("out_rowdev", C.c_void_p * NM_MAX_EXP)]


class NmDraw(C.Structure):
    """nm_draw_t: one entry of nm_devpass_draws' [n_jobs][n_draws] table (device memory)."""
    _fields_ = [("seed", C.c_uint64), ("eps", C.c_void_p)]


class NmPred(C.Structure):
    """nm_pred_t: one job's predictive exports, nm_devpass_draws' [n_jobs] table (device memory)."""
    _fields_ = [("pred_mean", C.c_void_p * NM_MAX_EXP), ("pred_var", C.c_void_p * NM_MAX_EXP),
                ("pred_msq", C.c_void_p * NM_MAX_EXP), ("pred_z", C.c_void_p * NM_MAX_EXP),
                ("pred_rowdev", C.c_void_p * NM_MAX_EXP), ("pred_rowz2", C.c_void_p * NM_MAX_EXP),
                ("noise_var", C.c_void_p * NM_MAX_EXP)]


class NmIw(C.Structure):
    """nm_iw_t: one job's likelihood request, nm_devpass_iw's [n_jobs] table (device memory)."""
    _fields_ = [("row", C.c_void_p), ("recon_ll", C.c_void_p * NM_MAX_EXP), ("noise_var", C.c_void_p * NM_MAX_EXP),
                ("ll_const", C.c_float * NM_MAX_EXP), ("dec_mask", C.c_uint32)]


class NmE2e(C.Structure):
    """nm_e2e_t: one job's request, nm_e2e_pass' [n_jobs] table (device memory)."""
    _fields_ = [("row", C.c_void_p), ("use_mean", C.c_int32), ("want_mask", C.c_int32)]


class NmFi(C.Structure):
    """nm_fi_t: one job's request, nm_fi_pass' [n_jobs] table (device memory)."""
    _fields_ = [("row", C.c_void_p), ("fi_draws", C.c_void_p), ("use_mean", C.c_int32), ("want_mask", C.c_int32)]


class NmDecode(C.Structure):
    """nm_decode_t: one job's request, nm_decode_pass' [n_jobs] table (device memory)."""
    _fields_ = [("z", C.c_void_p), ("n_rows", C.c_int32), ("rows_alloc", C.c_int32), ("n_cells", C.c_int32),
                ("cgrid", C.c_void_p), ("cz", C.c_void_p * NM_MAX_EXP), ("x", C.c_void_p * NM_MAX_EXP),
                ("loc", C.c_void_p * NM_MAX_EXP), ("sqerr", C.c_void_p * NM_MAX_EXP), ("rowdev", C.c_void_p * NM_MAX_EXP)]


class NmChart(C.Structure):
    """nm_chart_t: one job's request, nm_chart_pass' [n_jobs] table (device memory)."""
    _fields_ = [("z", C.c_void_p), ("n_rows", C.c_int32), ("rows_alloc", C.c_int32), ("n_cells", C.c_int32),
                ("cgrid", C.c_void_p), ("part", C.c_void_p * NM_MAX_EXP), ("chart", C.c_void_p * NM_MAX_EXP),
                ("loc", C.c_void_p * NM_MAX_EXP)]


class NmRoiSet(C.Structure):
    """nm_roi_set_t: one matrix of nm_roi_effect's pointer table."""
    _fields_ = [("x", C.c_void_p), ("group", C.c_void_p), ("rows", C.c_int32), ("pitch", C.c_int32)]


class NmRegSet(C.Structure):
    """nm_reg_set_t: one table of nm_column_regress's pointer table."""
    _fields_ = [("x", C.c_void_p), ("target", C.c_void_p), ("cov", C.c_void_p), ("include", C.c_void_p),
                ("rows", C.c_int32), ("pitch", C.c_int32), ("cov_pitch", C.c_int32), ("pad", C.c_int32)]


class NmNormSet(C.Structure):
    """nm_norm_set_t: one table of the pointer table of nm_cohort_moments, nm_normative_z, nm_cohort_cov, nm_mahalanobis."""
    _fields_ = [("x", C.c_void_p), ("sub", C.c_void_p), ("group", C.c_void_p), ("z", C.c_void_p),
                ("rows", C.c_int32), ("pitch", C.c_int32), ("sub_pitch", C.c_int32), ("z_pitch", C.c_int32),
                ("row_off", C.c_int32), ("pad", C.c_int32)]


class NmFitSet(C.Structure):
    """nm_fit_set_t: one entry of the pointer table of nm_fit_quality and nm_fit_rank."""
    _fields_ = [("x", C.c_void_p), ("loc", C.c_void_p), ("var", C.c_void_p), ("col_var", C.c_void_p), ("group", C.c_void_p),
                ("rows", C.c_int32), ("pitch", C.c_int32), ("loc_pitch", C.c_int32), ("var_pitch", C.c_int32)]


class NmOpRule(C.Structure):
    """nm_op_rule_t: one row of nm_operating_points' rule table (host memory)."""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("a", C.c_double), ("b", C.c_double),
                ("cost_fn", C.c_double), ("cost_fp", C.c_double)]


class NmError(RuntimeError):
    pass


_lib = None


def load():
    """Load libnmhip.so from the package directory; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NmError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    lib = C.CDLL(str(LIB_PATH))
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    lib.nm_version.restype = C.c_int
    lib.nm_status_string.restype = C.c_char_p
    lib.nm_status_string.argtypes = [C.c_int]
    lib.nm_abi_sizes.argtypes = [C.POINTER(i64), C.POINTER(i64)]
    lib.nm_workspace_bytes.restype = i64
    lib.nm_fill_shadow.restype = i64
    lib.nm_fill_shadow.argtypes = [C.POINTER(NmJob)]
    lib.nm_sync_shadow.argtypes = [vp, i32, vp]
    lib.nm_xb_elems.restype = i64
    lib.nm_xb_elems.argtypes = [i32, i32]
    lib.nm_workspace_bytes.argtypes = [C.POINTER(NmJob)]
    lib.nm_workspace_offset.restype = i64
    lib.nm_workspace_offset.argtypes = [C.POINTER(NmJob), i32]
    lib.nm_validate_job.argtypes = [C.POINTER(NmJob)]
    for name in ("nm_launch", "nm_launch_scalar_tr"):
        getattr(lib, name).argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.nm_launch_split.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.nm_launch_wide.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.nm_split_errors.argtypes = [vp, i32, vp, i32, vp]
    lib.nm_launch_rowsplit.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.nm_launch_rowsplit_mixed.argtypes = [vp, i32, C.POINTER(i32), i32, i32, i32, i32, i32, i32, vp]
    lib.nm_rowsplit_groups.argtypes = [C.POINTER(i32), i32, C.POINTER(i32), i32]
    lib.nm_rowsplit_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_plain_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_sync_reset.argtypes = [vp, i32, vp]
    lib.nm_trace_read_rs.argtypes = [C.POINTER(C.c_ulonglong), i32]
    lib.nm_devpass.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.nm_trace_read_dv.argtypes = [C.POINTER(C.c_ulonglong), i32]
    lib.nm_devpass_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_devpass_multi.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.nm_devpass_multi_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_devpass_subsets.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp]
    lib.nm_devpass_subsets_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_devpass_draws.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp]
    lib.nm_devpass_draws_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_devpass_iw.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp]
    lib.nm_devpass_iw_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_iw_check.argtypes = [C.POINTER(NmJob), C.POINTER(NmIw)]
    lib.nm_e2e_pass.argtypes = [vp, i32, vp, i32, i32, i32, vp]
    lib.nm_e2e_pass_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_e2e_alpha_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_fi_pass.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp]
    lib.nm_fi_pass_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_latent_pass.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.nm_latent_pass_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_decode_pass.argtypes = [vp, i32, vp, i32, i32, i32, vp]
    lib.nm_decode_pass_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_chart_pass.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp]
    lib.nm_chart_pass_ok.argtypes = [C.POINTER(NmJob)]
    lib.nm_latent_stats.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.nm_latent_score.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.nm_combine_latent.argtypes = [vp, vp, i32, i64, i32, vp, i32, i32, i32, f32, vp, vp, vp]
    lib.nm_total_correlation.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.nm_train_steps.argtypes = [vp, i32, i32, i32, vp]
    lib.nm_train_steps_persistent.argtypes = [vp, i32, i32, i32, vp]
    lib.nm_deviation.argtypes = [vp, i32, i32, i32, vp]
    lib.nm_grads.argtypes = [vp, i32, i32, vp]
    lib.nm_forward.argtypes = [vp, i32, i32, i32, vp]
    lib.nm_head_regression.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.nm_head_classifier.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.nm_train_steps_head.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.nm_train_steps_head.restype = i32
    lib.nm_train_steps_head_split.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.nm_train_steps_head_split.restype = i32
    lib.nm_posthoc_metrics.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.nm_confusion_metrics.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.nm_roi_effect.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.nm_roi_significance_workspace.restype = C.c_size_t
    lib.nm_roi_significance_workspace.argtypes = [i32, i32, i32, i32]
    lib.nm_roi_significance.argtypes = [vp, i32, i32, i32, i32, C.c_uint64, vp, C.c_size_t, vp, vp, vp]
    lib.nm_auc_bootstrap_workspace.restype = C.c_size_t
    lib.nm_auc_bootstrap_workspace.argtypes = [i32, i32, i32, i32]
    lib.nm_auc_bootstrap.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, C.c_uint64, vp, i32, vp, C.c_size_t, vp, vp, vp, vp]
    lib.nm_operating_points_workspace.restype = C.c_size_t
    lib.nm_operating_points_workspace.argtypes = [i32, i32]
    lib.nm_operating_points.argtypes = [vp, vp, vp, i32, i32, C.POINTER(NmOpRule), i32, vp, i32, vp, C.c_double, C.c_double,
                                        C.c_double, vp, C.c_size_t, vp, vp, vp, i32, vp]
    lib.nm_column_regress.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    lib.nm_cohort_moments.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.nm_normative_z.argtypes = [vp, i32, i32, i32, vp, i32, vp, C.c_double, vp, vp, vp]
    lib.nm_cohort_cov.argtypes = [vp, i32, i32, i32, C.c_double, vp, vp, vp, vp]
    lib.nm_mahalanobis.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.nm_cohort_quantiles.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_double), i32, vp, vp, vp]
    lib.nm_normative_centile_workspace.restype = C.c_size_t
    lib.nm_normative_centile_workspace.argtypes = [i32, i32]
    lib.nm_normative_centile.argtypes = [vp, i32, i32, i32, i32, vp, C.c_double, i32, vp, C.c_size_t, vp, vp, vp]
    lib.nm_fit_quality.argtypes = [vp, i32, i32, i32, vp, i32, vp, C.c_double, vp, vp, vp]
    lib.nm_fit_rank.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.nm_student_t_two_sided.restype = C.c_double
    lib.nm_student_t_two_sided.argtypes = [C.c_double, C.c_double]
    lib.nm_adam_step.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, vp]
    lib.nm_pack_table.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp]
    lib.nm_prep_scaler_fit.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp]
    lib.nm_prep_onehot.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, vp, vp]
    lib.nm_pack_table_raw.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp]
    lib.nm_test_gemm.argtypes = [i32, vp, vp, vp, i32, i32, i32, vp]
    lib.nm_prof_read.argtypes = [C.POINTER(C.c_ulonglong), i32]
    lib.nm_trace_read.argtypes = [C.POINTER(C.c_ulonglong), i32]
    lib.nm_wgtimes_read.argtypes = [C.POINTER(C.c_ulonglong)]
    sj, sm = i64(0), i64(0)
    lib.nm_abi_sizes(C.byref(sj), C.byref(sm))
    if sj.value != C.sizeof(NmJob) or sm.value != C.sizeof(NmModality):
        raise NmError(f"ABI mismatch: C sizeof(nm_job_t)={sj.value}, sizeof(nm_modality_t)={sm.value}; "
                      f"ctypes {C.sizeof(NmJob)}, {C.sizeof(NmModality)}")
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "nm_version", "nm_status_string", "nm_abi_sizes", "nm_workspace_bytes", "nm_validate_job", "nm_launch",
    "nm_launch_scalar_tr", "nm_train_steps", "nm_grads", "nm_forward", "nm_adam_step", "nm_pack_table",
    "nm_test_gemm", "nm_prof_read", "nm_trace_read", "nm_wgtimes_read", "nm_head_regression", "nm_head_classifier", "nm_train_steps_head", "nm_train_steps_head_split", "nm_train_steps_persistent", "nm_deviation", "nm_posthoc_metrics", "nm_confusion_metrics",
    "nm_fill_shadow", "nm_sync_shadow", "nm_xb_elems", "nm_launch_split", "nm_launch_wide", "nm_split_errors", "nm_combine_latent", "nm_total_correlation",
    "nm_prep_scaler_fit", "nm_prep_onehot", "nm_pack_table_raw",
    "nm_launch_rowsplit", "nm_rowsplit_ok", "nm_sync_reset", "nm_trace_read_rs", "nm_devpass", "nm_devpass_ok", "nm_trace_read_dv", "nm_workspace_offset",
    "nm_launch_rowsplit_mixed", "nm_rowsplit_groups", "nm_devpass_multi", "nm_devpass_multi_ok",
    "nm_latent_pass", "nm_latent_pass_ok", "nm_latent_stats", "nm_latent_score",
    "nm_roi_effect", "nm_roi_significance_workspace", "nm_roi_significance",
    "nm_auc_bootstrap_workspace", "nm_auc_bootstrap",
    "nm_column_regress", "nm_student_t_two_sided",
    "nm_plain_ok",
    "nm_cohort_moments", "nm_normative_z", "nm_cohort_cov", "nm_mahalanobis",
    "nm_operating_points_workspace", "nm_operating_points",
    "nm_cohort_quantiles", "nm_normative_centile_workspace", "nm_normative_centile",
    "nm_devpass_subsets", "nm_devpass_subsets_ok",
    "nm_devpass_draws", "nm_devpass_draws_ok",
    "nm_devpass_iw", "nm_devpass_iw_ok", "nm_iw_check",
    "nm_decode_pass", "nm_decode_pass_ok",
    "nm_chart_pass", "nm_chart_pass_ok",
    "nm_fit_quality", "nm_fit_rank",
    "nm_e2e_pass", "nm_e2e_pass_ok", "nm_e2e_alpha_ok",
    "nm_fi_pass", "nm_fi_pass_ok",
]


def check(status: int, what: str = "nmhip"):
    if status != 0:
        msg = load().nm_status_string(status).decode()
        raise NmError(f"{what} failed with status {status}: {msg}")
