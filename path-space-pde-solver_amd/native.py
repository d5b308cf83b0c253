"""ctypes binding of libpsp_hip.so (C ABI in include/psp.h).

The library is the product path for the HJB rollout; there is no CPU fallback behind it.
``load()`` raises ``NativeLibraryError`` if the shared object is missing or does not export
every symbol the header declares.  torch is imported first on purpose: libpsp_hip.so needs
``libamdhip64.so.7`` and must bind to the HIP runtime torch already loaded, because stream
handles and device pointers are shared between the two.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen below)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PSP_LIB_PATH", os.path.join(HERE, "csrc", "libpsp_hip.so"))   # override: diagnostic builds

# enums (include/psp.h)
DRIFT_ZERO, DRIFT_DENSE, DRIFT_DIAG, DRIFT_DOUBLE_WELL = 0, 1, 2, 3
DRIFT_WELL_DIAG, DRIFT_RADIAL_WELL = 8, 9             # DenseNet-control family (psp_dnet_*) only
SIGMA_IDENTITY, SIGMA_DENSE, SIGMA_SCALED_IDENTITY = 0, 1, 2
RUNCOST_ZERO, RUNCOST_DIAG_QUAD = 0, 1
TERM_LINEAR, TERM_DIAG_QUAD, TERM_SHIFTED_QUAD = 0, 1, 2
TERM_QUAD_LINEAR, TERM_RADIAL_QUAD = 8, 9              # DenseNet-control family (psp_dnet_*) only
DNET_ONLY_KINDS = {'drift': (DRIFT_WELL_DIAG, DRIFT_RADIAL_WELL), 'term': (TERM_QUAD_LINEAR, TERM_RADIAL_QUAD)}


def dnet_only_kind(spec):
    """Why a native_spec() can run on the DenseNet-control kernels alone (csrc/hjbd_kernels.h), or None: the per-coordinate and
    radial drift / terminal kinds of DoubleWell_OU and DoubleWell_multidim_2 exist in that family only."""
    for key in ('drift', 'term'):
        if spec is not None and spec.get(key) is not None and spec[key][0] in DNET_ONLY_KINDS[key]:
            return ('the %s kind %d of this problem (per-coordinate / radial double well) exists in the DenseNet-control kernel '
                    'family only (psp_dnet_*: Solver with DenseNet controls)' % (key, spec[key][0]))
    return None
LOSS_LOG_VARIANCE, LOSS_MOMENT, LOSS_WEIGHTS, LOSS_REL_ENTROPY = 0, 1, 2, 3
UL2_TABLE, UL2_LINEAR, UL2_GRID = 0, 1, 2
ISC_NONE, ISC_TABLE, ISC_LINEAR, ISC_GRID = 0, 1, 2, 3
IS_MAX_D = 64                     # native range of psp_is_rollout (include/psp.h)
ISW_MAX_D = 256                   # native range of psp_isw_rollout (include/psp.h PSP_ISW_MAX_D)
GENL_MAX_HIDDEN_LAYERS, GENL_MAX_WIDTH, GENL_MAX_INPUT = 4, 128, 112      # the run-time-shaped value-net kernels (csrc/genl_kernels.h)
NOISE_SUPPLIED, NOISE_PHILOX = 0, 1
GH_ZERO, GH_QUAD, GH_ALLEN_CAHN, GH_EXPBALL_LIN, GH_EXPBALL_SQ, GH_EXPBALL_SIN, GH_EXPBALL_SIN_FULL = 0, 1, 2, 3, 4, 5, 6
GH_AFFINE_EXP, GH_SINE_SOURCE, GH_SINNORM2 = 7, 8, 9     # p0 + p1 y + p2 |z|^2 + p3 exp(-y); c y + s(x); SinNorm2.h (dense sigma)
GENL_SIGMA_SCALED, GENL_SIGMA_DENSE = 0, 1      # psp_genl_config.sigma_kind
MLP_FP32, MLP_BF16_FWD, MLP_BF16, MLP_F16X3 = 0, 1, 2, 3
DT_F32, DT_F64 = 0, 1
COMM_ID_BYTES = 128
DOM_NONE, DOM_SPHERE, DOM_BOX, DOM_BOX_UPPER_ALL, DOM_BOX_UPPER_ANY, DOM_ANNULUS = 0, 1, 2, 3, 4, 5
ACT_RELU2, ACT_TANH2, ACT_TANH = 0, 1, 2
TSAMPLE_SUPPLIED, TSAMPLE_BALL, TSAMPLE_ANNULUS, TSAMPLE_BOX = 0, 1, 2, 3     # psp_genl_eval_config.sample_kind
VTRUE_EXP, VTRUE_QUAD, VTRUE_COMMITTOR = 0, 1, 2                              # psp_genl_eval_config.vtrue_kind
VTRUE_LOGQ, VTRUE_SINPROD, VTRUE_SINSUM, VTRUE_SINR2 = 16, 17, 18, 19         # ... the group that also sees x_0, x_1


class NativeLibraryError(RuntimeError):
    pass


class NativeCallError(RuntimeError):
    pass


class HjbConfig(C.Structure):
    _fields_ = [
        ("d", C.c_int32), ("H", C.c_int32), ("K_local", C.c_int32), ("N", C.c_int32),
        ("K_global", C.c_int64), ("k_offset", C.c_int64),
        ("dt", C.c_float), ("sqrt_dt", C.c_float),
        ("drift_kind", C.c_int32), ("sigma_kind", C.c_int32), ("runcost_kind", C.c_int32),
        ("term_kind", C.c_int32), ("adaptive", C.c_int32), ("loss_kind", C.c_int32),
        ("noise_mode", C.c_int32), ("store_path", C.c_int32),
        ("sigma_scale", C.c_float), ("coord_split", C.c_int32),
        ("drift", C.c_void_p), ("sigma", C.c_void_p), ("runcost", C.c_void_p), ("term", C.c_void_p),
        ("u_ref", C.c_void_p), ("u_l2_out", C.c_void_p),
        ("mlp_dtype", C.c_int32), ("reserved2", C.c_int32),
        ("iter_dev", C.c_void_p),
        ("range_flag", C.c_void_p),
    ]


class IterState(C.Structure):
    _fields_ = [("iter", C.c_uint32), ("step", C.c_uint32), ("beta1_pow", C.c_double), ("beta2_pow", C.c_double)]


class HjbSizes(C.Structure):
    _fields_ = [
        ("path_bytes", C.c_int64), ("fwd_partial_bytes", C.c_int64), ("grad_partial_bytes", C.c_int64),
        ("n_params", C.c_int32), ("fwd_workgroups", C.c_int32), ("bwd_workgroups", C.c_int32),
        ("fwd_coop_tiles", C.c_int32),
    ]


class GenConfig(C.Structure):
    _fields_ = [
        ("d", C.c_int32), ("H", C.c_int32), ("K_local", C.c_int32), ("N", C.c_int32),
        ("k_offset", C.c_int64),
        ("dt", C.c_float), ("sqrt_dt", C.c_float), ("T", C.c_float), ("sigma_scale", C.c_float),
        ("drift_kind", C.c_int32), ("h_kind", C.c_int32), ("adaptive", C.c_int32), ("noise_mode", C.c_int32),
        ("store_path", C.c_int32), ("domain_kind", C.c_int32),
        ("drift", C.c_void_p),
        ("dom_a", C.c_float), ("dom_b", C.c_float), ("h_par", C.c_float * 4),
        ("d_real", C.c_int32), ("mlp_dtype", C.c_int32),
        ("v_steps_out", C.c_void_p), ("y_steps_out", C.c_void_p),
        ("per_sample_weights", C.c_int32), ("dwell_form", C.c_int32),
        ("range_flag", C.c_void_p),
    ]


class DnetConfig(C.Structure):
    _fields_ = [("base", HjbConfig), ("d_real", C.c_int32), ("H_real", C.c_int32), ("time_input", C.c_int32),
                ("per_step", C.c_int32), ("r1_out", C.c_void_p), ("r2_out", C.c_void_p), ("images_out", C.c_void_p),
                # u_L2 log of reference controls that depend on x (include/psp.h: PSP_UL2_*)
                ("ul2_kind", C.c_int32), ("ul2_ntables", C.c_int32), ("ul2_nrows", C.c_int32), ("ul2_ncols", C.c_int32),
                ("ul2_tables", C.c_void_p), ("ul2_group", C.c_void_p), ("ul2_row", C.c_void_p),
                ("ul2_xb", C.c_float), ("ul2_dx", C.c_float), ("ul2_xhi", C.c_float), ("ul2_reserved", C.c_int32)]


class IsConfig(C.Structure):
    _fields_ = [("d", C.c_int32), ("K_local", C.c_int32), ("N", C.c_int32), ("control_kind", C.c_int32),
                ("K_global", C.c_int64), ("k_offset", C.c_int64), ("dt", C.c_float), ("sqrt_dt", C.c_float),
                ("drift_kind", C.c_int32), ("sigma_kind", C.c_int32), ("runcost_kind", C.c_int32), ("term_kind", C.c_int32),
                ("noise_mode", C.c_int32), ("dwell_form", C.c_int32), ("sigma_scale", C.c_float), ("reserved", C.c_int32),
                ("x0", C.c_void_p), ("drift", C.c_void_p), ("sigma", C.c_void_p), ("runcost", C.c_void_p), ("term", C.c_void_p),
                ("u_ref", C.c_void_p), ("u_group", C.c_void_p), ("u_row", C.c_void_p),
                ("u_ntables", C.c_int32), ("u_nrows", C.c_int32), ("u_ncols", C.c_int32),
                ("u_xb", C.c_float), ("u_dx", C.c_float), ("u_xhi", C.c_float)]


class IswSizes(C.Structure):
    """psp_isw_sizes; ``struct_bytes`` is set here and checked by the library."""
    _fields_ = [("struct_bytes", C.c_int32), ("lds_bytes", C.c_int32), ("table_bytes", C.c_int64), ("workgroups", C.c_int32),
                ("max_d", C.c_int32)]

    def __init__(self):
        super().__init__()
        self.struct_bytes = C.sizeof(IswSizes)


class AffConfig(C.Structure):
    """psp_aff_config: a linear / affine / constant control per time step (psp_aff_*).  The library checks ``struct_bytes``
    itself; the struct is not part of psp_abi_struct_sizes*."""
    _fields_ = [("base", HjbConfig), ("struct_bytes", C.c_int32), ("d_real", C.c_int32), ("has_matrix", C.c_int32),
                ("has_bias", C.c_int32), ("ul2_kind", C.c_int32), ("reserved", C.c_int32), ("ul2_ref", C.c_void_p)]


class AffSizes(C.Structure):
    _fields_ = [("path_bytes", C.c_int64), ("fwd_partial_bytes", C.c_int64), ("partial_bytes", C.c_int64),
                ("fwd_workgroups", C.c_int32), ("fwd_threads", C.c_int32), ("slices", C.c_int32), ("padded_params", C.c_int32),
                ("bwd_workgroups", C.c_int32), ("lds_bytes", C.c_int32)]


class DnetSizes(C.Structure):
    _fields_ = [("table_bytes", C.c_int64), ("fwd_partial_bytes", C.c_int64), ("n_params_per_set", C.c_int64),
                ("fwd_workgroups", C.c_int32), ("reserved", C.c_int32),
                ("image_bytes", C.c_int64), ("partial_bytes", C.c_int64),
                ("bwd_supported", C.c_int32), ("slices", C.c_int32), ("padded_params", C.c_int32), ("bwd_workgroups", C.c_int32)]


class GenSizes(C.Structure):
    _fields_ = [
        ("path_bytes", C.c_int64), ("ahat_bytes", C.c_int64), ("grad_partial_bytes", C.c_int64),
        ("n_params", C.c_int32), ("fwd_workgroups", C.c_int32), ("bwd_workgroups", C.c_int32),
        ("fwd_coop_tiles", C.c_int32),
    ]


class GenlConfig(C.Structure):
    _fields_ = [("base", GenConfig), ("has_time", C.c_int32), ("n_hidden", C.c_int32), ("widths", C.c_int32 * 4),
                ("activation", C.c_int32), ("linear_layout", C.c_int32), ("time_first", C.c_int32), ("time_scale", C.c_float),
                # appended: a dense constant diffusion matrix (0: base.sigma_scale * I; 1: `sigma`, device, d*d row-major)
                ("sigma_kind", C.c_int32), ("reserved", C.c_int32), ("sigma", C.c_void_p)]


GENL_Z_SIGMA_T, GENL_Z_SIGMA = 0, 1             # psp_genl_coeffs.z_kind


class GenlCoeffs(C.Structure):
    """psp_genl_coeffs: the linear-quadratic coefficients beside a GenlConfig (psp_genl_query_lq / psp_genl_rollout_fwd_lq).  The
    library checks ``struct_bytes`` itself; the struct is not part of psp_abi_struct_sizes*."""
    _fields_ = [("struct_bytes", C.c_int32), ("z_kind", C.c_int32), ("runcost_kind", C.c_int32), ("reserved", C.c_int32),
                ("drift_matrix", C.c_void_p), ("runcost", C.c_void_p)]


class GenlUl2(C.Structure):
    """psp_genl_ul2: the u_L2 log beside a GenlConfig and a GenlCoeffs (psp_genl_query_ul2 / psp_genl_ul2_stage /
    psp_genl_rollout_fwd_ul2).  The library checks ``struct_bytes`` itself; the struct is not part of psp_abi_struct_sizes*."""
    _fields_ = [("struct_bytes", C.c_int32), ("kind", C.c_int32), ("u_l2_out", C.c_void_p), ("u_ref", C.c_void_p),
                ("tables", C.c_void_p), ("group", C.c_void_p), ("row", C.c_void_p),
                ("ntables", C.c_int32), ("nrows", C.c_int32), ("ncols", C.c_int32),
                ("xb", C.c_float), ("dx", C.c_float), ("xhi", C.c_float), ("K_global", C.c_int64)]


GH_EIG_FP, GH_EIG_NLS, DRIFT_EIG_FP = 16, 17, 16      # the eigenvalue problems: psp_genl_query_eig / psp_genl_rollout_fwd_eig only


class GenlEig(C.Structure):
    """psp_genl_eig: a trained lambda in device memory, the output ReLU's gate and the S_k output beside a GenlConfig
    (psp_genl_query_eig / psp_genl_rollout_fwd_eig).  The library checks ``struct_bytes`` itself."""
    _fields_ = [("struct_bytes", C.c_int32), ("output_relu", C.c_int32), ("lambda_", C.c_void_p), ("s_out", C.c_void_p)]


class GenlAdj(C.Structure):
    """psp_genl_adj: the adjoint sweep of the state path beside a GenlConfig, a GenlCoeffs and a GenlUl2 (psp_genl_query_adj /
    psp_genl_adjoint_sweep).  The library checks ``struct_bytes`` itself and psp_genl_query_adj writes ``drift_t_offset``."""
    _fields_ = [("struct_bytes", C.c_int32), ("reserved", C.c_int32), ("mu", C.c_void_p), ("resid_coeff", C.c_void_p),
                ("lam_N", C.c_void_p), ("lam0_out", C.c_void_p), ("drift_t_offset", C.c_int64)]


class GenlSizes(C.Structure):
    _fields_ = [("table_bytes", C.c_int64), ("path_bytes", C.c_int64), ("ahat_bytes", C.c_int64), ("n_params", C.c_int64),
                ("grad_partial_bytes", C.c_int64), ("n_blocks", C.c_int32), ("fwd_workgroups", C.c_int32),
                ("bwd_workgroups", C.c_int32), ("waves_per_tile", C.c_int32), ("seg_block_offset", C.c_int32 * 5),
                ("reserved", C.c_int32)]


class GenlEvalConfig(C.Structure):
    _fields_ = [("d", C.c_int32), ("has_time", C.c_int32), ("n_hidden", C.c_int32), ("widths", C.c_int32 * 4),
                ("activation", C.c_int32), ("linear_layout", C.c_int32), ("time_first", C.c_int32), ("time_scale", C.c_float),
                ("K_points", C.c_int32), ("sample_kind", C.c_int32), ("k_offset", C.c_int64),
                ("bound_a", C.c_float), ("bound_b", C.c_float), ("T", C.c_float), ("vtrue_kind", C.c_int32),
                ("vtrue_par", C.c_float * 4), ("log_slots", C.c_int32), ("reserved", C.c_int32)]


class GenlEvalSizes(C.Structure):
    _fields_ = [("table_bytes", C.c_int64), ("partial_bytes", C.c_int64), ("n_params", C.c_int64),
                ("workgroups", C.c_int32), ("waves_per_tile", C.c_int32), ("lds_bytes", C.c_int32), ("reserved", C.c_int32)]


class PinnConfig(C.Structure):
    """psp_pinn_config: the PINN residual of a dense-concat value net (psp_pinn_query / psp_pinn_residual / psp_pinn_backward, and
    psp_pinn_pairs_* for an h that reads t)."""
    _fields_ = [("d", C.c_int32), ("K", C.c_int32), ("has_time", C.c_int32), ("n_hidden", C.c_int32), ("widths", C.c_int32 * 4),
                ("activation", C.c_int32), ("linear_layout", C.c_int32), ("drift_kind", C.c_int32), ("h_kind", C.c_int32),
                ("sigma_kind", C.c_int32), ("n_dirs", C.c_int32), ("sigma_scale", C.c_float), ("h_par", C.c_float * 4),
                ("reserved_f", C.c_float), ("drift", C.c_void_p), ("dirs", C.c_void_p)]


class PinnSizes(C.Structure):
    _fields_ = [("n_params", C.c_int64), ("scratch_bytes", C.c_int64), ("grad_partial_bytes", C.c_int64),
                ("dir_blocks", C.c_int32), ("tiles", C.c_int32), ("bwd_workgroups", C.c_int32), ("lds_fwd_bytes", C.c_int32),
                ("lds_bwd_bytes", C.c_int32), ("reserved", C.c_int32)]


_P = C.c_void_p
SIGNATURES = {
    "psp_version": (C.c_int, []),
    "psp_abi_struct_sizes": (C.c_int, [C.POINTER(C.c_int32 * 6)]),
    "psp_abi_struct_sizes2": (C.c_int, [C.POINTER(C.c_int32 * 2)]),
    "psp_last_error": (C.c_char_p, []),
    "psp_abi_struct_sizes3": (C.c_int, [C.POINTER(C.c_int32 * 1)]),
    "psp_is_rollout": (C.c_int, [C.POINTER(IsConfig), _P, C.c_uint64, C.c_uint32, _P, _P, _P]),
    "psp_is_query": (C.c_int, [C.POINTER(IsConfig), C.POINTER(C.c_int32)]),
    "psp_isw_query": (C.c_int, [C.POINTER(IsConfig), C.POINTER(IswSizes)]),
    "psp_isw_rollout": (C.c_int, [C.POINTER(IsConfig), _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P]),
    "psp_abi_struct_sizes4": (C.c_int, [C.POINTER(C.c_int32 * 2)]),
    "psp_genl_eval_query": (C.c_int, [C.POINTER(GenlEvalConfig), C.POINTER(GenlEvalSizes)]),
    "psp_genl_test_error": (C.c_int, [C.POINTER(GenlEvalConfig), _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, C.c_int32, _P,
                                      _P, _P, _P, _P, _P, _P]),
    "psp_abi_struct_sizes5": (C.c_int, [C.POINTER(C.c_int32 * 2)]),
    "psp_pinn_query": (C.c_int, [C.POINTER(PinnConfig), C.POINTER(PinnSizes)]),
    "psp_pinn_residual": (C.c_int, [C.POINTER(PinnConfig), _P, _P, _P, _P, _P, _P]),
    "psp_pinn_backward": (C.c_int, [C.POINTER(PinnConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_pinn_pairs_query": (C.c_int, [C.POINTER(PinnConfig), C.POINTER(PinnSizes), C.POINTER(C.c_int64)]),
    "psp_pinn_pairs_residual": (C.c_int, [C.POINTER(PinnConfig), _P, _P, _P, _P, _P, _P]),
    "psp_pinn_pairs_reduce": (C.c_int, [C.POINTER(PinnConfig), _P, _P, _P, _P, C.c_float, _P, _P, _P, _P, _P]),
    "psp_pinn_pairs_backward": (C.c_int, [C.POINTER(PinnConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_loss_stats_state_bytes": (C.c_int64, []),
    "psp_loss_stats_accumulate": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "psp_loss_stats_finish": (C.c_int, [_P, _P, _P]),
    "psp_genl_query": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlSizes)]),
    "psp_genl_rollout_fwd": (C.c_int, [C.POINTER(GenlConfig), _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P, _P, _P,
                                       _P, _P]),
    "psp_genl_rollout_bwd": (C.c_int, [C.POINTER(GenlConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_genl_query_lq": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), C.POINTER(GenlSizes)]),
    "psp_genl_rollout_fwd_lq": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P,
                                          _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_genl_query_ul2": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), C.POINTER(GenlUl2), C.POINTER(GenlSizes)]),
    "psp_genl_ul2_stage": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), C.POINTER(GenlUl2), _P, _P]),
    "psp_genl_rollout_fwd_ul2": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), C.POINTER(GenlUl2), _P, _P, _P, _P,
                                           C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_genl_query_eig": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlEig), C.POINTER(GenlSizes)]),
    "psp_genl_rollout_fwd_eig": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlEig), _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P,
                                           _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_genl_query_adj": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), C.POINTER(GenlUl2), C.POINTER(GenlAdj),
                                     C.POINTER(GenlSizes)]),
    "psp_genl_adjoint_sweep": (C.c_int, [C.POINTER(GenlConfig), C.POINTER(GenlCoeffs), C.POINTER(GenlAdj), _P, _P, _P, _P, _P, _P]),
    "psp_hjb_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "psp_hjb_family": (C.c_int, [C.c_int32, C.c_int32]),
    "psp_hjb_adjoint_sweep": (C.c_int, [C.POINTER(HjbConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_dnet_instance_count": (C.c_int, []),
    "psp_dnet_instance_get": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "psp_dnet_query": (C.c_int, [C.POINTER(DnetConfig), C.POINTER(DnetSizes)]),
    "psp_dnet_terminal_reduce": (C.c_int, [C.POINTER(DnetConfig), _P, _P, _P]),
    "psp_dnet_rollout_bwd": (C.c_int, [C.POINTER(DnetConfig), _P, _P, _P, _P, _P]),
    "psp_dnet_rollout_bwd_sq": (C.c_int, [C.POINTER(DnetConfig), _P, _P, _P, _P, _P]),
    "psp_gradvar_finish": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P,
                                     _P, _P, _P, _P, _P, _P]),
    "psp_dnet_adjoint_sweep": (C.c_int, [C.POINTER(DnetConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_dnet_ul2_stage": (C.c_int, [C.POINTER(DnetConfig), _P, _P]),
    "psp_dnet_rollout_fwd": (C.c_int, [C.POINTER(DnetConfig), _P, _P, C.c_int32, _P, _P, C.c_uint64, C.c_uint32, _P,
                                       _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "psp_aff_instance_count": (C.c_int, []),
    "psp_aff_instance_get": (C.c_int, [C.c_int32, C.POINTER(C.c_int32)]),
    "psp_aff_query": (C.c_int, [C.POINTER(AffConfig), C.POINTER(AffSizes)]),
    "psp_aff_rollout_fwd": (C.c_int, [C.POINTER(AffConfig), _P, _P, _P, C.c_int32, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P,
                                      _P, _P, _P]),
    "psp_aff_terminal_reduce": (C.c_int, [C.POINTER(AffConfig), _P, _P, _P]),
    "psp_aff_adjoint_sweep": (C.c_int, [C.POINTER(AffConfig), _P, _P, _P, _P, _P, _P, _P]),
    "psp_aff_rollout_bwd": (C.c_int, [C.POINTER(AffConfig), _P, _P, _P, _P]),
    "psp_gen_instance_count": (C.c_int, []),
    "psp_gen_instance_get": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "psp_hjb_instance_count": (C.c_int, []),
    "psp_hjb_instance_get": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "psp_hjb_query": (C.c_int, [C.POINTER(HjbConfig), C.POINTER(HjbSizes)]),
    "psp_hjb_rollout_fwd": (C.c_int, [C.POINTER(HjbConfig), _P, _P, C.c_int32, _P, _P, C.c_uint64, C.c_uint32,
                                      _P, _P, _P, _P, _P, _P]),
    "psp_hjb_rollout_eval": (C.c_int, [C.POINTER(HjbConfig), _P, _P, C.c_int32, _P, C.c_uint64, C.c_uint32, _P, _P, _P,
                                       _P, _P, _P]),
    "psp_hjb_terminal_reduce": (C.c_int, [C.POINTER(HjbConfig), _P, _P, _P]),
    "psp_hjb_rollout_bwd": (C.c_int, [C.POINTER(HjbConfig), _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "psp_adam_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "psp_hjb_basis_params": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int64, _P]),
    "psp_hjb_basis_grad": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "psp_philox_normal_fill": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_uint64, C.c_uint32, _P]),
    "psp_hjb_control_eval": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_float, _P, _P]),
    "psp_debug_set_stamp_buffer": (C.c_int, [_P, C.c_int64]),
    "psp_iter_state_init": (C.c_int, [C.POINTER(IterState), C.c_uint32, C.c_int32, C.c_float, C.c_float]),
    "psp_iter_state_advance": (C.c_int, [_P, C.c_float, C.c_float, _P]),
    "psp_hjb_terminal_reduce_loss": (C.c_int, [C.POINTER(HjbConfig), _P, _P, _P, _P, _P]),
    "psp_hjb_rollout_bwd_step": (C.c_int, [C.POINTER(HjbConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float,
                                           C.c_float, C.c_float, _P]),
    "psp_adam_step_dev": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "psp_comm_unique_id": (C.c_int, [_P]),
    "psp_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, _P]),
    "psp_comm_destroy": (C.c_int, [_P]),
    "psp_allreduce": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P]),
    "psp_gen_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "psp_gen_query": (C.c_int, [C.POINTER(GenConfig), C.POINTER(GenSizes)]),
    "psp_gen_rollout_fwd": (C.c_int, [C.POINTER(GenConfig), _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P,
                                      _P, _P, _P, _P]),
    "psp_gen_rollout_bwd": (C.c_int, [C.POINTER(GenConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
}

# the structs each psp_abi_struct_sizes* call reports, in its order
ABI_STRUCTS = (
    ("psp_abi_struct_sizes", (HjbConfig, HjbSizes, GenConfig, GenSizes, DnetConfig, DnetSizes)),
    ("psp_abi_struct_sizes2", (GenlConfig, GenlSizes)),
    ("psp_abi_struct_sizes3", (IsConfig,)),
    ("psp_abi_struct_sizes4", (GenlEvalConfig, GenlEvalSizes)),
    ("psp_abi_struct_sizes5", (PinnConfig, PinnSizes)),
)

_lib = None


def load():
    """dlopen libpsp_hip.so (once) and bind every symbol of include/psp.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "%s not found: build it with `python path-space-pde-solver_amd/build.py` "
            "(or __graft_entry__.build()). The HJB rollout has no non-HIP fallback." % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise NativeLibraryError("%s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    for symbol, structs in ABI_STRUCTS:
        sizes = (C.c_int32 * len(structs))()
        getattr(lib, symbol)(C.byref(sizes))
        mine = [C.sizeof(t) for t in structs]
        if list(sizes) != mine:      # a stale build or a drifted struct declaration would corrupt kernel arguments silently
            raise NativeLibraryError("%s was built for other struct layouts (library %s, binding %s): rebuild it"
                                     % (LIB_PATH, list(sizes), mine))
    _lib = lib
    return lib


def is_built():
    return os.path.exists(LIB_PATH)


def last_error():
    return load().psp_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise NativeCallError("%s failed (%d): %s" % (what, rc, last_error()))


def ptr(t, offset=0):
    """Raw device/host pointer of a tensor (or None), optionally `offset` ELEMENTS into it."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + int(offset) * t.element_size())


def stream_ptr(device):
    if device.type != "cuda":
        return None
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def supported(d, H):
    return bool(load().psp_hjb_supported(int(d), int(H)))


def family(d, H):
    """0 none, 1 narrow kernels, 2 wide kernels (large d)."""
    return int(load().psp_hjb_family(int(d), int(H)))


def _instances(family, n_fields):
    """The rows of psp_<family>_instance_get, `n_fields` int32 each."""
    lib = load()
    count, get = getattr(lib, "psp_%s_instance_count" % family), getattr(lib, "psp_%s_instance_get" % family)
    out = []
    for i in range(count()):
        row = [C.c_int32() for _ in range(n_fields)]
        check(get(i, *[C.byref(v) for v in row]), "psp_%s_instance_get" % family)
        out.append(tuple(v.value for v in row))
    return out


def instances():
    """[(d, H, family)] of the compiled HJB kernel instances (family 1 narrow, 2 wide)."""
    return _instances("hjb", 3)


def gen_instances():
    """[(d, H)] of the compiled GeneralSolver kernel instances."""
    return _instances("gen", 2)


def aff_instances():
    """[d] of the compiled linear-control buckets."""
    return [t[0] for t in _instances("aff", 1)]


def dnet_instances():
    """[(d, H)] of the compiled DenseNet-control forward kernels."""
    return _instances("dnet", 2)


def _query(symbol, cfg, sizes):
    """One size query without raising: (rc, sizes, message)."""
    lib = load()
    rc = getattr(lib, symbol)(C.byref(cfg), C.byref(sizes))
    return rc, sizes, (lib.psp_last_error().decode() if rc else '')


def gen_query_rc(cfg):
    return _query("psp_gen_query", cfg, GenSizes())


def query_rc(cfg):
    """psp_hjb_query without raising: (rc, sizes, message)."""
    return _query("psp_hjb_query", cfg, HjbSizes())


def gen_supported(d, H):
    return bool(load().psp_gen_supported(int(d), int(H)))


def gen_query(cfg):
    rc, sizes, _ = gen_query_rc(cfg)
    check(rc, "psp_gen_query")
    return sizes


def query(cfg):
    rc, sizes, _ = query_rc(cfg)
    check(rc, "psp_hjb_query")
    return sizes
