"""ctypes binding of ``liboasisx_hip.so`` (declared in ``include/oasisx_hip.h``).

The HIP library IS the compute path: there is no CPU fallback.  ``load()`` raises
if the shared object is missing, and every wrapper raises ``OasisxHipError`` with the
library's message when a call fails.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OX_LIB_PATH") or os.path.join(_HERE, "liboasisx_hip.so")  # override: tuning builds

KSP_CG, KSP_BCGS, KSP_CG_SINGLE, KSP_BCGS_MERGED, KSP_CG_MERGED = 1, 2, 3, 4, 5
KSP_CG_MG = 6  # OX_KSP_CG_MG: CG preconditioned by the V-cycle of ox_ksp_options.mg
MG_MAX_DEGREE = 8  # OX_MG_MAX_DEGREE
ROW_BLOCK_WAVES, ROW_BLOCK_LDS = 8, 134 * 1024  # OX_ROW_BLOCK_WAVES / OX_ROW_BLOCK_LDS of include/oasisx_hip.h
CONVERGED_RTOL, CONVERGED_ATOL, CONVERGED_ITS = 2, 3, 4
DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_BREAKDOWN, DIVERGED_NANORINF = -3, -4, -5, -9


class OasisxHipError(RuntimeError):
    pass


class ox_sell(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int64),
        ("n_cols", C.c_int64),
        ("n_slices", C.c_int32),
        ("n_dict", C.c_int32),
        ("slice_ptr", C.c_void_p),
        ("cols", C.c_void_p),
        ("vals", C.c_void_p),
        ("cols16", C.c_void_p),
        ("cbase", C.c_void_p),
        ("vcode", C.c_void_p),
        ("vdict", C.c_void_p),
        ("ib_slices", C.c_void_p),
        ("n_interior", C.c_int32),
        ("n_wb_interior", C.c_int32),
        ("ps_ptr", C.c_void_p),
        ("ps_code", C.c_void_p),
        ("ps_base", C.c_void_p),
        ("wb_slices", C.c_void_p),
        ("wb_waves", C.c_void_p),
        ("wb_ptr", C.c_void_p),
        ("wlist", C.c_void_p),
        ("wt_ptr", C.c_void_p),
        ("wcode", C.c_void_p),
        ("wvcode", C.c_void_p),
        ("n_wblocks", C.c_int32),
        ("w_max", C.c_int32),
        ("levels", C.c_int32),
        ("w_cap", C.c_int32),
    ]


class ox_window_info(C.Structure):
    _fields_ = [
        ("n_wblocks", C.c_int32),
        ("w_max", C.c_int32),
        ("n_list", C.c_int64),
        ("n_tiles", C.c_int64),
        ("n_over_16bit", C.c_int64),
        ("wb_slices", C.c_void_p),
        ("wb_waves", C.c_void_p),
        ("wb_ptr", C.c_void_p),
        ("wlist", C.c_void_p),
        ("wt_ptr", C.c_void_p),
        ("wcode", C.c_void_p),
    ]


class ox_cells(C.Structure):
    _fields_ = [
        ("gdim", C.c_int32),
        ("reserved", C.c_int32),
        ("n_cells", C.c_int64),
        ("geom", C.c_void_p),
    ]


class ox_adj(C.Structure):
    _fields_ = [
        ("n_slices", C.c_int32),
        ("nd", C.c_int32),
        ("adj_ptr", C.c_void_p),
        ("adj_cell", C.c_void_p),
        ("adj_loc", C.c_void_p),
    ]


class ox_mesh_info(C.Structure):
    _fields_ = [
        ("gdim", C.c_int32),
        ("tile_bits", C.c_int32),
        ("n_vertices", C.c_int64),
        ("n_cells", C.c_int64),
        ("lo", C.c_double * 3),
        ("span", C.c_double * 3),
        ("coords", C.c_void_p),
        ("cells", C.c_void_p),
        ("cell_perm", C.c_void_p),
        ("cells_struct", ox_cells),
        ("lattice", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ox_pattern_info(C.Structure):
    _fields_ = [
        ("sell", ox_sell),
        ("size", C.c_int64),
        ("nnz", C.c_int64),
        ("n_compressed", C.c_int64),
        ("row_len", C.c_void_p),
        ("n_bins", C.c_int32),
        ("bin_ptr_host", C.c_void_p),
        ("bin_width_host", C.c_void_p),
        ("bin_slices", C.c_void_p),
        ("widths_host", C.c_void_p),
        ("n_row_blocks", C.c_int32),
        ("reserved_rb", C.c_int32),
        ("row_blk_ptr", C.c_void_p),
        ("row_blk_entries", C.c_int64),
    ]


class ox_space_info(C.Structure):
    _fields_ = [
        ("degree", C.c_int32),
        ("nd", C.c_int32),
        ("pw", C.c_int32),
        ("gdim", C.c_int32),
        ("n_dofs", C.c_int64),
        ("n_edges", C.c_int64),
        ("n_pairs", C.c_int64),
        ("cell_dofs", C.c_void_p),
        ("x", C.c_void_p),
        ("rank_initial", C.c_void_p),
        ("edge_keys", C.c_void_p),
        ("adj", ox_adj),
        ("adj_pos", C.c_void_p),
        ("pair_start", C.c_void_p),
        ("pattern", ox_pattern_info),
        ("n_faces", C.c_int64),
        ("face_keys", C.c_void_p),
    ]


class ox_rect_info(C.Structure):
    _fields_ = [
        ("pw", C.c_int32),
        ("pos", C.c_void_p),
        ("pattern", ox_pattern_info),
    ]


class ox_first_args(C.Structure):
    _fields_ = [
        ("uab", C.c_void_p),
        ("u1", C.c_void_p),
        ("b0", C.c_void_p),
        ("b_first", C.c_void_p),
        ("dt", C.c_double),
        ("nu", C.c_double),
        ("a_u1", C.c_void_p),
        ("nut", C.c_void_p),
    ]


class ox_vandriest(C.Structure):
    _fields_ = [
        ("dist", C.c_void_p),
        ("nearest", C.c_void_p),
        ("wss", C.c_void_p),
        ("u_tau", C.c_double),
        ("nu", C.c_double),
        ("a_plus", C.c_double),
        ("n_facets", C.c_int64),
    ]


class ox_viscosity_args(C.Structure):
    _fields_ = [
        ("model", C.c_int),
        ("degree", C.c_int),
        ("cell_dofs", C.c_void_p),
        ("uab", C.c_void_p),
        ("nut", C.c_void_p),
        ("coefficient", C.c_double),
        ("params", C.POINTER(C.c_double)),
        ("n_params", C.c_int),
        ("damping", C.POINTER(ox_vandriest)),
        ("cs2", C.c_void_p),
        ("cs2_stride", C.c_int64),
        ("n_coef", C.c_int64),
        ("cell_bin", C.c_void_p),
    ]


class ox_mg_level(C.Structure):
    _fields_ = [
        ("A", ox_sell),
        ("P", ox_sell),
        ("R", ox_sell),
        ("dinv", C.c_void_p),
        ("n_rows", C.c_int64),
        ("degree", C.c_int32),
        ("reserved", C.c_int32),
        ("cheb", C.c_double * (2 * MG_MAX_DEGREE)),
    ]


class ox_ksp_result(C.Structure):
    _fields_ = [
        ("reason", C.c_int32 * 4),
        ("its", C.c_int32 * 4),
        ("rnorm", C.c_double * 4),
        ("bnorm", C.c_double * 4),
        ("resumed", C.c_int32 * 4),
    ]


class ox_ksp_options(C.Structure):
    _fields_ = [
        ("rtol", C.c_double),
        ("atol", C.c_double),
        ("divtol", C.c_double),
        ("max_it", C.c_int32),
        ("nonzero_guess", C.c_int32),
        ("check_every", C.c_int32),
        ("max_restarts", C.c_int32),
        ("fold_blocks", C.c_int32),
        ("run_ahead", C.c_int32),
        ("ax0", C.c_void_p),
        ("dinv_code", C.c_void_p),
        ("dinv_dict", C.c_void_p),
        ("n_dinv_dict", C.c_int32),
        ("reserved", C.c_int32),
        ("mg", C.c_void_p),
    ]


TRACER_SCHEMES = {"euler": 0, "rk2": 1, "rk4": 2}  # OX_TRACER_EULER / _RK2 / _RK4
TRACER_MAX_SUBSTEPS = 1024  # OX_TRACER_MAX_SUBSTEPS


class ox_tracer_args(C.Structure):
    _fields_ = [
        ("loc", C.c_void_p),
        ("degree", C.c_int),
        ("gdim", C.c_int),
        ("nc", C.c_int),
        ("cell_dofs", C.c_void_p),
        ("n_cells", C.c_int64),
        ("n_rows", C.c_int64),
        ("cell_inv", C.c_void_p),
        ("n_mesh_cells", C.c_int64),
        ("u_a", C.c_void_p),
        ("u_b", C.c_void_p),
        ("t", C.c_double),
        ("dt", C.c_double),
        ("substeps", C.c_int),
        ("scheme", C.c_int),
        ("use_hint", C.c_int),
        ("tol", C.c_double),
        ("n", C.c_int64),
        ("x", C.c_void_p),
        ("cell", C.c_void_p),
        ("status", C.c_void_p),
        ("age", C.c_void_p),
        ("path", C.c_void_p),
        ("t_exit", C.c_void_p),
    ]


PARTICLE_SCHEMES = {"exp1": 0, "exp2": 1}  # OX_PARTICLE_EXP1 / _EXP2
PARTICLE_DRAG = {"stokes": 0, "schiller_naumann": 1}  # OX_PARTICLE_STOKES / _SCHILLER_NAUMANN


class ox_particle_args(C.Structure):
    _fields_ = [
        ("loc", C.c_void_p),
        ("walls", C.c_void_p),
        ("degree", C.c_int),
        ("gdim", C.c_int),
        ("nc", C.c_int),
        ("cell_dofs", C.c_void_p),
        ("n_cells", C.c_int64),
        ("n_rows", C.c_int64),
        ("cell_inv", C.c_void_p),
        ("n_mesh_cells", C.c_int64),
        ("u_a", C.c_void_p),
        ("u_b", C.c_void_p),
        ("t", C.c_double),
        ("dt", C.c_double),
        ("substeps", C.c_int),
        ("scheme", C.c_int),
        ("drag", C.c_int),
        ("use_hint", C.c_int),
        ("tol", C.c_double),
        ("nu", C.c_double),
        ("g", C.c_double * 3),
        ("periodic", C.c_int * 3),
        ("lo", C.c_double * 3),
        ("hi", C.c_double * 3),
        ("period", C.c_double * 3),
        ("facet_action", C.c_void_p),
        ("n_facets", C.c_int64),
        ("n", C.c_int64),
        ("x", C.c_void_p),
        ("v", C.c_void_p),
        ("cell", C.c_void_p),
        ("status", C.c_void_p),
        ("age", C.c_void_p),
        ("path", C.c_void_p),
        ("t_exit", C.c_void_p),
        ("wraps", C.c_void_p),
        ("facet", C.c_void_p),
        ("xq", C.c_void_p),
        ("tau_p", C.c_void_p),
        ("diam", C.c_void_p),
        ("beta", C.c_void_p),
    ]


class ox_lagrangian_args(C.Structure):
    _fields_ = [
        ("loc", C.c_void_p),
        ("gdim", C.c_int),
        ("first", C.c_int),
        ("n_vertices", C.c_int64),
        ("x", C.c_void_p),
        ("u", C.c_void_p),
        ("u_stride", C.c_int64),
        ("hint", C.c_void_p),
        ("cell_inv", C.c_void_p),
        ("n_mesh_cells", C.c_int64),
        ("cell_verts", C.c_void_p),
        ("n_cells", C.c_int64),
        ("src", C.c_void_p),
        ("delta", C.c_void_p),
        ("f_old", C.c_void_p),
        ("f_new", C.c_void_p),
        ("cs2v", C.c_void_p),
        ("status", C.c_void_p),
        ("h", C.c_double),
        ("time_scale", C.c_double),
        ("cs2_floor", C.c_double),
        ("cs2_max", C.c_double),
        ("cs2_initial", C.c_double),
        ("tol", C.c_double),
        ("periodic", C.c_int * 3),
        ("lo", C.c_double * 3),
        ("hi", C.c_double * 3),
        ("period", C.c_double * 3),
    ]


class ox_buoy_term(C.Structure):
    _fields_ = [
        ("c1", C.c_void_p),
        ("c2", C.c_void_p),
        ("nc", C.c_int32),
        ("col", C.c_int32),
        ("ref", C.c_double),
        ("coef", C.c_double * 3),
    ]


REACT_MAXS, REACT_MAXR = 6, 12  # OX_REACT_MAXS / OX_REACT_MAXR


class ox_react_net(C.Structure):
    _fields_ = [
        ("S", C.c_int32),
        ("R", C.c_int32),
        ("nu", (C.c_double * REACT_MAXR) * REACT_MAXS),
        ("order", (C.c_int32 * REACT_MAXS) * REACT_MAXR),
        ("k", C.c_double * REACT_MAXR),
        ("kdof", C.c_void_p * REACT_MAXR),
        ("arr", C.c_int32 * REACT_MAXR),
        ("Ta", C.c_double * REACT_MAXR),
    ]


class ox_react_species(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("out", C.c_void_p),
        ("out2", C.c_void_p),
        ("held", C.c_void_p),
        ("nc", C.c_int32),
        ("col", C.c_int32),
    ]


class ox_scalar_bc_args(C.Structure):
    _fields_ = [
        ("degree", C.c_int),
        ("nc", C.c_int),
        ("robin", C.c_int),
        ("adv", C.c_int),
        ("n_rows", C.c_int64),
        ("rows", C.c_void_p),
        ("row_ptr", C.c_void_p),
        ("pair_facet", C.c_void_p),
        ("pair_loc", C.c_void_p),
        ("pair_off", C.c_void_p),
        ("n_facets", C.c_int64),
        ("facet_rec", C.c_void_p),
        ("q", C.c_void_p),
        ("h", C.c_void_p),
        ("c_inf", C.c_void_p),
        ("beta", C.c_void_p),
        ("uab", C.c_void_p),
        ("c1", C.c_void_p),
        ("a_vals", C.c_void_p),
        ("a_size", C.c_int64),
        ("b", C.c_void_p),
        ("n_dofs", C.c_int64),
    ]


PROF_TAG_BUOYANCY_ROWS = 190  # OX_TAG_BUOYANCY_ROWS of csrc/ox_kernels.h (ox_profile_get: key = 2 x terms + dictionary)
PROF_TAG_SCALAR_ROWS_CELLVISC = 192  # OX_TAG_SCALAR_ROWS_CELLVISC (ox_profile_get: key = columns)
PROF_TAG_SCALAR_ROWS_SUPG = 193  # OX_TAG_SCALAR_ROWS_SUPG (ox_profile_get: key = columns)
PROF_TAG_SUPG_CELLS = 194  # OX_TAG_SUPG_CELLS (ox_profile_get: key = cells)
PROF_TAG_SCALAR_BOUNDARY = 183  # OX_TAG_SCALAR_BOUNDARY, beside OX_TAG_OUTLET_BACKFLOW = 182 (ox_profile_get: key = rows)

_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_D = C.c_double

# name -> (restype, argtypes); the complete export list of include/oasisx_hip.h
SIGNATURES = {
    "ox_version": (_I, []),
    "ox_last_error": (C.c_char_p, []),
    "ox_sell_kv": (_I, []),
    "ox_device_info": (_I, [C.POINTER(_I), C.c_char_p, _I]),
    "ox_mesh_create": (_I, [_P, _L, _P, _L, _I, _I, _I, C.POINTER(_P)]),
    "ox_mesh_view": (_I, [_P, C.POINTER(ox_mesh_info)]),
    "ox_mesh_create_periodic": (_I, [_P, _L, _P, _P, _L, _L, _I, _I, _I, C.POINTER(_D), C.POINTER(_P)]),
    "ox_mesh_destroy": (_I, [_P]),
    "ox_space_create": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "ox_space_create_ordered": (_I, [_P, _I, _I, _I, C.POINTER(_P)]),
    "ox_mesh_create_sub": (_I, [_P, _L, _P, _L, _I, _I, C.POINTER(_D), C.POINTER(_D), _I, _I, _L, C.POINTER(_P)]),
    "ox_space_create_part": (_I, [_P, _I, _I, _P, _L, _I, _L, C.POINTER(_P)]),
    "ox_space_view": (_I, [_P, C.POINTER(ox_space_info)]),
    "ox_space_windows": (_I, [_P, C.POINTER(ox_window_info)]),
    "ox_space_windows_split": (_I, [_P, _I, C.POINTER(ox_window_info)]),
    "ox_space_destroy": (_I, [_P]),
    "ox_rect_create": (_I, [_P, _P, C.POINTER(_P)]),
    "ox_rect_view": (_I, [_P, C.POINTER(ox_rect_info)]),
    "ox_rect_destroy": (_I, [_P]),
    "ox_value_dictionary": (_I, [_P, _L, _I, _P, _P, C.POINTER(_I), _P]),
    "ox_pair_stream_size": (_I, [C.POINTER(ox_sell), _P, _P, C.POINTER(_L), _P]),
    "ox_pair_stream_fill": (_I, [C.POINTER(ox_sell), _P, _P, _P, _P, C.POINTER(_L), _P]),
    "ox_gather_images": (_I, [_P, _L, _P, _L, _I, _P, _P]),
    "ox_malloc": (_I, [C.c_size_t, C.POINTER(_P)]),
    "ox_free": (_I, [_P]),
    "ox_memset": (_I, [_P, _I, C.c_size_t, _P]),
    "ox_synchronize": (_I, [_P]),
    "ox_spmv": (_I, [C.POINTER(ox_sell), _P, _P, _I, _P, _P]),
    "ox_sell_compress_cols": (_I, [C.POINTER(ox_sell), _P, _P, C.POINTER(_L), _P]),
    "ox_spmv_multi": (_I, [_I, _I, C.POINTER(ox_sell), _P, _P, _D, _P, _P, _P]),
    "ox_assemble_rect": (_I, [_I, _I, _I, C.POINTER(ox_cells), C.POINTER(ox_adj), _P, _I, C.POINTER(ox_sell), _P]),
    "ox_axpby": (_I, [_L, _D, _P, _D, _P, _P, _P]),
    "ox_dot": (_I, [_L, _I, _P, _P, C.POINTER(_D), _P, _P]),
    "ox_set_bc": (_I, [_P, _P, _P, _L, _I, _I, _P]),
    "ox_scatter_add": (_I, [_P, _P, _P, _L, _I, _I, _D, _P]),
    "ox_zero_rows": (_I, [C.POINTER(ox_sell), _P, _L, _D, _P]),
    "ox_zero_rows_au": (_I, [C.POINTER(ox_sell), _P, _L, _D, _P, _P, _I, _P]),
    "ox_zero_rows_cols": (_I, [C.POINTER(ox_sell), _P, _D, _P]),
    "ox_assemble_matrix": (_I, [_I, C.POINTER(ox_cells), C.POINTER(ox_space_info), C.POINTER(ox_sell), _I, _P]),
    "ox_assemble_weights": (_I, [_I, C.POINTER(ox_cells), C.POINTER(ox_adj), _L, _P, _P]),
    "ox_assemble_load_vector": (_I, [C.POINTER(ox_cells), C.POINTER(ox_adj), _L, _I, _I, _P, _P, _P, _P]),
    "ox_assemble_first": (_I, [C.POINTER(ox_cells), C.POINTER(ox_space_info), C.POINTER(ox_sell), C.POINTER(ox_sell),
                               C.POINTER(ox_sell), C.POINTER(ox_first_args), _I, _P]),
    "ox_cell_viscosity": (_I, [C.POINTER(ox_cells), C.POINTER(ox_viscosity_args), _P]),
    "ox_dynamic_cells": (_I, [_I, C.POINTER(ox_cells), _P, _P, _P, _P]),
    "ox_dynamic_vertices": (_I, [_I, _L, _P, _P, _L, _P, _P, _P]),
    "ox_dynamic_products": (_I, [_I, _L, _P, _L, _P, _P, _D, _P, _P]),
    "ox_dynamic_bin_sums": (_I, [_L, _P, _P, _L, _P, _P, _L, _P, _P]),
    "ox_dynamic_bin_coefficients": (_I, [_L, _P, _P, _D, _P, _P]),
    "ox_patch_filter_vertices": (_I, [_I, _L, _P, _P, _L, _L, _P, _P, _L, _P, _P]),
    "ox_patch_filter_cells": (_I, [_I, _I, _L, _P, _L, _P, _P, _P]),
    "ox_dynamic_clip": (_I, [_L, _P, _D, _P, _P]),
    "ox_assemble_stress_transpose": (_I, [_I, C.POINTER(ox_cells), _P, C.POINTER(ox_adj), _L, _P, _P, _D, _P, _P]),
    "ox_flow_cells": (_I, [_I, C.POINTER(ox_cells), _P, _P, _P, _D, _D, _P, _P, _P, _P]),
    "ox_flow_reduce": (_I, [_L, _P, _P, _L, _L, _P]),
    "ox_stats_accumulate": (_I, [_I, _L, _P, _L, _D, _D, _P, _P, _P]),
    "ox_profile_cells": (_I, [_I, C.POINTER(ox_cells), _P, _I, _I, C.POINTER(_P), C.POINTER(_L), _P, _P, _L, _P, _P, _P]),
    "ox_profile_update": (_I, [_I, _L, _P, _P, _P, _D, _D, _I, _P, _P, _P, _P, _P]),
    "ox_assemble_grad_vector": (_I, [_I, _I, _I, C.POINTER(ox_cells), _P, C.POINTER(ox_adj), _L, _P,
                                     _P, _D, _P, _P]),
    "ox_assemble_div_vector": (_I, [_I, _I, C.POINTER(ox_cells), _P, C.POINTER(ox_adj), _L, _P, _D,
                                    _P, _P]),
    "ox_dg1_grad_rhs": (_I, [_I, C.POINTER(ox_cells), _P, _P, _P, _P]),
    "ox_dg1_mass": (_I, [_I, C.POINTER(ox_cells), _I, _P, _P, _P]),
    "ox_jacobi_setup": (_I, [C.POINTER(ox_sell), _P, _P]),
    "ox_ksp_work_bytes": (C.c_size_t, [_L, _L, _I, _I]),
    "ox_remove_mean": (_I, [_L, _L, _P, _P, _D, _P, _P]),
    "ox_window_retile": (_I, [C.POINTER(ox_sell), _P, _P, _I, _P, _P]),
    "ox_ksp_default_fold_blocks": (_I, []),
    "ox_ksp_kernels_per_iteration": (_I, [_I, C.POINTER(ox_sell), _I, _I, _I, _I]),
    "ox_ksp_options_default": (_I, [C.POINTER(ox_ksp_options)]),
    "ox_ksp_solve": (_I, [_I, C.POINTER(ox_sell), _P, _P, _P, _I, C.POINTER(ox_ksp_options), _P, C.c_size_t,
                          C.POINTER(ox_ksp_result), _P, _P]),
    "ox_ksp_work_bytes_for": (C.c_size_t, [C.POINTER(ox_sell), _I, _I]),
    "ox_mg_create": (_I, [_I, C.POINTER(ox_mg_level), _P, _I, C.POINTER(_P)]),
    "ox_mg_destroy": (_I, [_P]),
    "ox_mg_apply": (_I, [_P, _P, _P, _P]),
    "ox_mg_kernels_per_cycle": (_I, [_P]),
    "ox_guess_create": (_I, [_L, _L, _I, _I, _I, C.POINTER(_P)]),
    "ox_guess_destroy": (_I, [_P]),
    "ox_guess_reset": (_I, [_P]),
    "ox_guess_dim": (_I, [_P]),
    "ox_guess_bytes": (C.c_size_t, [_P]),
    "ox_guess_form": (_I, [_P, C.POINTER(ox_sell), _P, _P, _I, _P, C.POINTER(_P), _P, _P]),
    "ox_guess_update": (_I, [_P, C.POINTER(ox_sell), _P, _P, _P]),
    "ox_locator_create": (_I, [_I, _P, _L, _P, _L, _P, _L, _D, _D, _P, C.POINTER(_P)]),
    "ox_locator_destroy": (_I, [_P]),
    "ox_locator_info": (_I, [_P, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L), C.POINTER(_I)]),
    "ox_locator_find": (_I, [_P, _L, _P, _D, _P, _P, _P]),
    "ox_locator_bary": (_I, [_P, _L, _P, _P, _P, _P]),
    "ox_eval_points": (_I, [_I, _I, _P, _L, _L, _L, _P, _P, _P, _P, _I, _I, _P, _L, _L, _P]),
    "ox_probe_sample": (_I, [_I, _I, _P, _L, _L, _L, _P, _P, _P, _P, _I, _I, _P, _L, _L, _L, _L, _P]),
    "ox_tracer_advance": (_I, [C.POINTER(ox_tracer_args), _P]),
    "ox_particle_advance": (_I, [C.POINTER(ox_particle_args), _P]),
    "ox_dynamic_lagrangian": (_I, [C.POINTER(ox_lagrangian_args), _P]),
    "ox_walldist_create": (_I, [_I, _P, _L, C.POINTER(_I), _P, C.POINTER(_P)]),
    "ox_walldist_destroy": (_I, [_P]),
    "ox_walldist_info": (_I, [_P, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L), C.POINTER(_I)]),
    "ox_walldist_query": (_I, [_P, _L, _P, C.POINTER(_D), _I, _P, _P, _P]),
    "ox_scalar_rows": (_I, [C.POINTER(ox_sell), C.POINTER(ox_sell), C.POINTER(ox_sell), C.POINTER(ox_sell), _D, _D, _I,
                            _P, _P, _P, _P, _P]),
    "ox_scalar_rows_cellvisc": (_I, [C.POINTER(ox_cells), C.POINTER(ox_space_info), C.POINTER(ox_sell), C.POINTER(ox_sell),
                                     C.POINTER(ox_sell), C.POINTER(ox_sell), _P, _D, _D, _D, _I, _P, _P, _P, _P, _I, _P]),
    "ox_supg_cells": (_I, [_I, C.POINTER(ox_cells), _P, _P, _P, _D, _D, _D, _D, _I, _P, _P]),
    "ox_scalar_rows_supg": (_I, [C.POINTER(ox_cells), C.POINTER(ox_space_info), C.POINTER(ox_sell), C.POINTER(ox_sell),
                                 C.POINTER(ox_sell), C.POINTER(ox_sell), _P, _P, _D, _D, _D, _I, _P, _P, _P, _P, _P, _I, _P]),
    "ox_buoyancy_rows": (_I, [C.POINTER(ox_sell), _I, _I, C.POINTER(ox_buoy_term), _P, _P]),
    "ox_scalar_react": (_I, [C.POINTER(ox_react_net), C.POINTER(ox_react_species), _L, _D, _I, _P]),
    "ox_reaction_rates": (_I, [C.POINTER(ox_react_net), C.POINTER(ox_react_species), _L, _P, _P]),
    "ox_scalar_flux": (_I, [_I, C.POINTER(ox_cells), _P, _L, _P, _P, _I, _I, _D, _D, _P, _P, _P, _P, _P]),
    "ox_scalar_flux_cells": (_I, [_I, C.POINTER(ox_cells), _P, _L, _P, _P, _I, _I, _D, _P, _D, _D, _P, _P, _P, _P, _P]),
    "ox_wall_stress": (_I, [_I, _I, C.POINTER(ox_cells), _P, _P, _L, _P, _P, _P, _P, _D, _D, _P, _P, _P, _P, _P, _P, _P]),
    "ox_wall_forces": (_I, [_I, _I, _P, _P, _D, _P, _L, _L, _P]),
    "ox_scalar_boundary": (_I, [C.POINTER(ox_cells), _P, C.POINTER(ox_scalar_bc_args), _P]),
    "ox_outlet_flux": (_I, [_I, C.POINTER(ox_cells), _P, _L, _P, _P, _P, _P]),
    "ox_outlet_update": (_I, [_I, _P, _P, _P, _L, _L, _P, _D, _P, _P, _P, _P, _P, _L, _P]),
    "ox_outlet_backflow": (_I, [_I, C.POINTER(ox_cells), _P, _L, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P, _P]),
    "ox_drag_sigma": (_I, [_I, C.POINTER(ox_cells), _P, _L, _P, _P, _P, _P, _P, _P, _P]),
    "ox_drag_rows": (_I, [C.POINTER(ox_cells), C.POINTER(ox_space_info), C.POINTER(ox_sell), _L, _P, _I, _P, _D, _P, _P, _P]),
    "ox_drag_force_cells": (_I, [_I, C.POINTER(ox_cells), _P, _L, _P, _P, _P, _P, _P, _P]),
    "ox_profile_begin": (_I, [_I, _I]),
    "ox_profile_end": (_I, []),
    "ox_profile_get": (_I, [_I, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(_D)]),
    "ox_range_push": (_I, [C.c_char_p]),
    "ox_range_pop": (_I, []),
    "ox_comm_unique_id": (_I, [C.c_char_p]),
    "ox_comm_create": (_I, [C.c_char_p, _I, _I, C.POINTER(_P)]),
    "ox_comm_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "ox_comm_destroy": (_I, [_P]),
    "ox_dist_create": (_I, [_P, _I, _I, _I, C.POINTER(C.c_int32), C.POINTER(_L), _P,
                            C.POINTER(_L), _L, _L, C.POINTER(_P)]),
    "ox_p2p_window_bytes": (C.c_size_t, [_I, _L]),
    "ox_p2p_window_create": (_I, [C.c_size_t, C.POINTER(_P), C.c_char_p]),
    "ox_p2p_window_open": (_I, [C.c_char_p, C.POINTER(_P)]),
    "ox_p2p_window_close": (_I, [_P]),
    "ox_p2p_window_free": (_I, [_P]),
    "ox_dist_enable_p2p": (_I, [_P, _P, C.POINTER(_P), C.POINTER(_L), C.POINTER(_L), _D]),
    "ox_dist_p2p_timeout": (_I, [_P, _D]),
    "ox_dist_disable_p2p": (_I, [_P]),
    "ox_dist_set_overlap": (_I, [_P, _I]),
    "ox_dist_set_p2p_release": (_I, [_P, _I]),
    "ox_dist_status": (_I, [_P]),
    "ox_dist_create_custom": (_I, [_I, _I, _I, C.POINTER(C.c_int32), C.POINTER(_L), _P, C.POINTER(_L), _L, _L,
                                   _P, _P, _P, C.POINTER(_P)]),
    "ox_memcpy": (_I, [_P, _P, C.c_size_t, _I, _P]),
    "ox_dist_destroy": (_I, [_P]),
    "ox_halo_forward": (_I, [_P, _P, _I, _P]),
    "ox_allreduce_sum": (_I, [_P, _P, _I, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OasisxHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  oasisx_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ox_last_error().decode(errors="replace")
        raise OasisxHipError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device (or host) address of a torch tensor / None."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def current_stream():
    """hipStream_t of torch's current stream on the current device (0 on CPU)."""
    import torch

    if torch.cuda.is_available():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(0)
