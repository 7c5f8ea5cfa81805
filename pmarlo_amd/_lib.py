"""ctypes binding of libmsmhip.so (include/msmhip.h).

The library is loaded from ``pmarlo_amd/csrc/libmsmhip.so`` only; there is no
CPU fallback.  If the shared object is missing, or a GPU call fails, the error
is raised -- a silent fallback would void every parity claim.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

__all__ = ["lib", "load", "LIB_PATH", "check", "MsmError", "DECLARED_SYMBOLS"]

LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libmsmhip.so"

MSM_OK, MSM_ERR_INVALID, MSM_ERR_HIP, MSM_ERR_NOMEM, MSM_ERR_UNSUPPORTED, MSM_ERR_NOCONV = range(6)
MSM_F32, MSM_F64 = 0, 1
# msm_featurize_spec (MSM_FEAT_*, MSM_MIC_* in include/msmhip.h): record kinds, record flags, minimum-image rules
FEAT_DISTANCE, FEAT_ANGLE, FEAT_DIHEDRAL, FEAT_CONTACT = range(4)
FEAT_MIC, FEAT_COSSIN = 1, 2
MIC_ROUND, MIC_SEARCH = 0, 1
# launch thresholds of msm_superpose (MSM_SUPERPOSE_* in include/msmhip.h)
SUPERPOSE_TILE_FRAMES, SUPERPOSE_TILE_FLOATS, SUPERPOSE_LDS_ATOMS, SUPERPOSE_NARROW_SEL = 64, 12288, 4096, 64
# representative frames (MSM_REP_* in include/msmhip.h): widest feature row, frames per grouping chunk, the
# i- and j-tiles of the all-pairs medoid pass, weight flags, score and selection modes
REP_MAX_D, REP_GROUP_CHUNK, REP_TILE_I, REP_TILE_J = 256, 1024, 128, 64
REP_FLAG_NONFINITE, REP_FLAG_NEGATIVE, REP_FLAG_NONPOSITIVE_SUM = 1, 2, 4
REP_SCORE_CENTROID, REP_SCORE_MEDOID = 0, 1
REP_SELECT_SMALLEST, REP_SELECT_DIVERSE = 0, 1
# silhouette samples (MSM_SIL_* in include/msmhip.h): members of a segment, query frames of a workgroup
SIL_SEG_LEN, SIL_TILE_I = 1024, 128
# trajectory bootstrap (MSM_COMBINE_MAX_SEG, MSM_FLUX_LDS_MAX_N in include/msmhip.h)
COMBINE_MAX_SEG, FLUX_LDS_MAX_N = 32, 127
# reactive pathways (MSM_PATHWAYS_* in include/msmhip.h): most states, the status words of the resumable entry
PATHWAYS_MAX_N = 2048
PATHWAYS_RUNNING, PATHWAYS_FRACTION, PATHWAYS_NO_PATH, PATHWAYS_MAXITER = range(4)
# effective counts (MSM_EFF_* in include/msmhip.h): lags of a block, blocks a launch takes by default, averages
EFF_LAG_BLOCK, EFF_BLOCKS_PER_LAUNCH = 256, 8
EFF_AVERAGE_ROW, EFF_AVERAGE_ALL, EFF_AVERAGE_NONE = range(3)
# count dispatch (MSM_COUNT_PATH_* in include/msmhip.h), the largest k msm_state_counts bins in the LDS
# (MSM_STATE_COUNTS_LDS_MAX_K), frames per block sum of the k-means++ draw (MSM_KPP_BLOCK)
COUNT_PATH_BUCKET, COUNT_PATH_PRIVATISED, COUNT_PATH_GLOBAL, COUNT_PATH_NONE = range(4)
STATE_COUNTS_LDS_MAX_K, KPP_BLOCK = 16384, 1024
# msm_mlp_forward's envelope: widest layer, most outputs, most Linear layers
MLP_MAX_WIDTH, MLP_MAX_OUT, MLP_MAX_LINEAR = 256, 64, 8
# msm_vamp2_loss's stats block (MSM_VAMP2_STATS): 16 scalars, then var_z0, var_zt, mean_z0, mean_zt of 64 entries
VAMP2_STATS = 16 + 4 * MLP_MAX_OUT
# msm_mlp_launch_plan: the kernel codes (MSM_MLP_KERNEL_*) and the slots per partial sum (MSM_MLP_CHUNK)
MLP_KERNELS = {"forward": 0, "vjp": 1, "train_forward": 2, "train_backward": 3}
MLP_CHUNK = 256
# MBAR (MSM_MBAR_* in include/msmhip.h): most sampled states, frames of a workgroup trip, the status bits
MBAR_MAX_K, MBAR_THREADS = 64, 256
MBAR_BAD_INPUT, MBAR_BAD_FRAME = 1, 2
# TRAM (MSM_TRAM_* in include/msmhip.h): most Markov states, frames of a pass segment, the modes of msm_tram_rows
TRAM_MAX_STATES, TRAM_SEGMENT = 2048, 256
TRAM_ROWS_MULTIPLIERS, TRAM_ROWS_COUNTS = 0, 1
# HMM (MSM_HMM_* in include/msmhip.h): most hidden states, steps of a chunk, the fixed point's iteration cap, status bits
HMM_MAX_HIDDEN, HMM_CHUNK, HMM_MAX_FIXED_POINT = 16, 64, 1_000_000
HMM_BAD_SYMBOL, HMM_ZERO_PROB, HMM_EMPTY_STATE, HMM_BAD_TABLE, HMM_NOT_CONVERGED = 1, 2, 4, 8, 16
# metadynamics (MSM_METAD_* in include/msmhip.h): most CVs of a hill and of a grid, frames of a workgroup trip, hills of
# an LDS tile, grid points of a scan tile, the hill kernels
METAD_MAX_D, METAD_GRID_MAX_D, METAD_THREADS, METAD_TILE, METAD_SCAN_TILE = 8, 3, 256, 128, 256
METAD_KERNELS = {"gaussian": 0, "stretched-gaussian": 1}
# OPES (MSM_OPES_* in include/msmhip.h): the parameter vector, the device state, the per-deposit row, status bits, flags
OPES_PARAMS, OPES_PAR_PERIOD, OPES_PAR_SIGMA0 = 6 + 2 * METAD_MAX_D, 6, 6 + METAD_MAX_D
OPES_STATE, OPES_PER_DEPOSIT = 8, 4
(OPES_STATE_COUNT, OPES_STATE_LIVE, OPES_STATE_W, OPES_STATE_W2, OPES_STATE_SUM, OPES_STATE_Z, OPES_STATE_STATUS,
 OPES_STATE_CURSOR) = range(8)
OPES_FULL, OPES_BAD_RECORD, OPES_BAD_STATE = 1, 2, 4
OPES_NO_SKIP = 1
OPES_ALIVE = 2**31 - 1      # death of a version that lives


class MsmError(RuntimeError):
    """A HIP-side failure reported through the C ABI."""


_vp = C.c_void_p
_i32 = C.c_int
_i64 = C.c_int64
_sz = C.c_size_t
_f64 = C.c_double
_pp = C.POINTER(C.c_void_p)

# name -> (restype, argtypes); mirrors include/msmhip.h one to one.
_PROTOTYPES: dict[str, tuple] = {
    "msm_version": (C.c_char_p, []),
    "msm_ctx_create": (_i32, [_i32, _vp, _pp]),
    "msm_ctx_destroy": (None, [_vp]),
    "msm_last_error": (C.c_char_p, [_vp]),
    "msm_device_info": (_i32, [_vp, C.c_char_p, _sz, C.POINTER(_i32), C.POINTER(_sz)]),
    "msm_malloc": (_i32, [_vp, _sz, _pp]),
    "msm_free": (_i32, [_vp, _vp]),
    "msm_memcpy_h2d": (_i32, [_vp, _vp, _vp, _sz]),
    "msm_memcpy_d2h": (_i32, [_vp, _vp, _vp, _sz]),
    "msm_memcpy_d2d": (_i32, [_vp, _vp, _vp, _sz]),
    "msm_memset": (_i32, [_vp, _vp, _i32, _sz]),
    "msm_sync": (_i32, [_vp]),
    "msm_event_create": (_i32, [_vp, _pp]),
    "msm_event_destroy": (None, [_vp]),
    "msm_event_record": (_i32, [_vp, _vp]),
    "msm_event_elapsed_ms": (_i32, [_vp, _vp, C.POINTER(C.c_float)]),
    "msm_graph_begin": (_i32, [_vp]),
    "msm_graph_end": (_i32, [_vp, _pp]),
    "msm_graph_launch": (_i32, [_vp, _vp]),
    "msm_graph_destroy": (None, [_vp]),
    "msm_featurize_distances": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _i32]),
    "msm_featurize_contacts": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, C.c_float, _vp, _i64, _i32]),
    "msm_featurize_rg": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _i32]),
    "msm_featurize_angles": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _i32]),
    "msm_featurize_dihedrals": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _i32]),
    "msm_box_from_cell": (_i32, [_vp, _vp, _i64, _vp]),
    "msm_featurize_spec": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32]),
    "msm_featurize_spec_vjp": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _vp, _vp,
                                      _f64, _vp]),
    "msm_featurize_sasa": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp]),
    "msm_hbond_presence": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, C.c_float, C.c_float, _vp]),
    "msm_dssp": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp]),
    "msm_superpose": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp]),
    "msm_count_transitions": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "msm_count_transitions_normalised": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "msm_count_transitions_weighted": (
        _i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "msm_count_transitions_lagscan": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "msm_count_transitions_plan": (_i32, [_vp, _i32, _i64, _i32, _vp]),
    "msm_state_counts": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "msm_column_moments_partial": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp]),
    "msm_moments_finalize": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "msm_column_moments": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _i32, _vp, _vp, _vp]),
    "msm_column_minmax": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp]),
    "msm_standardise_params": (_i32, [_vp, _vp, _vp, _i32, _f64, _i32, _vp, _vp, _vp]),
    "msm_lagged_moments": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "msm_tica_solve": (_i32, [_vp, _vp, _vp, _i32, _f64, _i32, _vp, _vp, _vp, _vp]),
    "msm_tica_solve_leading": (_i32, [_vp, _vp, _vp, _i32, _f64, _i32, _vp, _vp, _vp, _vp, _i32]),
    "msm_lagged_moments_reversible": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "msm_lagged_moments_onesided": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "msm_onesided_tica_eigenvalues": (_i32, [_vp, _vp, _i32, _f64, _vp]),
    "msm_moments_from_lagged": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "msm_moments_tail": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _f64, _i32, _vp, _vp,
                                _vp, _vp]),
    "msm_project_preset": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _vp, _i32]),
    "msm_project": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _vp]),
    "msm_project_finite": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _vp]),
    "msm_eigh": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "msm_autocorr_lagscan": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _i32, _f64, _vp, _vp]),
    "msm_hstack_f64": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _i32, _i32, _i64, _i64, _vp]),
    "msm_mlp_forward": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _sz,
                               _vp, _i64]),
    "msm_vamp2_workspace": (_sz, [_i64, _i32]),
    "msm_vamp2_loss": (_i32, [_vp, _vp, _vp, _i64, _i32, _i64, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _i64]),
    "msm_mlp_train_workspace": (_sz, [_i64, _i32, _vp, _i32, _i32, _i32]),
    "msm_mlp_loss_grad": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _sz,
                                 _vp, _vp, _i64, _vp, C.c_uint64, C.c_uint64, _f64, _f64, _f64, _f64, _vp, _sz, _vp,
                                 _vp, _vp, _i64]),
    "msm_vamp2_weighted_workspace": (_sz, [_i64, _i32]),
    "msm_vamp2_loss_weighted": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i64, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp,
                                       _i64]),
    "msm_mlp_train_weighted_workspace": (_sz, [_i64, _i32, _vp, _i32, _i32, _i32]),
    "msm_mlp_loss_grad_weighted": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32,
                                          _vp, _sz, _vp, _vp, _vp, _i64, _vp, C.c_uint64, C.c_uint64, _f64, _f64, _f64,
                                          _f64, _vp, _sz, _vp, _vp, _vp, _i64]),
    "msm_mlp_launch_plan": (_i32, [_vp, _i32, _i32, _i64, _i32, _vp, _i32, _i32, _i32, _vp]),
    "msm_adamw_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _f64, _f64, _f64, _f64, _f64, _f64, _vp]),
    "msm_mlp_vjp_workspace": (_sz, [_i64, _i32, _vp, _i32, _i32, _i32]),
    "msm_mlp_vjp": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _i64,
                           _f64, _vp, _vp, _i64, _vp, _i64, _vp, _sz]),
    "msm_bias_workspace": (_sz, [_i64, _i32, _i32, _vp, _i32, _i32, _i32]),
    "msm_bias_energy_forces": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp,
                                      _i32, _i32, _i32, _i32, _vp, _sz, _f64, _vp, _sz, _vp, _vp, _i64, _vp]),
    "msm_kmeans_assign": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "msm_kmeans_fit": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, C.c_uint64, _i32, _i32, _f64, _vp, _vp]),
    "msm_kmeans_fit_begin": (
        _i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, C.c_uint64, _i32, _f64, _f64, _vp, _vp, _i32]),
    "msm_kmeans_fit_begin_clear": (
        _i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, C.c_uint64, _i32, _f64, _f64, _vp, _vp, _i32, _vp, _vp]),
    "msm_kmeans_accumulate": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "msm_kmeans_update": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32]),
    "msm_comm_unique_id": (_i32, [_vp, _sz]),
    "msm_comm_init": (_i32, [_vp, _i32, _i32, _vp, _sz, _pp]),
    "msm_comm_destroy": (None, [_vp]),
    "msm_comm_info": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(C.c_uint64)]),
    "msm_allreduce_i64": (_i32, [_vp, _vp, _sz]),
    "msm_allreduce_i64_from": (_i32, [_vp, _vp, _vp, _sz]),
    "msm_allreduce_f64": (_i32, [_vp, _vp, _sz]),
    "msm_allreduce_min_f64": (_i32, [_vp, _vp, _sz]),
    "msm_allreduce_max_f64": (_i32, [_vp, _vp, _sz]),
    "msm_broadcast": (_i32, [_vp, _vp, _sz, _i32]),
    "msm_rcp_f64": (_i32, [_vp, _vp, _sz, _vp]),
    "msm_kmeans_image_bytes": (_i32, [_i64, _i32, C.POINTER(_sz)]),
    "msm_kmeans_pack": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp]),
    "msm_kmeans_pack_bounded": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    "msm_kmeans_assign_packed": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "msm_kmeans_accumulate_packed": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "msm_kmeans_lloyd_pass": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "msm_kmeans_accumulate_delta": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp]),
    "msm_kmeans_lloyd_pass_from": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _i32]),
    "msm_kmeans_accumulate_delta_from": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                                _vp, _i32]),
    "msm_kmeans_lloyd_pass_deferred": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(_i32)]),
    "msm_kmeans_assign_closing": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _i32, _vp, _vp, C.POINTER(_i32)]),
    "msm_kmeans_filter_scanned": (_i32, [_vp, C.POINTER(C.c_uint64), _i32]),
    "msm_kmeans_init_plusplus": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, C.c_uint64, _f64, _vp, _vp, _vp]),
    "msm_mfma_bf16_probe": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "msm_mfma_f16_probe": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "msm_run_lengths": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    "msm_sum_f64": (_i32, [_vp, _vp, _i64, _vp]),
    "msm_transition_matrix": (_i32, [_vp, _vp, _i32, _i32, _i32, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "msm_embed_full": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "msm_spectrum_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "msm_spectrum": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _i32, _vp, _vp, _vp,
                            _i64, _vp, _vp, _i32, _vp, _vp, _vp, _f64, _vp, _i32]),
    "msm_matrix_power": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "msm_spectrum_powered": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _i32, _vp, _vp,
                                    _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _f64, _vp, _i32]),
    "msm_sample_transition_matrices": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _f64, C.c_uint64, _i32, _i32, _vp, _i64,
                                              _i32]),
    "msm_sample_reversible_transition_matrices": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, C.c_uint64, _i32, _i32, _i32,
                                                         _vp, _i64, _i32, _vp]),
    "msm_active_counts": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _f64, _vp]),
    "msm_reversible_mle": (_i32, [_vp, _vp, _i32, _i32, _f64, _i32, _vp, _i32, _vp, _vp, _vp]),
    "msm_reversible_mle_batched_lds_max_n": (_i32, []),
    "msm_reversible_mle_batched_scratch_bytes": (_sz, [_i32, _i32]),
    "msm_reversible_mle_batched": (_i32, [_vp, _vp, _i32, _i32, _f64, _f64, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _vp,
                                          _vp]),
    "msm_kis_scores": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "msm_philox4x32": (_i32, [_vp, C.c_uint64, _vp, _vp]),
    "msm_gemm_f64": (_i32, [_vp, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _i64]),
    "msm_diff_norms": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "msm_gather_f64": (_i32, [_vp, _vp, _i32, _vp, _i64, _vp]),
    "msm_clip_or_wrap": (_i32, [_vp, _vp, _i64, _i64, _f64, _f64, _i32, _vp]),
    "msm_order_statistics": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _vp]),
    "msm_weighted_stats": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "msm_hist2d": (_i32, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _f64, _vp, _i32, _vp, _i32, _vp]),
    "msm_smooth_sparse_bins": (_i32, [_vp, _vp, _i32, _i32, _f64, _vp, _vp]),
    "msm_scale_to_total": (_i32, [_vp, _vp, _i32, _f64]),
    "msm_fes_finalize": (_i32, [_vp, _vp, _i32, _f64, _vp, _vp]),
    "msm_kde2d": (_i32, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _f64, _vp, _i32, _vp, _i32, _f64, _f64, _i32, _vp]),
    "msm_solve_f64": (_i32, [_vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
    "msm_reactive_flux": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "msm_lump_macro": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _vp, _vp]),
    "msm_macro_mfpt": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "msm_reactive_pathways_work_bytes": (_sz, [_i32]),
    "msm_reactive_pathways_launch_paths": (_i32, [_i32]),
    "msm_reactive_pathways_begin": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "msm_reactive_pathways_run": (_i32, [_vp, _vp, _i32, _f64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "msm_effective_counts_work_bytes": (_sz, [_i64, _i32, _i32]),
    "msm_effective_counts": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f64, _i32, _vp, _sz, _vp, _vp, _vp,
                                    _vp, C.POINTER(_i64)]),
    "msm_combine_counts": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i64, _vp, _i32]),
    "msm_row_normalise_batched": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "msm_reactive_flux_batched_scratch_bytes": (_sz, [_i32, _i32, _i32]),
    "msm_reactive_flux_batched": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "msm_silhouette": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _i32, _vp, _vp]),
    "msm_silhouette_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "msm_silhouette_samples": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _i32, _vp, _sz, _i64, _vp, _vp]),
    "msm_grid_cells": (_i32, [_vp, _vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp]),
    "msm_first_occurrence": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "msm_relabel": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp]),
    "msm_ck_test": (_i32, [_vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _vp]),
    "msm_group_by_label": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "msm_state_centroids": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "msm_state_scores": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "msm_state_select": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "msm_mbar_plan": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp]),
    "msm_mbar_pass": (_i32, [_vp, _vp, _i32, _i32, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "msm_mbar_state_means": (_i32, [_vp, _vp, _i32, _i32, _i64, _i64, _vp, _vp]),
    "msm_mbar_newton_system": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "msm_mbar_weights": (_i32, [_vp, _vp, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "msm_mbar_reduced_potentials": (_i32, [_vp, _vp, _vp, _i64, _vp, _i32, _i64, _i64, _vp]),
    "msm_tram_plan": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp]),
    "msm_tram_rows": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "msm_tram_pass": (_i32, [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "msm_tram_update": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "msm_tram_iterations": (_i32, [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _i32, _i32, _vp, _vp, _vp]),
    "msm_tram_transition_matrices": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "msm_hmm_workspace_bytes": (_sz, [_i32, _i64, _i32, _i64]),
    "msm_hmm_plan": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp]),
    "msm_hmm_estep": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                             _vp, _vp, _vp, _vp]),
    "msm_hmm_emissions": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "msm_hmm_mstep": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _f64, _vp, _vp, _vp, _vp, _vp]),
    "msm_hmm_viterbi_workspace_bytes": (_sz, [_i32, _i32, _i64, _i32]),
    "msm_hmm_viterbi": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                               _vp]),
    "msm_hmm_iterations": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32,
                                  _i32, _i32, _f64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp]),
    "msm_metad_plan": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp]),
    "msm_metad_bias": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _f64, _vp, _i32, _vp, _vp, _i64]),
    "msm_metad_grid_scan": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _f64, _vp, _i32, _f64, _f64, _i32,
                                   _vp, _vp]),
    "msm_metad_append": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _f64]),
    "msm_opes_plan": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp]),
    "msm_opes_deposit": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i64, _i32, _i32]),
    "msm_opes_bias": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp,
                             _i64]),
}

DECLARED_SYMBOLS = tuple(_PROTOTYPES)

_lib = None


def load() -> C.CDLL:
    """Load libmsmhip.so and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m pmarlo_amd.csrc.build` "
            "(hipcc, gfx950).  pmarlo_amd has no CPU fallback."
        )
    handle = C.CDLL(str(LIB_PATH))
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(handle, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return handle


class _LazyLib:
    def __getattr__(self, name):
        return getattr(load(), name)


lib = _LazyLib()

_EXC = {
    MSM_ERR_INVALID: ValueError,
    MSM_ERR_HIP: MsmError,
    MSM_ERR_NOMEM: MemoryError,
    MSM_ERR_UNSUPPORTED: NotImplementedError,
    MSM_ERR_NOCONV: MsmError,
}


def check(status: int, ctx_handle=None) -> None:
    """Map an msm_status to the Python exception the reference would raise."""
    if status == MSM_OK:
        return
    msg = ""
    if ctx_handle:
        raw = load().msm_last_error(ctx_handle)
        msg = raw.decode("utf-8", "replace") if raw else ""
    exc = _EXC.get(status, MsmError)
    raise exc(msg or f"libmsmhip call failed with status {status}")
