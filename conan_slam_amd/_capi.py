"""ctypes binding of libcslam_hip.so -- exactly the entry points include/cslam.h declares.

The library is loaded from conan_slam_amd/lib/ (in-tree).  If it is missing or cannot be loaded this
module raises: the engine has no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcslam_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "cslam.h")

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_HIP, ERR_NO_DEVICE, ERR_ALLOC = 0, 1, 2, 3, 4, 5
FACTOR_OK, FACTOR_FALLBACK, FACTOR_ZEROED, FACTOR_SKIPPED, FACTOR_BAD_IDF, FACTOR_INTERNAL = 0, 1, 2, 4, 8, 16
FACTOR_HEADING_SKIPPED = 32  # batched engine only: a heading step with P22 + R <= 0 was skipped for that instance
F32, F64 = 0, 1
Q_LOWER_CHOL_GAIN, Q_PREDICT_NM4, Q_REF_EXACT, Q_TEXTBOOK = 1, 2, 3, 0
STAGE_GATHER, STAGE_FACTOR, STAGE_GAIN, STAGE_DOWNDATE, N_STAGES = 0, 1, 2, 3, 4
STAGE_NAMES = ["gather", "factor", "gain", "downdate"]


class CslamError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"cslam status {code}: {msg}")
        self.code = code


# The batched engine's Monte-Carlo entry points (declared in include/cslam.h, found by declared_symbols like every other):
# per-instance controls and the pose read of every instance.
BATCH_MC_SYMBOLS = ("cslam_ekf_batch_predict_each", "cslam_ekf_batch_get_poses")

# The landmark reads (means and marginal covariance blocks without applying the pending downdate), with their prototypes.
LANDMARK_SYMBOLS = ("cslam_ekf_get_landmarks", "cslam_ekf_batch_get_landmarks")
_PROTOTYPES = {
    "cslam_ekf_get_landmarks": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "cslam_ekf_batch_get_landmarks": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    # launches of the look-ahead windows' rows kernel (zero where the row-major panel mirror serves the blocks kernel)
    "cslam_ekf_rows_launches": [C.c_void_p, C.POINTER(C.c_longlong)],
    # whole tiles and strips of the last f32 P-GEMM launch (the tail phase, CSLAM_PGEMM_TAIL)
    "cslam_ekf_pgemm_split": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "cslam_ekf_batch_pgemm_split": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    # the batched scan generator and the two batch calls that consume its scans
    "cslam_sim_batch_create": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_void_p)],
    "cslam_sim_batch_destroy": [C.c_void_p],
    "cslam_sim_batch_scan": [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_longlong, C.POINTER(C.c_int),
                             C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "cslam_sim_batch_get_scan": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cslam_sim_batch_get_table": [C.c_void_p, C.c_void_p],
    "cslam_sim_batch_set_table": [C.c_void_p, C.c_void_p],
    "cslam_ekf_batch_update_scan": [C.c_void_p, C.c_void_p, C.c_void_p],
    "cslam_ekf_batch_augment_scan": [C.c_void_p, C.c_void_p, C.c_void_p],
    # the particle filter's read path: best particle, mixture moments, all features (single handle and sharded)
    "cslam_pf_best_particle": [C.c_void_p, C.c_int, C.POINTER(C.c_int)] + [C.c_void_p] * 5,
    "cslam_pf_estimate": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)] + [C.c_void_p] * 4,
    "cslam_pf_get_all_features": [C.c_void_p, C.c_void_p],
    "cslam_pf_best_particle_sharded": [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_longlong)] + [C.c_void_p] * 5,
    "cslam_pf_estimate_sharded": [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
                                 + [C.c_void_p] * 4,
}
PF_ESTIMATE_SYMBOLS = tuple(k for k in _PROTOTYPES if k.startswith("cslam_pf_"))
PF_PICK_MAX, PF_PICK_MIN = 0, 1
SIM_BATCH_SYMBOLS = tuple(k for k in _PROTOTYPES if "sim_batch" in k or k.endswith("_scan"))

# The score of a Monte-Carlo study kept on the device (cslam_ekf_batch_score_*): indices into one instance's totals, in the
# order of the enum in include/cslam.h, and the prototypes.
SCORE_FIELD_NAMES = ("POSE_N", "POSE_BAD", "POSE_IN", "POSE_ERR2", "POSE_EPHI2", "POSE_NEES",
                     "LM_N", "LM_BAD", "LM_IN", "LM_ERR2", "LM_NEES")
(SCORE_POSE_N, SCORE_POSE_BAD, SCORE_POSE_IN, SCORE_POSE_ERR2, SCORE_POSE_EPHI2, SCORE_POSE_NEES,
 SCORE_LM_N, SCORE_LM_BAD, SCORE_LM_IN, SCORE_LM_ERR2, SCORE_LM_NEES) = range(len(SCORE_FIELD_NAMES))
SCORE_FIELDS = len(SCORE_FIELD_NAMES)
_PROTOTYPES.update({
    "cslam_ekf_batch_score_reset": [C.c_void_p, C.c_int, C.c_double, C.c_double],
    "cslam_ekf_batch_score_set_truth": [C.c_void_p, C.c_void_p, C.c_int],
    "cslam_ekf_batch_score": [C.c_void_p, C.c_void_p],
    "cslam_ekf_batch_score_scan": [C.c_void_p, C.c_void_p, C.c_void_p],
    "cslam_ekf_batch_get_scores": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                   C.POINTER(C.c_longlong)],
})
SCORE_SYMBOLS = tuple(k for k in _PROTOTYPES if "_score" in k)


# The particle filter's data association (EKF.cpp:131-144, 235-326 on every particle's own state) and the consumers of
# its per-particle table.
_PROTOTYPES.update({
    "cslam_pf_associate": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double],
    "cslam_pf_get_association": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cslam_pf_sample_proposal_assoc": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double],
    "cslam_pf_feature_update_assoc": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "cslam_pf_get_stream": [C.c_void_p, C.POINTER(C.c_void_p)],
})
PF_ASSOC_SYMBOLS = tuple(k for k in _PROTOTYPES if k.startswith("cslam_pf_") and "assoc" in k)
PF_ASSOC_FEAT_CHUNK, PF_ASSOC_OBS_CHUNK = 32, 8  # kPfAssocFeatChunk / kPfAssocObsChunk of csrc/pf_assoc_kernels.hpp


# The particle filter's random inputs drawn on the device (slam.h:753-764, PF.cpp:557, 579-596) and the calls that consume
# them; cslam_pf_stage_copies counts the staged host-to-device copies of a handle.
_PROTOTYPES.update({
    "cslam_pf_seed_draws": [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong],
    "cslam_pf_get_draws": [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p],
    "cslam_pf_sample_proposal_drawn": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong],
    "cslam_pf_sample_proposal_assoc_drawn": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                             C.c_longlong],
    "cslam_pf_resample_local_drawn": [C.c_void_p, C.c_longlong, C.c_double, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int)],
    "cslam_pf_resample_sharded_drawn": [C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_int, C.POINTER(C.c_double),
                                        C.POINTER(C.c_int)],
    "cslam_pf_observation_step_drawn": [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_int],
    "cslam_pf_stage_copies": [C.c_void_p, C.POINTER(C.c_longlong)],
})
PF_DRAW_SYMBOLS = ("cslam_pf_seed_draws", "cslam_pf_get_draws", "cslam_pf_sample_proposal_drawn",
                   "cslam_pf_sample_proposal_assoc_drawn", "cslam_pf_resample_local_drawn",
                   "cslam_pf_resample_sharded_drawn", "cslam_pf_observation_step_drawn", "cslam_pf_stage_copies")
PF_DRAW_OBS_MAX = 32  # kPfDrawObsMax of csrc/pf_draw_kernels.hpp: observations that travel as kernel arguments

# The scan that observes only new features (test/main.cpp:314-328): sample every pose from its own Gaussian
# (slam.h:753-764, 413-436), zero Pv, add the features at the sampled pose (PF.cpp:9-60), optionally behind the predict
# (PF.cpp:419-471).
_PROTOTYPES.update({
    "cslam_pf_sample_pose": [C.c_void_p, C.c_void_p],
    "cslam_pf_sample_pose_drawn": [C.c_void_p, C.c_longlong],
    "cslam_pf_new_feature_step": [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_void_p],
    "cslam_pf_new_feature_step_drawn": [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_longlong],
})
PF_NEW_FEATURE_SYMBOLS = ("cslam_pf_sample_pose", "cslam_pf_sample_pose_drawn", "cslam_pf_new_feature_step",
                          "cslam_pf_new_feature_step_drawn")

# The vote on new features kept on the device (the split of test/main.cpp:279-328 decided from the summary of
# EKF.cpp:131-144, 235-326 per particle), the consumers that read its mask where it lies (PF.cpp:502-544, 222-277), the
# add of the voted observations (PF.cpp:9-60) and the whole unknown-correspondence scan in one call.
_PROTOTYPES.update({
    "cslam_pf_associate_vote": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double],
    "cslam_pf_associate_vote_sharded": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                        C.c_double],
    "cslam_pf_vote_wait": [C.c_void_p, C.POINTER(C.c_int), C.c_void_p],
    "cslam_pf_get_vote": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)],
    "cslam_pf_sample_proposal_voted": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double],
    "cslam_pf_sample_proposal_voted_drawn": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_longlong],
    "cslam_pf_feature_update_voted": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "cslam_pf_add_features_voted": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)],
    "cslam_pf_assoc_scan_step_drawn": [C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_longlong,
                                       C.c_double, C.c_int, C.POINTER(C.c_int)],
})
PF_VOTE_SYMBOLS = ("cslam_pf_associate_vote", "cslam_pf_associate_vote_sharded", "cslam_pf_vote_wait", "cslam_pf_get_vote",
                   "cslam_pf_sample_proposal_voted", "cslam_pf_sample_proposal_voted_drawn",
                   "cslam_pf_feature_update_voted", "cslam_pf_add_features_voted", "cslam_pf_assoc_scan_step_drawn")
PF_VOTE_LANES = 256  # kPfVoteLanes of csrc/pf_vote_kernels.hpp: observations per tile of the compaction

# A run of control steps in one launch per PF_CONTROL_MAX (test/main.cpp:279-286: PF.cpp:419-471 then PF.cpp:382-417 per
# step), the count of those launches, and the whole iteration block of test/main.cpp:249-334 in one call, with known and
# with unknown correspondences.
_CONTROL_ARGS = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int]
_PROTOTYPES.update({
    "cslam_pf_control_run": [C.c_void_p] + _CONTROL_ARGS,
    "cslam_pf_control_launches": [C.c_void_p, C.POINTER(C.c_longlong)],
    "cslam_pf_cycle_drawn": [C.c_void_p] + _CONTROL_ARGS + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                            C.c_void_p, C.c_longlong, C.c_double, C.c_int],
    "cslam_pf_assoc_cycle_drawn": [C.c_void_p] + _CONTROL_ARGS + [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                                                  C.c_double, C.c_double, C.c_longlong, C.c_double,
                                                                  C.c_int, C.POINTER(C.c_int)],
})
PF_CONTROL_SYMBOLS = ("cslam_pf_control_run", "cslam_pf_control_launches", "cslam_pf_cycle_drawn",
                      "cslam_pf_assoc_cycle_drawn")
PF_CONTROL_MAX = 16  # kPfControlMax of csrc/pf_control_kernels.hpp: control steps of one launch

# The FastSLAM-1.0 step (slam.h:102): the control run with per-particle control noise (slam.h:149-159), its normals, the
# likelihood weights with the feature update riding along (PF.cpp:343-359, 222-277) and the iteration block in one call.
_PROTOTYPES.update({
    "cslam_pf_control_run_sampled": [C.c_void_p] + _CONTROL_ARGS + [C.c_longlong],
    "cslam_pf_get_control_draws": [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p],
    "cslam_pf_likelihood_update": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int],
    "cslam_pf_fs1_cycle_drawn": [C.c_void_p] + _CONTROL_ARGS + [C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                                C.c_int, C.c_void_p, C.c_longlong, C.c_double, C.c_int],
})
PF_FS1_SYMBOLS = ("cslam_pf_control_run_sampled", "cslam_pf_get_control_draws", "cslam_pf_likelihood_update",
                  "cslam_pf_fs1_cycle_drawn")


# The particle filter's score and trajectory log kept on the device (test/main.cpp:330, slam.h:493-511, 513-539): the
# totals use the SCORE_* indices above; a series record is 4 floats, a track record 5 doubles.
PF_SCORE_MEAN, PF_SCORE_BEST = 0, 1
PF_SCORE_SERIES, PF_SCORE_TRACK = 4, 5
_PROTOTYPES.update({
    "cslam_pf_score_reset": [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double],
    "cslam_pf_score_set_truth": [C.c_void_p, C.c_void_p, C.c_int],
    "cslam_pf_score": [C.c_void_p, C.c_void_p, C.c_int],
    "cslam_pf_score_sharded": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "cslam_pf_get_scores": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                            C.POINTER(C.c_longlong)],
})
PF_SCORE_SYMBOLS = ("cslam_pf_score_reset", "cslam_pf_score_set_truth", "cslam_pf_score", "cslam_pf_score_sharded",
                    "cslam_pf_get_scores")


# The single EKF handle's pose read and its score and trajectory log kept on the device (test/main.cpp:136,
# EKF.cpp:131-144): the totals use the SCORE_* indices above; a series record is 4 floats, a track record 5 doubles
# (X[0], X[1], X[2], trace(P), n).
EKF_SCORE_SERIES, EKF_SCORE_TRACK = 4, 5
_PROTOTYPES.update({
    "cslam_ekf_get_pose": [C.c_void_p, C.c_void_p, C.c_void_p],
    "cslam_ekf_score_reset": [C.c_void_p, C.c_int, C.c_double, C.c_double],
    "cslam_ekf_score_set_truth": [C.c_void_p, C.c_void_p, C.c_int],
    "cslam_ekf_score": [C.c_void_p, C.c_void_p, C.c_int],
    "cslam_ekf_get_scores": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                             C.POINTER(C.c_longlong)],
})
EKF_SCORE_SYMBOLS = ("cslam_ekf_get_pose", "cslam_ekf_score_reset", "cslam_ekf_score_set_truth", "cslam_ekf_score",
                     "cslam_ekf_get_scores")


# The single EKF handle's data association read from the deferred covariance (EKF.cpp:131-144, 235-326, slam.h:482-487):
# host answer plus the reference's split left on the device.
_PROTOTYPES.update({
    "cslam_ekf_associate_deferred": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "cslam_ekf_association_device_ptrs": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p)],
})
EKF_ASSOC_DEFERRED_SYMBOLS = ("cslam_ekf_associate_deferred", "cslam_ekf_association_device_ptrs")


# The update with the observation count read on the device (slam.h:938-943, EKF.cpp:93-129) and the association call that
# does not wait, which together run associate -> update with no host round trip in between.
FACTOR_COUNT_CLAMPED = 64
EKF_COUNTED_M_CAP = {F32: 64, F64: 32}  # largest m_cap cslam_ekf_update_counted accepts
_PROTOTYPES.update({
    "cslam_ekf_update_counted": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "cslam_ekf_associate_deferred_async": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double],
    "cslam_ekf_association_wait": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
})
EKF_COUNTED_SYMBOLS = ("cslam_ekf_update_counted", "cslam_ekf_associate_deferred_async", "cslam_ekf_association_wait")


# Slam::augment with the new features read from device memory, one launch per EKF_AUGMENT_CHUNK features (test/main.cpp:
# 188-189, slam.h:190-191, EKF.cpp:9-91), and the count of augment kernel launches of a handle.
EKF_AUGMENT_CHUNK = 64  # kAugChunk of csrc/ekf_augment_kernels.hpp
_PROTOTYPES.update({
    "cslam_ekf_augment_device": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "cslam_ekf_augment_launches": [C.c_void_p, C.POINTER(C.c_longlong)],
})
EKF_AUGMENT_DEVICE_SYMBOLS = ("cslam_ekf_augment_device", "cslam_ekf_augment_launches")


# The Monte-Carlo driver over single handles: one host thread and one stream pair per handle (ekf.run_many).  The handle
# and pointer tables and the controls travel as plain addresses.
_PROTOTYPES.update({
    "cslam_ekf_run_many": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int],
})


def declared_symbols(header_path: str = HEADER_PATH):
    """Names of every function include/cslam.h declares (used by the export test)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cslam_[a-z0-9_]+)\s*\(", text)))


_lib = None
hip_runtime_path = None  # which libamdhip64 the engine ended up bound to (diagnostics)


def _preload_shared_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (SONAME libamdhip64.so.7, the same SONAME libcslam_hip.so is linked against); if the engine bound the
    system copy under /opt/rocm and torch later loaded its own, the second runtime would see no GPU.  So when
    torch is installed its bundled runtime is loaded first (without importing torch) and the engine's
    DT_NEEDED resolves to it by SONAME.  CSLAM_HIP_RUNTIME=system keeps the /opt/rocm runtime (for processes
    that never touch torch's GPU side)."""
    global hip_runtime_path
    if os.environ.get("CSLAM_HIP_RUNTIME", "torch") == "system":
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        cand = os.path.join(libdir, "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            hip_runtime_path = cand
            # (RCCL, used by cslam_pf_resample_sharded, is bound by the engine with dlopen("librccl.so.1"): a process
            # that has imported torch gets torch's copy by SONAME, any other process the system one.  It must NOT be
            # preloaded here: loading torch's librccl ahead of `import torch` ends in a double free at exit.)
    except Exception:
        pass  # fall back to the system runtime


def lib() -> C.CDLL:
    """Load the engine; raises if the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -m conan_slam_amd.build` (hipcc, gfx950). "
                "There is no CPU fallback for the engine.")
        _preload_shared_hip_runtime()
        _lib = C.CDLL(LIB_PATH)
        _lib.cslam_last_error.restype = C.c_char_p
        for name, args in _PROTOTYPES.items():
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = args, C.c_int
    return _lib


def check(rc: int):
    if rc != OK:
        raise CslamError(rc, lib().cslam_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    c = C.c_int(0)
    rc = lib().cslam_device_count(C.byref(c))
    return c.value if rc == OK else 0
