// sim_scan_view.hpp -- what the batched engine (cslam_ekf_batch.hip) sees of the batched scan generator's current scan
// (cslam_sim_batch.hip): device-resident pointer tables into the scan slot, the common counts, and the event that guards
// the slot against being rewritten under a window in flight.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/cslam.h"

namespace cslam
{

constexpr int kScanMaxObs = 32;              // observations per scan: the batched update's limit (kLaMaxObs)
constexpr int kScanStride = 2 * kScanMaxObs; // floats per instance in the ZF / ZN slabs of a slot

struct SimScanView
{
    int device, instances;
    int m, mf, mn;          // scan size and its split (common to the instances)
    int nf;                 // the feature count the scan was split against
    int updated, augmented; // consumed by update_scan / augment_scan already
    const float* const* Ztab;   // device [instances]: instance i's ZF (2 x mf, column-major)
    const int* const*   idftab; // device [instances]: the common idf (mf)
    const float*        ZN;     // device: instance i's ZN (2 x mn) at ZN + i * kScanStride
    hipEvent_t          consumed; // to be recorded behind the last kernel that reads the slot
    const float*        LM;       // device [nlm][2]: the true map (read by the score's truth gather)
    const int*          table;    // device [nlm]: tag t -> state feature table[t - 1], 0: not seen yet
    int                 nlm;
};

enum
{
    kScanUpdated   = 1,
    kScanAugmented = 2
};

// the current scan of the generator; CSLAM_ERR_BAD_ARG when there is none
int sim_batch_current(cslam_sim_batch_t s, SimScanView* v);
// marks the current scan consumed by `what`; recorded: the slot's event has been recorded on a consumer's stream
int sim_batch_mark(cslam_sim_batch_t s, int what, bool recorded);

} // namespace cslam
