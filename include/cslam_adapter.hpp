// cslam_adapter.hpp -- the reference-side binding of libcslam_hip.so: `HipEKF` and `HipPF`, subclasses of the
// reference's own back-ends that forward the hot-path virtuals of `class Slam` (slam/include/slam.h) to the C ABI of
// include/cslam.h.  Header-only; it is compiled BY the reference (which owns Eigen) -- a maintainer adds
//
//     #include "cslam_adapter.hpp"
//     std::shared_ptr<Slam> pSLAM = std::make_shared<HipEKF>(LM, WP, /*maxLandmarks*/ LM.cols());   // test/main.cpp:89
//
// and links -lcslam_hip.  Everything that is NOT on the hot path (dataAssociateTable, the simulator helpers, ...) stays
// the reference's own code, inherited from EKF / PF.
//
// Interfaces replaced (reference file:line):
//   HipEKF::predict          slam.h:841-847   EKF.cpp:406-455        -> cslam_ekf_predict
//   HipEKF::update           slam.h:938-943   EKF.cpp:481-496        -> cslam_ekf_update   (batchUpdate / singleUpdate too)
//   HipEKF::augment          slam.h:190-191   EKF.cpp:9-26           -> cslam_ekf_augment  (addOneNewFeature too)
//   HipEKF::augmentDevice / augmentAssociated   (the same Slam::augment, test/main.cpp:188-189, with the new features read
//                            from device memory, one launch for all of them)  -> cslam_ekf_augment_device
//   HipEKF::observeHeading   slam.h:788       EKF.cpp:328-352        -> cslam_ekf_observe_heading
//   HipEKF::dataAssociate    slam.h:482-487   EKF.cpp:235-326        -> cslam_ekf_associate, or, after
//                            setDeferredAssociation(true),              -> cslam_ekf_associate_deferred (nothing flushed)
//   HipEKF::pose / scoreReset / scoreTruth / score / scores   (the pose test/main.cpp:136 prints and the blocks
//                            EKF.cpp:131-144 reads, scored and logged on the device)
//                                                                    -> cslam_ekf_get_pose / _score_reset / _score_set_truth / _score / _get_scores
//   HipPF::resampleParticles slam.h:871-872   PF.cpp:473-500         -> cslam_pf_resample_local / _sharded
//   HipPF (particle-set forms of) predict / observeHeading / sampleProposal / featureUpdate / addOneNewFeature
//                            slam.h:858-863, 796, 881-884, 549-552, 134; PF.cpp:419-471, 382-417, 502-544, 222-277, 9-60
//   HipPF::extractStates     slam.h:493-511                          -> cslam_pf_best_particle
//   HipPF::extractFeatures   slam.h:513-539                          -> cslam_pf_get_all_features
//   HipPF::extractMap        (the mixture's feature means)           -> cslam_pf_estimate
//   HipPF::scoreReset / scoreTruth / score / scores   (the estimate test/main.cpp:330 prints, scored and logged on the
//                            device; slam.h:493-511, 513-539)        -> cslam_pf_score_reset / _set_truth / _score / _get_scores
//   HipPF::associateVoteAll / sampleProposalVotedAll / addVotedFeaturesAll / scanStepUnknownAll   (the loop of
//                            test/main.cpp:279-328 without its table: EKF.cpp:131-144, 235-326 per particle, the vote on
//                            new features kept on the device)         -> cslam_pf_associate_vote / _sample_proposal_voted_drawn
//                                                                       / _add_features_voted / _assoc_scan_step_drawn
//   HipPF::controlRunAll / cycleAll / cycleUnknownAll   (the control steps between two scans, test/main.cpp:279-286, in one
//                            launch per 16, and the whole iteration block of test/main.cpp:249-334 in one call)
//                                                                    -> cslam_pf_control_run / _cycle_drawn / _assoc_cycle_drawn
//   HipPF::controlRunSampledAll / likelihoodUpdateAll / cycleFastSlam1All   (the FastSLAM-1.0 loop behind slam.h:102:
//                            slam.h:149-159 per particle, PF.cpp:343-359, 222-277, 473-500, 9-60)
//                                                                    -> cslam_pf_control_run_sampled / _likelihood_update / _fs1_cycle_drawn
//
// Ownership: the reference passes X and P by reference into every call; here the handle owns them in HBM.  X is
// refreshed after every call (the driver reads it every iteration, test/main.cpp:136); P is refreshed on demand
// (`syncP`), because the driver never reads it between calls (test/main.cpp:165-196).  If the caller edits X or P itself
// it calls `invalidate()` and the next call uploads them again.
//
// The reference's error convention is print-and-continue (e.g. EKF.cpp:125-128): `report` does the same with
// cslam_last_error().
//
// Build variants:
//   * inside the reference tree (Eigen + EKF.h + PF.h on the include path): nothing to define;
//   * CSLAM_ADAPTER_STANDIN="file.hpp": a header that declares stand-ins for the Eigen types and for EKF / PF with the
//     same virtual signatures -- used by this repository's CPU tests (tests/adapter_standin.hpp) to compile the
//     forwarding without Eigen.
#pragma once

#if defined(CSLAM_ADAPTER_STANDIN)
#include CSLAM_ADAPTER_STANDIN
#define CSLAM_ADAPTER_AVAILABLE 1
#elif defined(__has_include)
#if __has_include(<Eigen/Dense>) && __has_include("EKF.h") && __has_include("PF.h")
#include "EKF.h"
#include "PF.h"
#define CSLAM_ADAPTER_AVAILABLE 1
#endif
#endif

#if defined(CSLAM_ADAPTER_AVAILABLE)

#include <iostream>
#include <vector>

#include "cslam.h"

class HipEKF : public EKF
{
  public:
    /// maxLandmarks bounds the state (P is preallocated: augment is O(n), EKF.cpp:67-71's copy-resize disappears)
    HipEKF(const Eigen::MatrixXf& landMarks, const Eigen::MatrixXf& wayPoints, int maxLandmarks, int device = -1,
           int quirks = CSLAM_Q_REF_EXACT)
        : EKF(landMarks, wayPoints)
    {
        report(cslam_ekf_create(maxLandmarks, CSLAM_F32, device, quirks, &h_), "HipEKF::create");
    }
    ~HipEKF() { cslam_ekf_destroy(h_); }
    HipEKF(const HipEKF&)            = delete;
    HipEKF& operator=(const HipEKF&) = delete;

    cslam_ekf_t handle() const { return h_; }
    /// the caller changed X or P behind the engine's back: upload them again at the next call
    void invalidate() { uploaded_ = false; }
    /// refresh the caller's P (and X) from HBM -- the engine's P is the authoritative one between calls
    void syncP(Eigen::VectorXf& X, Eigen::MatrixXf& P)
    {
        int n = 0;
        cslam_ekf_get_n(h_, &n);
        X.resize(n);
        P.resize(n, n);
        report(cslam_ekf_get_state(h_, X.data(), P.data(), static_cast<int>(P.outerStride())), "HipEKF::syncP");
    }

    void predict(Eigen::VectorXf& X, Eigen::MatrixXf& P, const float& v, const float& swa, const Eigen::MatrixXf& Q,
                 const float& wb, const float& dt) override
    {
        push(X, P);
        report(cslam_ekf_predict(h_, v, swa, Q.data(), wb, dt), "HipEKF::predict");
        pullX(X);
    }

    void update(Eigen::VectorXf& X, Eigen::MatrixXf& P, const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R,
                const Eigen::VectorXi& idf, bool batch = false) override
    {
        push(X, P);
        report(cslam_ekf_update(h_, Z.data(), static_cast<int>(Z.cols()), R.data(), idf.data(), batch ? 1 : 0),
               "HipEKF::update");
        pullX(X);
    }
    void batchUpdate(Eigen::VectorXf& X, Eigen::MatrixXf& P, const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R,
                     const Eigen::VectorXi& idf) override
    {
        update(X, P, Z, R, idf, true);
    }
    void singleUpdate(Eigen::VectorXf& X, Eigen::MatrixXf& P, const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R,
                      const Eigen::VectorXi& idf) override
    {
        update(X, P, Z, R, idf, false);
    }

    void augment(Eigen::VectorXf& X, Eigen::MatrixXf& P, const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R) override
    {
        push(X, P);
        report(cslam_ekf_augment(h_, Z.data(), static_cast<int>(Z.cols()), R.data()), "HipEKF::augment");
        pullX(X); // X grows by two per new feature (EKF.cpp:40-49); P keeps growing on the device only
    }
    void addOneNewFeature(Eigen::VectorXf& X, Eigen::MatrixXf& P, const Eigen::MatrixXf& Z,
                          const Eigen::MatrixXf& R) override
    {
        augment(X, P, Z, R);
    }
    using EKF::addOneNewFeature; // (the particle overload stays the reference's empty stub, EKF.h:22-24)

    /// augment with Z (2 x q floats, column-major) already in device memory: all q features in one launch
    /// (cslam_ekf_augment_device).  Plain forwarding: the engine holds the state of the last hot-path call, and the
    /// caller's X grows at the next one (or at syncP).
    void augmentDevice(const void* dZ, int q, const Eigen::MatrixXf& R)
    {
        report(cslam_ekf_augment_device(h_, dZ, q, R.data()), "HipEKF::augmentDevice");
    }
    /// after a dataAssociate under setDeferredAssociation(true): augment with the new-feature list ZN that call left on
    /// the device, taking the count it returned (the ZN the reference's dataAssociate loses at EKF.cpp:307).  Each
    /// association is consumed once; without one this does nothing.
    void augmentAssociated(const Eigen::MatrixXf& R)
    {
        const void* dZN = nullptr;
        const int   q   = associatedNew_;
        associatedNew_  = 0;
        if (q <= 0)
        {
            return;
        }
        report(cslam_ekf_association_device_ptrs(h_, nullptr, nullptr, &dZN, nullptr), "HipEKF::augmentAssociated");
        augmentDevice(dZN, q, R);
    }
    /// new features the last deferred dataAssociate found and augmentAssociated has not consumed yet
    int associatedNew() const { return associatedNew_; }

    void observeHeading(Eigen::VectorXf& X, Eigen::MatrixXf& P, const float& phi, bool useHeading = false) override
    {
        push(X, P);
        report(cslam_ekf_observe_heading(h_, phi, useHeading ? 1 : 0), "HipEKF::observeHeading");
        pullX(X);
    }
    using EKF::observeHeading;

    Association_t dataAssociate(const Eigen::VectorXf& X, const Eigen::MatrixXf& P, const Eigen::MatrixXf& Z,
                                const Eigen::MatrixXf& R, const float& gate1, const float& gate2) override
    {
        push(X, P);
        const int        m = static_cast<int>(Z.cols());
        std::vector<int> idf(static_cast<size_t>(m > 0 ? m : 1)), kind(static_cast<size_t>(m > 0 ? m : 1));
        associatedNew_ = 0;
        if (deferredAssociation_)
        {
            int counts[3] = {0, 0, 0};
            report(cslam_ekf_associate_deferred(h_, Z.data(), m, R.data(), gate1, gate2, idf.data(), kind.data(), counts),
                   "HipEKF::dataAssociate");
            associatedNew_ = counts[1]; // (left on the device as ZN: augmentAssociated)
        }
        else
        {
            report(cslam_ekf_associate(h_, Z.data(), m, R.data(), gate1, gate2, idf.data(), kind.data()),
                   "HipEKF::dataAssociate");
        }
        int nf = 0;
        for (int i = 0; i < m; i++)
        {
            nf += (kind[static_cast<size_t>(i)] == 1) ? 1 : 0;
        }
        Association_t out;
        out.ZF.resize(2, nf);
        out.idf.resize(nf);
        out.ZN.resize(0, 0); // EKF.cpp:307 re-declares ZN: the reference returns an EMPTY new-feature list
        for (int i = 0, c = 0; i < m; i++)
        {
            if (kind[static_cast<size_t>(i)] == 1)
            {
                out.ZF(0, c)  = Z(0, i);
                out.ZF(1, c)  = Z(1, i);
                out.idf(c++) = idf[static_cast<size_t>(i)];
            }
        }
        return out;
    }

    /// on: dataAssociate reads the deferred covariance as it stands (cslam_ekf_associate_deferred: the pending downdate
    /// stays pending, the run continues bit for bit as without the call); off (the default): cslam_ekf_associate
    void setDeferredAssociation(bool on) { deferredAssociation_ = on; }
    bool deferredAssociation() const { return deferredAssociation_; }

    /// the pose and its 3 x 3 covariance block without touching P (no downdate, no copy of P): what a host scorer reads
    /// beside the line test/main.cpp:136 prints
    void pose(Eigen::VectorXf& x, Eigen::MatrixXf& Pvv)
    {
        x.resize(3);
        Pvv.resize(3, 3);
        float pv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        report(cslam_ekf_get_pose(h_, x.data(), pv), "HipEKF::pose");
        for (int c = 0; c < 3; c++)
        {
            for (int r = 0; r < 3; r++)
            {
                Pvv(r, c) = pv[3 * c + r];
            }
        }
    }

    // ---- the score of the filter and its trajectory log, kept on the device: a consistency study scores the pose
    //      test/main.cpp:136 prints and the blocks EKF.cpp:131-144 reads after every step without reading them back
    void scoreReset(int seriesCapacity = 0, double gatePose = 0.0, double gateLm = 0.0)
    {
        report(cslam_ekf_score_reset(h_, seriesCapacity, gatePose, gateLm), "HipEKF::scoreReset");
    }
    /// lmTrue: 2 x count, column j the true position of state feature j + 1 (the layout of the reference's landmarks)
    void scoreTruth(const Eigen::MatrixXf& lmTrue)
    {
        const int           count = static_cast<int>(lmTrue.cols());
        std::vector<double> rows(static_cast<size_t>(2 * (count > 0 ? count : 1)));
        for (int j = 0; j < count; j++)
        {
            rows[static_cast<size_t>(2 * j)]     = static_cast<double>(lmTrue(0, j));
            rows[static_cast<size_t>(2 * j + 1)] = static_cast<double>(lmTrue(1, j));
        }
        report(cslam_ekf_score_set_truth(h_, rows.data(), count), "HipEKF::scoreTruth");
    }
    /// one score step against the true pose (3); asynchronous, nothing returns.  (The engine's X and P are scored: a
    /// caller that edited its own copies calls invalidate() and makes a hot-path call first.)
    void score(const Eigen::VectorXf& xvTrue, bool withMap = true)
    {
        const double x[3] = {static_cast<double>(xvTrue(0)), static_cast<double>(xvTrue(1)), static_cast<double>(xvTrue(2))};
        report(cslam_ekf_score(h_, x, withMap ? 1 : 0), "HipEKF::score");
    }
    /// the one synchronising read: totals [CSLAM_SCORE_FIELDS]; series (4 floats) and track (5 doubles: x, y, phi,
    /// trace(P), n) per record held; returns the number of score calls since the reset
    long long scores(std::vector<double>& totals, std::vector<float>* series = nullptr, std::vector<double>* track = nullptr)
    {
        int       records = 0;
        long long calls   = 0;
        totals.assign(static_cast<size_t>(CSLAM_SCORE_FIELDS), 0.0);
        report(cslam_ekf_get_scores(h_, nullptr, nullptr, nullptr, 0, &records, &calls), "HipEKF::scores");
        if (series)
        {
            series->assign(static_cast<size_t>(4 * records), 0.f);
        }
        if (track)
        {
            track->assign(static_cast<size_t>(5 * records), 0.0);
        }
        report(cslam_ekf_get_scores(h_, totals.data(), series && records ? series->data() : nullptr,
                                    track && records ? track->data() : nullptr, records, &records, &calls),
               "HipEKF::scores");
        return calls;
    }

  private:
    cslam_ekf_t h_        = nullptr;
    bool        uploaded_ = false;
    bool        deferredAssociation_ = false;
    int         associatedNew_ = 0;

    static void report(int rc, const char* who)
    {
        if (rc != CSLAM_OK)
        {
            std::cout << cslam_last_error() << "\t" << who << std::endl; // cf. EKF.cpp:125-128
        }
    }
    void push(const Eigen::VectorXf& X, const Eigen::MatrixXf& P)
    {
        if (!uploaded_)
        {
            report(cslam_ekf_set_state(h_, X.data(), static_cast<int>(X.rows()), P.data(), static_cast<int>(P.outerStride())),
                   "HipEKF::set_state");
            uploaded_ = true;
        }
    }
    void pullX(Eigen::VectorXf& X)
    {
        int n = 0;
        cslam_ekf_get_n(h_, &n);
        if (X.rows() != n)
        {
            X.resize(n);
        }
        report(cslam_ekf_get_x(h_, X.data(), n), "HipEKF::get_x");
    }
};

// FastSLAM-2: the reference calls the per-particle virtuals in a loop over std::vector<Particle_t>
// (test/main.cpp:279-286, 303-311); the GPU wants the whole set at once, so HipPF adds set-level overloads with the
// same names and argument meaning, and overrides the one virtual that is set-level in the reference already:
// resampleParticles.  The particle set lives in HBM (structure of arrays); `upload` / `download` move it.
class HipPF : public PF
{
  public:
    HipPF(const Eigen::MatrixXf& landMarks, const Eigen::MatrixXf& wayPoints, int numParticles, int maxFeatures,
          int device = -1, int quirks = CSLAM_Q_REF_EXACT)
        : PF(landMarks, wayPoints)
        , np_(numParticles)
    {
        report(cslam_pf_create(numParticles, maxFeatures, CSLAM_F32, device, quirks, &h_), "HipPF::create");
        report(cslam_pf_set_uniform_weight(h_, 1.0 / numParticles), "HipPF::init"); // PF.cpp:327
    }
    ~HipPF() { cslam_pf_destroy(h_); }
    HipPF(const HipPF&)            = delete;
    HipPF& operator=(const HipPF&) = delete;

    cslam_pf_t handle() const { return h_; }

    void upload(const std::vector<Particle_t>& particles)
    {
        std::vector<float> pf;
        for (int i = 0; i < np_ && i < static_cast<int>(particles.size()); i++)
        {
            const Particle_t& p  = particles[static_cast<size_t>(i)];
            const int         nf = static_cast<int>(p.XF.cols());
            pf.resize(static_cast<size_t>(4 * nf));
            for (int f = 0; f < nf; f++)
            {
                for (int e = 0; e < 4; e++)
                {
                    pf[static_cast<size_t>(4 * f + e)] = p.PF[static_cast<size_t>(f)].data()[e];
                }
            }
            report(cslam_pf_set_particle(h_, i, &p.w, p.X.data(), p.P.data(), nf ? p.XF.data() : nullptr,
                                         nf ? pf.data() : nullptr, nf),
                   "HipPF::upload");
        }
    }
    void download(std::vector<Particle_t>& particles)
    {
        int np = 0, nf = 0;
        cslam_pf_get_counts(h_, &np, &nf);
        particles.resize(static_cast<size_t>(np));
        std::vector<float> pf(static_cast<size_t>(4 * (nf > 0 ? nf : 1)));
        for (int i = 0; i < np; i++)
        {
            Particle_t& p = particles[static_cast<size_t>(i)];
            p.X.resize(3);
            p.P.resize(3, 3);
            p.XF.resize(2, nf);
            p.PF.resize(static_cast<size_t>(nf));
            report(cslam_pf_get_particle(h_, i, &p.w, p.X.data(), p.P.data(), nf ? p.XF.data() : nullptr,
                                         nf ? pf.data() : nullptr),
                   "HipPF::download");
            for (int f = 0; f < nf; f++)
            {
                p.PF[static_cast<size_t>(f)].resize(2, 2);
                for (int e = 0; e < 4; e++)
                {
                    p.PF[static_cast<size_t>(f)].data()[e] = pf[static_cast<size_t>(4 * f + e)];
                }
            }
        }
    }

    // ---- set-level forms of the per-particle virtuals (every owned particle in one call)
    void predictAll(const float& v, const float& swa, const Eigen::MatrixXf& Q, const float& wb, const float& dt)
    {
        report(cslam_pf_predict(h_, v, swa, Q.data(), wb, dt), "HipPF::predict"); // PF.cpp:419-471
    }
    void observeHeadingAll(const float& phi, bool useHeading = false)
    {
        report(cslam_pf_observe_heading(h_, phi, useHeading ? 1 : 0), "HipPF::observeHeading"); // PF.cpp:382-417
    }
    /// normals: 3 x numParticles standard-normal draws, the ones slam.h:753-764 would make (column i for particle i)
    void sampleProposalAll(const Eigen::MatrixXf& Z, const Eigen::VectorXi& idf, const Eigen::MatrixXf& R,
                           const Eigen::MatrixXf& normals)
    {
        // the engine wants the draws component-major (normals[e * numParticles + p], one coalesced load per component);
        // an Eigen 3 x numParticles matrix is particle-major
        std::vector<float> nrm;
        if (!componentMajor(normals, nrm, "sampleProposal"))
        {
            return;
        }
        report(cslam_pf_sample_proposal(h_, Z.data(), static_cast<int>(Z.cols()), idf.data(), R.data(), nrm.data()),
               "HipPF::sampleProposal"); // PF.cpp:502-544
    }
    /// the same with the normals of slam.h:753-764 drawn on the device for the step set with setStep(): needs seedDraws()
    void sampleProposalAll(const Eigen::MatrixXf& Z, const Eigen::VectorXi& idf, const Eigen::MatrixXf& R)
    {
        report(cslam_pf_sample_proposal_drawn(h_, Z.data(), static_cast<int>(Z.cols()), idf.data(), R.data(), step_),
               "HipPF::sampleProposal"); // PF.cpp:502-544
    }
    void featureUpdateAll(const Eigen::MatrixXf& Z, const Eigen::VectorXi& idf, const Eigen::MatrixXf& R)
    {
        report(cslam_pf_feature_update(h_, Z.data(), static_cast<int>(Z.cols()), idf.data(), R.data()),
               "HipPF::featureUpdate"); // PF.cpp:222-277
    }
    void addNewFeaturesAll(const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R)
    {
        report(cslam_pf_add_features(h_, Z.data(), static_cast<int>(Z.cols()), R.data()), "HipPF::addOneNewFeature");
    }
    // ---- the scan that observes only new features (test/main.cpp:314-328): the pose of every particle is drawn from its
    //      own Gaussian (slam.h:753-764 with slam.h:413-436), P <- 0, and the features are added at the sampled pose
    /// test/main.cpp:321-324 for every owned particle; normals: 3 x numParticles, as sampleProposalAll takes them
    void sampleNewFeaturePoseAll(const Eigen::MatrixXf& normals)
    {
        std::vector<float> nrm;
        if (componentMajor(normals, nrm, "sampleNewFeaturePose"))
        {
            report(cslam_pf_sample_pose(h_, nrm.data()), "HipPF::sampleNewFeaturePose");
        }
    }
    /// the same with the normals of the step set with setStep() drawn on the device: needs seedDraws()
    void sampleNewFeaturePoseAll() { report(cslam_pf_sample_pose_drawn(h_, step_), "HipPF::sampleNewFeaturePose"); }
    /// test/main.cpp:314-328 in one launch: sample the pose, zero P, addOneNewFeature (PF.cpp:9-60) at the sampled pose
    void addNewFeaturesSampledAll(const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R, const Eigen::MatrixXf& normals)
    {
        std::vector<float> nrm;
        if (componentMajor(normals, nrm, "addNewFeaturesSampled"))
        {
            report(cslam_pf_new_feature_step(h_, 0.0, 0.0, nullptr, 0.0, 0.0, Z.data(), static_cast<int>(Z.cols()), R.data(),
                                             nrm.data()),
                   "HipPF::addNewFeaturesSampled");
        }
    }
    /// the same with the normals of the step set with setStep() drawn on the device: needs seedDraws()
    void addNewFeaturesSampledAll(const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R)
    {
        report(cslam_pf_new_feature_step_drawn(h_, 0.0, 0.0, nullptr, 0.0, 0.0, Z.data(), static_cast<int>(Z.cols()), R.data(),
                                               step_),
               "HipPF::addNewFeaturesSampled");
    }
    /// One scan of the reference's loop -- predict (test/main.cpp:279-286) and the branches of test/main.cpp:303-328 --
    /// with every random input of the step set with setStep() drawn on the device (needs seedDraws()).  ZF / idf: the
    /// observations of known features, ZN: those of new ones, as dataAssociateTable splits them (test/main.cpp:300).
    /// Known features seen: predict + sampleProposal + featureUpdate + resampleParticles, then addOneNewFeature of ZN.
    /// Only new ones: predict, the pose sample, P <- 0 and addOneNewFeature in one launch.  Neither: predict.
    void scanStepAll(const float& v, const float& swa, const Eigen::MatrixXf& Q, const float& wb, const float& dt,
                     const Eigen::MatrixXf& ZF, const Eigen::VectorXi& idf, const Eigen::MatrixXf& ZN,
                     const Eigen::MatrixXf& R, int numEffective, bool resampleStatus = false)
    {
        const int mf = static_cast<int>(ZF.cols()), mn = static_cast<int>(ZN.cols());
        if (mf > 0 && comm_ == nullptr)
        {
            report(cslam_pf_observation_step_drawn(h_, v, swa, Q.data(), wb, dt, ZF.data(), mf, idf.data(), R.data(), step_,
                                                   numEffective, resampleStatus ? 1 : 0),
                   "HipPF::scanStep");
        }
        else if (mf > 0) // a sharded set: the same calls one by one, the resample over the communicator
        {
            double neff      = 0.0;
            int    resampled = 0;
            predictAll(v, swa, Q, wb, dt);
            sampleProposalAll(ZF, idf, R);
            featureUpdateAll(ZF, idf, R);
            report(cslam_pf_resample_sharded_drawn(h_, comm_, step_, numEffective, resampleStatus ? 1 : 0, &neff, &resampled),
                   "HipPF::scanStep");
            lastNeff_      = static_cast<float>(neff);
            lastResampled_ = resampled != 0;
        }
        if (mf > 0 && mn > 0)
        {
            addNewFeaturesAll(ZN, R);
        }
        else if (mf == 0 && mn > 0)
        {
            report(cslam_pf_new_feature_step_drawn(h_, v, swa, Q.data(), wb, dt, ZN.data(), mn, R.data(), step_),
                   "HipPF::scanStep");
        }
        else if (mf == 0)
        {
            predictAll(v, swa, Q, wb, dt);
        }
    }

    // ---- unknown correspondences with the vote on new features kept on the device: no host decision inside the scan
    /// Every particle's own gated nearest-neighbour association (EKF.cpp:131-144, 235-326), then the vote on which
    /// observations become features of every particle (the split test/main.cpp:300 takes from its table), left on the
    /// device.  newFraction: the share of the weight mass that must call an observation new.  With a communicator the
    /// vote reads the summaries of all ranks.  Asynchronous.
    void associateVoteAll(const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R, float gate1, float gate2,
                          float newFraction = 0.5f)
    {
        const int m = static_cast<int>(Z.cols());
        if (comm_ != nullptr)
        {
            report(cslam_pf_associate_vote_sharded(h_, comm_, Z.data(), m, R.data(), gate1, gate2, newFraction),
                   "HipPF::associateVote");
        }
        else
        {
            report(cslam_pf_associate_vote(h_, Z.data(), m, R.data(), gate1, gate2, newFraction), "HipPF::associateVote");
        }
    }
    /// sampleProposal + featureUpdate (PF.cpp:502-544, 222-277) with every particle's own correspondences and the mask of
    /// the vote, read on the device; the normals of the step set with setStep() are drawn there too (needs seedDraws()).
    /// Z: the observations of associateVoteAll.  A particle without a match pays missLikelihood.
    void sampleProposalVotedAll(const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R, float missLikelihood = 1.0f)
    {
        report(cslam_pf_sample_proposal_voted_drawn(h_, Z.data(), static_cast<int>(Z.cols()), R.data(), missLikelihood, step_),
               "HipPF::sampleProposalVoted");
    }
    /// addOneNewFeature (PF.cpp:9-60) of the voted observations, read on the device; returns how many there were
    int addVotedFeaturesAll(const Eigen::MatrixXf& R)
    {
        int q = 0;
        report(cslam_pf_add_features_voted(h_, R.data(), &q), "HipPF::addVotedFeatures");
        return q;
    }
    /// One scan of the reference's loop (test/main.cpp:279-328) WITHOUT its table, for a set held by one handle: predict,
    /// associateVoteAll, sampleProposalVotedAll, resampleParticles with the strata of the step set with setStep() and
    /// addVotedFeaturesAll, in one call that waits for the vote alone.  Returns the number of features added.  No
    /// observations: predict.
    int scanStepUnknownAll(const float& v, const float& swa, const Eigen::MatrixXf& Q, const float& wb, const float& dt,
                           const Eigen::MatrixXf& Z, const Eigen::MatrixXf& R, float gate1, float gate2, int numEffective,
                           bool resampleStatus = false, float newFraction = 0.5f, float missLikelihood = 1.0f)
    {
        int q = 0;
        report(cslam_pf_assoc_scan_step_drawn(h_, v, swa, Q.data(), wb, dt, Z.data(), static_cast<int>(Z.cols()), R.data(),
                                              gate1, gate2, newFraction, missLikelihood, step_, numEffective,
                                              resampleStatus ? 1 : 0, &q),
               "HipPF::scanStepUnknown");
        return q;
    }

    // ---- a run of control steps in one launch, and the whole iteration block of test/main.cpp:249-334 in one call
    /// k = v.rows() iterations of test/main.cpp:279-286 for every owned particle -- predict(v[j], swa[j], Q, wb, dt)
    /// (PF.cpp:419-471) then observeHeading(phi[j], useHeading) (PF.cpp:382-417) -- bit for bit, in one launch per 16
    /// steps.  phi may be empty when useHeading is false.
    void controlRunAll(const Eigen::VectorXf& v, const Eigen::VectorXf& swa, const Eigen::MatrixXf& Q, const float& wb,
                       const float& dt, const Eigen::VectorXf& phi, bool useHeading = false)
    {
        std::vector<double> c;
        if (controls(v, swa, phi, useHeading, c, "controlRun"))
        {
            const int k = static_cast<int>(v.rows());
            report(cslam_pf_control_run(h_, k, c.data(), c.data() + k, Q.data(), wb, dt, useHeading ? c.data() + 2 * k : nullptr,
                                        useHeading ? 1 : 0),
                   "HipPF::controlRun");
        }
    }
    /// One iteration block of the reference's loop with mSwitchHeadingKnown as the caller has it: ALL the control steps
    /// since the last scan (the last one included), then the scan without a predict of its own, every random input of the
    /// step set with setStep() drawn on the device (needs seedDraws()).  ZF / idf / ZN as scanStepAll takes them.
    void cycleAll(const Eigen::VectorXf& v, const Eigen::VectorXf& swa, const Eigen::MatrixXf& Q, const float& wb,
                  const float& dt, const Eigen::VectorXf& phi, bool useHeading, const Eigen::MatrixXf& ZF,
                  const Eigen::VectorXi& idf, const Eigen::MatrixXf& ZN, const Eigen::MatrixXf& R, int numEffective,
                  bool resampleStatus = false)
    {
        const int mf = static_cast<int>(ZF.cols()), mn = static_cast<int>(ZN.cols());
        if (comm_ == nullptr)
        {
            std::vector<double> c;
            if (controls(v, swa, phi, useHeading, c, "cycle"))
            {
                const int k = static_cast<int>(v.rows());
                report(cslam_pf_cycle_drawn(h_, k, c.data(), c.data() + k, Q.data(), wb, dt,
                                            useHeading ? c.data() + 2 * k : nullptr, useHeading ? 1 : 0, ZF.data(), mf,
                                            idf.data(), ZN.data(), mn, R.data(), step_, numEffective, resampleStatus ? 1 : 0),
                       "HipPF::cycle");
            }
            return;
        }
        // a sharded set: the run, then the same calls one by one, the resample over the communicator (as scanStepAll)
        controlRunAll(v, swa, Q, wb, dt, phi, useHeading);
        if (mf > 0)
        {
            double neff      = 0.0;
            int    resampled = 0;
            sampleProposalAll(ZF, idf, R);
            featureUpdateAll(ZF, idf, R);
            report(cslam_pf_resample_sharded_drawn(h_, comm_, step_, numEffective, resampleStatus ? 1 : 0, &neff, &resampled),
                   "HipPF::cycle");
            lastNeff_      = static_cast<float>(neff);
            lastResampled_ = resampled != 0;
            if (mn > 0)
            {
                addNewFeaturesAll(ZN, R);
            }
        }
        else if (mn > 0)
        {
            addNewFeaturesSampledAll(ZN, R);
        }
    }
    /// The same WITHOUT the table of test/main.cpp:300, for a set held by one handle: the control steps, then the body of
    /// scanStepUnknownAll behind its predict.  Returns the number of features added.  No observations: the run alone.
    int cycleUnknownAll(const Eigen::VectorXf& v, const Eigen::VectorXf& swa, const Eigen::MatrixXf& Q, const float& wb,
                        const float& dt, const Eigen::VectorXf& phi, bool useHeading, const Eigen::MatrixXf& Z,
                        const Eigen::MatrixXf& R, float gate1, float gate2, int numEffective, bool resampleStatus = false,
                        float newFraction = 0.5f, float missLikelihood = 1.0f)
    {
        int                 q = 0;
        std::vector<double> c;
        if (controls(v, swa, phi, useHeading, c, "cycleUnknown"))
        {
            const int k = static_cast<int>(v.rows());
            report(cslam_pf_assoc_cycle_drawn(h_, k, c.data(), c.data() + k, Q.data(), wb, dt,
                                              useHeading ? c.data() + 2 * k : nullptr, useHeading ? 1 : 0, Z.data(),
                                              static_cast<int>(Z.cols()), R.data(), gate1, gate2, newFraction, missLikelihood,
                                              step_, numEffective, resampleStatus ? 1 : 0, &q),
                   "HipPF::cycleUnknown");
        }
        return q;
    }

    // ---- the FastSLAM-1.0 step: the loop the reference's mSwitchSampleProposal (slam.h:102) would select when false
    /// controlRunAll with every particle's own noisy controls (addControlNoise, slam.h:149-159, per particle; Q taken as
    /// diagonal), the normals of control steps ctlStep .. ctlStep + k - 1 drawn on the device: needs seedDraws().
    void controlRunSampledAll(const Eigen::VectorXf& v, const Eigen::VectorXf& swa, const Eigen::MatrixXf& Q, const float& wb,
                              const float& dt, const Eigen::VectorXf& phi, bool useHeading, long long ctlStep)
    {
        std::vector<double> c;
        if (controls(v, swa, phi, useHeading, c, "controlRunSampled"))
        {
            const int k = static_cast<int>(v.rows());
            report(cslam_pf_control_run_sampled(h_, k, c.data(), c.data() + k, Q.data(), wb, dt,
                                                useHeading ? c.data() + 2 * k : nullptr, useHeading ? 1 : 0, ctlStep),
                   "HipPF::controlRunSampled");
        }
    }
    /// PF::likelihood at every particle's own pose, w <- w * like (PF.cpp:343-359), with featureUpdate (PF.cpp:222-277)
    /// riding along and P <- 0 afterwards, in one launch
    void likelihoodUpdateAll(const Eigen::MatrixXf& Z, const Eigen::VectorXi& idf, const Eigen::MatrixXf& R,
                             bool updateFeatures = true, bool zeroP = true)
    {
        report(cslam_pf_likelihood_update(h_, Z.data(), static_cast<int>(Z.cols()), idf.data(), R.data(),
                                          updateFeatures ? 1 : 0, zeroP ? 1 : 0),
               "HipPF::likelihoodUpdate");
    }
    /// One iteration block of the FastSLAM-1 loop: the sampled control run from ctlStep, then -- known features seen --
    /// likelihoodUpdateAll, resampleParticles with the strata of the step set with setStep() (PF.cpp:473-500), then
    /// addOneNewFeature (PF.cpp:9-60) of ZN at every particle's own pose.  No pose is sampled.  Needs seedDraws().
    void cycleFastSlam1All(const Eigen::VectorXf& v, const Eigen::VectorXf& swa, const Eigen::MatrixXf& Q, const float& wb,
                           const float& dt, const Eigen::VectorXf& phi, bool useHeading, long long ctlStep,
                           const Eigen::MatrixXf& ZF, const Eigen::VectorXi& idf, const Eigen::MatrixXf& ZN,
                           const Eigen::MatrixXf& R, int numEffective, bool resampleStatus = false)
    {
        const int mf = static_cast<int>(ZF.cols()), mn = static_cast<int>(ZN.cols());
        if (comm_ == nullptr)
        {
            std::vector<double> c;
            if (controls(v, swa, phi, useHeading, c, "cycleFastSlam1"))
            {
                const int k = static_cast<int>(v.rows());
                report(cslam_pf_fs1_cycle_drawn(h_, k, c.data(), c.data() + k, Q.data(), wb, dt,
                                                useHeading ? c.data() + 2 * k : nullptr, useHeading ? 1 : 0, ctlStep, ZF.data(),
                                                mf, idf.data(), ZN.data(), mn, R.data(), step_, numEffective,
                                                resampleStatus ? 1 : 0),
                       "HipPF::cycleFastSlam1");
            }
            return;
        }
        // a sharded set: the same calls one by one, the resample over the communicator (as cycleAll)
        controlRunSampledAll(v, swa, Q, wb, dt, phi, useHeading, ctlStep);
        if (mf > 0)
        {
            double neff      = 0.0;
            int    resampled = 0;
            likelihoodUpdateAll(ZF, idf, R, true, true);
            report(cslam_pf_resample_sharded_drawn(h_, comm_, step_, numEffective, resampleStatus ? 1 : 0, &neff, &resampled),
                   "HipPF::cycleFastSlam1");
            lastNeff_      = static_cast<float>(neff);
            lastResampled_ = resampled != 0;
        }
        if (mn > 0)
        {
            addNewFeaturesAll(ZN, R);
        }
    }

    /// the strata positions of PF.cpp:557 (stratifiedRandom): supplied by the caller so that runs are reproducible
    /// (the reference seeds from the clock, slam.h:587-594); when a communicator is set, `select` has one entry per
    /// particle of the WHOLE set (numParticles x ranks) and must be identical on every rank
    /// The reference draws fresh strata on every call (stratifiedRandom, PF.cpp:557): so must the caller -- the strata
    /// are consumed by the next resampleParticles and have to be set again before the one after.
    void setStrata(const Eigen::VectorXf& select) { select_ = select; }
    /// Draw the normals of sampleProposalAll(Z, idf, R) and the strata of resampleParticles on the device instead, from
    /// this seed (the reference's generators are seeded from the clock, slam.h:587-594): a draw depends on (seed, step,
    /// particle slot of the WHOLE set) only, so with a communicator every rank passes the same seed and nothing else.
    void seedDraws(long long seed)
    {
        seed_   = seed;
        seeded_ = true;
        applySeed();
    }
    /// the step whose draws the next sampleProposalAll(Z, idf, R) and resampleParticles consume (the caller counts)
    void setStep(long long step) { step_ = step; }
    /// shard the particle set over ranks: resampleParticles then runs the three collectives of SURVEY 8e over RCCL
    void setCommunicator(cslam_comm_t comm)
    {
        comm_  = comm;
        world_ = 1;
        if (comm != nullptr)
        {
            int rank = 0;
            report(cslam_comm_info(comm, &rank, &world_), "HipPF::setCommunicator");
            rank_ = rank;
        }
        else
        {
            rank_ = 0;
        }
        if (seeded_)
        {
            applySeed(); // (the draws are keyed by the slot in the whole set)
        }
    }

    /// slam.h:871-872, PF.cpp:473-500 -- on the particle set held in HBM.  `particles` is not touched: call download()
    /// when the host copy is needed.
    void resampleParticles(std::vector<Particle_t>& /*particles*/, int numEffective, bool resampleStatus = false) override
    {
        double neff      = 0.0;
        int    resampled = 0;
        if (seeded_ && select_.rows() == 0) // no strata set: those of step_, drawn on the device (PF.cpp:557)
        {
            if (comm_ != nullptr)
            {
                report(cslam_pf_resample_sharded_drawn(h_, comm_, step_, numEffective, resampleStatus ? 1 : 0, &neff,
                                                       &resampled),
                       "HipPF::resampleParticles");
            }
            else
            {
                report(cslam_pf_resample_local_drawn(h_, step_, numEffective, resampleStatus ? 1 : 0, &neff, &resampled),
                       "HipPF::resampleParticles");
            }
            lastNeff_      = static_cast<float>(neff);
            lastResampled_ = resampled != 0;
            return;
        }
        // the engine reads numParticles x ranks strata positions from this pointer: refuse anything else, as loudly as
        // the reference's catch blocks do (PF.cpp:215-218), instead of reading past the caller's vector
        if (select_.rows() != static_cast<long>(np_) * world_)
        {
            std::cout << "HipPF::resampleParticles: setStrata() must supply " << static_cast<long>(np_) * world_
                      << " strata positions before every resample (got " << select_.rows() << ")"
                      << "\t" << "resampleParticles" << std::endl;
            return;
        }
        if (comm_ != nullptr)
        {
            report(cslam_pf_resample_sharded(h_, comm_, select_.data(), numEffective, resampleStatus ? 1 : 0, &neff,
                                             &resampled),
                   "HipPF::resampleParticles");
        }
        else
        {
            report(cslam_pf_resample_local(h_, select_.data(), numEffective, resampleStatus ? 1 : 0, &neff, &resampled),
                   "HipPF::resampleParticles");
        }
        lastNeff_      = static_cast<float>(neff);
        lastResampled_ = resampled != 0;
        select_.resize(0); // consumed: the next resample needs its own strata
    }
    float lastNeff() const { return lastNeff_; }
    bool  lastResampled() const { return lastResampled_; }

    // ---- the estimate, read from the set held in HBM (no download())
    /// slam.h:493-511 (the PF loop prints it on every iteration, test/main.cpp:330): the pose of the maximum-weight
    /// particle, which is what the reference meant; referencePick = true takes the MINIMUM-weight particle, which is
    /// what slam.h:505-506 does (`result.first` of std::minmax_element)
    Eigen::VectorXf extractStates(bool referencePick = false)
    {
        Eigen::VectorXf X;
        X.resize(3);
        report(cslam_pf_best_particle(h_, referencePick ? CSLAM_PF_PICK_MIN : CSLAM_PF_PICK_MAX, nullptr, nullptr, X.data(),
                                      nullptr, nullptr, nullptr),
               "HipPF::extractStates");
        return X;
    }
    /// slam.h:513-539: every particle's features side by side, 2 x (numParticles * nf), particle p's block at column p * nf
    Eigen::MatrixXf extractFeatures()
    {
        int np = 0, nf = 0;
        cslam_pf_get_counts(h_, &np, &nf);
        Eigen::MatrixXf XF;
        XF.resize(2, static_cast<long>(np) * nf);
        if (nf > 0)
        {
            report(cslam_pf_get_all_features(h_, XF.data()), "HipPF::extractFeatures");
        }
        return XF;
    }
    /// the map the particle set stands for: the weighted mean of every feature over the particles, 2 x nf
    Eigen::MatrixXf extractMap()
    {
        int np = 0, nf = 0;
        cslam_pf_get_counts(h_, &np, &nf);
        Eigen::MatrixXf XF;
        XF.resize(2, nf);
        if (nf > 0)
        {
            report(cslam_pf_estimate(h_, nullptr, nullptr, nullptr, nullptr, XF.data(), nullptr), "HipPF::extractMap");
        }
        return XF;
    }

    // ---- the score of the estimate and its trajectory log, kept on the device: a study that scores the line
    //      test/main.cpp:330 prints (slam.h:493-511, the map slam.h:513-539) after every step without reading it back
    /// estimator: CSLAM_PF_SCORE_MEAN (what extractMap's estimate is) or CSLAM_PF_SCORE_BEST (what extractStates returns)
    void scoreReset(int estimator = CSLAM_PF_SCORE_MEAN, int seriesCapacity = 0, double gatePose = 0.0, double gateLm = 0.0)
    {
        report(cslam_pf_score_reset(h_, estimator, seriesCapacity, gatePose, gateLm), "HipPF::scoreReset");
    }
    /// lmTrue: 2 x count, column j the true position of state feature j + 1 (the layout of the reference's landmarks)
    void scoreTruth(const Eigen::MatrixXf& lmTrue)
    {
        const int           count = static_cast<int>(lmTrue.cols());
        std::vector<double> rows(static_cast<size_t>(2 * (count > 0 ? count : 1)));
        for (int j = 0; j < count; j++)
        {
            rows[static_cast<size_t>(2 * j)]     = static_cast<double>(lmTrue(0, j));
            rows[static_cast<size_t>(2 * j + 1)] = static_cast<double>(lmTrue(1, j));
        }
        report(cslam_pf_score_set_truth(h_, rows.data(), count), "HipPF::scoreTruth");
    }
    /// one score step against the true pose (3); asynchronous, nothing returns
    void score(const Eigen::VectorXf& xvTrue, bool withMap = true)
    {
        const double x[3] = {static_cast<double>(xvTrue(0)), static_cast<double>(xvTrue(1)), static_cast<double>(xvTrue(2))};
        if (comm_)
        {
            report(cslam_pf_score_sharded(h_, comm_, x, withMap ? 1 : 0), "HipPF::score");
        }
        else
        {
            report(cslam_pf_score(h_, x, withMap ? 1 : 0), "HipPF::score");
        }
    }
    /// the one synchronising read: totals [CSLAM_SCORE_FIELDS]; series (4 floats) and track (5 doubles) per record held;
    /// returns the number of score calls since the reset
    long long scores(std::vector<double>& totals, std::vector<float>* series = nullptr, std::vector<double>* track = nullptr)
    {
        int       records = 0;
        long long calls   = 0;
        totals.assign(static_cast<size_t>(CSLAM_SCORE_FIELDS), 0.0);
        report(cslam_pf_get_scores(h_, nullptr, nullptr, nullptr, 0, &records, &calls), "HipPF::scores");
        if (series)
        {
            series->assign(static_cast<size_t>(4 * records), 0.f);
        }
        if (track)
        {
            track->assign(static_cast<size_t>(5 * records), 0.0);
        }
        report(cslam_pf_get_scores(h_, totals.data(), series && records ? series->data() : nullptr,
                                   track && records ? track->data() : nullptr, records, &records, &calls),
               "HipPF::scores");
        return calls;
    }

  private:
    cslam_pf_t      h_    = nullptr;
    cslam_comm_t    comm_ = nullptr;
    int             world_ = 1;
    int             rank_  = 0;
    int             np_   = 0;
    long long       seed_   = 0;
    long long       step_   = 0;
    bool            seeded_ = false;
    Eigen::VectorXf select_;
    float           lastNeff_      = 0.f;
    bool            lastResampled_ = false;

    static void report(int rc, const char* who)
    {
        if (rc != CSLAM_OK)
        {
            std::cout << cslam_last_error() << "\t" << who << std::endl; // cf. PF.cpp:215-218
        }
    }
    // an Eigen 3 x numParticles matrix of draws (particle-major) as the engine takes them: nrm[e * numParticles + p]
    bool componentMajor(const Eigen::MatrixXf& normals, std::vector<float>& nrm, const char* who) const
    {
        if (normals.rows() != 3 || normals.cols() != np_)
        {
            std::cout << "HipPF::" << who << ": normals must be 3 x " << np_ << "\t" << who << std::endl;
            return false;
        }
        nrm.resize(static_cast<size_t>(3) * static_cast<size_t>(np_));
        for (int p = 0; p < np_; p++)
        {
            for (int e = 0; e < 3; e++)
            {
                nrm[static_cast<size_t>(e) * static_cast<size_t>(np_) + static_cast<size_t>(p)] = normals(e, p);
            }
        }
        return true;
    }
    // the per-step controls of a run as the engine takes them: c = v[k] | swa[k] | phi[k] in double (a float widens
    // exactly, so the engine's cast to its own dtype gives the caller's float back)
    static bool controls(const Eigen::VectorXf& v, const Eigen::VectorXf& swa, const Eigen::VectorXf& phi, bool useHeading,
                         std::vector<double>& c, const char* who)
    {
        const int k = static_cast<int>(v.rows());
        if (static_cast<int>(swa.rows()) != k || (useHeading && static_cast<int>(phi.rows()) != k))
        {
            std::cout << "HipPF::" << who << ": v, swa and (with the heading known) phi need one value per step\t" << who
                      << std::endl;
            return false;
        }
        c.assign(static_cast<size_t>(3 * k) + 1, 0.0); // (+ 1: data() of an empty run is still an address)
        for (int j = 0; j < k; j++)
        {
            c[static_cast<size_t>(j)]         = v(j);
            c[static_cast<size_t>(k + j)]     = swa(j);
            c[static_cast<size_t>(2 * k + j)] = useHeading ? phi(j) : 0.0f;
        }
        return true;
    }
    void applySeed()
    {
        report(cslam_pf_seed_draws(h_, seed_, static_cast<long long>(rank_) * np_, static_cast<long long>(world_) * np_),
               "HipPF::seedDraws");
    }
};

#endif // CSLAM_ADAPTER_AVAILABLE
