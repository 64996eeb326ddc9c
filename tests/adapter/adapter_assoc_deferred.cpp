// Three steps of the reference's unknown-association branch (test/main.cpp:193-196: dataAssociate, update, augment on
// every observation step) through std::shared_ptr<Slam> bound to HipEKF (include/cslam_adapter.hpp), with
// HipEKF::setDeferredAssociation on or off -- cslam_ekf_associate_deferred or cslam_ekf_associate behind the same virtual.
// Built with g++ against the Eigen-free stand-in (adapter_standin.hpp) and RUN on the GPU box by
// tests/test_adapter_assoc_deferred_gpu.py.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   N steps m deferred(0 | 1) gate1 gate2
//   1 line       X, 3 + 2 N values
//   1 line       P, (3 + 2 N)^2 values column-major
//   1 line       R, 4 values column-major
//   steps lines  `v swa Z[2 m]`: a predict with these controls, then dataAssociate / update(batch) / augment on Z
// Output: one JSON line {"deferred": d, "idf": [[...] per step], "zf": [[...] per step, 2 x mf column-major],
// "zn_cols": [per step], "n": final state size}.
#define CSLAM_ADAPTER_STANDIN "adapter_standin.hpp"
#include "cslam_adapter.hpp"

#include <cstdio>
#include <fstream>
#include <memory>
#include <string>

static void read_mat(std::istream& in, Eigen::MatrixXf& M, long r, long c)
{
    M.resize(r, c);
    for (long i = 0; i < r * c; i++)
    {
        in >> M.data()[i];
    }
}

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: adapter_assoc_deferred <run>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           N = 0, steps = 0, m = 0, deferred = 0;
    float         gate1 = 0.f, gate2 = 0.f;
    if (!(in >> N >> steps >> m >> deferred >> gate1 >> gate2) || N < 1 || steps < 0 || m < 1)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const long      n = 3 + 2 * static_cast<long>(N);
    Eigen::VectorXf X;
    Eigen::MatrixXf P, R;
    read_mat(in, X, n, 1);
    read_mat(in, P, n, n);
    read_mat(in, R, 2, 2);
    if (!in)
    {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1), Q(2, 2);
    Q(0, 0) = 0.18f;
    Q(1, 1) = 6e-4f;
    // (test/main.cpp:89.  CSLAM_Q_TEXTBOOK: the scan is built to be decisive for a filter whose update is the Kalman
    // update; under the reference's lower-Cholesky gain, slam.h:250-260, the state after the first 60-row batch on this
    // map is not one the builder vouches for)
    std::shared_ptr<Slam> pSLAM = std::make_shared<HipEKF>(LM, WP, N + m, -1, CSLAM_Q_TEXTBOOK);
    static_cast<HipEKF*>(pSLAM.get())->setDeferredAssociation(deferred != 0);
    if (static_cast<HipEKF*>(pSLAM.get())->deferredAssociation() != (deferred != 0))
    {
        return 1;
    }
    std::string idf_json, zf_json, zn_json;
    for (int t = 0; t < steps; t++)
    {
        Eigen::MatrixXf Z;
        float           v = 0.f, swa = 0.f;
        in >> v >> swa;
        read_mat(in, Z, 2, m);
        if (!in)
        {
            std::fprintf(stderr, "short input\n");
            return 2;
        }
        pSLAM->predict(X, P, v, swa, Q, 73.0f, 0.01f);
        Slam::Association_t as = pSLAM->dataAssociate(X, P, Z, R, gate1, gate2); // test/main.cpp:193
        pSLAM->update(X, P, as.ZF, R, as.idf, true);                             // :194
        pSLAM->augment(X, P, as.ZN, R);                                          // :195
        if (as.ZF.cols() != as.idf.rows() || (as.ZF.cols() > 0 && as.ZF.rows() != 2))
        {
            std::fprintf(stderr, "bad shapes\n");
            return 1;
        }
        char buf[64];
        idf_json += t ? ", [" : "[";
        zf_json += t ? ", [" : "[";
        for (long i = 0; i < as.idf.rows(); i++)
        {
            std::snprintf(buf, sizeof buf, "%s%d", i ? ", " : "", as.idf(i));
            idf_json += buf;
        }
        for (long i = 0; i < 2 * as.ZF.cols(); i++)
        {
            std::snprintf(buf, sizeof buf, "%s%.9g", i ? ", " : "", static_cast<double>(as.ZF.data()[i]));
            zf_json += buf;
        }
        idf_json += "]";
        zf_json += "]";
        std::snprintf(buf, sizeof buf, "%s%ld", t ? ", " : "", as.ZN.cols());
        zn_json += buf;
    }
    std::printf("{\"deferred\": %d, \"idf\": [%s], \"zf\": [%s], \"zn_cols\": [%s], \"n\": %ld}\n", deferred, idf_json.c_str(),
                zf_json.c_str(), zn_json.c_str(), X.rows());
    return 0;
}
