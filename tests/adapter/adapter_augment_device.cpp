// One step of the reference's unknown-association branch (test/main.cpp:193-196) through std::shared_ptr<Slam> bound to
// HipEKF (include/cslam_adapter.hpp) with setDeferredAssociation(true): predict, dataAssociate, update, and then the
// augment either from the ZN the association left on the device (HipEKF::augmentAssociated -> cslam_ekf_augment_device)
// or from a host ZN through the virtual (HipEKF::augment -> cslam_ekf_augment).  Built with g++ against the Eigen-free
// stand-in (adapter_standin.hpp) and RUN on the GPU box by tests/test_adapter_augment_device_gpu.py.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   N m device(0 | 1) gate1 gate2 q
//   1 line  X, 3 + 2 N values
//   1 line  P, (3 + 2 N)^2 values column-major
//   1 line  R, 4 values column-major
//   1 line  `v swa Z[2 m]`
//   1 line  ZN[2 q]: the new-feature columns of Z in scan order (used when device = 0)
// Output: one JSON line {"device": d, "new": count the association reported, "n": final state size, "x": [...],
// "p": [...] column-major}.
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

static void print_list(const char* name, const float* v, long count, const char* tail)
{
    std::printf("\"%s\": [", name);
    for (long i = 0; i < count; i++)
    {
        std::printf("%s%.9g", i ? ", " : "", static_cast<double>(v[i]));
    }
    std::printf("]%s", tail);
}

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: adapter_augment_device <run>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           N = 0, m = 0, device = 0, q = 0;
    float         gate1 = 0.f, gate2 = 0.f;
    if (!(in >> N >> m >> device >> gate1 >> gate2 >> q) || N < 1 || m < 1 || q < 0)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const long      n = 3 + 2 * static_cast<long>(N);
    Eigen::VectorXf X;
    Eigen::MatrixXf P, R, Z, ZN;
    float           v = 0.f, swa = 0.f;
    read_mat(in, X, n, 1);
    read_mat(in, P, n, n);
    read_mat(in, R, 2, 2);
    in >> v >> swa;
    read_mat(in, Z, 2, m);
    read_mat(in, ZN, 2, q);
    if (!in)
    {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1), Q(2, 2);
    Q(0, 0) = 0.18f;
    Q(1, 1) = 6e-4f;
    // (CSLAM_Q_TEXTBOOK: see adapter_assoc_deferred.cpp)
    std::shared_ptr<Slam> pSLAM = std::make_shared<HipEKF>(LM, WP, N + m, -1, CSLAM_Q_TEXTBOOK);
    HipEKF*               hip   = static_cast<HipEKF*>(pSLAM.get());
    hip->setDeferredAssociation(true);
    pSLAM->predict(X, P, v, swa, Q, 73.0f, 0.01f);
    Slam::Association_t as = pSLAM->dataAssociate(X, P, Z, R, gate1, gate2); // test/main.cpp:193
    const int           found = hip->associatedNew();
    pSLAM->update(X, P, as.ZF, R, as.idf, true);                             // :194
    if (device)
    {
        hip->augmentAssociated(R); // :195 with the device's ZN
        if (hip->associatedNew() != 0)
        {
            return 1; // consumed once
        }
        hip->augmentAssociated(R); // a second call does nothing
    }
    else
    {
        pSLAM->augment(X, P, ZN, R);
    }
    hip->syncP(X, P);
    std::printf("{\"device\": %d, \"new\": %d, \"n\": %ld, ", device, found, static_cast<long>(X.rows()));
    print_list("x", X.data(), X.rows(), ", ");
    print_list("p", P.data(), P.rows() * P.cols(), "}\n");
    return 0;
}
