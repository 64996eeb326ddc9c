// Scores a short filter run through the reference-side binding (include/cslam_adapter.hpp: HipEKF::scoreReset /
// scoreTruth / score / scores / pose) -- the pose test/main.cpp:136 prints and the blocks EKF.cpp:131-144 reads, scored
// and logged on the device with X and P in HBM and no syncP().  Built with g++ against the Eigen-free stand-in
// (adapter_standin.hpp): compiled and linked by tests/test_ekf_score_cpu.py, RUN on the GPU box by
// tests/test_adapter_ekf_score_gpu.py.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   N steps m
//   1 line       X, 3 + 2 N values
//   1 line       P, (3 + 2 N)^2 values column-major
//   1 line       the truth, 2 x N column-major
//   steps lines  `xt yt phit v swa idf[m] Z[2 m]`: a predict with these controls, a batch update with these
//                observations (Z 2 x m column-major), then a score against this true pose
// Output: one JSON line {"calls": n, "totals": [11], "series": [4 per record], "track": [5 per record], "x": [3],
// "pvv": [9]}.
#define CSLAM_ADAPTER_STANDIN "adapter_standin.hpp"
#include "cslam_adapter.hpp"

#include <cstdio>
#include <fstream>

static void read_mat(std::istream& in, Eigen::MatrixXf& M, long r, long c)
{
    M.resize(r, c);
    for (long i = 0; i < r * c; i++)
    {
        in >> M.data()[i];
    }
}

template <typename S>
static void print_list(const char* name, const S* v, size_t count, const char* tail)
{
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < count; i++)
    {
        const double x = static_cast<double>(v[i]);
        if (x != x)
        {
            std::printf("%sNaN", i ? ", " : "");
        }
        else
        {
            std::printf("%s%.17g", i ? ", " : "", x);
        }
    }
    std::printf("]%s", tail);
}

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: adapter_ekf_score <run>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           N = 0, steps = 0, m = 0;
    if (!(in >> N >> steps >> m) || N < 1 || steps < 0 || m < 1 || m > N)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const long      n = 3 + 2 * static_cast<long>(N);
    Eigen::VectorXf X;
    Eigen::MatrixXf P, truth;
    read_mat(in, X, n, 1);
    read_mat(in, P, n, n);
    read_mat(in, truth, 2, N);
    if (!in)
    {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1), Q(2, 2), R(2, 2);
    Q(0, 0) = 0.18f;
    Q(1, 1) = 6e-4f;
    R(0, 0) = 0.08f;
    R(1, 1) = 0.0024f;
    HipEKF ekf(LM, WP, N);
    ekf.scoreReset(steps);
    ekf.scoreTruth(truth);
    for (int t = 0; t < steps; t++)
    {
        Eigen::VectorXf xt(3);
        Eigen::VectorXi idf(m);
        Eigen::MatrixXf Z;
        float           v = 0.f, swa = 0.f;
        in >> xt(0) >> xt(1) >> xt(2) >> v >> swa;
        for (int i = 0; i < m; i++)
        {
            in >> idf(i);
        }
        read_mat(in, Z, 2, m);
        if (!in)
        {
            std::fprintf(stderr, "short input\n");
            return 2;
        }
        ekf.predict(X, P, v, swa, Q, 73.0f, 0.01f);
        ekf.update(X, P, Z, R, idf, true);
        ekf.score(xt);
    }
    std::vector<double> totals, track;
    std::vector<float>  series;
    const long long     calls = ekf.scores(totals, &series, &track);
    Eigen::VectorXf     x;
    Eigen::MatrixXf     Pvv;
    ekf.pose(x, Pvv);
    if (totals.size() != static_cast<size_t>(CSLAM_SCORE_FIELDS) || series.size() != static_cast<size_t>(4 * steps) ||
        track.size() != static_cast<size_t>(5 * steps) || x.rows() != 3 || Pvv.rows() != 3 || Pvv.cols() != 3)
    {
        std::fprintf(stderr, "bad shapes\n");
        return 1;
    }
    std::printf("{\"calls\": %lld, ", calls);
    print_list("totals", totals.data(), totals.size(), ", ");
    print_list("series", series.data(), series.size(), ", ");
    print_list("track", track.data(), track.size(), ", ");
    print_list("x", x.data(), 3, ", ");
    print_list("pvv", Pvv.data(), 9, "}\n");
    return 0;
}
