// Scores a short replay through the reference-side binding (include/cslam_adapter.hpp: HipPF::scoreReset / scoreTruth /
// score / scores) -- the estimate test/main.cpp:330 prints (slam.h:493-511, the map slam.h:513-539), scored and logged on
// the device with the set in HBM and no download().  Built with g++ against the Eigen-free stand-in
// (adapter_standin.hpp) and RUN on the GPU box by tests/test_adapter_score_gpu.py.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   np nf estimator steps
//   np lines     `w x y phi p[9] xf[2nf] pf[4nf]`  (matrices column-major)
//   1 line       the truth, 2 x nf column-major
//   steps lines  `xt yt phit v swa`: a predict with these controls, then a score against this true pose
// Output: one JSON line {"calls": n, "totals": [11], "series": [4 records], "track": [5 records]}.
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
static void print_list(const char* name, const std::vector<S>& v, const char* tail)
{
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++)
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
        std::fprintf(stderr, "usage: adapter_score <replay>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           np = 0, nf = 0, estimator = 0, steps = 0;
    if (!(in >> np >> nf >> estimator >> steps) || np < 1 || nf < 0 || steps < 0)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<Slam::Particle_t> parts(static_cast<size_t>(np));
    for (auto& p : parts)
    {
        in >> p.w;
        p.X.resize(3);
        in >> p.X(0) >> p.X(1) >> p.X(2);
        read_mat(in, p.P, 3, 3);
        read_mat(in, p.XF, 2, nf);
        p.PF.resize(static_cast<size_t>(nf));
        for (auto& b : p.PF)
        {
            read_mat(in, b, 2, 2);
        }
    }
    Eigen::MatrixXf truth;
    read_mat(in, truth, 2, nf);
    if (!in)
    {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1), Q(2, 2);
    Q(0, 0) = 0.18f;
    Q(1, 1) = 6e-4f;
    HipPF pf(LM, WP, np, nf);
    pf.upload(parts);
    pf.scoreReset(estimator, steps);
    pf.scoreTruth(truth);
    for (int t = 0; t < steps; t++)
    {
        Eigen::VectorXf xt(3);
        float           v = 0.f, swa = 0.f;
        in >> xt(0) >> xt(1) >> xt(2) >> v >> swa;
        if (!in)
        {
            std::fprintf(stderr, "short input\n");
            return 2;
        }
        pf.predictAll(v, swa, Q, 2.83f, 0.025f);
        pf.score(xt);
    }
    std::vector<double> totals, track;
    std::vector<float>  series;
    const long long     calls = pf.scores(totals, &series, &track);
    if (totals.size() != static_cast<size_t>(CSLAM_SCORE_FIELDS) || series.size() != static_cast<size_t>(4 * steps) ||
        track.size() != static_cast<size_t>(5 * steps))
    {
        std::fprintf(stderr, "bad shapes\n");
        return 1;
    }
    std::printf("{\"calls\": %lld, ", calls);
    print_list("totals", totals, ", ");
    print_list("series", series, ", ");
    print_list("track", track, "}\n");
    return 0;
}
