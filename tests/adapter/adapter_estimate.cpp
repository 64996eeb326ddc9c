// Reads the estimate out of a particle set through the reference-side binding (include/cslam_adapter.hpp: HipPF) --
// extractStates (slam.h:493-511), extractFeatures (slam.h:513-539), extractMap -- with the set in HBM and no download().
// Built with g++ against the Eigen-free stand-in (adapter_standin.hpp) and RUN on the GPU box by
// tests/test_adapter_estimate_gpu.py.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   np nf
//   np lines  `w x y phi p[9] xf[2nf] pf[4nf]`  (matrices column-major)
// Output: one JSON line {"states_max": [3], "states_min": [3], "features": [2 np nf], "map": [2 nf]}, column-major.
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

static void print_list(const char* name, const float* v, long n, const char* tail)
{
    std::printf("\"%s\": [", name);
    for (long i = 0; i < n; i++)
    {
        std::printf("%s%.9g", i ? ", " : "", static_cast<double>(v[i]));
    }
    std::printf("]%s", tail);
}

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: adapter_estimate <particles>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           np = 0, nf = 0;
    if (!(in >> np >> nf) || np < 1 || nf < 0)
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
    if (!in)
    {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1);
    HipPF           pf(LM, WP, np, nf);
    pf.upload(parts);
    const Eigen::VectorXf smax = pf.extractStates();
    const Eigen::VectorXf smin = pf.extractStates(true);
    const Eigen::MatrixXf feat = pf.extractFeatures();
    const Eigen::MatrixXf map  = pf.extractMap();
    if (smax.rows() != 3 || smin.rows() != 3 || feat.rows() != 2 || feat.cols() != static_cast<long>(np) * nf ||
        map.rows() != 2 || map.cols() != nf)
    {
        std::fprintf(stderr, "bad shapes\n");
        return 1;
    }
    std::printf("{");
    print_list("states_max", smax.data(), 3, ", ");
    print_list("states_min", smin.data(), 3, ", ");
    print_list("features", feat.data(), 2L * np * nf, ", ");
    print_list("map", map.data(), 2L * nf, "}\n");
    return 0;
}
