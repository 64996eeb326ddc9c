// Runs the reference's FastSLAM-2 loop from an empty map (test/main.cpp:279-328) through HipPF::scanStepAll
// (include/cslam_adapter.hpp) on a fresh, seeded particle set -- X = 0, P = 0, w = 1/N -- and prints every particle's
// record, for tests/test_adapter_new_features_gpu.py to hold against ParticleShard.scan_step_drawn bit for bit.  Built
// with g++ against the Eigen-free stand-in (adapter_standin.hpp) and RUN on the GPU box.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   np maxFeatures seed lines
//   lines of     `0 v swa wb dt q[4]`                                                        a predict alone
//             or `1 step v swa wb dt q[4] mf zf[2mf] idf[mf] mn zn[2mn] r[4] numEffective`   one scan
// Output: one JSON line {"nf": .., "records": [[w, x, y, phi, p[9], xf[2nf], pf[4nf]], ..]} (%.9g: exact for float).
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

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: adapter_new_features <input>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           np = 0, cap = 0, lines = 0;
    long long     seed = 0;
    if (!(in >> np >> cap >> seed >> lines) || np < 1 || cap < 1 || lines < 1)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1);
    HipPF           pf(LM, WP, np, cap);
    pf.seedDraws(seed);
    for (int t = 0; t < lines; t++)
    {
        int             kind = 0, mf = 0, mn = 0, neff_min = 0;
        long long       step = 0;
        float           v, swa, wb, dt;
        Eigen::MatrixXf Q, R, ZF, ZN;
        Eigen::VectorXi idf;
        in >> kind;
        if (kind == 1)
        {
            in >> step;
        }
        in >> v >> swa >> wb >> dt;
        read_mat(in, Q, 2, 2);
        if (kind == 0)
        {
            if (!in)
            {
                std::fprintf(stderr, "short input at line %d\n", t);
                return 2;
            }
            pf.predictAll(v, swa, Q, wb, dt);
            continue;
        }
        in >> mf;
        read_mat(in, ZF, 2, mf);
        idf.resize(mf);
        for (int i = 0; i < mf; i++)
        {
            in >> idf(i);
        }
        in >> mn;
        read_mat(in, ZN, 2, mn);
        read_mat(in, R, 2, 2);
        if (!(in >> neff_min))
        {
            std::fprintf(stderr, "short input at line %d\n", t);
            return 2;
        }
        pf.setStep(step);
        pf.scanStepAll(v, swa, Q, wb, dt, ZF, idf, ZN, R, neff_min, true);
    }
    std::vector<Slam::Particle_t> ps;
    pf.download(ps);
    const int nf = ps.empty() ? 0 : static_cast<int>(ps[0].XF.cols());
    std::printf("{\"nf\": %d, \"records\": [", nf);
    for (size_t i = 0; i < ps.size(); i++)
    {
        const Slam::Particle_t& p = ps[i];
        std::printf("%s[%.9g", i ? ", " : "", static_cast<double>(p.w));
        for (int e = 0; e < 3; e++)
        {
            std::printf(", %.9g", static_cast<double>(p.X(e)));
        }
        for (int e = 0; e < 9; e++)
        {
            std::printf(", %.9g", static_cast<double>(p.P.data()[e]));
        }
        for (int e = 0; e < 2 * nf; e++)
        {
            std::printf(", %.9g", static_cast<double>(p.XF.data()[e]));
        }
        for (int f = 0; f < nf; f++)
        {
            for (int e = 0; e < 4; e++)
            {
                std::printf(", %.9g", static_cast<double>(p.PF[static_cast<size_t>(f)].data()[e]));
            }
        }
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}
