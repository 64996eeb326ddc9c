// Runs iteration blocks of the FastSLAM-1 loop (the one slam.h:102 would select) through HipPF::controlRunSampledAll /
// likelihoodUpdateAll / cycleFastSlam1All (include/cslam_adapter.hpp) on a fresh, seeded particle set -- X = 0, P = 0,
// w = 1/N -- and prints every particle's record, for tests/test_adapter_fs1_gpu.py to hold against
// ParticleShard.control_run_sampled / likelihood_update / fs1_cycle_drawn bit for bit.  Built with g++ against the
// Eigen-free stand-in (adapter_standin.hpp) and RUN on the GPU box.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   np maxFeatures seed lines numEffective
//   lines of `mode step ctlStep k v[k] swa[k] phi[k] useHeading wb dt q[4] mf zf[2mf] idf[mf] mn zn[2mn] r[4]`
//   mode 0: controlRunSampledAll (the scan is read and ignored); 1: cycleFastSlam1All; 2: likelihoodUpdateAll on zf / idf
//   with the features updated and P zeroed (controls and zn ignored)
// Output: one JSON line {"nf": .., "records": [[w, x, y, phi, p[9], xf[2nf], pf[4nf]], ..]}.
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
        std::fprintf(stderr, "usage: adapter_fs1 <input>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           np = 0, cap = 0, lines = 0, neff_min = 0;
    long long     seed = 0;
    if (!(in >> np >> cap >> seed >> lines >> neff_min) || np < 1 || cap < 1 || lines < 1)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1);
    HipPF           pf(LM, WP, np, cap);
    pf.seedDraws(seed);
    for (int t = 0; t < lines; t++)
    {
        long long       step = 0, ctl = 0;
        int             mode = 0, k = 0, use = 0, mf = 0, mn = 0;
        float           wb, dt;
        Eigen::MatrixXf Q, R, ZF, ZN, V, S, PHI;
        Eigen::VectorXi idf;
        in >> mode >> step >> ctl >> k;
        read_mat(in, V, k, 1);
        read_mat(in, S, k, 1);
        read_mat(in, PHI, k, 1);
        in >> use >> wb >> dt;
        read_mat(in, Q, 2, 2);
        in >> mf;
        read_mat(in, ZF, 2, mf);
        idf.resize(mf);
        for (int i = 0; i < mf; i++)
        {
            in >> idf.data()[i];
        }
        in >> mn;
        read_mat(in, ZN, 2, mn);
        read_mat(in, R, 2, 2);
        if (!in)
        {
            std::fprintf(stderr, "short input at line %d\n", t);
            return 2;
        }
        pf.setStep(step);
        if (mode == 0)
        {
            pf.controlRunSampledAll(V, S, Q, wb, dt, PHI, use != 0, ctl);
        }
        else if (mode == 1)
        {
            pf.cycleFastSlam1All(V, S, Q, wb, dt, PHI, use != 0, ctl, ZF, idf, ZN, R, neff_min, true);
        }
        else
        {
            pf.likelihoodUpdateAll(ZF, idf, R, true, true);
        }
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
