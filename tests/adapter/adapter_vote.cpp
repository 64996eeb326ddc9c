// Runs scans of the reference's FastSLAM-2 loop WITHOUT its table (test/main.cpp:279-328, unknown correspondences) through
// HipPF::scanStepUnknownAll (include/cslam_adapter.hpp) on a fresh, seeded particle set -- X = 0, P = 0, w = 1/N -- and
// prints every particle's record, for tests/test_adapter_vote_gpu.py to hold against ParticleShard.assoc_scan_step_drawn
// bit for bit.  With `separate` the same scans go through associateVoteAll, sampleProposalVotedAll, resampleParticles and
// addVotedFeaturesAll one by one.  Built with g++ against the Eigen-free stand-in (adapter_standin.hpp) and RUN on the
// GPU box.  TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   np maxFeatures seed lines gate1 gate2 newFraction missLikelihood numEffective
//   lines of `step v swa wb dt q[4] m z[2m] r[4]`          (m = 0: a predict alone; r is read all the same)
// Output: one JSON line {"nf": .., "added": [q per line], "records": [[w, x, y, phi, p[9], xf[2nf], pf[4nf]], ..]}.
#define CSLAM_ADAPTER_STANDIN "adapter_standin.hpp"
#include "cslam_adapter.hpp"

#include <cstdio>
#include <cstring>
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
        std::fprintf(stderr, "usage: adapter_vote <input> [separate]\n");
        return 2;
    }
    const bool    separate = argc > 2 && std::strcmp(argv[2], "separate") == 0;
    std::ifstream in(argv[1]);
    int           np = 0, cap = 0, lines = 0, neff_min = 0;
    long long     seed = 0;
    float         gate1 = 0.f, gate2 = 0.f, frac = 0.f, miss = 0.f;
    if (!(in >> np >> cap >> seed >> lines >> gate1 >> gate2 >> frac >> miss >> neff_min) || np < 1 || cap < 1 || lines < 1)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Eigen::MatrixXf LM(2, 1), WP(2, 1);
    HipPF           pf(LM, WP, np, cap);
    pf.seedDraws(seed);
    std::vector<int> added;
    for (int t = 0; t < lines; t++)
    {
        long long       step = 0;
        int             m    = 0;
        float           v, swa, wb, dt;
        Eigen::MatrixXf Q, R, Z;
        in >> step >> v >> swa >> wb >> dt;
        read_mat(in, Q, 2, 2);
        in >> m;
        read_mat(in, Z, 2, m);
        read_mat(in, R, 2, 2);
        if (!in)
        {
            std::fprintf(stderr, "short input at line %d\n", t);
            return 2;
        }
        pf.setStep(step);
        if (!separate || m == 0)
        {
            added.push_back(pf.scanStepUnknownAll(v, swa, Q, wb, dt, Z, R, gate1, gate2, neff_min, true, frac, miss));
            continue;
        }
        std::vector<Slam::Particle_t> unused;
        pf.predictAll(v, swa, Q, wb, dt);
        pf.associateVoteAll(Z, R, gate1, gate2, frac);
        pf.sampleProposalVotedAll(Z, R, miss);
        pf.resampleParticles(unused, neff_min, true);
        added.push_back(pf.addVotedFeaturesAll(R));
    }
    std::vector<Slam::Particle_t> ps;
    pf.download(ps);
    const int nf = ps.empty() ? 0 : static_cast<int>(ps[0].XF.cols());
    std::printf("{\"nf\": %d, \"added\": [", nf);
    for (size_t i = 0; i < added.size(); i++)
    {
        std::printf("%s%d", i ? ", " : "", added[i]);
    }
    std::printf("], \"records\": [");
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
