// Runs a SEEDED HipPF (include/cslam_adapter.hpp: seedDraws / setStep, sampleProposalAll without normals,
// resampleParticles without strata) next to an unseeded one that is handed the same draws through the `normals` overload
// and setStrata, step by step, and reports after how many steps the two particle sets were bit-equal and finite.
// Between steps both sets go back with the P and PF they started with (download / upload): the reference's
// sampleProposal leaves P = 0 (PF.cpp:502-544), and a next step on that would lose its weights.  Built with g++ against
// the Eigen-free stand-in (adapter_standin.hpp) and RUN on the GPU box by tests/test_adapter_draws_gpu.py.
// TEST INFRASTRUCTURE.
//
// Input (text; floats with 9 significant digits, i.e. exact for float):
//   np nf seed steps
//   np lines     `w x y phi p[9] xf[2nf] pf[4nf]`                         (matrices column-major)
//   steps lines  `v swa wb dt q[4] m z[2m] idf[m] r[4] numEffective`
// Output: one JSON line {"steps", "equal_steps", "finite_steps", "resamples", "late_resamples", "moved"}: steps after
// which the two sets were bit-equal / every weight, pose and feature of the seeded one finite; resamples performed, and
// those at a step other than 0; metres slot 0 of the seeded filter ended away from where it started.
#define CSLAM_ADAPTER_STANDIN "adapter_standin.hpp"
#include "cslam_adapter.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>

static void read_mat(std::istream& in, Eigen::MatrixXf& M, long r, long c)
{
    M.resize(r, c);
    for (long i = 0; i < r * c; i++)
    {
        in >> M.data()[i];
    }
}

static bool same(const Eigen::MatrixXf& a, const Eigen::MatrixXf& b)
{
    return a.rows() == b.rows() && a.cols() == b.cols() &&
           std::memcmp(a.data(), b.data(), static_cast<size_t>(a.rows() * a.cols()) * sizeof(float)) == 0;
}

static bool same_sets(const std::vector<Slam::Particle_t>& pa, const std::vector<Slam::Particle_t>& pb)
{
    bool equal = pa.size() == pb.size();
    for (size_t i = 0; equal && i < pa.size(); i++)
    {
        equal = std::memcmp(&pa[i].w, &pb[i].w, sizeof(float)) == 0 && same(pa[i].X, pb[i].X) && same(pa[i].P, pb[i].P) &&
                same(pa[i].XF, pb[i].XF) && pa[i].PF.size() == pb[i].PF.size();
        for (size_t f = 0; equal && f < pa[i].PF.size(); f++)
        {
            equal = same(pa[i].PF[f], pb[i].PF[f]);
        }
    }
    return equal;
}

static bool finite_mat(const Eigen::MatrixXf& a)
{
    bool ok = true;
    for (long i = 0; i < a.rows() * a.cols(); i++)
    {
        ok = ok && std::isfinite(a.data()[i]);
    }
    return ok;
}

static bool finite_set(const std::vector<Slam::Particle_t>& ps)
{
    bool ok = true;
    for (const auto& p : ps)
    {
        ok = ok && std::isfinite(p.w) && finite_mat(p.X) && finite_mat(p.P) && finite_mat(p.XF);
        for (const auto& b : p.PF)
        {
            ok = ok && finite_mat(b);
        }
    }
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::fprintf(stderr, "usage: adapter_draws <input>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int           np = 0, nf = 0, steps = 0;
    long long     seed = 0;
    if (!(in >> np >> nf >> seed >> steps) || np < 1 || nf < 1 || steps < 1)
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
    Eigen::MatrixXf        LM(2, 1), WP(2, 1);
    std::shared_ptr<HipPF> drawn = std::make_shared<HipPF>(LM, WP, np, nf), given = std::make_shared<HipPF>(LM, WP, np, nf);
    drawn->upload(parts);
    given->upload(parts);
    drawn->seedDraws(seed);
    int                resamples = 0, late_resamples = 0, equal_steps = 0, finite_steps = 0;
    double             moved = 0.0;
    std::vector<Slam::Particle_t> pa, pb;
    std::vector<float> nrm(static_cast<size_t>(3) * static_cast<size_t>(np));
    for (int t = 0; t < steps; t++)
    {
        float           v, swa, wb, dt;
        int             m = 0, neff_min = 0;
        Eigen::MatrixXf Q, R, Z;
        Eigen::VectorXi idf;
        in >> v >> swa >> wb >> dt;
        read_mat(in, Q, 2, 2);
        in >> m;
        read_mat(in, Z, 2, m);
        idf.resize(m);
        for (int i = 0; i < m; i++)
        {
            in >> idf(i);
        }
        read_mat(in, R, 2, 2);
        if (!(in >> neff_min))
        {
            std::fprintf(stderr, "short input at step %d\n", t);
            return 2;
        }
        // what the seeded filter is about to consume, for the other one (component-major -> Eigen's 3 x np)
        Eigen::VectorXf select(np);
        if (cslam_pf_get_draws(drawn->handle(), t, nrm.data(), select.data()) != CSLAM_OK)
        {
            std::fprintf(stderr, "%s\n", cslam_last_error());
            return 1;
        }
        Eigen::MatrixXf normals(3, np);
        for (int p = 0; p < np; p++)
        {
            for (int e = 0; e < 3; e++)
            {
                normals(e, p) = nrm[static_cast<size_t>(e) * static_cast<size_t>(np) + static_cast<size_t>(p)];
            }
        }
        drawn->setStep(t);
        drawn->predictAll(v, swa, Q, wb, dt);
        drawn->sampleProposalAll(Z, idf, R);
        drawn->featureUpdateAll(Z, idf, R);
        given->predictAll(v, swa, Q, wb, dt);
        given->sampleProposalAll(Z, idf, R, normals);
        given->featureUpdateAll(Z, idf, R);
        given->setStrata(select);
        std::shared_ptr<Slam> a = drawn, b = given; // test/main.cpp:310 calls it through the base pointer
        a->resampleParticles(parts, neff_min, true);
        b->resampleParticles(parts, neff_min, true);
        const float na = drawn->lastNeff(), nb = given->lastNeff(); // (bits: a NaN must equal itself)
        if (drawn->lastResampled() != given->lastResampled() || std::memcmp(&na, &nb, sizeof(float)) != 0)
        {
            std::fprintf(stderr, "step %d: the two filters decided differently\n", t);
            return 1;
        }
        resamples += drawn->lastResampled() ? 1 : 0;
        late_resamples += (t > 0 && drawn->lastResampled()) ? 1 : 0;
        drawn->download(pa);
        given->download(pb);
        equal_steps += same_sets(pa, pb) ? 1 : 0;
        finite_steps += finite_set(pa) ? 1 : 0;
        moved = std::hypot(static_cast<double>(pa[0].X(0)) - static_cast<double>(parts[0].X(0)),
                           static_cast<double>(pa[0].X(1)) - static_cast<double>(parts[0].X(1)));
        for (size_t i = 0; i < pa.size(); i++) // both sets go on with the covariances they started with
        {
            pa[i].P = pb[i].P = parts[i].P;
            pa[i].PF = pb[i].PF = parts[i].PF;
        }
        drawn->upload(pa);
        given->upload(pb);
    }
    std::printf("{\"steps\": %d, \"equal_steps\": %d, \"finite_steps\": %d, \"resamples\": %d, \"late_resamples\": %d, "
                "\"moved\": %.9g}\n",
                steps, equal_steps, finite_steps, resamples, late_resamples, moved);
    return 0;
}
