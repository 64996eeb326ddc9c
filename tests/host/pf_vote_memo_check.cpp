// pf_vote_memo_check.cpp -- host-only check of PfVoteMemo (conan_slam_amd/csrc/pf_host_parts.hpp), the bookkeeping of the
// vote on new features kept on the device, next to the PfAssocMemo it is sequenced with (built and run by
// tests/test_pf_vote_cpu.py with plain g++ and once more under the address and undefined-behaviour sanitizers).  The
// struct below calls the two memos in the order cslam_pf.hip calls them; what the GPU does in between is left out.  No HIP.
#include <cstdio>
#include <vector>

#include "pf_host_parts.hpp"

using namespace cslam;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do                                                                    \
    {                                                                     \
        if (!(cond))                                                      \
        {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

enum Answer
{
    OK,
    NO_VOTE,
    ADDED,
    MOVED,
    OTHER_SCAN,
    SHRANK,
    NEVER,
    CAPACITY
};

template <typename T>
struct Handle
{
    PfAssocMemo<T> assoc;
    PfVoteMemo     vote;
    int            nf = 0, nfcap = 0;
    int            device_q = 0; // what the vote kernel would count

    void associate(const T* Z, int m)
    {
        assoc.associated(Z, m, nf);
        vote.forget();
    }
    void associate_vote(const T* Z, int m, int q)
    {
        associate(Z, m);
        vote.voted(m);
        device_q = q;
        if (m == 0)
        {
            vote.arrived(0);
        }
    }
    void resample() { assoc.moved(); }
    Answer wait(int* q)
    {
        if (vote.check_read() != PfVoteRefusal::none)
        {
            return NO_VOTE;
        }
        if (!vote.waited())
        {
            vote.arrived(device_q);
        }
        *q = vote.q();
        return OK;
    }
    Answer consume(const T* Z, int m)
    {
        if (vote.check_read() != PfVoteRefusal::none)
        {
            return NO_VOTE;
        }
        switch (assoc.check_scan(Z, m, nf))
        {
        case PfAssocRefusal::none:
            return OK;
        case PfAssocRefusal::moved:
            return MOVED;
        case PfAssocRefusal::other_scan:
            return OTHER_SCAN;
        case PfAssocRefusal::map_shrank:
            return SHRANK;
        default:
            return NEVER;
        }
    }
    Answer add()
    {
        switch (vote.check_add())
        {
        case PfVoteRefusal::no_vote:
            return NO_VOTE;
        case PfVoteRefusal::already_added:
            return ADDED;
        case PfVoteRefusal::none:
            break;
        }
        if (!vote.waited())
        {
            vote.arrived(device_q);
        }
        if (nf + vote.q() > nfcap)
        {
            return CAPACITY;
        }
        nf += vote.q();
        vote.features_added();
        return OK;
    }
};

template <typename T>
static void check_vote_memo()
{
    const T Z[6]  = {(T)1, (T)2, (T)3, (T)4, (T)5, (T)6};
    const T Z2[6] = {(T)1, (T)2, (T)3, (T)4, (T)5, (T)7};
    int     q     = -1;

    // no vote before associate, nor after a plain associate
    Handle<T> h;
    h.nfcap = 8;
    CHECK(!h.vote.live() && h.wait(&q) == NO_VOTE && h.consume(Z, 3) == NO_VOTE && h.add() == NO_VOTE);
    h.associate(Z, 3);
    CHECK(h.wait(&q) == NO_VOTE && h.consume(Z, 3) == NO_VOTE && h.add() == NO_VOTE);
    CHECK(h.assoc.check_scan(Z, 3, h.nf) == PfAssocRefusal::none); // (the table itself is there)

    // a vote: q unknown until somebody waits; wait may be repeated; consumers need the associate's Z and m
    h.associate_vote(Z, 3, 2);
    CHECK(h.vote.live() && h.vote.m() == 3 && !h.vote.waited() && !h.vote.added());
    CHECK(h.consume(Z, 3) == OK && h.consume(Z2, 3) == OTHER_SCAN && h.consume(Z, 2) == OTHER_SCAN);
    CHECK(h.wait(&q) == OK && q == 2 && h.vote.waited());
    h.device_q = 99; // (a second wait reads what the first brought, not the device)
    CHECK(h.wait(&q) == OK && q == 2);
    // added once; the vote stays readable afterwards
    CHECK(h.add() == OK && h.nf == 2 && h.vote.added());
    CHECK(h.add() == ADDED && h.nf == 2);
    CHECK(h.wait(&q) == OK && q == 2 && h.consume(Z, 3) == OK); // (the map grew: still fine for the consumers)

    // dropped by a later associate; replaced by a later vote (which can be added again)
    h.associate(Z, 3);
    CHECK(!h.vote.live() && h.add() == NO_VOTE && h.wait(&q) == NO_VOTE);
    h.associate_vote(Z2, 3, 1);
    CHECK(h.vote.live() && !h.vote.added() && !h.vote.waited());
    CHECK(h.add() == OK && h.nf == 3 && h.vote.waited() && h.vote.q() == 1); // (add waits itself)

    // after a resample: the add still works, the consumers say moved
    h.associate_vote(Z, 3, 3);
    h.resample();
    CHECK(h.consume(Z, 3) == MOVED);
    CHECK(h.wait(&q) == OK && q == 3);
    CHECK(h.add() == OK && h.nf == 6);
    CHECK(h.consume(Z, 3) == MOVED && h.add() == ADDED);

    // a refused add (capacity) leaves the vote live, waited and not added; it goes through once there is room
    h.associate_vote(Z, 3, 3);
    CHECK(h.add() == CAPACITY && h.nf == 6);
    CHECK(h.vote.live() && h.vote.waited() && h.vote.q() == 3 && !h.vote.added());
    CHECK(h.add() == CAPACITY && h.consume(Z, 3) == OK && h.wait(&q) == OK && q == 3);
    h.nfcap = 9;
    CHECK(h.add() == OK && h.nf == 9 && h.add() == ADDED);

    // a shrunken map refuses the consumers, not the add
    h.associate_vote(Z, 3, 0);
    h.nf = 4;
    CHECK(h.consume(Z, 3) == SHRANK && h.add() == OK && h.nf == 4 && h.vote.added());

    // no observations: a vote with q = 0 known at once
    h.associate_vote(nullptr, 0, 0);
    CHECK(h.vote.live() && h.vote.waited() && h.vote.q() == 0 && h.vote.m() == 0);
    CHECK(h.consume(nullptr, 0) == OK && h.add() == OK && h.add() == ADDED);

    // forget() (the buffers were replaced) drops it
    h.associate_vote(Z, 3, 1);
    h.vote.forget();
    CHECK(h.add() == NO_VOTE && h.consume(Z, 3) == NO_VOTE);

    // PfAssocMemo::check is check_scan plus the host mask
    PfAssocMemo<T> a;
    int            idx = -1;
    const int      use[3] = {1, 0, 2};
    CHECK(a.check_scan(Z, 3, 0) == PfAssocRefusal::never_associated);
    a.associated(Z, 3, 0);
    CHECK(a.check_scan(Z, 3, 0) == PfAssocRefusal::none);
    CHECK(a.check(Z, 3, 0, use, &idx) == PfAssocRefusal::bad_use && idx == 2);
    a.moved();
    CHECK(a.check(Z, 3, 0, use, &idx) == PfAssocRefusal::moved && a.check_scan(Z, 3, 0) == PfAssocRefusal::moved);
}

int main()
{
    check_vote_memo<float>();
    check_vote_memo<double>();
    std::printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
