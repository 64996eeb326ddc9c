// pgemm_tiles_check.cpp -- host-only check of conan_slam_amd/csrc/ekf_pgemm_tiles.hpp (the work list of the f32 P-GEMM:
// whole tiles, then 32-row strips) and of the switch CSLAM_PGEMM_TAIL in ekf_options.hpp.  Built and run by
// tests/test_pgemm_tiles_cpu.py, with plain g++ and once more under the address and undefined-behaviour sanitizers.  No HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ekf_options.hpp"
#include "ekf_pgemm_tiles.hpp"

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

// today's list: lower-triangular tiles, column-of-tiles major
static std::vector<PgemmEntry> todays_list(int tile_rows)
{
    std::vector<PgemmEntry> h;
    for (int tj = 0; tj < tile_rows; tj++)
    {
        for (int ti = tj; ti < tile_rows; ti++)
        {
            h.push_back(PgemmEntry{ti, tj});
        }
    }
    return h;
}

// the properties every list must have; returns false at the first that fails
static bool check_work(const PgemmWork& w, int tile_rows, int n, int instances)
{
    const int T = tile_rows * (tile_rows + 1) / 2;
    if ((int)w.list.size() != w.whole + w.strips)
    {
        return false;
    }
    // cover[instance][tile index in today's order][strip]
    std::vector<int> cover((size_t)instances * T * 4, 0);
    auto             tile_index = [&](int ti, int tj) { return tj * tile_rows - tj * (tj - 1) / 2 + (ti - tj); };
    int              prev       = -1; // whole tiles keep today's order (instance-major)
    for (int e = 0; e < (int)w.list.size(); e++)
    {
        const int ti = w.list[(size_t)e].x & 0xFFFF, inst = w.list[(size_t)e].x >> 16;
        const int tj = w.list[(size_t)e].y & 0xFFFF, s = w.list[(size_t)e].y >> 16;
        if (ti < tj || ti >= tile_rows || tj < 0 || inst < 0 || inst >= instances || s < 0 || s > 3)
        {
            return false;
        }
        const int at = inst * T + tile_index(ti, tj);
        if (e < w.whole)
        {
            if (s != 0 || at <= prev)
            {
                return false;
            }
            prev = at;
            for (int q = 0; q < 4; q++)
            {
                cover[(size_t)at * 4 + q]++;
            }
        }
        else
        {
            if (ti * kPgemmTile + s * kPgemmStrip >= n) // no strip lies wholly beyond n
            {
                return false;
            }
            cover[(size_t)at * 4 + s]++;
        }
    }
    // every (tile, strip) with a row below n exactly once; a strip wholly beyond n only inside a whole tile
    for (int inst = 0; inst < instances; inst++)
    {
        for (int tj = 0; tj < tile_rows; tj++)
        {
            for (int ti = tj; ti < tile_rows; ti++)
            {
                for (int s = 0; s < 4; s++)
                {
                    const int  c     = cover[((size_t)inst * T + tile_index(ti, tj)) * 4 + s];
                    const bool below = ti * kPgemmTile + s * kPgemmStrip < n;
                    if (below ? c != 1 : c > 1)
                    {
                        return false;
                    }
                }
            }
        }
    }
    return true;
}

static void check_lists()
{
    const int rows_set[] = {1, 2, 3, 10, 79};
    const int past_set[] = {0, 1, 19, 51}; // n on the tile edge, one past it, 19 and 51 rows past it
    for (int tile_rows : rows_set)
    {
        const int T = tile_rows * (tile_rows + 1) / 2;
        for (int past : past_set)
        {
            // `past` rows into the last tile row (0: the row is full, n on the edge)
            const int n       = past == 0 ? tile_rows * kPgemmTile : (tile_rows - 1) * kPgemmTile + past;
            const int G_set[] = {1, 3, 2 * T, 510};
            for (int G : G_set)
            {
                const int tail_set[] = {0, -1, 1, T + 7};
                for (int tail : tail_set)
                {
                    for (int c = 0; c < 3; c++)
                    {
                        const PgemmWork w = pgemm_build_work(tile_rows, n, G, c, tail);
                        CHECK(check_work(w, tile_rows, n, 1));
                        const int valid = pgemm_valid_strips(tile_rows, n);
                        if (tail == 0)
                        {
                            // today's list, entry for entry
                            const std::vector<PgemmEntry> h = todays_list(tile_rows);
                            CHECK(w.strips == 0 && w.split == 0 && w.whole == T && w.list.size() == h.size());
                            for (size_t e = 0; e < h.size() && e < w.list.size(); e++)
                            {
                                CHECK(w.list[e].x == h[e].x && w.list[e].y == h[e].y);
                            }
                        }
                        else if (tail > 0)
                        {
                            CHECK(w.split == std::min(tail, T) && w.whole == T - w.split);
                            if (tail == 1)
                            {
                                // the last diagonal tile: all of its strips that hold rows below n
                                CHECK(w.strips == valid);
                                CHECK(w.list.back().x == tile_rows - 1 && (w.list.back().y & 0xFFFF) == tile_rows - 1);
                            }
                            else
                            {
                                CHECK(w.whole == 0 && w.strips == 4 * T - (4 - valid) * tile_rows);
                            }
                        }
                        else
                        {
                            const int last_row = valid < 4 ? tile_rows : 0;
                            CHECK(w.split == pgemm_tail_rule(T, last_row, G, c));
                            CHECK(T > 2 * G || w.split == 0); // all tiles static: nothing to fill
                            if (w.split > 0 && last_row > 0)
                            {
                                // the whole last tile row is split, and its strips beyond n are gone
                                for (int e = 0; e < w.whole; e++)
                                {
                                    CHECK(w.list[(size_t)e].x != tile_rows - 1);
                                }
                            }
                        }
                        // the batched form: two instances
                        const PgemmWork b = pgemm_build_work_batch(2, tile_rows, n, G, c, tail);
                        CHECK(check_work(b, tile_rows, n, 2));
                        if (tail == 0)
                        {
                            CHECK(b.strips == 0 && b.whole == 2 * T);
                        }
                        else if (tail > 0)
                        {
                            CHECK(b.split == 2 * std::min(tail, T) && b.strips == 2 * w.strips);
                        }
                    }
                }
            }
        }
    }
}

static void check_rule()
{
    // n = 10 003 on 510 workgroups (the headline): 3160 tiles; the 79 of the last tile row (19 valid rows: one strip each)
    // are split and no others -- the value measured best (79 against 200 and 355)
    for (int c = 0; c < 3; c++)
    {
        CHECK(pgemm_tail_rule(3160, 79, 510, c) == 79);
        const PgemmWork w = pgemm_build_work(79, 10003, 510, c, -1);
        CHECK(w.split == 79 && w.whole == 3081 && w.strips == 79);
    }
    // the batched engine at n = 4003 (N = 2000): 32 tile rows, 528 tiles per instance, 35 valid rows (two strips); eight
    // instances on 496 workgroups: 4224 tiles, the 256 of the last tile rows
    CHECK(pgemm_tail_rule(8 * 528, 8 * 32, 496, 2) == 256);
    const PgemmWork b = pgemm_build_work_batch(8, 32, 4003, 496, 2, -1);
    CHECK(b.split == 256 && b.whole == 4224 - 256 && b.strips == 8 * 32 * 2);
    CHECK(check_work(b, 32, 4003, 8));
    // small problems keep today's launch
    CHECK(pgemm_tail_rule(55, 10, 510, 0) == 0 && pgemm_tail_rule(1020, 0, 510, 2) == 0 && pgemm_tail_rule(1021, 0, 510, 2) == 0 && pgemm_tail_rule(1021, 45, 510, 2) == 45);
    CHECK(pgemm_chunk_class(8) == 0 && pgemm_chunk_class(64) == 0 && pgemm_chunk_class(72) == 1 && pgemm_chunk_class(96) == 1 &&
          pgemm_chunk_class(104) == 2 && pgemm_chunk_class(128) == 2);
    CHECK(pgemm_valid_strips(79, 10003) == 1 && pgemm_valid_strips(10, 1203) == 2 && pgemm_valid_strips(2, 256) == 4 &&
          pgemm_valid_strips(2, 129) == 1 && pgemm_valid_strips(3, 257 + 96) == 4);
}

static EkfOptions with_tail(const char* value)
{
    if (value)
    {
        setenv("CSLAM_PGEMM_TAIL", value, 1);
    }
    else
    {
        unsetenv("CSLAM_PGEMM_TAIL");
    }
    const EkfOptions o = EkfOptions::from_env();
    unsetenv("CSLAM_PGEMM_TAIL");
    return o;
}
static EkfBatchOptions bwith_tail(const char* value)
{
    if (value)
    {
        setenv("CSLAM_PGEMM_TAIL", value, 1);
    }
    else
    {
        unsetenv("CSLAM_PGEMM_TAIL");
    }
    const EkfBatchOptions o = EkfBatchOptions::from_env();
    unsetenv("CSLAM_PGEMM_TAIL");
    return o;
}

static void check_options()
{
    CHECK(EkfOptions().pgemm_tail == -1 && with_tail(nullptr).pgemm_tail == -1); // the rule
    CHECK(with_tail("0").pgemm_tail == 0 && with_tail("1").pgemm_tail == 1 && with_tail("355").pgemm_tail == 355);
    CHECK(with_tail("-1").pgemm_tail == -1 && with_tail("-7").pgemm_tail == -1);
    CHECK(with_tail("99999999").pgemm_tail == kPgemmTailMax);
    // the batched engine: the rule too
    CHECK(EkfBatchOptions().pgemm_tail == -1 && bwith_tail(nullptr).pgemm_tail == -1);
    CHECK(bwith_tail("0").pgemm_tail == 0 && bwith_tail("12").pgemm_tail == 12 && bwith_tail("-1").pgemm_tail == -1);
    CHECK(bwith_tail("99999999").pgemm_tail == kPgemmTailMax);
    // the variable touches nothing else
    const EkfOptions a = with_tail("5"), d = with_tail(nullptr);
    CHECK(a.lookahead == d.lookahead && a.xcd_queues == d.xcd_queues && a.psym_nt == d.psym_nt && a.lower == d.lower);
}

int main()
{
    check_lists();
    check_rule();
    check_options();
    std::printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
