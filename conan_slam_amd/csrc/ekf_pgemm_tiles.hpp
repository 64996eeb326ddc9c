// ekf_pgemm_tiles.hpp -- the work list of the f32 P-GEMM ekf_downdate_psym4_f32 (DESIGN.md 5 "The P-GEMM").  Host only,
// no HIP: tests/host/pgemm_tiles_check.cpp checks it on the CPU.
//
// The list is the lower-triangular 128 x 128 tiles (ti >= tj), column-of-tiles major so that consecutive entries share
// the column panel, followed by the STRIPS of the tiles that are split: a strip is 32 consecutive rows x 128 columns of
// one tile (four per tile).  The kernel's persistent workgroups work through the whole tiles in their pipelined loop and
// then draw strips from the same ticket counter; a strip that lies wholly at or beyond row n is not on the list at all,
// which is what the default rule uses the strips for (pgemm_tail_rule).
#pragma once

#include <algorithm>
#include <vector>

namespace cslam
{
struct PgemmEntry // (the layout of int2)
{
    int x, y; // whole tile: (ti, tj).  strip s of tile (ti, tj): (ti, tj | s << 16)
};

struct PgemmWork
{
    std::vector<PgemmEntry> list; // `whole` tiles, then `strips` strips
    int whole  = 0;
    int strips = 0;
    int split  = 0; // tiles split into strips
};

constexpr int kPgemmTile  = 128;
constexpr int kPgemmStrip = 32;

// chunk class of a launch: 0: k <= 64 (two chunks of 32), 1: k <= 96 (four of 24), 2: k <= 128 (four of 32)
inline int pgemm_chunk_class(int k8) { return k8 <= 64 ? 0 : (k8 <= 96 ? 1 : 2); }

// strips of the last tile row that hold rows below n (1 .. 4)
inline int pgemm_valid_strips(int tile_rows, int n)
{
    const int rows = std::max(0, std::min(kPgemmTile, n - (tile_rows - 1) * kPgemmTile));
    return (rows + kPgemmStrip - 1) / kPgemmStrip;
}

// The rule for the number of tiles that are split, S.  tiles: lower-triangular tiles; last_row: the tiles of the last
// tile row when that row is partly beyond n (else 0); G: persistent workgroups.
//   - T <= 2 G: every tile is handed out statically (two per workgroup), there is no last round to fill: S = 0.
//   - otherwise the last-row tiles, whose strips beyond n are dropped, and no others: S = last_row.
// The first form also split the tiles of the partial last round plus half a round, to fill the idle slots of the last
// round with quarter tiles.  Measured at n = 10 003, G = 510, k = 128: a strip costs well over a
// quarter of a tile (its panel DMA and its P loads are exposed, a whole tile's are hidden in the pipelined loop), and
// S = 79 / 200 / 355 gave 14 215 / 14 076 / 13 613 steps/s against 13 892 without strips.  The same rule serves the
// three chunk classes (the argument is there so that a class can get its own count).
inline int pgemm_tail_rule(int tiles, int last_row, int G, int chunk_class)
{
    (void)chunk_class;
    if (G < 1 || tiles <= 2 * G)
    {
        return 0;
    }
    return last_row;
}

// tile_rows: 128-row tiles that hold rows below n; tail: the switch CSLAM_PGEMM_TAIL (< 0: the rule, 0: no strips,
// N > 0: exactly min(N, tiles) tiles are split).  The tiles split are, first, those of the last tile row if that row is
// partly beyond n (from its last tile backwards), then the end of the list.
inline PgemmWork pgemm_build_work(int tile_rows, int n, int G, int chunk_class, int tail)
{
    PgemmWork w;
    const int T = tile_rows * (tile_rows + 1) / 2;
    std::vector<PgemmEntry> all;
    all.reserve((size_t)T);
    for (int tj = 0; tj < tile_rows; tj++)
    {
        for (int ti = tj; ti < tile_rows; ti++)
        {
            all.push_back(PgemmEntry{ti, tj});
        }
    }
    // (a last tile row all of whose four strips hold rows below n has nothing to drop: it counts as whole, so the list
    // depends on n only through the number of its strips that do)
    const bool partial    = tile_rows > 0 && pgemm_valid_strips(tile_rows, n) < kPgemmTile / kPgemmStrip;
    const int  last_row   = partial ? tile_rows : 0;
    int        S          = tail < 0 ? pgemm_tail_rule(T, last_row, G, chunk_class) : std::min(tail, T);
    std::vector<char> is_split((size_t)T, 0);
    int               left = S;
    if (partial)
    {
        for (int i = T - 1; i >= 0 && left > 0; i--)
        {
            if (all[(size_t)i].x == tile_rows - 1)
            {
                is_split[(size_t)i] = 1;
                left--;
            }
        }
    }
    for (int i = T - 1; i >= 0 && left > 0; i--)
    {
        if (!is_split[(size_t)i])
        {
            is_split[(size_t)i] = 1;
            left--;
        }
    }
    w.list.reserve((size_t)T + 3 * (size_t)S);
    for (int i = 0; i < T; i++)
    {
        if (!is_split[(size_t)i])
        {
            w.list.push_back(all[(size_t)i]);
        }
    }
    w.whole = (int)w.list.size();
    for (int i = 0; i < T; i++)
    {
        if (is_split[(size_t)i])
        {
            const PgemmEntry t = all[(size_t)i];
            for (int s = 0; s < kPgemmTile / kPgemmStrip; s++)
            {
                if (t.x * kPgemmTile + s * kPgemmStrip < n)
                {
                    w.list.push_back(PgemmEntry{t.x, t.y | (s << 16)});
                }
            }
        }
    }
    w.strips = (int)w.list.size() - w.whole;
    w.split  = S;
    return w;
}

// The batched engine: `instances` filters of the same size in one launch.  The rule sees the union (instances x tiles on G
// workgroups) and the split tiles are shared out evenly over the instances (the first instances take the remainder);
// tail = N > 0 splits min(N, tiles) tiles of EVERY instance.  Entries carry the instance in the upper 16 bits of x; whole
// tiles instance-major in today's order, then the strips instance-major.
inline PgemmWork pgemm_build_work_batch(int instances, int tile_rows, int n, int G, int chunk_class, int tail)
{
    PgemmWork u;
    const int T        = tile_rows * (tile_rows + 1) / 2;
    const int last_row = pgemm_valid_strips(tile_rows, n) < kPgemmTile / kPgemmStrip ? tile_rows : 0;
    const int S = tail < 0 ? pgemm_tail_rule(instances * T, instances * last_row, G, chunk_class) : instances * std::min(tail, T);
    std::vector<PgemmEntry> strips;
    for (int i = 0; i < instances; i++)
    {
        const PgemmWork w = pgemm_build_work(tile_rows, n, G, chunk_class, S / instances + (i < S % instances ? 1 : 0));
        for (int e = 0; e < (int)w.list.size(); e++)
        {
            const PgemmEntry t{w.list[(size_t)e].x | (i << 16), w.list[(size_t)e].y};
            (e < w.whole ? u.list : strips).push_back(t);
        }
        u.split += w.split;
    }
    u.whole  = (int)u.list.size();
    u.strips = (int)strips.size();
    u.list.insert(u.list.end(), strips.begin(), strips.end());
    return u;
}

} // namespace cslam
