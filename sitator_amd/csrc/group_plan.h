// The plan of sit_group_by_site (group.hip) in a form the host compiler takes too (tests/test_group_ref.py runs it with
// g++ under ASan / UBSan): how the entries are cut into chunks, how large the chunk x site table is, where the small
// tables lie in the scratch buffer, which of the two forms of the kernels runs, and how many frames of a host trajectory
// are staged at a time.
//
// The grouping is a counting sort of the entries e = frame * M + ion by their label.  A chunk is GP_CHUNK consecutive
// entries and belongs to ONE wave, which walks it tile by tile (GP_TILE = 64 entries, a lane each) in ascending e:
//   histogram  table[chunk][site] = entries of the chunk with that label
//   scan       table[chunk][site] <- the sum over the earlier chunks of the same site; totals[site]
//   scatter    destination = offsets[site] + table[chunk][site] + rank among the equal labels before it in the chunk
// While a row of the table fits (n_sites <= GP_LDS_MAX_SITES, 32 KB of cursors) a wave keeps its row in LDS; beyond
// that it works on its row of the table in global memory.
#pragma once

#include <stdint.h>

#include "scratch_carve.h"

#define GP_TILE 64
#define GP_CHUNK 4096                                  // entries per chunk: 64 tiles
#define GP_LDS_MAX_SITES 8192                          // cursors of 4 bytes: 32 KB of LDS
#define GP_MAX_ENTRIES ((int64_t)1 << 31)              // destinations and cursors are 32-bit words
#define GP_MAX_TABLE_BYTES ((int64_t)8 << 30)          // the chunk x site table
#define GP_DEFAULT_WORKSPACE ((int64_t)1 << 30)        // staged frames of a host trajectory

struct GroupPlan {
    int64_t n_entries, n_sites, n_mobile, n_chunks;
    int lds;                                           // 1: a wave's row of the table lives in LDS
    int label_bits;                                    // bits that tell the labels [0, n_sites) apart
    int64_t table_words;                               // n_chunks * n_sites (uint32)
    int ok;                                            // 0: beyond GP_MAX_ENTRIES or GP_MAX_TABLE_BYTES
    // the small tables in the scratch buffer: status words (32 bytes), totals [n_sites], offsets [n_sites + 1], the mobile
    // columns [n_mobile], the table
    unsigned long long *status;
    int64_t *totals, *offsets;
    int32_t *midx;
    unsigned *table;
    void lay(Carve &cv)
    {
        status = cv.take<unsigned long long>(4); totals = cv.take<int64_t>(n_sites); offsets = cv.take<int64_t>(n_sites + 1);
        midx = cv.take<int32_t>(n_mobile); table = cv.take<unsigned>(table_words);
    }
};

static inline int gp_label_bits(int64_t n_sites)
{
    int b = 0;
    while (b < 62 && ((int64_t)1 << b) < n_sites) b++;
    return b;
}

// entries [gp_chunk_begin(c), gp_chunk_end(p, c)) belong to chunk c
static inline int64_t gp_chunk_begin(int64_t chunk) { return chunk * GP_CHUNK; }
static inline int64_t gp_chunk_end(const GroupPlan &p, int64_t chunk)
{
    const int64_t e = (chunk + 1) * GP_CHUNK;
    return e < p.n_entries ? e : p.n_entries;
}

// n_entries = F * M, n_sites = K >= 0, n_mobile = M (the mobile columns of a host trajectory are uploaded too)
static inline GroupPlan gp_plan(int64_t n_entries, int64_t n_sites, int64_t n_mobile)
{
    GroupPlan p;
    p.n_entries = n_entries; p.n_sites = n_sites; p.n_mobile = n_mobile;
    p.n_chunks = (n_entries + GP_CHUNK - 1) / GP_CHUNK;
    p.lds = n_sites <= GP_LDS_MAX_SITES ? 1 : 0;
    p.label_bits = gp_label_bits(n_sites);
    p.ok = n_entries >= 0 && n_sites >= 0 && n_mobile >= 0 && n_entries <= GP_MAX_ENTRIES && n_sites < ((int64_t)1 << 31)
           && (p.n_chunks == 0 || n_sites == 0 || n_sites <= GP_MAX_TABLE_BYTES / 4 / p.n_chunks);
    p.table_words = p.ok ? p.n_chunks * n_sites : 0;
    p.status = nullptr; p.totals = p.offsets = nullptr; p.midx = nullptr; p.table = nullptr;
    return p;
}

// frames of a host trajectory [F, A, 3] staged at a time under a cap of `workspace_bytes` (0: the default); 0: the cap is
// below one frame
static inline int64_t gp_frames_per_stage(int64_t workspace_bytes, int64_t n_frames, int64_t n_atoms)
{
    const int64_t cap = workspace_bytes > 0 ? workspace_bytes : GP_DEFAULT_WORKSPACE;
    const int64_t frame_bytes = n_atoms * 24;
    if (frame_bytes <= 0) return n_frames;
    const int64_t fc = cap / frame_bytes;
    return fc < n_frames ? fc : n_frames;
}
