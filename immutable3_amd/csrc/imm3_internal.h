// imm3_internal.h -- shared between the HIP kernels (imm3_kernels.hip) and the C-ABI (imm3_api.cpp).
// gfx950 (MI355X, CDNA4) only: wave64, 256 CUs in 8 XCDs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "imm3_int_list_plan.h"
#include "imm3_hi16_plan.h"

// Ablation switches ("what does the kernel cost without its stores?") exist only in the tools' build of the library
// (make -C csrc ablate: -DIMM3_ABLATE -> lib/libimm3_ablate.so, loaded through IMM3_LIB_PATH).  In the shipped build
// IMM3_ABLATED is the constant false and the kernels carry none of it.
#ifdef IMM3_ABLATE
#define IMM3_ABLATED(args, value) ((args).ablate == (value))
#define IMM3_ABLATE_BIT(args, bit) (((args).ablate & (bit)) != 0) /* k_filter_project: ablate = a mask */
#else
#define IMM3_ABLATED(args, value) false
#define IMM3_ABLATE_BIT(args, bit) false
#endif

namespace imm3 {

// A wave owns one TILE = 1024 rows = 16 bitmap words = exactly one 128-byte line of the bitmap,
// so no two waves (let alone two XCDs, whose L2s are not coherent) ever write the same line.
constexpr int kTileRows = 1024;
constexpr int kTileWords = 16;
constexpr int kWavesPerBlock = 4;   // 256-thread workgroups
constexpr int kBlockThreads = 256;
constexpr int kChunkTiles = 256;    // tiles per offsets-scan chunk (one scan workgroup; 382 of them per 100 M rows: every CU has one)
constexpr int kSpanTiles = 16;      // tiles per gather workgroup (kChunkTiles % kSpanTiles == 0)
constexpr int kSpanWords = kSpanTiles * kTileWords;

constexpr int kMaxPredCols = 4;     // distinct predicate columns fused per launch (more -> extra AND pass)
constexpr int kMaxMatch = 8;        // IN-list values carried in kernel arguments
constexpr int kMaxProj = 8;         // projected columns per gather launch

enum ColKind : int32_t { KIND_I32 = 0, KIND_I8 = 1, KIND_STR = 2 };

// Canonical per-column predicate.  All SelectOp leaves on one column are folded on the host:
//   numeric: GT/LT/EQ conjunction -> one closed interval [lo, hi] (narrowing of Select.scala:65,73
//            already applied; empty intervals never reach the kernel),
//   string : Match IN-lists intersected; values whose length != width can never match and are dropped.
struct ColPred {
    const void *data;            // flat column in HBM (DENSE_* decode == little-endian reinterpretation)
    int32_t kind;                // ColKind
    int32_t width;               // bytes per value
    int32_t lo, hi;              // numeric closed interval (int8 values sign-extended)
    int32_t n_match;             // string: IN-list size
    int32_t match_in_args;       // 1: width <= 8 and n_match <= kMaxMatch -> values packed in match[]
    int32_t negated;             // string, select trees only (k_filter_expr_generic): 1 = keep the rows that equal NONE of the values
    int32_t range;               // string: 1 = a byte-order range (IMM3_STR_RANGE): keep the rows with lo' <= row <= hi', the bounds (width bytes each,
                                 // lo' then hi') at match_blob; n_match is 0
    uint64_t match[kMaxMatch];   // value bytes packed little-endian (byte 0 = first character)
    const uint8_t *match_blob;   // otherwise: n_match * width bytes in device memory
    // numeric, IMM3_INT_IN: != 0 = the row must also be a member of the folded list (inside [lo, hi]) -- int8 (1): the 256-bit set in the
    // first 32 bytes of match[]; int32 (1): the probe table (imm3_int_list_plan.h) at match_blob, list_mask + 1 slots; int32 with at most
    // kMaxMatch values (2): the values as int32 in the first 32 bytes of match[], the unused entries repeating the first -- no table
    int32_t list;
    int32_t list_empty;
    uint32_t list_mask, list_shift, list_max_probe;
};

// ---- tile kernel (compile-time column kinds) ----
// The numbers are template arguments (they show in the kernels' names) and stay as they are; a launch's kinds are sorted by
// tile_kind_rank(), in which TK_NONE stays last: TK_H16 ranks behind TK_S2, whose place it takes in the lane (lane_tile()).
// TK_H16: a DENSE_INT column scanned over its 16-bit high-half plane (SegCol::d_hi16), exact through the full column where a half
// does not decide (ColRegs<TK_H16>).  Segment select passes only: no records (rec_layout / ring_layout never see it), no table.
enum TileKind : int32_t { TK_I32 = 0, TK_I8 = 1, TK_S2 = 2, TK_NONE = 3, TK_H16 = 4 };
constexpr int tile_kind_rank(int kind) { return kind == TK_H16 ? 3 : (kind == TK_NONE ? 4 : kind); }
constexpr int kMaxTileCols = 3;
constexpr int kDeferLines = 64;     // bitmap lines a wave parks in LDS between store bursts (32 KiB per work-group)
constexpr int kMaxTileMatch = 8;
constexpr int kMaxArenaSlots = 256; // tiles per wave of a staging launch (the wave's start table sits in LDS)

struct TileCol {
    const void *data;               // flat column in HBM, 16-byte aligned (TK_H16: the plane)
    int32_t lo, hi;                 // TK_I32 / TK_I8 / TK_H16: closed interval
    int32_t n_match;                // TK_S2: IN-list size (1..kMaxTileMatch)
    int32_t negated;                // TK_S2, select trees only (k_filter_expr): 1 = keep the rows that equal NONE of the values
    uint32_t match[kMaxTileMatch];  // TK_S2: the two value bytes, little-endian; TK_H16: match[0..3] = the interval's windows over the halves (Hi16Bounds),
                                    // match[4..5] = the int32 column itself (undecided rows, the partial tile): tile_col_full(),
                                    // match[6..7] = the query's "a tile refined" word: tile_col_refined()
};
// TK_H16's pointer to the full column rides in two words of match[] that an int kind never uses: the record keeps the size and the
// field offsets it had, so the code of every instance without a plane is what it was
IMM3_HOST_DEVICE inline const void *tile_col_full(const TileCol &c) { return (const void *)(uintptr_t)(((uint64_t)c.match[5] << 32) | (uint64_t)c.match[4]); }
inline void tile_col_set_full(TileCol &c, const void *full) {
    c.match[4] = (uint32_t)(uintptr_t)full;
    c.match[5] = (uint32_t)((uint64_t)(uintptr_t)full >> 32);
}
// ... and in match[6..7] a device word of the query (finish[kFinishHi16Refined]) that a wave sets when a tile of its takes the refine:
// diagnostics (imm3_query_hi16_refined), one plain store per refining tile
IMM3_HOST_DEVICE inline unsigned long long *tile_col_refined(const TileCol &c) { return (unsigned long long *)(uintptr_t)(((uint64_t)c.match[7] << 32) | (uint64_t)c.match[6]); }
inline void tile_col_set_refined(TileCol &c, unsigned long long *word) {
    c.match[6] = (uint32_t)(uintptr_t)word;
    c.match[7] = (uint32_t)((uint64_t)(uintptr_t)word >> 32);
}

struct TileArgs {
    TileCol cols[kMaxTileCols];
    int32_t kinds[kMaxTileCols];    // sorted by tile_kind_rank(), TK_NONE last (selects the template instance)
    int32_t and_existing;
    int32_t defer_lines;            // > 0: park the bitmap lines in (dynamic) LDS and store them in bursts (single segment only)
    int32_t ablate;                 // read only by the tools' build (IMM3_ABLATED below); 0 otherwise
    int64_t n_rows, n_words, n_tiles;
    uint64_t *bitmap;               // null: count-only run -- no bitmap line is stored (single-pass chains only: and_existing = 0, defer_lines = 0)
    uint32_t *block_partials;
    unsigned long long *finish;     // {total, n_emit, status, limit, tally, log, log index, log capacity}: the count is reduced in the kernel (block_partial_finish); null = k_total does
    void *stage_rec;                // survivor records (rec_layout(kinds).dwords dwords each): one arena of wave_cap records per wave, or null
    uint32_t *tile_start;           // [wave * max_slots + i]: where in its arena the wave's i-th staged tile starts
    int64_t wave_cap;               // records per arena
    int32_t max_slots;              // tiles a wave stages at most (<= kMaxArenaSlots)
    int32_t chunked;                // 1 (2: the run's first): this launch is one CHUNK of a limit scan (run_select, imm3_api.cpp): it adds to the running count
                                    // finish[kFinishLimitRows] / finish[kFinishLimitTiles], and does nothing at all once that count has reached the limit
    unsigned long long *stamps;     // diagnostics only: per work-group {start, end} of the 100 MHz device clock, or null
    // table queries (imm3_table): the tile table replaces cols[k].data / n_rows.  Tile t holds tile_rows[t] valid rows
    // (1024 except the last tile of each segment) starting at tile_ptrs[k][t] in column k.  Null for one segment.
    const uint32_t *tile_rows;
    const void *const *tile_ptrs[kMaxTileCols];
};

// Survivor record (k_filter_tile's STAGE instances -> k_emit): dword 0 carries the row's position in its tile in bits 0-9;
// the narrow predicate columns (int8: 8 bits, 2-byte string: 16 bits) are packed behind it from bit 16, a field that
// does not fit starting the next dword at bit 0; every int32 predicate column takes a dword of its own after those.
// 1, 2 or 4 dwords per record (3 is padded to 4: 16-byte LDS and global accesses).
struct RecField {
    int dword, shift, bits; // where column `col` sits
    int dwords;             // record size
};
constexpr RecField rec_layout(const int (&kinds)[kMaxTileCols], int col) {
    RecField f{0, 0, 0, 0};
    int d = 0, b = 16;
    for (int i = 0; i < kMaxTileCols; ++i) {
        const int w = kinds[i] == TK_I8 ? 8 : (kinds[i] == TK_S2 ? 16 : 0);
        if (!w) continue;
        if (b + w > 32) {
            ++d;
            b = 0;
        }
        if (i == col) {
            f.dword = d;
            f.shift = b;
            f.bits = w;
        }
        b += w;
    }
    int n = d + 1;
    for (int i = 0; i < kMaxTileCols; ++i) {
        if (kinds[i] != TK_I32) continue;
        if (i == col) {
            f.dword = n;
            f.shift = 0;
            f.bits = 32;
        }
        ++n;
    }
    f.dwords = n == 3 ? 4 : n;
    return f;
}

// Ring record of k_filter_project (imm3_project.hip): it never leaves the CU, so its layout is the streamers' to choose.  Dword 0 =
// the narrow predicate columns from bit 0, as long as they fit 16 bits | the row's position in its RANGE (tile in the range * 1024 +
// position in the tile) << 16; a narrow field that does not fit starts the next dword at bit 0; every int32 predicate column takes a
// dword of its own after those.  With the position on top, a record's first dword is ONE v_or3 in the streamer (value as loaded |
// a per-word constant register | the tile's index) and the row is ONE shift in the writer.  Same sizes as rec_layout: 1, 2 or 4 dwords.
constexpr RecField ring_layout(const int (&kinds)[kMaxTileCols], int col) {
    RecField f{0, 0, 0, 0};
    int d = 0, b = 0, room = 16;
    for (int i = 0; i < kMaxTileCols; ++i) {
        const int w = kinds[i] == TK_I8 ? 8 : (kinds[i] == TK_S2 ? 16 : 0);
        if (!w) continue;
        if (b + w > room) {
            ++d;
            b = 0;
            room = 32;
        }
        if (i == col) {
            f.dword = d;
            f.shift = b;
            f.bits = w;
        }
        b += w;
    }
    int n = d + 1;
    for (int i = 0; i < kMaxTileCols; ++i) {
        if (kinds[i] != TK_I32) continue;
        if (i == col) {
            f.dword = n;
            f.shift = 0;
            f.bits = 32;
        }
        ++n;
    }
    f.dwords = n == 3 ? 4 : n;
    return f;
}

// k_emit: ProjectOp from the staged records
constexpr int kEmitTiles = 32;      // tiles per emit work-group (kChunkTiles % kEmitTiles == 0).  32 beat 64 on C3 (34 -> 31 us) and on clustered survivors (2 % contiguous: 77 -> 40 us), lost on 50 % contiguous (167 -> 196 us); 16 lost on C4 (50 -> 60 us)
constexpr int kMaxEmitGather = 4;   // SELECT-list columns that are not predicate columns: gathered at the record's position
struct EmitCol {
    void *dst;                      // packed output, width bytes per emitted row
    const void *src;                // gathered column (flat), or null when the value comes out of the record
    int32_t width;                  // 1, 2 or 4
    int32_t rec_dword, rec_shift;   // staged column: where it sits in the record
    int32_t pad;
};
struct EmitArgs {
    const void *stage;              // records, R dwords each: one arena per wave of the filter launch that staged them
    const uint32_t *tile_start;     // [wave * max_slots + i]
    int64_t wave_cap, n_waves, main_tiles; // arena size in records; waves of the filter launch; tiles its main loop covered (the rest: leftovers)
    int32_t max_slots, T;           // T: tiles per wave iteration of that launch
    int32_t ablate, pad;            // read only by the tools' build (IMM3_ABLATED); 0 otherwise
    const uint32_t *tile_offsets;
    const uint32_t *chunk_sums;
    int64_t n_tiles;
    uint64_t cap_rows;
    uint32_t *row_index;
    EmitCol cols[kMaxProj];         // gathered columns first
    int32_t n_cols;
    int32_t R;
};
void launch_emit(const EmitArgs &a, int n_gather, int grid_blocks, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// ---- k_filter_project (imm3_project.hip): ScanOp -> SelectOp* -> ProjectOp of one uniform segment in ONE pass ----
// A work-group owns SPANS of kProjectStreamers * P consecutive tiles (each of its streaming waves P consecutive tiles);
// spans go to the work-groups round-robin.  The survivors' records of a wave's range wait in LDS; where they go in the output -- the
// number of survivors in all earlier tiles -- comes from a scan over per-span DESCRIPTORS, one ROUND of spans (one span per
// work-group) at a time: the round's last span to arrive scans the round's counts (imm3_project.hip, span_arrive):
//   desc[s] = epoch << 38 | flag << 36 | value     flag 1: value = survivors of span s (published when the span is done)
//                                                  flag 2: value = survivors of spans 0..s-1: the span's first output row
//                                                  flag 3: the run is being abandoned (a wait timed out)
// `epoch` (the low 26 bits of finish[kFinishEpoch], bumped by the launch's last work-group) tells this run's descriptors from
// earlier runs', so nothing is cleared between runs: a stale tag could only alias after 2^26 runs of the query in which its
// descriptor was never rewritten (round 3 carried 8 bits: 256 bumps -- every count of the query bumps the counter -- and a graph
// that keeps a larger P than the direct runs touches descriptors those never rewrite).  A segment has < 2^32 rows, so 36 value
// bits are plenty.  P is a launch argument: the host lowers it once it has seen how many rows survive (imm3_api.cpp,
// single_pass_adapt); kProjectMinP sizes the descriptor array.
constexpr int kProjectMinP = 1;
constexpr int kProjectMaxP = 64;        // tiles per wave per span (the tile's index in its range takes 6 bits of the record)
// (tools: -DIMM3_PROJECT_STREAMERS=12 -DIMM3_PROJECT_RING_KB=9 was tried -- 16 waves cap the kernel at 128 VGPRs: C3 137 us against 125)
#ifndef IMM3_PROJECT_STREAMERS
#define IMM3_PROJECT_STREAMERS 8
#endif
#ifndef IMM3_PROJECT_RING_KB
#define IMM3_PROJECT_RING_KB 14
#endif
constexpr int kProjectStreamers = IMM3_PROJECT_STREAMERS;  // waves of a work-group that stream tiles: a span is kProjectStreamers * P consecutive tiles
constexpr int kProjectWriters = 4;    // waves of a work-group that write the rows
constexpr int kProjectRingBytes = IMM3_PROJECT_RING_KB * 1024; // a streamer's LDS ring of survivor records
// finish[2], the query's status word: bit 0 malformed PFOR block (k_filter_pfor); single-pass projection: bit 1 = the run's ROWS
// are incomplete because a prefix never came (abandoned), bit 2 = ... because another launch of the kernel owned the device (busy).
// Bits 1-2 are valid for ONE run: bits 8..31 carry the low 24 bits of that run's epoch (status_flag_set / status_raise,
// imm3_project.hip), so a later launch of the query never mistakes an earlier run's flags for its own and the host never
// has to clear the word.  Whatever the flags say, a run's COUNT (finish[0], finish[1]) and BITMAP are exact: a work-group that gives up
// on the rows goes on streaming in count + bitmap mode.
constexpr int kFinishStatus = 2;
constexpr unsigned long long kStatusPfor = 1ULL, kStatusAbandoned = 2ULL, kStatusBusy = 4ULL;
constexpr int kStatusEpochShift = 8;
constexpr unsigned long long kStatusEpochMask = 0xFFFFFFULL;
constexpr int kFinishEpoch = 8;         // finish[8]: run counter of the query (descriptor epochs)
constexpr int kFinishDense = 9;         // finish[9]: single-pass projection: ranges of the last run that outgrew their LDS ring (finish[10]: the running sum)
// `limit` stops the scan (ProjectIterator.hasNext returns false at the limit and the bounded queue stalls the workers:
// Project.scala:73-80, Engine.scala:166,253-258): a projection with a limit runs its select pass as CHUNKS of growing size, each a
// launch that first looks at the rows selected so far and leaves at once when the limit has been reached.
constexpr int kFinishLimitRows = 11;    // finish[11]: rows selected by the chunks of this run so far
constexpr int kFinishLimitTiles = 12;   // finish[12]: tiles those chunks scanned (the offsets scan and the gather stop there)
constexpr int kFinishLimitGaveUp = 13;  // finish[13]: k_limit_gather's look-back ran into its poll cap in the run with this tag: gather with k_scan + k_gather
constexpr int kFinishHi16Refined = 14;  // finish[14]: non-zero once a full tile of a plane scan (TK_H16) has compared full values; imm3_query_hi16_refined reads and clears it
// A TABLE query's limit stops the scan inside ONE launch (k_filter_table_limit, imm3_kernels.hip): its work-groups claim runs of
// kTableLimitClaimTiles consecutive virtual tiles from a ticket counter, in ascending order, and stop claiming once the runs that are
// done have selected `limit` rows (finish[kFinishLimitRows]); the launch's last work-group turns the tickets into finish[kFinishLimitTiles]
// and sets the ticket counter and the rows word back to zero for the next run (no memset, nothing for a recorded graph to miss).
// The ticket counter sits on a 128-byte line of its own, away from the header line that holds the rows word (every claim is one
// returning atomic on the ticket and one access to the rows word; on ONE line they queue behind each other): a spare word of the
// last sub-tally's line, which the tally touches once per work-group, at its exit.
constexpr int kFinishLimitTicketLineWord = 8; // (word 0 of a sub-tally's line is the sub-tally)
constexpr int kTableLimitMaxGrid = 512; // work-groups of the limit-aware launch at most (2 per CU): what they claim at once is what a `limit 10` scans at least
constexpr int kTableLimitClaimTiles = 32; // tiles per claim: eight per wave.  A multiple of kSpanTiles: the gather walks whole spans of the scanned prefix
static_assert(kTableLimitClaimTiles % kSpanTiles == 0 && kTableLimitClaimTiles % kWavesPerBlock == 0, "the scanned prefix ends on a span boundary; a claim splits evenly over the waves");
constexpr int kDescValueBits = 36, kDescFlagShift = 36, kDescEpochShift = 38;
constexpr unsigned long long kDescValueMask = (1ULL << kDescValueBits) - 1;
constexpr unsigned long long kDescEpochMask = (1ULL << (64 - kDescEpochShift)) - 1;
constexpr uint32_t kProjectMaxPolls = 1u << 17; // polls of a look-back wait (~0.1-0.2 s) before the run's rows are given up
struct ProjectTile {                // 32 bytes: one scalar load (s_load_dwordx8) per tile, issued a tile ahead of its use
    const void *p[kMaxTileCols];    // the tile's first value in each tile column of the launch (kinds order)
    uint32_t rows;                  // valid rows (kTileRows: a full tile)
    uint32_t pad;
};
struct ProjectArgs {
    TileCol cols[kMaxTileCols];
    int32_t kinds[kMaxTileCols];    // sorted ascending, TK_NONE last
    int32_t P;                      // tiles per wave per span
    int64_t n_rows, n_tiles, n_spans;
    int64_t n_rounds;               // ceil(n_spans / grid)
    uint64_t *bitmap;
    unsigned long long *finish;     // the query's {total, n_emit, status, limit, tally, log ..., epoch} block
    unsigned long long *desc;       // n_spans span descriptors
    unsigned long long *round_total; // n_rounds inclusive totals through the round ...
    uint32_t *round_ctr;            // ... and n_rounds arrival counters (zero between runs).  At fixed places whatever P is: the host changes P between runs
    uint8_t *trash;                 // one 64-byte line per writer wave: where a dense range's unwanted lanes store (keeps its loop free of branches)
    uint64_t cap_rows;              // capacity of the output arrays
    uint32_t *row_index;
    void *pred_dst[kMaxTileCols];   // where the values of predicate column k go (packed, its width per row), or null: not in the SELECT list
    EmitCol gather[kMaxEmitGather]; // the other SELECT-list columns (and second mentions of a predicate column): gathered at the row
    int32_t n_gather;
    int32_t ablate;
    unsigned long long *stamps;     // diagnostics only
    unsigned long long *device_lock; // one word per device: the ticket of the launch of this kernel that owns the device, or 0
    // fault injection (imm3_diag.h, imm3_ctx_inject_fault): read only by the tools' build (IMM3_ABLATE); the shipped kernel carries none of it
    uint32_t max_polls;             // polls before a look-back wait gives up (0: kProjectMaxPolls)
    int32_t fault_wg, fault_span;   // work-group fault_wg never announces its fault_span-th span (-1: none)
    int32_t pad2;
    // table queries (imm3_table; the TABLE instances, imm3_project_table.hip): one descriptor per tile of the table's virtual row
    // space -- where the tile starts in each of the launch's columns and how many of its 1024 rows exist (1024 except the last tile
    // of each segment) -- replaces cols[k].data / n_rows.  Null for one segment.
    const ProjectTile *tile_desc;
};
// false: no instance for these kinds.  grid <= project_max_grid(): every work-group must be resident (they wait on each other)
bool launch_filter_project(const ProjectArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
bool launch_filter_project_table(const ProjectArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // a.tile_desc set
// the per-query tile descriptors of a table query, from the table's per-column tile pointers (null pointer: no such column)
void launch_project_tile_desc(const uint32_t *tile_rows, const void *const *p0, const void *const *p1, const void *const *p2, ProjectTile *out, int64_t n_tiles, hipStream_t s);
int project_max_grid(const int32_t *kinds, int P);   // resident work-groups of the instance on the current device (0: none)
int project_rec_dwords(const int32_t *kinds);

struct FilterArgs {
    ColPred cols[kMaxPredCols];
    int32_t ncols;
    int32_t and_existing;        // 1: AND into the bitmap already in memory (second pass for > kMaxPredCols columns)
    int64_t n_rows;              // uniform layout: rows of the segment
    int64_t n_words;             // bitmap words (batch-major)
    int64_t n_tiles;             // ceil(n_words / 16)
    uint64_t *bitmap;
    uint32_t *block_partials;    // selected rows per workgroup of this launch (no same-address atomics:
                                 // ~12 ns each, serialised -- 4096 of them cost 40 us on MI355X)
    // ragged layout only: per bitmap word, first row and number of valid rows (0..64)
    const uint32_t *word_row_base;
    const uint8_t *word_nvalid;
};

// ---- the one-column passes of the select chain: k_filter_str_rows, k_filter_str_range (imm3_strmatch.hip), k_filter_int_list
// (imm3_intlist.hip).  One wave per 1024-row tile, lane l on row 64 j + l; the tile's 16 bitmap words leave as one 128-byte line.
// What every such pass takes is the head below; what a kernel does with it is imm3_pass.h.
// (The order is measured, not taste: with the three row counts in front of the pointers, k_filter_str_rows<2, 2, false, false>
// -- whose eight values fill the scalar registers -- compiled to 20 bytes of scratch per lane, whatever code the kernel used.)
struct ColumnPassArgs {
    const void *data;                // flat (decoded) column in HBM, 16-byte aligned
    int32_t width;                   // bytes per row
    int32_t and_existing;            // 1: AND into the bitmap already in memory
    uint64_t *bitmap;                // allocated in whole tiles
    uint32_t *block_partials;
    // table queries: tile t holds tile_rows[t] valid rows starting at tile_ptrs[t] (as TileArgs); null for one segment
    const uint32_t *tile_rows;
    const void *const *tile_ptrs;
    int64_t n_rows, n_words, n_tiles;
};

// k_filter_str_rows: Match on one string column whose width is a whole number of dwords (pass.width: a multiple of 4, 4 .. 256)
constexpr int kStrPrefixDwords = 4;  // dwords of a row compared first; the rest only for the rows that pass (widths above 16 bytes)
struct StrRowsArgs {
    ColumnPassArgs pass;
    int32_t n_match;                 // IN-list size
    int32_t pad;
    uint32_t inl[kMaxMatch][2];      // values == null (width <= 8 and n_match <= kMaxMatch): the values' dwords, little-endian
    const uint32_t *values;          // else: n_match * width bytes in device memory (FoldedPred::d_blob)
};
bool str_rows_width_ok(int32_t width);            // a multiple of 4 in 4 .. 256
int str_rows_grid(int64_t n_tiles, int grid_blocks);
bool launch_filter_str_rows(const StrRowsArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // false: no instance for this width
// k_filter_str_range: lo' <= row <= hi' in byte order on one such column; k_filter_str_rows' grid
struct StrRangeArgs {
    ColumnPassArgs pass;
    uint32_t lo[kStrPrefixDwords];   // the first min(width, 16) bytes of lo' and hi', each dword's bytes swapped (its first byte most
    uint32_t hi[kStrPrefixDwords];   // significant): unsigned dword order is then byte order
    const uint32_t *tails;           // device memory: all width / 4 swapped dwords of lo', then of hi' (read for widths above 16 bytes only)
};
bool launch_filter_str_range(const StrRangeArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // false: no instance for this width

// k_filter_int_list: IMM3_INT_IN on one int32 / int8 column (pass.width: 4 or 1)
struct IntListArgs {
    ColumnPassArgs pass;
    int32_t form;                    // IntListForm (imm3_int_list_plan.h): selects the instance
    int32_t n_values;                // INT_LIST_ARGS: values in inl[]
    int32_t lo, hi;                  // the folded interval: the list's minimum and maximum
    union {
        int32_t inl[kMaxMatch];      // INT_LIST_ARGS: the values, the unused entries repeating the first
        uint32_t set[8];             // INT_LIST_I8: bit (uint8_t)v of the 256-bit membership set
    };
    const int32_t *table;            // INT_LIST_LDS / INT_LIST_GLOBAL: the probe table in device memory, mask + 1 slots
    uint32_t mask, shift, max_probe; // slots - 1 (INT_LIST_LDS: < kIntListLdsSlots), 32 - log2(slots), the step bound of every probe
    int32_t empty;                   // what an empty slot holds (never a member)
};
int int_list_grid(int64_t n_tiles, int grid_blocks, int32_t width);
bool launch_filter_int_list(const IntListArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // false: arguments no instance takes

// ---- integer sets built from selections (imm3_intset.hip): imm3_int_set_create's device passes; DESIGN.md §3d ----
// The header every pass reports through, one per build, in device memory (32-bit words; the host reads it whole)
enum IntSetHeaderWord : int {
    ISH_MIN = 0,        // int32: the smallest selected value (INT32_MAX before any)
    ISH_MAX = 1,        // int32: the largest (INT32_MIN before any)
    ISH_ROWS_LO = 2,    // the selected rows of all sources, 64 bits (ISH_ROWS_LO, + 1)
    ISH_COUNT0 = 4,     // values the insert pass placed in the scratch table
    ISH_PROBE0 = 5,     // ... the longest insertion distance + 1 there
    ISH_OVERFLOW = 6,   // != 0: a value found no free slot (more distinct values than the table was sized for)
    ISH_COUNT1 = 7,     // values the rehash placed in the final table
    ISH_PROBE1 = 8,     // ... the longest insertion distance + 1 there
    ISH_SET256 = 16,    // 8 words: bit (uint8_t)v per value in -128 .. 127
    ISH_WORDS = 24,
};
// one source: a query's select bitmap and one of its columns (flat, or through a table's tile pointers)
struct IntSetSource {
    const uint64_t *bitmap;
    int64_t n_words, n_rows;            // n_rows: uniform segment layouts (a word's valid rows)
    const void *data;                   // flat (decoded) column; null for a table
    const void *const *tile_ptrs;       // table: per-tile column pointers
    const uint32_t *tile_rows;          // table: valid rows per tile
    const uint32_t *word_row_base;      // ragged layouts: the first row of every bitmap word, else null
    const uint8_t *word_nvalid;         // ... and its valid rows
    int32_t width;                      // 4 (int32) or 1 (int8, sign-extended)
    int32_t has_skip, skip;             // has_skip: rows whose value is `skip` are passed over (the host route adds that value itself)
};
struct IntSetTable {
    int32_t *slots;                     // mask + 1 of them, a power of two
    uint32_t mask, shift;               // shift = 32 - log2(slots): int_list_home
    int32_t empty;                      // what a free slot holds: a value no source row has
};
void launch_int_set_init(uint32_t *header, hipStream_t s);
void launch_int_set_stats(const IntSetSource &src, uint32_t *header, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_int_set_fill(const IntSetTable &t, hipStream_t s);
// `cap`: the distinct values the build may hold; the pass raises the overflow flag as soon as its running count passes it, and leaves
void launch_int_set_insert(const IntSetSource &src, const IntSetTable &t, uint32_t cap, uint32_t *header, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// one pass over the slots of `from`: every value into `to` (to.slots == null: none -- the table stays) and the values in -128 .. 127 into the header's 256-bit set
void launch_int_set_rehash(const IntSetTable &from, const IntSetTable &to, uint32_t *header, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// ---- select trees (imm3_expr.hip): AND / OR over the leaves, as a disjunction of TERMS ----
// The host rewrites a tree into terms (imm3_expr_norm.cpp): each term is a conjunction with at most one folded predicate per column --
// exactly what a flat select list folds to -- and the selection is the OR of the terms.
constexpr int kMaxExprTerms = 8;         // terms the tile form carries in its kernel arguments
constexpr int kMaxExprGenericTerms = 64; // terms the generic form takes (its predicates sit in device memory)

// k_filter_expr<K0, K1, K2>: k_filter_tile's geometry (one wave per 1024-row tile, one 128-byte bitmap line per tile); the columns
// are loaded once per tile and tested once per term.  ~1.4 KB of kernel arguments.
// ExprTermArgs is what the single-segment instances take as their kernel arguments -- the terms and where the results go --
// and ExprTileArgs, what the host fills, adds the tile table the TABLE instances walk: the segment instances' argument block (and
// with it their code, down to the offsets of the implicit arguments behind it) does not know that tables exist.
struct ExprTermArgs {
    TileCol cols[kMaxExprTerms][kMaxTileCols]; // [t][k]: term t's predicate on tile column k (data: the same column in every term)
    uint32_t use[kMaxExprTerms];               // bit k: term t constrains tile column k (an unconstrained column is not tested)
    int32_t kinds[kMaxTileCols];               // sorted ascending, TK_NONE last (selects the template instance)
    int32_t n_terms;
    int64_t n_rows, n_words, n_tiles;
    uint64_t *bitmap;                          // null: count-only run -- no bitmap line is stored
    uint32_t *block_partials;
    unsigned long long *finish;                // the query's finish block: the count is reduced in the kernel; null = k_total does
};
struct ExprTileArgs : ExprTermArgs {
    // table queries (imm3_table; the TABLE instances): the tile table replaces cols[t][k].data / n_rows, exactly as in TileArgs.  Tile t
    // holds tile_rows[t] valid rows (1024 except the last tile of each segment) starting at tile_ptrs[k][t] in column k.  Null for one segment.
    const uint32_t *tile_rows;
    const void *const *tile_ptrs[kMaxTileCols];
};
static_assert(sizeof(ExprTileArgs) <= 2048, "ExprTileArgs travels as kernel arguments: keep it well under the 4 KiB limit");

// k_filter_expr_generic: any column kind, any layout, up to kMaxExprGenericTerms terms; one wave per bitmap word per iteration.
struct ExprGenericArgs {
    const ColPred *preds;          // device memory: the terms' predicates, term after term
    const int32_t *term_start;     // device memory: n_terms + 1 indices into preds
    int32_t n_terms;
    int32_t pad;
    int64_t n_rows, n_words, n_tiles;
    uint64_t *bitmap;
    uint32_t *block_partials;
    const uint32_t *word_row_base; // ragged layout only (as FilterArgs)
    const uint8_t *word_nvalid;
};
bool launch_filter_expr(const ExprTileArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // false: no instance for these kinds
void launch_filter_expr_generic(const ExprGenericArgs &a, bool negated, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // negated: a predicate with ColPred::negated among them

struct TotalArgs {               // k_total: sum of the filter launch's per-workgroup partials
    const uint32_t *block_partials;
    int32_t n_partials;
    int32_t pad;
    unsigned long long *total;   // selected rows of the segment
    unsigned long long *n_emit;  // rows ProjectOp emits = limit > 0 ? min(total, limit) : total
    int64_t limit;
};

struct ScanArgs {
    const uint64_t *bitmap;      // allocated in whole tiles, zero past n_words
    uint32_t *tile_offsets;      // exclusive prefix of the per-tile survivor counts WITHIN its chunk
    uint32_t *chunk_sums;        // selected rows per chunk of kChunkTiles tiles
    int64_t n_tiles;
    unsigned long long *finish;  // the query's {total, n_emit, status, limit, tally, log ...} block when THIS kernel publishes the count, else null
    const unsigned long long *scanned_tiles; // a limit scan stopped early: tiles [0, *scanned_tiles) hold this run's bitmap lines, the rest count as empty; null: all
    // A records run that stored NO bitmap (round 5): a tile's survivors = the length of its piece of its wave's arena, read from the
    // staging launch's start table (one more entry per wave holds the arena's end) through the launch geometry, as k_emit finds it.
    const uint32_t *rec_tile_start;          // null: the counts come from the bitmap
    int64_t rec_n_waves, rec_main_tiles;
    int32_t rec_max_slots, rec_T;
};

struct ProjCol {
    const void *src;             // flat column
    void *dst;                   // packed output, width bytes per emitted row
    const void *staged;          // survivors' values staged per tile by the filter kernel (width 4 or 1), or null
    const void *const *tile_ptrs; // table queries: per-tile pointer into this column (src unused), else null
    int32_t width;
    int32_t pad;
};

struct GatherArgs {
    const uint64_t *bitmap;
    const uint32_t *tile_offsets;
    const uint32_t *chunk_sums;
    int64_t n_tiles;
    int64_t n_words;
    int64_t limit;               // <= 0: unlimited
    uint64_t cap_rows;           // capacity of the output buffers
    uint32_t *row_index;         // segment-global row of each emitted row
    ProjCol proj[kMaxProj];
    int32_t n_proj;
    int32_t pad;
    int64_t n_staged_tiles;        // tiles [0, n) have staged values (the full tiles)
    const uint32_t *word_row_base; // ragged layout, else null
    const uint32_t *tile_rows;     // table queries: valid rows per tile (staged iff 1024), else null
    const unsigned long long *scanned_tiles; // a limit scan stopped early: only spans below *scanned_tiles are walked; null: all
};

// k_limit_gather: the offsets scan and the gather of a SMALL `limit` in one launch, over the tiles a limit scan got to.
constexpr int kLimitGatherMaxChunks = 64;   // chunks of 256 tiles per work-group at most (the launch has one work-group per CU)
constexpr int64_t kLimitGatherMaxRows = 4096;
constexpr uint32_t kLimitGatherMaxPolls = 1u << 18; // look-back polls (with s_sleep 4, ~0.5 us each) before the launch gives its rows up
struct LimitGatherArgs {
    const uint64_t *bitmap;
    unsigned long long *finish;        // [kFinishLimitTiles] = tiles scanned, [kFinishEpoch] = the run's tag; [kFinishLimitGaveUp] is written
    unsigned long long *wg_state;      // [grid]: (tag << 40) | survivors of the work-group's tiles
    int64_t n_tiles;
    int64_t limit;
    uint64_t cap_rows;
    uint32_t *row_index;
    ProjCol proj[kMaxProj];
    int32_t n_proj;
    int32_t fault_wg;                  // tools' build (-DIMM3_ABLATE, imm3_ctx_inject_fault): this work-group never publishes its count (-1: none)
    uint32_t max_polls, pad;           // tools' build: the poll cap (0: kLimitGatherMaxPolls)
};

// launchers (imm3_kernels.hip)
// ---- group-by aggregation (imm3_agg.hip) ----
constexpr int kMaxGroupCols = 4;
constexpr int kMaxAggs = 4;
enum AggKind : int32_t { AGG_COUNT = 0, AGG_MIN = 1, AGG_MAX = 2, AGG_SUM = 3, AGG_COUNT_DISTINCT = 5 }; // SUM: exact int64 over int32 / int8 columns
// COUNT_DISTINCT: no fold in the aggregation launch -- k_distinct_mark fills AggCol::dset behind it and counts into the value table
// The kernel forms of the aggregation, fastest first (imm3_agg.hip).  A query starts at AGG_FORM_LANES; a form whose
// per-work-group table cannot hold the query's keys raises the overflow word (3: a lanes form, 2: direct / tile) and the
// host aggregates again from the next form, remembering it in the query handle.
enum AggForm : int32_t { AGG_FORM_LANES = 0, AGG_FORM_LANES_WIDE = 1, AGG_FORM_DIRECT = 2, AGG_FORM_TILE = 3, AGG_FORM_GENERAL = 4 };
constexpr int kMaxDevices = 64; // per-device launch state (dynamic-LDS limits raised)

struct GroupCol {
    const void *data;
    const void *const *tile_ptrs; // table queries: per-tile pointer, else null
    int32_t width;
    int32_t shift;               // byte position of this column inside the u64 group key
};

struct AggCol {
    const void *data;
    const void *const *tile_ptrs; // table queries: per-tile pointer, else null
    int32_t width;
    int32_t kind;                // AggKind
    int32_t is_str;              // AGG_MAX over a string column: values compared as big-endian-packed bytes
    int32_t pad;
    // AGG_MAX over a string column wider than 8 bytes (else null): the aggregation launch folds the first 8 bytes and marks the
    // rows that may hold the maximum in `alive` (a bitmap the size of the selection's); refine pass k = 1 .. ceil(width / 8) - 1
    // keeps the rows whose chunk k - 1 equals the group's and folds chunk k into chunks[k - 1][slot] (mask + 2 slots per chunk)
    unsigned long long *chunks;
    uint64_t *alive;
    // AGG_COUNT_DISTINCT (else null): the exact set of (group, value) pairs, dset_mask + 1 open-addressing entries of
    // slot << 32 | the value's raw bytes, ~0 = empty (a slot is <= 2^27: no entry is the empty marker).  Cleared before every run.
    unsigned long long *dset;
    uint32_t dset_mask, pad2;
};
constexpr int kStrMaxWidth = 256; // widest string MAX (IMM3_STRING_MAX_WIDTH)

// SelectOp fused into the aggregation (k_group_agg_lanes' FUSED instances): ProjectAggIterator walks the selected positions of the
// batch it is handed (ProjectAggregate.scala:158-177); with the predicates evaluated on the rows the aggregation kernel already holds
// there is no bitmap to store and to read back, and a column that is both predicate and aggregate is read once.
constexpr int kMaxAggPreds = 2;
struct AggPred {
    const void *data;            // flat column (int8 or int32), or null: the predicate is on the value aggregate's own column (share = 1)
    int32_t width;               // 1 or 4
    int32_t lo, hi;              // closed interval (int8 values sign-extended)
    int32_t share;               // 1: the rows are the first value aggregate's, already in registers
};
struct AggArgs {
    const uint64_t *bitmap;
    int64_t n_words, n_tiles, n_rows;
    const uint32_t *word_row_base; // ragged layout, else null
    GroupCol groups[kMaxGroupCols];
    AggCol aggs[kMaxAggs];
    int32_t n_group, n_agg;
    int32_t first_form;          // AggForm: where the chain of kernel forms starts for this query
    int32_t ablate;              // read only by the tools' build (IMM3_ABLATED); 0 otherwise
    AggPred fused[kMaxAggPreds]; // n_fused > 0: the select chain, evaluated by the aggregation kernel itself (no bitmap is read)
    int32_t n_fused;
    int32_t fused_all;           // 1: no predicate at all -- every row of the segment is selected (n_fused == 0, no bitmap either)
    // global open-addressing table: mask + 1 slots, plus one for the all-ones key
    unsigned long long *keys;
    uint32_t *first;             // first (lowest) selected row of the group
    unsigned long long *counts;
    long long *vals;             // kMaxAggs per slot
    uint32_t mask;
    uint32_t out_cap;
    uint32_t *n_groups;
    uint32_t *overflow;
    // dense output of k_group_collect
    unsigned long long *out_keys;
    uint32_t *out_first;
    unsigned long long *out_counts;
    long long *out_vals;
    // group key wider than 8 bytes (wide_key = 1; only the general kernel's KEYW instance): a table's u64 is a TAG, hash32 << 32 |
    // rep_row, and the key bytes are read from the group columns at rep_row.  GroupCol::shift is not used then.
    int32_t wide_key;
    uint32_t hash_mask;          // hash32 &= hash_mask: all ones, or a few bits under TV_AGG_WEAK_HASH (collisions by construction)
};
constexpr int kGroupKeyMaxWidth = 256; // widest group key of the wide entry points (IMM3_GROUP_KEY_MAX_WIDTH)

int launch_group_agg(const AggArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // returns the AggForm it launched
bool group_agg_fuses_select(const AggArgs &a); // would launch_group_agg run a form that evaluates a.fused[] itself (no select launch needed)?

// ---- cross-segment / cross-GPU merge of group tables (ProjectAggregateQueueOp, ProjectAggregateQueue.scala:9-55) ----
// Keys of <= 2 bytes index a DIRECT table (256 or 65 536 slots; one slot for no group column): every query's dense group
// list is scattered into it with 64-bit atomics (counts add, first = min of segment << 32 | row, values max / min), and the
// tables of the ranks then meet in element-wise all-reduces (imm3_merge_groups.cpp).  SUM columns add (64-bit atomics, ncclSum).
struct MergeArgs {
    const unsigned long long *keys;   // one query's dense groups (k_group_collect's output)
    const uint32_t *first;
    const unsigned long long *counts;
    const long long *vals;            // kMaxAggs per group
    uint32_t n_groups;
    uint32_t slots;                   // K
    unsigned long long seg_hi;        // the query's segment index << 32
    unsigned long long *t_counts;     // [K]
    unsigned long long *t_first;      // [K], ~0 = empty
    long long *t_vals;                // [kMaxAggs][K]
    int32_t n_agg;
    int32_t kinds[kMaxAggs];          // AggKind
    int32_t is_str[kMaxAggs];         // MAX over strings: unsigned compare of the big-endian-packed bytes
    // keys wider than 2 bytes: the table is a hash table -- t_keys[slots] (open addressing, linear probing; slots = mask + 2, the
    // last slot is the one key that equals the empty marker), sized >= 2 x the entries that can arrive: it cannot fill up
    unsigned long long *t_keys;       // null: direct-indexed (slot = key)
    uint32_t mask;
    // packed lists (kMergeListWords u64 words per entry: key, first, count, kMaxAggs values; count 0 = padding): what the ranks
    // exchange with ncclAllGather and what the collect kernel writes
    const unsigned long long *list;   // k_merge_insert_list: n_groups entries
    unsigned long long *out_list;     // k_merge_collect_list: occupied slots, in no particular order ...
    unsigned long long *out_n;        // ... and how many (starts at 0)
    uint32_t out_cap;
};
constexpr int kMergeListWords = 3 + kMaxAggs;
void launch_merge_init(const MergeArgs &a, hipStream_t s);
void launch_merge_scatter(const MergeArgs &a, hipStream_t s);
void launch_merge_insert_list(const MergeArgs &a, hipStream_t s);
void launch_merge_collect_list(const MergeArgs &a, hipStream_t s);
// ---- the merge by BYTE key (imm3_comm_merge_groups_wide): group keys of 0 .. kGroupKeyMaxWidth bytes, string maxima of any width ----
// One fixed-stride RECORD of u64 words per (query, group), written once by k_mergew_pack and never changed:
//   [0] segment << 32 | first row   [1] count (0 = padding)   [2 .. 2 + kMaxAggs) values
//   [kMergeWideHead .. + key_words) the key bytes, zero-padded to 8   then, per string MAX wider than 8 bytes, its bytes zero-padded to 8
// The records are the hash table's input, the ncclAllGather payload and the collect kernel's output.  A table slot holds the INDEX
// of the record that claimed it (32-bit compare-and-swap from kMergeWideEmpty, which no index can be: entries <= 2^30); a later
// arrival compares its key with the claimant's record -- immutable input, so there is no half-published key to read and no key value
// is reserved.  Per wide string MAX a slot holds the index of the record with the greatest string so far (compare-and-swap loop).
constexpr int kMergeWideHead = 2 + kMaxAggs;
constexpr uint32_t kMergeWideEmpty = 0xFFFFFFFFu;
struct MergeWideArgs {
    int32_t rec_words, key_words, key_bytes, n_agg;
    int32_t kinds[kMaxAggs];           // AggKind
    int32_t is_str[kMaxAggs];          // MAX over strings: values[j] compares unsigned (the first <= 8 bytes packed big-endian)
    int32_t str_off[kMaxAggs];         // word offset of aggregate j's wide string in the record, 0: none
    int32_t str_words[kMaxAggs];       // its words
    int32_t str_width[kMaxAggs];       // its bytes
    int32_t best_plane[kMaxAggs];      // which plane of t_best is aggregate j's, -1: none
    // k_mergew_pack: one query's dense groups (k_group_collect's output) -> n_groups records at rec_out
    const unsigned long long *q_keys;  // the u64 keys (a key of <= 8 bytes; else q_key_bytes)
    const uint8_t *q_key_bytes;        // launch_group_keys' output, key_bytes per group (a key wider than 8 bytes)
    const uint32_t *q_first;
    const unsigned long long *q_counts;
    const long long *q_vals;           // kMaxAggs per group
    const uint8_t *q_str[kMaxAggs];    // launch_strmax_collect's output, str_width[j] per group (wide string maxima)
    uint32_t n_groups;
    unsigned long long seg_hi;         // the query's segment index << 32
    unsigned long long *rec_out;
    // the table: slots = mask + 1, a power of two >= 2 x the records that can arrive
    uint32_t *t_claim;                 // [slots] record index of the slot's key, kMergeWideEmpty = free
    unsigned long long *t_counts;      // [slots]
    unsigned long long *t_first;       // [slots]
    long long *t_vals;                 // [kMaxAggs][slots]
    uint32_t *t_best;                  // [planes][slots] record index of the greatest wide string so far, kMergeWideEmpty = none
    uint32_t slots, mask;
    // k_mergew_insert: n_recs records at recs (count 0: padding of the all-gather slots, skipped)
    const unsigned long long *recs;
    uint32_t n_recs;
    // k_mergew_collect: the occupied slots as records, in no particular order, and how many (starts at 0)
    unsigned long long *out_recs;
    unsigned long long *out_n;
    uint32_t out_cap;
};
void launch_mergew_pack(const MergeWideArgs &a, hipStream_t s);
void launch_mergew_init(const MergeWideArgs &a, hipStream_t s);
void launch_mergew_insert(const MergeWideArgs &a, hipStream_t s);
void launch_mergew_collect(const MergeWideArgs &a, hipStream_t s);
void launch_group_collect(const AggArgs &a, hipStream_t s);
// string MAX wider than 8 bytes (AggCol::chunks / alive): zero every such aggregate's alive bitmap and chunk table (before the
// aggregation launch); refine pass k of aggregate j; the exact values of aggregate j's groups, `width` bytes per dense group
// (k_group_collect's order: after it)
void launch_strmax_init(const AggArgs &a, hipStream_t s);
void launch_strmax_refine(const AggArgs &a, int j, int k, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_strmax_collect(const AggArgs &a, int j, uint32_t n_groups, uint8_t *out, hipStream_t s);
// AGG_COUNT_DISTINCT aggregate j (AggCol::dset, cleared): one walk of the select bitmap behind the aggregation launch; every pair's
// first arrival adds 1 to vals[slot][j]
void launch_distinct_mark(const AggArgs &a, int j, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// wide keys: the packed key bytes (the group columns' raw bytes in order, key_bytes per group) of every dense group, read at its
// first row (k_group_collect's order: after it)
void launch_group_keys(const AggArgs &a, uint32_t n_groups, int key_bytes, uint8_t *out, hipStream_t s);

constexpr int kSubTallies = 32;                       // in-kernel count reduce: sub-tallies (finish_add, imm3_device.h)
constexpr int kFinishWords = 16 + kSubTallies * 16;   // u64 words of a query's `finish` block: header (15 used, padded to a 128-byte line) + one line per sub-tally
constexpr int kFinishLimitTicket = 16 + 16 * (kSubTallies - 1) + kFinishLimitTicketLineWord; // finish[520]: claims handed out so far in this launch (zero between runs)
static_assert(kFinishLimitTicket < kFinishWords && kFinishLimitTicketLineWord > 0 && kFinishLimitTicketLineWord < 16, "the ticket word lies inside the finish block, beside the last sub-tally");
constexpr int kMaxFilterGrid = 4096; // capacity of block_partials
// what every launch_filter_* of a one-column pass asks of the head: a bitmap, a grid block_partials can hold, and a column -- flat
// data, or a complete tile table
inline bool column_pass_ok(const ColumnPassArgs &p, int grid) {
    if (!p.bitmap || grid < 1 || grid > kMaxFilterGrid) return false;
    return p.tile_rows ? p.tile_ptrs != nullptr : p.data != nullptr;
}
int filter_grid(int64_t units, bool generic, bool any_i32, int grid_blocks, int narrow_row_bytes = 0, bool lone_plane = false); // narrow_row_bytes: bytes per row of a launch without an int32 column; lone_plane: it is the lone TK_H16 column
// ev0/ev1: optional events stamped with the kernel's own start/end (hipExtLaunchKernelGGL), else null
// ---- PFOR_INT blocks (imm3_codec.hip) ----
struct PforArgs {
    const uint8_t *data;          // the column's .dat bytes in HBM (blocks start on 4-byte boundaries)
    const uint32_t *block_off;    // n_blocks + 1 byte offsets
    const uint32_t *row_base;     // decode: n_blocks + 1 first rows (prefix sum of the blocks' value counts)
    int64_t n_blocks;
    int32_t lo, hi;               // filter: closed interval
    int32_t and_existing;
    int32_t pad;
    int64_t n_rows, n_words, n_tiles;
    uint64_t *bitmap;
    uint32_t *block_partials;
    int32_t *out;                 // decode: dense int32 column
    uint32_t *status;             // bit 0 set when a block is malformed
};
// k_hi16_build (imm3_kernels.hip): dst[i] = (int16_t)(src[i] >> 16) for i < n_rows; min_max = {smallest, largest} half (the caller
// starts them at {32767, -32768})
void launch_hi16_build(const int32_t *src, int16_t *dst, int64_t n_rows, int32_t *min_max, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_pfor_counts(const uint8_t *data, const uint32_t *block_off, int64_t n_blocks, int32_t *counts, hipStream_t s);
void launch_filter_pfor(const PforArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_pfor_decode(const PforArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// ---- snappy-coded blocks (imm3_snappy.hip) ----
struct SnappyArgs {
    const uint8_t *data;          // the column's .dat bytes in HBM (blocks start on any byte)
    const uint32_t *block_off;    // n_blocks + 1 byte offsets
    const uint32_t *row_base;     // n_blocks + 1 first rows
    const uint32_t *xpow8;        // 32769 entries: x^(8 n) mod the CRC-32C polynomial, reflected
    int64_t n_blocks;
    int32_t width;                // bytes per value of the decoded column
    int32_t in_cap, out_cap;      // LDS bytes for the staged block / one chunk
    int32_t pad;
    uint8_t *out;                 // dense column
    uint32_t *status;             // bit 0 set when a block is malformed or a checksum does not match
};
void launch_snappy_sizes(const uint8_t *data, const uint32_t *block_off, int64_t n_blocks, uint32_t *sizes, uint32_t *max_chunk, hipStream_t s);
void launch_snappy_decode(const SnappyArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// k_sum_counts: the selected-row counts of up to kMaxSumCounts queries (device words) -> one device word; the send buffer
// of the RCCL count all-reduce (imm3_comm.cpp)
constexpr int kMaxSumCounts = 32;
struct SumCountsArgs {
    const unsigned long long *src[kMaxSumCounts];
    int32_t n;
    int32_t accumulate;          // 1: add to *dst instead of overwriting it (more than kMaxSumCounts queries)
    unsigned long long *dst;
};
void launch_sum_counts(const SumCountsArgs &a, hipStream_t s);

bool launch_filter_tile(const TileArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
bool launch_filter_table_limit(const TileArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // a.tile_rows, a.bitmap and a.finish set; false: no instance for these kinds
int filter_tile_group(const int32_t *kinds); // tiles per wave iteration of the instance for these kinds (0: none)
void launch_filter_generic(const FilterArgs &a, int grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_total(const TotalArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_read_stream(const int32_t *data, int64_t n_tiles, int32_t *sink, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_scan(const ScanArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_gather(const GatherArgs &a, int grid_blocks, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_limit_gather(const LimitGatherArgs &a, int grid_blocks, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// ---- ORDER BY (imm3_order.hip): a stable LSD radix sort of (normalised key, permutation) behind the projection, with an exact
// radix select in front of it for a top-k.  Every launch has the same fixed geometry -- kOrderWaves waves, each owning ONE contiguous
// piece of the rows -- and takes the row count from a device word, so the host enqueues the whole order without knowing it. ----
constexpr int kOrderMaxKeys = 4;
constexpr int kOrderKeyMaxBytes = 16;
constexpr int kOrderKeyWords = kOrderKeyMaxBytes / 4;
constexpr int kOrderWaves = 1024;                       // waves of every order launch = "blocks" of the (digit, block) count table
constexpr int kOrderBlockThreads = 256;
constexpr int kOrderGrid = kOrderWaves * 64 / kOrderBlockThreads;
constexpr int64_t kOrderSweepRows = (int64_t)kOrderWaves * 64; // rows one step of all waves covers: above it a wave walks its piece in several steps
constexpr int kOrderSelectFactor = 4;                   // the select runs when survivors >= this x limit
// the order's device words (uint32): written by k_order_plan and k_order_find, read by every launch behind them
enum OrderWord : int {
    OW_N = 0,        // rows the projection emitted (clamped to the arrays' capacity)
    OW_N_SORT = 1,   // rows the sort passes move: OW_N, or `limit` behind the select
    OW_N_OUT = 2,    // rows of the ordered result, min(OW_N, limit); OW_N_OUT + 1 stays 0: the pair reads as one uint64
    OW_ACTIVE = 4,   // bit p set: key byte p (0 = most significant) differs between rows -- its pass moves something
    OW_SELECT = 5,   // 1: the radix select compacts the candidates first
    OW_NEED = 6,     // select: rows still wanted among those that match the threshold's bytes found so far
    OW_THR = 8,      // 4 words: the threshold key, found byte by byte
    OW_KEY0 = 12,    // 4 words: the first row's key (what a byte position that never differs holds)
    OW_WORDS = 16,
};
struct OrderKeyCol {
    const uint8_t *src;  // the projected (unordered) column, width bytes per row
    int32_t width;
    int32_t kind;        // KIND_I32 / KIND_I8 / KIND_STR
    int32_t descending;
    int32_t pad;
};
struct OrderArgs {
    const unsigned long long *n_emit; // the projection's row-count word
    uint64_t cap_rows;                // capacity of the row arrays (a run that outgrew them is ordered again once settled)
    int64_t limit;                    // <= 0: none
    OrderKeyCol cols[kOrderMaxKeys];
    int32_t n_cols, key_bytes, key_words, force_full;
    uint32_t *keys[2];                // ping-pong: key word w of row i at keys[b][w * cap_rows + i], word 0 most significant
    uint32_t *perm[2];
    uint32_t *state;                  // OrderWord
    uint32_t *counts;                 // 256 x kOrderWaves: [digit][wave] counts, scanned in place to first positions
    uint32_t *diff;                   // kOrderWaves x 4: OR of key ^ first key per wave
    uint32_t *tally;                  // kOrderWaves x 2: select: {rows below the threshold, rows equal to it} per wave; then {first output, equal rows before}
    int32_t byte_pos, pad;            // the key byte this launch works on
};
struct OrderApplyCol {
    const uint8_t *src;
    uint8_t *dst;
    int32_t width, pad;
};
struct OrderApplyArgs {
    const uint32_t *perm[2];
    const uint32_t *state;
    int32_t key_bytes, n_cols;
    const uint32_t *row_index;        // null: the columns only (a later group of a wide SELECT list)
    uint32_t *row_index_out;
    OrderApplyCol cols[kMaxProj];
};
void launch_order_keys(const OrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);   // k_order_keys + k_order_plan
void launch_order_select(const OrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // the radix select: per key byte count + find, then offsets, compact
void launch_order_pass(const OrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);   // one LSD pass on a.byte_pos: count, scan, scatter
void launch_order_apply(const OrderApplyArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// ---- merging ordered results (imm3_merge_order.hip; the record: imm3_merge_order.h): every ordered row of every query becomes one
// record whose first six words are its sort key; sorted lists of records are merged by ranking each record in the other lists. ----
struct MergeOrderPackCol {
    const uint8_t *src;  // an ORDERED SELECT-list column, width bytes per row
    int32_t width;
    int32_t rec_off;     // word offset of its bytes in a record
};
struct MergeOrderPackArgs {
    OrderKeyCol keys[kOrderMaxKeys]; // src: the ordered key columns (the key is built again from them: imm3_order_key.h)
    int32_t n_keys, key_bytes;
    int32_t with_key;                // 1: this launch writes the six key words (the first column group of a long SELECT list)
    int32_t n_cols;
    const uint32_t *row_index;       // the query's ordered row indices (a table query: virtual rows)
    uint32_t n_rows;                 // host-known: the grid is sized from it
    uint32_t segment;                // a segment query's global segment
    int32_t n_tsegs, rec_words;      // table query: segments of its table (0: a segment query)
    const uint32_t *tile_start;      // table query: n_tsegs + 1 first tiles
    const uint32_t *global_index;    // table query: the global segment of each table segment
    MergeOrderPackCol cols[kMaxProj];
    uint32_t *recs;                  // record i of this query at recs + i * rec_words
};
// a table query whose global indices are not ascending: its records (in list order) cut into one sorted list per table segment
struct MergeOrderSplitArgs {
    const uint32_t *src;               // the query's n_rows records, in the query's order
    uint32_t *dst;                     // the merge's input buffer
    unsigned long long dst_word;       // word offset of this query's first record there
    uint32_t n_rows;
    int32_t n_tsegs, rec_words, pad;
    const uint32_t *global_index;      // n_tsegs
    uint32_t *counts;                  // n_tsegs: rows of each table segment (written by the count launch)
    unsigned long long *lists;         // this query's n_tsegs entries of the list table, written by the move launch
};
struct MergeOrderArgs {
    const uint32_t *recs;              // the input lists
    unsigned long long buf_words;      // words of `recs`: a list that would reach past them counts as empty
    const unsigned long long *lists;   // list l = {word offset of its first record in recs, records}; unused when slot_words != 0
    unsigned long long slot_words;     // != 0: the gathered form -- list l's length is the uint64 at word l * slot_words, its records follow
    int32_t n_lists, rec_words;
    uint32_t list_cap;                 // no list is longer (host-known): ceil(list_cap / 64) waves per list
    uint32_t cut;                      // records whose place is below it are stored
    uint32_t *out;                     // room for `cut` records
    unsigned long long *out_total;     // the lists' lengths summed
};
void launch_merge_order_pack(const MergeOrderPackArgs &a, hipStream_t s);
void launch_merge_order_split(const MergeOrderSplitArgs &a, hipStream_t s); // count + move
void launch_merge_order_rank(const MergeOrderArgs &a, hipStream_t s);

} // namespace imm3

// ---- ORDER BY over groups (imm3_group_order.hip; the key layout: imm3_group_order_plan.h): the dense groups of a settled aggregation
// ordered by a normalised key of 5 .. 16 bytes (the user's keys, then first_row) into dense arrays of their own.  The host knows the
// group count behind the settle and picks the path: one launch of one work-group up to kGroupOrderSmall groups, above it the radix
// sort / select of imm3_order.hip over the keys written as ONE byte-string column. ----
#include "imm3_group_order_plan.h"
namespace imm3 {
// Groups the one-work-group path takes.  Its keys and indices live in static LDS as structure-of-arrays words: 4 key words + 1 index
// word = 20 bytes per group, 2048 x 20 = 40 KiB of the 64 KiB a work-group may declare statically.
constexpr int kGroupOrderSmall = 2048;
constexpr int kGroupOrderSmallThreads = 1024;
enum GroupOrderPath : int32_t { GROUP_ORDER_NONE = 0, GROUP_ORDER_SMALL = 1, GROUP_ORDER_RADIX_FULL = 2, GROUP_ORDER_RADIX_SELECT = 3 };
struct GroupOrderArgs {
    GroupOrderLayout layout;
    uint32_t n;                          // dense groups (host-known: the settle has synchronised)
    uint32_t n_out;                      // min(n, limit)
    int32_t n_agg;
    int32_t key_bytes;                   // bytes of the packed group key
    int32_t wide_key;                    // 1: the packed key comes from src_keyb (out_keys holds tags), else from out_keys (little-endian)
    int32_t str_width[kMaxAggs];         // per aggregate with a wide string MAX: its width, else 0
    // the dense groups (k_group_collect's output), launch_group_keys' bytes of a wide key, launch_strmax_collect's of wide string maxima
    const unsigned long long *src_keys;
    const uint32_t *src_first;
    const unsigned long long *src_counts;
    const long long *src_vals;           // kMaxAggs per group
    const uint8_t *src_keyb;
    const uint8_t *src_str[kMaxAggs];
    // the ordered groups
    unsigned long long *dst_keys;
    uint32_t *dst_first;
    unsigned long long *dst_counts;
    long long *dst_vals;
    uint8_t *dst_keyb;
    uint8_t *dst_str[kMaxAggs];
    unsigned long long *dst_n;           // the ordered count, one 64-bit device word
    // radix path: the key column (layout.key_bytes per group), the group count as the 64-bit word the order launches read, and the
    // order's state and permutations (OrderArgs) for the gather behind the last pass
    uint8_t *key_col;
    unsigned long long *n_word;
    const uint32_t *perm[2];
    const uint32_t *state;
};
void launch_group_order_small(const GroupOrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_group_order_keys(const GroupOrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_group_order_apply(const GroupOrderArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
} // namespace imm3

// ---- HAVING (imm3_query_set_group_filter; the program and its evaluator: imm3_group_filter_plan.h): the FILTERED instances of the three
// kernels above, a second kernel argument beside GroupOrderArgs.  Small path: a dropped group becomes a pad of the bitonic network and
// the launch writes {min(kept, n_out), kept} to dst_n[0 .. 1].  Radix path: the keys kernel writes the kept groups' keys compacted (a
// wave ballot, one atomic add per wave on n_word, which the host zeroes on the stream first -- no work-group waits on another) and
// map[kept position] = dense index; the order launches read n_word = kept as always; the apply gathers through map[perm[i]]. ----
#include "imm3_group_filter_plan.h"
namespace imm3 {
struct GroupFilterArgs {
    GroupFilterProg prog;
    uint32_t *map;                       // radix path: kept position -> dense index, room for n
};
void launch_group_order_small_filtered(const GroupOrderArgs &a, const GroupFilterArgs &f, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_group_order_keys_filtered(const GroupOrderArgs &a, const GroupFilterArgs &f, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_group_order_apply_filtered(const GroupOrderArgs &a, const GroupFilterArgs &f, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
} // namespace imm3

// ---- views of MERGED groups (imm3_comm_merge_groups_view; imm3_merge_view.hip; the plan and the key builder: imm3_merge_view_plan.h):
// filter, then order, then limit over the record list a merge by byte key leaves on the device (MergeWideArgs::out_recs), into a list
// of n_out ordered records.  The two paths of the group order: one launch of one work-group up to kGroupOrderSmall records, above it
// a keys launch (plain, or filtered: compacted by one atomic add per wave on n_word, with map[kept position] = record index), the
// order launches of imm3_order.hip over the key column as ONE KIND_STR key, and an apply launch that gathers whole records. ----
#include "imm3_merge_view_plan.h"
namespace imm3 {
static_assert(kMergeViewAggs == kMaxAggs && kMergeViewHead == kMergeWideHead && kMergeViewKeyBytes == kOrderKeyMaxBytes, "imm3_merge_view_plan.h restates these");
struct MergeViewArgs {
    MergeViewPlan plan;
    const unsigned long long *recs;      // n records of plan.rec_words words
    uint32_t n;                          // host-known
    uint32_t n_out;                      // min(n, limit)
    unsigned long long *dst;             // room for n_out records
    unsigned long long *dst_n;           // {records of the view, records kept}
    // radix path (as GroupOrderArgs)
    uint8_t *key_col;
    unsigned long long *n_word;
    uint32_t *map;
    const uint32_t *perm[2];
    const uint32_t *state;
};
void launch_merge_view_small(const MergeViewArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
void launch_merge_view_keys(const MergeViewArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1); // (filtered: n_word zeroed on the stream first)
void launch_merge_view_apply(const MergeViewArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
} // namespace imm3

#ifdef __HIPCC__
#include <hip/hip_ext.h>
// Kernel launch with optional start / stop events stamped by the launch itself (hipExtLaunchKernelGGL); the plain launch
// when there are none: that is the one a stream capture (imm3_ctx_capture_begin) records.
#define IMM3_LAUNCH_LDS(kern, grid, block, lds, s, ev0, ev1, ...)                                                \
    do {                                                                                                         \
        if (ev0 || ev1) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, ev0, ev1, 0, __VA_ARGS__);  \
        else hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, __VA_ARGS__);                             \
    } while (0)
#define IMM3_LAUNCH(kern, grid, block, s, ev0, ev1, ...) IMM3_LAUNCH_LDS(kern, grid, block, 0, s, ev0, ev1, __VA_ARGS__)
// A one-column pass (ColumnPassArgs): launches kern<..., TABLE> on the launcher's (a, grid, s, ev0, ev1) -- the table instance when
// the pass has a tile table -- and returns true.  The variadic arguments are the kernel's template arguments in front of TABLE.
#define IMM3_COLUMN_PASS_LAUNCH(kern, ...)                                                                          \
    do {                                                                                                            \
        if (a.pass.tile_rows) IMM3_LAUNCH((kern<__VA_ARGS__, true>), grid, kBlockThreads, s, ev0, ev1, a);          \
        else IMM3_LAUNCH((kern<__VA_ARGS__, false>), grid, kBlockThreads, s, ev0, ev1, a);                          \
        return true;                                                                                                \
    } while (0)
#endif

