// ta_sweep_switches.h -- every compile-time switch of the sweep (kernels_scan.hip, ta_sweep_common.h) in ONE place: what the product
// is built with (the defaults below), what experiments measured before they were deleted, and the instrumentation / ablation builds of
// scripts/build_variant.py (`python scripts/build_variant.py NAME -DTA_...` -> scratch/libNAME.so; never the product library).
// The switches are USED where the code they change lives; this header only names and documents them.
#pragma once

// ---- tuning: what the product runs with ---------------------------------------------------------------------------------
#ifndef TA_WAVES
#define TA_WAVES 4               // waves per workgroup, stacked along axis 1
#endif
#ifndef TA_PSLOTS
#define TA_PSLOTS 512            // pair-table slots per workgroup (<= 128 TA_WAVES: the flush takes two pairs a thread, flush_tables asserts it)
#endif
#ifndef TA_LSLOTS
#define TA_LSLOTS 128            // label-table slots per workgroup (<= 0.25 TA_PSLOTS: the flush stages 80 bytes a label in the pair table's 20 a slot)
#endif
#ifndef TA_FCAP
#define TA_FCAP 256              // face records a wave's buffer holds (the top-of-plane drain takes the LAST groups: nothing moves)
#endif
#ifndef TA_RCAP
#define TA_RCAP 128              // run records a wave's buffer holds (the drain takes the first 64, the rest moves to the front: <= 128)
#endif
#ifndef TA_FDRAIN
#define TA_FDRAIN 128            // faces in the buffer from which the top-of-plane drain takes two groups of 64 (the tiles of eight voxels
#endif                           // a lane: and one group from 64 on -- kernels_scan.hip, at its use)
#ifndef TA_XCD_CHUNK
#define TA_XCD_CHUNK 4           // consecutive tiles given to one XCD (0 = plain order).  Round 5: 8 .. 64 cut the HBM fetch by 2 .. 5 % and
#endif                           // cost 1 .. 12 % of time on C4 (tissue and background no longer mix over the XCDs); flat on C5
#ifndef TA_PLANES_CAP_ADJ8
#define TA_PLANES_CAP_ADJ8 32    // the tallest tile the kernels of eight voxels a lane pack their sums for (SumPack)
#endif
#ifndef TA_U16_VPL
#define TA_U16_VPL 8             // uint16 volumes with adjacency: 8 voxels a lane (125 VGPRs, four waves) or 4 (the uint32 kernel's shape, five
#endif                           // waves: faster only where cells are everywhere -- profiles/NOTES.md, round 4 section 7)
#ifndef TA_U16_MOM_RB
#define TA_U16_MOM_RB 2          // rows a wave of the moments-only uint16 kernel (512 columns each)
#endif

// ---- tried, measured, deleted (the code is in git history before the commit that removed these switches) -----------------
// Persistent workgroups on per-XCD tile queues for the narrow uint32 kernel (TA_PERSIST): 1.30 against 1.07 ms on C4 (round 4).
// A second landing zone, two planes in flight at 109 VGPRs and four waves (TA_PLANES_IN_FLIGHT = 2): slower (round 4).
// Two replicas of a label slot's sums by row parity (TA_LSUM_REP = 2): +4 % time.  A pair's three face counts in one u64 LDS
// word of 21-bit fields (TA_PCNT64): equal time, twice the cost per LDS atomic.  Gone with them: TA_LDS_PAD, TA_DBG_EMIT and
// TA_FLUSH_SCOPE (gfx950 encodes agent and workgroup scope alike: there was nothing to measure).
// Settled since (their switches are gone, the choice is code): what ships, and what the other path measured (profiles/NOTES.md; the wide
// kernel, C4 / tissue-filled, unless another volume is named).
//   Record stores predicated by the exec mask (v_cmpx).  Own offset or trash slot by selects: 0.987 / 1.354 against 0.958 / 1.300 ms.
//   A probe round = a compare-and-swap that returns nothing + a plain re-read.  A returning compare-and-swap: equal time.
//   Eight voxels a lane: the plane before a tile and its first plane in flight together.  One after the other: C5 6.79 against 6.63 ms.
//   The flush reads a label's global box and sends only the bounds its tile extends.  Six unconditional minima: filled 1.37 against 1.35 ms.
//   The flush sends a label's sums lane = (label, word).  Lane = label: 0.987 / 1.330 against 0.958 / 1.300 ms.
//   The hot label's private row per workgroup, also with adjacency.  Without: every tile's background on one global row (ta_sweep_common.h).
//   The top-of-plane drains: full groups, every lookup in flight together.  In-plane drains only: equal on C4, 2 - 3 % slower tissue-filled.
//   ... for the full tiles of uint16 volumes too (with the predicated stores, C2 0.137 -> 0.134 ms).  Without: 0.143 - 0.144 against 0.140 - 0.143 ms.
//   Eight voxels a lane: one group of 64 faces leaves at the top of a plane from 64 on.  From 128 on only: equal time, 29 % instead of 7 %
//   of C4's face records through the in-plane drain.
//   The global pair table is one array of 32-byte slots {key, f0, f1, f2}.  Keys u64[cap] and counts u64[cap][3] in two arrays: sweep
//   0.976 / 1.26 against 0.968 / 1.27 ms (inside the noise), the collect 0.027 / 0.037 against 0.021 / 0.027 ms (profiles/pair_slots_ab.txt).
//   The out-of-line label spill takes its sums and box in registers.  By pointer to a stack frame (112 bytes of scratch a lane in every
//   sweep kernel): equal time, 0.968 / 1.27 against 0.966 / 1.25 ms.

// ---- ablations (results WRONG by construction; only the time matters) and instrumentation ---------------------------------------
//   TA_ABLATE = 1 records produced and stored, nothing consumed; 2 = placed, not stored; 3 = not even placed
//   TA_ABL_HOT = 1 the top-of-plane drains add nothing to the tables; 2 ... and run no probe rounds; 3 ... and read no keys; 4 ... nor records
//   TA_ABL_NOFLUSH the tile tables are not flushed;  TA_ABL_NOFLUSH_PAIRS / TA_ABL_NOFLUSH_LABELS only one kind is
//   TA_ABL_NOSLOW the in-plane drains and the end of the tile consume nothing;  TA_ABL_NOHOT no top-of-plane drains
//   TA_ABL_NOFACE0 / TA_ABL_NOFACE1 no axis-0 / axis-1 face records;  TA_ABL_NOSUMS, TA_ABL_NOBOX, TA_ABL_NOBOXHOT, TA_ABL_NOPCNT, TA_ABL_NOLOOP,
//   TA_ABL_SHARE1 (every lane of an add its own address), TA_ABL_L2 (every plane re-reads the tile's first: an L2-resident run)
//   TA_ABL_NOHALO = 1 a workgroup's first wave reads no row above (the row another tile owns: 12.5 % of the bytes fetched); 2 = no wave does
//   TA_RECCOUNT   flags[8..12] = face / run records and calls through the in-plane drain, faces / runs through the top-of-plane drains
//   TA_BARSTAMP   flags[8..11] = cycles >> 8 over the waves: sweep of the tile, wait at the barrier before the flush, flush; wave-tiles
#ifndef TA_ABLATE
#define TA_ABLATE 0
#endif
#ifndef TA_ABL_HOT
#define TA_ABL_HOT 0
#endif
