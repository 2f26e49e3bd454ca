// sspp_knobs.h — the build-time tuning knobs of the kernels (sspp_kern.h), each with its default and
// the measurement behind it.  -DNAME=value (tools/build_variant.sh, A/B runs) overrides a default.
#pragma once

// k_tsp forms (bit f = form f) that run several sub-batches per workgroup (SSPP_OPT_TSP_REP)
#ifndef SSPP_TSP_REP_FORMS
#define SSPP_TSP_REP_FORMS (1 << 3)
#endif
#ifndef SSPP_SCORE_WAVES_PER_EU
#define SSPP_SCORE_WAVES_PER_EU 4  // min waves per SIMD (4 -> <=128 VGPRs; measured best on gfx950)
#endif

// ---- TaskSpacePlanner kernels (sspp_kern.h)
#ifndef SSPP_TSP_LEAN_GEOM
#ifdef SSPP_TSP_STATS  // (the statistics read the geom record at every pair)
#define SSPP_TSP_LEAN_GEOM 0
#else
#define SSPP_TSP_LEAN_GEOM 1
#endif
#endif
#ifndef SSPP_TSP_WAVES_PER_EU
#define SSPP_TSP_WAVES_PER_EU 3
#endif
#ifndef SSPP_TSP_WAVES_PER_EU_CB  // with the exact cylinder-box test (its live state doubles)
#define SSPP_TSP_WAVES_PER_EU_CB 2
#endif
// Several moving geoms (the gripper's 7): 3 waves per SIMD, 168 VGPRs with ~50 spilled, beats
// 2 waves without spills (multi-goal 40.6 against 34.6 M cand/s; 4 waves: 29.8)
#ifndef SSPP_TSP_WAVES_PER_EU_MG
#define SSPP_TSP_WAVES_PER_EU_MG 3
#endif
#ifndef SSPP_TSP_SUB_LAUNDER
#define SSPP_TSP_SUB_LAUNDER 1
#endif
// 4 waves per SIMD, no spills.  5 waves (96 VGPRs, ~75 spilled) measured 106.0 against 101.6 M
// cand/s on stacking, but its spills raised the HBM traffic from 1.4x to 140x the algorithmic bytes
#ifndef SSPP_TSP_WAVES_PER_EU_DEF
#define SSPP_TSP_WAVES_PER_EU_DEF 4
#endif

// ---- the split launch's survivor queue (sspp_kern.h)
// Ready-word ordering.  Every access to the queue's shared data (rows, ready words, counters)
// is an agent-scope atomic (global_load / global_store ... sc1: coherent across the XCDs, not
// held in a non-coherent cache level), and the protocol orders them with s_waitcnt: the producer
// waits for its row stores to complete (vmcnt(0), each thread, then the workgroup barrier)
// before it stores the ready word, and the consumer issues its row loads only after its load of
// the word has returned.  That is the hardware ordering of CDNA4 for sc1 accesses.  The C++
// release / acquire pair (SSPP_QUEUE_FENCES 1) compiles to buffer_wbl2 sc1 (write back this
// XCD's whole L2) before each word store and buffer_inv sc1 (invalidate it) after each word
// load: 49.4 -> 73.4 us per 20-step launch (profiles/r06d_*), for data that never passes
// through those caches.  It stays a build option (tools/runs, A/B); the default is the
// relaxed form.
#ifndef SSPP_QUEUE_FENCES
#define SSPP_QUEUE_FENCES 0
#endif
#if SSPP_QUEUE_FENCES
#define SSPP_QUEUE_RELEASE_ORDER __ATOMIC_RELEASE
#define SSPP_QUEUE_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#else
#define SSPP_QUEUE_RELEASE_ORDER __ATOMIC_RELAXED
#define SSPP_QUEUE_ACQUIRE() do { } while (0)
#endif
#ifndef SSPP_SPLIT_PRIO  // split launches: issue priority by phase (s_setprio; A/B: 0)
#define SSPP_SPLIT_PRIO 1
#endif
#ifndef SSPP_PRIO_ALL  // the same priorities in the unsplit instances (A/B)
#define SSPP_PRIO_ALL 0
#endif
#ifndef SSPP_SPLIT_PRIO_CONSUMER  // the priority of a wave past phase 1 (push, queued survivors)
#define SSPP_SPLIT_PRIO_CONSUMER 0
#endif
#ifndef SSPP_QUEUE_WAITERS  // tickets per shard that may wait for slots not reserved yet
#define SSPP_QUEUE_WAITERS 4
#endif
#ifndef SSPP_LINGER_SLEEP  // s_sleep between a waiting wave's polls (x 64 clocks)
#define SSPP_LINGER_SLEEP 16
#endif

// ---- k_sspp_c2f (sspp_kern.h)
#ifndef SSPP_CB_INLINE
#define SSPP_CB_INLINE __attribute__((noinline))
#endif
// Occupancy per shape: one- and two-wave workgroups of a single-geom mover at 5 waves per SIMD
// (96 VGPRs: 20 waves per CU, so the 20-step launch of 4096-candidate steps at 128 x 4 is one
// resident round); 4-wave workgroups and multi-geom movers at 4 (128 VGPRs; at 5 they spill).
// Round 6 (tools/kres.py, profiles/r06pmc_*): the robocrane d7 instances at 128 threads spill
// no VGPR, split and unsplit; the split one has no scratch at all (Registers).
#ifndef SSPP_C2F_WAVES_PER_EU
#define SSPP_C2F_WAVES_PER_EU 5
#endif
#ifndef SSPP_C2F_WAVES_PER_EU_WIDE
#define SSPP_C2F_WAVES_PER_EU_WIDE 4
#endif
// Workgroups of up to 128 threads run at SSPP_C2F_WAVES_PER_EU (96 VGPRs); the 256-thread
// latency shape carries the phase-2 pair groups (few survivor items over many lanes), which
// cost registers (at 5 waves per SIMD they spill), and runs at SSPP_C2F_WAVES_PER_EU_WIDE.
// profiling builds only (tools/build_variant.sh -DSSPP_ABLATE=mask): 1 no sampling, 2 no
// collision, 4 no arc, 8 no phase 2, 16 no phase 1, 64 return at entry (launch cost only)
#ifndef SSPP_ABLATE
#define SSPP_ABLATE 0
#endif
#ifndef SSPP_C2F_FIVE_MAX  // profiling builds: the largest workgroup at SSPP_C2F_WAVES_PER_EU
#define SSPP_C2F_FIVE_MAX 128
#endif
#ifndef SSPP_C2F_GP_NT     // profiling builds: the workgroup size that carries the pair groups
#define SSPP_C2F_GP_NT 256
#endif
// phase 2's hull masks, from this many pairs on: with 8 pairs or fewer the masks cull too little to
// pay for their two barriers and the hull pass: robocrane (4 pairs) kernel 54.9 -> 53.7 us at 20
// steps, 79.9 -> 78.1 us at 1000 (profiles/r04aa_mask_ab.txt); the scan tests every pair exactly
// either way
#ifndef SSPP_P2_MASK_MIN
#define SSPP_P2_MASK_MIN 9
#endif
