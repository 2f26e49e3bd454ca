// sspp_prof.h — profiling and debugging hooks of the kernels (sspp_kern.h).  Every macro here
// compiles to nothing by default; the -D switches are set by tools/build_variant.sh only, and the
// device arrays are read by tools/wg_timing.py, c2f_stats.py, tsp_stats.py and split_beacons.py.
#pragma once
#include <hip/hip_runtime.h>

#ifdef SSPP_TSP_STATS  // profiling builds only: point_collide's pair work (tools/tsp_stats.py)
__device__ unsigned long long g_tsp_stats[16];
#define TSP_STAT(i, c) do { const unsigned long long m_ = __ballot(c), a_ = __ballot(1);                  \
        if (__lane_id() == __builtin_ctzll(a_) && m_) atomicAdd(&g_tsp_stats[i], (unsigned long long)__popcll(m_)); } while (0)
#else
#define TSP_STAT(i, c) do { } while (0)
#endif
#ifdef SSPP_C2F_STATS  // profiling builds only (tools/build_variant.sh stats -DSSPP_C2F_STATS)
__device__ unsigned long long g_c2f_stats[16];
#define SSPP_CB_STAT(i) atomicAdd(&g_c2f_stats[i], 1ull)
#endif
#ifdef SSPP_WG_TIMING  // profiling builds only: per-workgroup (start, end, CU, survivors) of k_sspp_c2f
__device__ unsigned long long g_wg_t[1 << 18];
__device__ unsigned long long g_wg_ph[8 << 16];  // per workgroup: shader clock after each phase
#define WG_PH(k) do { if (threadIdx.x == 0 && blockIdx.x < (1 << 16)) g_wg_ph[8 * blockIdx.x + (k)] = clock64(); } while (0)
__device__ unsigned long long g_p2_t[8 << 12];  // split launch: [4095] the last arriver's epilogue (start, end, grid)
__device__ unsigned long long g_p2_w[8 << 13];  // split launch per queue slot: start, end (wall), passes, FP64 passes, feasible, p2/p3 clocks, wave
// k_sspp_c2f: the workgroup's wall-clock start and survivor count (declarations, at function scope),
// and its g_wg_t record (start, end, CU, NS) when it leaves
#define WG_T_BEGIN() const unsigned long long wg_t0 = wall_clock64(); int wg_ns = -1
#define WG_T_SURVIVORS(NS) wg_ns = (NS)
#define WG_T_NS ((unsigned long long)(long long)wg_ns)
#define WG_T_RECORD(TID, NS)                                             \
    do {                                                                 \
        if ((TID) == 0 && blockIdx.x < (1 << 16)) {                      \
            g_wg_t[4 * blockIdx.x] = wg_t0;                              \
            g_wg_t[4 * blockIdx.x + 1] = wall_clock64();                 \
            g_wg_t[4 * blockIdx.x + 2] = __smid();                       \
            g_wg_t[4 * blockIdx.x + 3] = (NS);                           \
        }                                                                \
    } while (0)
// the split launch's last workgroup: its epilogue's g_p2_t record (start, end, grid)
#define WG_EP_BEGIN() const unsigned long long t_ep = wall_clock64()
#define WG_EP_RECORD() do { g_p2_t[8 * 4095] = t_ep; g_p2_t[8 * 4095 + 1] = wall_clock64(); g_p2_t[8 * 4095 + 2] = gridDim.x; } while (0)
// surv_finish: one queued survivor's g_p2_w record (see g_p2_w) — clocks and pass counters declared
// at its start, the shader clock between phase 2 and phase 3, the record by thread 0
#define WG_SURV_BEGIN() const unsigned long long w_t0 = wall_clock64(), c0 = clock64(); unsigned w_np = 0, w_nf = 0
#define WG_SURV_PASS() ++w_np
#define WG_SURV_PASS64() ++w_nf
#define WG_SURV_P2_DONE() const unsigned long long c1 = clock64()
#define WG_SURV_RECORD(SLOT, FEAS)                                                           \
    do {                                                                                     \
        unsigned long long* t_ = g_p2_w + 8 * ((SLOT) & ((8u << 10) - 1u));                  \
        t_[0] = w_t0; t_[1] = wall_clock64(); t_[2] = w_np; t_[3] = w_nf; t_[4] = (FEAS);    \
        t_[5] = c1 - c0; t_[6] = clock64() - c1; t_[7] = blockIdx.x;                         \
    } while (0)
#else
#define WG_PH(k) do { } while (0)
#define WG_T_BEGIN() do { } while (0)
#define WG_T_SURVIVORS(NS) do { } while (0)
#define WG_T_NS 0ull
#define WG_T_RECORD(TID, NS) do { } while (0)
#define WG_EP_BEGIN() do { } while (0)
#define WG_EP_RECORD() do { } while (0)
#define WG_SURV_BEGIN() do { } while (0)
#define WG_SURV_PASS() do { } while (0)
#define WG_SURV_PASS64() do { } while (0)
#define WG_SURV_P2_DONE() do { } while (0)
#define WG_SURV_RECORD(SLOT, FEAS) do { } while (0)
#endif

#ifdef SSPP_C2F_STATS
#define C2F_STAT(i, v) do { const unsigned long long v_ = (v); if ((threadIdx.x & 63) == 0 && v_) atomicAdd(&g_c2f_stats[i], v_); } while (0)
#else
#define C2F_STAT(i, v) do { } while (0)
#endif

#ifdef SSPP_DEBUG_PROGRESS  // progress beacons of the split launch: plain stores into a [grid][8]
// buffer (device memory for timing; mapped host memory to watch a launch that does not finish)
#define SSPP_BEACON(B_PH, B_X, B_Y)                                                                              \
    do {                                                                                                        \
        if (q.beacon && threadIdx.x == 0) {                                                                     \
            q.beacon[8 * blockIdx.x + 1] = (unsigned)(B_X);                                                     \
            q.beacon[8 * blockIdx.x + 2] = (unsigned)(B_Y);                                                     \
            q.beacon[8 * blockIdx.x] = (unsigned)(B_PH);                                                        \
        }                                                                                                       \
    } while (0)
// wave 1's progress (thread 64) in the workgroup's fourth word
#define SSPP_BEACON1(B_PH)                                                                                      \
    do {                                                                                                        \
        if (q.beacon && threadIdx.x == 64) q.beacon[8 * blockIdx.x + 3] = (unsigned)(B_PH);                    \
    } while (0)
// the 100 MHz wall clock's low word at a workgroup event, word 4 + B_K of its record
#define SSPP_BEACON_T(B_K)                                                                                      \
    do {                                                                                                        \
        if (q.beacon && threadIdx.x == 0) q.beacon[8 * blockIdx.x + 4 + (B_K)] = (unsigned)wall_clock64();    \
    } while (0)
// the last workgroup's epilogue stages: word B_K after the grid's records
#define SSPP_BEACON_E(B_K)                                                                                      \
    do {                                                                                                        \
        if (q.beacon && threadIdx.x == 0) q.beacon[8 * gridDim.x + (B_K)] = (unsigned)wall_clock64();          \
    } while (0)
// (thread 0) the survivors this workgroup finished, in the workgroup's fourth word
#define SSPP_BEACON_FIN_DECL() unsigned nfin = 0
#define SSPP_BEACON_FIN(B_TID)                                                                                  \
    do {                                                                                                        \
        if ((B_TID) == 0 && q.beacon) q.beacon[8 * blockIdx.x + 3] = ++nfin;                                    \
    } while (0)
#else
#define SSPP_BEACON_FIN_DECL() do { } while (0)
#define SSPP_BEACON_FIN(B_TID) do { } while (0)
#define SSPP_BEACON(B_PH, B_X, B_Y) do { } while (0)
#define SSPP_BEACON1(B_PH) do { } while (0)
#define SSPP_BEACON_T(B_K) do { } while (0)
#define SSPP_BEACON_E(B_K) do { } while (0)
#endif
