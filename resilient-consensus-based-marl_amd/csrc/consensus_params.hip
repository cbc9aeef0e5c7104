// K1 -- resilient consensus over the hidden-layer parameters of all agents.
//
// Replaces the reference's per-agent / per-layer Python loop
//   RPBCAC_agent.resilient_consensus_critic_hidden / _TR_hidden
//   (agents/resilient_CAC_agents.py:142-166) and the aggregation rule
//   RPBCAC_agent._resilient_aggregation (agents/resilient_CAC_agents.py:42-58)
// as called from training/train_agents.py:129-135.
//
// For every seed s, cooperative agent i and hidden parameter p < P_hid:
//   v_k   = msg[s][nbr[i][k]][p],  k = 0..d-1   (v_0 = the agent's own message)
//   lower = min(sorted(v)[H], v_0),  upper = max(sorted(v)[d-H-1], v_0)
//   theta[s][i][p] = (sum_k clamp(v_k, lower, upper)) / d
// Columns >= P_hid (output layer) and rows of non-cooperative agents are not
// written (the aggregated W3,b3 are discarded by the reference, :150-153).
//
// MI355X mapping: one workgroup owns one (seed, 64-column tile).  The tile of
// ALL N message rows is staged once into LDS with 16-B coalesced loads (each
// message row is read from HBM exactly once: compulsory traffic), then every
// lane owns one column and walks the agents; the neighbour list of an agent is
// wave-uniform (scalar loads), the d candidate values sit in VGPRs and the two
// order statistics come from a pruned min/max network (selnet_generated.inc).
// HBM roofline: 4*(P read + P_hid written) bytes per (seed, agent).
#include "rcmarl_common.h"
#include <stdlib.h>
#include "selnet_generated.inc"
#include "selmid_generated.inc"

namespace {

// x / D for a small integer constant D, bit-identical to the IEEE division in 3 instructions instead of ~10:
// q0 = x*rcp, one fma residual, one fma correction (Markstein).  Checked EXHAUSTIVELY over all 2^32 inputs for every
// D in 2..66 (tools/micro/check_div_const.c): the only mismatches have a subnormal quotient (|x| < 2.4e-38 * D), and
// the callers send |x| < 1e-30 to the true division on a wavefront-uniform branch (rc_any) that real weights never
// enter -- an if-converted IEEE division costs ~10 instructions per value.
template <int D>
__device__ __forceinline__ float rc_div_fast(float x) {
  constexpr float rcp = 1.0f / (float)D;
  const float q0 = x * rcp;
  return fmaf(fmaf(-q0, (float)D, x), rcp, q0);
}

// The clip window of one (agent, column) from the generated network: [min(sorted(v)[H], v_0), max(sorted(v)[D-H-1], v_0)].
// Shared by the aggregation below and by the clip-count kernel, so that both see the same bits.
template <int D, int H>
__device__ __forceinline__ void window_regs(const float (&v)[D], float& lower, float& upper) {
  float lo, hi;
  SelNet<D, H>::run(v, lo, hi);
  lower = fminf(lo, v[0]);
  upper = fmaxf(hi, v[0]);
}

// want_window: the caller stores lower/upper (debug outputs of the bit-exactness tests).  H == 0 (BASELINE configs[0],
// agents/resilient_CAC_agents.py:50-56 with H = 0): the window is [min, max] of the d values, clipping is the identity and
// the aggregate is the plain mean -- no selection network and no clamps unless the window itself is asked for.
template <int D, int H>
__device__ __forceinline__ float aggregate_regs(const float (&v)[D], float& lower, float& upper, bool want_window = true) {
  float sum = 0.f;
  if (H == 0) {
    lower = upper = v[0];
    if (want_window) window_regs<D, H>(v, lower, upper);
#pragma unroll
    for (int k = 0; k < D; ++k) sum += v[k];
  } else {
    window_regs<D, H>(v, lower, upper);
#pragma unroll
    for (int k = 0; k < D; ++k) sum += __builtin_amdgcn_fmed3f(v[k], lower, upper);  // clamp
  }
  float q = rc_div_fast<D>(sum);
  if (__builtin_expect(rc_any(fabsf(sum) < 1e-30f), 0)) {
    RC_NO_SPECULATE();
    q = sum / (float)D;
  }
  return q;
}

// Software-pipelined tile staging: a workgroup walks a strided sequence of (seed, column-tile)
// work items.  The [N][TC] image of the NEXT item is fetched into registers (up to PF float4 per
// thread, all issued back-to-back) while the current item is being aggregated out of LDS, and
// committed to LDS after the barrier that retires the current item.  ldp % 64 == 0, c0 % TC == 0.
constexpr int PF = 16;   // 256 threads x 16 float4 = 64 KiB = the largest tile image
struct TileStager {
  const float* msg; int N, ldp, log2tc, tiles_per_seed;
  __device__ __forceinline__ void fetch(int t, float (&pf)[4 * PF]) const {
    const int lq = log2tc - 2, total = N << lq;
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) << log2tc;
    const float* m = msg + (size_t)s * N * ldp + c0;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      int idx = threadIdx.x + 256 * u;
      idx = idx < total ? idx : total - 1;     // clamp instead of predicate: keeps pf[] in registers
      const float4 x = *reinterpret_cast<const float4*>(m + (size_t)(idx >> lq) * ldp + 4 * (idx & ((1 << lq) - 1)));
      pf[4 * u] = x.x; pf[4 * u + 1] = x.y; pf[4 * u + 2] = x.z; pf[4 * u + 3] = x.w;
    }
  }
  __device__ __forceinline__ void commit(const float (&pf)[4 * PF], float* tile) const {
    const int lq = log2tc - 2, total = N << lq;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int idx = threadIdx.x + 256 * u;
      if (idx < total) *reinterpret_cast<float4*>(tile + ((idx >> lq) << log2tc) + 4 * (idx & ((1 << lq) - 1))) =
            make_float4(pf[4 * u], pf[4 * u + 1], pf[4 * u + 2], pf[4 * u + 3]);
    }
  }
};

template <int D, int H>
__global__ __launch_bounds__(256) void k_consensus_params(const float* __restrict__ msg, float* __restrict__ theta,
                                                          const int* __restrict__ nbr,
                                                          const int* __restrict__ coop, int N, int ldp,
                                                          int P_hid, int log2tc, int tiles_per_seed, int total_tiles,
                                                          float* __restrict__ lo_dbg, float* __restrict__ hi_dbg) {
  RCMARL_DYN_SMEM(float, tile);
  const int TC = 1 << log2tc;
  const TileStager st{msg, N, ldp, log2tc, tiles_per_seed};
  float pf[4 * PF];
  int t = blockIdx.x;
  if (t < total_tiles) st.fetch(t, pf);
  const int c = threadIdx.x & (TC - 1);
  const int rows_per_pass = 256 >> log2tc;
  for (; t < total_tiles; t += gridDim.x) {
    __syncthreads();                       // every wave is done with the previous tile image
    st.commit(pf, tile);
    __syncthreads();
    if (t + (int)gridDim.x < total_tiles) st.fetch(t + gridDim.x, pf);   // in flight during the aggregation below
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) << log2tc;
    const bool col_ok = (c0 + c) < P_hid;
    auto load_vals = [&](const int i, float (&v)[D]) {
#pragma unroll
      for (int k = 0; k < D; ++k) v[k] = tile[(nbr[i * D + k] << log2tc) + c];
    };
    auto finish = [&](const int i, const float (&v)[D]) {
      float lower, upper;
      const float out = aggregate_regs<D, H>(v, lower, upper, lo_dbg != nullptr);
      if (col_ok) {
        const size_t o = ((size_t)s * N + i) * ldp + c0 + c;
        theta[o] = out;
        if (lo_dbg) { lo_dbg[o] = lower; hi_dbg[o] = upper; }
      }
    };
    if (log2tc == 6) {
      // one wavefront = one agent: the agent index is an SGPR, so the neighbour list and the
      // cooperation flag come through the scalar cache; two agents per trip for ILP
      int i = threadIdx.x >> 6;
      for (; i + 4 < N; i += 8) {
        const int ia = __builtin_amdgcn_readfirstlane(i), ib = __builtin_amdgcn_readfirstlane(i + 4);
        const bool ca = coop[ia] != 0, cb = coop[ib] != 0;
        float va[D], vb[D];
        if (ca) load_vals(ia, va);
        if (cb) load_vals(ib, vb);
        if (ca) finish(ia, va);
        if (cb) finish(ib, vb);
      }
      for (; i < N; i += 4) {
        const int ia = __builtin_amdgcn_readfirstlane(i);
        if (coop[ia]) { float va[D]; load_vals(ia, va); finish(ia, va); }
      }
    } else {
      for (int i = threadIdx.x >> log2tc; i < N; i += rows_per_pass) {
        if (coop[i]) { float va[D]; load_vals(i, va); finish(i, va); }
      }
    }
  }
}

// ---- v2: LDS-DMA double buffering, neighbour table in VGPRs -----------------------------------
// One persistent workgroup per CU slot walks (seed, 64-column) tiles.  The [N][64] fp32 image of
// tile t+1 streams global -> LDS with `global_load_lds_dwordx4` (no staging VGPRs, no commit pass)
// into the second LDS buffer while tile t is aggregated, one barrier per tile.  A wave owns the
// agents {w, w+nw, w+2nw, ...}; their neighbour lists never change, so they are loaded ONCE:
// lane j of VGPR k holds the LDS byte offset of row nbr[agent_j][k], and the per-agent list is
// pulled into SGPRs with v_readlane -- no scalar-memory latency inside the tile loop.
#ifdef RCMARL_EMU
__device__ __forceinline__ void rc_glds16(const float* g, float* lds_wave_base) {
  const float4 v = *reinterpret_cast<const float4*>(g);
  *reinterpret_cast<float4*>(lds_wave_base + 4 * hipemu::lane()) = v;
}
__device__ __forceinline__ int rc_readlane(int v, int l) { return __hipemu_xch(v, l); }
#else
__device__ __forceinline__ void rc_glds16(const float* g, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ int rc_readlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
#endif

template <int D, int H>
__global__ __launch_bounds__(1024) void k_consensus_params_v2(const float* __restrict__ msg, float* __restrict__ theta,
                                                              const int* __restrict__ nbr,
                                                              const int* __restrict__ coop, int N, int ldp,
                                                              int P_hid, int tiles_per_seed, int total_tiles,
                                                              float* __restrict__ lo_dbg, float* __restrict__ hi_dbg) {
  RCMARL_DYN_SMEM(float, lds);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int tile_floats = N * 64;
  // neighbour table of this wave's agents (agent of slot j = wave + nw*j), as LDS byte offsets
  const int my_agent = wave + nw * lane;
  int tab[D];
  int coop_l = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) tab[k] = 0;
  if (my_agent < N) {
    coop_l = coop[my_agent];
#pragma unroll
    for (int k = 0; k < D; ++k) tab[k] = nbr[my_agent * D + k] * 256;
  }
  const int n_slots = (N - wave + nw - 1) / nw;          // agents owned by this wave (<= 64)
  const int rows_per_wave = (N + nw - 1) / nw;           // staging: wave w copies rows [w*rpw, (w+1)*rpw)
  auto stage = [&](int t, float* buf) {
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) * 64;
    const float* m = msg + (size_t)s * N * ldp + c0;
    const int r_begin = wave * rows_per_wave, r_end = min(N, r_begin + rows_per_wave);
    for (int r = r_begin; r < r_end; r += 4) {           // one instruction = 4 rows x 256 B = 1 KiB of LDS
      int row = r + (lane >> 4);
      row = row < N ? row : N - 1;                       // (tail lanes re-read the last row into the slack rows)
      rc_glds16(m + (size_t)row * ldp + 4 * (lane & 15), buf + (size_t)r * 64);
    }
  };
  int t = blockIdx.x;
  int cur = 0;
  if (t < total_tiles) stage(t, lds);
  for (; t < total_tiles; t += gridDim.x) {
    // Tile t must have LANDED before anybody reads it.  hipcc does NOT put the vmcnt(0) in front of this barrier
    // by itself when the LDS-DMA was issued in the previous trip of the loop (it did only for the first tile):
    // without the explicit wait short tiles (small N, small d) were aggregated from stale LDS -- wrong and
    // run-to-run different results at e.g. N=5, d=4, S>=256.
    RC_WAIT_VMEM();
    __syncthreads();                                     // everybody's part of tile t landed; buffer cur^1 is free
    const int tn = t + gridDim.x;
    if (tn < total_tiles) stage(tn, lds + (cur ^ 1) * (tile_floats + 256));
    const float* tile = lds + cur * (tile_floats + 256);
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) * 64;
    const bool col_ok = (c0 + lane) < P_hid;
    const char* tb = reinterpret_cast<const char*>(tile + lane);
    for (int j = 0; j < n_slots; ++j) {
      if (!rc_readlane(coop_l, j)) continue;             // wave-uniform
      float v[D];
#pragma unroll
      for (int k = 0; k < D; ++k) v[k] = *reinterpret_cast<const float*>(tb + rc_readlane(tab[k], j));
      float lower, upper;
      const float out = aggregate_regs<D, H>(v, lower, upper, lo_dbg != nullptr);
      if (col_ok) {
        const size_t o = ((size_t)s * N + (wave + nw * j)) * ldp + c0 + lane;
        theta[o] = out;
        if (lo_dbg) { lo_dbg[o] = lower; hi_dbg[o] = upper; }
      }
    }
    cur ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------
// Circulant graphs (the reference's own topology: in_nodes[i] = [i, i+1, .., i+d-1 mod N], main.py:28) with
// d == 2H+2: G consecutive agents share d-G+1 of their d inputs, so ONE selection network over the shared values
// (SelMid: their middle G+1 order statistics) serves G agents; each agent then merges its own G-1 extra values:
//   sorted(v_i)[H]   = min_{a=0..E} max(t[a-1], c[E-a])       E = G-1, t = the agent's sorted extras (t[-1] = -inf),
//   sorted(v_i)[H+1] = min_{a=0..E} max(t[a-1], c[E+1-a])     c = ranks H-E .. H+1 of the shared values
// (a lattice identity: exact for ties too).  (18, 8): 96/4 + 13 min/max ops per agent instead of 128; (66, 32):
// 796/8 + 54 instead of 904.  Clip window and the summation order of the mean are those of aggregate_regs, so the
// results are bit-identical to the general kernels.  Tile = [N][TC] columns in LDS (LDS-DMA double buffer as v2);
// a wavefront holds 64/TC groups side by side.
template <int E> struct SortSmall;
template <> struct SortSmall<1> { static __device__ __forceinline__ void run(float (&)[1]) {} };
template <> struct SortSmall<3> {
  static __device__ __forceinline__ void run(float (&t)[3]) {
    const float a = t[0], b = t[1], c = t[2];
    t[0] = fminf(fminf(a, b), c); t[1] = __builtin_amdgcn_fmed3f(a, b, c); t[2] = fmaxf(fmaxf(a, b), c);
  }
};
#define RC_CE(i, j) { const float lo_ = fminf(t[i], t[j]), hi_ = fmaxf(t[i], t[j]); t[i] = lo_; t[j] = hi_; }
template <> struct SortSmall<5> {      // 9 comparators (optimal)
  static __device__ __forceinline__ void run(float (&t)[5]) {
    RC_CE(0, 1) RC_CE(3, 4) RC_CE(2, 4) RC_CE(2, 3) RC_CE(1, 4) RC_CE(0, 3) RC_CE(0, 2) RC_CE(1, 3) RC_CE(1, 2)
  }
};
template <> struct SortSmall<7> {      // 16 comparators (optimal)
  static __device__ __forceinline__ void run(float (&t)[7]) {
    RC_CE(1, 2) RC_CE(3, 4) RC_CE(5, 6) RC_CE(0, 2) RC_CE(3, 5) RC_CE(4, 6) RC_CE(0, 1) RC_CE(4, 5)
    RC_CE(2, 6) RC_CE(0, 4) RC_CE(1, 5) RC_CE(0, 3) RC_CE(2, 5) RC_CE(1, 3) RC_CE(2, 4) RC_CE(2, 3)
  }
};
#undef RC_CE

template <int D, int H, int G, int TC, int THREADS>
__global__ __launch_bounds__(THREADS) void k_consensus_params_circ(const float* __restrict__ msg,
                                                                   float* __restrict__ theta,
                                                                   const int* __restrict__ coop, int N, int ldp,
                                                                   int P_hid, int tiles_per_seed, int total_tiles,
                                                                   float* __restrict__ lo_dbg,
                                                                   float* __restrict__ hi_dbg) {
  static_assert(D == 2 * H + 2 && H >= G - 1 && 64 % TC == 0 && TC % 4 == 0, "circulant kernel: d = 2H+2, H >= G-1");
  constexpr int E = G - 1, M = D - G + 1, U = D + G - 1, SUB = 64 / TC, RPI = 256 / TC;   // RPI: rows per LDS-DMA burst
  RCMARL_DYN_SMEM(float, lds);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = THREADS >> 6;   // wave: an SGPR
  // the tile carries the first U-1 rows a second time after row N-1: a group's window never wraps
  const int NR = N + U - 1, tile_floats = NR * TC, buf_floats = tile_floats + 256;
  const int c = lane % TC, sub = lane / TC;
  const int n_groups = (N + G - 1) / G, per_pass = nw * SUB, n_iter = (n_groups + per_pass - 1) / per_pass;
  const int rows_per_wave = (NR + nw - 1) / nw;
  auto stage = [&](int t, float* buf) {
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) * TC;
    const float* m = msg + (size_t)s * N * ldp + c0;
    const int r_begin = wave * rows_per_wave, r_end = min(NR, r_begin + rows_per_wave);
    for (int r = r_begin; r < r_end; r += RPI) {         // one instruction = RPI rows x TC*4 B = 1 KiB of LDS
      int row = r + lane / (TC / 4);
      row = row < NR ? row : NR - 1;                     // (tail lanes re-read the last row into the slack rows)
      if (row >= N) row -= N;
      if (row >= N) row -= N;                            // (U - 1 < 2N)
      rc_glds16(m + (size_t)row * ldp + 4 * (lane % (TC / 4)), buf + (size_t)r * TC);
    }
  };
  int t = blockIdx.x;
  int cur = 0;
  if (t < total_tiles) stage(t, lds);
  // (while the first tile is in flight) the groups a lane serves are the same for every tile: their "exists and is cooperative" flags, G bits per pass
  static_assert(G % 2 == 0, "agents are finished in pairs");
  unsigned long long okmask = 0;
  for (int j = 0; j < n_iter; ++j) {
    const int gi = wave * SUB + sub + per_pass * j;
    for (int g = 0; g < G; ++g) {
      const int agent = gi * G + g;
      if (gi < n_groups && agent < N && coop[agent]) okmask |= 1ull << (j * G + g);
    }
  }
  for (; t < total_tiles; t += gridDim.x) {
    RC_WAIT_VMEM();                                      // the LDS-DMA of tile t (see k_consensus_params_v2)
    __syncthreads();
    const int tn = t + gridDim.x;
    if (tn < total_tiles) stage(tn, lds + (cur ^ 1) * buf_floats);
    const float* tile = lds + cur * buf_floats;
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) * TC;
    const bool col_ok = (c0 + c) < P_hid;
    for (int j = 0; j < n_iter; ++j) {
      const int gi = wave * SUB + sub + per_pass * j;
      if (gi >= n_groups) continue;
      const int i0 = gi * G;
      float v[U];
      const float* p0 = tile + i0 * TC + c;              // constant offsets from one base
#pragma unroll
      for (int q = 0; q < U; ++q) v[q] = p0[q * TC];
      float cm[M], mid[G + 1];
#pragma unroll
      for (int q = 0; q < M; ++q) cm[q] = v[G - 1 + q];
      SelMid<M, H - G + 1, G + 1>::run(cm, mid);
      // bounds of the G agents, then clip + mean for two agents at a time: the D additions of a mean are taken in
      // neighbour order, as aggregate_regs does (the general kernels' results, bit for bit; the reference's tf.reduce_mean
      // fixes no order and parity with it is to fp32 tolerance), and two agents' chains ride in one v_pk_add_f32
      float lower[G], upper[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float tx[E];
#pragma unroll
        for (int q = 0; q < E; ++q) tx[q] = (q < E - g) ? v[g + q] : v[D + q - (E - g)];
        SortSmall<E>::run(tx);
        float slo = mid[E], shi = mid[E + 1];
#pragma unroll
        for (int a = 1; a <= E; ++a) {
          slo = fminf(slo, fmaxf(tx[a - 1], mid[E - a]));
          shi = fminf(shi, fmaxf(tx[a - 1], mid[E + 1 - a]));
        }
        const float own = v[g];
        lower[g] = fminf(slo, own);
        upper[g] = fmaxf(shi, own);
      }
      float res[G];
#pragma unroll
      for (int g = 0; g < G; g += 2) {
        rc_f2 sum = rc_bcast2(0.f);
#pragma unroll
        for (int k = 0; k < D; ++k)
          sum = rc_add2(sum, rc_f2{__builtin_amdgcn_fmed3f(v[g + k], lower[g], upper[g]),
                                   __builtin_amdgcn_fmed3f(v[g + 1 + k], lower[g + 1], upper[g + 1])});
        res[g] = sum.x;
        res[g + 1] = sum.y;
      }
      // x / D by reciprocal + two fma corrections (rc_div_fast); its only inexact cases have a subnormal quotient, and
      // those take the true division on a wavefront-uniform branch that real weights never enter
      // (a zero sum also takes it: same result, and only all-zero columns such as fresh biases have one)
      float amin = fabsf(res[0]);
#pragma unroll
      for (int g = 1; g < G; ++g) amin = fminf(amin, fabsf(res[g]));
      float q[G];
#pragma unroll
      for (int g = 0; g < G; ++g) q[g] = rc_div_fast<D>(res[g]);
      if (__builtin_expect(rc_any(amin < 1e-30f), 0)) {
        RC_NO_SPECULATE();                             // (keeps the IEEE division's ~10 instructions out of the fast path)
#pragma unroll
        for (int g = 0; g < G; ++g) q[g] = res[g] / (float)D;
      }
      const unsigned ok = col_ok ? (unsigned)(okmask >> (j * G)) & ((1u << G) - 1u) : 0u;   // bit g: agent i0+g exists and is cooperative
      const size_t o0 = ((size_t)s * N + i0) * ldp + c0 + c;
      float* tp = theta + o0;
      if (rc_all(ok == (1u << G) - 1u)) {                // the usual case: no per-agent predicates
#pragma unroll
        for (int g = 0; g < G; ++g) RC_NT_STORE(tp + (size_t)g * ldp, q[g]);
      } else {
#pragma unroll
        for (int g = 0; g < G; ++g)
          if ((ok >> g) & 1u) tp[(size_t)g * ldp] = q[g];
      }
      if (lo_dbg) {
#pragma unroll
        for (int g = 0; g < G; ++g)
          if ((ok >> g) & 1u) { lo_dbg[o0 + (size_t)g * ldp] = lower[g]; hi_dbg[o0 + (size_t)g * ldp] = upper[g]; }
      }
    }
    cur ^= 1;
  }
}

// G per (d, H): measured choice among the generated SelMid networks
int circ_group(int d, int H) {
  if (d == 4 && H == 1) return 2;
  if (d == 6 && H == 2) return 2;
  if (d == 10 && H == 4) return 4;
  if (d == 18 && H == 8) return 4;
  if (d == 34 && H == 16) return 4;
  if (d == 66 && H == 32) return 8;
  return 0;
}

// LDS of the circulant kernel: two tiles of N + (d+G-2) rows (the wrapped rows twice) + one DMA burst of slack each
size_t circ_smem(int N, int d, int G, int TC) { return 2 * ((size_t)(N + d + G - 2) * TC + 256) * sizeof(float); }

// Any (d, H) without a generated network: order statistics by rank counting
// out of the LDS tile (O(d^2) LDS reads).  Correct for every d >= 2H+1; slow.
// One agent, one column: nb = the agent's neighbour list, c = the lane's column of the [N][TC] tile.
__device__ __forceinline__ void window_rank_count(const float* tile, const int* nb, int log2tc, int c, int d, int H,
                                                  float& lower, float& upper) {
  const float own = tile[(nb[0] << log2tc) + c];
  float lo = own, hi = own;
  for (int k = 0; k < d; ++k) {
    const float x = tile[(nb[k] << log2tc) + c];
    int rank = 0;
    for (int m = 0; m < d; ++m) {
      const float y = tile[(nb[m] << log2tc) + c];
      rank += (y < x || (y == x && m < k)) ? 1 : 0;
    }
    if (rank == H) lo = x;
    if (rank == d - H - 1) hi = x;
  }
  lower = fminf(lo, own);
  upper = fmaxf(hi, own);
}

__device__ __forceinline__ float aggregate_rank_count(const float* tile, const int* nb, int log2tc, int c, int d, int H,
                                                      float& lower, float& upper) {
  window_rank_count(tile, nb, log2tc, c, d, H, lower, upper);
  float sum = 0.f;
  for (int k = 0; k < d; ++k) sum += __builtin_amdgcn_fmed3f(tile[(nb[k] << log2tc) + c], lower, upper);
  return sum / (float)d;
}

__global__ __launch_bounds__(256) void k_consensus_params_generic(const float* __restrict__ msg,
                                                                  float* __restrict__ theta,
                                                                  const int* __restrict__ nbr,
                                                                  const int* __restrict__ coop, int N,
                                                                  int ldp, int P_hid, int log2tc, int d, int H,
                                                                  float* __restrict__ lo_dbg,
                                                                  float* __restrict__ hi_dbg) {
  RCMARL_DYN_SMEM(float, tile);
  const int TC = 1 << log2tc;
  const int s = blockIdx.y;
  const int c0 = blockIdx.x << log2tc;
  {
    const TileStager st{msg, N, ldp, log2tc, (int)gridDim.x};
    float pf[4 * PF];
    st.fetch(s * gridDim.x + blockIdx.x, pf);
    st.commit(pf, tile);
  }
  __syncthreads();
  const int c = threadIdx.x & (TC - 1);
  const int rows_per_pass = blockDim.x >> log2tc;
  const bool col_ok = (c0 + c) < P_hid;
  for (int i = threadIdx.x >> log2tc; i < N; i += rows_per_pass) {
    if (!coop[i]) continue;
    float lower, upper;
    const float out = aggregate_rank_count(tile, nbr + i * d, log2tc, c, d, H, lower, upper);
    if (col_ok) {
      const size_t o = ((size_t)s * N + i) * ldp + c0 + c;
      theta[o] = out;
      if (lo_dbg) { lo_dbg[o] = lower; hi_dbg[o] = upper; }
    }
  }
}

// ---- irregular graphs: every (d, H) class of the cooperative agents in ONE launch ----------------------------------------
// The graph arrives as CSR (nbr_off[N+1], nbr_idx[nnz]; nbr_idx[nbr_off[i]] == i) and the cooperative agents sorted by their
// (d, H) class (order[]; the class table {d, H, first, count} rides in the kernel arguments).  Same persistent tile walk and
// TileStager as k_consensus_params: the [N][TC] message tile is staged ONCE per (seed, column tile) -- one launch of
// k_consensus_params per class would read the whole message matrix once per class, and K1 is HBM-bound at small d.  The workgroup
// then walks the classes; (d, H) of a class is uniform, a scalar branch picks the generated SelNet<D, H> (aggregate_regs: the
// per-agent code of k_consensus_params, so an agent's result has the bits rcmarl_consensus_params gives on a regular graph of its
// class) or the rank counting of k_consensus_params_generic.
// Code size: the switch instantiates each network once (d <= RC_RAGGED_MAX_NET_D; the few wider generated networks would
// set the register budget of the whole kernel and take the rank-counting branch here).
constexpr int RC_RAGGED_MAX_CLASSES = 32;   // classes per launch (the entry point issues further launches beyond)
constexpr int RC_RAGGED_MAX_NET_D = 20;
struct RaggedClasses {
  int n;
  int d[RC_RAGGED_MAX_CLASSES], H[RC_RAGGED_MAX_CLASSES], first[RC_RAGGED_MAX_CLASSES], count[RC_RAGGED_MAX_CLASSES];
};

template <int D, int H>
__device__ __forceinline__ void ragged_class(const float* tile, float* __restrict__ theta, const int* __restrict__ nbr_off,
                                             const int* __restrict__ nbr_idx, const int* __restrict__ order, int first,
                                             int count, int N, int ldp, int log2tc, int s, int c0, int c, bool col_ok,
                                             float* __restrict__ lo_dbg, float* __restrict__ hi_dbg) {
  auto load_vals = [&](const int i, float (&v)[D]) {
    const int* nb = nbr_idx + nbr_off[i];
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = tile[(nb[k] << log2tc) + c];
  };
  auto finish = [&](const int i, const float (&v)[D]) {
    float lower, upper;
    const float out = aggregate_regs<D, H>(v, lower, upper, lo_dbg != nullptr);
    if (col_ok) {
      const size_t o = ((size_t)s * N + i) * ldp + c0 + c;
      theta[o] = out;
      if (lo_dbg) { lo_dbg[o] = lower; hi_dbg[o] = upper; }
    }
  };
  if (log2tc == 6) {
    // one wavefront = one agent (an SGPR index: the neighbour list comes through the scalar cache); two agents per trip for ILP
    int j = threadIdx.x >> 6;
    for (; j + 4 < count; j += 8) {
      const int ia = __builtin_amdgcn_readfirstlane(order[first + j]), ib = __builtin_amdgcn_readfirstlane(order[first + j + 4]);
      float va[D], vb[D];
      load_vals(ia, va);
      load_vals(ib, vb);
      finish(ia, va);
      finish(ib, vb);
    }
    for (; j < count; j += 4) {
      const int ia = __builtin_amdgcn_readfirstlane(order[first + j]);
      float va[D];
      load_vals(ia, va);
      finish(ia, va);
    }
  } else {
    for (int j = threadIdx.x >> log2tc; j < count; j += 256 >> log2tc) {
      const int i = order[first + j];
      float va[D];
      load_vals(i, va);
      finish(i, va);
    }
  }
}

__global__ __launch_bounds__(256) void k_consensus_params_ragged(const float* __restrict__ msg, float* __restrict__ theta,
                                                                 const int* __restrict__ nbr_off,
                                                                 const int* __restrict__ nbr_idx,
                                                                 const int* __restrict__ order, const RaggedClasses cls, int N,
                                                                 int ldp, int P_hid, int log2tc, int tiles_per_seed,
                                                                 int total_tiles, float* __restrict__ lo_dbg,
                                                                 float* __restrict__ hi_dbg) {
  RCMARL_DYN_SMEM(float, tile);
  const int TC = 1 << log2tc;
  const TileStager st{msg, N, ldp, log2tc, tiles_per_seed};
  float pf[4 * PF];
  int t = blockIdx.x;
  if (t < total_tiles) st.fetch(t, pf);
  const int c = threadIdx.x & (TC - 1);
  for (; t < total_tiles; t += gridDim.x) {
    __syncthreads();                       // every wave is done with the previous tile image
    st.commit(pf, tile);
    __syncthreads();
    if (t + (int)gridDim.x < total_tiles) st.fetch(t + gridDim.x, pf);   // in flight during the aggregation below
    const int s = t / tiles_per_seed, c0 = (t - s * tiles_per_seed) << log2tc;
    const bool col_ok = (c0 + c) < P_hid;
    for (int q = 0; q < cls.n; ++q) {
      const int d = cls.d[q], H = cls.H[q], first = cls.first[q], count = cls.count[q];
      switch (d <= RC_RAGGED_MAX_NET_D ? d * 64 + H : -1) {
#define RC_RCASE(DD, HH)                                                                                                     \
        case (DD <= RC_RAGGED_MAX_NET_D ? DD * 64 + HH : -2 - (DD * 64 + HH)):                                               \
          if constexpr (DD <= RC_RAGGED_MAX_NET_D)                                                                           \
            ragged_class<DD, HH>(tile, theta, nbr_off, nbr_idx, order, first, count, N, ldp, log2tc, s, c0, c, col_ok,       \
                                 lo_dbg, hi_dbg);                                                                            \
          break;
        RCMARL_SELNET_COMBOS(RC_RCASE)
#undef RC_RCASE
        default:
          for (int j = threadIdx.x >> log2tc; j < count; j += 256 >> log2tc) {
            const int i = order[first + j];
            float lower, upper;
            const float out = aggregate_rank_count(tile, nbr_idx + nbr_off[i], log2tc, c, d, H, lower, upper);
            if (col_ok) {
              const size_t o = ((size_t)s * N + i) * ldp + c0 + c;
              theta[o] = out;
              if (lo_dbg) { lo_dbg[o] = lower; hi_dbg[o] = upper; }
            }
          }
      }
    }
  }
}

template <class K>
bool k1_want_lds(K kernel, size_t smem) {
  return rc_want_lds(kernel, smem, 64 * 1024);
}

// v2 is instantiated only where the d values + the neighbour table fit 128 VGPRs (16 waves per CU)
template <int DD, int HH>
bool launch_v2(const float* msg, float* theta, const int* nbr, const int* coop, int N, int ldp, int P_hid, int tps,
               int tot, float* lo_dbg, float* hi_dbg, int nwg, int threads, size_t smem, void* stream, int& rc) {
  if constexpr (DD <= 32) {
    if (!k1_want_lds(k_consensus_params_v2<DD, HH>, smem)) { rc = RCMARL_ERR_LAUNCH; return true; }
    RCMARL_LAUNCH((k_consensus_params_v2<DD, HH>), dim3(nwg), dim3(threads), smem, stream, msg, theta, nbr, coop, N, ldp,
                  P_hid, tps, tot, lo_dbg, hi_dbg);
    return true;
  } else {
    return false;
  }
}

// ---- clip report: what the clip window trims, per in-neighbour slot ---------------------------------------------------------
// For every cooperative agent i and slot k of its in-neighbourhood: how many of the P_hid hidden-layer parameters of neighbour k's
// message lie strictly below / above i's clip window (the window K1 computes and then discards: window_regs / window_rank_count).
//
// Grid = (column ranges, agent groups, seeds).  A workgroup walks the column tiles of its range; per tile it stages the [N][TC]
// image K1 stages, but ONLY the rows its agent group reads (a byte map in LDS, filled once from the group's neighbour lists: a group
// of G consecutive agents of a circulant graph fetches G + d - 1 rows, not N).  A wavefront owns TC-column slices of whole agents;
// a slot's comparison becomes popcount(ballot) and one lane adds it to the group's counters in LDS (one wavefront per agent: no
// two wavefronts share a counter).  After the last tile the counters go to `scratch` with plain stores -- every (range, seed,
// agent, slot) entry has exactly one writer -- and k_clip_fold adds the ranges' partials into the 64-bit accumulators, one thread
// per accumulator.  No atomics on global memory: the same integers on every run.
struct ClipGraph {
  const int* nbr; const int* coop; int d;                               // regular graph: nbr[N][d], coop[N]
  const int* nbr_off; const int* nbr_idx; const int* order;             // irregular graph (CSR; order[] lists the cooperative agents)
  __device__ __forceinline__ const int* nb(int i) const { return nbr ? nbr + (size_t)i * d : nbr_idx + nbr_off[i]; }
};

struct ClipPlan {
  bool ok;
  int log2tc, tiles_per_seed, CR, tiles_per_range, GA, AG;
  size_t smem;
  long long scratch_ints;
};

// Everything the launch shape depends on is (S, N, ldc, P_hid): the scratch query and the entry points agree by construction.
ClipPlan clip_plan(int S, int N, int ldc, int P_hid) {
  ClipPlan p{};
  if (S <= 0 || N <= 0 || ldc <= 0 || P_hid <= 0) return p;
  p.log2tc = 6;                                             // widest column tile whose [N][TC] image fits 64 KiB, as K1
  while (p.log2tc > 2 && ((size_t)N << p.log2tc) * sizeof(float) > 64 * 1024) --p.log2tc;
  if (((size_t)N << p.log2tc) * sizeof(float) > 64 * 1024) return p;
  p.tiles_per_seed = rc_ceil_div(P_hid, 1 << p.log2tc);
  // agents per group: both counters of a group within 12 KiB, so that image + counters + row map leave two workgroups per CU
  int ga = 12288 / (8 * ldc);
  ga = ga < 1 ? 1 : (ga > N ? N : ga);
  p.AG = rc_ceil_div(N, ga);
  p.GA = rc_ceil_div(N, p.AG);
  p.AG = rc_ceil_div(N, p.GA);
  // column ranges: enough workgroups for the chip, at most 16 partial planes, no empty range
  const long long per_range = (long long)p.AG * S;
  const int target = rc_persistent_grid(1024);
  long long cr = (target + per_range - 1) / per_range;
  if (cr > 16) cr = 16;
  if (cr > p.tiles_per_seed) cr = p.tiles_per_seed;
  if (cr < 1) cr = 1;
  const long long plane = 2LL * S * N * ldc;                // below + above of one column range
  while (cr > 1 && cr * plane > 0x7fffffffLL) --cr;
  if (cr * plane > 0x7fffffffLL) return p;
  p.tiles_per_range = rc_ceil_div(p.tiles_per_seed, (int)cr);
  p.CR = rc_ceil_div(p.tiles_per_seed, p.tiles_per_range);
  p.scratch_ints = p.CR * plane;
  p.smem = ((size_t)N << p.log2tc) * sizeof(float) + 2 * (size_t)p.GA * ldc * sizeof(int) + (((size_t)N + 15) & ~(size_t)15);
  p.ok = p.AG <= 65535 && S <= 65535;
  return p;
}

struct ClipCtx {
  const float* tile; int* cnt;                              // counters: below [GA][ldc], then above [GA][ldc]
  int log2tc, c, g0, ga, GA, ldc, rpp;                      // rpp: agents the workgroup takes per pass
  bool col_ok;
  unsigned long long submask;                               // the lanes that hold this lane's agent
};

// One agent (per TC lanes): window, then one ballot pair per slot.  nb must be readable for d entries for every lane; `valid`
// lanes own a real agent whose counters are cb / ca.  Every lane of the wavefront runs this (ballots).
template <int D, int H>
__device__ __forceinline__ void clip_agent(const ClipCtx& x, const int* nb, bool valid, int* cb, int* ca, int d, int Hrt) {
  const bool ok = valid && x.col_ok;
  const int tcm = (1 << x.log2tc) - 1;
  float lower, upper;
  if constexpr (D > 0) {
    float v[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = x.tile[(nb[k] << x.log2tc) + x.c];
    window_regs<D, H>(v, lower, upper);
    if (x.log2tc == 6) {
      // one wavefront = one agent (`valid` is uniform): the counts are scalars; lane k keeps slot k in a register and the
      // counters in LDS take one add per lane and tile (slots from 64 on go there directly)
      int accb = 0, acca = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const int nbl = (int)__builtin_popcountll(rc_ballot(ok && v[k] < lower));
        const int nab = (int)__builtin_popcountll(rc_ballot(ok && v[k] > upper));
        if (k < 64) {
          accb += x.c == k ? nbl : 0;
          acca += x.c == k ? nab : 0;
        } else if (valid && x.c == k - 64) {
          atomicAdd(cb + k, nbl);
          atomicAdd(ca + k, nab);
        }
      }
      if (valid && x.c < (D < 64 ? D : 64)) {
        atomicAdd(cb + x.c, accb);
        atomicAdd(ca + x.c, acca);
      }
    } else {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const unsigned long long mb = rc_ballot(ok && v[k] < lower), ma = rc_ballot(ok && v[k] > upper);
        if (valid && x.c == (k & tcm)) {
          atomicAdd(cb + k, (int)__builtin_popcountll(mb & x.submask));
          atomicAdd(ca + k, (int)__builtin_popcountll(ma & x.submask));
        }
      }
    }
  } else {
    window_rank_count(x.tile, nb, x.log2tc, x.c, d, Hrt, lower, upper);
    for (int k = 0; k < d; ++k) {
      const float v = x.tile[(nb[k] << x.log2tc) + x.c];
      const unsigned long long mb = rc_ballot(ok && v < lower), ma = rc_ballot(ok && v > upper);
      if (valid && x.c == (k & tcm)) {
        atomicAdd(cb + k, (int)__builtin_popcountll(mb & x.submask));
        atomicAdd(ca + k, (int)__builtin_popcountll(ma & x.submask));
      }
    }
  }
}

// The agents of one class that belong to this workgroup's group [g0, g0 + ga).  Regular graph (no order[]): agent = position.
__device__ __forceinline__ int clip_agent_of(const ClipGraph& g, int first, int j, int j_end, int g0, int ga) {
  if (j >= j_end) return -1;
  const int i = g.order ? g.order[first + j] : j;
  if (i < g0 || i >= g0 + ga) return -1;
  if (g.coop && !g.coop[i]) return -1;
  return i;
}

template <int D, int H>
__device__ __forceinline__ void clip_class(const ClipCtx& x, const ClipGraph& g, int first, int count, int d, int Hrt) {
  const int j_begin = g.order ? 0 : x.g0, j_end = g.order ? count : x.g0 + x.ga;
  const int rpp = x.rpp;
  const int fallback = g.order ? g.order[first] : x.g0;     // an agent of this class: its list has d entries
  for (int j0 = j_begin; j0 < j_end; j0 += rpp) {
    int i = clip_agent_of(g, first, j0 + (int)(threadIdx.x >> x.log2tc), j_end, x.g0, x.ga);
    if (x.log2tc == 6) {                                    // one wavefront = one agent: an SGPR index, a uniform skip
      i = __builtin_amdgcn_readfirstlane(i);
      if (i < 0) continue;
    }
    const bool valid = i >= 0;
    const int a = valid ? i - x.g0 : 0;
    clip_agent<D, H>(x, g.nb(valid ? i : fallback), valid, x.cnt + a * x.ldc, x.cnt + (x.GA + a) * x.ldc, d, Hrt);
  }
}

// WD > 0: the regular entry's kernel for one generated network (WD, WH); WD == 0: any classes -- networks up to
// RC_RAGGED_MAX_NET_D through a scalar switch, rank counting otherwise (the rule of k_consensus_params_ragged).
// Workgroup size: the image and the counters leave two workgroups per CU at most, so the wavefronts that hide the LDS latency have
// to come from the workgroup itself: 1024 threads (128 VGPRs each) wherever the network fits them, 512 for the widest networks.
template <int WD> constexpr int clip_threads() { return WD <= 34 ? 1024 : 512; }

template <int WD, int WH>
__global__ __launch_bounds__(clip_threads<WD>()) void k_clip_counts(const float* __restrict__ msg, const ClipGraph g,
                                                                    const RaggedClasses cls, int* __restrict__ scratch, int N,
                                                                    int ldp, int P_hid, int log2tc, int ldc, int tiles_per_seed,
                                                                    int tiles_per_range, int GA) {
  RCMARL_DYN_SMEM(float, tile);
  const int TC = 1 << log2tc, lq = log2tc - 2, nt = clip_threads<WD>();
  int* cnt = reinterpret_cast<int*>(tile + ((size_t)N << log2tc));
  unsigned char* need = reinterpret_cast<unsigned char*>(cnt + 2 * GA * ldc);
  const int r = blockIdx.x, g0 = blockIdx.y * GA, s = blockIdx.z, S = gridDim.z, CR = gridDim.x;
  const int ga = min(GA, N - g0);
  const int tid = threadIdx.x;
  for (int idx = tid; idx < 2 * GA * ldc; idx += nt) cnt[idx] = 0;
  for (int idx = tid; idx < N; idx += nt) need[idx] = 0;
  __syncthreads();
  // the rows this group reads
  for (int q = 0; q < cls.n; ++q) {
    const int d = cls.d[q], first = cls.first[q], count = cls.count[q];
    if (cls.H[q] == 0) continue;
    const int j_begin = g.order ? 0 : g0, j_end = g.order ? count : g0 + ga;
    for (int idx = tid; idx < (j_end - j_begin) * d; idx += nt) {
      const int jj = idx / d, k = idx - jj * d;
      const int i = clip_agent_of(g, first, j_begin + jj, j_end, g0, ga);
      if (i >= 0) need[g.nb(i)[k]] = 1;
    }
  }
  ClipCtx x;
  x.tile = tile; x.cnt = cnt; x.log2tc = log2tc; x.c = tid & (TC - 1); x.rpp = nt >> log2tc; x.g0 = g0; x.ga = ga; x.GA = GA; x.ldc = ldc;
  x.submask = TC == 64 ? ~0ull : (((1ull << TC) - 1ull) << (((tid & 63) >> log2tc) << log2tc));
  const int t_begin = r * tiles_per_range, t_end = min(tiles_per_seed, t_begin + tiles_per_range);
  const float* ms = msg + (size_t)s * N * ldp;
  for (int t = t_begin; t < t_end; ++t) {
    const int c0 = t << log2tc;
    __syncthreads();                                        // the row map is complete / every wave is done with the previous image
    for (int idx = tid; idx < (N << lq); idx += nt) {
      const int row = idx >> lq, c4 = 4 * (idx & ((1 << lq) - 1));
      if (need[row])
        *reinterpret_cast<float4*>(tile + ((size_t)row << log2tc) + c4) =
            *reinterpret_cast<const float4*>(ms + (size_t)row * ldp + c0 + c4);
    }
    __syncthreads();
    x.col_ok = (c0 + x.c) < P_hid;
    for (int q = 0; q < cls.n; ++q) {
      const int d = cls.d[q], H = cls.H[q], first = cls.first[q], count = cls.count[q];
      if (H == 0) continue;                                 // window = [min, max]: nothing is clipped
      if constexpr (WD > 0) {
        clip_class<WD, WH>(x, g, first, count, d, H);
      } else {
        switch (d <= RC_RAGGED_MAX_NET_D ? d * 64 + H : -1) {
#define RC_CCASE(DD, HH)                                                                                                     \
          case (DD <= RC_RAGGED_MAX_NET_D ? DD * 64 + HH : -2 - (DD * 64 + HH)):                                             \
            if constexpr (DD <= RC_RAGGED_MAX_NET_D && HH > 0) clip_class<DD, HH>(x, g, first, count, d, H);                 \
            break;
          RCMARL_SELNET_COMBOS(RC_CCASE)
#undef RC_CCASE
          default:
            clip_class<0, 0>(x, g, first, count, d, H);
        }
      }
    }
  }
  __syncthreads();
  // partials of this (range, seed): plain stores, one writer per entry
  const size_t plane = (size_t)CR * S * N * ldc;
  int* part = scratch + ((size_t)r * S + s) * N * ldc;
  for (int q = 0; q < cls.n; ++q) {
    const int d = cls.d[q], first = cls.first[q], count = cls.count[q];
    if (cls.H[q] == 0) continue;
    const int j_begin = g.order ? 0 : g0, j_end = g.order ? count : g0 + ga;
    for (int idx = tid; idx < (j_end - j_begin) * d; idx += nt) {
      const int jj = idx / d, k = idx - jj * d;
      const int i = clip_agent_of(g, first, j_begin + jj, j_end, g0, ga);
      if (i >= 0) {
        part[(size_t)i * ldc + k] = cnt[(i - g0) * ldc + k];
        part[plane + (size_t)i * ldc + k] = cnt[(GA + i - g0) * ldc + k];
      }
    }
  }
}

// below/above[s][i][k] += sum over the column ranges' partials: one thread per accumulator (its only writer)
__global__ __launch_bounds__(256) void k_clip_fold(const int* __restrict__ scratch, const ClipGraph g, const RaggedClasses cls,
                                                   long long* __restrict__ below, long long* __restrict__ above, int N, int ldc,
                                                   int CR) {
  const int s = blockIdx.y, S = gridDim.y;
  const size_t plane = (size_t)CR * S * N * ldc, range = (size_t)S * N * ldc;
  for (int q = 0; q < cls.n; ++q) {
    const int d = cls.d[q], first = cls.first[q];
    if (cls.H[q] == 0) continue;
    const int j_end = g.order ? cls.count[q] : N;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < j_end * d; idx += gridDim.x * 256) {
      const int jj = idx / d, k = idx - jj * d;
      const int i = clip_agent_of(g, first, jj, j_end, 0, N);
      if (i < 0) continue;
      const size_t o = ((size_t)s * N + i) * ldc + k;
      long long nb_ = 0, na_ = 0;
      for (int r = 0; r < CR; ++r) { nb_ += scratch[r * range + o]; na_ += scratch[plane + r * range + o]; }
      below[o] += nb_;
      above[o] += na_;
    }
  }
}

template <int WD, int WH>
int clip_launch(const ClipPlan& p, const float* msg, const ClipGraph& g, const RaggedClasses& cls, long long* below,
                long long* above, int* scratch, int S, int N, int ldp, int P_hid, int ldc, void* stream) {
  if (!k1_want_lds(k_clip_counts<WD, WH>, p.smem)) return RCMARL_ERR_LAUNCH;
  RCMARL_LAUNCH((k_clip_counts<WD, WH>), dim3(p.CR, p.AG, S), dim3(clip_threads<WD>()), p.smem, stream, msg, g, cls, scratch, N, ldp, P_hid,
                p.log2tc, ldc, p.tiles_per_seed, p.tiles_per_range, p.GA);
  int rc = rcmarl_check_launch();
  if (rc != RCMARL_OK) return rc;
  int fb = rc_ceil_div(N * ldc, 256);
  if (fb > 64) fb = 64;
  RCMARL_LAUNCH(k_clip_fold, dim3(fb, S), dim3(256), 0, stream, (const int*)scratch, g, cls, below, above, N, ldc, p.CR);
  return rcmarl_check_launch();
}

}  // namespace

// C-ABI: see include/rcmarl.h
RCMARL_EXPORT int rcmarl_consensus_params(const float* msg, float* theta, const int* nbr, const int* coop,
                                          int S, int N, int ldp, int P_hid, int d, int H, float* lo_dbg,
                                          float* hi_dbg, void* stream) {
  if (!msg || !theta || !nbr || !coop || S <= 0 || N <= 0 || d <= 0 || H < 0 || d < 2 * H + 1 || (ldp & 63) ||
      P_hid <= 0 || P_hid > ldp || (!!lo_dbg != !!hi_dbg))
    return RCMARL_ERR_ARG;
  // widest column tile whose [N][TC] fp32 image fits 64 KiB of LDS (two workgroups per CU)
  int log2tc = 6;
  while (log2tc > 2 && ((size_t)N << log2tc) * sizeof(float) > 64 * 1024) --log2tc;
  if (((size_t)N << log2tc) * sizeof(float) > 64 * 1024) return RCMARL_ERR_UNSUPPORTED;
  const int TC = 1 << log2tc;
  const size_t smem = ((size_t)N << log2tc) * sizeof(float);
  const int tiles_per_seed = rc_ceil_div(P_hid, TC), total_tiles = tiles_per_seed * S;
  // persistent-style launch: as many workgroups as fit the chip at once (LDS-limited), each
  // walking total_tiles with stride gridDim.x so that loads of tile t+1 overlap compute of tile t
  int wg_per_cu = (int)((160 * 1024) / (smem + 512));
  if (wg_per_cu > 4) wg_per_cu = 4;
  if (wg_per_cu < 1) wg_per_cu = 1;
  int nwg = 256 * wg_per_cu;
  nwg = rc_persistent_grid(nwg);
  if (nwg > total_tiles) nwg = total_tiles;
  const dim3 grid_p(nwg), grid(tiles_per_seed, S), block(256);
  bool done = false;
  // v2 (LDS-DMA double buffer + VGPR neighbour table): whole tiles of 64 columns, two buffers in LDS
  static int k1_variant = -1;
  if (k1_variant < 0) { const char* e = getenv("RCMARL_K1"); k1_variant = e ? atoi(e) : 2; }
  const size_t smem2 = 2 * ((size_t)N * 64 + 256) * sizeof(float);
  if (k1_variant == 2 && smem2 <= 158 * 1024) {
    const int tps = rc_ceil_div(P_hid, 64), tot = tps * S;
    int wg_cu = (int)((160 * 1024) / (smem2 + 1024));
    if (wg_cu > 4) wg_cu = 4;
    const int threads = wg_cu >= 4 ? 256 : (wg_cu >= 2 ? 512 : 1024);
    int nwg2 = 256 * wg_cu;
    nwg2 = rc_persistent_grid(nwg2);
    if (nwg2 > tot) nwg2 = tot;
    if (N <= 64 * (threads / 64)) {
#define RC_CASE2(DD, HH)                                                                                             \
      if (!done && d == DD && H == HH)                                                                               \
        done = launch_v2<DD, HH>(msg, theta, nbr, coop, N, ldp, P_hid, tps, tot, lo_dbg, hi_dbg, nwg2, threads, smem2, \
                                 stream, rc);
      int rc = RCMARL_OK;
      RCMARL_SELNET_COMBOS(RC_CASE2)
#undef RC_CASE2
      if (rc != RCMARL_OK) return rc;
      if (done) return rcmarl_check_launch();
    }
  }
#define RC_CASE(DD, HH)                                                                                              \
  if (!done && d == DD && H == HH) {                                                                                 \
    RCMARL_LAUNCH((k_consensus_params<DD, HH>), grid_p, block, smem, stream, msg, theta, nbr, coop, N, ldp, P_hid,   \
                  log2tc, tiles_per_seed, total_tiles, lo_dbg, hi_dbg);                                              \
    done = true;                                                                                                     \
  }
  RCMARL_SELNET_COMBOS(RC_CASE)
#undef RC_CASE
  if (!done)
    RCMARL_LAUNCH(k_consensus_params_generic, grid, block, smem, stream, msg, theta, nbr, coop, N, ldp, P_hid, log2tc,
                  d, H, lo_dbg, hi_dbg);
  return rcmarl_check_launch();
}

// The same aggregation for a CIRCULANT graph, nbr[i][k] == (i + k) % N (the caller guarantees it; the reference's
// main.py:28 pattern), d == 2H+2.  Returns RCMARL_ERR_UNSUPPORTED when no kernel is compiled for (N, d, H): use
// rcmarl_consensus_params then.  Results are bit-identical to rcmarl_consensus_params.
RCMARL_EXPORT int rcmarl_consensus_params_circulant_supported(int N, int d, int H) {
  if (N <= 0 || d != 2 * H + 2 || d > N || circ_group(d, H) == 0) return 0;
  return circ_smem(N, d, circ_group(d, H), 16) <= 158 * 1024 ? 1 : 0;
}

RCMARL_EXPORT int rcmarl_consensus_params_circulant(const float* msg, float* theta, const int* coop, int S, int N,
                                                    int ldp, int P_hid, int d, int H, float* lo_dbg, float* hi_dbg,
                                                    void* stream) {
  if (!msg || !theta || !coop || S <= 0 || N <= 0 || d <= 0 || H < 0 || (ldp & 63) || P_hid <= 0 || P_hid > ldp ||
      (!!lo_dbg != !!hi_dbg))
    return RCMARL_ERR_ARG;
  if (!rcmarl_consensus_params_circulant_supported(N, d, H)) return RCMARL_ERR_UNSUPPORTED;
  const int G = circ_group(d, H);
  // 32 columns = one 128-byte line per row and two resident workgroups per CU up to N ~ 580 (measured best: 64-column
  // tiles leave one workgroup per CU and coarser tile counts); 16 columns only when nothing wider fits
  int TC = circ_smem(N, d, G, 32) <= 158 * 1024 ? 32 : 16;
  const size_t smem = circ_smem(N, d, G, TC);
  const int tps = rc_ceil_div(P_hid, TC), tot = tps * S;
  int wg_cu = (int)((160 * 1024) / (smem + 1024));
  const int wg_threads = d >= 34 ? 512 : 1024;        // (RC_CIRC_CASE below)
  if (wg_cu > 2048 / wg_threads) wg_cu = 2048 / wg_threads;          // resident workgroups only: the tile loop is persistent
  if (wg_cu < 1) wg_cu = 1;
  int nwg = 256 * wg_cu;
  nwg = rc_persistent_grid(nwg);
  if (nwg > tot) nwg = tot;
  {   // the kernel keeps one "agent exists and is cooperative" bit per (pass, agent of the group) in a 64-bit mask per lane
    const int per_pass = (wg_threads / 64) * (64 / TC), n_groups = rc_ceil_div(N, G);
    if (rc_ceil_div(n_groups, per_pass) * G > 64) return RCMARL_ERR_UNSUPPORTED;      // (N > ~2000: beyond the LDS tile anyway)
  }
  int rc = RCMARL_ERR_UNSUPPORTED;
#define RC_CIRC_LAUNCH(DD, HH, GG, TT, THR)                                                                          \
  do {                                                                                                               \
    if (!k1_want_lds(k_consensus_params_circ<DD, HH, GG, TT, THR>, smem)) return RCMARL_ERR_LAUNCH;                   \
    RCMARL_LAUNCH((k_consensus_params_circ<DD, HH, GG, TT, THR>), dim3(nwg), dim3(THR), smem, stream, msg, theta,     \
                  coop, N, ldp, P_hid, tps, tot, lo_dbg, hi_dbg);                                                    \
    rc = rcmarl_check_launch();                                                                                      \
  } while (0)
  // wide windows keep U = d+G-1 values plus the network's temporaries live: 512 threads (256 VGPRs) from d = 34
#define RC_CIRC_CASE(DD, HH, GG)                                                                                     \
  if (rc == RCMARL_ERR_UNSUPPORTED && d == DD && H == HH && G == GG) {                                               \
    constexpr int THR = (DD >= 34) ? 512 : 1024;                                                                     \
    if (TC == 64) RC_CIRC_LAUNCH(DD, HH, GG, 64, THR); else if (TC == 32) RC_CIRC_LAUNCH(DD, HH, GG, 32, THR);        \
    else RC_CIRC_LAUNCH(DD, HH, GG, 16, THR);                                                                        \
  }
  RCMARL_CIRC_COMBOS(RC_CIRC_CASE)
#undef RC_CIRC_CASE
#undef RC_CIRC_LAUNCH
  return rc;
}

// Irregular graphs: all (d, H) classes of the cooperative agents in one launch (k_consensus_params_ragged above).  `classes` is
// HOST memory, read during the call only.  More than RC_RAGGED_MAX_CLASSES classes: one launch per 32 of them.
RCMARL_EXPORT int rcmarl_consensus_params_ragged(const float* msg, float* theta, const int* nbr_off, const int* nbr_idx,
                                                 const int* order, const rcmarl_ragged_class* classes, int n_classes, int S,
                                                 int N, int ldp, int P_hid, float* lo_dbg, float* hi_dbg, void* stream) {
  if (!msg || !theta || !nbr_off || !nbr_idx || !order || !classes || n_classes <= 0 || S <= 0 || N <= 0 || (ldp & 63) ||
      P_hid <= 0 || P_hid > ldp || (!!lo_dbg != !!hi_dbg))
    return RCMARL_ERR_ARG;
  for (int q = 0; q < n_classes; ++q) {
    const rcmarl_ragged_class& k = classes[q];
    if (k.d <= 0 || k.d > N || k.H < 0 || k.d < 2 * k.H + 1 || k.first < 0 || k.count <= 0 || k.first > N - k.count)
      return RCMARL_ERR_ARG;
  }
  // widest column tile whose [N][TC] fp32 image fits 64 KiB of LDS, as rcmarl_consensus_params
  int log2tc = 6;
  while (log2tc > 2 && ((size_t)N << log2tc) * sizeof(float) > 64 * 1024) --log2tc;
  if (((size_t)N << log2tc) * sizeof(float) > 64 * 1024) return RCMARL_ERR_UNSUPPORTED;
  const int TC = 1 << log2tc;
  const size_t smem = ((size_t)N << log2tc) * sizeof(float);
  const int tiles_per_seed = rc_ceil_div(P_hid, TC), total_tiles = tiles_per_seed * S;
  // resident workgroups only (the tile walk is persistent): the kernel's 224 VGPRs leave 2 wavefronts per SIMD = 2 workgroups of 256
  // threads per CU, whatever the LDS would allow
  int wg_per_cu = (int)((160 * 1024) / (smem + 512));
  if (wg_per_cu > 2) wg_per_cu = 2;
  if (wg_per_cu < 1) wg_per_cu = 1;
  int nwg = rc_persistent_grid(256 * wg_per_cu);
  if (nwg > total_tiles) nwg = total_tiles;
  if (!k1_want_lds(k_consensus_params_ragged, smem)) return RCMARL_ERR_LAUNCH;
  for (int q0 = 0; q0 < n_classes; q0 += RC_RAGGED_MAX_CLASSES) {
    RaggedClasses cls;
    cls.n = n_classes - q0 < RC_RAGGED_MAX_CLASSES ? n_classes - q0 : RC_RAGGED_MAX_CLASSES;
    for (int q = 0; q < RC_RAGGED_MAX_CLASSES; ++q) {
      const bool in = q < cls.n;
      cls.d[q] = in ? classes[q0 + q].d : 0; cls.H[q] = in ? classes[q0 + q].H : 0;
      cls.first[q] = in ? classes[q0 + q].first : 0; cls.count[q] = in ? classes[q0 + q].count : 0;
    }
    RCMARL_LAUNCH(k_consensus_params_ragged, dim3(nwg), dim3(256), smem, stream, msg, theta, nbr_off, nbr_idx, order, cls, N, ldp,
                  P_hid, log2tc, tiles_per_seed, total_tiles, lo_dbg, hi_dbg);
    const int rc = rcmarl_check_launch();
    if (rc != RCMARL_OK) return rc;
  }
  return RCMARL_OK;
}

// ---- clip report (k_clip_counts above; include/rcmarl.h has the contract) ----------------------------------------------------
RCMARL_EXPORT int rcmarl_consensus_clip_counts_scratch(int S, int N, int ldc, int P_hid) {
  const ClipPlan p = clip_plan(S, N, ldc, P_hid);
  return p.ok ? (int)p.scratch_ints : 0;
}

RCMARL_EXPORT int rcmarl_consensus_clip_counts(const float* msg, const int* nbr, const int* coop, long long* below,
                                               long long* above, int* scratch, int S, int N, int ldp, int P_hid, int d, int H,
                                               int ldc, void* stream) {
  if (!msg || !nbr || !coop || !below || !above || S <= 0 || N <= 0 || d <= 0 || H < 0 || d < 2 * H + 1 || d > N || ldc < d ||
      (ldp & 63) || P_hid <= 0 || P_hid > ldp)
    return RCMARL_ERR_ARG;
  const ClipPlan p = clip_plan(S, N, ldc, P_hid);
  if (p.ok && p.scratch_ints > 0 && !scratch) return RCMARL_ERR_ARG;
  if (H == 0) return RCMARL_OK;                            // the window is [min, max]: nothing can be clipped
  if (!p.ok) return RCMARL_ERR_UNSUPPORTED;
  ClipGraph g{nbr, coop, d, nullptr, nullptr, nullptr};
  RaggedClasses cls{};
  cls.n = 1; cls.d[0] = d; cls.H[0] = H; cls.first[0] = 0; cls.count[0] = N;
  // a kernel of its own for the networks the switch of the general kernel leaves out (d > 20) and for the d = 2H+2 shapes of the
  // reference's graphs; every other generated network runs through the switch, any other (d, H) counts ranks
#define RC_CLIP_CASE(DD, HH)                                                                                          \
  if constexpr (HH > 0 && (DD > RC_RAGGED_MAX_NET_D || DD == 2 * HH + 2)) {                                            \
    if (d == DD && H == HH)                                                                                           \
      return clip_launch<DD, HH>(p, msg, g, cls, below, above, scratch, S, N, ldp, P_hid, ldc, stream);               \
  }
  RCMARL_SELNET_COMBOS(RC_CLIP_CASE)
#undef RC_CLIP_CASE
  return clip_launch<0, 0>(p, msg, g, cls, below, above, scratch, S, N, ldp, P_hid, ldc, stream);
}

RCMARL_EXPORT int rcmarl_consensus_clip_counts_ragged(const float* msg, const int* nbr_off, const int* nbr_idx, const int* order,
                                                      const rcmarl_ragged_class* classes, int n_classes, long long* below,
                                                      long long* above, int* scratch, int S, int N, int ldp, int P_hid, int ldc,
                                                      void* stream) {
  if (!msg || !nbr_off || !nbr_idx || !order || !classes || !below || !above || n_classes <= 0 || S <= 0 || N <= 0 || ldc <= 0 ||
      (ldp & 63) || P_hid <= 0 || P_hid > ldp)
    return RCMARL_ERR_ARG;
  bool any = false;
  for (int q = 0; q < n_classes; ++q) {
    const rcmarl_ragged_class& k = classes[q];
    if (k.d <= 0 || k.d > N || k.H < 0 || k.d < 2 * k.H + 1 || k.first < 0 || k.count <= 0 || k.first > N - k.count || ldc < k.d)
      return RCMARL_ERR_ARG;
    any = any || k.H > 0;
  }
  const ClipPlan p = clip_plan(S, N, ldc, P_hid);
  if (p.ok && p.scratch_ints > 0 && !scratch) return RCMARL_ERR_ARG;
  if (!any) return RCMARL_OK;
  if (!p.ok) return RCMARL_ERR_UNSUPPORTED;
  ClipGraph g{nullptr, nullptr, 0, nbr_off, nbr_idx, order};
  for (int q0 = 0; q0 < n_classes; q0 += RC_RAGGED_MAX_CLASSES) {      // (the fold of a chunk runs before the next chunk's counts)
    RaggedClasses cls{};
    cls.n = n_classes - q0 < RC_RAGGED_MAX_CLASSES ? n_classes - q0 : RC_RAGGED_MAX_CLASSES;
    bool chunk_any = false;
    for (int q = 0; q < cls.n; ++q) {
      cls.d[q] = classes[q0 + q].d; cls.H[q] = classes[q0 + q].H;
      cls.first[q] = classes[q0 + q].first; cls.count[q] = classes[q0 + q].count;
      chunk_any = chunk_any || cls.H[q] > 0;
    }
    if (!chunk_any) continue;
    const int rc = clip_launch<0, 0>(p, msg, g, cls, below, above, scratch, S, N, ldp, P_hid, ldc, stream);
    if (rc != RCMARL_OK) return rc;
  }
  return RCMARL_OK;
}
