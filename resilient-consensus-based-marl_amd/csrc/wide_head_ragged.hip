// K2+K3 for a wide head (any hidden width) on an IRREGULAR in-graph: rcmarl_wide_consensus_head_ragged.
//
// The uniform chain (rcmarl_wide_consensus_head, wide_kernels.hip) gathers the neighbours' heads into hmat [S][N][d+1][hid], runs the
// 128 x 128 GEMM tile on its d + 1 rows, materialises est [S][N][d+1][ldb] and selects in a third launch -- all sized by ONE d.  Here one
// kernel does gather + skinny GEMM + selection + residual per (seed, agent, chunk of 128 replay rows), with the agent's own d_i and the
// H of its class, and needs no scratch:
//
//   estimates   V_m[b] = phi[:, b] . W3_m + b3_m on v_mfma_f32_32x32x2_f32: the heads are the 32 A-rows of a tile (ceil((d_i + 1) / 32)
//               tiles, slot d_i = the live head), the replay rows the B-columns (each of the 4 wavefronts owns 32 of the 128), k runs
//               over hid.  Both operands pass through LDS in k-tiles of 16 as [k][m] / [k][row] (one float per lane per operand is the
//               instruction's contract; a half-wavefront reads 32 consecutive banks), register-prefetched double buffer, one barrier
//               per k-tile.  The heads are read straight from the msg rows through the CSR; phi is feature-major, so a k-row of the
//               B tile is one contiguous segment, loaded 16 bytes wide where the alignment allows.
//   order       accumulators start at zero, k-pairs (0,1), (2,3), .. ascending through ONE accumulator per estimate, k never split
//               across wavefronts, zero padding beyond hid, b3 added afterwards: the order of w_loop_f32 + WEPI_BIAS, so on a regular
//               graph the estimates carry the bits of the uniform entry (the instruction is bitwise an fmaf chain).
//   |phi|^2     with nparts: their sum in w_norm1's order; without: accumulated by the lanes that feed the B operand in the same pass
//               (even k in lanes 0-31, odd k in lanes 32-63, the two added at the end) -- phi is read once.
//   selection   the accumulators go to LDS as [m][row] (over the staging buffers); one thread per replay row counts ranks with index
//               tie-break at run time (any d, H: k_wselect's statement), clamps with fmed3, sums in ascending m, divides by d.
//   grads       k_wrows<WROW_DOT> (rcmarl_wide_rows.h) over the agents of the call's classes: second and last launch.
#include "rcmarl_common.h"
#include "rcmarl_wide_rows.h"

namespace {

constexpr int RH_ROWS = 128;             // replay rows per workgroup: 4 wavefronts x 32 MFMA columns
constexpr int RH_KT = 16;                // k-tile
constexpr int RH_BLD = RH_ROWS + 4;      // floats per k-row of the B tile in LDS (16-byte aligned rows)
constexpr int RH_MAX_TILES = 4;          // head tiles of 32 (d + 1 <= 128)
constexpr int RH_MAX_CLASSES = 32;       // classes per launch (the entry point issues further launches beyond)
constexpr size_t RH_LDS_LIMIT = 64 * 1024;      // per workgroup: two resident on a CU's 160 KiB, no opt-in to more dynamic LDS

struct RhClasses {
  int n;
  int d[RH_MAX_CLASSES], H[RH_MAX_CLASSES], first[RH_MAX_CLASSES], count[RH_MAX_CLASSES];
};

struct RhArgs {
  const float* phi; const float* nparts; int n_parts;
  const float* theta; const float* msg;
  const int* nbr_off; const int* nbr_idx; const int* order;
  float* ebuf; float* agg_out; float* est_dbg; int lde;
  int N, B, in_dim, hid, ldp, ldb, vec;
};

__host__ __device__ static inline int rh_tiles(int d) { return (d + 1 + 31) / 32; }
__host__ __device__ static inline int rh_ald(int nt) { return nt * 32 + 2; }      // [k][m] stride: the 16 k x 2 m a half-wavefront
                                                                                  // stores land on 32 different banks
// floats of the region the staging buffers and the estimates share
__host__ __device__ static inline int rh_shared_floats(int d) {
  const int stage = 2 * RH_KT * (rh_ald(rh_tiles(d)) + RH_BLD), est = (d + 1) * RH_ROWS;
  return stage > est ? stage : est;
}
// + |phi|^2 halves [2][RH_ROWS], b3 per slot, source agent per slot
static inline size_t rh_smem(int d) { return ((size_t)rh_shared_floats(d) + 2 * RH_ROWS + 2 * RH_MAX_TILES * 32) * sizeof(float); }

template <int NT>
__device__ __forceinline__ void rh_load_a(const RhArgs& a, const int* __restrict__ s_src, int s, int d, int o_W3, int k0, float (&ra)[2 * NT]) {
#pragma unroll
  for (int q = 0; q < 2 * NT; ++q) {
    const int idx = threadIdx.x + 256 * q, m = idx >> 4, k = k0 + (idx & 15);
    float v = 0.f;
    if (m <= d && k < a.hid) {
      const float* __restrict__ row = (m < d ? a.msg : a.theta) + ((long)s * a.N + s_src[m]) * a.ldp;
      v = row[o_W3 + k];
    }
    ra[q] = v;
  }
}

template <int NT>
__device__ __forceinline__ void rh_store_a(float* __restrict__ sA, const float (&ra)[2 * NT]) {
#pragma unroll
  for (int q = 0; q < 2 * NT; ++q) {
    const int idx = threadIdx.x + 256 * q;
    sA[(idx & 15) * rh_ald(NT) + (idx >> 4)] = ra[q];
  }
}

// this thread's 8 floats of the [16 k][128 rows] tile of phi (zero beyond hid; columns beyond B are never read back)
__device__ __forceinline__ void rh_load_b(const RhArgs& a, const float* __restrict__ P, int b0, int k0, float (&rb)[8]) {
  const int t = threadIdx.x;
  if (a.vec) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = t + 256 * q, k = k0 + (idx >> 5), r4 = (idx & 31) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < a.hid && b0 + r4 < a.B) v = *reinterpret_cast<const float4*>(P + (long)k * a.ldb + b0 + r4);      // (ldb % 4 == 0: inside the row)
      rb[4 * q] = v.x; rb[4 * q + 1] = v.y; rb[4 * q + 2] = v.z; rb[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q, k = k0 + (idx >> 7), r = idx & 127;
      rb[q] = (k < a.hid && b0 + r < a.B) ? P[(long)k * a.ldb + b0 + r] : 0.f;
    }
  }
}

__device__ __forceinline__ void rh_store_b(const RhArgs& a, float* __restrict__ sB, const float (&rb)[8]) {
  const int t = threadIdx.x;
  if (a.vec) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = t + 256 * q;
      *reinterpret_cast<float4*>(sB + (idx >> 5) * RH_BLD + (idx & 31) * 4) = make_float4(rb[4 * q], rb[4 * q + 1], rb[4 * q + 2], rb[4 * q + 3]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q;
      sB[(idx >> 7) * RH_BLD + (idx & 127)] = rb[q];
    }
  }
}

// one (seed s, agent i with in-degree d and trim parameter H, replay rows b0 .. b0 + 127)
template <int NT>
__device__ __forceinline__ void rh_body(const RhArgs& a, float* __restrict__ smem, int s, int i, int d, int H, int b0) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  constexpr int ALD = NT * 32 + 2;
  float* __restrict__ sA = smem;                                  // [2][RH_KT][ALD]
  float* __restrict__ sB = smem + 2 * RH_KT * ALD;                // [2][RH_KT][RH_BLD]
  float* __restrict__ sE = smem;                                  // [d + 1][RH_ROWS], once the k-loop is done
  float* __restrict__ sN = smem + rh_shared_floats(d);            // [2][RH_ROWS]
  float* __restrict__ s_b3 = sN + 2 * RH_ROWS;                    // [NT * 32]
  int* __restrict__ s_src = reinterpret_cast<int*>(s_b3 + RH_MAX_TILES * 32);
  const NetGeom g = make_geom(a.in_dim, a.hid, 1);
  const long zi = (long)s * a.N + i;
  if (t <= d) {
    const int j = t < d ? a.nbr_idx[a.nbr_off[i] + t] : i;
    s_src[t] = j;
    s_b3[t] = ((t < d ? a.msg : a.theta) + ((long)s * a.N + j) * a.ldp)[g.o_b3];
  }
  __syncthreads();
  const float* __restrict__ P = a.phi + zi * a.hid * a.ldb;
  rc_f32x16 acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  float nrm = 0.f;
  float ra[2 * NT], rb[8];
  const int nk = (a.hid + RH_KT - 1) / RH_KT;
  rh_load_a<NT>(a, s_src, s, d, g.o_W3, 0, ra);
  rh_load_b(a, P, b0, 0, rb);
  rh_store_a<NT>(sA, ra);
  rh_store_b(a, sB, rb);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      rh_load_a<NT>(a, s_src, s, d, g.o_W3, (kt + 1) * RH_KT, ra);
      rh_load_b(a, P, b0, (kt + 1) * RH_KT, rb);
    }
    const float* __restrict__ pa = sA + cur * (RH_KT * ALD) + (l >> 5) * ALD + (l & 31);
    const float* __restrict__ pb = sB + cur * (RH_KT * RH_BLD) + (l >> 5) * RH_BLD + w * 32 + (l & 31);
#pragma unroll
    for (int kk = 0; kk < RH_KT; kk += 2) {
      const float bv = pb[kk * RH_BLD];
      nrm = fmaf(bv, bv, nrm);
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk * ALD + q * 32], bv, acc[q], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      rh_store_a<NT>(sA + (cur ^ 1) * (RH_KT * ALD), ra);
      rh_store_b(a, sB + (cur ^ 1) * (RH_KT * RH_BLD), rb);
    }
    __syncthreads();
  }
  // register r of tile q is estimate m = q*32 + (r&3) + 8*(r>>2) + 4*(l>>5) of replay row w*32 + (l&31)
  {
    const int col = w * 32 + (l & 31);
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = q * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        if (m <= d) sE[m * RH_ROWS + col] = acc[q][r] + s_b3[m];
      }
    sN[(l >> 5) * RH_ROWS + col] = nrm;
  }
  __syncthreads();
  const int r = t, b = b0 + r;
  if (r >= RH_ROWS || b >= a.B) return;                           // no barrier below: every thread works on its own LDS column
  float n1 = 0.f;
  if (a.nparts != nullptr) {
    for (int p = 0; p < a.n_parts; ++p) n1 += a.nparts[(zi * a.n_parts + p) * a.ldb + b];
  } else {
    n1 = sN[r] + sN[RH_ROWS + r];
  }
  n1 += 1.0f;
  const float own = sE[r];
  float lo = own, hi = own;
  for (int k = 0; k < d; ++k) {
    const float x = sE[k * RH_ROWS + r];
    int rank = 0;
    for (int m = 0; m < d; ++m) {
      const float yv = sE[m * RH_ROWS + r];
      rank += (yv < x || (yv == x && m < k)) ? 1 : 0;
    }
    if (rank == H) lo = x;
    if (rank == d - H - 1) hi = x;
  }
  const float lower = fminf(lo, own), upper = fmaxf(hi, own);
  float sum = 0.f;
  for (int k = 0; k < d; ++k) sum += __builtin_amdgcn_fmed3f(sE[k * RH_ROWS + r], lower, upper);
  const float agg = sum / (float)d;
  const long o = zi * a.ldb + b;
  a.ebuf[o] = (agg - sE[d * RH_ROWS + r]) / n1;
  if (a.agg_out) a.agg_out[o] = agg;
  if (a.est_dbg)
    for (int m = 0; m <= d; ++m) a.est_dbg[(zi * a.lde + m) * a.ldb + b] = sE[m * RH_ROWS + r];
}

// grid: (row chunks, agents of the launch's classes, seeds)
__global__ __launch_bounds__(256) void k_whead_ragged(const RhArgs a, const RhClasses cls) {
  RCMARL_DYN_SMEM(float, smem);
  int pos = blockIdx.y, q = 0;
  while (q < cls.n && pos >= cls.count[q]) pos -= cls.count[q++];
  if (q >= cls.n) return;                                         // (workgroup-uniform)
  const int d = cls.d[q], H = cls.H[q], i = a.order[cls.first[q] + pos];
  const int s = blockIdx.z, b0 = blockIdx.x * RH_ROWS;
  switch (rh_tiles(d)) {
    case 1: rh_body<1>(a, smem, s, i, d, H, b0); break;
    case 2: rh_body<2>(a, smem, s, i, d, H, b0); break;
    case 3: rh_body<3>(a, smem, s, i, d, H, b0); break;
    default: rh_body<4>(a, smem, s, i, d, H, b0); break;
  }
}

static inline bool rh_al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// does the fused kernel serve a hid-unit head on in-neighbourhoods up to d_max?  (d_max + 1 estimates of 128 replay rows, or the
// staging buffers of the k-loop, beside the small per-slot arrays inside 64 KiB of LDS: two workgroups per CU; at most 4 head tiles)
RCMARL_EXPORT int rcmarl_wide_consensus_head_ragged_supported(int hid, int d_max) {
  if (hid < 1 || d_max < 1 || rh_tiles(d_max) > RH_MAX_TILES) return 0;
  return rh_smem(d_max) <= RH_LDS_LIMIT ? 1 : 0;
}

RCMARL_EXPORT int rcmarl_wide_consensus_head_ragged(const float* phi, const float* nparts, int n_parts, const float* theta,
                                                    const float* msg, const int* nbr_off, const int* nbr_idx, const int* order,
                                                    const rcmarl_ragged_class* classes, int n_classes, float* ebuf, float* grads,
                                                    float* agg_out, float* est_dbg, int lde, int S, int N, int B, int in_dim,
                                                    int hid, int ldp, int ldb, void* stream) {
  if (!phi || !theta || !msg || !nbr_off || !nbr_idx || !order || !classes || !ebuf || !grads || n_classes <= 0 ||
      (nparts != nullptr && n_parts <= 0) || !w_dims_ok(S, N, B, in_dim, hid, ldp, ldb))
    return RCMARL_ERR_ARG;
  int dmax = 0;
  for (int q = 0; q < n_classes; ++q) {
    const rcmarl_ragged_class& k = classes[q];
    if (k.d <= 0 || k.d > N || k.H < 0 || k.d < 2 * k.H + 1 || k.first < 0 || k.count <= 0 || k.first > N - k.count)
      return RCMARL_ERR_ARG;
    dmax = k.d > dmax ? k.d : dmax;
  }
  if (est_dbg != nullptr && lde < dmax + 1) return RCMARL_ERR_ARG;
  if (!rcmarl_wide_consensus_head_ragged_supported(hid, dmax)) return RCMARL_ERR_UNSUPPORTED;
  RhArgs a{};
  a.phi = phi; a.nparts = nparts; a.n_parts = nparts ? n_parts : 0; a.theta = theta; a.msg = msg;
  a.nbr_off = nbr_off; a.nbr_idx = nbr_idx; a.order = order;
  a.ebuf = ebuf; a.agg_out = agg_out; a.est_dbg = est_dbg; a.lde = lde;
  a.N = N; a.B = B; a.in_dim = in_dim; a.hid = hid; a.ldp = ldp; a.ldb = ldb;
  a.vec = (rh_al4(phi) && !(ldb & 3)) ? 1 : 0;                   // every k-row segment of every (seed, agent) 16-byte aligned
  for (int q0 = 0; q0 < n_classes; q0 += RH_MAX_CLASSES) {
    RhClasses cls{};
    cls.n = n_classes - q0 < RH_MAX_CLASSES ? n_classes - q0 : RH_MAX_CLASSES;
    int agents = 0, dm = 0;
    for (int q = 0; q < cls.n; ++q) {
      cls.d[q] = classes[q0 + q].d; cls.H[q] = classes[q0 + q].H;
      cls.first[q] = classes[q0 + q].first; cls.count[q] = classes[q0 + q].count;
      agents += cls.count[q];
      dm = cls.d[q] > dm ? cls.d[q] : dm;
    }
    RCMARL_LAUNCH(k_whead_ragged, dim3(rc_ceil_div(B, RH_ROWS), agents, S), dim3(256), rh_smem(dm), stream, a, cls);
    const int rc = rcmarl_check_launch();
    if (rc != RCMARL_OK) return rc;
  }
  // grads[s][i][0..hid] = [sum_b e phi | sum_b e] of the listed agents: one launch per run of classes that follow each other in
  // order[] (a class table sorted by class, as EngineConfig.consensus_classes() builds it, is ONE run)
  for (int q = 0; q < n_classes;) {
    const int first = classes[q].first;
    int end = first + classes[q].count;
    for (++q; q < n_classes && classes[q].first == end; ++q) end += classes[q].count;
    RCMARL_LAUNCH((k_wrows<WROW_DOT>), dim3(rc_ceil_div(hid + 1, 4), end - first, S), dim3(256), 0, stream, const_cast<float*>(phi),
                  (const float*)ebuf, (const float*)nullptr, (const int*)nullptr, grads, 0, N, B, in_dim, hid, ldp, ldb, order + first);
    const int rc = rcmarl_check_launch();
    if (rc != RCMARL_OK) return rc;
  }
  return RCMARL_OK;
}
