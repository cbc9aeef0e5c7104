// Fast path of the two layer-1 GEMMs (included by layer1_gemm.hip).
//
// Same math as the generic kernels in layer1_gemm.hip, restructured for the shapes that carry
// the time (in_dim % 32 == 0, hid == 20): every global->LDS move is a branch-free 16-byte
// access, the epilogue's per-row constants are staged once, and LDS->register fragment loads
// are issued one MFMA step ahead.
//
// Both GEMMs are written as   D[m][n] = sum_s A[s][m] * B[n][s]   with
//   forward   m = (agent,unit) column of W1, n = replay row b,     s = input feature k
//   backward  m = input feature k,           n = (agent,unit) col, s = replay row b
// and in both the two operand tiles arrive exactly as they lie in memory:
//   As[s][m]  : rows contiguous along m  (W1 rows: 20-float chunks per agent | X rows)
//   Bs[n][s]  : rows contiguous along s  (X rows                            | dz1t rows)
// v_mfma_f32_32x32x2_f32 takes ONE A and ONE B float per lane (A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]).
// The reduction index may be visited in any order as long as A and B agree, so step (g,c) of a
// 32-deep tile uses s = 8g+c in lanes 0-31 and s = 8g+4+c in lanes 32-63: a lane then needs FOUR
// CONSECUTIVE s of its B row per g -> one ds_read_b128 from Bs[n][8g+4*half] (row stride 36 floats:
// the 16-lane groups of ds_read_b128 hit 16 distinct 16-B bank groups), no transposition anywhere.
//
// Workgroup = 256 threads = 4 wavefronts; wave w owns the 32 columns n0+32w.. and ALL MT 32-row
// m-tiles (MT accumulators of 16 VGPRs): per step MT MFMAs for MT A-fragment reads + 1/4 B read.

namespace fast {

constexpr int FBK = 32;          // reduction depth per tile
constexpr int FBN = 128;         // n extent per workgroup
constexpr int FBS = FBK + 4;     // Bs row stride (floats)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 sel4(bool ok, const float4& v) { return ok ? v : zero4(); }

// ---- operand loaders: fetch(tile index s0) -> registers, commit(registers) -> LDS ------------
// forward A: W1 of the 8 agents of this m-tile; per agent the 32x20 block [k][j] is contiguous
template <int MT> struct FwdA {
  static constexpr int BM = 32 * MT, NF4 = FBK * BM / 4, PER = (NF4 + 255) / 256;   // MT=5: 1280 float4, 5 per thread
  const float* theta_s; int ldp, N, agent0;
  __device__ __forceinline__ void fetch(int s0, float4 (&r)[PER]) const {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int f = threadIdx.x + 256 * q;
      const int a = f / (FBK * 5), w = f - a * (FBK * 5);            // 160 float4 per agent
      const int ag = agent0 + a;
      const bool ok = (NF4 % 256 == 0 || f < NF4) && ag < N;
      r[q] = sel4(ok, ld4(theta_s + (long)(ok ? ag : 0) * ldp + (long)s0 * 20 + 4 * (ok ? w : 0)));
    }
  }
  __device__ __forceinline__ void commit(const float4 (&r)[PER], float* As) const {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int f = threadIdx.x + 256 * q;
      if (NF4 % 256 == 0 || f < NF4) {
        const int a = f / (FBK * 5), w = f - a * (FBK * 5);
        st4(As + (w / 5) * BM + a * 20 + 4 * (w % 5), r[q]);
      }
    }
  }
};

// backward A: X rows (s = replay row b, m = input feature), zero beyond B and beyond in_dim
template <int MT> struct BwdA {
  static constexpr int BM = 32 * MT, NF4 = FBK * BM / 4, PER = NF4 / 256;           // MT=4: 1024 float4, 4 per thread
  const float* x_s; int in_dim, B, m0;
  __device__ __forceinline__ void fetch(int s0, float4 (&r)[PER]) const {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int f = threadIdx.x + 256 * q;
      const int bl = f / (BM / 4), w = f - bl * (BM / 4);
      const bool ok = (s0 + bl) < B && (m0 + 4 * w) < in_dim;
      r[q] = sel4(ok, ld4(x_s + (long)(ok ? s0 + bl : 0) * in_dim + (ok ? m0 + 4 * w : 0)));
    }
  }
  __device__ __forceinline__ void commit(const float4 (&r)[PER], float* As) const {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int f = threadIdx.x + 256 * q;
      const int bl = f / (BM / 4), w = f - bl * (BM / 4);
      st4(As + bl * BM + 4 * w, r[q]);
    }
  }
};

// B operand of both GEMMs: 128 rows n, 32 consecutive s each (8 float4 per row).
// forward: row n = replay row (X[b][s0..]); backward: row n = column of dz1t (dz1t[col][s0..]).
struct RowsB {
  static constexpr int PER = FBN * FBK / 4 / 256;     // 4 float4 per thread
  const float* src; long ld; int n_lim, s_lim, n0;    // s >= s_lim reads as zero (only used by backward)
  bool mask_s;
  __device__ __forceinline__ void fetch(int s0, float4 (&r)[PER]) const {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int f = threadIdx.x + 256 * q;
      const int nl = f >> 3, sq = f & 7;
      const int n = n0 + nl;
      const bool ok = n < n_lim;
      float4 v = ld4(src + (long)(ok ? n : 0) * ld + s0 + 4 * sq);
      if (mask_s) {
        const int s = s0 + 4 * sq;
        v.x = s + 0 < s_lim ? v.x : 0.f; v.y = s + 1 < s_lim ? v.y : 0.f;
        v.z = s + 2 < s_lim ? v.z : 0.f; v.w = s + 3 < s_lim ? v.w : 0.f;
      }
      r[q] = v;
    }
  }
  __device__ __forceinline__ void commit(const float4 (&r)[PER], float* Bs) const {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int f = threadIdx.x + 256 * q;
      st4(Bs + (f >> 3) * FBS + 4 * (f & 7), r[q]);
    }
  }
};

// ---- the tile loop ---------------------------------------------------------------------------
// One LDS buffer per operand; the next tile waits in registers (a double-buffered LDS form measured slower).
template <int MT, class LA, class LB>
__device__ __forceinline__ void mainloop(const LA& la, const LB& lb, int n_tiles, float* As, float* Bs,
                                         rc_f32x16 (&acc)[MT]) {
  constexpr int BM = 32 * MT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
  float4 ra[LA::PER], rb[LB::PER];
  la.fetch(0, ra);
  lb.fetch(0, rb);
  for (int t = 0; t < n_tiles; ++t) {
    __syncthreads();               // previous tile fully consumed
    la.commit(ra, As);
    lb.commit(rb, Bs);
    __syncthreads();
    if (t + 1 < n_tiles) { la.fetch((t + 1) * FBK, ra); lb.fetch((t + 1) * FBK, rb); }
    const float* arow = As + (4 * half) * BM + l31;                 // As[8g+4half+c][32mt+l31]
    const float* brow = Bs + (wave * 32 + l31) * FBS + 4 * half;    // Bs[n][8g+4half .. +3]
    float4 bq = ld4(brow);
    float af[2][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) af[0][mt] = arow[32 * mt];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int g = st >> 2, c = st & 3;
      float4 bnext = bq;
      if (st + 1 < 16) {             // fragments of the next step are requested before this step's MFMAs
        const int g1 = (st + 1) >> 2, c1 = (st + 1) & 3;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[(st + 1) & 1][mt] = arow[(8 * g1 + c1) * BM + 32 * mt];
        if (c1 == 0) bnext = ld4(brow + 8 * g1);
      }
      const float bv = c == 0 ? bq.x : (c == 1 ? bq.y : (c == 2 ? bq.z : bq.w));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[st & 1][mt], bv, acc[mt], 0, 0, 0);
      bq = bnext;
      (void)g;
    }
  }
}

// ---- forward: a1t[col][b] = lrelu(z + b1[col]) ------------------------------------------------
__global__ __launch_bounds__(256, 3) void k_fwd(const float* __restrict__ x, long x_seed_stride,
                                             const float* __restrict__ theta, float* __restrict__ a1t, int N, int B,
                                             int in_dim, int ldp, int ldb) {
  constexpr int MT = 5, BM = 160;
  RCMARL_DYN_SMEM(float, smem);
  float* As = smem;
  float* Bs = As + FBK * BM;
  float* bias = Bs + FBN * FBS;                            // [BM]
  const int s = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * FBN;
  const int ncols = N * 20;
  const float* theta_s = theta + (long)s * N * ldp;
  float* a1t_s = a1t + (long)s * ncols * ldb;
  if (threadIdx.x < BM) {
    const int col = m0 + threadIdx.x;
    const int ag = col / 20;
    bias[threadIdx.x] = col < ncols ? theta_s[(long)ag * ldp + in_dim * 20 + (col - ag * 20)] : 0.f;
  }
  const FwdA<MT> la{theta_s, ldp, N, m0 / 20};
  const RowsB lb{x + (long)s * x_seed_stride, (long)in_dim, B, 0, n0, false};
  rc_f32x16 acc[MT];
  mainloop<MT>(la, lb, in_dim / FBK, As, Bs, acc);         // (its barriers publish bias[])
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = n0 + wave * 32 + (lane & 31);
  if (n < B) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m0 + ml < ncols) a1t_s[(long)(m0 + ml) * ldb + n] = rc_lrelu(acc[mt][r] + bias[ml]);
      }
  }
}

// ---- backward: W1[k][col] <- optimiser(W1[k][col], sum_b X[b][k]*dz1t[col][b]) ------------------
struct ApplySgd {
  float lr;
  __device__ __forceinline__ void operator()(float* w, long, float g) const { *w = *w - lr * g; }
};
struct ApplyAdam {      // TF2 ResourceApplyAdam (see EpiAdam)
  float* m_s; float* v_s; float alpha, one_m_b1, one_m_b2, eps;
  __device__ __forceinline__ void operator()(float* w, long o, float g) const {
    float mm = m_s[o], vv = v_s[o], wv = *w;
    rc_adam_apply(g, wv, mm, vv, alpha, one_m_b1, one_m_b2, eps);
    m_s[o] = mm; v_s[o] = vv;
    *w = wv;
  }
};

template <class Apply>
__global__ __launch_bounds__(256) void k_bwd(const float* __restrict__ x, long x_seed_stride,
                                             const float* __restrict__ dz1t, float* __restrict__ theta,
                                             const int* __restrict__ mask, int N, int B, int in_dim, int ldp, int ldb,
                                             Apply apply) {
  constexpr int MT = 4, BM = 128;
  RCMARL_DYN_SMEM(float, smem);
  float* As = smem;
  float* Bs = As + FBK * BM;
  const int s = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * FBN;
  const int ncols = N * 20;
  const BwdA<MT> la{x + (long)s * x_seed_stride, in_dim, B, m0};
  const RowsB lb{dz1t + (long)s * ncols * ldb, (long)ldb, ncols, B, n0, true};
  rc_f32x16 acc[MT];
  mainloop<MT>(la, lb, (B + FBK - 1) / FBK, As, Bs, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = n0 + wave * 32 + (lane & 31);
  if (col < ncols) {
    const int ag = col / 20, j = col - ag * 20;
    if (mask == nullptr || mask[ag]) {
      const long so = (long)s * N * ldp + (long)ag * ldp + j;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = m0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (k < in_dim) {
            const long o = so + (long)k * 20;
            apply(theta + o, o, acc[mt][r]);
          }
        }
    }
  }
}

inline size_t smem_fwd() { return sizeof(float) * (FBK * 160 + FBN * FBS + 160); }
inline size_t smem_bwd() { return sizeof(float) * (FBK * 128 + FBN * FBS); }

}  // namespace fast
