// X1 for the widest networks -- the adversaries' mini-batch fits of a critic-family net whose THREE activation images no longer
// fit the LDS (csrc/minibatch_wide.hip refuses them: more than 384 units) but whose TWO do: 385 .. 576 units, BASELINE configs[4]'s
// 512 among them.  One whole Keras `fit(batch_size=32, epochs=10)` per workgroup, all (job, seed, adversary) chains of a consensus
// epoch in ONE launch, as there.  The step is the sibling's (one workgroup of four wavefronts per chain, a mini-batch = one 32-row
// tile of v_mfma_f32_32x32x2_f32, unit tile t owned by wavefront t % 4, parameters in the theta row in global memory and updated
// IN PLACE, a workgroup barrier between the stores of one phase and the loads of the next, every gradient of a step from the
// pre-step weights), with two differences:
//   * dz1 is written over a1.  In the backward pass through layer 2 the wavefront that owns unit tile `it` takes the a1 columns of
//     that tile into registers before its walk over the W2 tiles, is the only reader of those columns in that phase, and writes dz1
//     of the same columns after the walk (each lane reads a1 at the very position it then overwrites).  LDS holds a1 (dz1) | a2 (dz2),
//     the staged input chunk and the per-row scalars: 4 * (64 LD + 2144) + 128 bytes, 139.9 KB at 512 units, 156.4 KB at 576;
//   * the layer-1 forward walks the input chunks in its OUTER loop with the accumulators of all (at most five) unit tiles of the
//     wavefront live across it, so a chunk is staged once per step there (and once in the W1 update) whatever the number of tiles
//     -- at in_dim = 2048 that is 32 stagings for 128.  The k order within a tile is unchanged: the arithmetic is the sibling's.
// Rows >= nb of a short last mini-batch carry dLoss/dv = 0, so they add nothing to any gradient; unit columns >= hid of the last
// tile are kept at zero.  Semantics: oracle/mlp_np.fit_mse (Keras SGD on the MSE loss, SUM_OVER_BATCH_SIZE).
#include "rcmarl_common.h"

RCMARL_EXPORT int rcmarl_minibatch_fit_wide_supported(int in_dim, int hid, int batch_size);      // csrc/minibatch_wide.hip

namespace {

constexpr int MW2_ROWS = 32;             // rows of a mini-batch tile = the largest batch_size served
constexpr int MW2_KC = 64;               // input columns staged per chunk
constexpr int MW2_XLD = MW2_KC + 1;      // LDS row stride of the staged chunk
constexpr int MW2_THREADS = 256, MW2_WAVES = 4, MW2_MAX_JOBS = 4;
constexpr int MW2_TU = 5;                // unit tiles a wavefront owns at most: 18 tiles (576 units) on four wavefronts
constexpr int MW2_MAX_HID = 1 << 16;     // (beyond any LDS; keeps the size arithmetic inside int)
constexpr size_t MW2_LDS_LIMIT = 160 * 1024;

struct Mw2Job {
  const float* x; long x_seed_stride; float* theta; const int* agents; const float* y; const int* perm; float* loss_out;
  int n_adv, in_dim, ldp, hid;
};
struct Mw2Args {
  Mw2Job job[MW2_MAX_JOBS];
  int first[MW2_MAX_JOBS + 1];           // block b belongs to job j with first[j] <= b < first[j + 1]
  int njobs, N, B, ldb, bs, epochs;
  float lr;
};

__host__ __device__ inline int mw2_ld(int hid) { return ((hid + 31) & ~31) + 1; }
// a1 (dz1) | a2 (dz2): [32][LD]; staged inputs [32][MW2_XLD]; dv[32] | loss[32] | row indices[32]
size_t mw2_smem_bytes(int hid) { return sizeof(float) * ((size_t)2 * MW2_ROWS * mw2_ld(hid) + MW2_ROWS * MW2_XLD + 2 * MW2_ROWS) + sizeof(int) * MW2_ROWS; }

// accumulator slot q of a lane in half h holds row mw2_drow(q, h) of the 32 x 32 product (column = lane & 31)
__device__ __forceinline__ int mw2_drow(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

__global__ __launch_bounds__(MW2_THREADS) void k_minibatch_wide2(Mw2Args m) {
  RCMARL_DYN_SMEM(float, smem);
  int jn = 0;
#pragma unroll
  for (int q = 1; q < MW2_MAX_JOBS; ++q) jn += (q < m.njobs && (int)blockIdx.x >= m.first[q]) ? 1 : 0;
  const Mw2Job a = m.job[jn];
  const int net = (int)blockIdx.x - m.first[jn];
  const int s = net / a.n_adv, adv = net - s * a.n_adv;
  const int hid = a.hid, in = a.in_dim, LD = mw2_ld(hid), ntiles = (hid + 31) >> 5, TU = (ntiles + MW2_WAVES - 1) / MW2_WAVES;
  const NetGeom g = make_geom(in, hid, 1);
  float* a1s = smem;                       // [32][LD]  a1, then dz1 in place
  float* a2s = a1s + MW2_ROWS * LD;        // [32][LD]  a2, then dz2 in place
  float* xs = a2s + MW2_ROWS * LD;         // [32][MW2_XLD] staged input chunk
  float* dvs = xs + MW2_ROWS * MW2_XLD;    // [32] dLoss/dv per row
  float* lossr = dvs + MW2_ROWS;           // [32]
  int* idxs = reinterpret_cast<int*>(lossr + MW2_ROWS);     // [32] replay rows of the mini-batch
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int agent = a.agents[adv];
  const long row = (long)s * m.N + agent;
  float* th = a.theta + row * a.ldp;
  const float* xg = a.x + (long)s * a.x_seed_stride;
  const float* yv = a.y + row * m.ldb;
  const int* perm = a.perm ? a.perm + ((long)s * a.n_adv + adv) * m.epochs * m.B : nullptr;
  const float lr = m.lr;
  const bool multi = in > MW2_KC;          // more input columns than one staged chunk: staged per chunk where they are needed
  float loss_part = 0.f;                   // threads (t & 7) == 0: sum over the epoch-0 batches of row t >> 3's squared error

  auto stage = [&](int k0) {
    for (int e = t; e < MW2_ROWS * MW2_KC; e += MW2_THREADS) {
      const int rr = e >> 6, kk = e & (MW2_KC - 1), k = k0 + kk;
      xs[rr * MW2_XLD + kk] = k < in ? xg[(long)idxs[rr] * in + k] : 0.f;
    }
  };

  for (int ep = 0; ep < m.epochs; ++ep) {
    for (int lo = 0; lo < m.B; lo += m.bs) {
      const int nb = min(m.bs, m.B - lo);
      if (t < MW2_ROWS) {
        const int p = lo + (t < nb ? t : 0);
        idxs[t] = perm ? perm[(long)ep * m.B + p] : p;
      }
      __syncthreads();
      if (!multi) {
        stage(0);
        __syncthreads();
      }
      // ---- layer 1: a1[r][j] = lrelu(sum_k x[r][k] W1[k][j] + b1[j]), k ascending.  Chunks outside, the wavefront's tiles inside:
      // one staged value feeds the (up to) MW2_TU independent accumulator chains
      {
        rc_f32x16 acc[MW2_TU];
#pragma unroll
        for (int u = 0; u < MW2_TU; ++u)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[u][q] = 0.f;
        for (int k0 = 0; k0 < in; k0 += MW2_KC) {
          if (multi) {
            __syncthreads();
            stage(k0);
            __syncthreads();
          }
          const int kc = min(MW2_KC, in - k0);
#pragma unroll 4
          for (int mm = 0; 2 * mm < kc; ++mm) {
            const int k = k0 + 2 * mm + h;
            const float av = xs[l31 * MW2_XLD + 2 * mm + h];
#pragma unroll
            for (int u = 0; u < MW2_TU; ++u) {
              const int jt = wave + MW2_WAVES * u, jc = jt * 32 + l31;
              if (jt < ntiles) {
                const bool ok = jc < hid && k < in;             // (a masked element loads th[0]: the loads stay straight-line code)
                const float wv = th[ok ? (long)k * hid + jc : 0];
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ok ? wv : 0.f, acc[u], 0, 0, 0);
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < MW2_TU; ++u) {
          const int jt = wave + MW2_WAVES * u, jc = jt * 32 + l31;
          if (jt < ntiles) {
            const float bias = jc < hid ? th[g.o_b1 + jc] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) a1s[mw2_drow(q, h) * LD + jc] = rc_lrelu(acc[u][q] + bias);
          }
        }
      }
      __syncthreads();
      // ---- layer 2: a2[r][j] = lrelu(sum_i a1[r][i] W2[i][j] + b2[j])
      for (int u = 0; u < TU; ++u) {
        const int jt = wave + MW2_WAVES * u, jc = jt * 32 + l31;
        const bool active = jt < ntiles, jok = active && jc < hid;
        if (active) {
          rc_f32x16 acc;
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll 8
          for (int mm = 0; 2 * mm < hid; ++mm) {
            const int i = 2 * mm + h;
            const float av = a1s[l31 * LD + i];
            const bool ok = jok && i < hid;
            const float wv = th[ok ? g.o_W2 + (long)i * hid + jc : 0];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ok ? wv : 0.f, acc, 0, 0, 0);
          }
          const float bias = jok ? th[g.o_b2 + jc] : 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) a2s[mw2_drow(q, h) * LD + jc] = rc_lrelu(acc[q] + bias);
        }
      }
      __syncthreads();
      // ---- head and loss gradient: eight threads per row
      {
        const int r = t >> 3, p = t & 7;
        float v = 0.f;
        for (int k = p; k < hid; k += 8) v = fmaf(a2s[r * LD + k], th[g.o_W3 + k], v);
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        if (p == 0) {
          const float diff = r < nb ? (v + th[g.o_b3]) - yv[idxs[r]] : 0.f;
          dvs[r] = (2.0f * diff) / (float)nb;                   // Keras MSE, SUM_OVER_BATCH_SIZE
          if (ep == 0) loss_part += diff * diff;
        }
      }
      __syncthreads();
      // ---- gW3, gb2 and dz2 = dv W3^T * lrelu'(z2) over a2 (one thread per unit; gW3 is taken before a2 is overwritten); gb3
      for (int k = t; k < hid; k += MW2_THREADS) {
        const float w3 = th[g.o_W3 + k];
        float g3 = 0.f, gb2 = 0.f;
        for (int r = 0; r < MW2_ROWS; ++r) {
          const float av = a2s[r * LD + k], d = dvs[r];
          g3 = fmaf(av, d, g3);
          const float dz = (d * w3) * rc_lrelu_grad_from_act(av);
          a2s[r * LD + k] = dz;
          gb2 += dz;
        }
        th[g.o_W3 + k] = w3 - lr * g3;
        th[g.o_b2 + k] = th[g.o_b2 + k] - lr * gb2;
      }
      if (t == MW2_THREADS - 1) {
        float gb3 = 0.f;
        for (int r = 0; r < MW2_ROWS; ++r) gb3 += dvs[r];
        th[g.o_b3] = th[g.o_b3] - lr * gb3;
      }
      __syncthreads();
      // ---- backward through layer 2.  The wavefront that owns unit tile `it` walks the tiles W2[it][jt]: the loaded tile gives
      // da1^T[i][r] += sum_j W2[i][j] dz2[r][j] (A operand, contraction slot (mm, half) = column mw2_drow(mm, half)) and takes
      // W2[i][j] -= lr * sum_r a1[r][i] dz2[r][j] (the product dz2^T a1 lands in the tile's own register layout).  The a1 columns of
      // the tile are in registers (a1f) before the walk and no other wavefront reads them in this phase: dz1 takes their place.
      for (int u = 0; u < TU; ++u) {
        const int it = wave + MW2_WAVES * u;
        if (it < ntiles) {
          const int ic = it * 32 + l31;
          const bool iok = ic < hid;
          float a1f[16];
#pragma unroll
          for (int mm = 0; mm < 16; ++mm) a1f[mm] = a1s[(2 * mm + h) * LD + ic];
          rc_f32x16 da;
#pragma unroll
          for (int q = 0; q < 16; ++q) da[q] = 0.f;
          for (int jt = 0; jt < ntiles; ++jt) {
            float* wt = th + g.o_W2 + (long)ic * hid + jt * 32;
            float w[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = (iok && jt * 32 + mw2_drow(q, h) < hid) ? wt[mw2_drow(q, h)] : 0.f;
            rc_f32x16 gw;
#pragma unroll
            for (int q = 0; q < 16; ++q) gw[q] = 0.f;
#pragma unroll
            for (int mm = 0; mm < 16; ++mm)
              gw = __builtin_amdgcn_mfma_f32_32x32x2f32(a2s[(2 * mm + h) * LD + jt * 32 + l31], a1f[mm], gw, 0, 0, 0);
#pragma unroll
            for (int mm = 0; mm < 16; ++mm)
              da = __builtin_amdgcn_mfma_f32_32x32x2f32(w[mm], a2s[l31 * LD + jt * 32 + mw2_drow(mm, h)], da, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 16; ++q)
              if (iok && jt * 32 + mw2_drow(q, h) < hid) wt[mw2_drow(q, h)] = w[q] - lr * gw[q];
          }
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int o = l31 * LD + it * 32 + mw2_drow(q, h);
            a1s[o] = da[q] * rc_lrelu_grad_from_act(a1s[o]);    // dz1 over a1
          }
        }
      }
      __syncthreads();
      // ---- gb1, and W1[k][j] -= lr * sum_r x[r][k] dz1[r][j]   (a1s holds dz1 now)
      for (int k = t; k < hid; k += MW2_THREADS) {
        float gb1 = 0.f;
        for (int r = 0; r < MW2_ROWS; ++r) gb1 += a1s[r * LD + k];
        th[g.o_b1 + k] = th[g.o_b1 + k] - lr * gb1;
      }
      for (int k0 = 0; k0 < in; k0 += MW2_KC) {
        if (multi) {
          __syncthreads();
          stage(k0);
          __syncthreads();
        }
        const int kc = min(MW2_KC, in - k0);
        for (int u = 0; u < TU; ++u) {
          const int jt = wave + MW2_WAVES * u, jc = jt * 32 + l31;
          if (jt < ntiles) {
            const bool jok = jc < hid;
            float dzf[16];
#pragma unroll
            for (int mm = 0; mm < 16; ++mm) dzf[mm] = a1s[(2 * mm + h) * LD + jc];
            for (int sub = 0; sub * 32 < kc; ++sub) {
              float w[16];                 // the tile's weights are on their way while the matrix core forms the gradient
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int k = k0 + sub * 32 + mw2_drow(q, h);
                w[q] = th[(jok && k < in) ? (long)k * hid + jc : 0];
              }
              rc_f32x16 gw;
#pragma unroll
              for (int q = 0; q < 16; ++q) gw[q] = 0.f;
#pragma unroll
              for (int mm = 0; mm < 16; ++mm)
                gw = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(2 * mm + h) * MW2_XLD + sub * 32 + l31], dzf[mm], gw, 0, 0, 0);
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int k = k0 + sub * 32 + mw2_drow(q, h);
                if (jok && k < in) th[(long)k * hid + jc] = w[q] - lr * gw[q];
              }
            }
          }
        }
      }
      __syncthreads();                     // this step's stores before the next step's loads; LDS free for the next mini-batch
    }
    if (ep == 0 && a.loss_out) {           // Keras History: first-epoch loss, the sample-weighted mean of the batch losses
      if ((t & 7) == 0) lossr[t >> 3] = loss_part;
      __syncthreads();
      if (t == 0) {
        float sum = 0.f;
        for (int q = 0; q < MW2_ROWS; ++q) sum += lossr[q];
        a.loss_out[row] = sum / (float)m.B;
      }
      __syncthreads();
    }
  }
}

}  // namespace

// 1 exactly for the widths the three-image layout of csrc/minibatch_wide.hip refuses and the two-image layout holds (385 .. 576
// units): every width keeps exactly one path
RCMARL_EXPORT int rcmarl_minibatch_fit_wide2_supported(int in_dim, int hid, int batch_size) {
  if (in_dim <= 0 || hid <= 0 || hid > MW2_MAX_HID || batch_size <= 0 || batch_size > MW2_ROWS) return 0;
  if (rcmarl_minibatch_fit_wide_supported(in_dim, hid, batch_size)) return 0;
  if (((hid + 31) >> 5) > MW2_TU * MW2_WAVES) return 0;
  return mw2_smem_bytes(hid) <= MW2_LDS_LIMIT ? 1 : 0;
}

RCMARL_EXPORT int rcmarl_minibatch_fit_wide2(const rcmarl_mb_job* jobs, const int* hid, int njobs, int S, int N, int B, int ldb,
                                             int batch_size, int epochs, float lr, void* stream) {
  if (!jobs || !hid || njobs <= 0 || njobs > MW2_MAX_JOBS || S <= 0 || N <= 0 || B <= 0 || batch_size <= 0 || epochs <= 0 || ldb < B)
    return RCMARL_ERR_ARG;
  for (int j = 0; j < njobs; ++j) {
    const rcmarl_mb_job& q = jobs[j];
    if (!q.x || !q.theta || !q.agents || !q.y || q.n_adv <= 0 || q.in_dim <= 0 || hid[j] <= 0 || q.ldp <= 0 || (q.ldp & 63))
      return RCMARL_ERR_ARG;
  }
  Mw2Args m{};
  m.njobs = njobs; m.N = N; m.B = B; m.ldb = ldb; m.bs = batch_size < B ? batch_size : B; m.epochs = epochs; m.lr = lr;
  int total = 0;
  size_t smem = 0;
  for (int j = 0; j < njobs; ++j) {
    const rcmarl_mb_job& q = jobs[j];
    if (!rcmarl_minibatch_fit_wide2_supported(q.in_dim, hid[j], batch_size)) return RCMARL_ERR_UNSUPPORTED;
    if (((long)q.in_dim + hid[j] + 3) * hid[j] + 1 > (long)q.ldp) return RCMARL_ERR_ARG;      // the net does not fit its row
    Mw2Job& a = m.job[j];
    a.x = q.x; a.x_seed_stride = q.x_seed_stride; a.theta = q.theta; a.agents = q.agents; a.y = q.y; a.perm = q.perm;
    a.loss_out = q.loss_out; a.n_adv = q.n_adv; a.in_dim = q.in_dim; a.ldp = q.ldp; a.hid = hid[j];
    m.first[j] = total;
    total += q.n_adv * S;
    const size_t b = mw2_smem_bytes(hid[j]);
    smem = b > smem ? b : smem;
  }
  for (int j = njobs; j <= MW2_MAX_JOBS; ++j) m.first[j] = total;
  if (!rc_want_lds(k_minibatch_wide2, smem, 48 * 1024)) return RCMARL_ERR_LAUNCH;
  RCMARL_LAUNCH(k_minibatch_wide2, dim3(total), dim3(MW2_THREADS), smem, stream, m);
  return rcmarl_check_launch();
}
