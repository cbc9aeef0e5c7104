// X1 for wide networks -- the adversaries' mini-batch fits of a critic-family net of ANY hidden width, one whole Keras
// `fit(batch_size=32, epochs=10)` per workgroup and all (job, seed, adversary) chains of a consensus epoch in ONE launch.
//
// csrc/minibatch_fit.hip serves the 20-unit nets (one wavefront per network, parameters in LDS).  A wider net took the same
// mini-batch steps through the dense per-agent GEMM entry points: eight launches per step, 940 sequentially dependent steps per
// chain at B = 3000, three chains per Malicious agent and consensus epoch, serialised over seeds and adversaries by a Python
// loop.  Here ONE workgroup (four wavefronts) owns one chain for the whole fit:
//   * a mini-batch of 32 rows is exactly one 32-row tile of v_mfma_f32_32x32x2_f32 (the exact-f32 matrix instruction: an fmaf
//     chain in k order -- no operand range, no overflow flag, no fix-up launch); the 32-unit tiles of a layer are distributed
//     over the wavefronts (tile t belongs to wavefront t % 4);
//   * the activations of the mini-batch stay in LDS: a1, a2 (overwritten by dz2) and dz1, each [32][LD] fp32 with LD = hid
//     rounded up to 32, plus one (odd stride: a column walk and a row walk are both conflict-free);
//   * the parameters stay in the theta row in global memory (L2-resident) and are updated IN PLACE; a workgroup barrier
//     separates the stores of one phase from the loads of the next, and every gradient of a step comes from the pre-step weights;
//   * W2 is read once per step in the backward pass: the 32 x 32 tile a wavefront loads (one row i per lane, the registers
//     walking j in the accumulator's row order) is the A operand of da1^T += W2 dz2^T and is updated from gW2^T = dz2^T a1, which
//     the matrix core returns in that very layout.
// Rows >= nb of a short last mini-batch carry dLoss/dv = 0, so they add nothing to any gradient; unit columns >= hid of the last
// tile are kept at zero.  Semantics: oracle/mlp_np.fit_mse (Keras SGD on the MSE loss, SUM_OVER_BATCH_SIZE).
#include "rcmarl_common.h"

namespace {

constexpr int MW_ROWS = 32;              // rows of a mini-batch tile = the largest batch_size served
constexpr int MW_KC = 64;                // input columns staged per chunk
constexpr int MW_XLD = MW_KC + 1;        // LDS row stride of the staged chunk
constexpr int MW_THREADS = 256, MW_WAVES = 4, MW_MAX_JOBS = 4;
constexpr int MW_MAX_HID = 1 << 16;      // (beyond any LDS; keeps the size arithmetic inside int)
constexpr size_t MW_LDS_LIMIT = 160 * 1024;

struct MwJob {
  const float* x; long x_seed_stride; float* theta; const int* agents; const float* y; const int* perm; float* loss_out;
  int n_adv, in_dim, ldp, hid;
};
struct MwArgs {
  MwJob job[MW_MAX_JOBS];
  int first[MW_MAX_JOBS + 1];            // block b belongs to job j with first[j] <= b < first[j + 1]
  int njobs, N, B, ldb, bs, epochs;
  float lr;
};

__host__ __device__ inline int mw_ld(int hid) { return ((hid + 31) & ~31) + 1; }
// a1 | a2 (dz2) | dz1: [32][LD]; staged inputs [32][MW_XLD]; dv[32] | loss[32] | row indices[32]
size_t mw_smem_bytes(int hid) { return sizeof(float) * ((size_t)3 * MW_ROWS * mw_ld(hid) + MW_ROWS * MW_XLD + 2 * MW_ROWS) + sizeof(int) * MW_ROWS; }

// accumulator slot q of a lane in half h holds row mw_drow(q, h) of the 32 x 32 product (column = lane & 31)
__device__ __forceinline__ int mw_drow(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

__global__ __launch_bounds__(MW_THREADS) void k_minibatch_wide(MwArgs m) {
  RCMARL_DYN_SMEM(float, smem);
  int jn = 0;
#pragma unroll
  for (int q = 1; q < MW_MAX_JOBS; ++q) jn += (q < m.njobs && (int)blockIdx.x >= m.first[q]) ? 1 : 0;
  const MwJob a = m.job[jn];
  const int net = (int)blockIdx.x - m.first[jn];
  const int s = net / a.n_adv, adv = net - s * a.n_adv;
  const int hid = a.hid, in = a.in_dim, LD = mw_ld(hid), ntiles = (hid + 31) >> 5, TU = (ntiles + MW_WAVES - 1) / MW_WAVES;
  const NetGeom g = make_geom(in, hid, 1);
  float* a1s = smem;                       // [32][LD]
  float* a2s = a1s + MW_ROWS * LD;         // [32][LD]  a2, then dz2 in place
  float* dz1s = a2s + MW_ROWS * LD;        // [32][LD]
  float* xs = dz1s + MW_ROWS * LD;         // [32][MW_XLD] staged input chunk
  float* dvs = xs + MW_ROWS * MW_XLD;      // [32] dLoss/dv per row
  float* lossr = dvs + MW_ROWS;            // [32]
  int* idxs = reinterpret_cast<int*>(lossr + MW_ROWS);      // [32] replay rows of the mini-batch
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int agent = a.agents[adv];
  const long row = (long)s * m.N + agent;
  float* th = a.theta + row * a.ldp;
  const float* xg = a.x + (long)s * a.x_seed_stride;
  const float* yv = a.y + row * m.ldb;
  const int* perm = a.perm ? a.perm + ((long)s * a.n_adv + adv) * m.epochs * m.B : nullptr;
  const float lr = m.lr;
  const bool multi = in > MW_KC;           // more input columns than one staged chunk: re-staged wherever they are needed
  float loss_part = 0.f;                   // threads (t & 7) == 0: sum over the epoch-0 batches of row t >> 3's squared error

  auto stage = [&](int k0) {
    for (int e = t; e < MW_ROWS * MW_KC; e += MW_THREADS) {
      const int rr = e >> 6, kk = e & (MW_KC - 1), k = k0 + kk;
      xs[rr * MW_XLD + kk] = k < in ? xg[(long)idxs[rr] * in + k] : 0.f;
    }
  };

  for (int ep = 0; ep < m.epochs; ++ep) {
    for (int lo = 0; lo < m.B; lo += m.bs) {
      const int nb = min(m.bs, m.B - lo);
      if (t < MW_ROWS) {
        const int p = lo + (t < nb ? t : 0);
        idxs[t] = perm ? perm[(long)ep * m.B + p] : p;
      }
      __syncthreads();
      if (!multi) {
        stage(0);
        __syncthreads();
      }
      // ---- layer 1: a1[r][j] = lrelu(sum_k x[r][k] W1[k][j] + b1[j]), k ascending
      for (int u = 0; u < TU; ++u) {
        const int jt = wave + MW_WAVES * u, jc = jt * 32 + l31;
        const bool active = jt < ntiles, jok = active && jc < hid;
        rc_f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int k0 = 0; k0 < in; k0 += MW_KC) {
          if (multi) {
            __syncthreads();
            stage(k0);
            __syncthreads();
          }
          if (active) {
            const int kc = min(MW_KC, in - k0);
            for (int mm = 0; 2 * mm < kc; ++mm) {
              const int k = k0 + 2 * mm + h;
              const float av = xs[l31 * MW_XLD + 2 * mm + h];
              const float bv = (jok && k < in) ? th[(long)k * hid + jc] : 0.f;
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
          }
        }
        if (active) {
          const float bias = jok ? th[g.o_b1 + jc] : 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) a1s[mw_drow(q, h) * LD + jc] = rc_lrelu(acc[q] + bias);
        }
      }
      __syncthreads();
      // ---- layer 2: a2[r][j] = lrelu(sum_i a1[r][i] W2[i][j] + b2[j])
      for (int u = 0; u < TU; ++u) {
        const int jt = wave + MW_WAVES * u, jc = jt * 32 + l31;
        const bool active = jt < ntiles, jok = active && jc < hid;
        if (active) {
          rc_f32x16 acc;
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[q] = 0.f;
          for (int mm = 0; 2 * mm < hid; ++mm) {
            const int i = 2 * mm + h;
            const float av = a1s[l31 * LD + i];
            const float bv = (jok && i < hid) ? th[g.o_W2 + (long)i * hid + jc] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
          }
          const float bias = jok ? th[g.o_b2 + jc] : 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) a2s[mw_drow(q, h) * LD + jc] = rc_lrelu(acc[q] + bias);
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
      for (int k = t; k < hid; k += MW_THREADS) {
        const float w3 = th[g.o_W3 + k];
        float g3 = 0.f, gb2 = 0.f;
        for (int r = 0; r < MW_ROWS; ++r) {
          const float av = a2s[r * LD + k], d = dvs[r];
          g3 = fmaf(av, d, g3);
          const float dz = (d * w3) * rc_lrelu_grad_from_act(av);
          a2s[r * LD + k] = dz;
          gb2 += dz;
        }
        th[g.o_W3 + k] = w3 - lr * g3;
        th[g.o_b2 + k] = th[g.o_b2 + k] - lr * gb2;
      }
      if (t == MW_THREADS - 1) {
        float gb3 = 0.f;
        for (int r = 0; r < MW_ROWS; ++r) gb3 += dvs[r];
        th[g.o_b3] = th[g.o_b3] - lr * gb3;
      }
      __syncthreads();
      // ---- backward through layer 2.  The wavefront that owns unit tile `it` walks the tiles W2[it][jt]: the loaded tile gives
      // da1^T[i][r] += sum_j W2[i][j] dz2[r][j] (A operand, contraction slot (mm, half) = column mw_drow(mm, half)) and takes
      // W2[i][j] -= lr * sum_r a1[r][i] dz2[r][j] (the product dz2^T a1 lands in the tile's own register layout).
      for (int u = 0; u < TU; ++u) {
        const int it = wave + MW_WAVES * u;
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
            for (int q = 0; q < 16; ++q) w[q] = (iok && jt * 32 + mw_drow(q, h) < hid) ? wt[mw_drow(q, h)] : 0.f;
            rc_f32x16 gw;
#pragma unroll
            for (int q = 0; q < 16; ++q) gw[q] = 0.f;
#pragma unroll
            for (int mm = 0; mm < 16; ++mm)
              gw = __builtin_amdgcn_mfma_f32_32x32x2f32(a2s[(2 * mm + h) * LD + jt * 32 + l31], a1f[mm], gw, 0, 0, 0);
#pragma unroll
            for (int mm = 0; mm < 16; ++mm)
              da = __builtin_amdgcn_mfma_f32_32x32x2f32(w[mm], a2s[l31 * LD + jt * 32 + mw_drow(mm, h)], da, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 16; ++q)
              if (iok && jt * 32 + mw_drow(q, h) < hid) wt[mw_drow(q, h)] = w[q] - lr * gw[q];
          }
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int o = l31 * LD + it * 32 + mw_drow(q, h);
            dz1s[o] = da[q] * rc_lrelu_grad_from_act(a1s[o]);
          }
        }
      }
      __syncthreads();
      // ---- gb1, and W1[k][j] -= lr * sum_r x[r][k] dz1[r][j]
      for (int k = t; k < hid; k += MW_THREADS) {
        float gb1 = 0.f;
        for (int r = 0; r < MW_ROWS; ++r) gb1 += dz1s[r * LD + k];
        th[g.o_b1 + k] = th[g.o_b1 + k] - lr * gb1;
      }
      for (int k0 = 0; k0 < in; k0 += MW_KC) {
        if (multi) {
          __syncthreads();
          stage(k0);
          __syncthreads();
        }
        const int kc = min(MW_KC, in - k0);
        for (int u = 0; u < TU; ++u) {
          const int jt = wave + MW_WAVES * u, jc = jt * 32 + l31;
          if (jt < ntiles) {
            const bool jok = jc < hid;
            float dzf[16];
#pragma unroll
            for (int mm = 0; mm < 16; ++mm) dzf[mm] = dz1s[(2 * mm + h) * LD + jc];
            for (int sub = 0; sub * 32 < kc; ++sub) {
              rc_f32x16 gw;
#pragma unroll
              for (int q = 0; q < 16; ++q) gw[q] = 0.f;
#pragma unroll
              for (int mm = 0; mm < 16; ++mm)
                gw = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(2 * mm + h) * MW_XLD + sub * 32 + l31], dzf[mm], gw, 0, 0, 0);
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int k = k0 + sub * 32 + mw_drow(q, h);
                if (jok && k < in) th[(long)k * hid + jc] = th[(long)k * hid + jc] - lr * gw[q];
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
        for (int q = 0; q < MW_ROWS; ++q) sum += lossr[q];
        a.loss_out[row] = sum / (float)m.B;
      }
      __syncthreads();
    }
  }
}

}  // namespace

RCMARL_EXPORT int rcmarl_minibatch_fit_wide_supported(int in_dim, int hid, int batch_size) {
  if (in_dim <= 0 || hid <= 0 || hid > MW_MAX_HID || batch_size <= 0 || batch_size > MW_ROWS) return 0;
  return mw_smem_bytes(hid) <= MW_LDS_LIMIT ? 1 : 0;
}

RCMARL_EXPORT int rcmarl_minibatch_fit_wide(const rcmarl_mb_job* jobs, const int* hid, int njobs, int S, int N, int B, int ldb,
                                            int batch_size, int epochs, float lr, void* stream) {
  if (!jobs || !hid || njobs <= 0 || njobs > MW_MAX_JOBS || S <= 0 || N <= 0 || B <= 0 || batch_size <= 0 || epochs <= 0 || ldb < B)
    return RCMARL_ERR_ARG;
  for (int j = 0; j < njobs; ++j) {
    const rcmarl_mb_job& q = jobs[j];
    if (!q.x || !q.theta || !q.agents || !q.y || q.n_adv <= 0 || q.in_dim <= 0 || hid[j] <= 0 || q.ldp <= 0 || (q.ldp & 63))
      return RCMARL_ERR_ARG;
  }
  MwArgs m{};
  m.njobs = njobs; m.N = N; m.B = B; m.ldb = ldb; m.bs = batch_size < B ? batch_size : B; m.epochs = epochs; m.lr = lr;
  int total = 0;
  size_t smem = 0;
  for (int j = 0; j < njobs; ++j) {
    const rcmarl_mb_job& q = jobs[j];
    if (!rcmarl_minibatch_fit_wide_supported(q.in_dim, hid[j], batch_size)) return RCMARL_ERR_UNSUPPORTED;
    if (((long)q.in_dim + hid[j] + 3) * hid[j] + 1 > (long)q.ldp) return RCMARL_ERR_ARG;      // the net does not fit its row
    MwJob& a = m.job[j];
    a.x = q.x; a.x_seed_stride = q.x_seed_stride; a.theta = q.theta; a.agents = q.agents; a.y = q.y; a.perm = q.perm;
    a.loss_out = q.loss_out; a.n_adv = q.n_adv; a.in_dim = q.in_dim; a.ldp = q.ldp; a.hid = hid[j];
    m.first[j] = total;
    total += q.n_adv * S;
    const size_t b = mw_smem_bytes(hid[j]);
    smem = b > smem ? b : smem;
  }
  for (int j = njobs; j <= MW_MAX_JOBS; ++j) m.first[j] = total;
  if (!rc_want_lds(k_minibatch_wide, smem, 48 * 1024)) return RCMARL_ERR_LAUNCH;
  RCMARL_LAUNCH(k_minibatch_wide, dim3(total), dim3(MW_THREADS), smem, stream, m);
  return rcmarl_check_launch();
}
