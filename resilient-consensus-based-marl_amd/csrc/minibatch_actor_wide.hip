// X1 for wide actors -- the adversaries' `actor.fit(batch_size=200, epochs=1)` (Adam on the sample-weighted sparse cross-entropy,
// agents/adversarial_CAC_agents.py:38-41,111-117,221-225) for an actor of ANY hidden width, one whole fit per workgroup and all
// (seed, adversary) chains in ONE launch.
//
// csrc/minibatch_fit.hip (k_minibatch_train<20, 5, true>) serves the 20-unit actor with its parameters in LDS.  This file follows its
// wide siblings csrc/minibatch_wide.hip / minibatch_wide2.hip: ONE workgroup (four wavefronts) owns one chain for the whole fit,
// the arithmetic is fp32 on v_mfma_f32_32x32x2_f32 (an fmaf chain in k order: no operand range, no overflow flag, no fix-up
// launch), the 32-unit tiles of a layer are dealt over the wavefronts (tile t belongs to wavefront t % 4), and the parameters and
// Adam slots stay in their theta / adam_m / adam_v rows in global memory (L2-resident), updated in place.
//
// What is new against the siblings: a mini-batch is up to 200 rows, not 32, so its activations do not fit the LDS.  The weights are
// constant inside a step, so the step walks the mini-batch in 32-row tiles.  Per row tile: forward through both hidden layers with
// a1, a2 in LDS ([32][LD] fp32, LD = hid rounded up to 32, plus one); the head (n_actions logits, softmax, dz3 = delta (p -
// onehot(a)) / nb in Keras's sample-weight reduction, as rcmarl_wide_actor_head computes it) and the loss; dz2 (over a2) and dz1 from
// the pre-step weights; and the tile's contribution to every weight and bias gradient is ADDED into the chain's row of `grad`
// (caller-owned scratch, zeroed by the kernel at the start of each step; every gradient element has ONE owner thread for the whole
// step, so the additions need no atomics and their order is fixed).  After the last row tile one pass over the P parameters applies
// Adam from `grad` (TF2 ResourceApplyAdam, rc_adam_apply; the step size of Adam step t0 + k formed in double and rounded to fp32 as
// k_minibatch_train does); a workgroup barrier separates that pass from the next step's loads.
// Rows >= nb of a short tile carry dz3 = 0, so they add nothing to any gradient; unit columns >= hid of the last tile stay zero;
// inputs wider than one staged chunk are re-staged wherever they are needed.  Semantics: oracle/mlp_np.fit_actor_ce.
//
// Two entry points share the kernel body through a compile-time flag.  rcmarl_minibatch_actor_wide keeps THREE [32][LD] images (a1,
// a2 / dz2, dz1): widths up to 384.  rcmarl_minibatch_actor_wide2 keeps TWO, dz1 written over a1, as csrc/minibatch_wide2.hip does for
// the critic family: widths 385 .. 576 (2 * 32 * 577 floats + the staged chunk + dz3 + indices + loss = 157 440 bytes of the 160 KiB).
// dz1 may take a1's place because in the backward pass through layer 2 the wavefront that owns unit tile `it` is the only reader of
// a1's columns of that tile: once as a1f (into registers, before the jt loop) and once for lrelu' at the very address the same lane
// then writes dz1 to; nothing after that phase reads a1 (gb1 and gW1 read dz1 and the staged inputs), and layer 1 of the next row
// tile rewrites the whole image, the padding columns of the last unit tile included (they stay zero in between: their masked weights
// make da zero there).
#include "rcmarl_common.h"
#include <limits.h>

namespace {

constexpr int AW_ROWS = 32;              // rows of a tile of the mini-batch
constexpr int AW_KC = 64;                // input columns staged per chunk
constexpr int AW_XLD = AW_KC + 1;        // LDS row stride of the staged chunk
constexpr int AW_THREADS = 256, AW_WAVES = 4;
constexpr int AW_UNR = 8;                // contraction steps of a forward layer whose operands are loaded together (2 * AW_UNR divides AW_KC)
constexpr int AW_MAX_A = 8;             // most actions served (one dz3 row of a tile = 8 floats)
constexpr int AW_MAX_HID = 1 << 16;      // (beyond any LDS; keeps the size arithmetic inside int)
constexpr size_t AW_LDS_LIMIT = 160 * 1024;

struct AwArgs {
  const float* x; long x_seed_stride; float* theta; float* adam_m; float* adam_v; float* grad; const int* agents;
  const float* act; const float* w; const int* perm; float* loss_out;
  int n_adv, N, B, in_dim, hid, A, ldp, ldb, bs, epochs, t0;
  float one_m_b1, one_m_b2, eps;
  double lr, beta1, beta2;
};

__host__ __device__ inline int aw_ld(int hid) { return ((hid + 31) & ~31) + 1; }
// a1 | a2 (dz2) | dz1: [32][LD] (`images` = 3), or a1 (dz1) | a2 (dz2) (`images` = 2); staged inputs [32][AW_XLD]; dz3 [32][8];
// row indices[32]; loss[32] (double)
size_t aw_smem_bytes(int hid, int images) {
  return sizeof(float) * ((size_t)images * AW_ROWS * aw_ld(hid) + AW_ROWS * AW_XLD + AW_ROWS * AW_MAX_A) + sizeof(int) * AW_ROWS +
         sizeof(double) * AW_ROWS;
}

// v where `keep` (all ones) allows it, +0 where it is zero.  The mask comes through rc_opaque_v, so the compiler sees no condition it
// could turn into a branch around the load of v: the loads of a batch stay back to back and their latencies overlap.
__device__ __forceinline__ unsigned aw_mask(bool keep) { return (unsigned)rc_opaque_v(keep ? -1 : 0); }
__device__ __forceinline__ float aw_keep(float v, unsigned keep) { return __uint_as_float(__float_as_uint(v) & keep); }

// accumulator slot q of a lane in half h holds row aw_drow(q, h) of the 32 x 32 product (column = lane & 31)
__device__ __forceinline__ int aw_drow(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// TWO: the two-image layout (dz1 over a1)
template <bool TWO>
__global__ __launch_bounds__(AW_THREADS) void k_minibatch_actor_wide(AwArgs m) {
  RCMARL_DYN_SMEM(float, smem);
  const int net = (int)blockIdx.x;
  const int s = net / m.n_adv, adv = net - s * m.n_adv;
  const int hid = m.hid, in = m.in_dim, A = m.A, LD = aw_ld(hid), ntiles = (hid + 31) >> 5, TU = (ntiles + AW_WAVES - 1) / AW_WAVES;
  const NetGeom g = make_geom(in, hid, A);
  float* a1s = smem;                       // [32][LD]
  float* a2s = a1s + AW_ROWS * LD;         // [32][LD]  a2, then dz2 in place
  float* dz1s = TWO ? a1s : a2s + AW_ROWS * LD;      // [32][LD]  (TWO: a1's image, each element written by the lane that read it last)
  float* xs = (TWO ? a2s : dz1s) + AW_ROWS * LD;     // [32][AW_XLD] staged input chunk
  float* dz3s = xs + AW_ROWS * AW_XLD;     // [32][8] dLoss/dlogits per row (columns >= A: zero)
  int* idxs = reinterpret_cast<int*>(dz3s + AW_ROWS * AW_MAX_A);      // [32] replay rows of the tile
  double* lossr = reinterpret_cast<double*>(idxs + AW_ROWS);           // [32] (8-byte aligned: an even number of 4-byte words precedes it)
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int agent = m.agents[adv];
  const long row = (long)s * m.N + agent;
  float* th = m.theta + row * m.ldp;
  float* mrow = m.adam_m + row * m.ldp;
  float* vrow = m.adam_v + row * m.ldp;
  float* gr = m.grad + (long)net * m.ldp;
  const float* xg = m.x + (long)s * m.x_seed_stride;
  const float* yv = m.act + row * m.ldb;
  const float* wv = m.w + row * m.ldb;
  const int* perm = m.perm ? m.perm + ((long)s * m.n_adv + adv) * m.epochs * m.B : nullptr;
  const bool multi = in > AW_KC;           // more input columns than one staged chunk: re-staged wherever they are needed
  double loss_part = 0.0;                  // threads (t & 7) == 0: sum over the epoch-0 rows (t >> 3 of every tile) of the weighted loss
                                           // (the weights carry both signs, so the sum cancels: kept in double, rounded once at the end)
  int step = m.t0;                         // optimiser steps taken so far (Adam bias correction)

  auto stage = [&](int k0) {
#pragma unroll
    for (int e = t; e < AW_ROWS * AW_KC; e += AW_THREADS) {
      const int rr = e >> 6, kk = e & (AW_KC - 1), k = k0 + kk;
      const float xv = xg[(long)idxs[rr] * in + min(k, in - 1)];
      xs[rr * AW_XLD + kk] = k < in ? xv : 0.f;
    }
  };

  for (int ep = 0; ep < m.epochs; ++ep) {
    for (int lo = 0; lo < m.B; lo += m.bs) {
      const int nb = min(m.bs, m.B - lo);
      for (int e = t; e < g.P; e += AW_THREADS) gr[e] = 0.f;         // (ordered before the first addition by the barriers below)
      for (int t0r = 0; t0r < nb; t0r += AW_ROWS) {
        const int nrt = min(AW_ROWS, nb - t0r);
        if (t < AW_ROWS) {
          const int p = lo + t0r + (t < nrt ? t : 0);
          idxs[t] = perm ? perm[(long)ep * m.B + p] : p;
        }
        __syncthreads();
        if (!multi) {
          stage(0);
          __syncthreads();
        }
        // ---- layer 1: a1[r][j] = lrelu(sum_k x[r][k] W1[k][j] + b1[j]), k ascending
        for (int u = 0; u < TU; ++u) {
          const int jt = wave + AW_WAVES * u, jc = jt * 32 + l31;
          const bool active = jt < ntiles, jok = active && jc < hid;
          rc_f32x16 acc;
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[q] = 0.f;
          for (int k0 = 0; k0 < in; k0 += AW_KC) {
            if (multi) {
              __syncthreads();
              stage(k0);
              __syncthreads();
            }
            if (active) {
              // the weights of AW_UNR contraction steps are loaded together, from clamped (always valid) addresses, and zeroed
              // afterwards where they lie outside the net: no branch sits between a load and the next, so their latencies overlap
              // (a predicated load per step made every step wait for its own)
              const int kc = min(AW_KC, in - k0), jcl = min(jc, hid - 1);
              const unsigned keepj = aw_mask(jok);
              for (int m0 = 0; 2 * m0 < kc; m0 += AW_UNR) {
                float av[AW_UNR], bv[AW_UNR];
#pragma unroll
                for (int v8 = 0; v8 < AW_UNR; ++v8) {
                  const int kk = 2 * (m0 + v8) + h, k = k0 + kk;         // kk < AW_KC; the staged chunk is zero beyond the inputs
                  av[v8] = xs[l31 * AW_XLD + kk];
                  const float wl = th[(long)min(k, in - 1) * hid + jcl];
                  bv[v8] = aw_keep(k < in ? wl : 0.f, keepj);
                }
#pragma unroll
                for (int v8 = 0; v8 < AW_UNR; ++v8) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v8], bv[v8], acc, 0, 0, 0);
              }
            }
          }
          if (active) {
            const float bias = jok ? th[g.o_b1 + jc] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) a1s[aw_drow(q, h) * LD + jc] = rc_lrelu(acc[q] + bias);
          }
        }
        __syncthreads();
        // ---- layer 2: a2[r][j] = lrelu(sum_i a1[r][i] W2[i][j] + b2[j])
        for (int u = 0; u < TU; ++u) {
          const int jt = wave + AW_WAVES * u, jc = jt * 32 + l31;
          const bool active = jt < ntiles, jok = active && jc < hid;
          if (active) {
            rc_f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
            const int jcl = min(jc, hid - 1);
            const unsigned keepj = aw_mask(jok);
            for (int i0 = 0; i0 < hid; i0 += 2 * AW_UNR) {
              float av[AW_UNR], bv[AW_UNR];
#pragma unroll
              for (int v8 = 0; v8 < AW_UNR; ++v8) {
                const int i = i0 + 2 * v8 + h;                           // < hid rounded up to 16 < LD; a1 is zero from hid on
                av[v8] = a1s[l31 * LD + i];
                const float wl = th[g.o_W2 + (long)min(i, hid - 1) * hid + jcl];
                bv[v8] = aw_keep(i < hid ? wl : 0.f, keepj);
              }
#pragma unroll
              for (int v8 = 0; v8 < AW_UNR; ++v8) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v8], bv[v8], acc, 0, 0, 0);
            }
            const float bias = jok ? th[g.o_b2 + jc] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) a2s[aw_drow(q, h) * LD + jc] = rc_lrelu(acc[q] + bias);
          }
        }
        __syncthreads();
        // ---- head: logits, softmax, dz3 and the loss -- eight threads per row
        {
          const int r = t >> 3, p = t & 7;
          float logit[AW_MAX_A];
#pragma unroll
          for (int a = 0; a < AW_MAX_A; ++a) logit[a] = 0.f;
#pragma unroll 2
          for (int k = p; k < hid; k += 8) {
            const float av = a2s[r * LD + k];
            const float* w3 = th + g.o_W3 + (long)k * A;
#pragma unroll
            for (int a = 0; a < AW_MAX_A; ++a) logit[a] = fmaf(av, w3[min(a, A - 1)], logit[a]);      // (slots >= A: never read)
          }
#pragma unroll
          for (int a = 0; a < AW_MAX_A; ++a) {
            float v = logit[a];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            logit[a] = v;
          }
          if (p == 0) {
            const bool valid = r < nrt;
            float mx = -3.0e38f;
#pragma unroll
            for (int a = 0; a < AW_MAX_A; ++a)
              if (a < A) {
                logit[a] += th[g.o_b3 + a];
                mx = fmaxf(mx, logit[a]);
              }
            float se = 0.f;
#pragma unroll
            for (int a = 0; a < AW_MAX_A; ++a)
              if (a < A) se += expf(logit[a] - mx);
            const float lse = logf(se);
            const int b = idxs[r];
            const int label = valid ? (int)yv[b] : 0;
            const float wgt = valid ? wv[b] : 0.f;
            const float wB = wgt / (float)nb;                        // Keras sample weights, SUM_OVER_BATCH_SIZE
#pragma unroll
            for (int a = 0; a < AW_MAX_A; ++a) {
              float d = 0.f;
              if (a < A) {
                const float logp = (logit[a] - mx) - lse;
                if (a == label && ep == 0) loss_part += (double)((-logp) * wgt);
                d = (expf(logp) - (a == label ? 1.f : 0.f)) * wB;
              }
              dz3s[r * AW_MAX_A + a] = d;
            }
          }
        }
        __syncthreads();
        // ---- gW3, gb2 and dz2 = (dz3 W3^T) * lrelu'(z2) over a2 (one thread per unit; gW3 is taken before a2 is overwritten); gb3
        for (int k = t; k < hid; k += AW_THREADS) {
          float w3[AW_MAX_A], g3[AW_MAX_A];
#pragma unroll
          for (int a = 0; a < AW_MAX_A; ++a) {
            const float wl = th[g.o_W3 + (long)k * A + min(a, A - 1)];
            w3[a] = a < A ? wl : 0.f;
            g3[a] = 0.f;
          }
          float gb2 = 0.f;
          for (int r = 0; r < AW_ROWS; ++r) {
            const float av = a2s[r * LD + k];
            float da = 0.f;
#pragma unroll
            for (int a = 0; a < AW_MAX_A; ++a) {
              const float d = dz3s[r * AW_MAX_A + a];
              g3[a] = fmaf(av, d, g3[a]);
              da = fmaf(d, w3[a], da);
            }
            const float dz = da * rc_lrelu_grad_from_act(av);
            a2s[r * LD + k] = dz;
            gb2 += dz;
          }
          float g0[AW_MAX_A];
#pragma unroll
          for (int a = 0; a < AW_MAX_A; ++a) g0[a] = gr[g.o_W3 + (long)k * A + min(a, A - 1)];
#pragma unroll
          for (int a = 0; a < AW_MAX_A; ++a)
            if (a < A) gr[g.o_W3 + (long)k * A + a] = g0[a] + g3[a];
          gr[g.o_b2 + k] += gb2;
        }
        if (t >= AW_THREADS - AW_MAX_A && t - (AW_THREADS - AW_MAX_A) < A) {
          const int a = t - (AW_THREADS - AW_MAX_A);
          float gb3 = 0.f;
          for (int r = 0; r < AW_ROWS; ++r) gb3 += dz3s[r * AW_MAX_A + a];
          gr[g.o_b3 + a] += gb3;
        }
        __syncthreads();
        // ---- backward through layer 2.  The wavefront that owns unit tile `it` walks the tiles W2[it][jt]: the loaded tile gives
        // da1^T[i][r] += sum_j W2[i][j] dz2[r][j] (A operand, contraction slot (mm, half) = column aw_drow(mm, half)); the tile's
        // gradient gW2 = a1^T dz2 is formed with j along the lanes and added to the gradient row.
        for (int u = 0; u < TU; ++u) {
          const int it = wave + AW_WAVES * u;
          if (it < ntiles) {
            const int ic = it * 32 + l31;
            const bool iok = ic < hid;
            const unsigned keepi = aw_mask(iok);
            float a1f[16];
#pragma unroll
            for (int mm = 0; mm < 16; ++mm) a1f[mm] = a1s[(2 * mm + h) * LD + ic];
            rc_f32x16 da;
#pragma unroll
            for (int q = 0; q < 16; ++q) da[q] = 0.f;
            for (int jt = 0; jt < ntiles; ++jt) {
              // (all loads of the tile -- its weights, and the gradient sums it adds to -- from clamped addresses, ahead of the products)
              const long wo = g.o_W2 + (long)min(ic, hid - 1) * hid;
              const int jc = jt * 32 + l31, jcl = min(jc, hid - 1);
              float w[16], g0[16];
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int col = jt * 32 + aw_drow(q, h);
                const float wl = th[wo + min(col, hid - 1)];
                w[q] = aw_keep(col < hid ? wl : 0.f, keepi);
              }
#pragma unroll
              for (int q = 0; q < 16; ++q) g0[q] = gr[g.o_W2 + (long)min(it * 32 + aw_drow(q, h), hid - 1) * hid + jcl];
              rc_f32x16 gw;
#pragma unroll
              for (int q = 0; q < 16; ++q) gw[q] = 0.f;
#pragma unroll
              for (int mm = 0; mm < 16; ++mm)
                gw = __builtin_amdgcn_mfma_f32_32x32x2f32(a1f[mm], a2s[(2 * mm + h) * LD + jt * 32 + l31], gw, 0, 0, 0);
#pragma unroll
              for (int mm = 0; mm < 16; ++mm)
                da = __builtin_amdgcn_mfma_f32_32x32x2f32(w[mm], a2s[l31 * LD + jt * 32 + aw_drow(mm, h)], da, 0, 0, 0);
              // gW2[i][j] with j along the lanes: the additions are 128-byte row segments of the gradient row
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int ir = it * 32 + aw_drow(q, h);
                if (ir < hid && jc < hid) gr[g.o_W2 + (long)ir * hid + jc] = g0[q] + gw[q];
              }
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int o = l31 * LD + it * 32 + aw_drow(q, h);
              dz1s[o] = da[q] * rc_lrelu_grad_from_act(a1s[o]);
            }
          }
        }
        __syncthreads();
        // ---- gb1, and gW1[k][j] += sum_r x[r][k] dz1[r][j]
        for (int k = t; k < hid; k += AW_THREADS) {
          float gb1 = 0.f;
          for (int r = 0; r < AW_ROWS; ++r) gb1 += dz1s[r * LD + k];
          gr[g.o_b1 + k] += gb1;
        }
        for (int k0 = 0; k0 < in; k0 += AW_KC) {
          if (multi) {
            __syncthreads();
            stage(k0);
            __syncthreads();
          }
          const int kc = min(AW_KC, in - k0);
          for (int u = 0; u < TU; ++u) {
            const int jt = wave + AW_WAVES * u, jc = jt * 32 + l31;
            if (jt < ntiles) {
              const bool jok = jc < hid;
              float dzf[16];
#pragma unroll
              for (int mm = 0; mm < 16; ++mm) dzf[mm] = dz1s[(2 * mm + h) * LD + jc];
              const int jcl = min(jc, hid - 1);
              for (int sub = 0; sub * 32 < kc; ++sub) {
                float g0[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) g0[q] = gr[(long)min(k0 + sub * 32 + aw_drow(q, h), in - 1) * hid + jcl];
                rc_f32x16 gw;
#pragma unroll
                for (int q = 0; q < 16; ++q) gw[q] = 0.f;
#pragma unroll
                for (int mm = 0; mm < 16; ++mm)
                  gw = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(2 * mm + h) * AW_XLD + sub * 32 + l31], dzf[mm], gw, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                  const int k = k0 + sub * 32 + aw_drow(q, h);
                  if (jok && k < in) gr[(long)k * hid + jc] = g0[q] + gw[q];
                }
              }
            }
          }
        }
        __syncthreads();                   // the tile's LDS images are free; its gradient additions are done
      }
      // ---- Adam step from the summed gradient (TF2 ResourceApplyAdam; alpha from the step counter, formed in double)
      ++step;
      const float alpha = (float)(m.lr * sqrt(1.0 - pow(m.beta2, (double)step)) / (1.0 - pow(m.beta1, (double)step)));
      for (int e0 = t; e0 < g.P; e0 += 4 * AW_THREADS) {      // four elements per thread and round: sixteen loads, then the stores
        float gg[4], mm[4], vv[4], w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int e = min(e0 + c * AW_THREADS, g.P - 1);
          gg[c] = gr[e]; mm[c] = mrow[e]; vv[c] = vrow[e]; w[c] = th[e];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int e = e0 + c * AW_THREADS;
          rc_adam_apply(gg[c], w[c], mm[c], vv[c], alpha, m.one_m_b1, m.one_m_b2, m.eps);
          if (e < g.P) {
            mrow[e] = mm[c];
            vrow[e] = vv[c];
            th[e] = w[c];
          }
        }
      }
      __syncthreads();                     // this step's stores before the next step's loads
    }
    if (ep == 0 && m.loss_out) {           // Keras History: first-epoch loss, the mean of the batch losses weighted by batch length
      if ((t & 7) == 0) lossr[t >> 3] = loss_part;
      __syncthreads();
      if (t == 0) {
        double sum = 0.0;
        for (int q = 0; q < AW_ROWS; ++q) sum += lossr[q];
        m.loss_out[row] = (float)(sum / (double)m.B);
      }
      __syncthreads();
    }
  }
}

}  // namespace

static bool aw_shape_ok(int in_dim, int hid, int n_actions, int batch_size) {
  if (in_dim <= 0 || hid <= 0 || hid > AW_MAX_HID || n_actions < 2 || n_actions > AW_MAX_A || batch_size <= 0) return false;
  return ((long)in_dim + hid + 2 + n_actions) * hid + n_actions <= (long)INT_MAX;      // parameter offsets are ints
}

RCMARL_EXPORT int rcmarl_minibatch_actor_wide_supported(int in_dim, int hid, int n_actions, int batch_size) {
  if (!aw_shape_ok(in_dim, hid, n_actions, batch_size)) return 0;
  return aw_smem_bytes(hid, 3) <= AW_LDS_LIMIT ? 1 : 0;
}

// the widths beyond the three-image layout that the two-image layout holds: never 1 together with the query above
RCMARL_EXPORT int rcmarl_minibatch_actor_wide2_supported(int in_dim, int hid, int n_actions, int batch_size) {
  if (!aw_shape_ok(in_dim, hid, n_actions, batch_size)) return 0;
  return aw_smem_bytes(hid, 3) > AW_LDS_LIMIT && aw_smem_bytes(hid, 2) <= AW_LDS_LIMIT ? 1 : 0;
}

template <bool TWO>
static int aw_run(const float* x, long x_seed_stride, float* theta, float* adam_m, float* adam_v, float* grad, const int* agents,
                  int n_adv, const float* act_t, const float* delta, const int* perm, int S, int N, int B, int in_dim, int hid,
                  int n_actions, int ldp, int ldb, int batch_size, int epochs, double lr, double beta1, double beta2, double eps, int t0,
                  float* loss_out, void* stream) {
  if (!x || !theta || !adam_m || !adam_v || !grad || !agents || !act_t || !delta || n_adv <= 0 || S <= 0 || N <= 0 || B <= 0 ||
      in_dim <= 0 || hid <= 0 || n_actions <= 0 || batch_size <= 0 || epochs <= 0 || t0 < 0 || ldp <= 0 || (ldp & 63) || ldb < B)
    return RCMARL_ERR_ARG;
  if (!(TWO ? rcmarl_minibatch_actor_wide2_supported : rcmarl_minibatch_actor_wide_supported)(in_dim, hid, n_actions, batch_size))
    return RCMARL_ERR_UNSUPPORTED;
  if (((long)in_dim + hid + 2 + n_actions) * hid + n_actions > (long)ldp) return RCMARL_ERR_ARG;      // the net does not fit its row
  if ((long)S * n_adv > (long)INT_MAX) return RCMARL_ERR_ARG;
  AwArgs m{};
  m.x = x; m.x_seed_stride = x_seed_stride; m.theta = theta; m.adam_m = adam_m; m.adam_v = adam_v; m.grad = grad; m.agents = agents;
  m.act = act_t; m.w = delta; m.perm = perm; m.loss_out = loss_out;
  m.n_adv = n_adv; m.N = N; m.B = B; m.in_dim = in_dim; m.hid = hid; m.A = n_actions; m.ldp = ldp; m.ldb = ldb;
  m.bs = batch_size < B ? batch_size : B; m.epochs = epochs; m.t0 = t0;
  m.lr = lr; m.beta1 = beta1; m.beta2 = beta2;      // alpha and (1 - beta) are formed in double, then rounded (Keras/TF2 order)
  m.one_m_b1 = (float)(1.0 - beta1); m.one_m_b2 = (float)(1.0 - beta2); m.eps = (float)eps;
  const size_t smem = aw_smem_bytes(hid, TWO ? 2 : 3);
  if (!rc_want_lds(k_minibatch_actor_wide<TWO>, smem, 48 * 1024)) return RCMARL_ERR_LAUNCH;
  RCMARL_LAUNCH(k_minibatch_actor_wide<TWO>, dim3(S * n_adv), dim3(AW_THREADS), smem, stream, m);
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_minibatch_actor_wide(const float* x, long x_seed_stride, float* theta, float* adam_m, float* adam_v,
                                              float* grad, const int* agents, int n_adv, const float* act_t, const float* delta,
                                              const int* perm, int S, int N, int B, int in_dim, int hid, int n_actions, int ldp,
                                              int ldb, int batch_size, int epochs, double lr, double beta1, double beta2, double eps,
                                              int t0, float* loss_out, void* stream) {
  return aw_run<false>(x, x_seed_stride, theta, adam_m, adam_v, grad, agents, n_adv, act_t, delta, perm, S, N, B, in_dim, hid, n_actions,
                       ldp, ldb, batch_size, epochs, lr, beta1, beta2, eps, t0, loss_out, stream);
}

RCMARL_EXPORT int rcmarl_minibatch_actor_wide2(const float* x, long x_seed_stride, float* theta, float* adam_m, float* adam_v,
                                               float* grad, const int* agents, int n_adv, const float* act_t, const float* delta,
                                               const int* perm, int S, int N, int B, int in_dim, int hid, int n_actions, int ldp,
                                               int ldb, int batch_size, int epochs, double lr, double beta1, double beta2, double eps,
                                               int t0, float* loss_out, void* stream) {
  return aw_run<true>(x, x_seed_stride, theta, adam_m, adam_v, grad, agents, n_adv, act_t, delta, perm, S, N, B, in_dim, hid, n_actions,
                      ldp, ldb, batch_size, epochs, lr, beta1, beta2, eps, t0, loss_out, stream);
}
