// Row passes over the feature-major activations of a wide net, shared by csrc/wide_kernels.hip and csrc/wide_head_ragged.hip:
// one wavefront per feature row j (contiguous over b), results to grads[s][n][...].
// grads record per (seed, agent): [gW3 (hid) | gb3 | gb2 (hid) | gb1 (hid)]
#pragma once
#include "rcmarl_common.h"

namespace {

__host__ __device__ static inline int w_grad_size(int hid) { return 3 * hid + 1; }

static inline bool w_dims_ok(int S, int N, int B, int K, int J, int ldp, int ldb) {
  return S > 0 && N > 0 && B > 0 && K > 0 && J > 0 && ldp > 0 && ldb >= B;
}

enum { WROW_FIT = 0, WROW_SUM = 1, WROW_DOT = 2 };

// FIT: gW3[j] = sum_b a2[j][b] dz3[b];  dz2[j][b] = W3[j] dz3[b] lrelu'(a2[j][b]) (in place);  gb2[j] = sum_b dz2;
//      row j == hid: gb3 = sum_b dz3[b]
// SUM: out[off + j] = sum_b act[j][b]
// DOT: out[j] = sum_b act[j][b] vec[b];  row j == hid: out[hid] = sum_b vec[b]
// agents (optional): blockIdx.y walks this list of agents instead of 0 .. N-1 (irregular graphs: the agents of the call's classes)
template <int MODE>
__global__ __launch_bounds__(256) void k_wrows(float* __restrict__ act, const float* __restrict__ vec,
                                               const float* __restrict__ theta, const int* __restrict__ coop,
                                               float* __restrict__ grads, int out_off, int N, int B, int in_dim, int hid,
                                               int ldp, int ldb, const int* __restrict__ agents) {
  const int s = blockIdx.z, i = agents ? agents[blockIdx.y] : (int)blockIdx.y, j = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  const int nrows = (MODE == WROW_SUM) ? hid : hid + 1;
  if (j >= nrows) return;
  if (coop && !coop[i]) return;
  float* __restrict__ gr = grads + ((long)s * N + i) * w_grad_size(hid);
  const float* __restrict__ v = vec ? vec + ((long)s * N + i) * ldb : nullptr;
  if (j == hid) {                                   // the bias of the head: plain sum of vec
    float acc = 0.f;
    for (int b = l; b < B; b += 64) acc += v[b];
    acc = rc_wave_sum(acc);
    if (l == 0) gr[hid] = acc;
    return;
  }
  float* __restrict__ row = act + (((long)s * N + i) * hid + j) * ldb;
  if (MODE == WROW_FIT) {
    const float w3 = theta[((long)s * N + i) * ldp + make_geom(in_dim, hid, 1).o_W3 + j];
    float gw = 0.f, gb = 0.f;
    for (int b = l; b < B; b += 64) {
      const float a2 = row[b], dv = v[b];
      gw = fmaf(a2, dv, gw);
      const float dz = dv * w3 * rc_lrelu_grad_from_act(a2);
      row[b] = dz;
      gb += dz;
    }
    gw = rc_wave_sum(gw);
    gb = rc_wave_sum(gb);
    if (l == 0) { gr[j] = gw; gr[hid + 1 + j] = gb; }
  } else if (MODE == WROW_SUM) {
    float acc = 0.f;
    for (int b = l; b < B; b += 64) acc += row[b];
    acc = rc_wave_sum(acc);
    if (l == 0) gr[out_off + j] = acc;
  } else {
    float acc = 0.f;
    for (int b = l; b < B; b += 64) acc = fmaf(row[b], v[b], acc);
    acc = rc_wave_sum(acc);
    if (l == 0) gr[j] = acc;
  }
}

}  // namespace
