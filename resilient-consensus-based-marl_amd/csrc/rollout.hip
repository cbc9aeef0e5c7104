// K8 + the single-row forwards of the rollout.
//
// Replaces, per environment step, the reference's N Keras `predict` calls on a
// batch of one (RPBCAC_agent.get_action, agents/resilient_CAC_agents.py:208-219;
// the reference's dominant wall-time cost) and the per-agent Python loop of
// Grid_World.step (environments/grid_world.py:47-64), and per episode the
// critic evaluations at the start state (training/train_agents.py:60-62).
//
// One wavefront owns one (seed, agent): lanes stride over the input features of
// layer 1 (W1 rows are 80-B contiguous -> fully coalesced), a butterfly sums the
// 20 partial pre-activations, the tiny layers 2-3 run redundantly in every lane
// with wave-uniform (scalar) weights.  Lane 0 then samples the action (Philox
// stream, rcmarl_rng.h) and applies the grid-world transition, writing this
// agent's slice of the replay row.  One launch per environment step for ALL
// seeds and agents; no host round trip.
#include "rcmarl_common.h"
#include "rcmarl_lattice.h"
#include "rcmarl_rng.h"

namespace {

struct EnvCfg {
  int nrow, ncol;
  double mean_x, mean_y, std_x, std_y;   // get_data() scaling (environments/grid_world.py:29-33,70)
};

template <int HID>
__device__ __forceinline__ void wave_hidden(const float* __restrict__ th, const NetGeom& g,
                                            const float* __restrict__ x /*[in_dim] state vector*/,
                                            float (&a2)[HID]) {
  const int lane = threadIdx.x & 63;
  float acc[HID];
#pragma unroll
  for (int j = 0; j < HID; ++j) acc[j] = 0.f;
  for (int k = lane; k < g.in_dim; k += 64) {
    const float xv = x[k];
    const float* w = th + (long)k * HID;
#pragma unroll
    for (int j = 0; j < HID; ++j) acc[j] = fmaf(xv, w[j], acc[j]);
  }
  float a1[HID];
#pragma unroll
  for (int j = 0; j < HID; ++j) a1[j] = rc_lrelu(rc_wave_sum(acc[j]) + th[g.o_b1 + j]);
#pragma unroll
  for (int k = 0; k < HID; ++k) a2[k] = 0.f;
#pragma unroll
  for (int j = 0; j < HID; ++j)
#pragma unroll
    for (int k = 0; k < HID; ++k) a2[k] = fmaf(a1[j], th[g.o_W2 + j * HID + k], a2[k]);
#pragma unroll
  for (int k = 0; k < HID; ++k) a2[k] = rc_lrelu(a2[k] + th[g.o_b2 + k]);
}

template <int HID, int A>
__device__ __forceinline__ void wave_policy(const float* __restrict__ th, const NetGeom& g,
                                            const float* __restrict__ x, float (&p)[A]) {
  float a2[HID];
  wave_hidden<HID>(th, g, x, a2);
  float mx = -3.0e38f;
#pragma unroll
  for (int a = 0; a < A; ++a) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < HID; ++k) acc = fmaf(a2[k], th[g.o_W3 + k * A + a], acc);
    p[a] = acc + th[g.o_b3 + a];
    mx = fmaxf(mx, p[a]);
  }
  float se = 0.f;
#pragma unroll
  for (int a = 0; a < A; ++a) { p[a] = expf(p[a] - mx); se += p[a]; }
#pragma unroll
  for (int a = 0; a < A; ++a) p[a] = p[a] / se;
}

// one grid-world transition of one agent (environments/grid_world.py:52-64 with the
// dist_to_agents branch being dead: an agent always "collides" with itself)
__device__ __forceinline__ void env_transition(const EnvCfg& c, int a, int px, int py, int gx, int gy, int& nx,
                                               int& ny, int& reward_int) {
  const int dist = abs(px - gx) + abs(py - gy);            // distance BEFORE the move
  const int mx = (a == 1) ? -1 : (a == 2 ? 1 : 0);
  const int my = (a == 3) ? -1 : (a == 4 ? 1 : 0);
  nx = min(max(px + mx, 0), c.nrow - 1);
  ny = min(max(py + my, 0), c.nrow - 1);                   // nrow-1 on BOTH axes (:55)
  reward_int = (dist == 0 && a == 0) ? 0 : -dist - 1;
}

struct Replay {
  float* s; float* ns; float* sa; float* a; float* r;      // [S][cap][2N|2N|3N|N|N]
  long cap;
};

__device__ __forceinline__ void record_step(const EnvCfg& c, const Replay& rp, int S_idx, int N, int i, long row,
                                            int px, int py, int nx, int ny, int a, int reward_int,
                                            int* __restrict__ pos_next, float* __restrict__ xs_next,
                                            double* __restrict__ ret, double gpow) {
  const float sx = (float)(((double)px - c.mean_x) / c.std_x), sy = (float)(((double)py - c.mean_y) / c.std_y);
  const float tx = (float)(((double)nx - c.mean_x) / c.std_x), ty = (float)(((double)ny - c.mean_y) / c.std_y);
  const double rew = (double)reward_int / 5.0;             // get_data(): reward / 5 (:71)
  const long base = (long)S_idx * rp.cap + row;
  rp.s[base * 2 * N + 2 * i] = sx;  rp.s[base * 2 * N + 2 * i + 1] = sy;
  rp.ns[base * 2 * N + 2 * i] = tx; rp.ns[base * 2 * N + 2 * i + 1] = ty;
  rp.sa[base * 3 * N + 3 * i] = sx; rp.sa[base * 3 * N + 3 * i + 1] = sy; rp.sa[base * 3 * N + 3 * i + 2] = (float)a;
  rp.a[base * N + i] = (float)a;
  rp.r[base * N + i] = (float)rew;
  pos_next[((long)S_idx * N + i) * 2] = nx; pos_next[((long)S_idx * N + i) * 2 + 1] = ny;
  xs_next[(long)S_idx * 2 * N + 2 * i] = tx; xs_next[(long)S_idx * 2 * N + 2 * i + 1] = ty;
  ret[(long)S_idx * N + i] += rew * gpow;                  // ep_returns += reward*gamma**j (train_agents.py:71)
}

// probs[s][i][:] = actor_i(xs[s])
template <int HID, int A>
__global__ __launch_bounds__(256) void k_policy_probs(const float* __restrict__ xs, const float* __restrict__ theta,
                                                      float* __restrict__ probs, int N, int in_dim, int ldp) {
  const int s = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const NetGeom g = make_geom(in_dim, HID, A);
  float p[A];
  wave_policy<HID, A>(theta + ((long)s * N + i) * ldp, g, xs + (long)s * in_dim, p);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < A; ++a) probs[((long)s * N + i) * A + a] = p[a];
  }
}

// out[s][i] = value_i(xs[s])  (linear head, out_dim 1)
template <int HID>
__global__ __launch_bounds__(256) void k_value_rows(const float* __restrict__ xs, const float* __restrict__ theta,
                                                    float* __restrict__ out, int N, int in_dim, int ldp) {
  const int s = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const NetGeom g = make_geom(in_dim, HID, 1);
  const float* th = theta + ((long)s * N + i) * ldp;
  float a2[HID];
  wave_hidden<HID>(th, g, xs + (long)s * in_dim, a2);
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < HID; ++k) v = fmaf(a2[k], th[g.o_W3 + k], v);
  if ((threadIdx.x & 63) == 0) out[(long)s * N + i] = v + th[g.o_b3];
}

// what follows the policy of one (seed, agent) in a fused step: get_action's three draws (agents/resilient_CAC_agents.py:208-219),
// the transition and the replay append -- one lane; shared by the 20-unit kernel and the wide-actor kernel
template <int A>
__device__ __forceinline__ void rollout_tail(const float (&p)[A], const int* __restrict__ pos, const int* __restrict__ goal,
                                             const unsigned long long* __restrict__ seeds, const EnvCfg& cfg, const Replay& rp,
                                             long row, int* __restrict__ pos_next, float* __restrict__ xs_next,
                                             double* __restrict__ ret, double gpow, int episode, int step, float mu, int N,
                                             int* __restrict__ act_out, int s, int i) {
  const unsigned long long key = seeds[s];
  const RcPhilox rn = rc_philox4x32_10((uint32_t)i, (uint32_t)step, (uint32_t)episode, 0u, (uint32_t)key,
                                       (uint32_t)(key >> 32));
  const int a_rand = rc_mulhi_range(rn.r0, A);
  const float u1 = rc_u01(rn.r1), u2 = rc_u01(rn.r2);
  float c = 0.f;
  int a_pol = 0;
#pragma unroll
  for (int a = 0; a < A - 1; ++a) { c += p[a]; a_pol += (u1 >= c) ? 1 : 0; }
  const int act = (u2 < 1.0f - mu) ? a_pol : a_rand;
  const long pi = ((long)s * N + i) * 2;
  int nx, ny, rew;
  env_transition(cfg, act, pos[pi], pos[pi + 1], goal[pi], goal[pi + 1], nx, ny, rew);
  record_step(cfg, rp, s, N, i, row, pos[pi], pos[pi + 1], nx, ny, act, rew, pos_next, xs_next, ret, gpow);
  if (act_out) act_out[(long)s * N + i] = act;
}

// fused step, device RNG: actor forward -> sample -> transition -> replay/returns
template <int HID, int A>
__global__ __launch_bounds__(256) void k_rollout_step(const float* __restrict__ xs, const int* __restrict__ pos,
                                                      const int* __restrict__ goal, const float* __restrict__ theta,
                                                      const unsigned long long* __restrict__ seeds, EnvCfg cfg,
                                                      Replay rp, long row, int* __restrict__ pos_next,
                                                      float* __restrict__ xs_next, double* __restrict__ ret,
                                                      double gpow, int episode, int step, float mu, int N, int in_dim,
                                                      int ldp, int* __restrict__ act_out) {
  const int s = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const NetGeom g = make_geom(in_dim, HID, A);
  float p[A];
  wave_policy<HID, A>(theta + ((long)s * N + i) * ldp, g, xs + (long)s * in_dim, p);
  if ((threadIdx.x & 63) != 0) return;
  rollout_tail<A>(p, pos, goal, seeds, cfg, rp, row, pos_next, xs_next, ret, gpow, episode, step, mu, N, act_out, s, i);
}

// host-sampled actions (rng_mode='numpy'): transition + replay/returns only
__global__ __launch_bounds__(256) void k_env_apply(const int* __restrict__ pos, const int* __restrict__ goal,
                                                   const int* __restrict__ actions, EnvCfg cfg, Replay rp, long row,
                                                   int* __restrict__ pos_next, float* __restrict__ xs_next,
                                                   double* __restrict__ ret, double gpow, int S, int N) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)S * N) return;
  const int s = (int)(t / N), i = (int)(t - (long)s * N);
  int nx, ny, rew;
  env_transition(cfg, actions[t], pos[t * 2], pos[t * 2 + 1], goal[t * 2], goal[t * 2 + 1], nx, ny, rew);
  record_step(cfg, rp, s, N, i, row, pos[t * 2], pos[t * 2 + 1], nx, ny, actions[t], rew, pos_next, xs_next, ret, gpow);
}

// episode start: positions (device RNG or copied from `pos_in`), scaled state vector, returns = 0
__global__ __launch_bounds__(256) void k_env_reset(const int* __restrict__ pos_in,
                                                   const unsigned long long* __restrict__ seeds, EnvCfg cfg,
                                                   int episode, int* __restrict__ pos, float* __restrict__ xs,
                                                   double* __restrict__ ret, int S, int N) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)S * N) return;
  const int s = (int)(t / N), i = (int)(t - (long)s * N);
  int px, py;
  if (pos_in) {
    px = pos_in[t * 2]; py = pos_in[t * 2 + 1];
  } else {
    const unsigned long long key = seeds[s];
    const RcPhilox rn = rc_philox4x32_10((uint32_t)i, 0u, (uint32_t)episode, 1u, (uint32_t)key, (uint32_t)(key >> 32));
    px = rc_mulhi_range(rn.r0, cfg.nrow); py = rc_mulhi_range(rn.r1, cfg.ncol);
  }
  pos[t * 2] = px; pos[t * 2 + 1] = py;
  xs[t * 2] = (float)(((double)px - cfg.mean_x) / cfg.std_x);
  xs[t * 2 + 1] = (float)(((double)py - cfg.mean_y) / cfg.std_y);
  ret[t] = 0.0;
}


// ---------------------------------------------------------------------------------------------
// Episode-parallel rollout (rng_mode 'device').
//
// Between two update blocks every network is frozen (training/train_agents.py:86: updates happen
// only after n_ep_fixed episodes) and, with the counter-based Philox stream, every draw is a pure
// function of (seed, episode, step, agent).  The n_ep_fixed episodes of a block are therefore
// independent and are stepped TOGETHER: one lane = one episode, one wavefront = one (seed, agent),
// so the agent's actor weights are read ONCE per environment step for all E episodes (wave-uniform
// scalar loads) instead of once per episode, and a block needs max_ep_len launches instead of
// n_ep_fixed*max_ep_len.  State is kept episode-minor so lanes are coalesced:
//   xsT[S][2N][EP]   scaled global state, feature-major      posT[S][N][2][EP]   integer cells
//   retT[S][N][EP]   discounted returns (double)             EP = E rounded up to 64
template <int HID>
__device__ __forceinline__ void lane_hidden(const float* __restrict__ th, const NetGeom& g,
                                            const float* __restrict__ xT /*[in_dim][EP]*/, int EP, int e,
                                            float (&a2)[HID]) {
  float acc[HID];
#pragma unroll
  for (int j = 0; j < HID; ++j) acc[j] = 0.f;
#pragma unroll 4
  for (int k = 0; k < g.in_dim; ++k) {
    const float xv = xT[(long)k * EP + e];
    const float* w = th + (long)k * HID;
#pragma unroll
    for (int j = 0; j < HID; ++j) acc[j] = fmaf(xv, w[j], acc[j]);
  }
  float a1[HID];
#pragma unroll
  for (int j = 0; j < HID; ++j) a1[j] = rc_lrelu(acc[j] + th[g.o_b1 + j]);
#pragma unroll
  for (int k = 0; k < HID; ++k) a2[k] = 0.f;
#pragma unroll
  for (int j = 0; j < HID; ++j)
#pragma unroll
    for (int k = 0; k < HID; ++k) a2[k] = fmaf(a1[j], th[g.o_W2 + j * HID + k], a2[k]);
#pragma unroll
  for (int k = 0; k < HID; ++k) a2[k] = rc_lrelu(a2[k] + th[g.o_b2 + k]);
}

// the same for lane = episode e of the episode-parallel step: draws, transition, replay row row0 + e*ep_len + step; shared by the
// 20-unit kernel and the wide-actor kernel
template <int A>
__device__ __forceinline__ void rollout_tail_ep(const float (&p)[A], const int* __restrict__ posT, const int* __restrict__ goal,
                                                const unsigned long long* __restrict__ seeds, const EnvCfg& cfg, const Replay& rp,
                                                long row0, int ep_len, int* __restrict__ posT_next, float* __restrict__ xsT_next,
                                                double* __restrict__ retT, double gpow, int episode0, int step, float mu, int N,
                                                int EP, int s, int i, int e) {
  const int in_dim = 2 * N;
  const unsigned long long key = seeds[s];
  const RcPhilox rn = rc_philox4x32_10((uint32_t)i, (uint32_t)step, (uint32_t)(episode0 + e), 0u, (uint32_t)key,
                                       (uint32_t)(key >> 32));
  const int a_rand = rc_mulhi_range(rn.r0, A);
  const float u1 = rc_u01(rn.r1), u2 = rc_u01(rn.r2);
  float c = 0.f;
  int a_pol = 0;
#pragma unroll
  for (int a = 0; a < A - 1; ++a) { c += p[a]; a_pol += (u1 >= c) ? 1 : 0; }
  const int act = (u2 < 1.0f - mu) ? a_pol : a_rand;
  const long pi = (((long)s * N + i) * 2) * EP + e;
  const int px = posT[pi], py = posT[pi + EP];
  const long gi = ((long)s * N + i) * 2;
  int nx, ny, rew;
  env_transition(cfg, act, px, py, goal[gi], goal[gi + 1], nx, ny, rew);
  const float sx = (float)(((double)px - cfg.mean_x) / cfg.std_x), sy = (float)(((double)py - cfg.mean_y) / cfg.std_y);
  const float tx = (float)(((double)nx - cfg.mean_x) / cfg.std_x), ty = (float)(((double)ny - cfg.mean_y) / cfg.std_y);
  const double rw = (double)rew / 5.0;
  const long base = (long)s * rp.cap + row0 + (long)e * ep_len + step;     // replay row of (episode e, step)
  rp.s[base * 2 * N + 2 * i] = sx;  rp.s[base * 2 * N + 2 * i + 1] = sy;
  rp.ns[base * 2 * N + 2 * i] = tx; rp.ns[base * 2 * N + 2 * i + 1] = ty;
  rp.sa[base * 3 * N + 3 * i] = sx; rp.sa[base * 3 * N + 3 * i + 1] = sy; rp.sa[base * 3 * N + 3 * i + 2] = (float)act;
  rp.a[base * N + i] = (float)act;
  rp.r[base * N + i] = (float)rw;
  posT_next[pi] = nx; posT_next[pi + EP] = ny;
  xsT_next[((long)s * in_dim + 2 * i) * EP + e] = tx;
  xsT_next[((long)s * in_dim + 2 * i + 1) * EP + e] = ty;
  retT[((long)s * N + i) * EP + e] += rw * gpow;
}

template <int HID, int A>
__global__ __launch_bounds__(256) void k_rollout_step_ep(const float* __restrict__ xsT, const int* __restrict__ posT,
                                                         const int* __restrict__ goal,
                                                         const float* __restrict__ theta,
                                                         const unsigned long long* __restrict__ seeds, EnvCfg cfg,
                                                         Replay rp, long row0, int ep_len, int* __restrict__ posT_next,
                                                         float* __restrict__ xsT_next, double* __restrict__ retT,
                                                         double gpow, int episode0, int step, float mu, int N, int E,
                                                         int EP, int ldp) {
  const int s = blockIdx.y;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (i >= N) return;
  const int e = blockIdx.z * 64 + (threadIdx.x & 63);
  const int in_dim = 2 * N;
  const NetGeom g = make_geom(in_dim, HID, A);
  const float* th = theta + ((long)s * N + i) * ldp;
  float a2[HID];
  lane_hidden<HID>(th, g, xsT + (long)s * in_dim * EP, EP, e, a2);
  float p[A];
  float mx = -3.0e38f;
#pragma unroll
  for (int a = 0; a < A; ++a) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < HID; ++k) acc = fmaf(a2[k], th[g.o_W3 + k * A + a], acc);
    p[a] = acc + th[g.o_b3 + a];
    mx = fmaxf(mx, p[a]);
  }
  float se = 0.f;
#pragma unroll
  for (int a = 0; a < A; ++a) { p[a] = expf(p[a] - mx); se += p[a]; }
#pragma unroll
  for (int a = 0; a < A; ++a) p[a] = p[a] / se;
  if (e >= E) return;
  rollout_tail_ep<A>(p, posT, goal, seeds, cfg, rp, row0, ep_len, posT_next, xsT_next, retT, gpow, episode0, step, mu, N, EP, s, i, e);
}

// est[(e*S + s)*N + i] = critic_i(start state of episode e)      (training/train_agents.py:60-62)
template <int HID>
__global__ __launch_bounds__(256) void k_value_rows_ep(const float* __restrict__ xsT, const float* __restrict__ theta,
                                                       float* __restrict__ est, int S, int N, int E, int EP, int ldp) {
  const int s = blockIdx.y;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (i >= N) return;
  const int e = blockIdx.z * 64 + (threadIdx.x & 63);
  const int in_dim = 2 * N;
  const NetGeom g = make_geom(in_dim, HID, 1);
  const float* th = theta + ((long)s * N + i) * ldp;
  float a2[HID];
  lane_hidden<HID>(th, g, xsT + (long)s * in_dim * EP, EP, e, a2);
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < HID; ++k) v = fmaf(a2[k], th[g.o_W3 + k], v);
  if (e < E) est[((long)e * S + s) * N + i] = v + th[g.o_b3];
}

__global__ __launch_bounds__(256) void k_env_reset_ep(const int* __restrict__ pos_in,
                                                      const unsigned long long* __restrict__ seeds, EnvCfg cfg,
                                                      int episode0, int* __restrict__ posT, float* __restrict__ xsT,
                                                      double* __restrict__ retT, int S, int N, int E, int EP) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)S * N * EP) return;
  const int e = (int)(t % EP);
  const long si = t / EP;
  const int s = (int)(si / N), i = (int)(si - (long)s * N);
  int px = 0, py = 0;
  if (e < E) {
    if (pos_in) {
      px = pos_in[si * 2]; py = pos_in[si * 2 + 1];
    } else {
      const unsigned long long key = seeds[s];
      const RcPhilox rn = rc_philox4x32_10((uint32_t)i, 0u, (uint32_t)(episode0 + e), 1u, (uint32_t)key, (uint32_t)(key >> 32));
      px = rc_mulhi_range(rn.r0, cfg.nrow); py = rc_mulhi_range(rn.r1, cfg.ncol);
    }
  }
  posT[(si * 2) * EP + e] = px; posT[(si * 2 + 1) * EP + e] = py;
  xsT[((long)s * 2 * N + 2 * i) * EP + e] = (float)(((double)px - cfg.mean_x) / cfg.std_x);
  xsT[((long)s * 2 * N + 2 * i + 1) * EP + e] = (float)(((double)py - cfg.mean_y) / cfg.std_y);
  retT[si * EP + e] = 0.0;
}

// ---------------------------------------------------------------------------------------------
// Wide actors (hid != 20; EngineConfig.actor_hid).  The same reference lines as above -- actor.predict inside get_action
// (agents/resilient_CAC_agents.py:208-219) and the step that follows (training/train_agents.py:66-80) -- for a policy network
// of any hidden width.
//
// Plain form, any width: one workgroup per (seed, agent), one state.  Thread = hidden unit (coalesced over the units of a weight
// row), fp32 FMAs in k order, activations in LDS (2 * hid floats).  The parity anchor of the matrix-core kernel below.
__device__ __forceinline__ void wide_policy_block(const float* __restrict__ th, const NetGeom& g, const float* __restrict__ x,
                                                  float* __restrict__ sm /*[2 * hid + 8]*/, float (&p)[5]) {
  constexpr int A = 5;
  const int t = threadIdx.x, hid = g.hid;
  float* __restrict__ a1 = sm;
  float* __restrict__ a2 = sm + hid;
  float* __restrict__ lg = sm + 2 * hid;
  for (int j = t; j < hid; j += 256) {
    float acc = 0.f;
    for (int k = 0; k < g.in_dim; ++k) acc = fmaf(x[k], th[(long)k * hid + j], acc);
    a1[j] = rc_lrelu(acc + th[g.o_b1 + j]);
  }
  __syncthreads();
  for (int k = t; k < hid; k += 256) {
    float acc = 0.f;
    for (int j = 0; j < hid; ++j) acc = fmaf(a1[j], th[g.o_W2 + (long)j * hid + k], acc);
    a2[k] = rc_lrelu(acc + th[g.o_b2 + k]);
  }
  __syncthreads();
  if (t < A) {
    float acc = 0.f;
    for (int k = 0; k < hid; ++k) acc = fmaf(a2[k], th[g.o_W3 + k * A + t], acc);
    lg[t] = acc + th[g.o_b3 + t];
  }
  __syncthreads();
  float mx = -3.0e38f;
#pragma unroll
  for (int a = 0; a < A; ++a) { p[a] = lg[a]; mx = fmaxf(mx, p[a]); }
  float se = 0.f;
#pragma unroll
  for (int a = 0; a < A; ++a) { p[a] = expf(p[a] - mx); se += p[a]; }
#pragma unroll
  for (int a = 0; a < A; ++a) p[a] = p[a] / se;
}

__global__ __launch_bounds__(256) void k_policy_probs_wide(const float* __restrict__ xs, const float* __restrict__ theta,
                                                           float* __restrict__ probs, int N, int in_dim, int hid, int ldp) {
  RCMARL_DYN_SMEM(float, sm);
  const int s = blockIdx.y, i = blockIdx.x;
  const NetGeom g = make_geom(in_dim, hid, 5);
  float p[5];
  wide_policy_block(theta + ((long)s * N + i) * ldp, g, xs + (long)s * in_dim, sm, p);
  if (threadIdx.x < 5) probs[((long)s * N + i) * 5 + threadIdx.x] = p[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_rollout_step_wide(const float* __restrict__ xs, const int* __restrict__ pos,
                                                           const int* __restrict__ goal, const float* __restrict__ theta,
                                                           const unsigned long long* __restrict__ seeds, EnvCfg cfg, Replay rp,
                                                           long row, int* __restrict__ pos_next, float* __restrict__ xs_next,
                                                           double* __restrict__ ret, double gpow, int episode, int step, float mu,
                                                           int N, int in_dim, int hid, int ldp, int* __restrict__ act_out) {
  RCMARL_DYN_SMEM(float, sm);
  const int s = blockIdx.y, i = blockIdx.x;
  const NetGeom g = make_geom(in_dim, hid, 5);
  float p[5];
  wide_policy_block(theta + ((long)s * N + i) * ldp, g, xs + (long)s * in_dim, sm, p);
  if (threadIdx.x != 0) return;
  rollout_tail<5>(p, pos, goal, seeds, cfg, rp, row, pos_next, xs_next, ret, gpow, episode, step, mu, N, act_out, s, i);
}

// Matrix-core form, episode-parallel (hid a multiple of 32, up to RW_MAX_HID): one workgroup of eight wavefronts per (seed, agent,
// block of 64 episodes).  Both layers are GEMMs with the 64 episodes as columns,
//     a1[hid x 64] = lrelu(W1^T[hid x 2N] xT[2N x 64] + b1),   a2[hid x 64] = lrelu(W2^T[hid x hid] a1 + b2),
// on v_mfma_f32_32x32x16_f16 with both operands as two f16 pieces of the value times a power of two (rcmarl_lattice.h: weights
// 2^10, activations and states 2^6) and three piece products per fp32 product (l*h + h*l + h*h), fp32 accumulate.  A wavefront
// owns two 32-unit row tiles of the output and both 32-episode column tiles.  Its weight fragments go straight from global memory
// to registers (a weight is used by one wavefront only: lane (unit, k-group) reads 8 k-rows of its unit's column, 128 contiguous
// bytes per k-row across the lanes) and are split there; the state tile, which all wavefronts share, is split once and staged through
// LDS in fragment order (two stages, one barrier per 32-feature tile).  a1 is written to LDS as pieces in the fragment order layer 2
// reads; a2 stays in the accumulators and is folded into the five logits at once.  So the kernel's global traffic is the actor's
// weights, read once per (seed, agent) and step, plus the (L2-resident) state tile.  A workgroup whose operands leave the f16 range
// (|scaled value| > 65000: weights beyond 63, activations beyond 1015) redoes both layers with v_mfma_f32_32x32x2_f32 on the fp32
// values, as k_wgemm16 does; with the exact operand form selected (rcmarl_lattice_set_f16_mode(0) / rcmarl_wide_set_f16_mode(0)) every
// workgroup takes that path.
constexpr int RW_THREADS = 512, RW_WAVES = 8, RW_MT = 2, RW_KT = 32, RW_MAX_HID = RW_WAVES * RW_MT * 32;
constexpr int RW_XPLANE = 4 * 64 * 16;                  // bytes: one piece of a [32 features x 64 episodes] state tile, fragment order
constexpr int RW_XSTAGES = 2 * 2 * RW_XPLANE;           // two stages of two pieces
constexpr int RW_PART = RW_WAVES * 5 * 64 * 4;          // logit parts [wave][action][episode]
#define RC_RW_RANGE 65000.f
static inline size_t rw_smem(int hid) { return (size_t)256 * hid + RW_XSTAGES + RW_PART + 16; }

struct RwCtx {
  const float* th; NetGeom g;
  const float* xT; int EP, e0;                         // state tile of this seed: xT[k * EP + e0 + episode]
  unsigned char* a1s; unsigned char* xst; float* part; // LDS
  int ut[RW_MT]; bool act[RW_MT];                      // this wavefront's unit tiles (wave-uniform)
};

// a2 tile -> logit parts of this lane's episode columns
__device__ __forceinline__ void rw_fold_logits(const RwCtx& c, const rc_f32x16 (&acc)[RW_MT][2], float unscale, float (&lp)[2][5]) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int mt = 0; mt < RW_MT; ++mt) {
    if (!c.act[mt]) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = c.ut[mt] + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
      const float b2 = c.th[c.g.o_b2 + u];
      const float* __restrict__ w3 = c.th + c.g.o_W3 + u * 5;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const float a2 = rc_lrelu(acc[mt][nt][r] * unscale + b2);
#pragma unroll
        for (int a = 0; a < 5; ++a) lp[nt][a] = fmaf(a2, w3[a], lp[nt][a]);
      }
    }
  }
}

__device__ __forceinline__ void rw_zero(rc_f32x16 (&acc)[RW_MT][2]) {
#pragma unroll
  for (int mt = 0; mt < RW_MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
}

// one layer on two-piece f16 operands: acc[mt][nt] = sum_k W[k][unit] B(k, episode), K a multiple of 32 or zero-filled beyond.
// FROM_X: B is the state tile (global -> split -> LDS stages); otherwise the a1 pieces already in LDS.  Returns max |scaled operand|.
template <bool FROM_X>
__device__ __forceinline__ float rw_layer_f16(const RwCtx& c, const float* __restrict__ W, int K, rc_f32x16 (&acc)[RW_MT][2], float amax) {
  const int t = threadIdx.x, l = t & 63, kg = l >> 5, i = l & 31, hid = c.g.hid;
  const int nk = (K + RW_KT - 1) / RW_KT;
  float wa[RW_MT][2][8], xr[8];
  const int xep = t & 63, xslot = t >> 6;              // staging: threads 0..255 own (episode, 8-feature group) of the tile
  auto load_w = [&](int kt) {
#pragma unroll
    for (int mt = 0; mt < RW_MT; ++mt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = kt * RW_KT + ks * 16 + kg * 8 + e;
          wa[mt][ks][e] = (c.act[mt] && k < K) ? W[(long)k * hid + c.ut[mt] + i] : 0.f;
        }
  };
  auto load_x = [&](int kt) {
    if (FROM_X && xslot < 4) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = kt * RW_KT + xslot * 8 + e;
        xr[e] = k < K ? c.xT[(long)k * c.EP + c.e0 + xep] : 0.f;
      }
    }
  };
  rw_zero(acc);
  load_w(0);
  load_x(0);
  for (int kt = 0; kt < nk; ++kt) {
    unsigned char* __restrict__ st = c.xst + (kt & 1) * (2 * RW_XPLANE);
    if (FROM_X) {
      if (xslot < 4) {
        float xs8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { xs8[e] = xr[e] * RC_F16_ACT_SCALE; amax = fmaxf(amax, fabsf(xs8[e])); }
        uint4 h, lo;
        rc_split2h_x8(xs8, h, lo);
        *reinterpret_cast<uint4*>(st + (xslot * 64 + xep) * 16) = h;
        *reinterpret_cast<uint4*>(st + RW_XPLANE + (xslot * 64 + xep) * 16) = lo;
      }
    }
    uint4 ah[RW_MT][2], al[RW_MT][2];
#pragma unroll
    for (int mt = 0; mt < RW_MT; ++mt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        float ws8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { ws8[e] = wa[mt][ks][e] * RC_F16_W_SCALE; amax = fmaxf(amax, fabsf(ws8[e])); }
        rc_split2h_x8(ws8, ah[mt][ks], al[mt][ks]);
      }
    if (FROM_X) __syncthreads();                       // stage kt filled; every wavefront is past its reads of stage kt - 2
    if (kt + 1 < nk) { load_w(kt + 1); load_x(kt + 1); }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        uint4 bh, bl;
        if (FROM_X) {
          bh = *reinterpret_cast<const uint4*>(st + ((ks * 2 + kg) * 64 + nt * 32 + i) * 16);
          bl = *reinterpret_cast<const uint4*>(st + RW_XPLANE + ((ks * 2 + kg) * 64 + nt * 32 + i) * 16);
        } else {
          const int slot = (kt * 2 + ks) * 2 + kg;
          bh = *reinterpret_cast<const uint4*>(c.a1s + ((long)slot * 64 + nt * 32 + i) * 16);
          bl = *reinterpret_cast<const uint4*>(c.a1s + (long)128 * hid + ((long)slot * 64 + nt * 32 + i) * 16);
        }
#pragma unroll
        for (int mt = 0; mt < RW_MT; ++mt) {
          if (!c.act[mt]) continue;                    // (wave-uniform)
          acc[mt][nt] = rc_mfma_f16(al[mt][ks], bh, acc[mt][nt]);
          acc[mt][nt] = rc_mfma_f16(ah[mt][ks], bl, acc[mt][nt]);
          acc[mt][nt] = rc_mfma_f16(ah[mt][ks], bh, acc[mt][nt]);
        }
      }
  }
  return amax;
}

// the same layer on the fp32 values (v_mfma_f32_32x32x2_f32): B(k, episode) = xT (global) or the fp32 a1 in LDS ([unit][64])
template <bool FROM_X>
__device__ __forceinline__ void rw_layer_f32(const RwCtx& c, const float* __restrict__ W, int K, rc_f32x16 (&acc)[RW_MT][2]) {
  const int l = threadIdx.x & 63, kg = l >> 5, i = l & 31, hid = c.g.hid;
  const float* __restrict__ a1f = reinterpret_cast<const float*>(c.a1s);
  rw_zero(acc);
  for (int k2 = 0; k2 < K; k2 += 2) {
    const int k = k2 + kg;
    float b[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      b[nt] = k >= K ? 0.f : (FROM_X ? c.xT[(long)k * c.EP + c.e0 + nt * 32 + i] : a1f[k * 64 + nt * 32 + i]);
#pragma unroll
    for (int mt = 0; mt < RW_MT; ++mt) {
      if (!c.act[mt]) continue;
      const float a = k < K ? W[(long)k * hid + c.ut[mt] + i] : 0.f;
      acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[0], acc[mt][0], 0, 0, 0);
      acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[1], acc[mt][1], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(RW_THREADS) void k_rollout_step_ep_wide(const float* __restrict__ xsT, const int* __restrict__ posT,
                                                                     const int* __restrict__ goal, const float* __restrict__ theta,
                                                                     const unsigned long long* __restrict__ seeds, EnvCfg cfg,
                                                                     Replay rp, long row0, int ep_len, int* __restrict__ posT_next,
                                                                     float* __restrict__ xsT_next, double* __restrict__ retT,
                                                                     double gpow, int episode0, int step, float mu, int N, int E,
                                                                     int EP, int hid, int ldp, int f16,
                                                                     float* __restrict__ probs_out) {
  RCMARL_DYN_SMEM(unsigned char, sm);
  const int s = blockIdx.y, i = blockIdx.x, t = threadIdx.x, l = t & 63, w = t >> 6;
  const int in_dim = 2 * N;
  RwCtx c;
  c.g = make_geom(in_dim, hid, 5);
  c.th = theta + ((long)s * N + i) * ldp;
  c.xT = xsT + (long)s * in_dim * EP;
  c.EP = EP; c.e0 = blockIdx.z * 64;
  c.a1s = sm;
  c.xst = sm + (size_t)256 * hid;
  c.part = reinterpret_cast<float*>(c.xst + RW_XSTAGES);
  int* s_ovf = reinterpret_cast<int*>(c.xst + RW_XSTAGES + RW_PART);
#pragma unroll
  for (int mt = 0; mt < RW_MT; ++mt) { c.ut[mt] = (w * RW_MT + mt) * 32; c.act[mt] = c.ut[mt] < hid; }
  if (t == 0) *s_ovf = 0;
  __syncthreads();
  rc_f32x16 acc[RW_MT][2];
  float lp[2][5];
  bool exact = !f16;
  if (!exact) {
    rc_f16_saturate();
    float amax = rw_layer_f16<true>(c, c.th, in_dim, acc, 0.f);
    // a1 -> LDS as pieces, in the fragment order of layer 2: unit u = contraction index, 8 consecutive units per 16-byte fragment
    const float un1 = 1.f / (RC_F16_W_SCALE * RC_F16_ACT_SCALE);
#pragma unroll
    for (int mt = 0; mt < RW_MT; ++mt) {
      if (!c.act[mt]) continue;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int u = c.ut[mt] + 8 * q + 4 * (l >> 5);                 // four consecutive units: registers 4q .. 4q+3
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = rc_lrelu(acc[mt][nt][4 * q + e] * un1 + c.th[c.g.o_b1 + u + e]) * RC_F16_ACT_SCALE;
            amax = fmaxf(amax, fabsf(v[e]));
          }
          uint2 h, lo;
          rc_split2h_pair(v[0], v[1], h.x, lo.x);
          rc_split2h_pair(v[2], v[3], h.y, lo.y);
          const long off = ((long)(u >> 3) * 64 + nt * 32 + (l & 31)) * 16 + (u & 7) * 2;
          *reinterpret_cast<uint2*>(c.a1s + off) = h;
          *reinterpret_cast<uint2*>(c.a1s + (long)128 * hid + off) = lo;
        }
    }
    __syncthreads();
    amax = rw_layer_f16<false>(c, c.th + c.g.o_W2, hid, acc, amax);
    if (amax > RC_RW_RANGE) *s_ovf = 1;               // (NaN operands do not take this branch: they poison either form alike)
    __syncthreads();
    exact = *s_ovf != 0;                               // workgroup-uniform
    if (!exact) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int a = 0; a < 5; ++a) lp[nt][a] = 0.f;
      rw_fold_logits(c, acc, un1, lp);
    }
  }
  if (exact) {
    rw_layer_f32<true>(c, c.th, in_dim, acc);
    float* __restrict__ a1f = reinterpret_cast<float*>(c.a1s);
#pragma unroll
    for (int mt = 0; mt < RW_MT; ++mt) {
      if (!c.act[mt]) continue;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int u = c.ut[mt] + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
          a1f[u * 64 + nt * 32 + (l & 31)] = rc_lrelu(acc[mt][nt][r] + c.th[c.g.o_b1 + u]);
        }
    }
    __syncthreads();
    rw_layer_f32<false>(c, c.th + c.g.o_W2, hid, acc);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int a = 0; a < 5; ++a) lp[nt][a] = 0.f;
    rw_fold_logits(c, acc, 1.f, lp);
  }
  // logit parts: the two row halves of a tile meet in the lane pair (l, l ^ 32), the wavefronts in LDS, summed in wavefront order
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      const float v = lp[nt][a] + __shfl_xor(lp[nt][a], 32, 64);
      if (l < 32) c.part[(w * 5 + a) * 64 + nt * 32 + l] = v;
    }
  __syncthreads();
  if (w != 0) return;
  float p[5];
  float mx = -3.0e38f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    float v = 0.f;
    for (int q = 0; q < RW_WAVES; ++q) v += c.part[(q * 5 + a) * 64 + l];
    p[a] = v + c.th[c.g.o_b3 + a];
    mx = fmaxf(mx, p[a]);
  }
  float se = 0.f;
#pragma unroll
  for (int a = 0; a < 5; ++a) { p[a] = expf(p[a] - mx); se += p[a]; }
#pragma unroll
  for (int a = 0; a < 5; ++a) p[a] = p[a] / se;
  const int e = c.e0 + l;
  if (e >= E) return;
  if (probs_out) {                                     // rcmarl_policy_probs_episodes_wide: the policy only (workgroup-uniform)
#pragma unroll
    for (int a = 0; a < 5; ++a) probs_out[(((long)s * N + i) * EP + e) * 5 + a] = p[a];
    return;
  }
  rollout_tail_ep<5>(p, posT, goal, seeds, cfg, rp, row0, ep_len, posT_next, xsT_next, retT, gpow, episode0, step, mu, N, EP, s, i, e);
}

}  // namespace

#define RC_HID_SWITCH(hid, STMT)               \
  switch (hid) {                               \
    case 20: { constexpr int HID_ = 20; STMT; } break; \
    default: return RCMARL_ERR_UNSUPPORTED;    \
  }

RCMARL_EXPORT int rcmarl_policy_probs(const float* xs, const float* theta, float* probs, int S, int N, int in_dim,
                                      int hid, int n_actions, int ldp, void* stream) {
  if (!xs || !theta || !probs || S <= 0 || N <= 0 || in_dim <= 0 || (ldp & 63)) return RCMARL_ERR_ARG;
  if (n_actions != 5) return RCMARL_ERR_UNSUPPORTED;
  const dim3 grid(rc_ceil_div(N, 4), S), block(256);
  RC_HID_SWITCH(hid, RCMARL_LAUNCH((k_policy_probs<HID_, 5>), grid, block, 0, stream, xs, theta, probs, N, in_dim, ldp));
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_value_rows(const float* xs, const float* theta, float* out, int S, int N, int in_dim, int hid,
                                    int ldp, void* stream) {
  if (!xs || !theta || !out || S <= 0 || N <= 0 || in_dim <= 0 || (ldp & 63)) return RCMARL_ERR_ARG;
  const dim3 grid(rc_ceil_div(N, 4), S), block(256);
  RC_HID_SWITCH(hid, RCMARL_LAUNCH((k_value_rows<HID_>), grid, block, 0, stream, xs, theta, out, N, in_dim, ldp));
  return rcmarl_check_launch();
}

// env_cfg = {nrow, ncol}; scale = {mean_x, mean_y, std_x, std_y}
RCMARL_EXPORT int rcmarl_rollout_step(const float* xs, const int* pos, const int* goal, const float* theta,
                                      const unsigned long long* seeds, int nrow, int ncol, const double* scale,
                                      float* rp_s, float* rp_ns, float* rp_sa, float* rp_a, float* rp_r, long cap,
                                      long row, int* pos_next, float* xs_next, double* ret, double gpow, int episode,
                                      int step, float mu, int S, int N, int hid, int n_actions, int ldp,
                                      int* act_out, void* stream) {
  if (!xs || !pos || !goal || !theta || !seeds || !scale || !rp_s || !rp_ns || !rp_sa || !rp_a || !rp_r ||
      !pos_next || !xs_next || !ret || row < 0 || row >= cap || S <= 0 || N <= 0 || (ldp & 63))
    return RCMARL_ERR_ARG;
  if (n_actions != 5) return RCMARL_ERR_UNSUPPORTED;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const Replay rp{rp_s, rp_ns, rp_sa, rp_a, rp_r, cap};
  const dim3 grid(rc_ceil_div(N, 4), S), block(256);
  RC_HID_SWITCH(hid, RCMARL_LAUNCH((k_rollout_step<HID_, 5>), grid, block, 0, stream, xs, pos, goal, theta, seeds, cfg,
                                   rp, row, pos_next, xs_next, ret, gpow, episode, step, mu, N, 2 * N, ldp, act_out));
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_env_apply(const int* pos, const int* goal, const int* actions, int nrow, int ncol,
                                   const double* scale, float* rp_s, float* rp_ns, float* rp_sa, float* rp_a,
                                   float* rp_r, long cap, long row, int* pos_next, float* xs_next, double* ret,
                                   double gpow, int S, int N, void* stream) {
  if (!pos || !goal || !actions || !scale || !rp_s || !rp_ns || !rp_sa || !rp_a || !rp_r || !pos_next || !xs_next ||
      !ret || row < 0 || row >= cap || S <= 0 || N <= 0)
    return RCMARL_ERR_ARG;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const Replay rp{rp_s, rp_ns, rp_sa, rp_a, rp_r, cap};
  const dim3 grid(rc_ceil_div(S * N, 256)), block(256);
  RCMARL_LAUNCH(k_env_apply, grid, block, 0, stream, pos, goal, actions, cfg, rp, row, pos_next, xs_next, ret, gpow, S, N);
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_env_reset(const int* pos_in, const unsigned long long* seeds, int nrow, int ncol,
                                   const double* scale, int episode, int* pos, float* xs, double* ret, int S, int N,
                                   void* stream) {
  if ((!pos_in && !seeds) || !scale || !pos || !xs || !ret || S <= 0 || N <= 0) return RCMARL_ERR_ARG;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const dim3 grid(rc_ceil_div(S * N, 256)), block(256);
  RCMARL_LAUNCH(k_env_reset, grid, block, 0, stream, pos_in, seeds, cfg, episode, pos, xs, ret, S, N);
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_rollout_step_episodes(const float* xsT, const int* posT, const int* goal, const float* theta,
                                               const unsigned long long* seeds, int nrow, int ncol, const double* scale,
                                               float* rp_s, float* rp_ns, float* rp_sa, float* rp_a, float* rp_r,
                                               long cap, long row0, int ep_len, int* posT_next, float* xsT_next,
                                               double* retT, double gpow, int episode0, int step, float mu, int S, int N,
                                               int E, int EP, int hid, int n_actions, int ldp, void* stream) {
  if (!xsT || !posT || !goal || !theta || !seeds || !scale || !rp_s || !rp_ns || !rp_sa || !rp_a || !rp_r ||
      !posT_next || !xsT_next || !retT || row0 < 0 || E <= 0 || EP < E || (EP & 63) || ep_len <= 0 || step < 0 ||
      step >= ep_len || row0 + (long)E * ep_len > cap || S <= 0 || N <= 0 || (ldp & 63))
    return RCMARL_ERR_ARG;
  if (n_actions != 5) return RCMARL_ERR_UNSUPPORTED;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const Replay rp{rp_s, rp_ns, rp_sa, rp_a, rp_r, cap};
  const dim3 grid(rc_ceil_div(N, 4), S, EP / 64), block(256);
  RC_HID_SWITCH(hid, RCMARL_LAUNCH((k_rollout_step_ep<HID_, 5>), grid, block, 0, stream, xsT, posT, goal, theta, seeds,
                                   cfg, rp, row0, ep_len, posT_next, xsT_next, retT, gpow, episode0, step, mu, N, E, EP,
                                   ldp));
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_value_rows_episodes(const float* xsT, const float* theta, float* est, int S, int N, int E, int EP,
                                             int hid, int ldp, void* stream) {
  if (!xsT || !theta || !est || S <= 0 || N <= 0 || E <= 0 || EP < E || (EP & 63) || (ldp & 63)) return RCMARL_ERR_ARG;
  const dim3 grid(rc_ceil_div(N, 4), S, EP / 64), block(256);
  RC_HID_SWITCH(hid, RCMARL_LAUNCH((k_value_rows_ep<HID_>), grid, block, 0, stream, xsT, theta, est, S, N, E, EP, ldp));
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_env_reset_episodes(const int* pos_in, const unsigned long long* seeds, int nrow, int ncol,
                                            const double* scale, int episode0, int* posT, float* xsT, double* retT,
                                            int S, int N, int E, int EP, void* stream) {
  if ((!pos_in && !seeds) || !scale || !posT || !xsT || !retT || S <= 0 || N <= 0 || E <= 0 || EP < E || (EP & 63))
    return RCMARL_ERR_ARG;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const long total = (long)S * N * EP;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  RCMARL_LAUNCH(k_env_reset_ep, grid, block, 0, stream, pos_in, seeds, cfg, episode0, posT, xsT, retT, S, N, E, EP);
  return rcmarl_check_launch();
}

// ---- wide actors (any hidden width) -------------------------------------------------------------------------------------
extern "C" int rcmarl_wide_f16_mode();

RCMARL_EXPORT int rcmarl_policy_probs_wide(const float* xs, const float* theta, float* probs, int S, int N, int in_dim, int hid,
                                           int n_actions, int ldp, void* stream) {
  if (!xs || !theta || !probs || S <= 0 || N <= 0 || in_dim <= 0 || hid <= 0 || (ldp & 63)) return RCMARL_ERR_ARG;
  if (n_actions != 5) return RCMARL_ERR_UNSUPPORTED;
  const size_t smem = (size_t)(2 * hid + 8) * sizeof(float);
  if (smem > 64 * 1024) return RCMARL_ERR_UNSUPPORTED;
  RCMARL_LAUNCH(k_policy_probs_wide, dim3(N, S), dim3(256), smem, stream, xs, theta, probs, N, in_dim, hid, ldp);
  return rcmarl_check_launch();
}

RCMARL_EXPORT int rcmarl_rollout_step_wide(const float* xs, const int* pos, const int* goal, const float* theta,
                                           const unsigned long long* seeds, int nrow, int ncol, const double* scale,
                                           float* rp_s, float* rp_ns, float* rp_sa, float* rp_a, float* rp_r, long cap,
                                           long row, int* pos_next, float* xs_next, double* ret, double gpow, int episode,
                                           int step, float mu, int S, int N, int hid, int n_actions, int ldp,
                                           int* act_out, void* stream) {
  if (!xs || !pos || !goal || !theta || !seeds || !scale || !rp_s || !rp_ns || !rp_sa || !rp_a || !rp_r ||
      !pos_next || !xs_next || !ret || row < 0 || row >= cap || S <= 0 || N <= 0 || hid <= 0 || (ldp & 63))
    return RCMARL_ERR_ARG;
  if (n_actions != 5) return RCMARL_ERR_UNSUPPORTED;
  const size_t smem = (size_t)(2 * hid + 8) * sizeof(float);
  if (smem > 64 * 1024) return RCMARL_ERR_UNSUPPORTED;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const Replay rp{rp_s, rp_ns, rp_sa, rp_a, rp_r, cap};
  RCMARL_LAUNCH(k_rollout_step_wide, dim3(N, S), dim3(256), smem, stream, xs, pos, goal, theta, seeds, cfg, rp, row, pos_next,
                xs_next, ret, gpow, episode, step, mu, N, 2 * N, hid, ldp, act_out);
  return rcmarl_check_launch();
}

// does the matrix-core kernel of rcmarl_rollout_step_episodes_wide serve this width?  (whole 32-unit tiles, a1 within the LDS)
RCMARL_EXPORT int rcmarl_rollout_wide_supported(int hid) { return hid > 0 && (hid & 31) == 0 && hid <= RW_MAX_HID ? 1 : 0; }

RCMARL_EXPORT int rcmarl_rollout_step_episodes_wide(const float* xsT, const int* posT, const int* goal, const float* theta,
                                                    const unsigned long long* seeds, int nrow, int ncol, const double* scale,
                                                    float* rp_s, float* rp_ns, float* rp_sa, float* rp_a, float* rp_r,
                                                    long cap, long row0, int ep_len, int* posT_next, float* xsT_next,
                                                    double* retT, double gpow, int episode0, int step, float mu, int S, int N,
                                                    int E, int EP, int hid, int n_actions, int ldp, void* stream) {
  if (!xsT || !posT || !goal || !theta || !seeds || !scale || !rp_s || !rp_ns || !rp_sa || !rp_a || !rp_r ||
      !posT_next || !xsT_next || !retT || row0 < 0 || E <= 0 || EP < E || (EP & 63) || ep_len <= 0 || step < 0 ||
      step >= ep_len || row0 + (long)E * ep_len > cap || S <= 0 || N <= 0 || hid <= 0 || (ldp & 63))
    return RCMARL_ERR_ARG;
  if (n_actions != 5 || !rcmarl_rollout_wide_supported(hid)) return RCMARL_ERR_UNSUPPORTED;
  const EnvCfg cfg{nrow, ncol, scale[0], scale[1], scale[2], scale[3]};
  const Replay rp{rp_s, rp_ns, rp_sa, rp_a, rp_r, cap};
  const size_t smem = rw_smem(hid);
  if (!rc_want_lds(k_rollout_step_ep_wide, smem, 48 * 1024)) return RCMARL_ERR_LAUNCH;
  const int f16 = (rc_lat_f16_mode() != 0 && rcmarl_wide_f16_mode() != 0) ? 1 : 0;
  RCMARL_LAUNCH(k_rollout_step_ep_wide, dim3(N, S, EP / 64), dim3(RW_THREADS), smem, stream, xsT, posT, goal, theta, seeds, cfg, rp,
                row0, ep_len, posT_next, xsT_next, retT, gpow, episode0, step, mu, N, E, EP, hid, ldp, f16, (float*)nullptr);
  return rcmarl_check_launch();
}

// probs[s][n][e][:] = actor_n(state of episode e), e < E, by the kernel of rcmarl_rollout_step_episodes_wide (same forward pass, no
// draw, no transition): what its sampled actions are drawn from
RCMARL_EXPORT int rcmarl_policy_probs_episodes_wide(const float* xsT, const float* theta, float* probs, int S, int N, int E, int EP,
                                                    int hid, int n_actions, int ldp, void* stream) {
  if (!xsT || !theta || !probs || S <= 0 || N <= 0 || E <= 0 || EP < E || (EP & 63) || hid <= 0 || (ldp & 63)) return RCMARL_ERR_ARG;
  if (n_actions != 5 || !rcmarl_rollout_wide_supported(hid)) return RCMARL_ERR_UNSUPPORTED;
  const size_t smem = rw_smem(hid);
  if (!rc_want_lds(k_rollout_step_ep_wide, smem, 48 * 1024)) return RCMARL_ERR_LAUNCH;
  const int f16 = (rc_lat_f16_mode() != 0 && rcmarl_wide_f16_mode() != 0) ? 1 : 0;
  const EnvCfg cfg{};
  const Replay rp{};
  RCMARL_LAUNCH(k_rollout_step_ep_wide, dim3(N, S, EP / 64), dim3(RW_THREADS), smem, stream, xsT, (const int*)nullptr,
                (const int*)nullptr, theta, (const unsigned long long*)nullptr, cfg, rp, 0L, 1, (int*)nullptr, (float*)nullptr,
                (double*)nullptr, 0.0, 0, 0, 0.f, N, E, EP, hid, ldp, f16, probs);
  return rcmarl_check_launch();
}
