// Native sliding-window n-step transition builder for an actor group (C ABI).
//
// Same semantics and emission order as the numpy NStepBuilder
// (apex_dqn_amd/actors/nstep.py, the test oracle), which replaces the reference
// ExperienceBuffer (actor.py:15-93) with the intended Ape-X rules: a transition
// every env step, R = sum_k gamma^k r_{t+k} once, Gamma = gamma^n (0 when the
// episode ended inside the window), partial windows flushed at episode end,
// unique int64 keys (env_id << 40 | seq), and the actor-side initial priority
// |R + Gamma * max_a q(S_{t+n}) - q(S_t, A_t)| computed when q(S_{t+n}) arrives
// one step later (actor.py:127-143 with defect A1 fixed).  Observations are
// opaque fixed-size byte payloads (frame sequence numbers for Atari, the state
// vector for CartPole).  The numpy version spends ~0.3 ms per step on 256 envs
// in Python-level indexing; this one is a few microseconds.
// Runtime.value_rescale (apex_rt_ns_set_rescale, eps > 0): the priorities are on the rescaled target's scale,
// |h(R + Gamma h^-1(max_a q(S_{t+n}))) - q| and |h(R) - q| on the terminal flush, h / h^-1 written operation by
// operation as learner/rescale.py writes them (fp64); the stored R stays raw.  eps = 0 is the code of before.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_runtime.h"

namespace {

struct NStep {
  int E, n, ob;  // envs, window, observation bytes
  double gamma, gamma_n;
  double rescale_eps = 0.0;          // > 0: Runtime.value_rescale_eps
  static double rs_h(double x, double eps) { return x / (std::sqrt(std::fabs(x) + 1.0) + 1.0) + eps * x; }
  static double rs_h_inv(double y, double eps) {
    const double ay = std::fabs(y);
    const double t = 2.0 * ay / (std::sqrt(1.0 + 4.0 * eps * (ay + 1.0 + eps)) + 1.0 + 2.0 * eps);
    const double sgn = (double)((y > 0.0) - (y < 0.0));
    return sgn * (t * (t + 2.0));
  }
  // the target of a transition's initial priority from the raw return and the bootstrap value
  double target(double R, double G, double qmax) const {
    if (rescale_eps > 0.0) return rs_h(R + G * rs_h_inv(qmax, rescale_eps), rescale_eps);
    return R + G * qmax;
  }
  double target_terminal(double R) const { return rescale_eps > 0.0 ? rs_h(R, rescale_eps) : R; }
  std::vector<uint8_t> w_obs;        // [E][n][ob]
  std::vector<int64_t> w_act;        // [E][n]
  std::vector<double> w_rew, w_qsa;  // [E][n]
  std::vector<int> cnt;              // [E]
  std::vector<uint8_t> p_valid;      // pending full-window transition per env
  std::vector<uint8_t> p_obs, p_next;
  std::vector<int64_t> p_act, p_key, seq, env_ids;
  std::vector<double> p_R, p_qsa, disc;
  // emitted, not yet taken (FIFO from `head`)
  std::vector<uint8_t> o_obs, o_nxt;
  std::vector<int64_t> o_act, o_key, o_env;
  std::vector<float> o_R, o_G, o_prio;
  size_t head = 0;

  int64_t key(int e) {
    const int64_t k = (env_ids[e] << 40) | (seq[e] & ((int64_t(1) << 40) - 1));
    seq[e] += 1;
    return k;
  }
  void emit(const uint8_t* obs, const uint8_t* nxt, int64_t act, double R, double G, double prio, int64_t k,
            int64_t env) {
    o_obs.insert(o_obs.end(), obs, obs + ob);
    o_nxt.insert(o_nxt.end(), nxt, nxt + ob);
    o_act.push_back(act);
    o_R.push_back((float)R);
    o_G.push_back((float)G);
    o_prio.push_back((float)prio);
    o_key.push_back(k);
    o_env.push_back(env);
  }
  size_t size() const { return o_act.size() - head; }
};

}  // namespace

APEX_RT_API void* apex_rt_ns_create(int E, int n, double gamma, int obs_bytes, int64_t env_id_offset) {
  if (E <= 0 || n <= 0 || obs_bytes <= 0) return nullptr;
  NStep* s = new NStep();
  s->E = E;
  s->n = n;
  s->ob = obs_bytes;
  s->gamma = gamma;
  s->gamma_n = std::pow(gamma, (double)n);
  s->w_obs.assign((size_t)E * n * obs_bytes, 0);
  s->w_act.assign((size_t)E * n, 0);
  s->w_rew.assign((size_t)E * n, 0.0);
  s->w_qsa.assign((size_t)E * n, 0.0);
  s->cnt.assign(E, 0);
  s->p_valid.assign(E, 0);
  s->p_obs.assign((size_t)E * obs_bytes, 0);
  s->p_next.assign((size_t)E * obs_bytes, 0);
  s->p_act.assign(E, 0);
  s->p_key.assign(E, 0);
  s->seq.assign(E, 0);
  s->env_ids.resize(E);
  for (int e = 0; e < E; ++e) s->env_ids[e] = e + env_id_offset;
  s->p_R.assign(E, 0.0);
  s->p_qsa.assign(E, 0.0);
  s->disc.resize(n);
  for (int k = 0; k < n; ++k) s->disc[k] = std::pow(gamma, (double)k);
  return s;
}

APEX_RT_API void apex_rt_ns_destroy(void* h) { delete static_cast<NStep*>(h); }

// eps of the rescaled target the priorities are measured against (0 = off); 1 when out of (0, 1]
APEX_RT_API int apex_rt_ns_set_rescale(void* h, double eps) {
  if (h == nullptr || !(eps >= 0.0 && eps <= 1.0)) return 1;
  static_cast<NStep*>(h)->rescale_eps = eps;
  return 0;
}

// One vectorised env step: obs / next_obs [E][obs_bytes], q [E][A] fp32,
// actions [E] int64, rewards [E] fp32, dones [E] uint8.
APEX_RT_API int apex_rt_ns_step(void* h, const void* obs_v, const float* q, int A, const int64_t* actions,
                                const float* rewards, const uint8_t* dones, const void* next_v) {
  NStep& s = *static_cast<NStep*>(h);
  const uint8_t* obs = static_cast<const uint8_t*>(obs_v);
  const uint8_t* nxt = static_cast<const uint8_t*>(next_v);
  const int E = s.E, n = s.n, ob = s.ob;
  for (int e = 0; e < E; ++e)
    if (actions[e] < 0 || actions[e] >= A) return 1;
  // 1) pending transitions complete: their bootstrap state is this step's S_t
  for (int e = 0; e < E; ++e) {
    if (!s.p_valid[e]) continue;
    double qmax = (double)q[(size_t)e * A];
    for (int a = 1; a < A; ++a) qmax = std::fmax(qmax, (double)q[(size_t)e * A + a]);
    const double target = s.target(s.p_R[e], s.gamma_n, qmax);
    s.emit(&s.p_obs[(size_t)e * ob], &s.p_next[(size_t)e * ob], s.p_act[e], s.p_R[e], s.gamma_n,
           std::fabs(target - s.p_qsa[e]), s.p_key[e], s.env_ids[e]);
    s.p_valid[e] = 0;
  }
  // 2) append step t to every window
  for (int e = 0; e < E; ++e) {
    const int c = s.cnt[e];
    const size_t w = (size_t)e * n + c;
    std::memcpy(&s.w_obs[w * ob], obs + (size_t)e * ob, ob);
    s.w_act[w] = actions[e];
    s.w_rew[w] = (double)rewards[e];
    s.w_qsa[w] = (double)q[(size_t)e * A + actions[e]];
    s.cnt[e] = c + 1;
  }
  // 3) terminal envs: every window entry becomes a terminal transition (Gamma 0)
  for (int e = 0; e < E; ++e) {
    if (!dones[e]) continue;
    const int m = s.cnt[e];
    const size_t w0 = (size_t)e * n;
    for (int j = 0; j < m; ++j) {
      double R = 0.0;
      for (int k = 0; k < m - j; ++k) R += s.disc[k] * s.w_rew[w0 + j + k];
      s.emit(&s.w_obs[(w0 + j) * ob], obs + (size_t)e * ob, s.w_act[w0 + j], R, 0.0,
             std::fabs(s.target_terminal(R) - s.w_qsa[w0 + j]), s.key(e), s.env_ids[e]);
    }
    s.cnt[e] = 0;
  }
  // 4) full non-terminal windows: the oldest entry waits for q(S_{t+n}); slide by one
  for (int e = 0; e < E; ++e) {
    if (dones[e] || s.cnt[e] != n) continue;
    const size_t w0 = (size_t)e * n;
    double R = 0.0;
    for (int k = 0; k < n; ++k) R += s.w_rew[w0 + k] * s.disc[k];
    s.p_valid[e] = 1;
    std::memcpy(&s.p_obs[(size_t)e * ob], &s.w_obs[w0 * ob], ob);
    std::memcpy(&s.p_next[(size_t)e * ob], nxt + (size_t)e * ob, ob);
    s.p_act[e] = s.w_act[w0];
    s.p_R[e] = R;
    s.p_qsa[e] = s.w_qsa[w0];
    s.p_key[e] = s.key(e);
    std::memmove(&s.w_obs[w0 * ob], &s.w_obs[(w0 + 1) * ob], (size_t)(n - 1) * ob);
    for (int k = 0; k + 1 < n; ++k) {
      s.w_act[w0 + k] = s.w_act[w0 + k + 1];
      s.w_rew[w0 + k] = s.w_rew[w0 + k + 1];
      s.w_qsa[w0 + k] = s.w_qsa[w0 + k + 1];
    }
    s.cnt[e] -= 1;
  }
  return 0;
}

APEX_RT_API int64_t apex_rt_ns_size(void* h) { return (int64_t) static_cast<NStep*>(h)->size(); }

// Pop up to `max_items` (all when < 0) emitted transitions, oldest first, into the
// caller's arrays; returns the count.
APEX_RT_API int64_t apex_rt_ns_take(void* h, int64_t max_items, void* obs, void* nxt, int64_t* act, float* R,
                                    float* G, float* prio, int64_t* key, int64_t* env) {
  NStep& s = *static_cast<NStep*>(h);
  int64_t k = (int64_t)s.size();
  if (max_items >= 0 && max_items < k) k = max_items;
  const size_t h0 = s.head, ob = (size_t)s.ob;
  std::memcpy(obs, &s.o_obs[h0 * ob], (size_t)k * ob);
  std::memcpy(nxt, &s.o_nxt[h0 * ob], (size_t)k * ob);
  std::memcpy(act, &s.o_act[h0], (size_t)k * sizeof(int64_t));
  std::memcpy(R, &s.o_R[h0], (size_t)k * sizeof(float));
  std::memcpy(G, &s.o_G[h0], (size_t)k * sizeof(float));
  std::memcpy(prio, &s.o_prio[h0], (size_t)k * sizeof(float));
  std::memcpy(key, &s.o_key[h0], (size_t)k * sizeof(int64_t));
  std::memcpy(env, &s.o_env[h0], (size_t)k * sizeof(int64_t));
  s.head += (size_t)k;
  if (s.head == s.o_act.size()) {  // drained: reuse the buffers
    s.head = 0;
    s.o_obs.clear(); s.o_nxt.clear(); s.o_act.clear(); s.o_R.clear(); s.o_G.clear(); s.o_prio.clear();
    s.o_key.clear(); s.o_env.clear();
  } else if (s.head >= 4096 && 2 * s.head >= s.o_act.size()) {  // partial takes: compact the front
    const size_t d = s.head;
    s.o_obs.erase(s.o_obs.begin(), s.o_obs.begin() + d * ob);
    s.o_nxt.erase(s.o_nxt.begin(), s.o_nxt.begin() + d * ob);
    s.o_act.erase(s.o_act.begin(), s.o_act.begin() + d);
    s.o_R.erase(s.o_R.begin(), s.o_R.begin() + d);
    s.o_G.erase(s.o_G.begin(), s.o_G.begin() + d);
    s.o_prio.erase(s.o_prio.begin(), s.o_prio.begin() + d);
    s.o_key.erase(s.o_key.begin(), s.o_key.begin() + d);
    s.o_env.erase(s.o_env.begin(), s.o_env.begin() + d);
    s.head = 0;
  }
  return k;
}
