// TEST INFRASTRUCTURE: the NUTS run-ahead helpers (stan4bart_amd/csrc/stan_host.hpp, Nuts::RunAhead) without any device layer, for a
// data-race check of the sampler's thread against its helper threads.  A HostModel with the default model family (two fixed coefficients,
// a grouping term with intercept and slope, a second one with intercepts: D = 26 unconstrained parameters) is evaluated over a synthetic
// dense Gram matrix; a Nuts sampler runs the same chain with 0, 1 and 2 helpers, the latter two also in the waiting mode (with "time": with the scalar and with the vector loops), and
// every row of every chain must equal the first chain's bit for bit.  tests/test_nuts_runahead.py builds this file with -fsanitize=thread and runs it
// as a child process; it is a plain program and reports through its exit status.
//   usage: nuts_runahead_race [transitions = 200] [time]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stan4bart_amd/csrc/stan_host.hpp"

namespace {

struct Gram {
  int K = 2, q = 18, M = 20, ld = 20;
  std::vector<double> G, cX, cZ; double s0 = 0;
};

// X: two columns; Z: (1 + x | g1) with 6 levels, (1 | g2) with 6 levels; a deterministic pseudo-random design (no generator state shared with
// the sampler)
Gram make_gram(int N) {
  Gram gr;
  gr.G.assign((size_t)gr.M * gr.ld, 0.0); gr.cX.assign((size_t)gr.K, 0.0); gr.cZ.assign((size_t)gr.q, 0.0);
  uint64_t s = 88172645463325252ull;
  auto unif = [&s] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
  std::vector<double> row((size_t)gr.M);
  for (int i = 0; i < N; ++i) {
    std::fill(row.begin(), row.end(), 0.0);
    const double x = unif(), z = unif() < 0.5 ? 0.0 : 1.0;
    const int g1 = (int)(unif() * 6) % 6, g2 = (int)(unif() * 6) % 6;
    row[0] = x; row[1] = z; row[(size_t)(2 + 2 * g1)] = 1.0; row[(size_t)(2 + 2 * g1 + 1)] = x; row[(size_t)(2 + 12 + g2)] = 1.0;
    const double y = 1.5 * x - 0.7 * z + 0.4 * (g1 - 2.5) + 0.3 * x * (g1 % 3) + 0.2 * (g2 - 2.5) + (unif() - 0.5);
    for (int a = 0; a < gr.M; ++a) {
      if (row[(size_t)a] == 0.0) continue;
      for (int b = 0; b < gr.M; ++b) gr.G[(size_t)a * gr.ld + b] += row[(size_t)a] * row[(size_t)b];
      (a < gr.K ? gr.cX[(size_t)a] : gr.cZ[(size_t)(a - gr.K)]) += row[(size_t)a] * y;
    }
    gr.s0 += y * y;
  }
  return gr;
}

s4b::StanSpec make_spec(int N) {
  s4b::StanSpec sp;
  sp.N = N; sp.K = 2; sp.q = 18; sp.t = 2; sp.len_theta_L = 4;
  sp.prior_dist = 1; sp.prior_scale = {2.5, 2.5}; sp.prior_mean = {0.0, 0.0}; sp.prior_df = {1.0, 1.0};
  sp.prior_dist_for_aux = 3; sp.prior_scale_for_aux = 1.0;
  sp.p = {2, 1}; sp.l = {6, 6}; sp.shape = {1.0, 1.0}; sp.scale = {1.0, 1.0}; sp.concentration = {1.0, 1.0}; sp.regularization = {1.0};
  return sp;
}

struct Chain { std::vector<double> rows; int64_t counters[4]; double seconds; long leapfrogs; };

Chain run_chain(const Gram& gr, int N, int transitions, int helpers, bool wait, int warmup, double stepsize, int maxDepth) {
  s4b::HostModel model(make_spec(N));
  model.lik = [&gr](const double* beta, const double* b, double* gX, double* gZ, double* th) {
    for (int k = 0; k < gr.K; ++k) th[k] = beta[k];
    for (int j = 0; j < gr.q; ++j) th[gr.K + j] = b[j];
    return s4b::hostloop::gram_dense(s4b::host_vector_on(), gr.G.data(), gr.ld, gr.M, gr.K, th, gr.cX.data(), gr.cZ.data(), gr.s0, gX, gZ);
  };
  if (!model.has_closed_form()) { std::fprintf(stderr, "the model has no closed-form gradient\n"); std::exit(2); }
  s4b::NutsControl nc; nc.seed = 4711; nc.stepsize = stepsize; nc.max_depth = maxDepth;
  s4b::Nuts nuts(model, nc, 1, warmup);
  nuts.set_helpers(helpers, wait); nuts.set_runahead_allowed(true);
  const int width = 7 + model.sp.n_constrained;
  Chain c; c.rows.assign((size_t)transitions * width, 0.0);
  for (int i = 0; i < warmup; ++i) nuts.run(c.rows.data());
  nuts.disengage();
  const auto t0 = std::chrono::steady_clock::now();
  c.leapfrogs = 0;
  for (int i = 0; i < transitions; ++i) { nuts.run(c.rows.data() + (size_t)i * width); c.leapfrogs += (long)c.rows[(size_t)i * width + 4]; }
  c.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  nuts.runahead_counters(c.counters);
  return c;
}

}  // namespace

int main(int argc, char** argv) {
  const int transitions = argc > 1 ? std::atoi(argv[1]) : 200;
  const bool timing = argc > 2 && std::strcmp(argv[2], "time") == 0;
  const int N = 600;
  const Gram gr = make_gram(N);
  int bad = 0;
  // (a process bound to one core gets no helper, whatever is asked for: the chains are compared all the same)
  bool room = true;
#if defined(__linux__)
  { cpu_set_t a, b; room = s4b::CpuNeighbours::helper_set(sched_getcpu(), &a, &b) != s4b::CpuNeighbours::NOWHERE; }
#endif
  // a short warm-up that adapts (deep trees afterwards); a large forced step with a tree depth of 3 (divergent transitions, the array's end)
  // (the race check limits the adapted chain's trees to depth 6, 63 leapfrogs: most transitions end at the limit with a helper still integrating;
  // the timing run lets them grow)
  struct Case { int warmup; double stepsize; int maxDepth; const char* name; } cases[] = {{60, 1.0, timing ? 10 : 6, "adapted"}, {0, 4.0, 3, "large step, depth 3"}};
  for (const Case& cs : cases) {
    Chain ref;
    bool have = false;
    // (timing: the scalar and the vector loops; otherwise the loops the process runs by default)
    const int vecLo = timing ? 0 : (s4b::host_vector_on() ? 1 : 0), vecHi = timing ? (s4b::host_vector_supported() ? 1 : 0) : vecLo;
    for (int vec = vecLo; vec <= vecHi; ++vec) {
      s4b::set_host_vector(vec);
      // helpers 0, 1, 2 as a sampler runs them (a state the helper has not finished is computed by the sampler's thread), then 1 and 2 with the
      // sampler's thread waiting for every state of a helper's direction
      for (int cfg = 0; cfg < 5; ++cfg) {
        const int helpers = cfg < 3 ? cfg : cfg - 2; const bool wait = cfg >= 3;
        Chain c = run_chain(gr, N, transitions, helpers, wait, cs.warmup, cs.stepsize, cs.maxDepth);
        if (!have) { ref = c; have = true; }
        const bool same = c.rows.size() == ref.rows.size() && std::memcmp(c.rows.data(), ref.rows.data(), c.rows.size() * sizeof(double)) == 0;
        const bool counted = (helpers == 0 || !room) ? (c.counters[0] == 0 && c.counters[3] > 0) : ((c.counters[0] > 0 || !wait) && c.counters[3] == 0);
        if (!same || !counted) ++bad;
        if (timing || !same || !counted)
          std::printf("%s: vector %d helpers %d%s: %ld leapfrogs, %.3f us each; taken %lld not ready %lld unconsumed %lld without %lld%s%s\n", cs.name, vec, helpers, wait ? " (waiting)" : "",
                      c.leapfrogs, 1e6 * c.seconds / (double)c.leapfrogs, (long long)c.counters[0], (long long)c.counters[1], (long long)c.counters[2],
                      (long long)c.counters[3], same ? "" : "  CHAIN DIFFERS", counted ? "" : "  COUNTERS WRONG");
      }
    }
  }
  if (bad) { std::printf("FAILED: %d chains\n", bad); return 1; }
  std::printf("ok\n");
  return 0;
}
