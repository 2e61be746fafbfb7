// C-ABI entry points of include/stan4bart_amd.h over a SamplerCore<S4B_DEV>.  Included once by the HIP
// translation unit (the product, prefix s4b_) and once by tests/emul (CPU emulation of the device layer,
// prefix emu_, test infrastructure only).  C++ exceptions never cross the boundary: they become a
// non-zero status + message, which the R shim turns into Rf_error (reference: Rf_error at
// src/init.cpp:319,367-382; exceptions are not caught there at all).
#include <memory>
#include <string>

struct s4b_sampler { s4b::SamplerCore<S4B_DEV> core; template <class... A> explicit s4b_sampler(A... a) : core(a...) {} };
struct s4b_sweep_group { std::unique_ptr<s4b::SweepGroup> g; };

namespace { thread_local std::string g_last_error; }

#define S4B_TRY try {
#define S4B_CATCH } catch (const std::exception& e) { g_last_error = e.what(); return 1; } catch (...) { g_last_error = "unknown error"; return 1; } return 0;
#define S4B_NEED(s, what) if (!(s)) { g_last_error = what " called on NULL sampler"; return 1; }

extern "C" {

const char* S4B_FN(last_error)(void) { return g_last_error.c_str(); }

int S4B_FN(create)(const s4b_bart_control* bc, const s4b_bart_data* bd, const s4b_stan_data* sd, const s4b_stan_control* sc,
                   const s4b_common_control* cc, const uint32_t* rstate, s4b_sampler** out) {
  S4B_TRY
  if (!out) throw std::invalid_argument("create: NULL output pointer");
  *out = new s4b_sampler(bc, bd, sd, sc, cc, rstate);
  S4B_CATCH
}
int S4B_FN(run)(s4b_sampler* s, int32_t num_iter, int32_t is_warmup, int32_t results_type, s4b_results* out) {
  S4B_NEED(s, "run") S4B_TRY s->core.dev().bind(); s4b::SamplerCore<S4B_DEV>::GroupRun inRun(s->core); s->core.run(num_iter, is_warmup != 0, results_type, out); S4B_CATCH
}
int S4B_FN(disengage_adaptation)(s4b_sampler* s) { S4B_NEED(s, "disengageAdaptation") S4B_TRY s->core.dev().bind(); s->core.disengage_adaptation(); S4B_CATCH }
int S4B_FN(print_initial_summary)(s4b_sampler* s) { S4B_NEED(s, "printInitialSummary") S4B_TRY s->core.dev().bind(); s->core.print_summary(); S4B_CATCH }
int S4B_FN(get_parametric_mean)(s4b_sampler* s, double* out) { S4B_NEED(s, "getParametricMean") S4B_TRY s->core.dev().bind(); s->core.parametric_mean(out); S4B_CATCH }
int S4B_FN(get_bart_data_range)(s4b_sampler* s, double out[2]) { S4B_NEED(s, "getBARTDataRange") S4B_TRY s->core.dev().bind(); s->core.data_range(out); S4B_CATCH }
int S4B_FN(get_r_rng_state)(s4b_sampler* s, uint32_t* st) { S4B_NEED(s, "get_r_rng_state") S4B_TRY s->core.dev().bind(); s->core.get_rng(st); S4B_CATCH }
int S4B_FN(set_r_rng_state)(s4b_sampler* s, const uint32_t* st) { S4B_NEED(s, "set_r_rng_state") S4B_TRY s->core.dev().bind(); s->core.set_rng(st); S4B_CATCH }
int S4B_FN(get_dims)(s4b_sampler* s, int64_t d[5]) { S4B_NEED(s, "get_dims") S4B_TRY s->core.dev().bind(); s->core.dims(d); S4B_CATCH }
int S4B_FN(get_stan_par_names)(s4b_sampler* s, char* buf, size_t cap) {
  S4B_NEED(s, "get_stan_par_names") S4B_TRY
  s->core.dev().bind();
  std::string o = s->core.par_names();
  if (o.size() + 1 > cap) throw std::invalid_argument("name buffer too small");
  std::memcpy(buf, o.c_str(), o.size() + 1);
  S4B_CATCH
}
int S4B_FN(get_trees)(s4b_sampler* s, int64_t cap, int32_t* tree, int32_t* n_obs, int32_t* var, int32_t* split, double* value, int64_t* num_nodes) {
  S4B_NEED(s, "getTrees") S4B_TRY s->core.dev().bind(); *num_nodes = s->core.get_trees(cap, tree, n_obs, var, split, value); S4B_CATCH
}
int S4B_FN(get_kept_trees)(s4b_sampler* s, int64_t sample, int64_t cap, int32_t* smp, int32_t* tree, int32_t* n_obs, int32_t* var, int32_t* split, double* value,
                            int64_t* num_nodes) {
  S4B_NEED(s, "getTrees") S4B_TRY s->core.dev().bind(); *num_nodes = s->core.get_kept_trees(sample, cap, smp, tree, n_obs, var, split, value); S4B_CATCH
}
int S4B_FN(get_kept_trees_indexed)(s4b_sampler* s, const int32_t* sidx, int64_t ns, const int32_t* tidx, int64_t nt, int64_t cap, int32_t* smp, int32_t* tree,
                                   int32_t* n_obs, int32_t* var, int32_t* split, double* value, int64_t* num_nodes) {
  S4B_NEED(s, "getTrees") S4B_TRY s->core.dev().bind(); *num_nodes = s->core.get_kept_trees_indexed(sidx, ns, tidx, nt, cap, smp, tree, n_obs, var, split, value); S4B_CATCH
}
int S4B_FN(print_trees)(s4b_sampler* s, const int32_t* sidx, int64_t ns, const int32_t* tidx, int64_t nt) {
  S4B_NEED(s, "printTrees") S4B_TRY s->core.print_trees(sidx, ns, tidx, nt); S4B_CATCH
}
int S4B_FN(set_progress)(s4b_sampler* s, s4b_progress_fn fn, void* user) { S4B_NEED(s, "set_progress") S4B_TRY s->core.set_progress(fn, user); S4B_CATCH }
int S4B_FN(predict_bart_offset)(s4b_sampler* s, const double* x_test, int64_t n_test, const double* offset_test, double* out, int64_t* num_samples) {
  S4B_NEED(s, "predictBART") S4B_TRY s->core.dev().bind(); *num_samples = s->core.predict(x_test, n_test, out, offset_test); S4B_CATCH
}
int S4B_FN(predict_bart)(s4b_sampler* s, const double* x_test, int64_t n_test, double* out, int64_t* num_samples) {
  S4B_NEED(s, "predictBART") S4B_TRY s->core.dev().bind(); *num_samples = s->core.predict(x_test, n_test, out); S4B_CATCH
}
int S4B_FN(predict_summary)(s4b_sampler* s, const s4b_summary_in* in, s4b_summary_out* out) {
  S4B_NEED(s, "predict_summary") S4B_TRY s->core.dev().bind(); s->core.predict_summary(in, out); S4B_CATCH
}
int S4B_FN(partial_dependence)(s4b_sampler* s, const s4b_pd_in* in, s4b_pd_out* out) {
  S4B_NEED(s, "partial_dependence") S4B_TRY s->core.dev().bind(); s->core.partial_dependence(in, out); S4B_CATCH
}
int S4B_FN(predict_quantiles)(s4b_sampler* s, const s4b_quantile_in* in, s4b_quantile_out* out) {
  S4B_NEED(s, "predict_quantiles") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && out->quantiles && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_quantiles(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_contrast)(s4b_sampler* s, const s4b_contrast_in* in, s4b_contrast_out* out) {
  S4B_NEED(s, "predict_contrast") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_contrast(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_groups)(s4b_sampler* s, const s4b_groups_in* in, s4b_groups_out* out) {
  S4B_NEED(s, "predict_groups") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->arms.n_peers > 0 && in->arms.peers) for (int x = 0; x < in->arms.n_peers; ++x) peers.push_back(in->arms.peers[x] ? &in->arms.peers[x]->core : nullptr);
  s->core.predict_groups(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_projection)(s4b_sampler* s, const s4b_projection_in* in, s4b_projection_out* out) {
  S4B_NEED(s, "predict_projection") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->arms.n_peers > 0 && in->arms.peers) for (int x = 0; x < in->arms.n_peers; ++x) peers.push_back(in->arms.peers[x] ? &in->arms.peers[x]->core : nullptr);
  s->core.predict_projection(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_spread)(s4b_sampler* s, const s4b_spread_in* in, s4b_spread_out* out) {
  S4B_NEED(s, "predict_spread") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->arms.n_peers > 0 && in->arms.peers) for (int x = 0; x < in->arms.n_peers; ++x) peers.push_back(in->arms.peers[x] ? &in->arms.peers[x]->core : nullptr);
  s->core.predict_spread(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_check)(s4b_sampler* s, const s4b_check_in* in, s4b_check_out* out) {
  S4B_NEED(s, "predict_check") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_check(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_curves)(s4b_sampler* s, const s4b_curves_in* in, s4b_curves_out* out) {
  S4B_NEED(s, "predict_curves") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_curves(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_describe)(s4b_sampler* s, const s4b_describe_in* in, s4b_describe_out* out) {
  S4B_NEED(s, "predict_describe") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->arms.n_peers > 0 && in->arms.peers) for (int x = 0; x < in->arms.n_peers; ++x) peers.push_back(in->arms.peers[x] ? &in->arms.peers[x]->core : nullptr);
  s->core.predict_describe(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_sorted)(s4b_sampler* s, const s4b_sorted_in* in, s4b_sorted_out* out) {
  S4B_NEED(s, "predict_sorted") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->arms.n_peers > 0 && in->arms.peers) for (int x = 0; x < in->arms.n_peers; ++x) peers.push_back(in->arms.peers[x] ? &in->arms.peers[x]->core : nullptr);
  s->core.predict_sorted(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_ppd)(s4b_sampler* s, const s4b_ppd_in* in, s4b_ppd_out* out) {
  S4B_NEED(s, "predict_ppd") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_ppd(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_loo)(s4b_sampler* s, const s4b_loo_in* in, s4b_loo_out* out) {
  S4B_NEED(s, "predict_loo") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_loo(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(predict_convergence)(s4b_sampler* s, const s4b_conv_in* in, s4b_conv_out* out) {
  S4B_NEED(s, "predict_convergence") S4B_TRY
  s->core.dev().bind();
  std::vector<const s4b::SamplerCore<S4B_DEV>*> peers;          // (a NULL handle stays NULL: the core refuses it by its position)
  if (in && out && in->n_peers > 0 && in->peers) for (int x = 0; x < in->n_peers; ++x) peers.push_back(in->peers[x] ? &in->peers[x]->core : nullptr);
  s->core.predict_convergence(in, out, peers.empty() ? nullptr : peers.data());
  S4B_CATCH
}
int S4B_FN(export_bart_state)(s4b_sampler* s, void* buf, int64_t cap, int64_t* size) {
  S4B_NEED(s, "exportBARTState") S4B_TRY s->core.dev().bind(); if (!size) throw std::invalid_argument("exportBARTState: NULL size pointer"); *size = s->core.export_state(buf, cap); S4B_CATCH
}
int S4B_FN(create_stored_bart_sampler)(const void* state, int64_t size, int32_t device, s4b_sampler** out) {
  S4B_TRY
  if (!out) throw std::invalid_argument("createStoredBARTSampler: NULL output pointer");
  *out = new s4b_sampler(state, size, (int)device);
  S4B_CATCH
}
int S4B_FN(get_state)(s4b_sampler* s, void* buf, int64_t cap, int64_t* size) {
  S4B_NEED(s, "get_state") S4B_TRY s->core.dev().bind(); if (!size) throw std::invalid_argument("get_state: NULL size pointer"); *size = s->core.get_state(buf, cap); S4B_CATCH
}
int S4B_FN(set_state)(s4b_sampler* s, const void* buf, int64_t size) { S4B_NEED(s, "set_state") S4B_TRY s->core.dev().bind(); s->core.set_state(buf, size); S4B_CATCH }
int S4B_FN(set_trace)(s4b_sampler* s, int32_t enable) { S4B_NEED(s, "set_trace") S4B_TRY s->core.dev().bind(); s->core.set_trace(enable != 0); S4B_CATCH }
int S4B_FN(get_trace)(s4b_sampler* s, int64_t cap, int32_t* out, int64_t* num) { S4B_NEED(s, "get_trace") S4B_TRY s->core.dev().bind(); *num = s->core.get_trace(cap, out); S4B_CATCH }
int S4B_FN(get_leaf_assignment)(s4b_sampler* s, int32_t t, int32_t* out) { S4B_NEED(s, "get_leaf_assignment") S4B_TRY s->core.dev().bind(); s->core.leaf_assignment(t, out); S4B_CATCH }
int S4B_FN(set_device_sharing)(s4b_sampler* s, int32_t chains) { S4B_NEED(s, "set_device_sharing") S4B_TRY s->core.dev().bind(); s->core.set_device_sharing(chains); S4B_CATCH }
int S4B_FN(set_tree_path)(s4b_sampler* s, int32_t path) { S4B_NEED(s, "set_tree_path") S4B_TRY s->core.dev().bind(); s->core.dev().set_tree_path(path); S4B_CATCH }
int S4B_FN(get_tree_path)(s4b_sampler* s, int32_t out[2]) { S4B_NEED(s, "get_tree_path") S4B_TRY if (!out) throw std::invalid_argument("get_tree_path: NULL output pointer"); s->core.dev().get_tree_path(out); S4B_CATCH }
int S4B_FN(set_hmc_mode)(s4b_sampler* s, int32_t mode) { S4B_NEED(s, "set_hmc_mode") S4B_TRY s->core.set_hmc_mode(mode); S4B_CATCH }
int S4B_FN(get_hmc_mode)(s4b_sampler* s, int32_t* mode) { S4B_NEED(s, "get_hmc_mode") S4B_TRY if (!mode) throw std::invalid_argument("get_hmc_mode: NULL output pointer"); *mode = s->core.hmc_mode(); S4B_CATCH }
int S4B_FN(set_latent_mode)(s4b_sampler* s, int32_t mode) { S4B_NEED(s, "set_latent_mode") S4B_TRY s->core.dev().bind(); s->core.set_latent_mode(mode); S4B_CATCH }
int S4B_FN(get_latent_mode)(s4b_sampler* s, int32_t* mode) { S4B_NEED(s, "get_latent_mode") S4B_TRY if (!mode) throw std::invalid_argument("get_latent_mode: NULL output pointer"); *mode = s->core.latent_mode(); S4B_CATCH }
int S4B_FN(get_fused_stats)(s4b_sampler* s, int64_t out[2]) { S4B_NEED(s, "get_fused_stats") S4B_TRY if (!out) throw std::invalid_argument("get_fused_stats: NULL output pointer"); s->core.dev().fused_stats(out); S4B_CATCH }
int S4B_FN(get_sweep_stats)(s4b_sampler* s, int64_t out[2]) { S4B_NEED(s, "get_sweep_stats") S4B_TRY if (!out) throw std::invalid_argument("get_sweep_stats: NULL output pointer"); s->core.dev().sweep_stats(out); S4B_CATCH }
int S4B_FN(get_sweep_spec)(s4b_sampler* s, int64_t out[4]) { S4B_NEED(s, "get_sweep_spec") S4B_TRY if (!out) throw std::invalid_argument("get_sweep_spec: NULL output pointer"); s->core.dev().sweep_spec(out); S4B_CATCH }
int S4B_FN(set_test_hook)(s4b_sampler* s, int32_t hook, int64_t value) { S4B_NEED(s, "set_test_hook") S4B_TRY s->core.dev().set_test_hook(hook, value); S4B_CATCH }
int S4B_FN(test_draw_latents)(s4b_sampler* s) { S4B_NEED(s, "test_draw_latents") S4B_TRY s->core.dev().bind(); s->core.test_draw_latents(); S4B_CATCH }
int S4B_FN(test_hand_off)(s4b_sampler* s, const double* beta, const double* b, double sigma, int32_t update_scale) {
  S4B_NEED(s, "test_hand_off") S4B_TRY s->core.dev().bind(); s->core.test_hand_off(beta, b, sigma, update_scale != 0); S4B_CATCH
}
int S4B_FN(test_stan_sums)(s4b_sampler* s, int32_t mode, const double* beta, const double* b, const int32_t* set_exp, double* sums, int64_t* info) {
  S4B_NEED(s, "test_stan_sums") S4B_TRY s->core.dev().bind(); s->core.test_stan_sums(mode, beta, b, set_exp, sums, info); S4B_CATCH
}
int S4B_FN(test_sorted_select)(s4b_sampler* s, const double* values, int64_t n, int64_t S, int64_t block_draws, int32_t n_ranks, const int32_t* ranks,
                               double* order_stats, int32_t n_cuts, const int32_t* cut_rank, int32_t* n_above, int32_t* n_below, int64_t* info) {
  S4B_NEED(s, "test_sorted_select") S4B_TRY s->core.dev().bind();
  s->core.test_sorted_select(values, n, S, block_draws, n_ranks, ranks, order_stats, n_cuts, cut_rank, n_above, n_below, info); S4B_CATCH
}
int S4B_FN(get_sweep_busy)(s4b_sampler* s, int64_t* out) { S4B_NEED(s, "get_sweep_busy") S4B_TRY if (!out) throw std::invalid_argument("get_sweep_busy: NULL output pointer"); *out = s->core.dev().sweep_busy(); S4B_CATCH }
int S4B_FN(get_counters)(s4b_sampler* s, int64_t out[3]) { S4B_NEED(s, "get_counters") S4B_TRY s->core.dev().bind(); s->core.counters(out); S4B_CATCH }
int S4B_FN(get_nuts_stats)(s4b_sampler* s, double out[4]) { S4B_NEED(s, "get_nuts_stats") S4B_TRY s->core.dev().bind(); s->core.nuts_stats(out); S4B_CATCH }
int S4B_FN(set_nuts_helpers)(s4b_sampler* s, int32_t n) { S4B_NEED(s, "set_nuts_helpers") S4B_TRY s->core.set_nuts_helpers(n); S4B_CATCH }
int S4B_FN(get_nuts_runahead)(s4b_sampler* s, int64_t out[4]) { S4B_NEED(s, "get_nuts_runahead") S4B_TRY if (!out) throw std::invalid_argument("get_nuts_runahead: NULL output pointer"); s->core.nuts_runahead(out); S4B_CATCH }
int S4B_FN(set_host_vector)(int32_t on, int32_t* effective) { S4B_TRY const int v = on < 0 ? (s4b::host_vector_on() ? 1 : 0) : s4b::set_host_vector(on); if (effective) *effective = v; S4B_CATCH }
int S4B_FN(profile_sweep)(s4b_sampler* s, int32_t n_sweeps, double out[8]) { S4B_NEED(s, "profile_sweep") S4B_TRY s->core.dev().bind(); s->core.profile_sweep(n_sweeps, out); S4B_CATCH }
int S4B_FN(profile_leapfrog)(s4b_sampler* s, int32_t n_evals, double out[8]) { S4B_NEED(s, "profile_leapfrog") S4B_TRY s->core.dev().bind(); s->core.profile_leapfrog(n_evals, out); S4B_CATCH }
int S4B_FN(stream_probe)(int32_t device, int64_t n_doubles, int32_t reps, double out[4]) { S4B_TRY S4B_DEV::probe_stream(device, n_doubles, reps, out); S4B_CATCH }
void S4B_FN(free)(s4b_sampler* s) { if (s) { try { s->core.leave_group(); } catch (...) {} } delete s; }

// sweep groups (sweep_group.hpp): SamplerCore makes the group — the device layer's batched launch or the host one — and is the members' side of it
int S4B_FN(sweep_group_create)(int32_t device, int32_t max_members, s4b_sweep_group** out) {
  S4B_TRY
  if (!out) throw std::invalid_argument("sweep_group_create: NULL output pointer");
  *out = new s4b_sweep_group{std::unique_ptr<s4b::SweepGroup>(s4b::SamplerCore<S4B_DEV>::make_group((int)device, (int)max_members))};
  S4B_CATCH
}
int S4B_FN(sweep_group_join)(s4b_sweep_group* g, s4b_sampler* s) {
  S4B_NEED(s, "sweep_group_join") S4B_TRY if (!g) throw std::invalid_argument("sweep_group_join: NULL group"); s->core.join_group(g->g.get()); S4B_CATCH
}
int S4B_FN(sweep_group_leave)(s4b_sampler* s) { S4B_NEED(s, "sweep_group_leave") S4B_TRY s->core.leave_group(); S4B_CATCH }
int S4B_FN(sweep_group_stats)(s4b_sweep_group* g, int64_t out[4]) {
  S4B_TRY if (!g || !out) throw std::invalid_argument("sweep_group_stats: NULL argument"); g->g->stats(out); S4B_CATCH
}
int S4B_FN(sweep_group_set_timeout)(s4b_sweep_group* g, double seconds) {
  S4B_TRY if (!g) throw std::invalid_argument("sweep_group_set_timeout: NULL group"); g->g->set_timeout(seconds); S4B_CATCH
}
int S4B_FN(sweep_group_free)(s4b_sweep_group* g) {
  S4B_TRY
  if (!g) return 0;
  if (g->g->members() != 0) throw std::invalid_argument("sweep_group_free: samplers are still joined (s4b_sweep_group_leave / s4b_free them first)");
  delete g;
  S4B_CATCH
}

}  // extern "C"
