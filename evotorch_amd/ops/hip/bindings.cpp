// Python bindings for the gfx950 kernel extension `evotorch_amd._C`.
#include <torch/extension.h>

namespace ea {
void sample_gaussian(torch::Tensor out, torch::Tensor mu, torch::Tensor sigma, bool symmetric, int64_t seed, int64_t row_offset);
void sample_gaussian_graphsafe(torch::Tensor out, torch::Tensor mu, torch::Tensor sigma, bool symmetric,
                               torch::Tensor seed_buf);
void affine_from_noise(torch::Tensor out, torch::Tensor z, torch::Tensor mu, torch::Tensor sigma, bool symmetric);
std::vector<torch::Tensor> es_gradients(torch::Tensor samples, torch::Tensor mu, torch::Tensor sigma,
                                        torch::Tensor weights, bool symmetric);
std::vector<torch::Tensor> snes_gradients(torch::Tensor samples, torch::Tensor mu, torch::Tensor sigma,
                                          torch::Tensor weights);
void clipup_step(torch::Tensor velocity, torch::Tensor grad, double step_size, double max_speed, double momentum);
std::vector<torch::Tensor> gaussian_clipup_update(torch::Tensor mu, torch::Tensor sigma, torch::Tensor velocity,
                                                  torch::Tensor mu_grad, torch::Tensor sigma_grad, double step_size,
                                                  double momentum, double max_speed, double sigma_lr,
                                                  c10::optional<double> stdev_min, c10::optional<double> stdev_max,
                                                  c10::optional<double> stdev_max_change, double mu_grad_scale,
                                                  double sigma_grad_scale);
int64_t gaussian_clipup_update_max_length();
void obsnorm_pack(torch::Tensor count, torch::Tensor sum, torch::Tensor sumsq, double min_variance,
                  torch::Tensor blob, int64_t offset);
void obsnorm_merge(torch::Tensor count, torch::Tensor sum, torch::Tensor sumsq, double c_host,
                   c10::optional<torch::Tensor> c_device, torch::Tensor s, torch::Tensor ss);
void adam_step(torch::Tensor step_out, torch::Tensor grad, torch::Tensor m, torch::Tensor v, int64_t step_count,
               double stepsize, double beta1, double beta2, double epsilon);
void adam_step_graphsafe(torch::Tensor step_out, torch::Tensor grad, torch::Tensor m, torch::Tensor v,
                         torch::Tensor t_buf, double stepsize, double beta1, double beta2, double epsilon);
torch::Tensor population_mlp_forward(torch::Tensor params, torch::Tensor obs, std::vector<int64_t> widths,
                                     std::vector<int64_t> activations, bool has_bias);
torch::Tensor population_mlp_forward_shared(torch::Tensor params, torch::Tensor x, std::vector<int64_t> widths,
                                            std::vector<int64_t> activations, bool has_bias);
int64_t population_mlp_forward_shared_batch_tile(std::vector<int64_t> widths);
torch::Tensor population_mlp_forward_shared_bf16(torch::Tensor params, torch::Tensor x, std::vector<int64_t> widths,
                                                 std::vector<int64_t> activations, bool has_bias,
                                                 int64_t batch_tile);
int64_t population_mlp_forward_shared_bf16_batch_tile(std::vector<int64_t> widths);
torch::Tensor population_mlp_loss_shared(torch::Tensor params, torch::Tensor x, torch::Tensor y,
                                         std::vector<int64_t> widths, std::vector<int64_t> activations, bool has_bias,
                                         int64_t loss_kind, bool bf16);
int64_t population_mlp_loss_shared_batch_tile(std::vector<int64_t> widths, bool bf16);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> population_recurrent_forward(
    torch::Tensor params, torch::Tensor obs, c10::optional<torch::Tensor> h, c10::optional<torch::Tensor> c,
    std::vector<int64_t> kinds, std::vector<int64_t> widths, std::vector<int64_t> activations, bool has_bias);
torch::Tensor rollout_linear(torch::Tensor params, torch::Tensor env_blob, torch::Tensor obs_stats_out,
                             int64_t obs_dim, int64_t act_dim, int64_t rank, int64_t steps, double alive_bonus,
                             double act_cost, int64_t init_seed, int64_t member_offset, int64_t policy_hidden,
                             c10::optional<torch::Tensor> seed_buf, c10::optional<torch::Tensor> env_image,
                             c10::optional<torch::Tensor> fitness_out, bool overwrite_stats);
torch::Tensor rollout_env_image_v7(torch::Tensor env_blob, int64_t obs_dim, int64_t act_dim, int64_t rank);
torch::Tensor rollout_terminating(torch::Tensor params, torch::Tensor env_blob, torch::Tensor obs_stats_out,
                                  torch::Tensor steps_out, int64_t obs_dim, int64_t act_dim, int64_t rank,
                                  int64_t steps, double alive_bonus, double act_cost, int64_t init_seed,
                                  int64_t member_offset, int64_t policy_hidden, int64_t health_index,
                                  double healthy_lo, double healthy_hi, c10::optional<torch::Tensor> seed_buf,
                                  c10::optional<torch::Tensor> env_image, c10::optional<torch::Tensor> fitness_out,
                                  bool overwrite_stats);
std::string rollout_kernel_name(int64_t obs_dim, int64_t act_dim, int64_t rank, int64_t policy_hidden,
                                bool terminating);
void bump_seed(torch::Tensor seed_buf);
void cma_update_c(torch::Tensor C, torch::Tensor Y, torch::Tensor w, torch::Tensor pc, torch::Tensor hs_f,
                  torch::Tensor wsum, double c1, double cmu, double cc);
void potrf_tile(torch::Tensor A, torch::Tensor info);
torch::Tensor fused_rank(torch::Tensor fitnesses, int64_t method, bool higher_better);
torch::Tensor nanmean_1d(torch::Tensor x);
int64_t nanmean_1d_max_length();
torch::Tensor domination_counts(torch::Tensor utils);
torch::Tensor pareto_ranks(torch::Tensor utils, int64_t min_assigned);
std::vector<torch::Tensor> mapelites_assign(torch::Tensor grid, torch::Tensor feats, torch::Tensor utils);
}  // namespace ea

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "evotorch_amd gfx950 (MI355X / CDNA4) HIP kernels";
    m.def("sample_gaussian", &ea::sample_gaussian, "K1: philox Gaussian population sampling (plain/antithetic)",
          py::arg("out"), py::arg("mu"), py::arg("sigma"), py::arg("symmetric"), py::arg("seed"),
          py::arg("row_offset") = 0);
    m.def("sample_gaussian_graphsafe", &ea::sample_gaussian_graphsafe,
          "K1 (hipGraph-safe): seed read from and advanced in device memory");
    m.def("affine_from_noise", &ea::affine_from_noise,
          "K1 overlap: mu + sigma*z from pre-generated side-stream noise");
    m.def("es_gradients", &ea::es_gradients, "K3: fused (mu, sigma) ES gradient reduction");
    m.def("snes_gradients", &ea::snes_gradients, "K3: SNES raw-noise gradient reduction");
    m.def("clipup_step", &ea::clipup_step, "K4: fused ClipUp velocity update (no host sync)");
    m.def("gaussian_clipup_update", &ea::gaussian_clipup_update,
          "K4b: ClipUp step, mu + velocity and the bounded sigma step in one launch; returns (new_mu, new_sigma)",
          py::arg("mu"), py::arg("sigma"), py::arg("velocity"), py::arg("mu_grad"), py::arg("sigma_grad"),
          py::arg("step_size"), py::arg("momentum"), py::arg("max_speed"), py::arg("sigma_lr"),
          py::arg("stdev_min") = c10::optional<double>(), py::arg("stdev_max") = c10::optional<double>(),
          py::arg("stdev_max_change") = c10::optional<double>(), py::arg("mu_grad_scale") = 1.0,
          py::arg("sigma_grad_scale") = 1.0);
    m.def("gaussian_clipup_update_max_length", &ea::gaussian_clipup_update_max_length,
          "largest solution length gaussian_clipup_update accepts");
    m.def("obsnorm_pack", &ea::obsnorm_pack,
          "K12: obs-norm mean/stdev from (count, sum, sumsq), written into blob[offset : offset + 2*O]");
    m.def("obsnorm_merge", &ea::obsnorm_merge,
          "K12: count += c; sum += s; sumsq += ss in one launch (c: host value, or a 0-dim device tensor)");
    m.def("adam_step", &ea::adam_step, "K4: fused Adam ascent step");
    m.def("adam_step_graphsafe", &ea::adam_step_graphsafe,
          "K4 (hipGraph-safe): Adam with device-side step counter");
    m.def("population_mlp_forward", &ea::population_mlp_forward,
          "K13: forward of a dense policy stack (1-4 Linear layers; activation codes 0 identity, 1 tanh, 2 ReLU) for "
          "every member's own flat parameter vector; fp32, returns [n, widths[-1]]",
          py::arg("params"), py::arg("obs"), py::arg("widths"), py::arg("activations"), py::arg("has_bias"));
    m.def("population_mlp_forward_shared", &ea::population_mlp_forward_shared,
          "K14: forward of a dense stack (as K13 describes it) for every member's own flat parameter vector on ONE "
          "shared minibatch x [B, widths[0]], on fp32 MFMA; fp32, returns [n, B, widths[-1]]",
          py::arg("params"), py::arg("x"), py::arg("widths"), py::arg("activations"), py::arg("has_bias"));
    m.def("population_mlp_forward_shared_batch_tile", &ea::population_mlp_forward_shared_batch_tile,
          "K14: rows per batch tile (16, 32 or 64) the kernel takes for these widths (host only)", py::arg("widths"));
    m.def("population_mlp_forward_shared_bf16", &ea::population_mlp_forward_shared_bf16,
          "K15: K14's forward with weights, x and hidden activations rounded to bf16, on bf16 MFMA with fp32 sums, "
          "bias and activation; fp32 in and out, returns [n, B, widths[-1]]. batch_tile 0 takes the kernel's own "
          "rule, 32 or 64 overrides it (for measuring)",
          py::arg("params"), py::arg("x"), py::arg("widths"), py::arg("activations"), py::arg("has_bias"),
          py::arg("batch_tile") = 0);
    m.def("population_mlp_forward_shared_bf16_batch_tile", &ea::population_mlp_forward_shared_bf16_batch_tile,
          "K15: rows per batch tile (32 or 64) the kernel takes for these widths (host only)", py::arg("widths"));
    m.def("population_mlp_loss_shared", &ea::population_mlp_loss_shared,
          "K17: K14's (or with bf16, K15's) forward on the shared minibatch x [B, widths[0]] with the mean loss fused "
          "into the last epilogue: loss_kind 0 is MSE against y fp32 [B, widths[-1]], 1 is cross-entropy against "
          "y int64 [B] (targets of -100 are ignored, as torch's default); fp32, returns [n]",
          py::arg("params"), py::arg("x"), py::arg("y"), py::arg("widths"), py::arg("activations"),
          py::arg("has_bias"), py::arg("loss_kind"), py::arg("bf16") = false);
    m.def("population_mlp_loss_shared_batch_tile", &ea::population_mlp_loss_shared_batch_tile,
          "K17: rows per batch tile the loss kernel takes for these widths (host only)", py::arg("widths"),
          py::arg("bf16") = false);
    m.def("population_recurrent_forward", &ea::population_recurrent_forward,
          "K16: one step of a stack of 1-4 weighted layers (kinds 0 dense, 1 RNN, 2 LSTM; exactly one recurrent) for "
          "every member's own flat parameter vector and state; h (and c for an LSTM) may be None for no state yet; "
          "fp32, returns (out [n, widths[-1]], new_h [n, H], new_c [n, H] or empty)",
          py::arg("params"), py::arg("obs"), py::arg("h"), py::arg("c"), py::arg("kinds"), py::arg("widths"),
          py::arg("activations"), py::arg("has_bias"));
    // Both rollout entry points take `obs_stats_out` either as one tensor, to
    // which the summed statistics are ADDED and a fresh fitness tensor is
    // returned, or as a pair (obs_stats_out, fitness_out) of plain outputs:
    // the statistics are then reduced straight into the first (no fill, no
    // add) and the kernels store the fitnesses into the second, which is
    // returned. Every other operand keeps its place.
    using OutPair = std::tuple<torch::Tensor, torch::Tensor>;
    m.def("rollout_linear",
          [](torch::Tensor params, torch::Tensor env_blob, torch::Tensor obs_stats_out, int64_t obs_dim,
             int64_t act_dim, int64_t rank, int64_t steps, double alive_bonus, double act_cost, int64_t init_seed,
             int64_t member_offset, int64_t policy_hidden, c10::optional<torch::Tensor> seed_buf,
             c10::optional<torch::Tensor> env_image) {
              return ea::rollout_linear(params, env_blob, obs_stats_out, obs_dim, act_dim, rank, steps, alive_bonus,
                                        act_cost, init_seed, member_offset, policy_hidden, seed_buf, env_image,
                                        c10::nullopt, false);
          },
          "K10+K11: fused policy episode rollout (linear or MLP-H, synthetic env)",
          pybind11::arg("params"), pybind11::arg("env_blob"), pybind11::arg("obs_stats_out"),
          pybind11::arg("obs_dim"), pybind11::arg("act_dim"), pybind11::arg("rank"), pybind11::arg("steps"),
          pybind11::arg("alive_bonus"), pybind11::arg("act_cost"), pybind11::arg("init_seed"),
          pybind11::arg("member_offset"), pybind11::arg("policy_hidden") = 0,
          pybind11::arg("seed_buf") = c10::optional<torch::Tensor>(),
          pybind11::arg("env_image") = c10::optional<torch::Tensor>());
    m.def("rollout_linear",
          [](torch::Tensor params, torch::Tensor env_blob, OutPair outputs, int64_t obs_dim, int64_t act_dim,
             int64_t rank, int64_t steps, double alive_bonus, double act_cost, int64_t init_seed,
             int64_t member_offset, int64_t policy_hidden, c10::optional<torch::Tensor> seed_buf,
             c10::optional<torch::Tensor> env_image) {
              return ea::rollout_linear(params, env_blob, std::get<0>(outputs), obs_dim, act_dim, rank, steps,
                                        alive_bonus, act_cost, init_seed, member_offset, policy_hidden, seed_buf,
                                        env_image, std::get<1>(outputs), true);
          },
          "rollout_linear writing into the pair (obs_stats_out, fitness_out): statistics overwritten, not added; "
          "fitness_out fp32, dense, exactly n elements, and returned",
          pybind11::arg("params"), pybind11::arg("env_blob"), pybind11::arg("outputs"), pybind11::arg("obs_dim"),
          pybind11::arg("act_dim"), pybind11::arg("rank"), pybind11::arg("steps"), pybind11::arg("alive_bonus"),
          pybind11::arg("act_cost"), pybind11::arg("init_seed"), pybind11::arg("member_offset"),
          pybind11::arg("policy_hidden") = 0, pybind11::arg("seed_buf") = c10::optional<torch::Tensor>(),
          pybind11::arg("env_image") = c10::optional<torch::Tensor>());
    m.def("rollout_env_image_v7", &ea::rollout_env_image_v7,
          "the v7 rollout kernel's prepacked environment (uint8): the constant range of its LDS layout for this env "
          "blob, independent of the blob's (mean, std) tail; pass it as env_image (Humanoid geometry only)",
          pybind11::arg("env_blob"), pybind11::arg("obs_dim"), pybind11::arg("act_dim"), pybind11::arg("rank"));
    m.def("rollout_terminating",
          [](torch::Tensor params, torch::Tensor env_blob, torch::Tensor obs_stats_out, torch::Tensor steps_out,
             int64_t obs_dim, int64_t act_dim, int64_t rank, int64_t steps, double alive_bonus, double act_cost,
             int64_t init_seed, int64_t member_offset, int64_t policy_hidden, int64_t health_index, double healthy_lo,
             double healthy_hi, c10::optional<torch::Tensor> seed_buf, c10::optional<torch::Tensor> env_image) {
              return ea::rollout_terminating(params, env_blob, obs_stats_out, steps_out, obs_dim, act_dim, rank, steps,
                                             alive_bonus, act_cost, init_seed, member_offset, policy_hidden,
                                             health_index, healthy_lo, healthy_hi, seed_buf, env_image, c10::nullopt,
                                             false);
          },
          "K10+K11 with early termination: an episode ends after the step whose bf16 o'[health_index] leaves "
          "[healthy_lo, healthy_hi]; episode lengths go to steps_out (v7 for the linear policy at the Humanoid "
          "geometry, the general v6 kernel elsewhere)",
          pybind11::arg("params"), pybind11::arg("env_blob"), pybind11::arg("obs_stats_out"),
          pybind11::arg("steps_out"), pybind11::arg("obs_dim"), pybind11::arg("act_dim"), pybind11::arg("rank"),
          pybind11::arg("steps"), pybind11::arg("alive_bonus"), pybind11::arg("act_cost"),
          pybind11::arg("init_seed"), pybind11::arg("member_offset"), pybind11::arg("policy_hidden"),
          pybind11::arg("health_index"), pybind11::arg("healthy_lo"), pybind11::arg("healthy_hi"),
          pybind11::arg("seed_buf") = c10::optional<torch::Tensor>(),
          pybind11::arg("env_image") = c10::optional<torch::Tensor>());
    m.def("rollout_terminating",
          [](torch::Tensor params, torch::Tensor env_blob, OutPair outputs, torch::Tensor steps_out, int64_t obs_dim,
             int64_t act_dim, int64_t rank, int64_t steps, double alive_bonus, double act_cost, int64_t init_seed,
             int64_t member_offset, int64_t policy_hidden, int64_t health_index, double healthy_lo, double healthy_hi,
             c10::optional<torch::Tensor> seed_buf, c10::optional<torch::Tensor> env_image) {
              return ea::rollout_terminating(params, env_blob, std::get<0>(outputs), steps_out, obs_dim, act_dim, rank,
                                             steps, alive_bonus, act_cost, init_seed, member_offset, policy_hidden,
                                             health_index, healthy_lo, healthy_hi, seed_buf, env_image,
                                             std::get<1>(outputs), true);
          },
          "rollout_terminating writing into the pair (obs_stats_out, fitness_out), as rollout_linear does",
          pybind11::arg("params"), pybind11::arg("env_blob"), pybind11::arg("outputs"), pybind11::arg("steps_out"),
          pybind11::arg("obs_dim"), pybind11::arg("act_dim"), pybind11::arg("rank"), pybind11::arg("steps"),
          pybind11::arg("alive_bonus"), pybind11::arg("act_cost"), pybind11::arg("init_seed"),
          pybind11::arg("member_offset"), pybind11::arg("policy_hidden"), pybind11::arg("health_index"),
          pybind11::arg("healthy_lo"), pybind11::arg("healthy_hi"),
          pybind11::arg("seed_buf") = c10::optional<torch::Tensor>(),
          pybind11::arg("env_image") = c10::optional<torch::Tensor>());
    m.def("rollout_kernel_name", &ea::rollout_kernel_name,
          "which rollout kernel the dispatcher picks, \"v7\", \"m7\" or \"v6\" (host only; reads "
          "EVOTORCH_AMD_ROLLOUT_V6 on every call)",
          pybind11::arg("obs_dim"), pybind11::arg("act_dim"), pybind11::arg("rank"), pybind11::arg("policy_hidden"),
          pybind11::arg("terminating"));
    m.def("bump_seed", &ea::bump_seed,
          "advance a device splitmix64 seed chain by one step (hipGraph-safe episode seeds)");
    m.def("cma_update_c", &ea::cma_update_c,
          "K5: fused CMA-ES covariance update (scale*C + c1*pc pc^T + cmu*Y^T diag(w) Y, exact symmetry)");
    m.def("potrf_tile", &ea::potrf_tile,
          "K5b: in-LDS Cholesky of one <=128x128 SPD diagonal panel (in place, device info flag)");
    m.def("fused_rank", &ea::fused_rank,
          "K2: fused bitonic ranking + utility map (centered/linear/nes) in one launch");
    m.def("nanmean_1d", &ea::nanmean_1d,
          "K2b: torch.nanmean of a dense fp32 vector of 1..nanmean_1d_max_length() elements in one launch, with "
          "torch's bits; returns a 0-dim fp32 tensor",
          py::arg("x"));
    m.def("nanmean_1d_max_length", &ea::nanmean_1d_max_length, "longest vector nanmean_1d accepts");
    m.def("domination_counts", &ea::domination_counts, "K7: NSGA-II domination counts (no N x N matrix)");
    m.def("pareto_ranks", &ea::pareto_ranks, "K7: NSGA-II non-dominated sorting by front peeling",
          py::arg("utils"), py::arg("min_assigned") = 0);
    m.def("mapelites_assign", &ea::mapelites_assign,
          "K9: MAPElites cell assignment, O(C+N) memory (streamed best-in-box argmax)");
}
