// The solver.
//
//   Solver / SGDSolver — src/caffe/solver.cpp (fork hooks :14-40, :132-148,
//       Step order :237-325, Test :385-458), src/caffe/solvers/sgd_solver.cpp (a4, a11)
//
// The fault model (failure.hpp), the fault-tolerance strategies
// (strategy.hpp), the Monte-Carlo fault-map driver (monte_carlo.hpp) and the
// hipGraph plumbing (graph.hpp) come with it.
#pragma once

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "failure.hpp"
#include "graph.hpp"
#include "monte_carlo.hpp"
#include "net.hpp"
#include "strategy.hpp"

namespace caffe {

template <typename Dtype>
class Solver {
 public:
  // solver_param: SolverParameter text; net_param (optional) overrides `net:`;
  // options: net options (data_shape, num_classes, fault_layers, fuse_relu)
  // plus `fused_update` (true: one fused HBM pass per blob for the training tail).
  Solver(const Msg& solver_param, const Msg* net_param, const Msg& options);
  virtual ~Solver();

  void Step(int iters);
  // solver.cpp:328-370; resume_file: a .solverstate to Restore() first
  void Solve(const char* resume_file = nullptr);
  // solver.cpp:461-518 (BINARYPROTO): <prefix>_iter_N.caffemodel and
  // .solverstate, plus <prefix>_iter_N.faultstate with the fault maps
  // (Appendix A Q11: the reference redraws them on resume).  Returns the
  // .solverstate path.
  std::string Snapshot();
  // sgd_solver.cpp:309-326; the fault maps come back too when the matching
  // .faultstate file exists
  void Restore(const std::string& state_file);
  const Msg& net_options() const { return options_; }
  void emit_log(const std::string& s) const {
    if (log) log(s);
  }
  // returns the mean of every output element of test net `id` over test_iter
  std::vector<Dtype> Test(int id = 0);
  std::vector<std::vector<Dtype>> TestAll();

  std::shared_ptr<Net<Dtype>> net() { return net_; }
  const std::vector<std::shared_ptr<Net<Dtype>>>& test_nets() const { return test_nets_; }
  int iter() const { return iter_; }
  const Msg& param() const { return param_; }
  Dtype GetLearningRate() const;
  std::shared_ptr<FailureMaker<Dtype>> failure_maker() { return fmaker_; }
  const std::vector<std::shared_ptr<FailureStrategy<Dtype>>>& strategies() const { return strategys_; }
  Dtype smoothed_loss() const { return smoothed_loss_; }
  // SGDSolver::history() (sgd_solver.hpp:29): one history blob per learnable
  // param; AdaDelta and Adam append a second set (adadelta_solver.cpp:8-16,
  // adam_solver.cpp:8-17), history()[i + nparams] pairing with param i
  const std::vector<std::unique_ptr<Blob<Dtype>>>& history() const { return history_; }
  // Solver::type() (sgd_solvers.hpp): "SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam"
  const char* type() const;
  int kind() const { return kind_; }  // RRAM_SOLVER_*
  // Solver::Callback::on_gradients_ready (solver.hpp:80-91): the data-parallel
  // hook (RCCL all-reduce of the flat gradient buffer).
  std::function<void()> on_gradients_ready;
  std::function<void(const std::string&)> log;
  // hipGraph replay of the training iteration (opt-in; launch-bound small
  // nets, no reference counterpart): [ClearParamDiffs + Forward + Backward]
  // and the fused update tail are each captured once, after one eager
  // iteration, and replayed; on_gradients_ready (the data-parallel RCCL
  // all-reduce) runs between the two launches, outside any graph.
  // Iterations that display, test, snapshot or average the loss run eager,
  // as does everything when the fused tail is off or a per-layer backward
  // hook is set; a changed learning rate or moved buffers recapture.  Nets
  // with per-iteration host state (Dropout, HDF5Data) are refused.
  // Bit-identical to the eager iterations.
  void set_graph(bool on);
  bool graph_active() const { return captured_[0].ready(); }
  // the flat learnable data / diff buffers every param is aliased into
  // (nullptr when the `flat_params: false` option turned them off)
  Dtype* flat_data() const { return static_cast<Dtype*>(flat_); }
  Dtype* flat_diff() const { return flat_ ? static_cast<Dtype*>(flat_) + net_->flat_param_count() : nullptr; }

 protected:
  bool graph_ = false, graph_warm_ = false;
  CapturedGraph captured_[2];  // 0: clear + forward + backward, 1: the fused tail
  GraphStream gstream_;
  Dtype graph_rate_ = 0, graph_prev_rate_ = -1;
  std::vector<const void*> graph_ptrs_;
  std::vector<const void*> graph_key() const;
  void drop_graphs();
  template <typename F>
  void capture_launch(int k, F&& body);
  void InitFailurePattern(const Msg& failure_param);
  void InitSolverType();
  void ComputeUpdate();
  void ApplyStrategy();
  void ApplyUpdate();
  void FusedTail();
  void Fail(int iter) {
    if (fmaker_) fmaker_->Fail(iter);
  }
  void ClipGradients();
  void Regularize(int param_id);
  void ComputeUpdateValue(int param_id, Dtype rate);
  // the rate the type's update kernel takes for param_id: rate * lr_mult, for
  // Adam times the bias correction of this iteration
  Dtype LocalRate(int param_id, Dtype rate) const;
  Dtype AdamCorrection() const;
  void emit(const std::string& s) {
    if (log) log(s);
  }

  std::string SnapshotFilename(const std::string& ext) const {
    return param_.str("snapshot_prefix") + "_iter_" + std::to_string(iter_) + ext;
  }

  Msg param_;
  Msg options_;
  // flat learnable data / diff buffers the params are aliased into
  // (ClearParamDiffs becomes one memset; the data-parallel all-reduce re-aliases)
  void* flat_ = nullptr;
  std::shared_ptr<Net<Dtype>> net_;
  std::vector<std::shared_ptr<Net<Dtype>>> test_nets_;
  std::vector<std::unique_ptr<Blob<Dtype>>> history_, temp_;
  std::shared_ptr<FailureMaker<Dtype>> fmaker_;
  std::vector<std::shared_ptr<FailureStrategy<Dtype>>> strategys_;
  int iter_ = 0, current_step_ = 0;
  Dtype smoothed_loss_ = 0;
  std::vector<Dtype> losses_;
  bool fused_update_ = false;
  int kind_ = RRAM_SOLVER_SGD;
  rram_solver_hyper hyper_{};  // momentum / beta1, momentum2 / rms_decay, delta (fp32, caffe.proto's `optional float`)
  bool flip_cache_ = true;  // option conv_flip_cache: FusedTail writes the flipped kernels (rram_update_seg.w_flip)
};

}  // namespace caffe
