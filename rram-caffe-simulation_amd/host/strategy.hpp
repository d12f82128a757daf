// Fault-tolerance strategies.
//
//   FailureStrategy / ThresholdFailureStrategy — include/caffe/strategy.hpp:34-82,
//       src/caffe/strategy.cpp:7-33 (a3)
//   RemappingFailureStrategy / GeneticFailureStrategy — include/caffe/strategy.hpp:84-183,
//       src/caffe/strategy.cpp:35-288
#pragma once

#include <memory>
#include <vector>

#include "failure.hpp"

namespace caffe {

template <typename Dtype>
class Solver;

template <typename Dtype>
class FailureStrategy {
 public:
  FailureStrategy(const Msg& param, std::shared_ptr<FailureMaker<Dtype>> fm, std::shared_ptr<Net<Dtype>> net,
                  const Solver<Dtype>* solver)
      : param_(param), fmaker_(fm), net_(net), solver_(solver) {}
  virtual ~FailureStrategy() = default;
  // strategy.hpp:34-50; unknown type -> Error (Appendix A Q10: fail cleanly)
  static std::shared_ptr<FailureStrategy<Dtype>> CreateStrategy(const Msg& param, std::shared_ptr<FailureMaker<Dtype>> fm,
                                                                std::shared_ptr<Net<Dtype>> net, const Solver<Dtype>* s);
  virtual void Apply() = 0;
  virtual const char* type() const = 0;

 protected:
  Msg param_;
  std::shared_ptr<FailureMaker<Dtype>> fmaker_;
  std::shared_ptr<Net<Dtype>> net_;
  const Solver<Dtype>* solver_;
};

template <typename Dtype>
class ThresholdFailureStrategy : public FailureStrategy<Dtype> {
 public:
  using FailureStrategy<Dtype>::FailureStrategy;
  void Apply() override;
  const char* type() const override { return "threshold"; }
  float threshold() const { return static_cast<float>(this->param_.num("threshold", 0.001)); }
  // per failure param: threshold * lr * lr_mult (strategy.cpp:12-14)
  float threshold_for(int failure_param_index) const;
  // Appendix A Q6: the reference indexes params_lr() with the failure-param
  // index; true reproduces that quirk, false (default) uses the param's own lr_mult.
  bool reference_lr_index = false;
};

// glibc rand()/random() (TYPE_3 additive feedback generator of srandom_r /
// random_r): the reference's genetic strategy draws with unseeded rand()
// (strategy.cpp:170-175, Appendix A Q9), i.e. this generator at seed 1.
class GlibcRand {
 public:
  explicit GlibcRand(uint32_t seed = 1);
  int operator()();  // in [0, RAND_MAX = 2^31 - 1]

 private:
  uint32_t r_[34];
  int i_ = 0;  // ring position of r[k - 34]
};

// strategy.hpp:84-142 / strategy.cpp:35-137.  Every `period` iterations after
// `start`, the FC neurons are re-ordered so that the neurons the pretrained
// prune order ranks most prunable land on the physical neurons with the most
// stuck-at-zero cells.  Counts on the device, sort on the host (std::sort with
// the reference comparator, so ties resolve identically), moves as gathers.
// rram_reference_compat: true reproduces Appendix A Q8 (bias rows copied from
// the weight array, strategy.cpp:118-119).
template <typename Dtype>
class RemappingFailureStrategy : public FailureStrategy<Dtype> {
 public:
  RemappingFailureStrategy(const Msg& param, std::shared_ptr<FailureMaker<Dtype>> fm, std::shared_ptr<Net<Dtype>> net,
                           const Solver<Dtype>* solver);
  void Apply() override;
  const char* type() const override { return "remapping"; }
  // orders[i-1] for FC pair (i-1, i): neuron indices of FC layer i-1 sorted
  // by (#flagged cells in its input row + #flagged cells in its output column)
  std::vector<std::vector<int>> SortFCNeurons();
  const std::vector<std::vector<int>>& prune_orders() const { return prune_orders_; }
  bool reference_compat = false;

 private:
  int period_ = 100, start_ = 0, times_ = 0;
  std::vector<std::vector<int>> prune_orders_;
};

// strategy.hpp:144-183 / strategy.cpp:139-288.  Random pairwise neuron swaps
// accepted when they move failed cells onto weights the prune net marks as
// prunable.  The decisions only read the fault state and the prune masks, so
// they run on host copies; the accepted swaps compose into one permutation
// per FC blob, applied on the device in one gather per array.
// rram_reference_compat: true reproduces Q9's flat prune_input[n1]/[n2] swap
// (strategy.cpp:265-267); rram_rand_seed (default 1 = glibc's unseeded rand).
template <typename Dtype>
class GeneticFailureStrategy : public FailureStrategy<Dtype> {
 public:
  GeneticFailureStrategy(const Msg& param, std::shared_ptr<FailureMaker<Dtype>> fm, std::shared_ptr<Net<Dtype>> net,
                         const Solver<Dtype>* solver);
  void Apply() override;
  const char* type() const override { return "genetic"; }
  int CalculateOverallDist();
  int last_before() const { return before_; }
  int last_after() const { return after_; }
  int last_accepted() const { return accepted_; }
  bool reference_compat = false;

 private:
  void FetchEndurance();
  int switch_time_ = 100, period_ = 100, start_ = 0, times_ = 0;
  int before_ = 0, after_ = 0, accepted_ = 0;
  GlibcRand rand_;
  std::vector<std::vector<float>> prune_;  // prune net failure params (host, mutated by swaps)
  std::vector<std::vector<float>> endur_;     // endurance of every failure param (host copy per Apply)
};

}  // namespace caffe
