// Fault model.
//
//   FailureMaker / GaussianFailureMaker  — include/caffe/failure_maker.hpp:11-96,
//       src/caffe/failure_maker.cpp, failure_maker.cu
#pragma once

#include <memory>
#include <vector>

#include "net.hpp"

namespace caffe {

template <typename Dtype>
class FailureMaker {
 public:
  explicit FailureMaker(const Msg& param) : param_(param) {}
  virtual ~FailureMaker();
  // failure_maker.hpp:23-30: nullptr unless type == "gaussian"
  static std::shared_ptr<FailureMaker<Dtype>> CreateMaker(const Msg& param, std::shared_ptr<Net<Dtype>> net);
  // failure_maker.hpp:32-58 without the per-iteration D2H count (Appendix A Q5):
  // the broken count accumulates on the device, read it with broken_counts().
  void Fail(int iter) { Fail_gpu(iter); }
  virtual void Fail_gpu(int iter) = 0;
  std::vector<Blob<Dtype>*> fail_iterations();
  std::vector<unsigned long long> broken_counts();  // per failure param, after the last Fail()
  unsigned long long* device_counts() { return d_counts_; }
  const Msg& param() const { return param_; }

 protected:
  Msg param_;
  std::shared_ptr<Net<Dtype>> net_;
  // endurance in data, stuck value in diff (reference layout, failure_maker.cpp:30-36)
  std::vector<std::unique_ptr<Blob<Dtype>>> fail_iterations_;
  unsigned long long* d_counts_ = nullptr;
};

template <typename Dtype>
class GaussianFailureMaker : public FailureMaker<Dtype> {
 public:
  GaussianFailureMaker(const Msg& param, std::shared_ptr<Net<Dtype>> net);
  void Fail_gpu(int iter) override;
  float decrement = 100.0f;  // "batch size FIXME" constant (failure_maker.cpp:73)
  float epsilon = 1e-20f;    // failure_maker.cpp:56
};

}  // namespace caffe
