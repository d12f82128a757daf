#include "failure.hpp"

#include <algorithm>

namespace caffe {

template <typename Dtype>
FailureMaker<Dtype>::~FailureMaker() {
  if (d_counts_) (void)hipFree(d_counts_);
}

template <typename Dtype>
std::shared_ptr<FailureMaker<Dtype>> FailureMaker<Dtype>::CreateMaker(const Msg& param,
                                                                      std::shared_ptr<Net<Dtype>> net) {
  const std::string type = param.str("type", "gaussian");
  if (type == "gaussian") return std::make_shared<GaussianFailureMaker<Dtype>>(param, net);
  CAFFE_CHECK(type != "uniform", "failure_pattern type 'uniform' is declared in caffe.proto but not implemented "
                                 "by the reference either (Appendix A Q13)");
  return nullptr;
}

template <typename Dtype>
std::vector<Blob<Dtype>*> FailureMaker<Dtype>::fail_iterations() {
  std::vector<Blob<Dtype>*> v;
  for (auto& b : fail_iterations_) v.push_back(b.get());
  return v;
}

template <typename Dtype>
std::vector<unsigned long long> FailureMaker<Dtype>::broken_counts() {
  std::vector<unsigned long long> h(fail_iterations_.size(), 0);
  if (d_counts_ && !h.empty()) {
    HIP_CALL(hipMemcpyAsync(h.data(), d_counts_, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            Caffe::hip_stream()));
    HIP_CALL(hipStreamSynchronize(Caffe::hip_stream()));
  }
  return h;
}

// failure_maker.cpp:5-52
template <typename Dtype>
GaussianFailureMaker<Dtype>::GaussianFailureMaker(const Msg& param, std::shared_ptr<Net<Dtype>> net)
    : FailureMaker<Dtype>(param) {
  this->net_ = net;
  long long neg = 10, zero = 20, pos = 10;  // defaults (failure_maker.cpp:17-21)
  if (const Msg* fp = param.sub("failure_prob")) {
    neg = fp->integer("neg", 10);
    zero = fp->integer("zero", 20);
    pos = fp->integer("pos", 10);
    CAFFE_CHECK(neg >= 0, "Probability for failure to -1 must be greater or equal than 0");
    CAFFE_CHECK(zero >= 0, "Probability for failure to 0 must be greater or equal than 0");
    CAFFE_CHECK(pos >= 0, "Probability for failure to 1 must be greater or equal than 0");
  }
  const long long sum = neg + zero + pos;
  CAFFE_CHECK(sum > 0, "failure_prob entries sum to 0");
  const uint64_t thr_neg = ((uint64_t)neg * (1ull << 32) + sum - 1) / sum;
  const uint64_t thr_zero = ((uint64_t)(neg + zero) * (1ull << 32) + sum - 1) / sum;
  const float mean = static_cast<float>(param.num("mean", 10000));  // caffe.proto:255 defaults
  const float std = static_cast<float>(param.num("std", 100));
  decrement = static_cast<float>(param.num("rram_decrement", 100.0));
  const auto& fps = net->failure_learnable_params();
  for (size_t i = 0; i < fps.size(); ++i) {
    auto b = std::make_unique<Blob<Dtype>>(fps[i]->shape());
    RRAM_CALL(rram_fault_init(b->mutable_gpu_data(), b->mutable_gpu_diff(), b->count(), mean, std, thr_neg,
                              thr_zero, Caffe::seed(), 0u, static_cast<uint32_t>(i), Caffe::stream()));
    this->fail_iterations_.push_back(std::move(b));
  }
  if (!fps.empty()) {
    HIP_CALL(hipMalloc(&this->d_counts_, fps.size() * sizeof(unsigned long long)));
    HIP_CALL(hipMemsetAsync(this->d_counts_, 0, fps.size() * sizeof(unsigned long long), Caffe::hip_stream()));
  }
}

// failure_maker.cu:44-58 — all blobs in batched launches of <= RRAM_MAX_SEGS
template <typename Dtype>
void GaussianFailureMaker<Dtype>::Fail_gpu(int /*iter*/) {
  const auto& fps = this->net_->failure_learnable_params();
  const size_t n = fps.size();
  if (!n) return;
  HIP_CALL(hipMemsetAsync(this->d_counts_, 0, n * sizeof(unsigned long long), Caffe::hip_stream()));
  std::vector<rram_fail_seg> segs(n);
  for (size_t i = 0; i < n; ++i) {
    auto& fi = this->fail_iterations_[i];
    segs[i] = rram_fail_seg{fps[i]->gpu_diff(), fps[i]->mutable_gpu_data(), fi->mutable_gpu_data(), fi->gpu_diff(),
                            fps[i]->count()};
  }
  for (size_t s = 0; s < n; s += RRAM_MAX_SEGS) {
    const int k = static_cast<int>(std::min<size_t>(RRAM_MAX_SEGS, n - s));
    RRAM_CALL(rram_fail_apply_batched(segs.data() + s, k, decrement, epsilon, this->d_counts_ + s, Caffe::stream()));
  }
}

template class FailureMaker<float>;
template class GaussianFailureMaker<float>;

}  // namespace caffe
