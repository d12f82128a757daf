// BatchNorm, Scale and Sigmoid (batch_norm_layer.cpp, scale_layer.cpp,
// sigmoid_layer.cpp), each a thin call into csrc/norm.hip.  A BatchNorm whose
// top's only reader is an in-place Scale, optionally followed by an in-place
// ReLU, runs the chain itself (Net::Net, option fuse_bn_scale): one streaming
// launch forward, one reduction + one streaming launch backward; the folded
// Scale and ReLU then only reshape, and their blobs stay where they are.
// Forward and Backward allocate nothing after the first Reshape and never
// synchronise, so the solver's captured-graph mode and MonteCarlo map batching
// (a TEST-phase BatchNorm treats images independently) hold.
#include "layers.hpp"

namespace caffe {

namespace {
uint32_t name_hash(const std::string& s) {
  uint32_t h = 2166136261u;
  for (unsigned char c : s) h = (h ^ c) * 16777619u;
  return h;
}
// NC(inner): channels = shape(1), inner = count / (num channels)
struct Dims {
  int num, C;
  int64_t inner;
};
template <typename Dtype>
Dims dims_of(const Blob<Dtype>& b) {
  return Dims{b.shape(0), b.shape(1), b.count(2)};
}
}  // namespace

void CheckNormLayerParam(const Msg& lp, int num_bottoms, int bottom_axes) {
  const std::string type = lp.str("type"), name = lp.str("name");
  if (type == "BatchNorm") {
    // the reference takes a 1-axis bottom as one channel; this build does not
    CAFFE_CHECK(bottom_axes >= 2, name << ": BatchNorm needs a bottom of at least 2 axes");
    // batch_norm_layer.cpp:39-48: the statistics are never trained
    auto specs = lp.subs("param");
    for (size_t i = 0; i < specs.size() && i < 3; ++i)
      CAFFE_CHECK(specs[i]->num("lr_mult", 1.0) == 0.0,
                  name << ": Cannot configure batch normalization statistics as layer parameters.");
  } else if (type == "Scale") {
    const Msg& sp = lp.sub_or_empty("scale_param");
    CAFFE_CHECK(num_bottoms == 1, name << ": the two-bottom Scale (the scale as an input) is not supported");
    CAFFE_CHECK(bottom_axes >= 2, name << ": Scale needs a bottom of at least 2 axes");
    int axis = static_cast<int>(sp.integer("axis", 1));
    if (axis < 0) axis += bottom_axes;
    CAFFE_CHECK(axis == 1 && sp.integer("num_axes", 1) == 1,
                name << ": only the channel-wise Scale (axis 1, num_axes 1) is supported");
  }
}


// ------------------------------------------------------------- BatchNorm
template <typename Dtype>
class BatchNormLayer : public Layer<Dtype> {
 public:
  explicit BatchNormLayer(const Msg& p) : Layer<Dtype>(p) {}
  const char* type() const override { return "BatchNorm"; }
  int ExactNumBottomBlobs() const override { return 1; }
  int ExactNumTopBlobs() const override { return 1; }
  void LayerSetUp(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>&) override {
    const Msg& bp = this->layer_param_.sub_or_empty("batch_norm_param");
    maf_ = static_cast<float>(bp.num("moving_average_fraction", 0.999));
    eps_ = static_cast<float>(bp.num("eps", 1e-5));
    use_global_ = bp.has("use_global_stats") ? bp.boolean("use_global_stats") : this->phase_ == TEST;
    CheckNormLayerParam(this->layer_param_, static_cast<int>(bottom.size()), bottom[0]->num_axes());
    C_ = bottom[0]->shape(1);
    if (this->blobs_.empty()) {  // else "Skipping parameter initialization"
      for (int n : {C_, C_, 1}) {
        this->blobs_.push_back(std::make_shared<Blob<Dtype>>(std::vector<int>{n}));
        RRAM_CALL(rram_set(n, 0.0f, this->blobs_.back()->mutable_gpu_data(), Caffe::stream()));
      }
    }
    this->param_propagate_down_.assign(3, false);
  }
  bool fixed_lr_mult(int, float* lr) const override {
    *lr = 0.0f;
    return true;
  }
  void Reshape(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>& top) override {
    CAFFE_CHECK(bottom[0]->num_axes() >= 2 && bottom[0]->shape(1) == C_, this->name() << ": input channels changed");
    top[0]->ReshapeLike(*bottom[0]);
    mean_.Reshape({C_});
    rstd_.Reshape({C_});
    const Dims d = dims_of(*bottom[0]);
    const size_t need = bottom[0]->count() > 0 ? rram_norm_workspace_floats(d.num, d.C, d.inner) : 0;
    ws_.Reshape({static_cast<int>(std::max<size_t>(need, 3 * (size_t)C_))});
    if (this->phase_ == TRAIN) xhat_.ReshapeLike(*bottom[0]);
  }
  bool fuse_scale_after(Layer<Dtype>* scale) override {
    if (scale != nullptr && (!scale->scale_foldable() || scale->blobs().empty() || scale->blobs()[0]->count() != C_))
      return false;
    scale_ = scale;
    if (scale == nullptr) relu_ = false;
    return true;
  }
  bool fuse_relu_after(float slope) override {
    if (scale_ == nullptr || slope != 0.0f) return false;
    relu_ = true;
    return true;
  }

 protected:
  const Dtype* gamma() const { return scale_ ? scale_->blobs()[0]->gpu_data() : nullptr; }
  const Dtype* beta() const { return scale_ && scale_->blobs().size() > 1 ? scale_->blobs()[1]->gpu_data() : nullptr; }
  void Forward_gpu(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>& top) override {
    if (bottom[0]->count() == 0) return;
    const Dims d = dims_of(*bottom[0]);
    const rram_stream_t s = Caffe::stream();
    if (use_global_)
      RRAM_CALL(rram_bn_stats_global(this->blobs_[0]->gpu_data(), this->blobs_[1]->gpu_data(),
                                     this->blobs_[2]->gpu_data(), C_, eps_, mean_.mutable_gpu_data(),
                                     rstd_.mutable_gpu_data(), s));
    else
      RRAM_CALL(rram_bn_stats_train(bottom[0]->gpu_data(), d.num, d.C, d.inner, eps_, maf_, mean_.mutable_gpu_data(),
                                    rstd_.mutable_gpu_data(), this->blobs_[0]->mutable_gpu_data(),
                                    this->blobs_[1]->mutable_gpu_data(), this->blobs_[2]->mutable_gpu_data(),
                                    ws_.mutable_gpu_data(), ws_.count() - 3 * C_, s));
    const Dtype* x = bottom[0]->gpu_data();
    RRAM_CALL(rram_norm_apply(x, top[0]->mutable_gpu_data(), this->phase_ == TRAIN ? xhat_.mutable_gpu_data() : nullptr,
                              mean_.gpu_data(), rstd_.gpu_data(), gamma(), beta(), relu_ ? 1 : 0, d.num, d.C, d.inner,
                              s));
  }
  void Backward_gpu(const std::vector<Blob<Dtype>*>& top, const std::vector<bool>& pd,
                    const std::vector<Blob<Dtype>*>& bottom) override {
    if (bottom[0]->count() == 0) return;
    const bool dx = pd.size() > 0 && pd[0];
    Dtype* dgamma = scale_ && scale_->param_propagate_down(0) ? scale_->blobs()[0]->mutable_gpu_diff() : nullptr;
    Dtype* dbeta = scale_ && scale_->blobs().size() > 1 && scale_->param_propagate_down(1)
                       ? scale_->blobs()[1]->mutable_gpu_diff()
                       : nullptr;
    if (!dx && !dgamma && !dbeta) return;
    const bool centred = !use_global_;
    CAFFE_CHECK(this->phase_ == TRAIN || (!centred && !dgamma && !dbeta),
                this->name() << ": this BatchNorm backward needs the TRAIN phase (it reads the stored x^)");
    const Dims d = dims_of(*bottom[0]);
    const rram_stream_t s = Caffe::stream();
    const Dtype* relu_y = relu_ ? top[0]->gpu_data() : nullptr;
    Dtype* coef = ws_.mutable_gpu_data() + (ws_.count() - 3 * C_);
    if (centred || dgamma || dbeta)
      RRAM_CALL(rram_norm_bwd_reduce(top[0]->gpu_diff(), relu_y, xhat_.gpu_data(), d.num, d.C, d.inner, gamma(),
                                     rstd_.gpu_data(), dgamma, dbeta, centred ? coef : nullptr,
                                     ws_.mutable_gpu_data(), ws_.count() - 3 * C_, s));
    if (dx)
      RRAM_CALL(rram_norm_bwd_apply(top[0]->gpu_diff(), relu_y, centred ? xhat_.gpu_data() : nullptr,
                                    centred ? coef : nullptr, gamma(), rstd_.gpu_data(),
                                    bottom[0]->mutable_gpu_diff(), d.num, d.C, d.inner, s));
  }
  float maf_ = 0.999f, eps_ = 1e-5f;
  bool use_global_ = false, relu_ = false;
  int C_ = 0;
  Layer<Dtype>* scale_ = nullptr;  // the folded in-place Scale that follows (Net::Net)
  Blob<Dtype> mean_, rstd_, xhat_, ws_;
};

// ----------------------------------------------------------------- Scale
// The one-bottom, channel-wise form (axis 1, num_axes 1) of scale_layer.cpp.
template <typename Dtype>
class ScaleLayer : public Layer<Dtype> {
 public:
  explicit ScaleLayer(const Msg& p) : Layer<Dtype>(p) {}
  const char* type() const override { return "Scale"; }
  int ExactNumTopBlobs() const override { return 1; }
  void LayerSetUp(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>&) override {
    const Msg& sp = this->layer_param_.sub_or_empty("scale_param");
    CheckNormLayerParam(this->layer_param_, static_cast<int>(bottom.size()), bottom.empty() ? 0 : bottom[0]->num_axes());
    C_ = bottom[0]->shape(1);
    const uint64_t seed = Caffe::seed() ^ (uint64_t)name_hash(this->name()) << 20;
    if (this->blobs_.empty()) {  // else "Skipping parameter initialization", as BatchNorm
      this->blobs_.push_back(std::make_shared<Blob<Dtype>>(std::vector<int>{C_}));
      if (sp.has("filler"))
        FillBlob(this->blobs_[0].get(), sp.sub_or_empty("filler"), seed, 0);
      else  // scale_layer.cpp:35-40: the default filler is the constant 1
        RRAM_CALL(rram_set(C_, 1.0f, this->blobs_[0]->mutable_gpu_data(), Caffe::stream()));
      if (sp.boolean("bias_term", false)) {
        this->blobs_.push_back(std::make_shared<Blob<Dtype>>(std::vector<int>{C_}));
        FillBlob(this->blobs_[1].get(), sp.sub_or_empty("bias_filler"), seed, 1);
      }
    }
    this->param_propagate_down_.assign(this->blobs_.size(), true);
  }
  void Reshape(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>& top) override {
    CAFFE_CHECK(bottom[0]->num_axes() >= 2 && bottom[0]->shape(1) == C_, this->name() << ": input channels changed");
    top[0]->ReshapeLike(*bottom[0]);
    if (this->folded_into_prev) return;
    const Dims d = dims_of(*bottom[0]);
    if (this->phase_ == TRAIN) {
      const size_t need = bottom[0]->count() > 0 ? rram_norm_workspace_floats(d.num, d.C, d.inner) : 0;
      ws_.Reshape({static_cast<int>(std::max<size_t>(need, 1))});
      // an in-place Scale keeps its bottom for dgamma (scale_layer.cpp's temp_)
      if (bottom[0] == top[0]) temp_.ReshapeLike(*bottom[0]);
    }
  }
  bool scale_foldable() const override { return true; }

 protected:
  void Forward_gpu(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>& top) override {
    if (this->folded_into_prev || bottom[0]->count() == 0) return;  // applied by the BatchNorm before
    const Dims d = dims_of(*bottom[0]);
    if (bottom[0] == top[0] && this->phase_ == TRAIN)
      HIP_CALL(hipMemcpyAsync(temp_.mutable_gpu_data(), bottom[0]->gpu_data(), bottom[0]->count() * sizeof(Dtype),
                              hipMemcpyDeviceToDevice, Caffe::hip_stream()));
    const Dtype* x = bottom[0]->gpu_data();
    RRAM_CALL(rram_norm_apply(x, top[0]->mutable_gpu_data(), nullptr, nullptr, nullptr, this->blobs_[0]->gpu_data(),
                              this->blobs_.size() > 1 ? this->blobs_[1]->gpu_data() : nullptr, 0, d.num, d.C,
                              d.inner, Caffe::stream()));
  }
  void Backward_gpu(const std::vector<Blob<Dtype>*>& top, const std::vector<bool>& pd,
                    const std::vector<Blob<Dtype>*>& bottom) override {
    if (this->folded_into_prev || bottom[0]->count() == 0) return;
    const Dims d = dims_of(*bottom[0]);
    Dtype* dgamma = this->param_propagate_down(0) ? this->blobs_[0]->mutable_gpu_diff() : nullptr;
    Dtype* dbeta = this->blobs_.size() > 1 && this->param_propagate_down(1) ? this->blobs_[1]->mutable_gpu_diff()
                                                                             : nullptr;
    if (dgamma || dbeta) {
      CAFFE_CHECK(this->phase_ == TRAIN, this->name() << ": Scale parameter gradients need the TRAIN phase");
      const Dtype* x = bottom[0] == top[0] ? temp_.gpu_data() : bottom[0]->gpu_data();
      RRAM_CALL(rram_norm_bwd_reduce(top[0]->gpu_diff(), nullptr, x, d.num, d.C, d.inner, nullptr, nullptr, dgamma,
                                     dbeta, nullptr, ws_.mutable_gpu_data(), ws_.count(), Caffe::stream()));
    }
    if (pd.size() > 0 && pd[0])
      RRAM_CALL(rram_norm_bwd_apply(top[0]->gpu_diff(), nullptr, nullptr, nullptr, this->blobs_[0]->gpu_data(), nullptr,
                                    bottom[0]->mutable_gpu_diff(), d.num, d.C, d.inner, Caffe::stream()));
  }
  int C_ = 0;
  Blob<Dtype> temp_, ws_;
};

// --------------------------------------------------------------- Sigmoid
template <typename Dtype>
class SigmoidLayer : public Layer<Dtype> {
 public:
  explicit SigmoidLayer(const Msg& p) : Layer<Dtype>(p) {}
  const char* type() const override { return "Sigmoid"; }
  int ExactNumBottomBlobs() const override { return 1; }
  int ExactNumTopBlobs() const override { return 1; }
  void Reshape(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>& top) override {
    top[0]->ReshapeLike(*bottom[0]);
  }

 protected:
  void Forward_gpu(const std::vector<Blob<Dtype>*>& bottom, const std::vector<Blob<Dtype>*>& top) override {
    const Dtype* x = bottom[0]->gpu_data();
    RRAM_CALL(rram_sigmoid_fwd(x, top[0]->mutable_gpu_data(), bottom[0]->count(), Caffe::stream()));
  }
  void Backward_gpu(const std::vector<Blob<Dtype>*>& top, const std::vector<bool>& pd,
                    const std::vector<Blob<Dtype>*>& bottom) override {
    if (!pd.size() || !pd[0]) return;
    RRAM_CALL(rram_sigmoid_bwd(top[0]->gpu_data(), top[0]->gpu_diff(), bottom[0]->mutable_gpu_diff(),
                               bottom[0]->count(), Caffe::stream()));
  }
};

REGISTER_LAYER_CLASS(BatchNorm);
REGISTER_LAYER_CLASS(Scale);
REGISTER_LAYER_CLASS(Sigmoid);

}  // namespace caffe
