#include "solver.hpp"

#include "hdf5.hpp"
#include "layers.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

namespace caffe {

// ================================================================ Solver
static Msg load_net_param(const Msg& sp, const Msg* net_param) {
  if (net_param) return *net_param;
  if (const Msg* np = sp.sub("net_param")) return *np;
  if (const Msg* np = sp.sub("train_net_param")) return *np;
  std::string f = sp.str("net", sp.str("train_net", ""));
  CAFFE_CHECK(!f.empty(), "solver: no net given (net / net_param / train_net)");
  return parse_prototxt_file(f);
}

template <typename Dtype>
Solver<Dtype>::Solver(const Msg& sp, const Msg* net_param, const Msg& options) : param_(sp), options_(options) {
  if (sp.has("random_seed") && sp.integer("random_seed") >= 0)
    Caffe::set_random_seed(static_cast<uint64_t>(sp.integer("random_seed")));
  fused_update_ = options.boolean("fused_update", false);
  flip_cache_ = options.boolean("conv_flip_cache", true);
  InitSolverType();
  const Msg np = load_net_param(sp, net_param);
  net_ = std::make_shared<Net<Dtype>>(np, TRAIN, options);
  // solver.cpp:132-148: fault maker and strategies on the root solver
  if (const Msg* fp = sp.sub("failure_pattern")) InitFailurePattern(*fp);
  for (auto* st : sp.subs("failure_strategy")) {
    auto p = FailureStrategy<Dtype>::CreateStrategy(*st, fmaker_, net_, this);
    strategys_.push_back(p);
  }
  // test nets (solver.cpp:155-230): test_net_param / test_net, else the train net in TEST phase
  std::vector<Msg> tnp;
  for (auto* t : sp.subs("test_net_param")) tnp.push_back(*t);
  for (auto& f : sp.strs("test_net")) tnp.push_back(parse_prototxt_file(f));
  if (tnp.empty() && sp.count("test_iter") > 0) tnp.push_back(np);
  for (auto& t : tnp) {
    test_nets_.push_back(std::make_shared<Net<Dtype>>(t, TEST, options));
    test_nets_.back()->ShareTrainedLayersWith(net_.get());
  }
  for (auto* p : net_->learnable_params()) {
    history_.push_back(std::make_unique<Blob<Dtype>>(p->shape()));
    HIP_CALL(hipMemsetAsync(history_.back()->mutable_gpu_data(), 0, p->count() * sizeof(Dtype), Caffe::hip_stream()));
    temp_.push_back(std::make_unique<Blob<Dtype>>(p->shape()));
  }
  // AdaDelta and Adam keep a second set of histories after the first
  // (adadelta_solver.cpp:8-16, adam_solver.cpp:8-17): history_[i + nparams]
  if (kind_ == RRAM_SOLVER_ADADELTA || kind_ == RRAM_SOLVER_ADAM)
    for (auto* p : net_->learnable_params()) {
      history_.push_back(std::make_unique<Blob<Dtype>>(p->shape()));
      HIP_CALL(hipMemsetAsync(history_.back()->mutable_gpu_data(), 0, p->count() * sizeof(Dtype), Caffe::hip_stream()));
    }
  const int64_t nflat = net_->flat_param_count();
  if (nflat > 0 && options.boolean("flat_params", true)) {
    HIP_CALL(hipMalloc(&flat_, 2 * nflat * sizeof(Dtype)));
    net_->alias_flat_params(static_cast<Dtype*>(flat_), static_cast<Dtype*>(flat_) + nflat);
  }
}

template <typename Dtype>
Solver<Dtype>::~Solver() {
  drop_graphs();
  if (flat_) {
    (void)hipStreamSynchronize(Caffe::hip_stream());
    (void)hipFree(flat_);
  }
}

// solver.cpp:14-23
template <typename Dtype>
void Solver<Dtype>::InitFailurePattern(const Msg& fp) {
  if (fp.str("type", "gaussian") == "none") return;
  fmaker_ = FailureMaker<Dtype>::CreateMaker(fp, net_);
}

// sgd_solver.cpp GetLearningRate
template <typename Dtype>
Dtype Solver<Dtype>::GetLearningRate() const {
  // sgd_solver.cpp:27-63.  base_lr / gamma / power are `optional float` in
  // caffe.proto, so they are rounded to fp32 first; the fp32 sub-expressions
  // (1 + gamma*iter, 1 - iter/max_iter) stay fp32 and pow/exp run in double
  // (the C library ::pow the unqualified calls bind to), as in the reference.
  const std::string policy = param_.str("lr_policy", "fixed");
  const float base = static_cast<float>(param_.num("base_lr", 0.01));
  const float gamma = static_cast<float>(param_.num("gamma", 0.0));
  const float power = static_cast<float>(param_.num("power", 0.0));
  const int it = iter_;
  if (policy == "fixed") return (Dtype)base;
  if (policy == "step") {
    const int step = it / (int)param_.integer("stepsize", 1);
    return (Dtype)((double)base * std::pow((double)gamma, (double)step));
  }
  if (policy == "exp") return (Dtype)((double)base * std::pow((double)gamma, (double)it));
  if (policy == "inv") {
    const float b = 1.0f + gamma * static_cast<float>(it);
    return (Dtype)((double)base * std::pow((double)b, (double)-power));
  }
  if (policy == "multistep") {
    auto sv = param_.nums("stepvalue");
    int step = 0;
    while (step < (int)sv.size() && it >= sv[step]) ++step;
    return (Dtype)((double)base * std::pow((double)gamma, (double)step));
  }
  if (policy == "poly") {
    const float b = 1.0f - static_cast<float>(it) / static_cast<float>(param_.integer("max_iter", 1));
    return (Dtype)((double)base * std::pow((double)b, (double)power));
  }
  if (policy == "sigmoid") {
    const float x = -gamma * (static_cast<float>(it) - static_cast<float>(param_.integer("stepsize", 1)));
    return (Dtype)((double)base * (1.0 / (1.0 + std::exp((double)x))));
  }
  throw Error("Unknown learning rate policy: " + policy);
}

template <typename Dtype>
void Solver<Dtype>::ClipGradients() {
  const double clip = param_.num("clip_gradients", -1.0);
  if (clip < 0) return;
  const auto& ps = net_->learnable_params();
  double sumsq = 0;
  Dtype* dtmp = nullptr;
  HIP_CALL(hipMallocAsync(reinterpret_cast<void**>(&dtmp), sizeof(Dtype), Caffe::hip_stream()));
  for (auto* p : ps) {
    Dtype h = 0;
    RRAM_CALL(rram_dot(p->count(), p->gpu_diff(), p->gpu_diff(), dtmp, Caffe::stream()));
    HIP_CALL(hipMemcpyAsync(&h, dtmp, sizeof(Dtype), hipMemcpyDeviceToHost, Caffe::hip_stream()));
    HIP_CALL(hipStreamSynchronize(Caffe::hip_stream()));
    sumsq += h;
  }
  HIP_CALL(hipFreeAsync(dtmp, Caffe::hip_stream()));
  const double l2 = std::sqrt(sumsq);
  if (l2 > clip)
    for (auto* p : ps) RRAM_CALL(rram_scal(p->count(), (Dtype)(clip / l2), p->mutable_gpu_diff(), Caffe::stream()));
}

// sgd_solver.cpp:148-214
template <typename Dtype>
void Solver<Dtype>::Regularize(int id) {
  auto* p = net_->learnable_params()[id];
  const Dtype decay = (Dtype)param_.num("weight_decay", 0.0) * net_->params_weight_decay()[id];
  if (decay == Dtype(0)) return;
  const std::string rt = param_.str("regularization_type", "L2");
  if (rt == "L2") {
    RRAM_CALL(rram_axpy(p->count(), decay, p->gpu_data(), p->mutable_gpu_diff(), Caffe::stream()));
  } else if (rt == "L1") {
    RRAM_CALL(rram_sign(p->count(), p->gpu_data(), temp_[id]->mutable_gpu_data(), Caffe::stream()));
    RRAM_CALL(rram_axpy(p->count(), decay, temp_[id]->gpu_data(), p->mutable_gpu_diff(), Caffe::stream()));
  } else {
    throw Error("Unknown regularization type: " + rt);
  }
}

static const char* const kSolverTypeNames[] = {"SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam"};
static const char* const kSolverTypeEnum[] = {"SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADADELTA", "ADAM"};

template <typename Dtype>
const char* Solver<Dtype>::type() const {
  return kSolverTypeNames[kind_];
}

// solver_factory.hpp / upgrade_proto.cpp:1017-1060: `type` (default "SGD"),
// or the deprecated `solver_type` enum (caffe.proto:233-242); then the
// classes' constructor checks (sgd_solvers.hpp:77,97-101) and the solver-wide
// scalars, `optional float` in caffe.proto (:217-223), so rounded to fp32
template <typename Dtype>
void Solver<Dtype>::InitSolverType() {
  int by_type = -1, by_enum = -1;
  if (param_.has("type")) {
    const std::string t = param_.str("type");
    for (int k = 0; k < 6; ++k)
      if (t == kSolverTypeNames[k]) by_type = k;
    CAFFE_CHECK(by_type >= 0, "Unknown solver type: " << t
                                  << " (known types: SGD, Nesterov, AdaGrad, RMSProp, AdaDelta, Adam)");
  }
  if (param_.has("solver_type")) {
    const std::string t = param_.str("solver_type");
    for (int k = 0; k < 6; ++k)
      if (t == kSolverTypeEnum[k] || t == std::to_string(k)) by_enum = k;
    CAFFE_CHECK(by_enum >= 0, "Unknown solver_type: " << t
                                  << " (known values: SGD, NESTEROV, ADAGRAD, RMSPROP, ADADELTA, ADAM)");
  }
  CAFFE_CHECK(by_type < 0 || by_enum < 0 || by_type == by_enum,
              "solver type: \"" << param_.str("type") << "\" and the deprecated solver_type: "
                                << param_.str("solver_type") << " disagree");
  kind_ = by_type >= 0 ? by_type : (by_enum >= 0 ? by_enum : RRAM_SOLVER_SGD);
  hyper_.momentum = static_cast<float>(param_.num("momentum", 0.0));
  hyper_.delta = static_cast<float>(param_.num("delta", 1e-8));
  hyper_.momentum2 = static_cast<float>(param_.num("momentum2", 0.999));
  if (kind_ == RRAM_SOLVER_ADAGRAD) CAFFE_CHECK(hyper_.momentum == 0.0f, "Momentum cannot be used with AdaGrad.");
  if (kind_ == RRAM_SOLVER_RMSPROP) {
    CAFFE_CHECK(hyper_.momentum == 0.0f, "Momentum cannot be used with RMSProp.");
    const float rms_decay = static_cast<float>(param_.num("rms_decay", 0.99));
    CAFFE_CHECK(rms_decay >= 0.0f && rms_decay < 1.0f, "rms_decay should lie between 0 and 1 (rms_decay: " << rms_decay << ")");
    hyper_.momentum2 = rms_decay;  // the decay rate of RMSProp's one history
  }
}

// adam_solver.cpp:39-41: t = iter_ + 1, correction = std::sqrt(Dtype(1) -
// pow(beta2, t)) / (Dtype(1.) - pow(beta1, t)).  The unqualified pow(float,
// int) promotes to double, so the subtractions, the sqrt and the division run
// in double too; the result is stored to fp32 and local_rate * correction
// (adam_solver.cpp:72) is an fp32 product.
template <typename Dtype>
Dtype Solver<Dtype>::AdamCorrection() const {
  const int t = iter_ + 1;
  const double b1 = hyper_.momentum, b2 = hyper_.momentum2;
  return (Dtype)(std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t)));
}

template <typename Dtype>
Dtype Solver<Dtype>::LocalRate(int id, Dtype rate) const {
  const Dtype local = rate * net_->params_lr()[id];
  return kind_ == RRAM_SOLVER_ADAM ? local * AdamCorrection() : local;
}

// sgd_solver.cpp:216-247 and the other classes' ComputeUpdateValue (GPU
// branch: one update kernel per type)
template <typename Dtype>
void Solver<Dtype>::ComputeUpdateValue(int id, Dtype rate) {
  auto* p = net_->learnable_params()[id];
  const Dtype local = LocalRate(id, rate);
  Dtype* g = p->mutable_gpu_diff();
  Dtype* h = history_[id]->mutable_gpu_data();
  const int64_t n = p->count();
  const size_t second = net_->learnable_params().size();  // update_history_offset
  switch (kind_) {
    case RRAM_SOLVER_SGD:
      RRAM_CALL(rram_sgd_update(g, h, n, hyper_.momentum, local, Caffe::stream()));
      break;
    case RRAM_SOLVER_NESTEROV:
      RRAM_CALL(rram_nesterov_update(g, h, n, hyper_.momentum, local, Caffe::stream()));
      break;
    case RRAM_SOLVER_ADAGRAD:
      RRAM_CALL(rram_adagrad_update(g, h, n, hyper_.delta, local, Caffe::stream()));
      break;
    case RRAM_SOLVER_RMSPROP:
      RRAM_CALL(rram_rmsprop_update(g, h, n, hyper_.momentum2, hyper_.delta, local, Caffe::stream()));
      break;
    case RRAM_SOLVER_ADADELTA:
      RRAM_CALL(rram_adadelta_update(g, h, history_[id + second]->mutable_gpu_data(), n, hyper_.momentum, hyper_.delta,
                                     local, Caffe::stream()));
      break;
    case RRAM_SOLVER_ADAM:
      RRAM_CALL(rram_adam_update(g, h, history_[id + second]->mutable_gpu_data(), n, hyper_.momentum, hyper_.momentum2,
                                 hyper_.delta, local, Caffe::stream()));
      break;
    default:
      throw Error("unknown solver kind");
  }
}

// sgd_solver.cpp:101-116 (Normalize for iter_size > 1 folded into a scale)
template <typename Dtype>
void Solver<Dtype>::ComputeUpdate() {
  const Dtype rate = GetLearningRate();
  ClipGradients();
  const int iter_size = (int)param_.integer("iter_size", 1);
  const auto& ps = net_->learnable_params();
  for (int i = 0; i < (int)ps.size(); ++i) {
    if (iter_size > 1) RRAM_CALL(rram_scal(ps[i]->count(), Dtype(1) / iter_size, ps[i]->mutable_gpu_diff(), Caffe::stream()));
    Regularize(i);
    ComputeUpdateValue(i, rate);
  }
}

// solver.cpp:25-33
template <typename Dtype>
void Solver<Dtype>::ApplyStrategy() {
  if (!fmaker_) return;
  for (auto& s : strategys_) s->Apply();
}

template <typename Dtype>
void Solver<Dtype>::ApplyUpdate() {
  net_->Update();
}

// Regularize(L2) + SGDUpdate + threshold + Update + Fail in
// one HBM pass per blob.  Same arithmetic sequence as the separate kernels.
template <typename Dtype>
void Solver<Dtype>::FusedTail() {
  const Dtype rate = GetLearningRate();
  const auto& ps = net_->learnable_params();
  const auto& fids = net_->failure_learnable_param_ids();
  const Dtype wd = (Dtype)param_.num("weight_decay", 0.0);
  // only reached when every configured strategy is a ThresholdFailureStrategy
  // and there is at most one (Step's can_fuse); anything else runs unfused
  ThresholdFailureStrategy<Dtype>* thr =
      strategys_.empty() ? nullptr : dynamic_cast<ThresholdFailureStrategy<Dtype>*>(strategys_[0].get());
  auto* gm = dynamic_cast<GaussianFailureMaker<Dtype>*>(fmaker_.get());
  std::vector<Blob<Dtype>*> fi = fmaker_ ? fmaker_->fail_iterations() : std::vector<Blob<Dtype>*>();
  // (cleared with the parameter diffs at the iteration's start, Step)
  unsigned long long* counts = fmaker_ ? fmaker_->device_counts() : nullptr;
  // one launch for all blobs (rram_fused_opt_update_fail_batched, SGD one kind
  // of its kernel like the others; a net with more learnable blobs than one
  // launch takes goes one launch per RRAM_MAX_SEGS)
  // The flipped kernels of the convolutions whose stride-1 data gradient
  // reads them (Layer::flip_geometry) come out of the same pass, for the next
  // iteration's backward within this Step call (Caffe::step_epoch); not while
  // a graph is captured.  They replace a flip launch per layer per iteration.
  const uint64_t epoch = Caffe::step_epoch();
  struct Flip {
    SyncedMemory* m;
    int g, ci, co, t;
  };
  std::vector<Flip> flips;
  if (flip_cache_ && epoch != 0 && !stream_capturing())
    for (const auto& l : net_->layers()) {
      Flip f{};
      if (!l->blobs().empty() && l->flip_geometry(&f.g, &f.ci, &f.co, &f.t)) {
        f.m = l->blobs()[0]->data().get();
        flips.push_back(f);
      }
    }
  std::vector<SyncedMemory*> flipped;
  const bool two = kind_ == RRAM_SOLVER_ADADELTA || kind_ == RRAM_SOLVER_ADAM;
  std::vector<rram_opt_seg> segs;
  for (int i = 0; i < (int)ps.size(); ++i) {
    int f = -1;
    for (int k = 0; k < (int)fids.size(); ++k)
      if (fids[k] == i) f = k;
    const bool faulty = gm && f >= 0;
    rram_opt_seg sg{};
    sg.w = ps[i]->mutable_gpu_data();
    sg.g = ps[i]->mutable_gpu_diff();
    sg.h = history_[i]->mutable_gpu_data();
    sg.endurance = faulty ? fi[f]->mutable_gpu_data() : nullptr;
    sg.values = faulty ? fi[f]->gpu_diff() : nullptr;
    sg.n = ps[i]->count();
    sg.decay = wd * net_->params_weight_decay()[i];
    sg.local_rate = LocalRate(i, rate);
    sg.apply_thr = (faulty && thr) ? 1 : 0;
    sg.thr = (faulty && thr) ? thr->threshold_for(f) : 0.0f;
    sg.broken_count = (faulty && counts) ? counts + f : nullptr;
    for (const Flip& fl : flips)
      if (fl.m == ps[i]->data().get() && (int64_t)fl.g * fl.ci * fl.co * fl.t == sg.n) {
        sg.w_flip = static_cast<float*>(fl.m->wflip(static_cast<size_t>(sg.n) * sizeof(Dtype)));
        sg.flip_groups = fl.g;
        sg.flip_cin = fl.ci;
        sg.flip_cout = fl.co;
        sg.flip_taps = fl.t;
        flipped.push_back(fl.m);
        break;
      }
    if (two) sg.h2 = history_[i + ps.size()]->mutable_gpu_data();
    segs.push_back(sg);
  }
  for (size_t b = 0; b < segs.size(); b += RRAM_MAX_SEGS)
    RRAM_CALL(rram_fused_opt_update_fail_batched(segs.data() + b, (int)std::min<size_t>(RRAM_MAX_SEGS, segs.size() - b),
                                                 kind_, &hyper_, gm ? gm->decrement : 100.0f,
                                                 gm ? gm->epsilon : 1e-20f, Caffe::stream()));
  for (SyncedMemory* m : flipped) m->set_wflip_valid(epoch);
}

template <typename Dtype>
void Solver<Dtype>::drop_graphs() {
  for (auto& g : captured_) g.drop();
  graph_warm_ = false;
  graph_ptrs_.clear();
}

template <typename Dtype>
void Solver<Dtype>::set_graph(bool on) {
  if (on)
    for (const auto& l : net_->layers()) {
      const std::string t = l->type();
      CAFFE_CHECK(t != "Dropout" && t != "HDF5Data",
                  "Solver graph replay: " << l->name() << " (" << t << ") changes per iteration on the host");
    }
  else
    drop_graphs();
  graph_ = on;
}

// the device pointers a captured iteration depends on
template <typename Dtype>
std::vector<const void*> Solver<Dtype>::graph_key() const {
  std::vector<const void*> k;
  for (const auto& b : net_->blobs()) {
    k.push_back(b->data()->gpu_data());
    k.push_back(b->diff()->gpu_data());
  }
  for (auto* p : net_->learnable_params()) {
    k.push_back(p->data()->gpu_data());
    k.push_back(p->diff()->gpu_data());
  }
  for (const auto& h : history_) k.push_back(h->data()->gpu_data());
  if (fmaker_) {
    for (auto* b : fmaker_->fail_iterations()) {
      k.push_back(b->data()->gpu_data());
      k.push_back(b->diff()->gpu_data());
    }
    k.push_back(fmaker_->device_counts());
  }
  append_graph_key_tail(k);
  return k;
}

// graph k (0: clear + forward + backward, 1: the fused tail): captured from
// body() on first use, then launched
template <typename Dtype>
template <typename F>
void Solver<Dtype>::capture_launch(int k, F&& body) {
  hipStream_t st = Caffe::hip_stream();
  if (!captured_[k].ready()) captured_[k].capture(st, body);
  captured_[k].launch(st);
}

// solver.cpp:237-325 (fork order: ComputeUpdate -> ApplyStrategy -> ApplyUpdate -> Fail)
template <typename Dtype>
void Solver<Dtype>::Step(int iters) {
  // a fresh Caffe::step_epoch for this call (the flipped-kernel companions
  // written by its updates are read only within it), 0 again on the way out
  struct EpochScope {
    EpochScope() {
      static std::atomic<uint64_t> next{0};
      Caffe::set_step_epoch(++next);
    }
    ~EpochScope() { Caffe::set_step_epoch(0); }
  } epoch_scope;
  const int stop = iter_ + iters;
  const int display = (int)param_.integer("display", 0);
  const int test_interval = (int)param_.integer("test_interval", 0);
  const int average_loss = (int)param_.integer("average_loss", 1);
  const int iter_size = (int)param_.integer("iter_size", 1);
  const long long snap = param_.integer("snapshot", 0);  // solver.cpp:312-318
  // The fused tail folds Regularize(L2) + SGDUpdate + threshold + Update +
  // Fail into one pass; remapping / genetic strategies (and more than one
  // strategy) need the reference order ComputeUpdate -> ApplyStrategy ->
  // ApplyUpdate -> Fail (solver.cpp:300-305), so they disable fusion.
  bool fusable_strategies = strategys_.size() <= 1;
  for (auto& st : strategys_)
    fusable_strategies = fusable_strategies && dynamic_cast<ThresholdFailureStrategy<Dtype>*>(st.get()) != nullptr;
  const bool can_fuse = fused_update_ && fusable_strategies && param_.num("clip_gradients", -1.0) < 0 &&
                        iter_size == 1 && param_.str("regularization_type", "L2") == "L2";
  // the fused tail's Fail counters are cleared with the parameter diffs (one launch)
  unsigned long long* fail_counts = can_fuse && fmaker_ ? fmaker_->device_counts() : nullptr;
  const int64_t n_fail_counts = fail_counts ? static_cast<int64_t>(fmaker_->fail_iterations().size()) : 0;
  while (iter_ < stop) {
    const bool test_now =
        test_interval && iter_ % test_interval == 0 && (iter_ > 0 || param_.boolean("test_initialization", true));
    const bool disp = display && iter_ % display == 0;
    // (a learning rate that moves every iteration, e.g. lr_policy "inv",
    // keeps the eager path: a graph is only worth its capture when replayed)
    // (Adam's bias correction moves its rate every iteration in the same way:
    // the corrected rate is the rate here, so Adam stays eager until the
    // correction has converged in fp32)
    const Dtype rate_now =
        graph_ ? (kind_ == RRAM_SOLVER_ADAM ? GetLearningRate() * AdamCorrection() : GetLearningRate()) : Dtype(0);
    const bool rate_stable = rate_now == graph_prev_rate_;
    graph_prev_rate_ = rate_now;
    if (graph_ && rate_stable && can_fuse && !test_now && !disp && average_loss <= 1 && !net_->on_backward_layer &&
        !net_->timing_on()) {
      // the first such iteration runs eager (workspaces and scratch buffers
      // get allocated on the section's stream), the next one captures
      const Dtype rate = rate_now;
      bool warm = graph_warm_;
      net_->set_iter((uint64_t)iter_);
      {
        GraphStreamScope sc(gstream_);
        // a new rate recaptures now; a key changed since the capture -- or
        // since the eager warm-up iteration -- means freed / reallocated
        // scratch: this iteration then runs eager again (rebuilding tables,
        // growing buffers outside any capture) and the next one captures
        const bool moved = warm && graph_key() != graph_ptrs_;
        if (captured_[0].ready() && (rate != graph_rate_ || moved)) drop_graphs();
        if (moved) warm = false;
        auto fb = [&] {
          net_->ClearParamDiffs(fail_counts, n_fail_counts);
          net_->Forward(false);
          net_->Backward();
        };
        if (warm)
          capture_launch(0, fb);
        else
          fb();
      }
      if (on_gradients_ready) on_gradients_ready();  // on the caller's stream, after the section
      {
        GraphStreamScope sc(gstream_);
        if (warm) {
          capture_launch(1, [&] { FusedTail(); });
          graph_rate_ = rate;
          // a replayed update rewrote the weights without FusedTail's host
          // side: no flipped kernel written before it is current
          for (auto* p : net_->learnable_params()) p->data()->drop_wflip();
        } else {
          FusedTail();
        }
        graph_ptrs_ = graph_key();  // the scratch this iteration ran (or was captured) with
      }
      graph_warm_ = true;
      ++iter_;
      if (snap && iter_ % snap == 0) Snapshot();
      continue;
    }
    net_->ClearParamDiffs(fail_counts, n_fail_counts);
    if (test_now) TestAll();
    net_->set_iter((uint64_t)iter_);
    Dtype loss = 0;
    for (int i = 0; i < iter_size; ++i) {
      loss += net_->Forward(disp || average_loss > 1);
      net_->Backward();
    }
    loss /= iter_size;
    if (disp || average_loss > 1) {
      if ((int)losses_.size() < average_loss) {
        losses_.push_back(loss);
        smoothed_loss_ = (smoothed_loss_ * (losses_.size() - 1) + loss) / losses_.size();
      } else {
        const int idx = iter_ % average_loss;
        smoothed_loss_ += (loss - losses_[idx]) / average_loss;
        losses_[idx] = loss;
      }
    }
    if (disp) {
      std::ostringstream o;
      o << "Iteration " << iter_ << ", loss = " << smoothed_loss_;
      emit(o.str());
    }
    if (on_gradients_ready) on_gradients_ready();
    if (can_fuse) {
      FusedTail();
    } else {
      ComputeUpdate();
      ApplyStrategy();
      ApplyUpdate();
      Fail(iter_);
    }
    ++iter_;
    if (snap && iter_ % snap == 0) Snapshot();
  }
}

template <typename Dtype>
void Solver<Dtype>::Solve(const char* resume_file) {
  if (resume_file) {
    emit(std::string("Restoring previous solver status from ") + resume_file);
    Restore(resume_file);
  }
  const int max_iter = (int)param_.integer("max_iter", 0);
  Step(max_iter - iter_);
  // solver.cpp:345-350 (only with a snapshot_prefix: the reference would write
  // "_iter_N.caffemodel" into the working directory without one)
  const long long snap = param_.integer("snapshot", 0);
  if (param_.has("snapshot_prefix") && param_.boolean("snapshot_after_train", true) && (!snap || iter_ % snap != 0))
    Snapshot();
  if (param_.integer("display", 0) && max_iter % std::max<long long>(1, param_.integer("display", 1)) == 0) {
    std::ostringstream o;
    o << "Iteration " << iter_ << ", loss = " << smoothed_loss_;
    emit(o.str());
  }
  const int ti = (int)param_.integer("test_interval", 0);
  if (ti && iter_ % ti == 0) TestAll();
  emit("Optimization Done.");
}

// solver.cpp:461-495 + sgd_solver.cpp:249-305: weights then solver state, as
// binary proto (.caffemodel / .solverstate) or HDF5 (.caffemodel.h5 /
// .solverstate.h5); the fault maps go to <prefix>_iter_N.faultstate either way
template <typename Dtype>
std::string Solver<Dtype>::Snapshot() {
  const std::string fmt = param_.str("snapshot_format", "BINARYPROTO");
  CAFFE_CHECK(fmt == "BINARYPROTO" || fmt == "HDF5", "Unsupported snapshot format " << fmt);
  const bool diff = param_.boolean("snapshot_diff", false);
  std::string state;
  if (fmt == "HDF5") {
    const std::string model = SnapshotFilename(".caffemodel.h5");
    emit("Snapshotting to HDF5 file " + model);
    net_->ToHDF5(model, diff);
    state = SnapshotFilename(".solverstate.h5");
    emit("Snapshotting solver state to HDF5 file " + state);
    h5::Handle f = h5::create_file(state);
    h5::save_int(f.id(), "iter", iter_);
    h5::save_string(f.id(), "learned_net", model);
    h5::save_int(f.id(), "current_step", current_step_);
    h5::Handle hg = h5::create_group(f.id(), "history");
    for (size_t i = 0; i < history_.size(); ++i) {
      const BlobProtoData p = BlobToProto(history_[i].get(), false);
      h5::save_floats(hg.id(), std::to_string(i),
                      std::vector<int64_t>(history_[i]->shape().begin(), history_[i]->shape().end()), p.data.data());
    }
  } else {
    const std::string model = SnapshotFilename(".caffemodel");
    emit("Snapshotting to binary proto file " + model);
    WriteFileBytes(model, SerializeNetParameter(net_->ToProto(diff)));
    SolverStateData st;
    st.iter = iter_;
    st.learned_net = model;
    st.current_step = current_step_;
    for (auto& h : history_) st.history.push_back(BlobToProto(h.get(), false));
    state = SnapshotFilename(".solverstate");
    emit("Snapshotting solver state to binary proto file " + state);
    WriteFileBytes(state, SerializeSolverState(st));
  }
  if (fmaker_) {
    std::vector<BlobProtoData> fs;
    for (auto* b : fmaker_->fail_iterations()) fs.push_back(BlobToProto(b, true));  // data = e, diff = v
    WriteFileBytes(SnapshotFilename(".faultstate"), SerializeBlobProtoVector(fs));
  }
  return state;
}

static bool ends_with(const std::string& s, const std::string& suf) {
  return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

// solver.cpp:520-530 + sgd_solver.cpp:307-351
template <typename Dtype>
void Solver<Dtype>::Restore(const std::string& state_file) {
  std::string fault_file;
  if (ends_with(state_file, ".h5")) {
    h5::Handle f = h5::open_file(state_file);
    iter_ = h5::load_int(f.id(), "iter");
    if (h5::dataset_exists(f.id(), "learned_net")) net_->CopyTrainedLayersFrom(h5::load_string(f.id(), "learned_net"));
    current_step_ = h5::load_int(f.id(), "current_step");
    h5::Handle hg = h5::open_group(f.id(), "history");
    CAFFE_CHECK(h5::num_links(hg.id()) == (int)history_.size(), "Incorrect length of history blobs.");
    for (size_t i = 0; i < history_.size(); ++i) {
      std::vector<int64_t> dims;
      BlobProtoData p;
      p.data = h5::load_floats(hg.id(), std::to_string(i), &dims);
      CAFFE_CHECK((int64_t)p.data.size() == history_[i]->count(), "history blob " << i << ": size mismatch");
      BlobFromProto(history_[i].get(), p);
    }
    if (ends_with(state_file, ".solverstate.h5"))
      fault_file = state_file.substr(0, state_file.size() - 15) + ".faultstate";
  } else {
    const SolverStateData st = ParseSolverState(ReadFileBytes(state_file));
    iter_ = st.iter;
    if (!st.learned_net.empty()) net_->CopyTrainedLayersFrom(st.learned_net);
    current_step_ = st.current_step;
    CAFFE_CHECK(st.history.size() == history_.size(), "Incorrect length of history blobs.");
    for (size_t i = 0; i < history_.size(); ++i) {
      CAFFE_CHECK(ShapeEquals(history_[i]->shape(), st.history[i]), "history blob " << i << ": shape mismatch");
      BlobFromProto(history_[i].get(), st.history[i]);
    }
    if (ends_with(state_file, ".solverstate"))
      fault_file = state_file.substr(0, state_file.size() - 12) + ".faultstate";
  }
  if (fmaker_ && !fault_file.empty()) {
    std::ifstream probe(fault_file, std::ios::binary);
    if (probe.good()) {
      const auto fs = ParseBlobProtoVector(ReadFileBytes(fault_file));
      auto fi = fmaker_->fail_iterations();
      CAFFE_CHECK(fs.size() == fi.size(), "fault state: " << fs.size() << " blobs, net has " << fi.size());
      for (size_t i = 0; i < fi.size(); ++i) {
        CAFFE_CHECK(ShapeEquals(fi[i]->shape(), fs[i]) && !fs[i].diff.empty(), "fault state blob " << i << ": mismatch");
        BlobFromProto(fi[i], fs[i]);
      }
      emit("Restored fault state from " + fault_file);
    }
  }
}

template <typename Dtype>
std::vector<std::vector<Dtype>> Solver<Dtype>::TestAll() {
  std::vector<std::vector<Dtype>> r;
  for (int i = 0; i < (int)test_nets_.size(); ++i) r.push_back(Test(i));
  return r;
}

// solver.cpp:385-458: mean over test_iter of every output element
template <typename Dtype>
std::vector<Dtype> Solver<Dtype>::Test(int id) {
  CAFFE_CHECK(id >= 0 && id < (int)test_nets_.size(), "test net index out of range");
  auto tn = test_nets_[id];
  auto ti = param_.nums("test_iter");
  const int iters = ti.empty() ? 1 : (int)ti[std::min<size_t>(id, ti.size() - 1)];
  std::vector<Dtype> score;
  Dtype loss = 0;
  for (int it = 0; it < iters; ++it) {
    loss += tn->Forward(true);
    int k = 0;
    for (auto* b : tn->output_blobs()) {
      std::vector<Dtype> h(b->count());
      HIP_CALL(hipMemcpyAsync(h.data(), b->gpu_data(), b->count() * sizeof(Dtype), hipMemcpyDeviceToHost,
                              Caffe::hip_stream()));
      HIP_CALL(hipStreamSynchronize(Caffe::hip_stream()));
      for (Dtype v : h) {
        if (it == 0) score.push_back(v);
        else score[k] += v;
        ++k;
      }
    }
  }
  for (auto& s : score) s /= iters;
  std::ostringstream o;
  o << "Iteration " << iter_ << ", Testing net (#" << id << ")";
  emit(o.str());
  int k = 0;
  for (size_t j = 0; j < tn->output_blobs().size(); ++j) {
    const int bid = tn->output_blob_indices()[j];
    const float lw = tn->blob_loss_weights()[bid];
    for (int64_t e = 0; e < tn->output_blobs()[j]->count(); ++e, ++k) {
      std::ostringstream l;
      l << "    Test net output #" << k << ": " << tn->blob_names()[bid] << " = " << score[k];
      if (lw) l << " (* " << lw << " = " << lw * score[k] << " loss)";
      emit(l.str());
    }
  }
  return score;
}

template class Solver<float>;

}  // namespace caffe
