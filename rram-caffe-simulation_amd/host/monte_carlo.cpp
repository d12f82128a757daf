#include "monte_carlo.hpp"

#include "layers.hpp"

#include <algorithm>
#include <cstdlib>
#include <set>
#include <string>

// Constants of the injection overlap (see the constructor;
// profiles/r05_ab_mc_overlap.txt).
// the injection is released after this many convolutions (0: with the prefix)
constexpr int kReleaseAfterConv = 2;
// overlapped, the injection gets a 256-block grid (it shares the CUs);
// serial, the default 2048
constexpr int kOverlapGrid = 256;

namespace caffe {

// call(first segment, segment count, index of the first) per RRAM_MAX_SEGS segments
template <typename F>
static void for_seg_chunks(const std::vector<rram_inject_seg>& segs, F&& call) {
  for (size_t s = 0; s < segs.size(); s += RRAM_MAX_SEGS)
    call(segs.data() + s, static_cast<int>(std::min<size_t>(RRAM_MAX_SEGS, segs.size() - s)), s);
}

// ============================================================ MonteCarlo
template <typename Dtype>
MonteCarlo<Dtype>::MonteCarlo(std::shared_ptr<Net<Dtype>> net, const std::vector<rram_inject_cfg>& cfgs,
                              uint64_t seed, int max_maps)
    : net_(net), seed_(seed), max_maps_(max_maps) {
  params_ = net_->failure_learnable_params();
  CAFFE_CHECK(!params_.empty(), "MonteCarlo: the net has no faultable (InnerProduct) parameters");
  CAFFE_CHECK(cfgs.size() == 1 || cfgs.size() == params_.size(),
              "MonteCarlo: give one inject config or one per faultable blob (" << params_.size() << ")");
  cfgs_ = cfgs;
  if (cfgs_.size() == 1) cfgs_.resize(params_.size(), cfgs[0]);
  for (auto* p : params_) {
    Dtype* c = nullptr;
    HIP_CALL(hipMalloc(reinterpret_cast<void**>(&c), p->count() * sizeof(Dtype)));
    HIP_CALL(hipMemcpyAsync(c, p->gpu_data(), p->count() * sizeof(Dtype), hipMemcpyDeviceToDevice, Caffe::hip_stream()));
    clean_.push_back(c);
  }
  for (auto* b : net_->output_blobs())
    if (b->count() == 1) outs_.push_back(b);
  const size_t no = n_out_alloc();
  HIP_CALL(hipMalloc(reinterpret_cast<void**>(&d_sums_), no * sizeof(Dtype)));
  HIP_CALL(hipMalloc(reinterpret_cast<void**>(&d_per_map_), std::max(1, max_maps_) * no * sizeof(Dtype)));
  HIP_CALL(hipMalloc(reinterpret_cast<void**>(&d_broken_), params_.size() * sizeof(unsigned long long)));
  const auto& fl = net_->failure_learnable_layer_ids();
  first_fault_layer_ = *std::min_element(fl.begin(), fl.end());
  // RRAM_MC_OVERLAP=1 runs each map's injection on a side stream under the
  // layers before the first faultable one, released after the second
  // convolution (the persistent conv1 kernel holds every CU; conv2, the
  // dominant kernel, keeps the chip to itself) on a 256-block grid.  Off by
  // default: the injection shares the CUs with norm2 / pool2 / conv3 and
  // stretches from 89 to ~310 us, conv3 from 0.303 to 0.375 ms, and the live
  // bench measured serial 0.2-1.1 % ahead (profiles/r05_ab_mc_overlap.txt;
  // with per-layer events the overlap had led by 1.2 %).  The graph replay
  // (set_graph) is serial either way.
  {
    const char* e = getenv("RRAM_MC_OVERLAP");
    overlap_ = e && atoi(e) == 1 && first_fault_layer_ > 0;
  }
  release_after_ = -1;  // no such convolution: the injection starts with the prefix
  for (int i = 0, n = 0; kReleaseAfterConv && i < first_fault_layer_ - 1; ++i)
    if (std::string(net_->layers()[i]->type()) == "Convolution" && ++n == kReleaseAfterConv) {
      release_after_ = i;
      break;
    }
  // between maps only the injection rewrites weights: the convolutions keep
  // their packed weights (Net::set_weight_pack_cache) unless a faultable blob
  // is theirs (the conv-fault extension), which every map's mutable access
  // invalidates, or a caller was handed the weights' pointer (SyncedMemory::expose)
  net_->set_weight_pack_cache(true);
  if (overlap_) {
    HIP_CALL(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
    HIP_CALL(hipEventCreateWithFlags(&ev_free_, hipEventDisableTiming));
    HIP_CALL(hipEventCreateWithFlags(&ev_injected_, hipEventDisableTiming));
  }
  Reset();
}

template <typename Dtype>
MonteCarlo<Dtype>::~MonteCarlo() {
  try {
    RestoreClean();
    net_->set_weight_pack_cache(false);
    Caffe::synchronize();
  } catch (...) {
  }
  drop_graph();
  if (d_state_) (void)hipFree(d_state_);
  try {
    apply_map_groups(1);
  } catch (...) {
  }
  for (auto* c : stacks_) (void)hipFree(c);
  for (auto* c : clean_) (void)hipFree(c);
  if (side_) {
    (void)hipStreamSynchronize(side_);
    (void)hipStreamDestroy(side_);
    (void)hipEventDestroy(ev_free_);
    (void)hipEventDestroy(ev_injected_);
  }
  (void)hipFree(d_sums_);
  (void)hipFree(d_per_map_);
  (void)hipFree(d_broken_);
}

template <typename Dtype>
void MonteCarlo<Dtype>::Reset() {
  maps_run_ = 0;
  if (d_state_) HIP_CALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state_ + 1), 0, 1, Caffe::hip_stream()));
  HIP_CALL(hipMemsetAsync(d_sums_, 0, n_out_alloc() * sizeof(Dtype), Caffe::hip_stream()));
  HIP_CALL(hipMemsetAsync(d_broken_, 0, params_.size() * sizeof(unsigned long long), Caffe::hip_stream()));
}

template <typename Dtype>
void MonteCarlo<Dtype>::RestoreClean() {
  for (size_t i = 0; i < params_.size(); ++i)
    HIP_CALL(hipMemcpyAsync(params_[i]->mutable_gpu_data(), clean_[i], params_[i]->count() * sizeof(Dtype),
                            hipMemcpyDeviceToDevice, Caffe::hip_stream()));
}

template <typename Dtype>
std::vector<rram_inject_seg> MonteCarlo<Dtype>::inject_segs(bool into_stacks) const {
  std::vector<rram_inject_seg> segs(params_.size());
  for (size_t i = 0; i < params_.size(); ++i)
    segs[i] = rram_inject_seg{clean_[i], into_stacks ? stacks_[i] : params_[i]->mutable_gpu_data(),
                              params_[i]->count(), (uint32_t)i, 0, cfgs_[i]};
  return segs;
}

template <typename Dtype>
int MonteCarlo<Dtype>::producer_of(const Blob<Dtype>* b) const {
  const auto& tops = net_->top_vecs();
  int prod = -1;
  for (size_t l = 0; l < net_->layers().size(); ++l)
    if (!tops[l].empty() && tops[l][0] == b) prod = static_cast<int>(l);
  return prod;
}

template <typename Dtype>
void MonteCarlo<Dtype>::set_reuse_prefix(bool on) {
  CAFFE_CHECK(!on || map_batch_ == 1, "MonteCarlo prefix reuse: not available while map batching is on (map_batch = "
                                          << map_batch_ << ")");
  if (on) {
    const auto& L = net_->layers();
    const auto& tops = net_->top_vecs();
    // compare the memory, not the Blob: Split, single-input Concat and
    // single-top Slice tops share their bottom's SyncedMemory (ShareData)
    std::set<const SyncedMemory*> prefix_mem;
    for (int i = 0; i < first_fault_layer_; ++i) {
      CAFFE_CHECK(std::string(L[i]->type()) != "HDF5Data",
                  "MonteCarlo prefix reuse: layer " << net_->layer_names()[i] << " (HDF5Data) advances between forwards");
      for (auto* b : tops[i]) prefix_mem.insert(b->data().get());
    }
    for (size_t i = first_fault_layer_; i < L.size(); ++i) {
      // Split / Concat / Slice tops that share a prefix blob's memory are
      // views of it, not writes (they write only into memory of their own)
      const std::string t = L[i]->type();
      if (t == "Split" || t == "Concat" || t == "Slice") continue;
      for (auto* b : tops[i])
        CAFFE_CHECK(!prefix_mem.count(b->data().get()), "MonteCarlo prefix reuse: layer " << net_->layer_names()[i]
                                                << " writes a blob of the layers before the first faultable one");
    }
  }
  reuse_prefix_ = on;
  prefix_done_ = false;  // (re-)enabling recomputes the prefix on the next map
}

template <typename Dtype>
void MonteCarlo<Dtype>::drop_graph() {
  captured_.drop();
  graph_warm_ = false;
  graph_ptrs_.clear();
}

template <typename Dtype>
void MonteCarlo<Dtype>::set_graph(bool on) {
  CAFFE_CHECK(!on || map_batch_ == 1, "MonteCarlo graph replay: not available while map batching is on (map_batch = "
                                          << map_batch_ << ")");
  if (on) {
    for (const auto& l : net_->layers())
      CAFFE_CHECK(std::string(l->type()) != "HDF5Data",
                  "MonteCarlo graph replay: " << l->name() << " (HDF5Data) advances between forwards");
    if (!d_state_) {
      HIP_CALL(hipMalloc(reinterpret_cast<void**>(&d_state_), 2 * sizeof(uint32_t)));
      HIP_CALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state_), 0, 1, Caffe::hip_stream()));
      HIP_CALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state_ + 1), maps_run_, 1, Caffe::hip_stream()));
    }
  } else {
    drop_graph();
  }
  graph_ = on;
}

// the device pointers a captured map depends on: every blob's and
// parameter's data and diff (a reshape or a set_gpu_data moves them), the
// clean copies and the statistics buffers
template <typename Dtype>
std::vector<const void*> MonteCarlo<Dtype>::graph_key() const {
  std::vector<const void*> k;
  for (const auto& b : net_->blobs()) k.push_back(b->data()->gpu_data());
  for (auto* p : net_->learnable_params()) {
    k.push_back(p->data()->gpu_data());
    k.push_back(static_cast<const void*>(p));
  }
  for (auto* c : clean_) k.push_back(c);
  k.push_back(d_sums_);
  k.push_back(d_per_map_);
  k.push_back(d_broken_);
  append_graph_key_tail(k);
  return k;
}

// One map on the working stream, the way the graph path warms up with,
// captures and replays it: injection with the map id from d_state_[0], the
// whole forward, the statistics into row d_state_[1], which then advances
// together with the map id.
template <typename Dtype>
void MonteCarlo<Dtype>::device_state_map() {
  for_seg_chunks(inject_segs(false), [&](const rram_inject_seg* seg, int k, size_t s) {
    RRAM_CALL(rram_inject_rng_batched_dev(seg, k, seed_, d_state_, d_broken_ + s, Caffe::stream()));
  });
  net_->Forward(false);
  const size_t no = outs_.size();
  if (no == 0) {  // still advance the map id and the row
    rram_mc_outputs mo{};
    RRAM_CALL(rram_mc_accumulate_dev(&mo, d_sums_, nullptr, 1, 0, reinterpret_cast<int*>(d_state_ + 1), d_state_, 1,
                                     Caffe::stream()));
  }
  for (size_t k0 = 0; k0 < no; k0 += RRAM_MC_MAX_OUTPUTS) {
    rram_mc_outputs mo{};
    mo.n = static_cast<int>(std::min<size_t>(RRAM_MC_MAX_OUTPUTS, no - k0));
    for (int k = 0; k < mo.n; ++k) mo.p[k] = outs_[k0 + k]->gpu_data();
    RRAM_CALL(rram_mc_accumulate_dev(&mo, d_sums_ + k0, d_per_map_ + k0, static_cast<int64_t>(no), max_maps_,
                                     reinterpret_cast<int*>(d_state_ + 1), d_state_,
                                     k0 + RRAM_MC_MAX_OUTPUTS >= no ? 1 : 0, Caffe::stream()));
  }
}

// ------------------------------------------------------------ map batching
// hand every layer its group count and, for its faulted blobs, their stacks
template <typename Dtype>
void MonteCarlo<Dtype>::apply_map_groups(int K) {
  const auto& L = net_->layers();
  std::string refused;
  for (size_t l = 0; l < L.size(); ++l) {
    const auto& bl = L[l]->blobs();
    std::vector<const Dtype*> gp(bl.size() + 1, nullptr);
    std::vector<int64_t> st(bl.size() + 1, 0);
    for (size_t j = 0; K > 1 && j < bl.size(); ++j)
      for (size_t i = 0; i < params_.size(); ++i)
        if (params_[i] == bl[j].get() || params_[i]->data().get() == bl[j]->data().get()) {
          gp[j] = stacks_[i];
          st[j] = params_[i]->count();
        }
    const bool ok = L[l]->set_map_groups(K, gp.data(), st.data());
    const auto& fl = net_->failure_learnable_layer_ids();
    if (!ok && K > 1 && refused.empty() && std::find(fl.begin(), fl.end(), (int)l) != fl.end())
      refused = net_->layer_names()[l] + " (" + L[l]->type() + ")";
  }
  CAFFE_CHECK(refused.empty(), "MonteCarlo map batching: faultable layer " << refused << " has no map-group forward");
}

template <typename Dtype>
void MonteCarlo<Dtype>::set_map_batch(int K) {
  CAFFE_CHECK(K >= 1, "MonteCarlo map batching: map_batch must be >= 1 (got " << K << ")");
  if (K == map_batch_) return;
  // back to the sequential driver first (also the K -> K' path)
  apply_map_groups(1);
  map_batch_ = 1;
  Caffe::synchronize();
  for (auto* c : stacks_) (void)hipFree(c);
  stacks_.clear();
  if (K == 1) return;
  CAFFE_CHECK(!reuse_prefix_, "MonteCarlo map batching: prefix reuse is on (every map runs its own whole forward; "
                              "turn it off first)");
  CAFFE_CHECK(!graph_, "MonteCarlo map batching: graph replay is on (turn it off first)");
  const auto& L = net_->layers();
  const auto& tops = net_->top_vecs();
  const auto& bots = net_->bottom_vecs();
  for (int l : net_->failure_learnable_layer_ids())
    CAFFE_CHECK(std::string(L[l]->type()) != "Convolution",
                "MonteCarlo map batching: a faultable blob belongs to Convolution layer "
                    << net_->layer_names()[l] << " (the conv-fault extension is not batched)");
  for (size_t l = 0; l < L.size(); ++l) {
    if (!bots[l].empty()) continue;
    CAFFE_CHECK(std::string(L[l]->type()) != "HDF5Data",
                "MonteCarlo map batching: source layer " << net_->layer_names()[l]
                                                         << " (HDF5Data) advances between forwards");
    for (auto* t : tops[l])
      CAFFE_CHECK(t->num_axes() > 0 && t->shape(0) % K == 0,
                  "MonteCarlo map batching: the batch " << (t->num_axes() > 0 ? t->shape(0) : 0) << " of source layer "
                                                        << net_->layer_names()[l] << " is not divisible by map_batch "
                                                        << K << " (build the net at batch K x B)");
  }
  // the producers of the statistics must keep the groups apart
  for (auto* o : outs_) {
    const int prod = producer_of(o);
    CAFFE_CHECK(prod >= 0, "MonteCarlo map batching: an output has no producing layer");
    const std::string t = L[prod]->type();
    CAFFE_CHECK(t == "SoftmaxWithLoss" || t == "Accuracy",
                "MonteCarlo map batching: the statistic of layer " << net_->layer_names()[prod] << " (" << t
                    << ") mixes the images of a batch, so it cannot be split into map groups");
  }
  // batch invariance of the layers before the faultable ones: a convolution
  // whose plan is chosen from num may sum an image in another order at K * B
  // than at B.  The fp32 engine's split-K is pinned to the batch-B plan by
  // the grouped ConvolutionLayer (rram_set_conv_plan_num); the engine choice
  // and the octet plan must agree, else the K is refused
  for (size_t l = 0; l < L.size(); ++l) {
    auto* cv = dynamic_cast<ConvolutionLayer<Dtype>*>(L[l].get());
    if (cv == nullptr || bots[l].empty() || bots[l][0]->num_axes() != 4) continue;
    rram_conv_desc big = cv->desc();
    big.num = bots[l][0]->shape(0);
    big.height = bots[l][0]->shape(2);
    big.width = bots[l][0]->shape(3);
    rram_conv_desc one = big;
    one.num = big.num / K;
    bool same = big.num % K == 0 && rram_f32_engine_for_conv(&big) == rram_f32_engine_for_conv(&one);
    int pb[5] = {0, 0, 0, 0, 0}, po[5] = {0, 0, 0, 0, 0};
    const int hb = rram_conv_octet_plan(&big, pb), ho = rram_conv_octet_plan(&one, po);
    same = same && hb == ho && std::equal(pb, pb + 5, po);
    CAFFE_CHECK(same, "MonteCarlo map batching: convolution " << net_->layer_names()[l] << " takes a different plan at batch "
                                                              << big.num << " than at " << one.num
                                                              << ", so map_batch " << K
                                                              << " would not reproduce the sequential maps' bits");
  }
  try {
    for (auto* p : params_) {
      Dtype* c = nullptr;
      const hipError_t e = hipMalloc(reinterpret_cast<void**>(&c), (size_t)K * p->count() * sizeof(Dtype));
      CAFFE_CHECK(e == hipSuccess, "MonteCarlo map batching: allocating " << K << " copies of a faultable blob ("
                                                                           << (size_t)K * p->count() * sizeof(Dtype)
                                                                           << " bytes) failed: " << hipGetErrorString(e));
      stacks_.push_back(c);
      // the slices of a short first group are stale but defined: the clean weights
      for (int j = 0; j < K; ++j)
        HIP_CALL(hipMemcpyAsync(c + (size_t)j * p->count(), clean_[stacks_.size() - 1], p->count() * sizeof(Dtype),
                                hipMemcpyDeviceToDevice, Caffe::hip_stream()));
    }
    // K spare per-map rows: a group that straddles max_maps writes its rows unclipped
    const size_t no = n_out_alloc();
    Dtype* rows = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&rows), (size_t)(std::max(1, max_maps_) + K) * no * sizeof(Dtype));
    CAFFE_CHECK(e == hipSuccess, "MonteCarlo map batching: per-map rows allocation failed: " << hipGetErrorString(e));
    HIP_CALL(hipMemcpyAsync(rows, d_per_map_, (size_t)std::max(1, max_maps_) * no * sizeof(Dtype), hipMemcpyDeviceToDevice,
                            Caffe::hip_stream()));
    Caffe::synchronize();
    (void)hipFree(d_per_map_);
    d_per_map_ = rows;
    apply_map_groups(K);
  } catch (...) {
    try {
      apply_map_groups(1);
    } catch (...) {
    }
    (void)hipGetLastError();
    for (auto* c : stacks_) (void)hipFree(c);
    stacks_.clear();
    throw;
  }
  map_batch_ = K;
}

template <typename Dtype>
void MonteCarlo<Dtype>::TileInputs() {
  const int K = map_batch_;
  if (K == 1) return;
  const auto& tops = net_->top_vecs();
  const auto& bots = net_->bottom_vecs();
  for (size_t l = 0; l < tops.size(); ++l) {
    if (!bots[l].empty()) continue;
    for (auto* t : tops[l]) {
      CAFFE_CHECK(t->num_axes() > 0 && t->shape(0) % K == 0, "MonteCarlo TileInputs: batch not divisible by map_batch");
      const size_t slice = static_cast<size_t>(t->count() / K);
      Dtype* d = t->mutable_gpu_data();
      for (int j = 1; j < K; ++j)
        HIP_CALL(hipMemcpyAsync(d + j * slice, d, slice * sizeof(Dtype), hipMemcpyDeviceToDevice, Caffe::hip_stream()));
    }
  }
}

// Run with map_batch_ > 1: groups of K consecutive map ids, each one
// rram_inject_rng_maps launch per RRAM_MAX_SEGS blobs, one forward, and the
// statistics folded by the heads in map order
template <typename Dtype>
void MonteCarlo<Dtype>::run_groups(uint32_t map_begin, uint32_t map_count) {
  const int K = map_batch_;
  const size_t no = outs_.size();
  std::vector<Layer<Dtype>*> acc_layers;
  ClearAcc clear_acc{acc_layers};
  for (size_t k = 0; k < no; ++k) {
    const int l = producer_of(outs_[k]);
    Layer<Dtype>* prod = l >= 0 ? net_->layers()[l].get() : nullptr;
    CAFFE_CHECK(prod != nullptr && prod->set_top_accumulator(d_sums_ + k, nullptr, (int64_t)no, 0),
                "MonteCarlo map batching: an output's producer cannot fold the statistics");
    acc_layers.push_back(prod);
  }
  const std::vector<rram_inject_seg> segs = inject_segs(true);
  std::vector<int64_t> strides(params_.size());
  for (size_t i = 0; i < params_.size(); ++i) strides[i] = params_[i]->count();
  const int prev_grid = rram_set_inject_grid(0);
  for (uint32_t done = 0; done < map_count; done += K) {
    const int live = static_cast<int>(std::min<uint32_t>(K, map_count - done));
    for (size_t k = 0; k < no; ++k)
      acc_layers[k]->set_top_accumulator(d_sums_ + k,
                                         maps_run_ < max_maps_ ? d_per_map_ + (size_t)maps_run_ * no + k : nullptr,
                                         (int64_t)no, live);
    if (timing_) timer_.start(0, Caffe::hip_stream());
    for_seg_chunks(segs, [&](const rram_inject_seg* seg, int k, size_t s) {
      RRAM_CALL(rram_inject_rng_maps(seg, k, seed_, map_begin + done, live, strides.data() + s, d_broken_ + s,
                                     Caffe::stream()));
    });
    if (timing_) timer_.stop(0, Caffe::hip_stream());
    net_->Forward(false);
    maps_run_ += live;
  }
  rram_set_inject_grid(prev_grid);
  if (d_state_)
    HIP_CALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state_ + 1), maps_run_, 1, Caffe::hip_stream()));
}

template <typename Dtype>
void MonteCarlo<Dtype>::Run(uint32_t map_begin, uint32_t map_count) {
  if (map_batch_ > 1) {
    run_groups(map_begin, map_count);
    return;
  }
  if (graph_ && !reuse_prefix_ && !timing_ && !net_->timing_on() && map_count > 0) {
    GraphStreamScope sc(gstream_);
    hipStream_t st = Caffe::hip_stream();
    HIP_CALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state_), static_cast<int>(map_begin), 1, st));
    // the scratch moved since the capture -- or since the eager warm-up map
    // (a capture now would rebuild freed tables inside it): eager again
    if ((captured_.ready() || graph_warm_) && graph_key() != graph_ptrs_) drop_graph();
    for (uint32_t m = map_begin; m < map_begin + map_count; ++m) {
      if (!captured_.ready()) {
        if (!graph_warm_) {
          // eager first (every workspace and pack buffer gets allocated), on
          // the device-state path the graph will replay
          device_state_map();
          graph_warm_ = true;
          graph_ptrs_ = graph_key();
          ++maps_run_;
          continue;
        }
        // every cache the forward keeps across calls (octet companions,
        // packed weights) is dropped, so the captured map recomputes what it
        // reads and stays exact whatever the host-side cache state is later
        for (const auto& b : net_->blobs()) (void)b->mutable_gpu_data();
        for (auto* p : net_->learnable_params()) (void)p->mutable_gpu_data();
        captured_.capture(st, [&] { device_state_map(); });
        graph_ptrs_ = graph_key();
      }
      captured_.launch(st);
      ++maps_run_;
    }
    return;
  }
  if (d_state_)  // keep the device-side row in step with the eager maps
    HIP_CALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state_ + 1), maps_run_ + static_cast<int>(map_count),
                               1, Caffe::hip_stream()));
  const std::vector<rram_inject_seg> segs = inject_segs(false);
  const size_t no = outs_.size();
  const auto& layers = net_->layers();
  const int L = static_cast<int>(layers.size());
  const int prev_grid = rram_set_inject_grid(overlap_ && !reuse_prefix_ ? kOverlapGrid : 0);
  // the statistics folded into the layers that store each scalar output
  // (Layer::set_top_accumulator): no rram_mc_accumulate launch per map when
  // every output's producer takes it (all or none)
  std::vector<Layer<Dtype>*> acc_layers;
  ClearAcc clear_acc{acc_layers};
  for (size_t k = 0; k < no; ++k) {
    const int prod = producer_of(outs_[k]);
    // a producer inside the reused prefix runs on the first map only: its
    // constant output is then accumulated by rram_mc_accumulate every map
    const bool in_prefix = reuse_prefix_ && prod < first_fault_layer_;
    if (prod < 0 || in_prefix || !layers[prod]->set_top_accumulator(d_sums_ + k, nullptr)) {
      for (auto* a : acc_layers) a->set_top_accumulator(nullptr, nullptr);
      acc_layers.clear();
      break;
    }
    acc_layers.push_back(layers[prod].get());
  }
  for (uint32_t m = map_begin; m < map_begin + map_count; ++m) {
    for (size_t k = 0; k < acc_layers.size(); ++k)
      acc_layers[k]->set_top_accumulator(d_sums_ + k, maps_run_ < max_maps_ ? d_per_map_ + (size_t)maps_run_ * no + k
                                                                            : nullptr);
    if (m != map_begin)
      for (auto* p : params_) (void)p->mutable_gpu_data();
    hipStream_t is = Caffe::hip_stream();
    const bool skip_prefix = reuse_prefix_ && prefix_done_ && first_fault_layer_ > 0;
    const bool overlap = overlap_ && !skip_prefix;
    if (overlap) {
      // released after the second convolution (see the constructor)
      if (release_after_ >= 0) net_->ForwardFromTo(0, release_after_, false);
      HIP_CALL(hipEventRecord(ev_free_, Caffe::hip_stream()));  // previous map's forward is done with the weights
      HIP_CALL(hipStreamWaitEvent(side_, ev_free_, 0));
      is = side_;
    }
    if (timing_) timer_.start(0, is);
    for_seg_chunks(segs, [&](const rram_inject_seg* seg, int k, size_t s) {
      RRAM_CALL(rram_inject_rng_batched(seg, k, seed_, m, d_broken_ + s, is));
    });
    if (timing_) timer_.stop(0, is);
    if (overlap) {
      HIP_CALL(hipEventRecord(ev_injected_, side_));
      net_->ForwardFromTo(release_after_ + 1, first_fault_layer_ - 1, false);  // the rest of the prefix runs under the injection
      HIP_CALL(hipStreamWaitEvent(Caffe::hip_stream(), ev_injected_, 0));
      net_->ForwardFromTo(first_fault_layer_, L - 1, false);
    } else if (skip_prefix) {
      net_->ForwardFromTo(first_fault_layer_, L - 1, false);  // the prefix's blobs hold the first map's bits
    } else {
      net_->Forward(false);
    }
    if (reuse_prefix_) prefix_done_ = true;
    for (size_t k0 = 0; acc_layers.empty() && k0 < no; k0 += RRAM_MC_MAX_OUTPUTS) {
      rram_mc_outputs mo{};
      mo.n = static_cast<int>(std::min<size_t>(RRAM_MC_MAX_OUTPUTS, no - k0));
      for (int k = 0; k < mo.n; ++k) mo.p[k] = outs_[k0 + k]->gpu_data();
      RRAM_CALL(rram_mc_accumulate(&mo, d_sums_ + k0,
                                   maps_run_ < max_maps_ ? d_per_map_ + (size_t)maps_run_ * no + k0 : nullptr,
                                   Caffe::stream()));
    }
    ++maps_run_;
  }
  rram_set_inject_grid(prev_grid);
}

template <typename Dtype>
void MonteCarlo<Dtype>::Stats(std::vector<double>& outputs, std::vector<unsigned long long>& broken,
                              std::vector<float>& per_map) const {
  const size_t no = outs_.size();
  std::vector<Dtype> s(no);
  broken.assign(params_.size(), 0);
  const int pm = std::min(maps_run_, max_maps_);
  per_map.assign((size_t)pm * no, 0.f);
  if (no) HIP_CALL(hipMemcpyAsync(s.data(), d_sums_, no * sizeof(Dtype), hipMemcpyDeviceToHost, Caffe::hip_stream()));
  HIP_CALL(hipMemcpyAsync(broken.data(), d_broken_, broken.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          Caffe::hip_stream()));
  if (pm && no)
    HIP_CALL(hipMemcpyAsync(per_map.data(), d_per_map_, per_map.size() * sizeof(float), hipMemcpyDeviceToHost,
                            Caffe::hip_stream()));
  HIP_CALL(hipStreamSynchronize(Caffe::hip_stream()));
  outputs.assign(s.begin(), s.end());
}

template class MonteCarlo<float>;

}  // namespace caffe
