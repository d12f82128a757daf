// The Monte-Carlo fault-map driver.
//
//   MonteCarlo — the reference's one-map-per-run fault-injected Test
//        generalised to many maps per launch sequence.
#pragma once

#include <algorithm>
#include <memory>
#include <vector>

#include "graph.hpp"
#include "net.hpp"

namespace caffe {

// Monte-Carlo fault-map inference (north_star).
// For every map m: inject(clean IP weights -> net weights) with the counter
// RNG keyed by (seed, m, blob), forward the TEST net, accumulate its outputs
// (accuracy, loss) and the per-blob broken-cell counts on the device.
template <typename Dtype>
class MonteCarlo {
 public:
  MonteCarlo(std::shared_ptr<Net<Dtype>> net, const std::vector<rram_inject_cfg>& cfgs, uint64_t seed,
             int max_maps);
  ~MonteCarlo();
  void Run(uint32_t map_begin, uint32_t map_count);
  void Reset();
  // sums over the maps run so far: outputs[n_outputs] (each output's mean over
  // its elements), broken[n_fault_blobs], per_map[maps_run][n_outputs]
  void Stats(std::vector<double>& outputs, std::vector<unsigned long long>& broken,
             std::vector<float>& per_map) const;
  int maps_run() const { return maps_run_; }
  int num_outputs() const { return static_cast<int>(outs_.size()); }
  void RestoreClean();
  // hipEvent timing of the injection launches (key 0)
  void set_timing(bool on) { timing_ = on; }
  // Prefix reuse (opt-in; a different workload from the reference's, which
  // runs every map's whole forward): under reference semantics only the
  // InnerProduct blobs are faulted, so the layers before the first faultable
  // one compute the same bits for every map of a fixed input batch.  On, the
  // next map runs them once and the following maps start at the first
  // faultable layer.  Refused when a source layer advances between forwards
  // (HDF5Data) or a later layer writes a prefix blob in place; the caller
  // re-enables it after changing the input batch or a prefix weight.
  void set_reuse_prefix(bool on);
  // hipGraph replay (opt-in; for launch-bound small nets): one map (injection
  // + forward + statistics) is captured once and replayed per map, the map
  // id and the per-map row advancing in device memory (rram_inject_rng_batched_dev,
  // rram_mc_accumulate_dev).  Bit-identical to the eager maps.  Falls back to
  // the eager path while timing, injection overlap or prefix reuse is on, and
  // refuses nets whose source layers advance between forwards (HDF5Data).
  void set_graph(bool on);
  bool graph_active() const { return captured_.ready(); }
  // Map batching (opt-in; for launch-bound small nets): K fault maps share
  // every launch of one forward.  The net must have been built at batch K * B:
  // its batch axis then carries K groups of B images, and map j of a group of
  // K consecutive map ids evaluates images [j B, (j + 1) B) of the batch with
  // its own faulted copy of every faultable blob (a driver-owned K-copy stack
  // per blob, written by one rram_inject_rng_maps launch).  Only the
  // InnerProduct layers and the loss / accuracy heads know about the groups
  // (Layer::set_map_groups); the other layers are per-image in TEST phase.
  // Every map still runs its own whole forward over its own B images, and the
  // statistics are the sequential driver's bit for bit when the K slices hold
  // the same B images (TileInputs) -- provided the layers before the first
  // faultable one give an image the same bits at batch K * B as at B, which
  // set_map_batch checks for the convolutions' plans and refuses otherwise.
  // A short last group (count % K maps) injects and folds only its live maps;
  // its other slices compute on stale weights and are dropped.
  // Throws, naming the cause, when a source top's num is not divisible by K,
  // a source advances between forwards (HDF5Data), a statistic's producer
  // mixes images (EuclideanLoss), a faultable blob is a Convolution's, or
  // prefix reuse / graph replay is on (their setters throw while K > 1).
  // RRAM_MC_OVERLAP is ignored while K > 1.  K = 1 undoes all of it.
  void set_map_batch(int K);
  int map_batch() const { return map_batch_; }
  // copy the first B images of every bottom-less layer's tops over the other
  // K - 1 slices (device to device): every map then sees the same B images
  void TileInputs();
  // the K-copy stack of faultable blob i ([K][count]; nullptr while K == 1)
  const Dtype* map_stack(int i) const { return i >= 0 && i < (int)stacks_.size() ? stacks_[i] : nullptr; }
  int num_fault_blobs() const { return static_cast<int>(params_.size()); }
  int64_t fault_blob_count(int i) const { return params_[i]->count(); }
  EventTimer& timer() { return timer_; }
  int64_t fault_weights() const {
    int64_t n = 0;
    for (auto* p : params_) n += p->count();
    return n;
  }

 private:
  bool timing_ = false;
  bool reuse_prefix_ = false, prefix_done_ = false;
  EventTimer timer_;
  std::shared_ptr<Net<Dtype>> net_;
  std::vector<rram_inject_cfg> cfgs_;
  uint64_t seed_;
  int max_maps_;
  int maps_run_ = 0;
  std::vector<Blob<Dtype>*> params_;
  std::vector<Dtype*> clean_;
  std::vector<Blob<Dtype>*> outs_;
  // injection overlap: map m's injection runs on side_ while the layers
  // before the first faultable one run on the working stream; the faultable
  // layers wait for it (ev_injected_), the next injection waits for the
  // previous map's forward (ev_free_)
  bool overlap_ = true;
  int first_fault_layer_ = 0;
  int release_after_ = -1;  // overlapped maps: the prefix layer after which the injection starts
  hipStream_t side_ = nullptr;
  hipEvent_t ev_free_ = nullptr, ev_injected_ = nullptr;
  Dtype* d_sums_ = nullptr;       // [n_outputs]
  Dtype* d_per_map_ = nullptr;    // [max_maps][n_outputs]
  unsigned long long* d_broken_ = nullptr;
  // graph replay: d_state_ = {map id, per-map row} on the device
  bool graph_ = false, graph_warm_ = false;
  uint32_t* d_state_ = nullptr;
  CapturedGraph captured_;
  GraphStream gstream_;
  std::vector<const void*> graph_ptrs_;  // the device pointers the graph was captured with
  // map batching: stacks_[i] = K faulted copies of params_[i]; d_per_map_ has
  // map_batch_ spare rows so a group's rows never need clipping
  int map_batch_ = 1;
  std::vector<Dtype*> stacks_;
  // the layers never keep pointers into this driver past Run (exceptions included)
  struct ClearAcc {
    std::vector<Layer<Dtype>*>& v;
    ~ClearAcc() {
      for (auto* a : v) a->set_top_accumulator(nullptr, nullptr);
    }
  };
  size_t n_out_alloc() const { return std::max<size_t>(outs_.size(), 1); }
  // one segment per faultable blob: clean copy -> the net's weights, or -> stacks_
  std::vector<rram_inject_seg> inject_segs(bool into_stacks) const;
  // index of the layer whose first top is b (the last such layer), or -1
  int producer_of(const Blob<Dtype>* b) const;
  void apply_map_groups(int K);
  void run_groups(uint32_t map_begin, uint32_t map_count);
  void device_state_map();  // one map's launches on the working stream, map id and row from d_state_
  std::vector<const void*> graph_key() const;
  void drop_graph();
};

}  // namespace caffe
