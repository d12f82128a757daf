#include "graph.hpp"

namespace caffe {

GraphStream::~GraphStream() {
  if (own_) {
    (void)hipStreamSynchronize(own_);
    (void)hipStreamDestroy(own_);
  }
  if (ev_in_) (void)hipEventDestroy(ev_in_);
  if (ev_out_) (void)hipEventDestroy(ev_out_);
}

void GraphStream::enter() {
  if (Caffe::hip_stream() != nullptr) return;
  if (!own_) {
    HIP_CALL(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    HIP_CALL(hipEventCreateWithFlags(&ev_in_, hipEventDisableTiming));
    HIP_CALL(hipEventCreateWithFlags(&ev_out_, hipEventDisableTiming));
  }
  HIP_CALL(hipEventRecord(ev_in_, nullptr));
  HIP_CALL(hipStreamWaitEvent(own_, ev_in_, 0));
  Caffe::set_stream(reinterpret_cast<rram_stream_t>(own_));
  active_ = true;
}

void GraphStream::leave() {
  if (!active_) return;
  active_ = false;
  Caffe::set_stream(nullptr);
  // no throw from a destructor path: a failed record / wait surfaces at the
  // caller's next synchronisation
  if (hipEventRecord(ev_out_, own_) == hipSuccess) (void)hipStreamWaitEvent(nullptr, ev_out_, 0);
}

void CapturedGraph::drop() {
  if (exec_) (void)hipGraphExecDestroy(exec_);
  if (graph_) (void)hipGraphDestroy(graph_);
  exec_ = nullptr;
  graph_ = nullptr;
}

void append_graph_key_tail(std::vector<const void*>& key) {
  key.push_back(Caffe::hip_stream());
  // the scratch the captured launches read and write (workspace, packs,
  // split-K partials, gather tables): eager work between replays may have
  // reallocated it (a larger test batch, another net on this thread)
  key.push_back(reinterpret_cast<const void*>(static_cast<uintptr_t>(Caffe::scratch_gen().load())));
  key.push_back(reinterpret_cast<const void*>(static_cast<uintptr_t>(rram_scratch_generation())));
}

}  // namespace caffe
