// hipGraph plumbing shared by Solver::Step and MonteCarlo::Run.  What goes
// into a graph, and when it is warmed up, recaptured or dropped, stays each
// driver's own policy.
#pragma once

#include <utility>
#include <vector>

#include "common.hpp"

namespace caffe {

// hipStreamBeginCapture refuses the legacy NULL stream (e.g. torch's default
// stream).  On it, a graph section (eager warm-up, capture, launches) runs on
// a private non-blocking stream instead, ordered after the caller's earlier
// work and before its later work by two events, with Caffe's stream switched
// for the section so every launch and stream-keyed scratch buffer of the
// section sees one stream.  On any other stream it does nothing.
class GraphStream {
 public:
  GraphStream() = default;
  GraphStream(const GraphStream&) = delete;
  GraphStream& operator=(const GraphStream&) = delete;
  ~GraphStream();
  void enter();
  void leave();

 private:
  hipStream_t own_ = nullptr;
  hipEvent_t ev_in_ = nullptr, ev_out_ = nullptr;
  bool active_ = false;
};
struct GraphStreamScope {
  explicit GraphStreamScope(GraphStream& g) : g_(g) { g_.enter(); }
  ~GraphStreamScope() { g_.leave(); }
  GraphStream& g_;
};

// One captured graph and the executable instantiated from it.
class CapturedGraph {
 public:
  CapturedGraph() = default;
  CapturedGraph(const CapturedGraph&) = delete;
  CapturedGraph& operator=(const CapturedGraph&) = delete;
  ~CapturedGraph() { drop(); }
  bool ready() const { return exec_ != nullptr; }  // an instantiated executable exists
  // a throw from body() ends the capture, destroys the partial graph and goes on up
  template <class F>
  void capture(hipStream_t st, F&& body) {
    HIP_CALL(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    try {
      std::forward<F>(body)();
    } catch (...) {
      hipGraph_t g = nullptr;
      (void)hipStreamEndCapture(st, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    HIP_CALL(hipStreamEndCapture(st, &graph_));
    HIP_CALL(hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0));
  }
  void launch(hipStream_t st) { HIP_CALL(hipGraphLaunch(exec_, st)); }
  void drop();  // errors ignored: also the destructor's path

 private:
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
};

// what every captured graph depends on besides its driver's own device pointers
void append_graph_key_tail(std::vector<const void*>& key);

}  // namespace caffe
