// device_graph.h -- a CSR graph with distances in HBM and the host plumbing the
// graph stages share (onng.cpp, refine.cpp, edges_api.cpp): the checks of a CSR
// argument, device selection, upload, download, the device check of the lists,
// the sort / dedupe / unpack tail that turns packed keys into a new CSR, and
// the host copy a *_get_graph entry point answers from.  What differs between
// the stages is an argument here: who is named in a message, whether slot 0
// may hold a list, whether the lists must be in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "index_internal.h"
#include "onng_kernels.h"

namespace ngt_amd {

struct DeviceGraph {
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> ids;
  DevBuf<float> d;
  uint64_t edges = 0;
  uint32_t maxlen = 0;
  // the bytes the three arrays hold go to *m
  explicit DeviceGraph(DevMeter* m = nullptr) : off(m), ids(m), d(m) {}
  onng::Csr csr() const { return onng::Csr{off.p, ids.p, d.p}; }
  void swap(DeviceGraph& o);
};

// A stage's result on the host: each family of entry points keeps one per thread.
struct HostGraph {
  std::vector<uint64_t> off;
  std::vector<uint32_t> ids;
  std::vector<float> d;
  bool ready = false;
};
// g into the caller's arrays (ids and dists may be null); `what` names the graph
// in "who: no <what> graph on this thread"
int copy_out(const HostGraph& g, const char* who, const char* what, uint64_t* offsets, uint32_t* ids, float* dists);

// Host checks of a CSR argument; the longest list goes to *longest.
// dummy_slot: slot 0 may not hold a list.
int check_csr(const char* who, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t nrows,
              bool dummy_slot, uint32_t* longest);

int select_device(const char* who, int device);

struct OwnedStream {
  hipStream_t s = nullptr;
  int create();
  ~OwnedStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

template <typename T>
int fetch(hipStream_t s, T* host, const T* dev, size_t count) {
  HIP_OK(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

// g.maxlen is the caller's (check_csr's longest)
int upload_graph(hipStream_t s, uint32_t n, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                 DeviceGraph& g);
int download_graph(hipStream_t s, uint32_t n, const DeviceGraph& g, HostGraph& out);

// Every id of a list names a row of [1, n); with need_order, every list is in
// (distance, id) order as well.  err is the caller's buffer of onng::kErrWords
// words (allocated here if it is not yet); check_lists' words stay in it.
int verify_lists(const char* who, hipStream_t s, uint32_t n, const DeviceGraph& g, bool need_order,
                 DevBuf<uint32_t>& err);

// Lists of packed (distance, id) keys, list u at keys_a[loff[u] .. loff[u + 1]),
// the longest of `longest` keys, into out: each sorted, repeats of an id
// dropped, unpacked.  keys_b is scratch of the same size, freed on the way; the
// list counter allocated here is charged to keys_a's meter.  Returns with the
// stream idle.
int lists_from_keys(hipStream_t s, uint32_t n, const uint64_t* loff, DevBuf<uint64_t>& keys_a,
                    DevBuf<uint64_t>& keys_b, uint32_t longest, DeviceGraph& out);
int max_of(hipStream_t s, const uint32_t* dev, uint32_t n, uint32_t* out);

}  // namespace ngt_amd
