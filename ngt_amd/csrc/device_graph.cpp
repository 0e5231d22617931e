// device_graph.cpp -- see device_graph.h.
#include "device_graph.h"

#include <string.h>

#include <algorithm>

namespace ngt_amd {

void DeviceGraph::swap(DeviceGraph& o) {
  off.swap(o.off);
  ids.swap(o.ids);
  d.swap(o.d);
  std::swap(edges, o.edges);
  std::swap(maxlen, o.maxlen);
}

int copy_out(const HostGraph& g, const char* who, const char* what, uint64_t* offsets, uint32_t* ids, float* dists) {
  if (!g.ready) return fail("%s: no %s graph on this thread", who, what);
  if (!offsets) return fail("%s: bad arguments", who);
  memcpy(offsets, g.off.data(), g.off.size() * 8);
  if (ids && !g.ids.empty()) memcpy(ids, g.ids.data(), g.ids.size() * 4);
  if (dists && !g.d.empty()) memcpy(dists, g.d.data(), g.d.size() * 4);
  return 0;
}

int check_csr(const char* who, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t nrows,
              bool dummy_slot, uint32_t* longest) {
  if (!offsets) return fail("%s: bad arguments", who);
  if (nrows == 0 || nrows >= (1ull << 31)) return fail("%s: %llu rows are not supported", who, (unsigned long long)nrows);
  if (offsets[0] != 0) return fail("%s: offsets[0] is not 0", who);
  *longest = 0;
  for (uint64_t v = 0; v < nrows; v++) {
    if (offsets[v + 1] < offsets[v]) return fail("%s: offsets decrease at node %llu", who, (unsigned long long)v);
    if (offsets[v + 1] - offsets[v] >= (1ull << 31)) return fail("%s: the list of node %llu is too long", who, (unsigned long long)v);
    *longest = std::max(*longest, (uint32_t)(offsets[v + 1] - offsets[v]));
  }
  if (dummy_slot && offsets[1] != 0) return fail("%s: slot 0 is the dummy and has no list", who);
  if (offsets[nrows] && (!ids || !dists)) return fail("%s: ids or dists is null", who);
  return 0;
}

int select_device(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("%s: no HIP device available (the MI355X path has no CPU fallback)", who);
  if (device < 0 || device >= ndev) return fail("%s: device %d out of range", who, device);
  HIP_OK(hipSetDevice(device));
  return 0;
}

int OwnedStream::create() {
  HIP_OK(hipStreamCreateWithFlags(&s, hipStreamDefault));
  return 0;
}

int upload_graph(hipStream_t s, uint32_t n, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                 DeviceGraph& g) {
  const uint64_t E = offsets[n];
  HIP_OK(g.off.alloc((size_t)n + 1));
  HIP_OK(g.ids.alloc(E));
  HIP_OK(g.d.alloc(E));
  HIP_OK(hipMemcpyAsync(g.off.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  if (E) HIP_OK(hipMemcpyAsync(g.ids.p, ids, E * 4, hipMemcpyHostToDevice, s));
  if (E) HIP_OK(hipMemcpyAsync(g.d.p, dists, E * 4, hipMemcpyHostToDevice, s));
  g.edges = E;
  return 0;
}

int download_graph(hipStream_t s, uint32_t n, const DeviceGraph& g, HostGraph& out) {
  out.off.resize((size_t)n + 1);
  out.ids.resize(g.edges);
  out.d.resize(g.edges);
  HIP_OK(hipMemcpyAsync(out.off.data(), g.off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (g.edges) HIP_OK(hipMemcpyAsync(out.ids.data(), g.ids.p, g.edges * 4, hipMemcpyDeviceToHost, s));
  if (g.edges) HIP_OK(hipMemcpyAsync(out.d.data(), g.d.p, g.edges * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int verify_lists(const char* who, hipStream_t s, uint32_t n, const DeviceGraph& g, bool need_order,
                 DevBuf<uint32_t>& err) {
  HIP_OK(err.alloc(onng::kErrWords));
  HIP_OK(hipMemsetAsync(err.p, 0xff, onng::kErrWords * 4, s));
  onng::check_lists(n, g.csr(), err.p, s);
  HIP_OK(hipGetLastError());
  uint32_t h[onng::kErrWords];
  if (fetch(s, h, err.p, onng::kErrWords)) return -1;
  if (h[onng::kErrBadId] != 0xffffffffu)
    return fail("%s: the list of node %u holds an id outside [1, %u)", who, h[onng::kErrBadId], n);
  if (need_order && h[onng::kErrOrder] != 0xffffffffu)
    return fail("%s: the list of node %u is not in (distance, id) order", who, h[onng::kErrOrder]);
  return 0;
}

int max_of(hipStream_t s, const uint32_t* dev, uint32_t n, uint32_t* out) {
  std::vector<uint32_t> h(n);
  if (fetch(s, h.data(), dev, n)) return -1;
  *out = 0;
  for (uint32_t x : h) *out = std::max(*out, x);
  return 0;
}

int lists_from_keys(hipStream_t s, uint32_t n, const uint64_t* loff, DevBuf<uint64_t>& keys_a,
                    DevBuf<uint64_t>& keys_b, uint32_t longest, DeviceGraph& out) {
  onng::sort_lists(n, loff, keys_a.p, keys_b.p, longest > onng::kFastCap, s);
  DevBuf<uint32_t> cnt(keys_a.meter);
  HIP_OK(cnt.alloc(n));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  onng::unique_lists(n, loff, keys_b.p, keys_a.p, cnt.p, s);
  keys_b.release();
  HIP_OK(out.off.alloc((size_t)n + 1));
  onng::scan_u32(cnt.p, n, out.off.p, s);
  HIP_OK(hipGetLastError());
  if (fetch(s, &out.edges, out.off.p + n, 1)) return -1;
  if (max_of(s, cnt.p, n, &out.maxlen)) return -1;
  HIP_OK(out.ids.alloc(out.edges));
  HIP_OK(out.d.alloc(out.edges));
  onng::unpack_lists(n, loff, keys_a.p, out.off.p, out.ids.p, out.d.p, s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

}  // namespace ngt_amd
