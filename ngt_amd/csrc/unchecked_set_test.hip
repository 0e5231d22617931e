// unchecked_set_test.hip -- testing only: one wave drives the UncheckedSet of
// unchecked_set.h, the type the latency and NGTQG search kernels instantiate,
// through a script of inserts and pops, so the set can be compared with a
// plain heap (tests/test_gpu_unchecked_set.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_internal.h"
#include "unchecked_set.h"

namespace ngt_amd {

namespace {

struct SetTestArgs {
  const uint64_t* script;   // [n] non-zero: insert this key; zero: pop
  const uint8_t* tag_lane;  // [n] tagged sets: after step i, tag this head lane (>= 64: none)
  uint32_t n;
  uint32_t tail_cap, spill_cap;
  float expr;
  uint64_t* spill;    // [spill_cap]
  uint64_t* popped;   // [n] one per pop, 0 when the set had nothing to give
  uint64_t* events;   // [3 n][2] {kind << 32 | tag, key}: 1 tagged, 2 popped with its tag, 3 orphaned
  uint32_t* out;      // npopped, nevents, maxq, error word
};

template <bool TAGGED, bool TRIM>
__global__ void __launch_bounds__(64) unchecked_set_test_kernel(SetTestArgs t) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint64_t* tail = reinterpret_cast<uint64_t*>(smem);
  uint64_t* stage = tail + t.tail_cap;
  uint32_t* hist = reinterpret_cast<uint32_t*>(stage + 64);
  const int lane = lane_id();
  const float expr = t.expr;
  UncheckedSet<TAGGED, TRIM> us(tail, t.tail_cap, t.spill, t.spill_cap, hist, stage, expr);
  uint32_t npop = 0, nev = 0;
  uint64_t freem = ~0ull;  // the tags nobody holds
  auto event = [&](uint32_t kind, uint32_t tag, uint64_t key) {
    if (nev < 3u * t.n && lane == 0) {
      t.events[2ull * nev] = ((uint64_t)kind << 32) | tag;
      t.events[2ull * nev + 1] = key;
    }
    nev++;
  };
  for (uint32_t i = 0; i < t.n; i++) {
    const uint64_t w = t.script[i];
    if (w != 0ull) {
      us.insert(w);
    } else {
      uint64_t key = 0ull;
      if constexpr (TAGGED) {
        uint32_t tag = kNoTag;
        if (!us.pop(key, tag)) key = 0ull;
        if (key != 0ull && tag != kNoTag) {
          event(2u, tag, key);
          freem |= 1ull << tag;
        }
      } else {
        if (!us.pop(key)) key = 0ull;
      }
      if (lane == 0) t.popped[npop] = key;
      npop++;
    }
    if constexpr (TAGGED) {
      while (us.orphan) {
        const uint32_t s = (uint32_t)(__ffsll((long long)us.orphan) - 1);
        us.orphan &= us.orphan - 1;
        event(3u, s, 0ull);
        freem |= 1ull << s;
      }
      const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.tag_lane[i]);
      if (l < us.hn && freem != 0ull && (uint32_t)__builtin_amdgcn_readlane((int)us.ht, (int)l) == kNoTag) {
        const uint32_t tag = (uint32_t)(__ffsll((long long)freem) - 1);
        freem &= ~(1ull << tag);
        if ((uint32_t)lane == l) us.ht = tag;
        event(1u, tag, readlane_u64(us.hk, (int)l));
      }
    }
  }
  if (lane == 0) {
    t.out[0] = npop;
    t.out[1] = nev;
    t.out[2] = us.maxq;
    t.out[3] = us.err;
  }
}

}  // namespace

}  // namespace ngt_amd

extern "C" int ngt_amd_test_unchecked_set(int device, int tagged, int trim, const uint64_t* script,
                                          const uint8_t* tag_lane, uint32_t n, uint32_t tail_cap, uint32_t spill_cap,
                                          float expr, uint64_t* popped, uint32_t* npopped, uint64_t* events,
                                          uint32_t* nevents, uint32_t* maxq, uint32_t* error) {
  using namespace ngt_amd;
  if (!script || !popped || !npopped || !maxq || !error || n == 0 || n > (1u << 20) || tail_cap < 64 ||
      tail_cap > 4096 || spill_cap == 0 || spill_cap > (1u << 20) || (tagged && (!tag_lane || !events || !nevents)))
    return fail("ngt_amd_test_unchecked_set: bad arguments");
  HIP_OK(hipSetDevice(device));
  DevBuf<uint64_t> d_script, d_spill, d_popped, d_events;
  DevBuf<uint8_t> d_lane;
  DevBuf<uint32_t> d_out;
  HIP_OK(d_script.upload(script, n));
  HIP_OK(d_lane.upload(tag_lane, tagged ? n : 0));
  HIP_OK(d_spill.alloc(spill_cap));
  HIP_OK(d_popped.alloc(n));
  HIP_OK(d_events.alloc(6ull * n));
  HIP_OK(d_out.alloc(4));
  HIP_OK(hipMemset(d_out.p, 0, 16));
  const SetTestArgs t{d_script.p, d_lane.p, n, tail_cap, spill_cap, expr, d_spill.p, d_popped.p, d_events.p, d_out.p};
  const size_t lds = (size_t)8 * tail_cap + 512 + 256;
#define SET_TEST(TG, TR) hipLaunchKernelGGL((unchecked_set_test_kernel<TG, TR>), dim3(1), dim3(64), lds, nullptr, t)
  if (tagged) {
    if (trim) SET_TEST(true, true); else SET_TEST(true, false);
  } else {
    if (trim) SET_TEST(false, true); else SET_TEST(false, false);
  }
#undef SET_TEST
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  uint32_t out[4];
  HIP_OK(hipMemcpy(out, d_out.p, 16, hipMemcpyDeviceToHost));
  if (out[0] > n || out[1] > 3u * n) return fail("ngt_amd_test_unchecked_set: counts out of range");
  HIP_OK(hipMemcpy(popped, d_popped.p, (size_t)8 * out[0], hipMemcpyDeviceToHost));
  if (tagged) {
    HIP_OK(hipMemcpy(events, d_events.p, (size_t)16 * out[1], hipMemcpyDeviceToHost));
    *nevents = out[1];
  }
  *npopped = out[0];
  *maxq = out[2];
  *error = out[3];
  return 0;
}
