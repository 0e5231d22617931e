// scan_mfma.hip -- the exact batch scan of ObjectSpaceRepository::linearSearch
// (lib/NGT/ObjectSpaceRepository.h:466-502) for float L2 and Cosine as a
// matrix-core filter plus a bit-exact recompute.  The kernel template is in
// scan_mfma_kernel.h; this file instantiates it for L2 and Cosine and holds
// the operand preparation, scan_mfma_dot.hip instantiates it for Angle and the
// normalized metrics (thresholds: scan_dot_bound.h).
//
// Every (row, query) pair gets a dot product from bf16 MFMAs
// (v_mfma_f32_32x32x16_bf16): rows and queries are split into bf16 hi + lo
// parts, and hi*hi + hi*lo + lo*hi carries ~16 mantissa bits, so the filter
// value v' is within a PROVEN bound of the real-number distance (DESIGN.md
// 4d: kappa terms below).  A pair is a candidate only when v' says its
// distance may beat the query's current k-th key; candidates (a handful per
// query and tile once the lists fill) get the reference comparator's own
// distance (quad_distance: the 16-lane FMA order, folds and double sqrt of
// PrimitiveComparator.h) and enter the query's k-best list by (distance, id).
// A pair the filter rejects has a reference distance strictly above the k-th
// key at that moment, so the lists end exactly as the comparator-order scan's.
//
//  * L2: v' = q.x - xnk/2 with xnk = |x|^2 (1 - kappa) folded into the MFMA
//    as one extra k-step (three bf16 terms of xnk against -0.5);
//    candidate iff v' >= H_q = hb_q - thr_s (1 + rho) / 2, hb_q =
//    |q|^2 (1 - kappa) / 2 - kappa |q| Xmax, thr_s the squared-sum bound of
//    the k-th distance.
//  * Cosine: rows and queries are normalized first; v' ~ cos;
//    candidate iff v' >= H_q = (1 - kappa_c) - kth.
//  * rows that are removed / padding carry NaN in the extra column (never
//    candidates), rows with non-finite values (or zero norm for Cosine) -inf
//    (always candidates, the comparator decides); queries likewise through
//    hb = NaN / -inf.
//
// Work: a workgroup (4 waves, one per SIMD) owns 256 queries x one
// contiguous part of the rows and walks it in 128-row tiles; wave (wr, wq)
// computes 64 rows x 128 queries (2 x 4 MFMA tiles, 128 accumulator
// registers).  Operands are stored
// in HBM in fragment order ([32-row tile][k-step][lane][8 bf16]), so a wave
// stages one 1 KiB block per load and reads its fragments conflict-free.
// Workgroups of the same part run on the same XCD (blockIdx -> (xcd, slot))
// and share the part's rows through that XCD's L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_mfma_kernel.h"

namespace ngt_amd {

__device__ __forceinline__ uint16_t bf16_bits(float v) {
  const __bf16 b = (__bf16)v;
  return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ float bf16_val(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }

// ---------------------------------------------------------------------------
// Operand preparation: one wave per 32-object tile.  Lane (h = l >> 5,
// r = l & 31) writes, per k-step s, dims 16s + 8h .. +7 of object 32t + r.
// ---------------------------------------------------------------------------
// F: kScanPrepL2 (the norm column carries |x|^2 (1 - kappa)), kScanPrepCos
// (both sides normalized, zero norms forced; Cosine and Angle) or kScanPrepDot
// (the normalized metrics: operands as they are, the column carries only the
// NaN / -inf flags, hb = -E_q and hm = E_q with E_q = kappa |q| Xmax + slack).
template <int F, bool QUERY>
__global__ void __launch_bounds__(64) ngt_scan_prep_kernel(ScanPrepArgs a) {
  constexpr bool COS = F == kScanPrepCos, DOT = F == kScanPrepDot;
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int nk = a.dp >> 4;
  for (uint64_t t = blockIdx.x; t < a.ntiles32; t += gridDim.x) {
    const uint64_t id = t * 32 + r;
    const bool ok = id < a.n && (QUERY || a.valid == nullptr || a.valid[id]);
    const float* x = reinterpret_cast<const float*>(a.src + (ok ? id : 0) * a.stride);
    float ss = 0.0f;
    bool fin = true;
    if (ok) {
      for (int s = 0; s < nk; s++) {
        const float4 u = *reinterpret_cast<const float4*>(x + 16 * s + 8 * h);
        const float4 v = *reinterpret_cast<const float4*>(x + 16 * s + 8 * h + 4);
        const float e[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; j++) {
          ss = __builtin_fmaf(e[j], e[j], ss);
          fin = fin && __builtin_isfinite(e[j]);
        }
      }
    }
    ss += __shfl_xor(ss, 32, 64);
    fin = __shfl_xor((int)fin, 32, 64) != 0 && fin;
    fin = fin && __builtin_isfinite(ss);
    const bool forced = ok && (!fin || (COS && !(ss > 0.0f)));
    const bool use = ok && !forced;
    const float scale = COS && use ? 1.0f / sqrtf(ss) : 1.0f;
    uint16_t* oh = a.out_h + (t * a.ks) * 512 + lane * 8;
    uint16_t* ol = a.out_l + (t * a.ks) * 512 + lane * 8;
    for (int s = 0; s < nk; s++) {
      uint16_t hv[8], lv[8];
      float e[8];
      if (use) {
        const float4 u = *reinterpret_cast<const float4*>(x + 16 * s + 8 * h);
        const float4 v = *reinterpret_cast<const float4*>(x + 16 * s + 8 * h + 4);
        e[0] = u.x; e[1] = u.y; e[2] = u.z; e[3] = u.w; e[4] = v.x; e[5] = v.y; e[6] = v.z; e[7] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) e[j] = 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float v = e[j] * scale;
        hv[j] = bf16_bits(v);
        lv[j] = bf16_bits(v - bf16_val(hv[j]));
      }
      uint4 ph, pl;
      ph.x = hv[0] | (uint32_t)hv[1] << 16; ph.y = hv[2] | (uint32_t)hv[3] << 16;
      ph.z = hv[4] | (uint32_t)hv[5] << 16; ph.w = hv[6] | (uint32_t)hv[7] << 16;
      pl.x = lv[0] | (uint32_t)lv[1] << 16; pl.y = lv[2] | (uint32_t)lv[3] << 16;
      pl.z = lv[4] | (uint32_t)lv[5] << 16; pl.w = lv[6] | (uint32_t)lv[7] << 16;
      *reinterpret_cast<uint4*>(oh + s * 512) = ph;
      *reinterpret_cast<uint4*>(ol + s * 512) = pl;
    }
    // the extra k-step: rows carry -2 * (their share of the filter value)
    // as three bf16 terms, queries the matching -0.5 weights
    uint16_t ev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (h == 0) {
      if (QUERY) {
        if (ok) ev[0] = ev[1] = ev[2] = bf16_bits(-0.5f);
      } else if (!ok) {
        ev[0] = 0x7fc0;  // NaN: never a candidate
      } else if (forced) {
        ev[0] = 0xff80;  // -inf: v' = +inf, always a candidate
      } else if (!COS && !DOT) {
        const float xnk = ss * a.one_minus_kappa;
        ev[0] = bf16_bits(xnk);
        const float r1 = xnk - bf16_val(ev[0]);
        ev[1] = bf16_bits(r1);
        ev[2] = bf16_bits(r1 - bf16_val(ev[1]));
      }
    }
    uint4 pe;
    pe.x = ev[0] | (uint32_t)ev[1] << 16; pe.y = ev[2] | (uint32_t)ev[3] << 16;
    pe.z = ev[4] | (uint32_t)ev[5] << 16; pe.w = ev[6] | (uint32_t)ev[7] << 16;
    *reinterpret_cast<uint4*>(oh + nk * 512) = pe;
    *reinterpret_cast<uint4*>(ol + nk * 512) = make_uint4(0u, 0u, 0u, 0u);
    if (!QUERY) {
      if (!COS) {
        // Xmax: an upper bound of every row's |x| (rounded up twice)
        float nx = use ? sqrtf(ss) * 1.0000005f : 0.0f;
        for (int o = 32; o >= 1; o >>= 1) nx = fmaxf(nx, __shfl_xor(nx, o, 64));
        if (lane == 0 && nx > 0.0f) atomicMax(a.xmax_bits, __float_as_uint(nx));
      }
    } else if (h == 0 && t * 32 + r < a.n_pad) {
      // hb: the filter base; hm: the margin of a threshold taken from the
      // filter values themselves (the first tile's bootstrap)
      float hb, hm = __builtin_huge_valf();
      if (!ok) {
        hb = __builtin_nanf("");
      } else if (forced) {
        hb = -__builtin_huge_valf();
      } else if (COS) {
        hb = a.hb_cos;
        hm = a.kappa_boot;
      } else if (DOT) {
        const float xmax = __uint_as_float(*a.xmax_bits);
        const float nq = sqrtf(ss) * 1.0000005f;
        hm = a.kappa * nq * xmax + a.slack;
        hb = -hm;
      } else {
        const float xmax = __uint_as_float(*a.xmax_bits);
        const float nq = sqrtf(ss) * 1.0000005f;
        hb = 0.5f * ss * a.one_minus_kappa - a.kappa * nq * xmax - a.slack;
        hm = a.kappa_boot * (nq + xmax) * (nq + xmax) + 2.0f * a.slack;
      }
      a.hb[t * 32 + r] = hb;
      a.hm[t * 32 + r] = hm;
    }
  }
}

size_t scan_mfma_lds_bytes(uint32_t k) {
  return kMxNst * kMxStage + (size_t)kMxQ * k * 8 + kMxQ * 8 + (size_t)kMxQ * kMxPend * 8 + kMxQ * 4 * 5 +
         kMxQ * kMxW * 4 + 16;
}

template <int F>
static void launch_scan_prep_t(const ScanPrepArgs& a, bool query, uint32_t blocks, hipStream_t s) {
  if (query) hipLaunchKernelGGL((ngt_scan_prep_kernel<F, true>), dim3(blocks), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((ngt_scan_prep_kernel<F, false>), dim3(blocks), dim3(64), 0, s, a);
}

hipError_t launch_scan_prep(const ScanPrepArgs& a, int form, bool query, hipStream_t s) {
  const uint64_t blocks = a.ntiles32 < 65536 ? a.ntiles32 : 65536;
  if (blocks == 0) return hipSuccess;
  if (form == kScanPrepCos) launch_scan_prep_t<kScanPrepCos>(a, query, (uint32_t)blocks, s);
  else if (form == kScanPrepDot) launch_scan_prep_t<kScanPrepDot>(a, query, (uint32_t)blocks, s);
  else if (form == kScanPrepL2) launch_scan_prep_t<kScanPrepL2>(a, query, (uint32_t)blocks, s);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

hipError_t launch_scan_mfma(const MfmaScanArgs& a, int metric, int passes, hipStream_t s) {
  const size_t lds = scan_mfma_lds_bytes(a.k);
  const uint32_t grid = a.nparts * a.mblocks;
  if (metric == kL2 && passes == 3) launch_scan_mfma_t<kL2, 3>(a, lds, grid, s);
  else if (metric == kL2 && passes == 1) launch_scan_mfma_t<kL2, 1>(a, lds, grid, s);
  else if (metric == kCosine && passes == 3) launch_scan_mfma_t<kCosine, 3>(a, lds, grid, s);
  else if (metric == kCosine && passes == 1) launch_scan_mfma_t<kCosine, 1>(a, lds, grid, s);
  else if (passes == 3 && (metric == kAngle || metric == kNormalizedAngle || metric == kNormalizedCosine ||
                           metric == kNormalizedL2))
    return launch_scan_mfma_dot(a, metric, lds, grid, s);  // scan_mfma_dot.hip
  else return hipErrorNotSupported;
  return hipGetLastError();
}

}  // namespace ngt_amd
