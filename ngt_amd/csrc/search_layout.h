// search_layout.h -- the LDS layouts of the three graph-search kernels
// (search_kernels.hip, search_la.hip, search_lat.hip), shared by the kernels
// that carve their dynamic LDS with them and the host's launch planning
// (search_plan.cpp) that sizes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ngt_amd.h"
#include "ngt_kernels.h"

namespace ngt_amd {

// ---- one-expansion kernel (search_kernels.hip) -------------------------------
inline size_t search_lds_bytes(const SearchArgs& a, int otype) {
  size_t b = (a.ht_log2 ? ((size_t)4 << a.ht_log2) : 0) + (size_t)8 * a.cq_cap;
  b += ((size_t)8 * ((a.cq_cap + 63) / 64) + 15) & ~(size_t)15;  // chunk minima
  b += a.vf_log2 ? ((size_t)1 << a.vf_log2) / 8 : 0;
  b += ((size_t)8 * (a.k + 1) + 15) & ~(size_t)15;
  b += 512;
  b += ((size_t)a.dp * (otype == NGT_AMD_OBJECT_FLOAT ? 4 : 1) + 15) & ~(size_t)15;
  if (a.fcodes) b += (size_t)a.dp + 256;  // the query's filter bytes and the pending survivors
  return b;
}

// ---- lookahead kernel (search_la.hip) ----------------------------------------
struct LaCtl {
  uint32_t qi, done, nt, ntl, nl, nx, fthr, fsq;
  uint32_t epoch, pad[7];
  // the filter threshold's double-precision terms, kept in LDS: in registers
  // they spill, and a scratch reload waits for every store still in flight
  double fe, finv_b, frq;
};

// 16-byte aligned LDS carve-out; the host's search_la_lds_bytes mirrors it.
struct LaLayout {
  uint32_t off_tkey, off_tcnt, off_loff, off_xoff, off_vf, off_cq, off_res, off_q, off_qb, off_l,
      off_lfl, off_x, off_xe, off_xd, off_sh, off_nid, off_nd, total;
  __host__ __device__ static uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }
  __host__ __device__ LaLayout(const SearchArgs& a, int P) {
    uint32_t o = up16(sizeof(LaCtl));
    off_tkey = o; o = up16(o + 8u * P);
    off_tcnt = o; o = up16(o + 4u * P);
    off_loff = o; o = up16(o + 4u * (P + 1));
    off_xoff = o; o = up16(o + 4u * (P + 1));
    off_vf = o; o = up16(o + ((1u << a.vf_log2) >> 3));
    off_cq = o; o = up16(o + 8u * a.cq_cap);
    off_res = o; o = up16(o + 8u * (a.k + 1));
    off_q = o; o = up16(o + 4u * (uint32_t)a.dp);
    off_qb = o; o = up16(o + (uint32_t)a.dp);
    off_l = o; o = up16(o + 4u * a.la_lmax);
    off_lfl = o; o = up16(o + a.la_lmax);
    off_x = o; o = up16(o + 4u * a.la_lmax);
    off_xe = o; o = up16(o + 4u * a.la_lmax);
    off_xd = o; o = up16(o + 4u * a.la_lmax);
    off_sh = o; o = up16(o + (4u << a.la_sh_log2));
    off_nid = o; o = up16(o + 256u);
    off_nd = o; o = up16(o + 256u);
    total = o;
  }
};

inline uint32_t search_la_lds_bytes(const SearchArgs& a, int P) { return LaLayout(a, P).total; }

// ---- speculating latency kernel (search_lat.hip) -----------------------------
struct LatCtl {
  uint32_t done;  // the commit wave has finished the query
  uint32_t qi;
  uint32_t quit;  // serving form: no more work for this workgroup
  uint32_t k;     // this query's SearchContainer::size, coefficient, radius
  float coef;
  float radius;
  float expr;     // the commit wave's exploration radius (read by the hop prefetch)
  uint32_t ns;    // serving form: seeds staged in the tail
  uint64_t sp[4]; // diagnostic build: speculation-wave cycles ([0] adjacency, [2] exact rows)
};

// one node's speculation: key (its unchecked-set key, the priority), state,
// the claim word of its list parts (generation << 8 | parts taken), parts
// finished, list length, fresh entries per part
struct LatSlot {
  uint64_t key;
  uint32_t state;
  uint32_t claim;
  uint32_t pready; // parts finished (bit p: part p's entries and count are final)
  uint32_t deg;    // list length read (getEdgeSize cap), summed over the parts
  uint32_t pn[8];  // neighbours not yet visited when the part was read
};

struct LatLayout {
  uint32_t off_slot, off_eid, off_ed, off_tail, off_q, off_nid, off_nd, off_hist, off_bm,
      total;
  __host__ __device__ static uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }
  __host__ __device__ LatLayout(const SearchArgs& a, uint32_t cap, uint32_t waves) {
    uint32_t o = up16(sizeof(LatCtl));
    const uint32_t ns = a.lat_slots;
    off_slot = o; o = up16(o + sizeof(LatSlot) * ns);
    off_eid = o; o = up16(o + 4u * ns * cap);
    off_ed = o; o = up16(o + 4u * ns * cap);
    off_tail = o; o = up16(o + 8u * a.lat_tail);
    off_q = o; o = up16(o + 4u * (uint32_t)a.dp);
    off_nid = o; o = up16(o + 256u);
    off_nd = o; o = up16(o + 256u);
    off_hist = o; o = up16(o + 256u);
    off_bm = o; o = up16(o + 4u * ((a.nrows + 31u) / 32u));
    total = o;
  }
};

inline uint32_t search_lat_lds_bytes(const SearchArgs& a) {
  const uint32_t cap = (uint32_t)(a.adj_stride < a.edge_size ? a.adj_stride : a.edge_size);
  return LatLayout(a, cap, 8).total;
}

}  // namespace ngt_amd
