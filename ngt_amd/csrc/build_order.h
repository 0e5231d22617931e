// build_order.h -- the order-deciding arithmetic of a DVP-tree leaf split
// (ngt_tree_insert_kernel, build_kernels.hip): the pivot variance in the
// reference's summation order and libstdc++'s std::sort over distance keys.
// Plain C++ marked __host__ __device__, so the same bodies run in the kernel
// and in the host test program (tests/cxx/build_order_host.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NGT_ORDER_HD __host__ __device__
#else
#define NGT_ORDER_HD
#endif

namespace ngt_amd {

#if defined(NGT_BUILD_ORDER_COUNT) && !defined(__HIP_DEVICE_COMPILE__)
// host test builds only: how often std_sort fell back to the heap sort
inline long& build_order_heap_sorts() {
  static long n = 0;
  return n;
}
#define NGT_ORDER_COUNT_HEAP_SORT() (++build_order_heap_sorts())
#else
#define NGT_ORDER_COUNT_HEAP_SORT() ((void)0)
#endif

// Node.cpp:117-129 as the reference's -Ofast build (GCC, AVX2) evaluates it
// (read from its object code): the sums over a row of the distance matrix
// run in four double lanes, lane l adding x[8b + l] + x[8b + l + 4] per block
// of 8, folded (l1 + l3) + (l0 + l2); then one 4-element block
// ((y1 + y3) + (y0 + y2)) if at least 4 remain, then the rest one by one;
// pow(d, 2) is d * d contracted into FMAs (lane l: fma(lo, lo, hi * hi)), and
// both divisions by fsize are multiplies by its reciprocal.  The order matters
// when variances tie in real arithmetic (duplicate-heavy or symmetric data).
NGT_ORDER_HD inline double pivot_variance(const float* x, uint32_t n) {
  const double inv = 1.0 / (double)n;
  const uint32_t n8 = n & ~7u;
  double s = 0.0;
  uint32_t j = 0;
  if (n > 7) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (uint32_t b = 0; b < n8; b += 8) {
      a0 += (double)x[b] + (double)x[b + 4];
      a1 += (double)x[b + 1] + (double)x[b + 5];
      a2 += (double)x[b + 2] + (double)x[b + 6];
      a3 += (double)x[b + 3] + (double)x[b + 7];
    }
    s = (a1 + a3) + (a0 + a2);
    j = n8;
    if (n - n8 >= 4) {
      s += ((double)x[j + 1] + (double)x[j + 3]) + ((double)x[j] + (double)x[j + 2]);
      j += 4;
    }
  }
  for (; j < n; j++) s += (double)x[j];
  const double avg = s * inv;
  double v = 0.0;
  j = 0;
  if (n > 7) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (uint32_t b = 0; b < n8; b += 8) {
      double lo, hi;
      lo = (double)x[b] - avg; hi = (double)x[b + 4] - avg; a0 += fma(lo, lo, hi * hi);
      lo = (double)x[b + 1] - avg; hi = (double)x[b + 5] - avg; a1 += fma(lo, lo, hi * hi);
      lo = (double)x[b + 2] - avg; hi = (double)x[b + 6] - avg; a2 += fma(lo, lo, hi * hi);
      lo = (double)x[b + 3] - avg; hi = (double)x[b + 7] - avg; a3 += fma(lo, lo, hi * hi);
    }
    v = (a1 + a3) + (a0 + a2);
    j = n8;
    if (n - n8 >= 4) {
      const double y0 = (double)x[j] - avg, y1 = (double)x[j + 1] - avg;
      const double y2 = (double)x[j + 2] - avg, y3 = (double)x[j + 3] - avg;
      v += fma(y1, y1, y3 * y3) + fma(y0, y0, y2 * y2);
      j += 4;
    }
  }
  for (; j < n; j++) {
    const double d = (double)x[j] - avg;
    v = fma(d, d, v);
  }
  return v * inv;
}

// ---- std::sort (libstdc++ introsort) over (distance) keys, lane 0 only -----
// Node::Object compares distances only (Node.h:66), so the order of equal
// distances is the one libstdc++'s algorithm leaves; it is restated here
// step for step (median-of-three to first, unguarded partition, threshold
// 16, final insertion sort).
struct SortItem {
  float d;
  uint32_t i;  // index into fs
};

NGT_ORDER_HD inline void iswap(SortItem* a, SortItem* b) {
  SortItem t = *a;
  *a = *b;
  *b = t;
}

NGT_ORDER_HD inline void move_median_to_first(SortItem* result, SortItem* a, SortItem* b, SortItem* c) {
  if (a->d < b->d) {
    if (b->d < c->d) iswap(result, b);
    else if (a->d < c->d) iswap(result, c);
    else iswap(result, a);
  } else if (a->d < c->d) {
    iswap(result, a);
  } else if (b->d < c->d) {
    iswap(result, c);
  } else {
    iswap(result, b);
  }
}

NGT_ORDER_HD inline SortItem* unguarded_partition(SortItem* first, SortItem* last, SortItem* pivot) {
  for (;;) {
    while (first->d < pivot->d) ++first;
    --last;
    while (pivot->d < last->d) --last;
    if (!(first < last)) return first;
    iswap(first, last);
    ++first;
  }
}

NGT_ORDER_HD inline void unguarded_linear_insert(SortItem* last) {
  SortItem val = *last;
  SortItem* next = last - 1;
  while (val.d < next->d) {
    *last = *next;
    last = next;
    --next;
  }
  *last = val;
}

NGT_ORDER_HD inline void insertion_sort(SortItem* first, SortItem* last) {
  if (first == last) return;
  for (SortItem* i = first + 1; i != last; ++i) {
    if (i->d < first->d) {
      SortItem val = *i;
      for (SortItem* p = i; p != first; --p) *p = *(p - 1);
      *first = val;
    } else {
      unguarded_linear_insert(i);
    }
  }
}

// libstdc++ heap sort of [first, last) (std::partial_sort(first, last, last):
// __make_heap + __sort_heap with __adjust_heap / __push_heap), used when the
// introsort depth limit is reached.
NGT_ORDER_HD inline void adjust_heap(SortItem* first, int hole, int len, SortItem value) {
  const int top = hole;
  int second = hole;
  while (second < (len - 1) / 2) {
    second = 2 * (second + 1);
    if (first[second].d < first[second - 1].d) second--;
    first[hole] = first[second];
    hole = second;
  }
  if ((len & 1) == 0 && second == (len - 2) / 2) {
    second = 2 * (second + 1);
    first[hole] = first[second - 1];
    hole = second - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && first[parent].d < value.d) {
    first[hole] = first[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  first[hole] = value;
}

NGT_ORDER_HD inline void heap_sort(SortItem* first, SortItem* last) {
  const int len = (int)(last - first);
  if (len < 2) return;
  for (int parent = (len - 2) / 2;; parent--) {
    adjust_heap(first, parent, len, first[parent]);
    if (parent == 0) break;
  }
  while (last - first > 1) {
    --last;
    SortItem value = *last;
    *last = *first;
    adjust_heap(first, 0, (int)(last - first), value);
  }
}

// std::sort: __introsort_loop (threshold 16, depth 2*lg(n)) then
// __final_insertion_sort.  Sub-ranges are disjoint, so processing them from
// an explicit stack instead of the recursion leaves the same result.
NGT_ORDER_HD inline void std_sort(SortItem* first, SortItem* last) {
  const int n = (int)(last - first);
  if (n < 2) return;
  SortItem* sf[64];
  SortItem* sl[64];
  int sd[64];
  int sp = 0;
  sf[sp] = first; sl[sp] = last; sd[sp] = 2 * (31 - __builtin_clz((unsigned)n)); sp++;
  while (sp) {
    sp--;
    SortItem* f = sf[sp];
    SortItem* l = sl[sp];
    int d = sd[sp];
    while (l - f > 16) {
      if (d == 0) {
        NGT_ORDER_COUNT_HEAP_SORT();
        heap_sort(f, l);
        break;
      }
      --d;
      SortItem* mid = f + (l - f) / 2;
      move_median_to_first(f, f + 1, mid, l - 1);
      SortItem* cut = unguarded_partition(f + 1, l, f);
      sf[sp] = cut; sl[sp] = l; sd[sp] = d; sp++;
      l = cut;
    }
  }
  if (n > 16) {
    insertion_sort(first, first + 16);
    for (SortItem* i = first + 16; i != last; ++i) unguarded_linear_insert(i);
  } else {
    insertion_sort(first, last);
  }
}

}  // namespace ngt_amd
