// Drives the pure host unit of the edge-count optimisation
// (ngt_amd/csrc/edge_optimizer.cpp) with scripted callbacks: no device, no
// Python.  The scripted search answers every query alike, so a batch's mean
// accuracy is hits / results for a number of hits the script chooses per edge
// count.  Prints "ok: ..." and returns 0 when every check holds.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../ngt_amd/csrc/edge_optimizer.h"

using namespace ngt_amd;

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                  \
    }                                                              \
  } while (0)

static bool contains(const std::string& s, const std::string& t) { return s.find(t) != std::string::npos; }

// ---- a scripted index -----------------------------------------------------------
struct Script {
  size_t nresults = 50;
  // per sample (in build order): K -> hits of every query at that K
  std::vector<std::map<size_t, size_t>> hits;
  // what the procedure did
  std::vector<uint64_t> builds;
  std::vector<std::vector<size_t>> cuts;  // per sample the K sequence
  size_t extracts = 0, searches = 0;
  size_t current = 0;  // the K the index is cut to; 0 = the sample's whole graph

  EdgeCallbacks callbacks() {
    EdgeCallbacks cb;
    cb.build = [this](uint64_t end_id) -> std::string {
      builds.push_back(end_id);
      cuts.push_back({});
      current = 0;
      return "";
    };
    cb.extract = [this]() -> std::string {
      extracts++;
      return "";
    };
    cb.recut = [this](size_t K) -> std::string {
      cuts.back().push_back(K);
      current = K;
      return "";
    };
    cb.search = [this](AccuracyBatch& b) -> std::string {
      searches++;
      size_t h = b.size;  // the whole graph answers with the ground truth itself
      if (current != 0) {
        const auto& m = hits[builds.size() - 1];
        auto it = m.find(current);
        h = it == m.end() ? 0 : it->second;
      }
      for (uint32_t q = 0; q < b.nq; q++) {
        for (size_t j = 0; j < b.size; j++) {
          // ids 1..size at distances 1, 2, ...; a miss is an id the ground truth
          // does not hold, beyond its farthest distance
          const bool hit = j < h;
          b.ids[q * b.size + j] = hit ? (uint32_t)(j + 1) : (uint32_t)(1000 + j);
          b.dists[q * b.size + j] = hit ? (float)(j + 1) : (float)(2000 + j);
        }
        b.n[q] = (uint32_t)b.size;
        b.counts[q] = 100;
      }
      return "";
    };
    return cb;
  }
};

static std::vector<float> some_queries(size_t nq, uint32_t dim) {
  std::vector<float> q(nq * dim);
  for (size_t i = 0; i < q.size(); i++) q[i] = (float)(i % 7) * 0.25f;
  return q;
}

static std::vector<size_t> seq(std::initializer_list<size_t> l) { return std::vector<size_t>(l); }

static void check_sample_walk() {
  const uint32_t dim = 4;
  const std::vector<float> queries = some_queries(8, dim);
  {
    // rising accuracy: stops at the first K at or above the target
    Script s;
    s.hits = {{{5, 20}, {10, 35}, {20, 44}, {30, 46}, {40, 50}}};
    EdgeCallbacks cb = s.callbacks();
    cb.build(1);
    EdgeSample out;
    std::string e = edge_optimize_sample(cb, queries, dim, 2, s.nresults, 0.9f, 100, kAccuracyWorkGuard, out);
    CHECK(e.empty());
    CHECK(s.cuts[0] == seq({5, 10, 20, 30}));
    CHECK(s.extracts == 1);
    CHECK(out.edge == 30);
    CHECK(out.accuracy == (double)(float)(46.0 / 50.0));
    CHECK(out.gain == ((double)(float)(46.0 / 50.0) - (double)(float)(44.0 / 50.0)) / 10.0);
    CHECK(out.steps.size() == 4 && out.steps[1].edge == 10 && out.steps[1].accuracy == (double)(float)(35.0 / 50.0));
    CHECK(!out.guard_fired);
    // the maxEpsilon loop: the first batch differs from the zeroed last distances, then six identical ones
    CHECK(s.searches == 7 + 1 + 4);
  }
  {
    // never reaching the target: 5, 10, 20, ..., 100
    Script s;
    s.hits = {{}};
    EdgeCallbacks cb = s.callbacks();
    cb.build(1);
    EdgeSample out;
    CHECK(edge_optimize_sample(cb, queries, dim, 2, s.nresults, 0.9f, 100, kAccuracyWorkGuard, out).empty());
    CHECK(s.cuts[0] == seq({5, 10, 20, 30, 40, 50, 60, 70, 80, 90, 100}));
    CHECK(out.edge == 100 && out.accuracy == 0.0 && out.gain == 0.0);
  }
  {
    // the cap: no K above maxNoOfEdges
    Script s;
    s.hits = {{}, {}, {}};
    EdgeCallbacks cb = s.callbacks();
    EdgeSample out;
    cb.build(1);
    CHECK(edge_optimize_sample(cb, queries, dim, 2, s.nresults, 0.9f, 25, kAccuracyWorkGuard, out).empty());
    CHECK(s.cuts[0] == seq({5, 10, 20}) && out.edge == 20);
    cb.build(1);
    CHECK(edge_optimize_sample(cb, queries, dim, 2, s.nresults, 0.9f, 30, kAccuracyWorkGuard, out).empty());
    CHECK(s.cuts[1] == seq({5, 10, 20, 30}) && out.edge == 30);
    cb.build(1);
    CHECK(edge_optimize_sample(cb, queries, dim, 2, s.nresults, 0.9f, 4, kAccuracyWorkGuard, out).empty());
    CHECK(s.cuts[2].empty() && out.edge == 0);
  }
  {
    // reaching the target at K = 5 leaves the gain at 0
    Script s;
    s.hits = {{{5, 50}}};
    EdgeCallbacks cb = s.callbacks();
    cb.build(1);
    EdgeSample out;
    CHECK(edge_optimize_sample(cb, queries, dim, 2, s.nresults, 0.9f, 100, kAccuracyWorkGuard, out).empty());
    CHECK(s.cuts[0] == seq({5}) && out.edge == 5 && out.accuracy == 1.0 && out.gain == 0.0);
  }
}

static EdgeSample sample(size_t objects, size_t edge, float accuracy, double gain) {
  EdgeSample s;
  s.objects = objects;
  s.edge = edge;
  s.accuracy = accuracy;
  s.gain = gain;
  return s;
}

static void check_estimate() {
  size_t edge = 0;
  float acc = 0.0f;
  // the reference's own samples on the f16 data (cases D and E of
  // tests/golden/edge_optimization.json) give its defaults' result (case C)
  std::vector<EdgeSample> de = {sample(12500, 10, 0.9467f, 0.02), sample(25000, 10, 0.9297f, 0.02)};
  CHECK(edge_estimate(de, 25401, 0.9f, 25401, 50000, edge, acc).empty());
  CHECK(edge == 10);
  CHECK(format_stream(acc) == "0.92931");
  CHECK(edge_round(edge, 100) == 20);
  // at the samples' own sizes the estimate is the sample (cases D and E)
  CHECK(edge_estimate(de, 12500, 0.9f, 25401, 50000, edge, acc).empty());
  CHECK(edge == 10 && format_stream(acc) == "0.9467");
  CHECK(edge_estimate(de, 25000, 0.9f, 25401, 50000, edge, acc).empty());
  CHECK(edge == 10 && format_stream(acc) == "0.9297");
  // below the target: the last sample's gain buys the missing accuracy
  std::vector<EdgeSample> gp = {sample(12500, 20, 0.96f, 0.004), sample(25000, 30, 0.955f, 0.002)};
  CHECK(edge_estimate(gp, 1000000, 0.95f, 25401, 50000, edge, acc).empty());
  {
    const double span = log2((double)1000000) - log2((double)12500);
    const size_t first = (size_t)(20 + 10.0 * span);
    const float a = (float)((double)0.96f + ((double)0.955f - (double)0.96f) * span);
    CHECK(a < 0.95f);
    CHECK(edge == (size_t)((double)first + (double)(0.95f - a) / 0.002));
    CHECK(acc == 0.95f);
  }
  // rounding and cap of the path form
  CHECK(edge_round(0, 100) == 10 && edge_round(4, 100) == 10 && edge_round(5, 100) == 15);
  CHECK(edge_round(14, 100) == 20 && edge_round(15, 100) == 25 && edge_round(89, 100) == 95);
  CHECK(edge_round(90, 100) == 100 && edge_round(95, 100) == 100 && edge_round(1000, 100) == 100);
  CHECK(edge_round(25, 30) == 30 && edge_round(10, 15) == 15);

  // fewer than two samples
  std::string e = edge_estimate({}, 3001, 0.9f, 3001, 12500, edge, acc);
  CHECK(e == "Optimizer::optimizeNumberOfEdgesForANNG: Cannot optimize the number of edges. Too small object set. "
             "# of objects=3001 target No.=12500");
  e = edge_estimate({de[0]}, 13000, 0.9f, 13000, 25000, edge, acc);
  CHECK(contains(e, "Too small object set. # of objects=13000 target No.=25000"));

  // where the reference is undefined: a gain of 0 (the last sample stopped at K = 5), a negative or
  // non-finite gain, an estimate that is no count
  const std::string cannot = "Optimizer::optimizeNumberOfEdgesForANNG: Cannot optimize the number of edges. ";
  std::vector<EdgeSample> z = {sample(12500, 5, 0.8f, 0.0), sample(25000, 5, 0.7f, 0.0)};
  e = edge_estimate(z, 1000000, 0.9f, 25401, 50000, edge, acc);
  CHECK(e.compare(0, cannot.size(), cannot) == 0 && contains(e, "gain per edge of the last sample is 0"));
  z[1].gain = -0.001;
  e = edge_estimate(z, 1000000, 0.9f, 25401, 50000, edge, acc);
  CHECK(e.compare(0, cannot.size(), cannot) == 0 && contains(e, "gain per edge of the last sample is -0.001"));
  z[1].gain = NAN;
  e = edge_estimate(z, 1000000, 0.9f, 25401, 50000, edge, acc);
  CHECK(e.compare(0, cannot.size(), cannot) == 0 && contains(e, "gain per edge"));
  // the gain is not looked at when the estimate reaches the target
  z[1].gain = 0.0;
  CHECK(edge_estimate(z, 25000, 0.65f, 25401, 50000, edge, acc).empty());
  CHECK(edge == 5);
  // edges falling from sample to sample: the reference's size_t difference wraps
  std::vector<EdgeSample> w = {sample(12500, 30, 0.95f, 0.01), sample(25000, 10, 0.95f, 0.01)};
  e = edge_estimate(w, 25000, 0.9f, 25401, 50000, edge, acc);
  CHECK(e.compare(0, cannot.size(), cannot) == 0 && contains(e, "is not a count"));
  // a target below the first sample pulls the estimate below zero
  std::vector<EdgeSample> n = {sample(12500, 10, 0.95f, 0.01), sample(25000, 40, 0.95f, 0.01)};
  e = edge_estimate(n, 100, 0.9f, 25401, 50000, edge, acc);
  CHECK(e.compare(0, cannot.size(), cannot) == 0 && contains(e, "is not a count"));
  // the reference's own refusal of an estimate of 0
  std::vector<EdgeSample> o = {sample(12500, 0, 0.0f, 0.0), sample(25000, 0, 0.0f, 0.0)};
  e = edge_estimate(o, 25000, 0.0f, 25401, 50000, edge, acc);
  CHECK(e == cannot + "0:0 # of objects=25401");
}

static void check_query_draw() {
  // the first values of glibc's rand() without srand()
  static const int kFirst[5] = {1804289383, 846930886, 1681692777, 1714636915, 1957747793};
  srand(1);
  for (int v : kFirst) CHECK(rand() == v);
  const uint64_t osize = 1001;
  const uint32_t dim = 3;
  std::vector<float> rows(osize * dim);
  for (size_t i = 0; i < rows.size(); i++) rows[i] = (float)i;
  auto row = [&](uint64_t id) -> const void* { return rows.data() + id * dim; };
  auto idx_of = [&](int r) { return (uint64_t)floor((double)osize * (((double)r + 1.0) / ((double)RAND_MAX + 2.0))) + 1; };
  {
    std::vector<uint8_t> valid(osize, 1);
    valid[0] = 0;
    valid[idx_of(kFirst[1])] = 0;  // the second draw meets an empty slot
    std::vector<float> queries;
    size_t draws = 0;
    srand(1);
    std::string e = edge_draw_queries([] { return rand(); }, row, valid, osize, dim, 2, 4, queries, &draws);
    CHECK(e.empty());
    CHECK(draws == 5);
    CHECK(queries.size() == 4 * dim);
    const int taken[4] = {kFirst[0], kFirst[2], kFirst[3], kFirst[4]};
    for (int i = 0; i < 4; i++) {
      const uint64_t id = idx_of(taken[i]);
      CHECK(queries[i * dim] == (float)(id * dim) && queries[i * dim + 2] == (float)(id * dim + 2));
      CHECK(valid[id] == 0);  // erased: never drawn twice, never built
    }
    size_t left = 0;
    for (uint8_t v : valid) left += v;
    CHECK(left == 1000 - 1 - 4);
  }
  {
    // uint8 objects come back as floats of their values
    std::vector<uint8_t> bytes(osize * dim);
    for (size_t i = 0; i < bytes.size(); i++) bytes[i] = (uint8_t)(i * 37);
    std::vector<uint8_t> valid(osize, 1);
    valid[0] = 0;
    std::vector<float> queries;
    srand(1);
    std::string e = edge_draw_queries([] { return rand(); },
                                      [&](uint64_t id) -> const void* { return bytes.data() + id * dim; }, valid, osize,
                                      dim, 1, 1, queries, nullptr);
    CHECK(e.empty() && queries.size() == dim);
    CHECK(queries[1] == (float)bytes[idx_of(kFirst[0]) * dim + 1]);
  }
  {
    // 1000 empty draws end the call, whatever was drawn before
    std::vector<uint8_t> valid(osize, 0);
    valid[idx_of(kFirst[0])] = 1;
    std::vector<float> queries;
    size_t draws = 0;
    srand(1);
    std::string e = edge_draw_queries([] { return rand(); }, row, valid, osize, dim, 2, 5, queries, &draws);
    CHECK(e == "Too small amount of objects. 1001:5");
    CHECK(draws == 1001);
  }
}

static void check_sample_loop() {
  const uint32_t dim = 4;
  const std::vector<float> queries = some_queries(8, dim);
  const uint64_t osize = 25401;
  std::vector<uint8_t> valid(osize, 1);
  valid[0] = 0;
  for (uint64_t id = 10; id < 2010; id += 10) valid[id] = 0;  // 200 drawn queries among the first 2010 slots
  EdgeParams p;
  p.nresults = 50;
  {
    Script s;
    s.hits = {{{5, 30}, {10, 48}}, {{5, 28}, {10, 40}, {20, 47}}};
    size_t edge = 0;
    float acc = 0.0f;
    EdgeTrace tr;
    std::string e = edge_optimize(s.callbacks(), valid, osize, dim, 2, queries, p, kAccuracyWorkGuard, edge, acc, &tr);
    CHECK(e.empty());
    // one past the slot at which the count of stored objects reaches the target
    CHECK(s.builds.size() == 2 && s.builds[0] == 12500 + 200 + 1 && s.builds[1] == 25000 + 200 + 1);
    CHECK(s.cuts[0] == seq({5, 10}) && s.cuts[1] == seq({5, 10, 20}));
    CHECK(tr.samples.size() == 2 && tr.samples[0].objects == 12500 && tr.samples[1].objects == 25000);
    CHECK(tr.samples[0].edge == 10 && tr.samples[1].edge == 20);
    // target 0 objects = the repository size
    const double span = log2((double)osize) - log2((double)12500);
    CHECK(edge == (size_t)(10 + 10.0 * span));
    CHECK(acc == (float)((double)(float)0.96 + ((double)(float)0.94 - (double)(float)0.96) * span));
  }
  {
    // a target the stored objects never reach: one past the end, and the count as it is
    const uint64_t small = 25001;
    std::vector<uint8_t> v(valid.begin(), valid.begin() + small);
    Script s;
    s.hits = {{{5, 50}}, {{5, 50}}};
    size_t edge = 0;
    float acc = 0.0f;
    EdgeTrace tr;
    CHECK(edge_optimize(s.callbacks(), v, small, dim, 2, queries, p, kAccuracyWorkGuard, edge, acc, &tr).empty());
    CHECK(s.builds.size() == 2 && s.builds[1] == small + 1);
    CHECK(tr.samples[1].objects == 25000 - 200);
    CHECK(edge == 5 && acc == 1.0f);
  }
  {
    // noOfSampleObjects below 25000: one sample, then the refusal
    Script s;
    s.hits = {{{5, 50}}};
    EdgeParams q = p;
    q.sample_objects = 20000;
    size_t edge = 0;
    float acc = 0.0f;
    std::string e = edge_optimize(s.callbacks(), valid, osize, dim, 2, queries, q, kAccuracyWorkGuard, edge, acc);
    CHECK(s.builds.size() == 1);
    CHECK(contains(e, "Too small object set. # of objects=25401 target No.=25000"));
  }
}

int main() {
  check_sample_walk();
  check_estimate();
  check_query_draw();
  check_sample_loop();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ok: edge-count optimisation host unit\n");
  return 0;
}
