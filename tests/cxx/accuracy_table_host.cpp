// Host check of ngt_amd/csrc/accuracy_table.cpp without a device and without
// Python: the whole procedure driven by recorded per-epsilon search results
// (tests/golden/accuracy_trace_c1_onng.bin, written by
// make_accuracy_table_goldens.py from the restatement over the CPU oracle),
// the query extraction on a hand-made repository, and the 6-digit formatting
// against printf("%g").
//
//   accuracy_table_host <trace file>
//
// Trace (little endian): "NGTACCT1", u32 dim, object type, nresults, nq,
// ncalls, npairs; f32 queries [nq][dim] (as extracted); per call u32 size,
// f32 epsilon, i32 edge size, u32 1 when the call takes the extracted queries
// and 0 when it takes the ones read back from their text, u32 n [nq],
// u64 counts [nq], u16 ids [nq][size], f32 dists [nq][size]; then f32
// maxEpsilon, npairs x {f32 epsilon, f64 accuracy}, u32 length and the table.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../ngt_amd/csrc/accuracy_table.h"

using namespace ngt_amd;

static int failures = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      failures++;                     \
      fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);   \
      fprintf(stderr, "\n");          \
    }                                 \
  } while (0)

struct Reader {
  std::vector<uint8_t> buf;
  size_t pos = 0;
  bool ok = true;
  template <typename T>
  T get() {
    T v{};
    if (pos + sizeof(T) > buf.size()) {
      ok = false;
      return v;
    }
    memcpy(&v, buf.data() + pos, sizeof(T));
    pos += sizeof(T);
    return v;
  }
  template <typename T>
  std::vector<T> array(size_t n) {
    std::vector<T> v;
    if (n > (buf.size() - pos) / sizeof(T)) {
      ok = false;
      return v;
    }
    v.resize(n);
    if (n) memcpy(v.data(), buf.data() + pos, n * sizeof(T));
    pos += n * sizeof(T);
    return v;
  }
};

struct Call {
  uint32_t size;
  float epsilon;
  int32_t edge_size;
  uint32_t extracted;
  std::vector<uint32_t> n;
  std::vector<uint64_t> counts;
  std::vector<uint16_t> ids;
  std::vector<float> dists;
};

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static std::string printf_g(double x) {
  char b[64];
  snprintf(b, sizeof b, "%g", x);
  return b;
}

static void check_formatting(const std::vector<float>& seen) {
  const float fs[] = {0.0f, -0.0f, 1.0f, -0.6f, 0.05f, 0.1f, 1e-5f, 9.99999e-5f, 1e-4f, 123456.0f, 1234567.0f,
                      999999.5f, 0.000123456789f, 3.4028235e38f, 1.17549435e-38f, 4.65661287e-08f, 255.0f, 127.5f};
  for (float f : fs) CHECK(format_stream(f) == printf_g(f), "%a", f);
  for (float f : seen) CHECK(format_stream(f) == printf_g(f), "%a", f);
  const double ds[] = {0.0, 1.0, 0.9945, 0.1325, 0.99999949, 0.9999995, 1e-7, 123456.5, 1234567.0, 0.30000001192092896};
  for (double d : ds) CHECK(format_stream(d) == printf_g(d), "%a", d);
  // the query stream keeps 6 digits of a float element
  const std::vector<float> one = accuracy_parse_queries(accuracy_query_text({0.123456789f, 2.5f}, 2, 2));
  CHECK(one.size() == 2 && one[0] == 0.123457f && one[1] == 2.5f, "%zu", one.size());
}

static void check_extraction() {
  // slots 0..8, slot 0 the dummy, 3 and 8 removed; dim 2
  const float rows[9][2] = {{0, 0}, {1, 10}, {2, 20}, {3, 30}, {4, 40}, {5, 50}, {6, 60}, {7, 70}, {8, 80}};
  const uint8_t valid[9] = {0, 1, 1, 0, 1, 1, 1, 1, 0};
  auto row = [&](uint64_t id) -> const void* { return rows[id]; };
  std::vector<float> q;
  // interval 9 / 4 = 2: id1 = 1, 3 (-> 4), 5, 7; id2 = 2, 5, 6, then 8 is removed and nothing follows
  std::string e = accuracy_extract_queries(row, valid, 9, 2, 2, 4, q);
  CHECK(e == "Too many empty entries to extract.", "%s", e.c_str());
  e = accuracy_extract_queries(row, valid, 9, 2, 2, 3, q);  // interval 3: 1, 4, 7 -> the last fails again
  CHECK(e == "Too many empty entries to extract.", "%s", e.c_str());
  e = accuracy_extract_queries(row, valid, 8, 2, 2, 3, q);  // osize 8, interval 2: 1, 3 (-> 4), 5
  CHECK(e.empty(), "%s", e.c_str());
  const float want[] = {1.5f, 15.0f, 4.5f, 45.0f, 5.5f, 55.0f};
  CHECK(q.size() == 6 && memcmp(q.data(), want, sizeof want) == 0, "%zu", q.size());
  // uint8: integer division of the sum
  const uint8_t brows[4][3] = {{0, 0, 0}, {1, 255, 7}, {2, 255, 8}, {9, 0, 1}};
  const uint8_t bvalid[4] = {0, 1, 1, 1};
  auto brow = [&](uint64_t id) -> const void* { return brows[id]; };
  e = accuracy_extract_queries(brow, bvalid, 4, 3, 1, 2, q);  // interval 2: 1, 3 -> id2 = 4 is past the end
  CHECK(e == "Too many empty entries to extract.", "%s", e.c_str());
  e = accuracy_extract_queries(brow, bvalid, 4, 3, 1, 1, q);
  const float bwant[] = {1.0f, 255.0f, 7.0f};
  CHECK(e.empty() && q.size() == 3 && memcmp(q.data(), bwant, sizeof bwant) == 0, "%s", e.c_str());
  CHECK(accuracy_query_text(q, 3, 1) == "1\t255\t7\n", "%s", accuracy_query_text(q, 3, 1).c_str());
  const uint8_t gone[3] = {0, 0, 0};
  e = accuracy_extract_queries(brow, gone, 3, 3, 1, 1, q);
  CHECK(e == "Too many empty entries to extract. Object repository size=3 1:2", "%s", e.c_str());
  CHECK(!accuracy_extract_queries(brow, bvalid, 4, 3, 1, 0, q).empty(), "no query asked for");

  CHECK(accuracy_refusal(0, 20).empty() && accuracy_refusal(-2, 50).empty(), "refusal");
  CHECK(accuracy_refusal(40, 20) ==
            "Optimizer::generateAccuracyTable: edgeSizeForSearch is invalid to call generateAccuracyTable, because "
            "accuracy 1.0 cannot be achieved with the setting. edgeSizeForSearch=40.",
        "%s", accuracy_refusal(40, 20).c_str());
  CHECK(accuracy_refusal(0, 10) == "Error: gt data is less than result size! 10:20", "%s",
        accuracy_refusal(0, 10).c_str());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: accuracy_table_host trace\n");
    return 2;
  }
  Reader r;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[1]);
      return 2;
    }
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) r.buf.insert(r.buf.end(), chunk, chunk + got);
    fclose(f);
  }
  std::vector<char> magic = r.array<char>(8);
  if (!r.ok || memcmp(magic.data(), "NGTACCT1", 8) != 0) {
    fprintf(stderr, "not a trace file\n");
    return 2;
  }
  const uint32_t dim = r.get<uint32_t>(), otype = r.get<uint32_t>(), nresults = r.get<uint32_t>();
  const uint32_t nq = r.get<uint32_t>(), ncalls = r.get<uint32_t>(), npairs = r.get<uint32_t>();
  if (!r.ok || dim == 0 || dim > 4096 || nq == 0 || nq > 4096 || ncalls > 4096 || npairs > 4096) {
    fprintf(stderr, "bad trace header\n");
    return 2;
  }
  const std::vector<float> queries = r.array<float>((size_t)nq * dim);
  std::vector<Call> calls(ncalls);
  std::vector<float> seen;
  for (Call& c : calls) {
    c.size = r.get<uint32_t>();
    c.epsilon = r.get<float>();
    c.edge_size = r.get<int32_t>();
    c.extracted = r.get<uint32_t>();
    if (!r.ok || c.size > 4096) break;
    c.n = r.array<uint32_t>(nq);
    c.counts = r.array<uint64_t>(nq);
    c.ids = r.array<uint16_t>((size_t)nq * c.size);
    c.dists = r.array<float>((size_t)nq * c.size);
    if (seen.size() < 20000) seen.insert(seen.end(), c.dists.begin(), c.dists.end());
  }
  const float want_max = r.get<float>();
  std::vector<std::pair<float, double>> want(npairs);
  for (auto& p : want) {
    p.first = r.get<float>();
    p.second = r.get<double>();
  }
  const uint32_t len = r.get<uint32_t>();
  const std::vector<char> text = r.array<char>(len);
  if (!r.ok || r.pos != r.buf.size()) {
    fprintf(stderr, "truncated or overlong trace\n");
    return 2;
  }
  const std::string want_text(text.begin(), text.end());

  const std::vector<float> rounded = accuracy_parse_queries(accuracy_query_text(queries, dim, (int)otype));
  CHECK(rounded.size() == queries.size(), "%zu", rounded.size());

  size_t next = 0;
  AccuracySearch search = [&](AccuracyBatch& b) -> std::string {
    if (next >= calls.size()) return "more searches than the trace holds";
    const Call& c = calls[next++];
    if (b.size != c.size || bits(b.epsilon) != bits(c.epsilon) || b.edge_size != c.edge_size || b.nq != nq ||
        b.dim != dim) {
      char m[200];
      snprintf(m, sizeof m, "call %zu: size %zu epsilon %a edge size %lld, the trace has %u %a %d", next - 1, b.size,
               b.epsilon, (long long)b.edge_size, c.size, c.epsilon, c.edge_size);
      return m;
    }
    const std::vector<float>& q = c.extracted ? queries : rounded;
    if (memcmp(b.queries, q.data(), q.size() * sizeof(float)) != 0) return "a call took the wrong queries";
    b.n = c.n;
    b.counts = c.counts;
    for (size_t i = 0; i < c.ids.size(); i++) b.ids[i] = c.ids[i];
    b.dists = c.dists;
    return "";
  };
  std::vector<std::pair<float, double>> table;
  AccuracyTrace trace;
  std::string e = accuracy_generate(search, queries, dim, (int)otype, nresults, kAccuracyWorkGuard, table, &trace);
  CHECK(e.empty(), "%s", e.c_str());
  CHECK(next == calls.size(), "%zu of %zu recorded searches used", next, calls.size());
  CHECK(bits(trace.max_epsilon) == bits(want_max), "%a %a", trace.max_epsilon, want_max);
  CHECK(table.size() == want.size(), "%zu %zu", table.size(), want.size());
  for (size_t i = 0; i < table.size() && i < want.size(); i++)
    CHECK(bits(table[i].first) == bits(want[i].first) && table[i].second == want[i].second, "pair %zu: %a:%a %a:%a", i,
          table[i].first, table[i].second, want[i].first, want[i].second);
  const std::string got = accuracy_table_string(table);
  CHECK(got == want_text, "\n%s\n%s", got.c_str(), want_text.c_str());
  // keys only float accumulation gives (-0.6f + 10 x 0.05f; the halved steps around 0)
  CHECK(("," + got).find(",-0.0999999:") != std::string::npos, "%s", got.c_str());
  CHECK(("," + got).find(",4.65661e-08:") != std::string::npos, "%s", got.c_str());

  // without the work guard the identity rule alone must give the same table here
  next = 0;
  std::vector<std::pair<float, double>> table2;
  e = accuracy_generate(search, queries, dim, (int)otype, nresults, 0.0, table2);
  CHECK(e.empty() && table2 == table, "%s", e.c_str());

  // a search error ends the procedure with that error
  AccuracySearch broken = [](AccuracyBatch&) -> std::string { return "no device"; };
  CHECK(accuracy_generate(broken, queries, dim, (int)otype, nresults, kAccuracyWorkGuard, table2) == "no device",
        "error propagation");

  check_formatting(seen);
  check_extraction();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("ok: %u searches, %zu pairs, maxEpsilon %s\n", ncalls, table.size(), format_stream(trace.max_epsilon).c_str());
  return 0;
}
