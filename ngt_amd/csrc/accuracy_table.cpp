// accuracy_table.cpp -- see accuracy_table.h.
#include "accuracy_table.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include <map>
#include <sstream>
#include <unordered_set>

namespace ngt_amd {

std::string format_stream(float x) {
  std::ostringstream ss;
  ss << x;
  return ss.str();
}
std::string format_stream(double x) {
  std::ostringstream ss;
  ss << x;
  return ss.str();
}

std::string accuracy_refusal(int32_t edge_size_for_search, size_t nresults) {
  std::ostringstream msg;
  if (edge_size_for_search != 0 && edge_size_for_search != -2) {
    msg << "Optimizer::generateAccuracyTable: edgeSizeForSearch is invalid to call generateAccuracyTable, because "
           "accuracy 1.0 cannot be achieved with the setting. edgeSizeForSearch="
        << edge_size_for_search << ".";
    return msg.str();
  }
  // the sweep always asks for kAccuracySweepSize results; the ground truth holds nresults
  if (nresults < kAccuracySweepSize) {
    msg << "Error: gt data is less than result size! " << nresults << ":" << kAccuracySweepSize;
    return msg.str();
  }
  return "";
}

std::string accuracy_extract_queries(const std::function<const void*(uint64_t)>& row, const uint8_t* valid,
                                     uint64_t osize, uint32_t dim, int object_type, size_t nqueries,
                                     std::vector<float>& queries) {
  queries.clear();
  if (nqueries == 0) return "Optimizer::extractQueries: the number of queries is 0";
  auto empty = [&](uint64_t id) { return id >= osize || !valid[id]; };  // Repository::isEmpty
  const uint64_t interval = osize / nqueries;
  size_t count = 0;
  for (uint64_t id1 = 1; id1 < osize && count < nqueries; id1 += interval, count++) {
    uint64_t oft = 0;
    while (empty(id1 + oft)) {
      oft++;
      if (id1 + oft >= osize) {
        std::ostringstream msg;
        msg << "Too many empty entries to extract. Object repository size=" << osize << " " << id1 << ":" << oft;
        return msg.str();
      }
    }
    uint64_t id2 = id1 + oft + 1;
    while (empty(id2)) {
      id2++;
      if (id2 >= osize) return "Too many empty entries to extract.";
    }
    // meanObject (:1068-1094)
    if (object_type == 1) {
      const uint8_t* a = static_cast<const uint8_t*>(row(id1 + oft));
      const uint8_t* b = static_cast<const uint8_t*>(row(id2));
      for (uint32_t i = 0; i < dim; i++) {
        int d = (a[i] + b[i]) / 2;
        queries.push_back((float)d);
      }
    } else {
      const float* a = static_cast<const float*>(row(id1 + oft));
      const float* b = static_cast<const float*>(row(id2));
      for (uint32_t i = 0; i < dim; i++) {
        float d = (a[i] + b[i]) / 2.0F;
        queries.push_back(d);
      }
    }
  }
  return "";
}

std::string accuracy_query_text(const std::vector<float>& queries, uint32_t dim, int object_type) {
  std::ostringstream os;
  for (size_t q = 0; q * dim < queries.size(); q++) {
    for (uint32_t i = 0; i < dim; i++) {
      if (object_type == 1) {
        int d = queries[q * dim + i];
        os << d;
      } else {
        os << queries[q * dim + i];
      }
      if (i + 1 != dim) os << "\t";
    }
    os << std::endl;
  }
  return os.str();
}

std::vector<float> accuracy_parse_queries(const std::string& text) {
  // Common::extractVector: strtod per token, stored as the object's element
  std::vector<float> out;
  const char* p = text.c_str();
  for (;;) {
    char* e = nullptr;
    double v = strtod(p, &e);
    if (e == p) break;
    out.push_back((float)v);
    p = e;
  }
  return out;
}

std::string accuracy_run_batch(const AccuracySearch& search, AccuracyBatch& b) {
  b.ids.assign((size_t)b.nq * b.size, 0);
  b.dists.assign((size_t)b.nq * b.size, 0.0f);
  b.n.assign(b.nq, 0);
  b.counts.assign(b.nq, 0);
  std::string e = search(b);
  if (!e.empty()) return e;
  for (uint32_t q = 0; q < b.nq; q++)
    if (b.n[q] > b.size) return "Optimizer: a search returned more results than its size";
  return "";
}

namespace {
double printed(float d) { return strtod(format_stream(d).c_str(), nullptr); }
}  // namespace

// evaluate (:175-226) of one epsilon's results against the ground truth;
// MeasuredValue::meanAccuracy is a float (:37).
std::string accuracy_evaluate(const AccuracyGroundTruth& gt, const AccuracyBatch& b, double& accuracy) {
  size_t size = 0;  // checkAndGetSize (:280-343): the first result size, raised by a larger one
  for (uint32_t q = 0; q < b.nq; q++)
    if (b.n[q] > size) size = b.n[q];
  if (size == 0) return "Fatal error! Cannot get any accuracy value.";
  double total = 0.0;
  for (uint32_t q = 0; q < b.nq; q++) {
    if (gt.ids[q].size() < size) {  // loadGroundTruth (:247-251)
      std::ostringstream msg;
      msg << "Error: gt data is less than result size! " << gt.ids[q].size() << ":" << size;
      return msg.str();
    }
    std::unordered_set<size_t> ids(gt.ids[q].begin(), gt.ids[q].begin() + size);
    const double farthest = gt.dists[q][size - 1];
    size_t relevant = 0;
    for (uint32_t j = 0; j < b.n[q]; j++) {  // sumup (:486-507)
      if (ids.count(b.ids[(size_t)q * b.size + j]) != 0) {
        relevant++;
      } else if (farthest > 0.0 && printed(b.dists[(size_t)q * b.size + j]) <= farthest) {
        relevant++;
      }
    }
    total += (double)relevant / (double)size;
  }
  float mean = total / (double)b.nq;
  accuracy = mean;
  return "";
}

std::string accuracy_pseudo_ground_truth(const AccuracySearch& search, const std::vector<float>& queries, uint32_t dim,
                                         int object_type, size_t nresults, double guard, std::vector<float>& rounded,
                                         AccuracyGroundTruth& gt, AccuracyTrace& tr) {
  if (dim == 0 || queries.empty() || queries.size() % dim) return "Optimizer: no query was extracted";
  const uint32_t nq = (uint32_t)(queries.size() / dim);
  tr = AccuracyTrace();
  gt = AccuracyGroundTruth();
  AccuracyBatch b;
  b.nq = nq;
  b.dim = dim;
  // generatePseudoGroundTruth (:1425-1481): the unrounded queries, nresults
  // results, the property's edge size
  float maxEpsilon = 0.0;
  {
    int identityCount = 0;
    std::vector<float> lastDistances(nq);
    uint64_t count0 = 0;
    double step = 0.02;
    for (float e = 0.0; e < 10.0; e += step) {
      b.queries = queries.data();
      b.size = nresults;
      b.epsilon = e;
      b.edge_size = -1;
      std::string err = accuracy_run_batch(search, b);
      if (!err.empty()) return err;
      bool identity = true;
      for (uint32_t idx = 0; idx < nq; idx++) {
        if (b.n[idx] == 0) return "Optimizer::generatePseudoGroundTruth: a search returned no result";
        float d = b.dists[(size_t)idx * b.size + b.n[idx] - 1];
        if (d != lastDistances[idx]) identity = false;
        lastDistances[idx] = d;
      }
      const uint64_t work = b.counts[nq - 1];  // the reference's timer holds the last query's search
      if (e == 0.0) count0 = work;
      if (guard > 0.0 && (double)work > (double)count0 * guard) {
        maxEpsilon = e;
        tr.guard_fired = true;
        break;
      }
      if (identity) {
        identityCount++;
        step *= 1.2;
        if (identityCount > 5) {
          maxEpsilon = e;
          break;
        }
      } else {
        identityCount = 0;
      }
    }
  }
  tr.max_epsilon = maxEpsilon;

  // from here on the queries are the ones the query stream's text gives back
  rounded = accuracy_parse_queries(accuracy_query_text(queries, dim, object_type));
  if (rounded.size() != queries.size()) return "Optimizer: the query stream does not hold the extracted queries";

  // createGroundTruth (:1223-1229, :1485-1491): all edges, epsilon = maxEpsilon
  {
    b.queries = rounded.data();
    b.size = nresults;
    b.epsilon = maxEpsilon;
    b.edge_size = 0;
    std::string err = accuracy_run_batch(search, b);
    if (!err.empty()) return err;
    gt.ids.resize(nq);
    gt.dists.resize(nq);
    for (uint32_t q = 0; q < nq; q++)
      for (uint32_t j = 0; j < b.n[q]; j++) {
        gt.ids[q].push_back(b.ids[(size_t)q * b.size + j]);
        gt.dists[q].push_back(printed(b.dists[(size_t)q * b.size + j]));
      }
  }
  return "";
}

std::string accuracy_generate(const AccuracySearch& search, const std::vector<float>& queries, uint32_t dim,
                              int object_type, size_t nresults, double guard,
                              std::vector<std::pair<float, double>>& table, AccuracyTrace* trace) {
  table.clear();
  if (dim == 0 || queries.empty() || queries.size() % dim) return "Optimizer: no query was extracted";
  const uint32_t nq = (uint32_t)(queries.size() / dim);
  AccuracyTrace tr;
  AccuracyBatch b;
  b.nq = nq;
  b.dim = dim;

  std::vector<float> rounded;
  AccuracyGroundTruth gt;
  {
    std::string err = accuracy_pseudo_ground_truth(search, queries, dim, object_type, nresults, guard, rounded, gt, tr);
    if (!err.empty()) return err;
  }
  const float maxEpsilon = tr.max_epsilon;

  // the sweep (:1514-1554)
  std::map<float, double> map;
  {
    float interval = 0.05;
    float prev = 0.0;
    float epsilon = -0.6;
    double accuracy = 0.0;
    do {
      auto pair = map.find(epsilon);
      if (pair == map.end()) {
        b.queries = rounded.data();
        b.size = kAccuracySweepSize;
        b.epsilon = epsilon;
        b.edge_size = -1;
        std::string err = accuracy_run_batch(search, b);
        if (!err.empty()) return err;
        err = accuracy_evaluate(gt, b, accuracy);
        if (!err.empty()) return err;
        map.insert(std::make_pair(epsilon, accuracy));
      } else {
        accuracy = (*pair).second;
      }
      if (prev != 0.0) {
        if (accuracy - prev < 0.02) {
          interval *= 2.0;
        } else if (accuracy - prev > 0.05 && interval > 0.0001) {
          epsilon -= interval;
          interval /= 2.0;
          accuracy = prev;
        }
      }
      prev = accuracy;
      epsilon += interval;
      if (accuracy > 0.98 && epsilon > maxEpsilon) break;
    } while (accuracy < 1.0);
  }

  // :1556-1570
  std::pair<float, double> prev(0.0, -1.0);
  for (auto i = map.begin(); i != map.end(); ++i) {
    if (fabs((*i).first - prev.first) <= FLT_EPSILON) continue;
    if ((*i).second - prev.second < DBL_EPSILON) continue;
    table.push_back(*i);
    if ((*i).second >= 1.0) break;
    prev = *i;
  }
  if (trace) *trace = tr;
  return "";
}

std::string accuracy_table_string(const std::vector<std::pair<float, double>>& table) {
  std::stringstream str;
  for (auto i = table.begin(); i != table.end(); ++i) {
    str << (*i).first << ":" << (*i).second;
    if (i + 1 != table.end()) str << ",";
  }
  return str.str();
}

}  // namespace ngt_amd
