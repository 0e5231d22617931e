"""``ngtpy``-compatible surface over the drop-in C API (python/src/ngtpy.cpp:30-330
for the behaviour, :505-560 for the names and defaults).

Same module-level ``create`` and ``Index`` class, same argument names and
defaults, same result shapes: a list of ``(id, distance)`` tuples, or an int32
id array with ``with_distance=False``, ids zero-based unless
``zero_based_numbering=False``.  Every search runs on the MI355X through
libngt_amd.so (``ngt_batch_search_index`` / ``_using_only_graph`` /
``ngt_batch_linear_search_index``); there is no host fallback.
"""
import os

import numpy as np

from . import NativeError
from . import base

FLT_MAX = 3.4028234663852886e38
DBL_MAX = 1.7976931348623157e308
INT_MIN = -(2 ** 31)


def create(path, dimension, edge_size_for_creation=10, edge_size_for_search=40, distance_type="L2",
           object_type="Float"):
    """ngtpy.create (ngtpy.cpp:52-101): an empty index directory."""
    ot = {"Float": "Float", "float": "Float", "Byte": "Integer", "byte": "Integer"}.get(object_type)
    if ot is None:
        raise NativeError("ngtpy::create: invalid object type. " + object_type)
    if distance_type not in ("L1", "L2", "Normalized L2", "Hamming", "Jaccard", "Sparse Jaccard", "Angle",
                             "Normalized Angle", "Cosine", "Normalized Cosine"):
        raise NativeError("ngtpy::create: invalid distance type. " + distance_type)
    base.Index.create(path, dimension, edge_size_for_creation, edge_size_for_search, ot, distance_type)


def accuracy_table(path):
    """The prf's AccuracyTable (Index.h:255, written by the optimizer) as
    Index::AccuracyTable::set parses it (Index.h:299-315): comma-separated
    ``epsilon:accuracy`` pairs, epsilon stored as float, accuracy as double;
    fewer than two tokens leave the table empty."""
    text = ""
    with open(os.path.join(path, "prf")) as f:
        for line in f:
            key, _, val = line.rstrip("\n").partition("\t")
            if key == "AccuracyTable":
                text = val
    return parse_accuracy_table(text)


def parse_accuracy_table(text):
    """Index::AccuracyTable::set of the table's string."""
    toks = [t for t in text.split(",") if t]
    if len(toks) < 2:
        return []
    table = []
    for t in toks:
        ts = [x for x in t.split(":") if x]
        if len(ts) != 2:
            raise NativeError("AccuracyTable: Invalid accuracy table string %s:%s" % (t, text))
        table.append((np.float32(float(ts[0])), float(ts[1])))
    return table


def epsilon_from_expected_accuracy(table, accuracy):
    """Index::AccuracyTable::getEpsilon (Index.h:317-346): linear
    interpolation between the entries that bracket `accuracy`, in the
    reference's mixed float/double arithmetic, clamped below at -0.9."""
    if len(table) <= 2:
        raise NativeError("AccuracyTable: The accuracy table is not set yet. The table size=%d" % len(table))
    accuracy = min(float(accuracy), 1.0)
    i = 0
    while i < len(table) and table[i][1] < accuracy:
        i += 1
    if i == len(table):
        i -= 2
    elif i != 0:
        i -= 1
    (lf, ls), (uf, us) = table[i], table[i + 1]
    e = np.float32(float(lf) + float(np.float32(uf - lf)) * (accuracy - ls) / (us - ls))
    return float(max(e, np.float32(-0.9)))


class Index(object):
    """ngtpy.Index (ngtpy.cpp:30-50): defaults k=20, epsilon=0.1,
    radius=FLT_MAX, edge size from the property."""

    def __init__(self, path, read_only=False, zero_based_numbering=True, tree_disabled=False,
                 log_disabled=False):
        self._ix = base.Index(path)
        self.read_only = read_only
        self.zero = zero_based_numbering
        self.tree = not tree_disabled
        self.num_of_search_objects = 20
        self.epsilon = 0.1
        self.radius = FLT_MAX
        self.edge_size = -1
        self.expected_accuracy = -1.0  # defaultExpectedAccuracy (ngtpy.cpp:49)
        self.distance_computations = 0
        self._table = None

    def _id_out(self, ids):
        return ids.astype(np.int64) - 1 if self.zero else ids.astype(np.int64)

    def _id_in(self, oid):
        return oid + 1 if self.zero else oid

    def _results(self, ids, ds, n, with_distance):
        ids = self._id_out(ids[0, :n[0]])
        if not with_distance:
            return ids.astype(np.int32)
        return [(int(i), float(d)) for i, d in zip(ids, ds[0, :n[0]])]

    def search(self, query, size=0, epsilon=-FLT_MAX, edge_size=INT_MIN, expected_accuracy=-FLT_MAX,
               with_distance=True):
        """ngtpy.cpp:141-214: tree-seeded search unless tree_disabled.  A
        positive expected_accuracy replaces epsilon with the one the prf's
        AccuracyTable maps it to (sc.setExpectedAccuracy, then
        GraphIndex::search's getEpsilonFromExpectedAccuracy, Index.h:1156-1158)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(1, -1)
        k = size if size > 0 else self.num_of_search_objects
        eps = self.epsilon if epsilon <= -1.0 else epsilon
        if expected_accuracy > 0.0:
            eps = self.epsilon_for(expected_accuracy)
        es = self.edge_size if edge_size < -2 else edge_size
        ids, ds, n = self._ix.batch_search(q, k, eps, self.radius, es, graph_only=not self.tree)
        self.distance_computations += int(self._ix.last_search_counters()[0])
        return self._results(ids, ds, n, with_distance)

    def epsilon_for(self, expected_accuracy):
        """The epsilon a search with this expected accuracy uses (the pybind
        argument is a float, widened to double for getEpsilon)."""
        if self._table is None:
            self._table = self._handle_table()
        return epsilon_from_expected_accuracy(self._table, float(np.float32(expected_accuracy)))

    def _handle_table(self):
        """The AccuracyTable of the open handle's property: the prf's as it was
        opened, or the one generate_accuracy_table stored since."""
        import ctypes
        ix = self._ix
        L = ix._L
        ix._check(L.ngt_get_property(ix.index, ix.prop, ix.err), ix.err)
        n = L.ngt_get_property_value(ix.prop, b"AccuracyTable", None, 0, ix.err)
        buf = ctypes.create_string_buffer(max(n, 0) + 1)
        L.ngt_get_property_value(ix.prop, b"AccuracyTable", buf, len(buf), ix.err)
        return parse_accuracy_table(buf.value.decode())

    def linear_search(self, query, size=0, with_distance=True):
        """ngtpy.cpp:216-268: exact k-NN by full scan within the index's search
        radius (sc.setRadius(defaultRadius)).  The reference adds
        sc.distanceComputationCount, which ObjectSpaceRepository::linearSearch
        (ObjectSpaceRepository.h:466-502) never increments: the count is unchanged."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(1, -1)
        k = size if size > 0 else self.num_of_search_objects
        ids, ds, n = self._ix.batch_linear_search(q, k, radius=self.radius)
        return self._results(ids, ds, n, with_distance)

    def get_num_of_distance_computations(self):
        return self.distance_computations

    def set(self, num_of_search_objects=0, search_radius=-FLT_MAX, epsilon=-FLT_MAX, edge_size=INT_MIN,
            expected_accuracy=-FLT_MAX):
        """ngtpy.cpp:322-333: a non-positive / out-of-range value keeps the
        default.  expected_accuracy is kept as defaultExpectedAccuracy, which
        the reference's search never reads (it takes only its own argument,
        ngtpy.cpp:168-172): a set() value changes no search there or here."""
        if num_of_search_objects > 0:
            self.num_of_search_objects = num_of_search_objects
        if epsilon > -1.0:
            self.epsilon = epsilon
        if search_radius >= 0.0:
            self.radius = search_radius
        if edge_size >= -2:
            self.edge_size = edge_size
        if expected_accuracy > 0.0:
            self.expected_accuracy = expected_accuracy

    def insert(self, object, debug=False):
        """ngtpy.cpp:119-139: append one object (no graph update until build_index)."""
        return self._id_out(np.array([self._ix.insert_object(object)]))[0].item()

    def batch_insert(self, objects, num_threads=8, debug=False):
        """ngtpy.cpp:98-117: append all rows, then build the index on the GPU."""
        objs = np.asarray(objects, dtype=np.float32)
        if objs.ndim != 2 or objs.shape[1] != self._ix.dim:
            raise NativeError("ngtpy::insert: Error! dimensions are inconsitency. %d:%d"
                              % (self._ix.dim, objs.shape[-1]))
        self._ix.insert(objs, num_threads)
        self.distance_computations = 0

    def build_index(self, num_threads=8, target_size_of_graph=0):
        self._ix.build_index(num_threads)

    def get_object(self, object_id):
        return [float(x) for x in self._ix.get_object(self._id_in(object_id))]

    def remove(self, object_id):
        """ngtpy.cpp remove -> GraphAndTreeIndex::remove: the object leaves the
        repository, the tree and the graph, and its neighbours are relinked, on
        the GPU.  The id follows zero_based_numbering; a missing id raises
        NativeError with the C API's message."""
        self._ix.remove(self._id_in(object_id))

    def refine_anng(self, epsilon=0.1, expected_accuracy=0.0, num_of_edges=0, num_of_explored_edges=INT_MIN,
                    batch_size=10000):
        """ngtpy.cpp:548-553 -> GraphReconstructor::refineANNG: one search per
        stored object on the GPU in batches, the results merged into the graph
        in place (outgoing edges; incoming edges when num_of_edges is 0; every
        list cut to num_of_edges when it is positive).  ``save`` then writes
        what ``ngt refine-anng`` writes.  On an error the graph is left as it
        was; a batch_size of 0 is an error."""
        L = self._ix._L
        self._ix._check(L.ngt_refine_anng(self._ix.index, float(epsilon), float(expected_accuracy),
                                          int(num_of_edges), int(num_of_explored_edges), int(batch_size),
                                          self._ix.err), self._ix.err)
        self._table = None

    def generate_accuracy_table(self, num_of_results=20, num_of_queries=100):
        """Optimizer::generateAccuracyTable (Optimizer.h:1495-1573) on the GPU
        for the open index: what ``ngt optimize-search-parameters -m a``
        computes.  The table goes into the index's property, so searches with
        ``expected_accuracy`` and ``refine_anng(expected_accuracy=...)`` use it
        at once and ``save`` writes it.  Returns the table as
        ``[(epsilon, accuracy), ...]``."""
        ix = self._ix
        ix._check(ix._L.ngt_generate_accuracy_table(ix.index, int(num_of_results), int(num_of_queries), ix.err),
                  ix.err)
        self._table = self._handle_table()
        return [(float(e), a) for e, a in self._table]

    def save(self):
        if self.read_only:
            raise NativeError("ngtpy::save: the index is read only")
        self._ix.save()

    def close(self):
        self._ix.close()


class Optimizer(object):
    """ngtpy.Optimizer (ngtpy.cpp:566-600): NGT::GraphOptimizer with the
    reference's argument names and defaults (negative values keep the
    optimizer's own defaults, GraphOptimizer.h:63-78, :545-591).  ``execute``
    runs edge and path adjustment on the MI355X; the three tuning steps have to
    be switched off with ``set_processing_modes`` first.
    ``optimize_search_parameters`` generates the accuracy table; search-parameter
    and prefetch optimisation have to be off for it.
    ``optimize_number_of_edges_for_anng`` is ``ngt optimize-#-of-edges``."""

    def __init__(self, num_of_outgoings=-1, num_of_incomings=-1, num_of_queries=-1, num_of_objects=-1,
                 low_accuracy_from=-1.0, low_accuracy_to=-1.0, high_accuracy_from=-1.0, high_accuracy_to=-1.0,
                 gt_epsilon=-DBL_MAX, margin=-1.0, log_disabled=False):
        from . import lib
        self._L = lib()
        self._err = self._L.ngt_create_error_object()
        self._opt = self._L.ngt_create_optimizer(bool(log_disabled), self._err)
        if not self._opt:
            raise NativeError(base._err_string(self._L, self._err))
        self._min_edges = 0
        self.set(num_of_outgoings, num_of_incomings, num_of_queries, num_of_objects, low_accuracy_from,
                 low_accuracy_to, high_accuracy_from, high_accuracy_to, gt_epsilon, margin)

    def __del__(self):
        if getattr(self, "_opt", None):
            self._L.ngt_destroy_optimizer(self._opt)
            self._opt = None
        if getattr(self, "_err", None):
            self._L.ngt_destroy_error_object(self._err)
            self._err = None

    def _check(self, ok):
        if not ok:
            raise NativeError(base._err_string(self._L, self._err))

    def set(self, num_of_outgoings=-1, num_of_incomings=-1, num_of_queries=-1, num_of_objects=-1,
            low_accuracy_from=-1.0, low_accuracy_to=-1.0, high_accuracy_from=-1.0, high_accuracy_to=-1.0,
            gt_epsilon=-DBL_MAX, margin=-1.0):
        """GraphOptimizer::set(outgoing, incoming, nofqs, nofrs, ...) (GraphOptimizer.h:545-552)."""
        L = self._L
        self._check(L.ngt_optimizer_set_minimum(self._opt, int(num_of_outgoings), int(num_of_incomings),
                                                int(num_of_queries), int(num_of_objects), self._err))
        self._check(L.ngt_optimizer_set_extension(self._opt, low_accuracy_from, low_accuracy_to, high_accuracy_from,
                                                  high_accuracy_to, gt_epsilon, margin, self._err))

    def set_processing_modes(self, shortcut_reduction=True, search_parameter_optimization=True,
                             prefetch_parameter_optimization=True, accuracy_table_generation=True):
        L = self._L
        self._check(L.ngt_optimizer_set_shortcut_reduction(self._opt, bool(shortcut_reduction), self._min_edges,
                                                           self._err))
        self._check(L.ngt_optimizer_set_processing_modes(self._opt, bool(search_parameter_optimization),
                                                         bool(prefetch_parameter_optimization),
                                                         bool(accuracy_table_generation), self._err))

    def get(self):
        """The optimizer's parameters by name (not in the reference)."""
        import ctypes
        v = (ctypes.c_double * 16)()
        self._check(self._L.ngt_optimizer_get(self._opt, v, self._err))
        names = ("num_of_outgoings", "num_of_incomings", "min_num_of_edges", "num_of_queries", "num_of_objects",
                 "low_accuracy_from", "low_accuracy_to", "high_accuracy_from", "high_accuracy_to", "gt_epsilon",
                 "margin", "log_disabled", "shortcut_reduction", "search_parameter_optimization",
                 "prefetch_parameter_optimization", "accuracy_table_generation")
        return dict(zip(names, list(v)))

    def execute(self, in_path, out_path):
        self._check(self._L.ngt_optimizer_execute(self._opt, os.fsencode(in_path), os.fsencode(out_path), self._err))

    def optimize_search_parameters(self, index_path):
        """GraphOptimizer::optimizeSearchParameters (GraphOptimizer.h:302-384) with
        accuracy-table generation alone: rewrites ``index_path``/prf with the
        table ``ngt optimize-search-parameters -m a`` writes."""
        self._check(self._L.ngt_optimizer_optimize_search_parameters(self._opt, os.fsencode(index_path), self._err))

    def optimize_number_of_edges_for_anng(self, path, num_of_queries=-1, num_of_results=-1, num_of_threads=-1,
                                          target_accuracy=-1.0, target_num_of_objects=-1, num_of_sample_objects=-1,
                                          max_num_of_edges=-1):
        """GraphOptimizer::optimizeNumberOfEdgesForANNG(path, parameter)
        (ngtpy.cpp:353-378; negative values, and zeros where the reference says
        so, keep the defaults): what ``ngt optimize-#-of-edges`` runs.  Rewrites
        ``path``/prf with the new EdgeSizeForCreation and returns it."""
        import ctypes
        p = self._L.ngt_get_anng_edge_optimization_parameter()
        if num_of_queries > 0:
            p.no_of_queries = int(num_of_queries)
        if num_of_results > 0:
            p.no_of_results = int(num_of_results)
        if num_of_threads >= 0:
            p.no_of_threads = int(num_of_threads)
        if target_accuracy > 0.0:
            p.target_accuracy = target_accuracy
        if target_num_of_objects >= 0:
            p.target_no_of_objects = int(target_num_of_objects)
        if num_of_sample_objects > 0:
            p.no_of_sample_objects = int(num_of_sample_objects)
        if max_num_of_edges > 0:
            p.max_of_no_of_edges = int(max_num_of_edges)
        p.log = not bool(self.get()["log_disabled"])
        edge = ctypes.c_size_t(0)
        acc = ctypes.c_float(0.0)
        self._check(self._L.ngt_optimize_number_of_edges_with_result(os.fsencode(path), p, ctypes.byref(edge),
                                                                      ctypes.byref(acc), self._err))
        return int(edge.value)
