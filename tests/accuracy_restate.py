"""Plain-Python restatement of the reference's accuracy-table generation
(Optimizer::generateAccuracyTable, lib/NGT/Optimizer.h:1495-1573, with
extractQueries :1139-1199, generatePseudoGroundTruth :1425-1493, the evaluation
of Optimizer::search :108-128 / sumup :345-507 and
Index::AccuracyTable::getString) -- the second checker of the device
implementation (ngt_amd/csrc/accuracy_table.cpp).

float32 where the reference has float, Python floats where it has double.  The
searches come from a callback ``search(queries, size, epsilon, edge_size) ->
(ids [nq, size], dists [nq, size] float32, n [nq], counts [nq])``; `oracle_search`
builds one over the CPU oracle (tree seeds plus graph search).  The one
deliberate difference from the reference is the guard of the maxEpsilon loop:
the reference stops when the last query's wall time exceeds 40 x its time at
epsilon 0 (:1461), this stops when that query's distance computations exceed
40 x their count at epsilon 0.  Test infrastructure only.
"""
import numpy as np

F32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
SWEEP_SIZE = 20  # Command::SearchParameters() (Command.h:39-52)
WORK_GUARD = 40.0


def fmt(x):
    """`stream << x` of a float or double with the stream's defaults."""
    return "%g" % float(x)


def extract_queries(rows, valid, dim, nqueries):
    """extractQueries(nqueries, queries): the mean of a stored object and the
    next stored one, at every (repository size / nqueries)-th id."""
    osize = len(valid)
    if nqueries == 0:
        raise ValueError("the number of queries is 0")
    interval = osize // nqueries
    u8 = rows.dtype == np.uint8
    out = []
    id1, count = 1, 0
    while id1 < osize and count < nqueries:
        oft = 0
        while not valid[id1 + oft]:
            oft += 1
            if id1 + oft >= osize:
                raise ValueError("Too many empty entries to extract. Object repository size=%d %d:%d"
                                 % (osize, id1, oft))
        id2 = id1 + oft + 1
        while id2 >= osize or not valid[id2]:
            id2 += 1
            if id2 >= osize:
                raise ValueError("Too many empty entries to extract.")
        a, b = rows[id1 + oft, :dim], rows[id2, :dim]
        if u8:
            out.append(((a.astype(np.int32) + b.astype(np.int32)) // 2).astype(F32))
        else:
            out.append(((a + b) / F32(2.0)).astype(F32))
        id1 += interval
        count += 1
    return np.array(out, F32)


def query_text(queries, u8):
    """outputObject (:1004-1031): one line per query."""
    return "".join("\t".join(("%d" % int(v)) if u8 else fmt(v) for v in q) + "\n" for q in queries)


def parse_queries(text):
    """Index::allocateObject(line, " \\t"): strtod per token, then the object type."""
    return np.array([[F32(float(t)) for t in line.split()] for line in text.splitlines()], F32)


def max_epsilon(search, queries, nresults, guard=WORK_GUARD):
    """The first loop of generatePseudoGroundTruth; returns (maxEpsilon, steps)
    with steps [(e, identical, last count)]."""
    nq = len(queries)
    last = [F32(0.0)] * nq
    identity_count = 0
    count0 = 0
    step = 0.02
    e = F32(0.0)
    steps = []
    maxeps = F32(0.0)
    while float(e) < 10.0:
        ids, ds, n, cnt = search(queries, nresults, e, -1)
        identity = True
        for i in range(nq):
            if n[i] == 0:
                raise ValueError("a search returned no result")
            d = ds[i, n[i] - 1]
            if d != last[i]:
                identity = False
            last[i] = d
        work = int(cnt[nq - 1])
        if float(e) == 0.0:
            count0 = work
        steps.append((float(e), identity, work))
        if guard is not None and float(work) > float(count0) * guard:
            maxeps = e
            break
        if identity:
            identity_count += 1
            step *= 1.2
            if identity_count > 5:
                maxeps = e
                break
        else:
            identity_count = 0
        e = F32(float(e) + step)
    return maxeps, steps


def ground_truth(search, rounded, nresults, maxeps):
    """createGroundTruth: per query (ids, printed distances as doubles)."""
    ids, ds, n, _ = search(rounded, nresults, maxeps, 0)
    return [([int(v) for v in ids[i, :n[i]]], [float(fmt(v)) for v in ds[i, :n[i]]]) for i in range(len(rounded))]


def mean_accuracy(gt, ids, ds, n):
    """evaluate / loadGroundTruth / sumup over one epsilon; MeasuredValue::meanAccuracy is a float."""
    size = int(max(n))  # checkAndGetSize: the first result size, raised by a larger one
    total = 0.0
    for q, (gids, gds) in enumerate(gt):
        if len(gids) < size:
            raise ValueError("Error: gt data is less than result size! %d:%d" % (len(gids), size))
        gset = set(gids[:size])
        farthest = gds[size - 1] if size else 0.0
        relevant = 0
        for j in range(int(n[q])):
            if int(ids[q, j]) in gset:
                relevant += 1
            elif farthest > 0.0 and float(fmt(ds[q, j])) <= farthest:
                relevant += 1
        total += relevant / float(size)
    return float(F32(total / float(len(gt))))


def sweep(search, rounded, gt, maxeps, log=None):
    """The do-while of generateAccuracyTable (:1514-1553); returns {float32 epsilon: accuracy}."""
    table = {}
    interval = F32(0.05)
    prev = F32(0.0)
    epsilon = F32(-0.6)
    while True:
        key = float(epsilon)
        if key not in table:
            ids, ds, n, _ = search(rounded, SWEEP_SIZE, epsilon, -1)
            accuracy = mean_accuracy(gt, ids, ds, n)
            table[key] = accuracy
            if log is not None:
                log.append((key, accuracy))
        else:
            accuracy = table[key]
        if float(prev) != 0.0:
            if accuracy - float(prev) < 0.02:
                interval = F32(float(interval) * 2.0)
            elif accuracy - float(prev) > 0.05 and float(interval) > 0.0001:
                epsilon = F32(epsilon - interval)
                interval = F32(float(interval) / 2.0)
                accuracy = float(prev)
        prev = F32(accuracy)
        epsilon = F32(epsilon + interval)
        if accuracy > 0.98 and float(epsilon) > float(maxeps):
            break
        if not accuracy < 1.0:
            break
    return table


def filter_table(table):
    """:1556-1570 over the std::map in key order."""
    out = []
    prev = (F32(0.0), -1.0)
    for k in sorted(table):
        if abs(float(F32(F32(k) - prev[0]))) <= FLT_EPSILON:
            continue
        if table[k] - prev[1] < DBL_EPSILON:
            continue
        out.append((F32(k), table[k]))
        if table[k] >= 1.0:
            break
        prev = (F32(k), table[k])
    return out


def table_string(pairs):
    """Index::AccuracyTable::getString."""
    return ",".join("%s:%s" % (fmt(e), fmt(a)) for e, a in pairs)


def refusal(prop, nresults):
    """The two refusals that need no search."""
    es = int(prop["EdgeSizeForSearch"])
    if es != 0 and es != -2:
        return ("Optimizer::generateAccuracyTable: edgeSizeForSearch is invalid to call generateAccuracyTable, "
                "because accuracy 1.0 cannot be achieved with the setting. edgeSizeForSearch=%d." % es)
    if nresults < SWEEP_SIZE:
        return "Error: gt data is less than result size! %d:%d" % (nresults, SWEEP_SIZE)
    return None


def generate(search, rows, valid, prop, nresults=20, nqueries=100, guard=WORK_GUARD, trace=None):
    """The whole procedure; returns (pairs, table string, maxEpsilon)."""
    why = refusal(prop, nresults)
    if why:
        raise ValueError(why)
    dim = int(prop["Dimension"])
    u8 = rows.dtype == np.uint8
    if trace is not None:
        inner = search

        def search(q, size, eps, es):  # noqa: F811
            r = inner(q, size, eps, es)
            trace.append((q, size, F32(eps), es, r))
            return r
    queries = extract_queries(rows, valid, dim, nqueries)
    maxeps, _ = max_epsilon(search, queries, nresults, guard)
    rounded = parse_queries(query_text(queries, u8))
    gt = ground_truth(search, rounded, nresults, maxeps)
    pairs = filter_table(sweep(search, rounded, gt, maxeps))
    return pairs, table_string(pairs), maxeps


def oracle_search(rows, tree, prop, offsets, edges, threads=8):
    """The search callback over the CPU oracle for an index's arrays."""
    import oracle_py as O
    import refine_restate as RR
    metric = {"L2": "l2", "L1": "l1", "Cosine": "cosine", "Angle": "angle"}[prop["DistanceType"]]
    seed_size = int(prop["SeedSize"])
    dim = int(prop["Dimension"])
    seeds_of = {}

    def search(queries, size, epsilon, edge_size):
        q = np.zeros((len(queries), rows.shape[1]), rows.dtype)
        q[:, :dim] = queries.astype(rows.dtype)
        key = (q.tobytes(), size)
        if key not in seeds_of:
            seeds_of[key] = [O.tree_seeds(metric, tree, v, size, seed_size, dtype=rows.dtype)[0] for v in q]
        es = RR.edge_size(prop, None if edge_size == -1 else edge_size, epsilon)
        ids, ds, n, cnt = O.search_batch(metric, rows, offsets, edges, q, seeds_of[key], size, F32(epsilon),
                                         edge_size=es, threads=threads)
        return ids, ds, n, cnt[:, 0]
    return search
