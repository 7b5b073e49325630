"""The reference of the label-propagation tests (bspgemm_label_propagation): a vectorised numpy model of synchronous CDLP on
the symmetrized diagonal-free graph that also counts the iterations and the changed vertices as the library defines them, a
naive implementation with a Counter per vertex to check the model with, the degree classes of csrc/lp.hip, and the graphs
the tests use.  Nothing here touches the GPU.
"""
from collections import Counter

import numpy as np

import color_ref
import kcore_ref
from kcore_ref import simple

LANE_CAP = 8             # csrc/lp.hip kLpLaneCap: the longest row one lane takes
WAVE_CAP = 256           # csrc/lp.hip kLpWaveCap: the longest row one wave sorts
GROUP_CAP = 4096         # csrc/lp.hip kLpGroupCap: the longest row one workgroup sorts; longer rows are hubs
CAPS = (LANE_CAP, WAVE_CAP, GROUP_CAP)


def _first_labels(n, initial):
    if initial is None:
        return np.arange(n, dtype=np.int64)
    L = np.asarray(initial, np.int64).copy()
    assert L.shape == (n,) and ((L >= 0) & (L < n)).all()
    return L


def step(srp, sci, n, L):
    """one synchronous iteration on a simple graph: every vertex with neighbours takes the smallest of the labels that
    occur most often among its neighbours' labels in L; the others keep theirs"""
    if sci.size == 0:
        return L.copy()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(srp))
    pair, count = np.unique(rows * n + L[sci], return_counts=True)      # (vertex, label) and how often
    p_row, p_label = pair // n, pair % n
    o = np.lexsort((p_label, -count, p_row))                           # per vertex: the largest count, then the smallest label
    head = np.flatnonzero(np.concatenate([[True], p_row[o][1:] != p_row[o][:-1]]))
    out = L.copy()
    out[p_row[o][head]] = p_label[o][head]
    return out


def trajectory(rp, ci, n, max_iter, initial=None):
    """(labels of every iteration run: [L_0, L_1, ...], changed per iteration, converged): stops after max_iter iterations
    or after the first one that changes nothing, which is listed; a graph without edges runs none and has converged"""
    srp, sci = simple(rp, ci, n)
    Ls, changed = [_first_labels(n, initial)], []
    if sci.size == 0:
        return Ls, changed, True
    while len(changed) < max_iter:
        Ls.append(step(srp, sci, n, Ls[-1]))
        changed.append(int((Ls[-1] != Ls[-2]).sum()))
        if changed[-1] == 0:
            return Ls, changed, True
    return Ls, changed, False


def label_propagation(rp, ci, n, max_iter, initial=None):
    """(labels int32[n], iterations, converged, changed, communities) as bspgemm_label_propagation defines them for the
    graph of A's entries: iterations counts the one that changed nothing, changed is the last iteration's (0 without one)"""
    Ls, changed, converged = trajectory(rp, ci, n, max_iter, initial)
    L = Ls[-1].astype(np.int32)
    return L, len(changed), int(converged), changed[-1] if changed else 0, int(np.unique(L).size)


def naive(rp, ci, n, max_iter, initial=None):
    """the same five, from the definition: a set of neighbours and a Counter per vertex"""
    nb = [set() for _ in range(n)]
    rp, ci = np.asarray(rp).tolist(), np.asarray(ci).tolist()
    for u in range(n):
        for w in ci[rp[u]:rp[u + 1]]:
            if w != u:
                nb[u].add(w)
                nb[w].add(u)
    L = _first_labels(n, initial).tolist()
    if not any(nb):
        return np.array(L, np.int32), 0, 1, 0, len(set(L))
    iterations = changed = converged = 0
    while iterations < max_iter:
        new = list(L)
        for v in range(n):
            if nb[v]:
                c = Counter(L[w] for w in nb[v])
                top = max(c.values())
                new[v] = min(l for l, k in c.items() if k == top)
        iterations += 1
        changed = sum(a != b for a, b in zip(new, L))
        L = new
        if changed == 0:
            converged = 1
            break
    return np.array(L, np.int32), iterations, converged, changed, len(set(L))


def mode(labels):
    """the smallest of the most frequent values"""
    c = Counter(int(x) for x in labels)
    top = max(c.values())
    return min(l for l, k in c.items() if k == top)


# ---------------------------------------------------------------- the degree classes of csrc/lp.hip ------------------
def class_of(d):
    """0 lane, 1 wave, 2 workgroup, 3 hub, for a degree d >= 1"""
    return 0 if d <= LANE_CAP else 1 if d <= WAVE_CAP else 2 if d <= GROUP_CAP else 3


def class_vertices(rp, ci, n, min_class=0):
    """bspgemm_lp_info.class_vertices: the vertices of degree >= 1 per class max(own, min_class)"""
    deg = np.diff(simple(rp, ci, n)[0])
    own = np.searchsorted(np.array(CAPS), deg[deg > 0], side="left")    # d <= cap: that class
    return np.bincount(np.maximum(own, min_class), minlength=4).tolist()


def hub_start(labels, d):
    """where the probe sequence of each label starts in a hub's table of 2 d slots: (mix32(label) * size) >> 32"""
    return ((color_ref.mix32(np.asarray(labels, np.uint32)).astype(np.uint64) * np.uint64(2 * d)) >> np.uint64(32)).astype(np.int64)


# ---------------------------------------------------------------- graphs ---------------------------------------------
GRAPHS = kcore_ref.GRAPHS
# the degrees at which the mode is tested: the wave's 64-entry step and one below, at and above every class cap (the
# smallest hub is GROUP_CAP + 1)
DEGREES = sorted({1, 2, 63, 64, 65} | {c + k for c in CAPS for k in (-1, 0, 1)})
MULTISETS = ("distinct", "equal", "halves", "ahead_by_one", "pairs_and_a_triple", "zero_wins", "zero_loses", "colliding")


def multiset(kind, d, n):
    """d labels in [0, n) (n >= 2 d + 8) whose mode tests one thing; the order is shuffled by the caller"""
    filler = np.arange(n - 1, n - 1 - d, -1)                 # distinct, large, each once: never the mode of a set with a pair
    if kind == "distinct":                                   # the sort or the table holds d keys; consecutive ids
        return np.arange(5, 5 + d)
    if kind == "equal":                                      # one counter takes d additions
        return np.full(d, 7)
    if kind == "halves":                                     # a tie: the smaller label wins
        return np.concatenate([np.full(d // 2, 9), np.full(d // 2, 3), filler[:d % 2]])
    if kind == "ahead_by_one":                               # the count beats the label
        k = (d - 1) // 2
        return np.concatenate([np.full(k + 1, 11), np.full(k, 2), filler[:d - 2 * k - 1]])
    if kind == "pairs_and_a_triple":                         # many labels twice, the largest id three times
        m = max((d - 3) // 2, 0)
        body = np.concatenate([np.repeat(np.arange(20, 20 + m), 2), np.full(min(3, d), n - 1)])
        return np.concatenate([body, filler[1:1 + d - body.size]])
    if kind == "zero_wins":                                  # label 0 must not be taken for an empty slot
        return np.concatenate([np.zeros(d // 2 + 1, np.int64), filler[:d - d // 2 - 1]])
    if kind == "zero_loses":                                 # (from d = 3 on; a shorter row has no room for a winner)
        return np.concatenate([np.zeros(1, np.int64), np.full(d - 1, 6)]) if d > 2 else np.concatenate([[0], filler[:d - 1]])
    assert kind == "colliding", kind
    # labels whose probe sequences start in ONE slot of a hub's table of 2 d slots, with equal low bits where that can be
    # had: the second of them twice, so that it wins from behind a collision
    for stride in (64, 1):
        cand = np.arange(0, n, stride)
        start = hub_start(cand, d)
        slot = np.bincount(start).argmax()
        same = cand[start == slot][:max(min(d // 2, 24), 1)]
        if same.size >= min(d // 2, 4):
            break
    body = np.concatenate([same, same[1:2]])[:d]
    return np.concatenate([body, filler[:d - body.size]])


def star_union(n_total=None, seed=5460, high=False):
    """(rp, ci, n, initial, hubs, expected): a disjoint union of stars, one per (multiset, degree); star i has a hub whose d
    leaves carry the multiset as their first labels, so that after ONE iteration the hub's label is the multiset's mode:
    expected[i] for vertex hubs[i].  Only the hub's row is stored.  n_total: pad with isolated vertices, which carry
    random first labels; high: every first label l of a star vertex becomes n - 1 - l (the large ids)."""
    rng = np.random.default_rng(seed)
    used = sum(d + 1 for d in DEGREES) * len(MULTISETS)
    n = n_total or used
    assert n >= used
    rows, cols, hubs, expected = [], [], [], []
    initial = rng.integers(0, n, size=n)
    at = 0
    for kind in MULTISETS:
        for d in DEGREES:
            labels = rng.permutation(multiset(kind, d, used))
            assert labels.size == d and labels.min() >= 0 and labels.max() < used, (kind, d)
            if high:
                labels = n - 1 - labels
            leaves = at + 1 + np.arange(d)
            initial[at], initial[leaves] = at, labels
            rows.append(np.full(d, at))
            cols.append(rng.permutation(leaves))
            hubs.append(at)
            expected.append(mode(labels))
            at += d + 1
    import cc_ref
    rp, ci, _ = cc_ref.csr(np.concatenate(rows), np.concatenate(cols), n)
    return rp, ci, n, initial.astype(np.int32), np.array(hubs), np.array(expected, np.int32)
